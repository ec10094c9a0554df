// ThreadLocalize.h -- per-robot localisation worker; public surface of the reference's
// ThreadLocalize (src/ThreadLocalize.h:73-104): same constructor, same laserCallBack entry point, same
// parameters, topic and message content.  The arithmetic of eventLoop (ray cast, ICP) runs on the GPU
// through obvious::TsdGrid::localize; scan ingest, gates and pose bookkeeping stay on the host.
// registration_mode 0 (ICP only), 1 (RandomNormalMatching pre-registration + ICP), 2 (PDFMatching pre-registration + ICP) and
// 3 (TSD_PDF pre-registration + ICP, what config/single-laser.yaml ships) are implemented; unknown modes fall back to 0 with a
// warning, as in the reference (ThreadLocalize.cpp:188-190).
#pragma once
#include <deque>
#include <memory>
#include <string>

#include "ThreadSLAM.h"
#include "ahead_ledger.hpp"
#include "ros_shim.h"

namespace ohm_tsd_slam
{

class ThreadMapping;

namespace
{
  const double TRNS_MIN = 0.05;   // minimal pose change that triggers a push (ThreadLocalize.h:63-64)
  const double ROT_MIN  = 0.03;
}

class ThreadLocalize: public ThreadSLAM
{
public:
  ThreadLocalize(obvious::TsdGrid* grid, ThreadMapping* mapper, const std::shared_ptr<rclcpp::Node>& node,
                 const std::string& robot_name, const double xOffset, const double yOffset);
  virtual ~ThreadLocalize();

  /** laser subscription callback (ThreadLocalize.cpp:248-276): first scan initialises synchronously,
   *  later scans are queued for the localisation thread (newest wins) */
  void laserCallBack(const std::shared_ptr<sensor_msgs::msg::LaserScan> scan);

  // ---- additions for tests / benchmarks (not in the reference) ----
  /** run the event-loop body on the caller's thread and push in stream order instead of handing
   *  over to the two worker threads: the strict R -> I -> P order the parity tests need */
  void setSynchronous(bool on) { _synchronous = on; }
  /** fused scan path (default): sensor state on the device, gates + push decided there in stream
   *  order (tsd_scan).  Off: tsd_localize, host gates, ThreadMapping::queuePush as in the reference. */
  void setFused(bool on) { _fused = on; }
  /** this grid is shared with other localisers (SlamNode's multi-robot mode): use the split scan of the fused path
   *  (tsd_scan_begin / _wait / _finish) so that the robots' registrations overlap on the device */
  void setConcurrent(bool on) { _concurrent = on; }
  /** the scan that will come NEXT is known already (queued behind the one being processed; a replayed log): the fused path
   *  ingests it and stages it on the device while the current registration runs (tsd_scan_stage).  The following
   *  laserCallBack with the same stamp then starts from the staged data. */
  void announceNext(const std::shared_ptr<sensor_msgs::msg::LaserScan> scan);
  /** start or re-seat the localiser at a known sensor pose (3x3 row-major), e.g. the result of a relocalisation in a stored map.
   *  Fresh localiser: what init does with `scan` as the first scan, but at pose33 instead of the configured start pose, WITHOUT
   *  freeFootprint and WITHOUT the initial push; the mapper is marked initialised, so the map in the grid is not overwritten.
   *  Running localiser: the sensor pose is re-seated (host sensor and its device twin, _lastPose forgotten) between two scans;
   *  `scan` is not used, and lastReport() reads like after a start: the new pose, T = identity, no verdict of the scan before.
   *  False when scans are queued or being processed, or a push of the mapper is still queued.  Nothing is registered or pushed by the call. */
  bool startAt(const double pose33[9], const sensor_msgs::msg::LaserScan& scan);
  struct ScanReport {
    double pose[9]; double T[9]; double rms; int pairs; int iterations; int icpState;
    int validModel; int validScene; bool regError; bool pushed; bool noModel; bool initialised;
    long long stampNs;
  };
  ScanReport lastReport();
  uint64_t processedScans();
  /** the last pre-registration of the reference's call structure (registration_modes 1 and 2, and mode 3 where it runs unfused;
   *  mode 1 reports bestRatio as the probability); false if there was none */
  bool lastPreregistration(tsd_tsdpdf_result* out);
  /** nothing queued and nothing being processed */
  bool idle();
  std::shared_ptr<rclcpp::Publisher<geometry_msgs::msg::PoseStamped>> posePublisher() { return _posePub; }
  /** the tf buffer sendTransform looks laser -> base_footprint and base_footprint -> odom up in (a TransformListener fills it under
   *  ROS; tests and ROS-free hosts feed it with Buffer::setTransform) and the broadcaster map -> odom leaves through */
  tf2_ros::Buffer* tfBuffer() { return _tf_buffer.get(); }
  tf2_ros::TransformBroadcaster* tfBroadcaster() { return _tfBroadcaster.get(); }
  obvious::SensorPolar2D* sensor() { return _sensor; }

  // every parameter the reference declares in the constructor (ThreadLocalize.cpp:86-129) / in init (:424-432)
  static void declareParameters(const std::shared_ptr<rclcpp::Node>& node, const std::string& robotName);
  static void declareInitParameters(const std::shared_ptr<rclcpp::Node>& node, const std::string& nameSpace);

  // gates (static: also unit-tested against the oracle)
  static double calcAngle(obvious::Matrix* T);                                               // :715-726
  static bool isRegistrationError(obvious::Matrix* T, const double trnsMax, const double rotMax);   // :593-600
  static bool isPoseChangeSignificant(obvious::Matrix* lastPose, obvious::Matrix* curPose);   // :728-736

protected:
  virtual void eventLoop(void);

private:
  void init(const sensor_msgs::msg::LaserScan& scan, const double* pose33 = nullptr);
  void processScan(const std::vector<float>& rangesIn, const builtin_interfaces::msg::Time& stamp);
  void processScanFused(ScanReport& rep);
  void processScanPreRegistered(ScanReport& rep);
  bool hostPreRegisters() const;
  bool scanHasModel(int rc, ScanReport& rep, int validModel, int validScene, bool noModel);
  void finishScan(ScanReport& rep, const tsd_icp_result& res, const tsd_scan_result* device = nullptr);
  int armPreregistration(bool reuseDraws);
  void stageNextScan(bool submitted);
  void publish(const ScanReport& rep);
  void deviceError(int rc, const ScanReport& rep);
  void clampRanges(sensor_msgs::msg::LaserScan& scan) const;
  static long long stampNs(const builtin_interfaces::msg::Time& stamp);
  void sendTransform(obvious::Matrix* T);
  void sendNanTransform();

  std::shared_ptr<rclcpp::Node> _node;
  ThreadMapping& _mapper;
  obvious::SensorPolar2D* _sensor;
  bool _initialized;
  bool _synchronous;
  bool _fused;
  bool _concurrent;
  const double _gridWidth, _gridHeight, _gridOffSetX, _gridOffSetY, _xOffset, _yOffset;
  std::string _robotName, _nameSpace;
  std::string _tfMapFrameId, _tfOdomFrameId, _tfLaserFrameId, _tfFootprintFrameId;
  double _trnsMax, _rotMax, _lasMinRange;
  int _regMode;
  double _ranPhiMax;
  // _RandomNormalMatcher / _PDFMatcher / _TSD_PDFMatcher (ThreadLocalize.h): the one the registration mode asks for, or none (ICP)
  std::unique_ptr<obvious::RandomMatching> _matcher;
  obvious::TSD_PDFMatching* _tsdPdf = nullptr;                // _matcher where it is mode 3's (the fused arming needs its params())
  tsd_tsdpdf_result _preResult;                               // (guarded by _reportMutex)
  bool _havePreResult = false;
  std::vector<double> _modelCoords, _modelNormals, _scene;     // beam-indexed buffers of the event loop (:342-350)
  std::vector<uint8_t> _maskM, _maskS;
  bool _reverseScan;
  tsd_icp_params _icpParams;
  obvious::Matrix* _lastPose;
  bool _haveLastPose;
  builtin_interfaces::msg::Time _stampLaser, _stampLaserOld;

  std::shared_ptr<sensor_msgs::msg::LaserScan> _ahead;      // announced next scan (clamped like laserCallBack does; guarded by _dataMutex)
  AheadLedger _lookAhead;           // what was staged, armed and drawn ahead of the next scan (ahead_ledger.hpp)
  std::vector<int> _dSub, _dCtrl, _dTrials;     // registration_mode 3, fused: the three rand() streams the ledger speaks of
  bool _asyncMapping = false;       // "async_mapping" (addition): the fused scan's push beside the next registration (tsd_sensor_set_async_mapping)
  std::deque<std::shared_ptr<sensor_msgs::msg::LaserScan>> _laserData;
  std::mutex _dataMutex;
  bool _busy;

  std::shared_ptr<rclcpp::Publisher<geometry_msgs::msg::PoseStamped>> _posePub;
  std::unique_ptr<tf2_ros::TransformBroadcaster> _tfBroadcaster;
  std::unique_ptr<tf2_ros::Buffer> _tf_buffer;                          // ThreadLocalize.h:403-404
  std::unique_ptr<tf2_ros::TransformListener> _tf_transform_listener;
  int _tfLookUpState[2] = {-1, -1};                                     // last outcome of the two look-ups (logged on change only)
  geometry_msgs::msg::PoseStamped _poseStamped;
  geometry_msgs::msg::TransformStamped _tf;

  std::mutex _reportMutex;
  ScanReport _report;
  uint64_t _processed;
};

} /* namespace ohm_tsd_slam */
