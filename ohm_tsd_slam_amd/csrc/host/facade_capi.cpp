// facade_capi.cpp -- a flat C surface over the C++ facade so that the Python test / bench drivers can
// exercise ThreadLocalize / ThreadMapping / ThreadGrid exactly as SlamNode wires them (SlamNode.cpp:27-129): one
// TsdGrid, one ThreadMapping, one ThreadGrid woken every occ_grid_time_interval, N ThreadLocalize sharing them, laser callbacks per robot.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "ThreadGrid.h"
#include "ThreadGridGroup.h"
#include "ThreadLocalize.h"
#include "ThreadMapping.h"

using namespace ohm_tsd_slam;

struct tsd_node;

// several nodes' grids on one GPU and the worker that merges and publishes their maps (ThreadGridGroup); the nodes outlive it
struct tsd_fleet
{
  std::vector<tsd_node*> nodes;
  std::vector<tsd_frontier> frontiers;    // the last tsd_fleet_frontiers
  ExplorePlan plan;                       // the last tsd_fleet_explore_plan
  ExploreDispatch dispatch;               // the last tsd_fleet_explore_dispatch
  ThreadGridGroup* group = nullptr;
  obvious::TsdGrid* fused = nullptr;      // the fleet's own grid: the TSD-level fusion of the nodes' grids (created by the first fusion)
};

struct tsd_node
{
  std::shared_ptr<rclcpp::Node> node;
  obvious::TsdGrid* grid = nullptr;
  ThreadMapping* mapping = nullptr;
  ThreadGrid* gridThread = nullptr;
  // SlamNode::_timer (SlamNode.cpp:128, :154-157): wakes the ThreadGrid every occ_grid_time_interval
  std::thread timer;
  std::mutex timerMutex;
  std::condition_variable timerCond;
  bool timerStop = false;
  std::vector<ThreadLocalize*> localizers;
  std::vector<uint64_t> submitted;
  bool synchronous = false;
  bool fused = true;
  std::vector<tsd_frontier> frontiers;    // the last tsd_node_frontiers
  ExplorePlan plan;                       // the last tsd_node_explore_plan
};

extern "C" {

tsd_node* tsd_node_create(const char* node_name)
{
  tsd_node* n = new tsd_node();
  n->node = std::make_shared<rclcpp::Node>(node_name ? node_name : "tsd_slam");
  return n;
}

void tsd_node_set_double(tsd_node* n, const char* name, double v) { n->node->set_parameter(name, v); }
void tsd_node_set_int(tsd_node* n, const char* name, int v) { n->node->set_parameter(name, v); }
void tsd_node_set_bool(tsd_node* n, const char* name, int v) { n->node->set_parameter(name, v != 0); }
void tsd_node_set_string(tsd_node* n, const char* name, const char* v) { n->node->set_parameter(name, std::string(v)); }

// the parameters SlamNode::initialize declares (SlamNode.cpp:40-58)
static void declare_node_parameters(const std::shared_ptr<rclcpp::Node>& node)
{
  node->declare_parameter("robot_nbr", 1);
  node->declare_parameter("x_off_factor", 0.5);
  node->declare_parameter("y_off_factor", 0.5);
  node->declare_parameter("x_offset", 0.0);
  node->declare_parameter("y_offset", 0.0);
  node->declare_parameter("map_size", 10);
  node->declare_parameter("cellsize", 0.025);
  node->declare_parameter("truncation_radius", 3);
  node->declare_parameter("occ_grid_time_interval", 2.0);
  node->declare_parameter("tf_map_frame", std::string("map"));
  // ThreadGrid's (ThreadGrid.cpp:42-47), declared here once: ThreadGrid reads them
  node->declare_parameter("pub_tsd_color_map", true);
  node->declare_parameter("object_inflation_factor", 2);
  node->declare_parameter("use_object_inflation", false);
}

#if !OHM_TSD_SLAM_HAVE_ROS
// Parameter surface without a device (CPU test): what SlamNode::initialize, every ThreadLocalize constructor and
// every ThreadLocalize::init would declare, as "name|type|default" lines.  Returns the bytes needed.
int tsd_node_declared_parameters(tsd_node* n, char* buf, int cap)
{
  auto& node = n->node;
  declare_node_parameters(node);
  const unsigned robotNbr = (unsigned)node->get_parameter("robot_nbr").as_int();
  const std::string node_name = std::string(node->get_name()) + "/";
  for(unsigned i = 0; i < robotNbr; i++)
  {
    std::string robot = "";
    if(robotNbr > 1)
    {
      const std::string key = "robot_" + std::to_string(i) + "/name";
      node->declare_parameter(key, "robot_" + std::to_string(i));
      robot = node->get_parameter(key).as_string();
      if(robot.size() > 0 && robot.back() != '/') robot += "/";
    }
    ThreadLocalize::declareParameters(node, robot);
    ThreadLocalize::declareInitParameters(node, node_name + robot);
  }
  std::string out;
  for(const auto& kv : node->declared_parameters())
  {
    const auto& v = kv.second.value();
    char num[64];
    if(std::holds_alternative<bool>(v)) out += kv.first + "|bool|" + (std::get<bool>(v) ? "true" : "false") + "\n";
    else if(std::holds_alternative<int64_t>(v)) out += kv.first + "|int|" + std::to_string(std::get<int64_t>(v)) + "\n";
    else if(std::holds_alternative<double>(v)) { std::snprintf(num, sizeof(num), "%.17g", std::get<double>(v)); out += kv.first + "|double|" + num + "\n"; }
    else out += kv.first + "|string|" + std::get<std::string>(v) + "\n";
  }
  if(buf && cap > 0)
  {
    std::strncpy(buf, out.c_str(), (size_t)cap - 1);
    buf[cap - 1] = 0;
  }
  return (int)out.size() + 1;
}
#endif

// SlamNode::initialize (SlamNode.cpp:40-122): grid parameters, grid, mapping thread, localisers
int tsd_node_initialize(tsd_node* n, int device)
{
  auto& node = n->node;
  declare_node_parameters(node);
  const unsigned robotNbr = (unsigned)node->get_parameter("robot_nbr").as_int();
  const double xOffset = node->get_parameter("x_offset").as_double();
  const double yOffset = node->get_parameter("y_offset").as_double();
  unsigned octaveFactor = (unsigned)node->get_parameter("map_size").as_int();
  const double cellSize = node->get_parameter("cellsize").as_double();
  const double truncationRadius = (double)node->get_parameter("truncation_radius").as_int();
  if(octaveFactor > 15)
    octaveFactor = 10;   // "Unknown map size -> set to default" (SlamNode.cpp:71-75)

  n->grid = new obvious::TsdGrid(cellSize, obvious::LAYOUT_32x32, static_cast<obvious::EnumTsdGridLayout>(octaveFactor), device);
  if(!n->grid->valid())
    return TSD_E_NODEVICE;
  n->grid->setMaxTruncation(truncationRadius * cellSize);
  n->mapping = new ThreadMapping(n->grid);
  n->gridThread = new ThreadGrid(n->grid, node, xOffset, yOffset);
  if(robotNbr == 1)
  {
    n->localizers.push_back(new ThreadLocalize(n->grid, n->mapping, node, "", xOffset, yOffset));
  }
  else
  {
    for(unsigned i = 0; i < robotNbr; i++)
    {
      const std::string key = "robot_" + std::to_string(i) + "/name";
      node->declare_parameter(key, "robot_" + std::to_string(i));
      const std::string robot_name = node->get_parameter(key).as_string();
      n->localizers.push_back(new ThreadLocalize(n->grid, n->mapping, node, robot_name, xOffset, yOffset));
    }
  }
  n->submitted.assign(n->localizers.size(), 0);
  const double interval = node->get_parameter("occ_grid_time_interval").as_double();
  if(interval > 0.0)
  {
    const auto period = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::duration<double>(interval));
    n->timer = std::thread([n, period] {
      std::unique_lock<std::mutex> lk(n->timerMutex);
      auto next = std::chrono::steady_clock::now() + period;
      while(!n->timerCond.wait_until(lk, next, [n] { return n->timerStop; }))
      {
        n->gridThread->unblock();            // SlamNode::timedGridPub
        next += period;
      }
    });
  }
  // several robots on one grid: their scans go through the grid's dispatcher as batched launches (TSD_NO_BATCH: the split
  // scan on one stream per robot instead; TSD_BATCH_SLOTS: batch slots used in turn, default 2 -- A/B switches for measurements)
  if(n->localizers.size() > 1 && !std::getenv("TSD_NO_CONCURRENT") && !std::getenv("TSD_NO_BATCH"))
  {
    const char* e = std::getenv("TSD_BATCH_SLOTS");
    n->grid->enableBatchedScans((int)n->localizers.size(), e ? std::atoi(e) : 2);
  }
  for(auto* l : n->localizers)
  {
    l->setSynchronous(n->synchronous);
    l->setFused(n->fused);
    l->setConcurrent(n->localizers.size() > 1 && !std::getenv("TSD_NO_CONCURRENT"));   // (env: A/B switch for tests / measurements)
  }
  return TSD_OK;
}

// before the first scan: choose the fused device scan (default) or the reference's three-call flow
void tsd_node_set_fused(tsd_node* n, int on)
{
  n->fused = on != 0;
  for(auto* l : n->localizers)
    l->setFused(n->fused);
}

void tsd_node_set_synchronous(tsd_node* n, int on)
{
  n->synchronous = on != 0;
  for(auto* l : n->localizers)
    l->setSynchronous(n->synchronous);
}

int tsd_node_laser(tsd_node* n, int robot, const float* ranges, int count, double angle_min,
                   double angle_increment, long long stamp_ns)
{
  if(!n || robot < 0 || robot >= (int)n->localizers.size())
    return TSD_E_ARG;
  auto scan = std::make_shared<sensor_msgs::msg::LaserScan>();
  scan->ranges.assign(ranges, ranges + count);
  scan->angle_min = (float)angle_min;
  scan->angle_increment = (float)angle_increment;
  scan->header.stamp.sec = (int32_t)(stamp_ns / 1000000000LL);
  scan->header.stamp.nanosec = (uint32_t)(stamp_ns % 1000000000LL);
  n->localizers[robot]->laserCallBack(scan);
  return TSD_OK;
}

// ThreadLocalize::startAt: start (first call: `ranges` is the first scan) or re-seat the robot's localiser at the sensor pose pose33
// without touching the map.  TSD_E_ARG while scans of the robot are queued or being processed, or a push is queued at the mapper.
int tsd_node_start_at(tsd_node* n, int robot, const double* pose33, const float* ranges, int count, double angle_min,
                      double angle_increment, long long stamp_ns)
{
  if(!n || robot < 0 || robot >= (int)n->localizers.size() || !pose33 || !ranges || count < 1)
    return TSD_E_ARG;
  sensor_msgs::msg::LaserScan scan;
  scan.ranges.assign(ranges, ranges + count);
  scan.angle_min = (float)angle_min;
  scan.angle_increment = (float)angle_increment;
  scan.header.stamp.sec = (int32_t)(stamp_ns / 1000000000LL);
  scan.header.stamp.nanosec = (uint32_t)(stamp_ns % 1000000000LL);
  return n->localizers[robot]->startAt(pose33, scan) ? TSD_OK : TSD_E_ARG;
}

// the scan that tsd_node_laser will deliver NEXT (ThreadLocalize::announceNext): known ahead in a replay, or queued
int tsd_node_laser_ahead(tsd_node* n, int robot, const float* ranges, int count, double angle_min, double angle_increment,
                         long long stamp_ns)
{
  if(!n || robot < 0 || robot >= (int)n->localizers.size())
    return TSD_E_ARG;
  auto scan = std::make_shared<sensor_msgs::msg::LaserScan>();
  scan->ranges.assign(ranges, ranges + count);
  scan->angle_min = (float)angle_min;
  scan->angle_increment = (float)angle_increment;
  scan->header.stamp.sec = (int32_t)(stamp_ns / 1000000000LL);
  scan->header.stamp.nanosec = (uint32_t)(stamp_ns % 1000000000LL);
  n->localizers[robot]->announceNext(scan);
  return TSD_OK;
}

// Replay of recorded scans, the way `rosbag play` feeds the reference node: one publisher thread per robot, each handing
// its robot's scans to laserCallBack in order (synchronous facade: the callback returns when the scan has been processed, so
// every robot runs as fast as the node lets it and the robots' scans overlap).  scans[r] = n_scans x count floats.
int tsd_node_play(tsd_node* n, int robots, const float* const* scans, int first, int n_scans, int count, double angle_min,
                  double angle_increment, long long stamp0_ns, long long stamp_step_ns)
{
  if(!n || robots < 1 || robots > (int)n->localizers.size() || !scans || n_scans < 0 || first < 0)
    return TSD_E_ARG;
  std::vector<std::thread> pubs;
  std::atomic<int> failed{0};
  for(int r = 0; r < robots; r++)
    pubs.emplace_back([&, r] {
      for(int k = first; k < first + n_scans; k++)
      {
        if(k + 1 < first + n_scans)       // (a replay knows the next scan: the localiser stages it during this registration)
          tsd_node_laser_ahead(n, r, scans[r] + (size_t)(k + 1) * (size_t)count, count, angle_min, angle_increment,
                               stamp0_ns + (long long)(k + 1) * stamp_step_ns);
        if(tsd_node_laser(n, r, scans[r] + (size_t)k * (size_t)count, count, angle_min, angle_increment,
                          stamp0_ns + (long long)k * stamp_step_ns) != TSD_OK)
          failed++;
      }
    });
  for(auto& t : pubs)
    t.join();
  return failed ? TSD_E_ARG : TSD_OK;
}

// multi-robot dispatcher: batches begun and scans they carried (0, 0 without a dispatcher)
void tsd_node_batch_stats(tsd_node* n, unsigned long long* batches, unsigned long long* scans)
{
  obvious::ScanBatcher::Stats st;
  if(n && n->grid && n->grid->batcher())
    st = n->grid->batcher()->stats();
  if(batches) *batches = st.batches;
  if(scans) *scans = st.scans;
}

// asynchronous mode: wait until the localiser has nothing queued, the mapping queue is drained and
// the device is idle.  Returns 0 when idle, 1 on timeout.
int tsd_node_wait_idle(tsd_node* n, int timeout_ms)
{
  const auto t0 = std::chrono::steady_clock::now();
  for(;;)
  {
    bool idle = true;
    for(auto* l : n->localizers)
      idle = idle && l->idle();
    idle = idle && n->mapping->pending() == 0;
    if(idle)
    {
      std::lock_guard<std::mutex> lk(n->grid->mutex());
      tsd_sync(n->grid->context());
      return 0;
    }
    if(std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms))
      return 1;
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

unsigned long long tsd_node_processed(tsd_node* n, int robot) { return n->localizers[robot]->processedScans(); }

// report layout: pose[9], T[9], rms, pairs, iterations, icpState, validModel, validScene, regError,
// pushed, noModel, initialised, stamp [ns]  (29 doubles)
void tsd_node_report(tsd_node* n, int robot, double* out28)
{
  const ThreadLocalize::ScanReport r = n->localizers[robot]->lastReport();
  std::memcpy(out28, r.pose, sizeof(r.pose));
  std::memcpy(out28 + 9, r.T, sizeof(r.T));
  out28[18] = r.rms; out28[19] = r.pairs; out28[20] = r.iterations; out28[21] = r.icpState;
  out28[22] = r.validModel; out28[23] = r.validScene; out28[24] = r.regError; out28[25] = r.pushed;
  out28[26] = r.noModel; out28[27] = r.initialised; out28[28] = (double)r.stampNs;
}

// the robot's last pre-registration (registration_mode 2 / unfused 3): T[9], probability, idx_model, idx_scene, candidates,
// valid_model, valid_scene, control_points.  Returns 0 if there was none.
int tsd_node_preregistration(tsd_node* n, int robot, double* out16)
{
  tsd_tsdpdf_result r;
  if(!n->localizers[robot]->lastPreregistration(&r))
    return 0;
  std::memcpy(out16, r.T, sizeof(r.T));
  out16[9] = r.probability; out16[10] = r.idx_model; out16[11] = r.idx_scene; out16[12] = r.candidates;
  out16[13] = r.valid_model; out16[14] = r.valid_scene; out16[15] = r.control_points;
  return 1;
}

// last PoseStamped on <node>/<robot/>estimated_pose: x, y, z, qx, qy, qz, qw, publish count
void tsd_node_pose_msg(tsd_node* n, int robot, double* out8)
{
  auto pub = n->localizers[robot]->posePublisher();
  const auto m = pub->last();
  out8[0] = m.pose.position.x; out8[1] = m.pose.position.y; out8[2] = m.pose.position.z;
  out8[3] = m.pose.orientation.x; out8[4] = m.pose.orientation.y; out8[5] = m.pose.orientation.z;
  out8[6] = m.pose.orientation.w; out8[7] = (double)pub->count();
}

const char* tsd_node_pose_topic(tsd_node* n, int robot)
{
  return n->localizers[robot]->posePublisher()->topic().c_str();
}

// last TransformStamped the robot's broadcaster sent (map -> odom): tx, ty, tz, qx, qy, qz, qw, send count; frames as "frame_id|child_frame_id"
void tsd_node_tf_msg(tsd_node* n, int robot, double* out8, char* frames, int cap)
{
  auto* b = n->localizers[robot]->tfBroadcaster();
  const auto m = b->last();
  out8[0] = m.transform.translation.x; out8[1] = m.transform.translation.y; out8[2] = m.transform.translation.z;
  out8[3] = m.transform.rotation.x; out8[4] = m.transform.rotation.y; out8[5] = m.transform.rotation.z;
  out8[6] = m.transform.rotation.w; out8[7] = (double)b->count();
  if(frames && cap > 0)
    std::snprintf(frames, (size_t)cap, "%s|%s", m.header.frame_id.c_str(), m.child_frame_id.c_str());
}

// feed the robot's tf buffer (what a TransformListener does under ROS): `child` expressed in `parent`
int tsd_node_set_transform(tsd_node* n, int robot, const char* parent, const char* child, const double xyz[3], const double qxyzw[4])
{
  geometry_msgs::msg::TransformStamped t;
  t.header.frame_id = parent; t.child_frame_id = child;
  t.transform.translation.x = xyz[0]; t.transform.translation.y = xyz[1]; t.transform.translation.z = xyz[2];
  t.transform.rotation.x = qxyzw[0]; t.transform.rotation.y = qxyzw[1]; t.transform.rotation.z = qxyzw[2]; t.transform.rotation.w = qxyzw[3];
  return n->localizers[robot]->tfBuffer()->setTransform(t, "tsd_node_set_transform", true) ? 0 : -1;
}

// ThreadGrid: one publication now, on the caller's thread (what a timer wake-up does); TSD_OK or the frame's error
int tsd_node_publish_map(tsd_node* n)
{
  if(!n || !n->gridThread)
    return TSD_E_ARG;
  return n->gridThread->publish();
}

unsigned long long tsd_node_map_frames(tsd_node* n) { return (n && n->gridThread) ? n->gridThread->frames() : 0; }

unsigned long long tsd_node_map_updates(tsd_node* n) { return (n && n->gridThread) ? n->gridThread->updates() : 0; }

// last message on <node>/map_updates: x, y, width, height, stamp [ns] (5 doubles); data (width * height) when data_out is given;
// header.frame_id into frame_id.  Returns the number of update messages so far.
unsigned long long tsd_node_map_update_msg(tsd_node* n, int8_t* data_out, double* out5, char* frame_id, int cap)
{
  if(!n || !n->gridThread || !out5)
    return 0;
  const map_msgs::msg::OccupancyGridUpdate m = n->gridThread->lastUpdate();
  out5[0] = m.x; out5[1] = m.y; out5[2] = m.width; out5[3] = m.height;
  out5[4] = (double)m.header.stamp.sec * 1e9 + (double)m.header.stamp.nanosec;
  if(data_out && !m.data.empty())
    std::memcpy(data_out, m.data.data(), m.data.size());
  if(frame_id && cap > 0)
    std::snprintf(frame_id, (size_t)cap, "%s", m.header.frame_id.c_str());
  return n->gridThread->updates();
}

// last message on <node>/surface (parameter publish_surface_cloud): width (points), point_step, stamp [ns], fields (4 doubles);
// data (width * point_step bytes) when data_out is given; "frame_id|field,field,.." into text.  Returns the number published.
unsigned long long tsd_node_surface(tsd_node* n, uint8_t* data_out, double* out4, char* text, int cap)
{
  if(!n || !n->gridThread || !out4)
    return 0;
  const sensor_msgs::msg::PointCloud2 m = n->gridThread->lastSurface();
  out4[0] = m.width; out4[1] = m.point_step; out4[2] = (double)m.header.stamp.sec * 1e9 + (double)m.header.stamp.nanosec;
  out4[3] = (double)m.fields.size();
  if(data_out && !m.data.empty())
    std::memcpy(data_out, m.data.data(), m.data.size());
  if(text && cap > 0)
  {
    std::string t = m.header.frame_id + "|";
    for(size_t i = 0; i < m.fields.size(); i++)
      t += (i ? "," : "") + m.fields[i].name;
    std::snprintf(text, (size_t)cap, "%s", t.c_str());
  }
  return n->gridThread->surfaces();
}

// an OccupancyGrid as flat values: resolution, width, height, origin x, y, z, qx, qy, qz, qw, stamp [ns], map_load_time [ns]
// (12 doubles); data (width * height) when data_out is given; header.frame_id into frame_id
static void map_out(const nav_msgs::msg::OccupancyGrid& m, int8_t* data_out, double* out12, char* frame_id, int cap)
{
  auto ns = [](const builtin_interfaces::msg::Time& t) { return (double)t.sec * 1e9 + (double)t.nanosec; };
  out12[0] = m.info.resolution; out12[1] = m.info.width; out12[2] = m.info.height;
  out12[3] = m.info.origin.position.x; out12[4] = m.info.origin.position.y; out12[5] = m.info.origin.position.z;
  out12[6] = m.info.origin.orientation.x; out12[7] = m.info.origin.orientation.y; out12[8] = m.info.origin.orientation.z;
  out12[9] = m.info.origin.orientation.w; out12[10] = ns(m.header.stamp); out12[11] = ns(m.info.map_load_time);
  if(data_out && !m.data.empty())
    std::memcpy(data_out, m.data.data(), m.data.size());
  if(frame_id && cap > 0)
    std::snprintf(frame_id, (size_t)cap, "%s", m.header.frame_id.c_str());
}

// last message on <node>/map (map_out layout); returns the publish count
unsigned long long tsd_node_map_msg(tsd_node* n, int8_t* data_out, double* out12, char* frame_id, int cap)
{
  auto pub = n->gridThread->gridPublisher();
  map_out(pub->last(), data_out, out12, frame_id, cap);
  return pub->count();
}

// <node>/costmap and <node>/costmap_updates (parameter publish_costmap): messages published on the two topics together
unsigned long long tsd_node_costmaps(tsd_node* n) { return (n && n->gridThread) ? n->gridThread->costmaps() : 0; }

// the inflation radius in cells the node computes its cost map with (0 with the parameter off)
int tsd_node_costmap_radius(tsd_node* n) { return (n && n->gridThread) ? n->gridThread->costmapRadiusCells() : 0; }

// last message on <node>/costmap (map_out layout) and the topic's name into `topic`; returns the topic's publish count.  Without the
// topic (the parameter is off): 0, an empty name, out12 zeroed.
unsigned long long tsd_node_costmap(tsd_node* n, int8_t* data_out, double* out12, char* frame_id, int cap, char* topic, int topic_cap)
{
  if(topic && topic_cap > 0)
    topic[0] = 0;
  if(!n || !n->gridThread || !out12)
    return 0;
  auto pub = n->gridThread->costmapPublisher();
  if(!pub)
  {
    for(int i = 0; i < 12; i++) out12[i] = 0.0;
    if(frame_id && cap > 0) frame_id[0] = 0;
    return 0;
  }
  map_out(pub->last(), data_out, out12, frame_id, cap);
  if(topic && topic_cap > 0)
    std::snprintf(topic, (size_t)topic_cap, "%s", pub->topic().c_str());
  return pub->count();
}

// last message on <node>/costmap_updates, as tsd_node_map_update_msg; returns the topic's publish count (0 without the topic)
unsigned long long tsd_node_costmap_update(tsd_node* n, int8_t* data_out, double* out5, char* frame_id, int cap)
{
  if(!n || !n->gridThread || !out5)
    return 0;
  const map_msgs::msg::OccupancyGridUpdate m = n->gridThread->lastCostmapUpdate();
  out5[0] = m.x; out5[1] = m.y; out5[2] = m.width; out5[3] = m.height;
  out5[4] = (double)m.header.stamp.sec * 1e9 + (double)m.header.stamp.nanosec;
  if(data_out && !m.data.empty())
    std::memcpy(data_out, m.data.data(), m.data.size());
  if(frame_id && cap > 0)
    std::snprintf(frame_id, (size_t)cap, "%s", m.header.frame_id.c_str());
  auto pub = n->gridThread->costmapUpdatePublisher();
  return pub ? pub->count() : 0;
}

// <node>/frontiers (parameter publish_frontiers): the last sensor_msgs/PointCloud2, as tsd_node_surface; returns the number published
unsigned long long tsd_node_frontier_cloud(tsd_node* n, uint8_t* data_out, double* out4, char* text, int cap)
{
  if(!n || !n->gridThread || !out4)
    return 0;
  const sensor_msgs::msg::PointCloud2 m = n->gridThread->lastFrontiers();
  out4[0] = m.width; out4[1] = m.point_step; out4[2] = (double)m.header.stamp.sec * 1e9 + (double)m.header.stamp.nanosec;
  out4[3] = (double)m.fields.size();
  if(data_out && !m.data.empty())
    std::memcpy(data_out, m.data.data(), m.data.size());
  if(text && cap > 0)
  {
    std::string t = m.header.frame_id + "|";
    for(size_t i = 0; i < m.fields.size(); i++)
      t += (i ? "," : "") + m.fields[i].name;
    std::snprintf(text, (size_t)cap, "%s", t.c_str());
  }
  return n->gridThread->frontierClouds();
}

// frontier_min_size as the node read it
unsigned tsd_node_frontier_min_size(tsd_node* n) { return (n && n->gridThread) ? n->gridThread->frontierMinSize() : 0u; }

// a pose's cell in a map with origin (ox, oy): floor((p - o) / cs); (-1, -1) for a pose that is not finite or far outside
static void pose_cell(double px, double py, double ox, double oy, double cs, int32_t* xy)
{
  const double fx = std::floor((px - ox) / cs), fy = std::floor((py - oy) / cs);
  const bool ok = fx >= 0.0 && fx < 2147483647.0 && fy >= 0.0 && fy < 2147483647.0;
  xy[0] = ok ? static_cast<int32_t>(fx) : -1;
  xy[1] = ok ? static_cast<int32_t>(fy) : -1;
}

// The seeds of a frontier or route call on the node's map and the map's placement: n_seeds < 0: one seed per robot of the node, the
// cell of its last estimated pose, else the caller's.  Returns their number.
static int node_seeds(tsd_node* n, const int32_t* seeds_xy, int n_seeds, double* place, int32_t* seeds)
{
  // (a map's origin and resolution are fixed when the node is built: the seeds' cells use the values the call returns below)
  n->gridThread->mapPlacement(place);
  const double ox = place[0], oy = place[1], cs = place[2];
  int ns = n_seeds;
  if(n_seeds < 0)
  {
    ns = static_cast<int>(std::min<size_t>(n->localizers.size(), TSD_FRONTIER_MAX_SEEDS));
    for(int r = 0; r < ns; r++)
    {
      const auto pose = n->localizers[(size_t)r]->posePublisher()->last();
      pose_cell(pose.pose.position.x, pose.pose.position.y, ox, oy, cs, &seeds[2 * r]);
    }
  }
  else
    std::memcpy(seeds, seeds_xy, (size_t)(2 * ns) * sizeof(int32_t));
  return ns;
}

// The frontiers of the map the node published last (ThreadGrid::frontiers), kept for tsd_node_frontiers_fetch.  n_seeds < 0: one seed
// per robot of the node, the cell of its last estimated pose.  min_size 0: frontier_min_size.  seeds_out (2 * TSD_FRONTIER_MAX_SEEDS
// int32) / n_seeds_out: the seeds taken; origin_cs: the map's origin x, y and its resolution.  Returns TSD_OK or the error code.
int tsd_node_frontiers(tsd_node* n, const int32_t* seeds_xy, int n_seeds, unsigned min_size, int* count, int* seeds_used,
                       int32_t* seeds_out, int* n_seeds_out, double* origin_cs)
{
  if(!n || !n->gridThread || !count || n_seeds > TSD_FRONTIER_MAX_SEEDS || (n_seeds > 0 && !seeds_xy))
    return TSD_E_ARG;
  double place[3];
  int32_t seeds[2 * TSD_FRONTIER_MAX_SEEDS];
  const int ns = node_seeds(n, seeds_xy, n_seeds, place, seeds);
  const int rc = n->gridThread->frontiers(seeds, ns, min_size ? min_size : n->gridThread->frontierMinSize(), &n->frontiers, seeds_used, place);
  if(rc != TSD_OK)
    return rc;
  *count = static_cast<int>(n->frontiers.size());
  if(seeds_out)
    std::memcpy(seeds_out, seeds, (size_t)(2 * ns) * sizeof(int32_t));
  if(n_seeds_out)
    *n_seeds_out = ns;
  if(origin_cs)
  {
    origin_cs[0] = place[0]; origin_cs[1] = place[1]; origin_cs[2] = place[2];
  }
  return TSD_OK;
}

void tsd_node_frontiers_fetch(tsd_node* n, tsd_frontier* out)
{
  if(n && out && !n->frontiers.empty())
    std::memcpy(out, n->frontiers.data(), n->frontiers.size() * sizeof(tsd_frontier));
}

// what a plan's fetch copies: counts[0] frontiers (as many goals and lengths), counts[1] path cells, counts[2] seeds used
static void plan_counts(const ExplorePlan& p, int* counts)
{
  counts[0] = static_cast<int>(p.frontiers.size());
  counts[1] = static_cast<int>(p.paths.size());
  counts[2] = p.seedsUsed;
}

static void plan_fetch(const ExplorePlan& p, tsd_frontier* rec, tsd_route_goal* goals, int32_t* lens, uint32_t* paths)
{
  if(rec && !p.frontiers.empty())
    std::memcpy(rec, p.frontiers.data(), p.frontiers.size() * sizeof(tsd_frontier));
  if(goals && !p.goals.empty())
    std::memcpy(goals, p.goals.data(), p.goals.size() * sizeof(tsd_route_goal));
  if(lens && !p.lens.empty())
    std::memcpy(lens, p.lens.data(), p.lens.size() * sizeof(int32_t));
  if(paths && !p.paths.empty())
    std::memcpy(paths, p.paths.data(), p.paths.size() * sizeof(uint32_t));
}

// Frontiers, cost-to-go field, goals and paths of the map the node published last (ThreadGrid::explorePlan), kept for
// tsd_node_explore_plan_fetch.  Seeds, min_size, seeds_out, n_seeds_out and origin_cs as tsd_node_frontiers (at least one seed);
// source TSD_ROUTE_MAP / TSD_ROUTE_COSTMAP; counts: see plan_counts; *info: the route's.
int tsd_node_explore_plan(tsd_node* n, const int32_t* seeds_xy, int n_seeds, unsigned min_size, int source, int max_weight, int max_len,
                          int* counts, tsd_route_info* info, int32_t* seeds_out, int* n_seeds_out, double* origin_cs)
{
  if(!n || !n->gridThread || !counts || !info || n_seeds == 0 || n_seeds > TSD_FRONTIER_MAX_SEEDS || (n_seeds > 0 && !seeds_xy))
    return TSD_E_ARG;
  double place[3];
  int32_t seeds[2 * TSD_FRONTIER_MAX_SEEDS];
  const int ns = node_seeds(n, seeds_xy, n_seeds, place, seeds);
  const int rc = n->gridThread->explorePlan(seeds, ns, min_size ? min_size : n->gridThread->frontierMinSize(), source, max_weight, max_len,
                                            &n->plan, place);
  if(rc != TSD_OK)
    return rc;
  plan_counts(n->plan, counts);
  *info = n->plan.route;
  if(seeds_out)
    std::memcpy(seeds_out, seeds, (size_t)(2 * ns) * sizeof(int32_t));
  if(n_seeds_out)
    *n_seeds_out = ns;
  if(origin_cs)
  {
    origin_cs[0] = place[0]; origin_cs[1] = place[1]; origin_cs[2] = place[2];
  }
  return TSD_OK;
}

void tsd_node_explore_plan_fetch(tsd_node* n, tsd_frontier* rec, tsd_route_goal* goals, int32_t* lens, uint32_t* paths)
{
  if(n)
    plan_fetch(n->plan, rec, goals, lens, paths);
}

// What a scan from each goal of the plan made last would uncover (ThreadGrid::exploreGains): one tsd_view_gain per goal of
// tsd_node_explore_plan's counts, on the same frame; *radius_cells: the radius the call used.
int tsd_node_explore_gains(tsd_node* n, double view_radius_m, int unknown_depth, tsd_view_gain* out, int* radius_cells)
{
  if(!n || !n->gridThread || (!out && !n->plan.goals.empty()))
    return TSD_E_ARG;
  return n->gridThread->exploreGains(n->plan.goals.data(), n->plan.goals.size(), view_radius_m, unknown_depth, out, radius_cells);
}

// The paths of the plan made last straightened into waypoints (ThreadGrid::exploreWaypoints): for each goal of
// tsd_node_explore_plan's counts one tsd_waypoint_info and way[i * max_way + k], k < min(n_way, max_way), linear cell indices, seed
// first and goal last; *lookahead_cells: the look-ahead the call used.
int tsd_node_explore_waypoints(tsd_node* n, double lookahead_m, unsigned slack, int max_len, int max_way, uint32_t* way, tsd_waypoint_info* info,
                               int* lookahead_cells)
{
  if(!n || !n->gridThread || ((!way || !info) && !n->plan.goals.empty()))
    return TSD_E_ARG;
  return n->gridThread->exploreWaypoints(n->plan.goals.data(), n->plan.goals.size(), lookahead_m, slack, max_len, max_way, way, info,
                                         lookahead_cells);
}

// what the drive entries take beside the poses: limits [v_max, w_max, horizon_s, nose_m], ints [n_speeds, a_end, a_nose, a_cost,
// a_turn, nose_miss, margin], the footprint as n_foot pairs (x, y) [m]
static bool drive_request(const double* limits, const int* ints, const double* footprint_xy, int n_foot, DriveRequest* q)
{
  if(!limits || !ints || n_foot < 0 || (n_foot > 0 && !footprint_xy) || ints[5] < 0 || ints[6] < 0)
    return false;
  q->vMax = limits[0]; q->wMax = limits[1]; q->horizon = limits[2]; q->nose = limits[3];
  q->nSpeeds = ints[0];
  q->aEnd = ints[1]; q->aNose = ints[2]; q->aCost = ints[3]; q->aTurn = ints[4];
  q->noseMiss = static_cast<uint32_t>(ints[5]);
  q->margin = static_cast<uint32_t>(ints[6]);
  q->footprint.assign(footprint_xy, footprint_xy + 2 * (size_t)n_foot);
  return true;
}

// one robot's answer as eight doubles -- v, w, end x, end y, admissible, next x, next y, next yaw; the record itself goes to
// `choice` --, and the call's shape as [T, V, Wn, B] with dt
static void drive_answer(const DriveAnswer& a, double* out8, tsd_drive_choice* choice)
{
  out8[0] = a.v; out8[1] = a.w; out8[2] = a.endXy[0]; out8[3] = a.endXy[1]; out8[4] = (double)a.choice.admissible;
  out8[5] = a.next[0]; out8[6] = a.next[1]; out8[7] = a.next[2];
  if(choice)
    *choice = a.choice;
}

static void drive_shape(const DriveSamples& s, int* shape4, double* dt)
{
  if(shape4)
  {
    shape4[0] = s.prm.steps; shape4[1] = s.prm.n_speeds; shape4[2] = s.prm.n_turns; shape4[3] = s.prm.n_body;
  }
  if(dt)
    *dt = s.dt;
}

// The velocity of the next step towards goal `goal` of the plan made last (ThreadGrid::exploreDrive): pose_xyt x, y [m], yaw [rad] in
// the map's frame; out8: v [m/s], w [rad/s], the end cell's centre x, y [m], the admissible samples, the pose after one step x, y,
// yaw; choice, shape4 [T, V, Wn, B] and dt may be NULL.
int tsd_node_explore_drive(tsd_node* n, int goal, const double* pose_xyt, const double* limits, const int* ints, const double* footprint_xy,
                           int n_foot, double* out8, tsd_drive_choice* choice, int* shape4, double* dt)
{
  DriveRequest q;
  if(!n || !n->gridThread || !pose_xyt || !out8 || goal < 0 || (size_t)goal >= n->plan.goals.size() ||
     !drive_request(limits, ints, footprint_xy, n_foot, &q))
    return TSD_E_ARG;
  DriveAnswer a;
  DriveSamples s;
  const int rc = n->gridThread->exploreDrive(n->plan.goals[(size_t)goal], pose_xyt, q, &a, &s);
  if(rc != TSD_OK)
    return rc;
  drive_answer(a, out8, choice);
  drive_shape(s, shape4, dt);
  return TSD_OK;
}

// what the live entries take beside that: n_live scan end points as pairs (x, y) [m] in the map's frame, the radius round each [m]
// and the radius round a robot's own pose inside which points are dropped [m]
static bool live_request(const double* live_xy, int n_live, double radius_m, double skip_m, LiveRequest* l)
{
  if(n_live < 0 || (n_live > 0 && !live_xy))
    return false;
  l->points.assign(live_xy, live_xy + 2 * (size_t)n_live);
  l->radius = radius_m;
  l->skipRadius = skip_m;
  return true;
}

// tsd_node_explore_drive with the current scans' end points keeping the arcs off what is not on the map yet (ThreadGrid::exploreDrive
// with a LiveRequest): live_kept the points the node's own disc did not drop, blocked_live the samples refused by reason 7; both may
// be NULL.
int tsd_node_explore_drive_live(tsd_node* n, int goal, const double* pose_xyt, const double* limits, const int* ints, const double* footprint_xy,
                                int n_foot, const double* live_xy, int n_live, double live_radius_m, double live_skip_m, double* out8,
                                tsd_drive_choice* choice, int* shape4, double* dt, int* live_kept, int32_t* blocked_live)
{
  DriveRequest q;
  LiveRequest l;
  if(!n || !n->gridThread || !pose_xyt || !out8 || goal < 0 || (size_t)goal >= n->plan.goals.size() ||
     !drive_request(limits, ints, footprint_xy, n_foot, &q) || !live_request(live_xy, n_live, live_radius_m, live_skip_m, &l))
    return TSD_E_ARG;
  DriveAnswer a;
  DriveSamples s;
  LiveAnswer la;
  const int rc = n->gridThread->exploreDrive(n->plan.goals[(size_t)goal], pose_xyt, q, &a, &s, &l, &la);
  if(rc != TSD_OK)
    return rc;
  drive_answer(a, out8, choice);
  drive_shape(s, shape4, dt);
  if(live_kept) *live_kept = la.kept;
  if(blocked_live) *blocked_live = la.blocked.empty() ? 0 : la.blocked[0];
  return TSD_OK;
}

// <node>/get_map (ThreadGrid::getMapServCallBack): the last map with a fresh stamp (map_out layout); 1 if the service answered
int tsd_node_get_map(tsd_node* n, int8_t* data_out, double* out12, char* frame_id, int cap)
{
  auto req = std::make_shared<nav_msgs::srv::GetMap::Request>();
  auto res = std::make_shared<nav_msgs::srv::GetMap::Response>();
  if(!n->gridThread->getMapServCallBack(req, res))
    return 0;
  map_out(res->map, data_out, out12, frame_id, cap);
  return 1;
}

// last message on <node>/map/image: height, width, step, is_bigendian, stamp [ns] (5 doubles); data (step * height) when
// data_out is given; "encoding|frame_id" into text.  Returns the publish count.
unsigned long long tsd_node_map_image_msg(tsd_node* n, uint8_t* data_out, double* out5, char* text, int cap)
{
  auto pub = n->gridThread->imagePublisher();
  const sensor_msgs::msg::Image m = pub->last();
  out5[0] = m.height; out5[1] = m.width; out5[2] = m.step; out5[3] = m.is_bigendian;
  out5[4] = (double)m.header.stamp.sec * 1e9 + (double)m.header.stamp.nanosec;
  if(data_out && !m.data.empty())
    std::memcpy(data_out, m.data.data(), m.data.size());
  if(text && cap > 0)
    std::snprintf(text, (size_t)cap, "%s|%s", m.encoding.c_str(), m.header.frame_id.c_str());
  return pub->count();
}

// ---- fleet: the merged map of several nodes' grids on one GPU (ThreadGridGroup) ----------------
// The first node publishes (<node>/merged_map, <node>/get_merged_map; its inflation parameters apply); every node's x_offset /
// y_offset places its grid.  NULL when the group is refused, with the reason in err.
tsd_fleet* tsd_fleet_create(int n, tsd_node* const* nodes, char* err, int cap)
{
  auto refuse = [&](const char* what) -> tsd_fleet* {
    if(err && cap > 0) std::snprintf(err, (size_t)cap, "%s", what);
    return nullptr;
  };
  if(n < 1 || !nodes)
    return refuse("tsd_fleet_create: no nodes");
  std::vector<ThreadGridGroup::Member> members;
  for(int i = 0; i < n; i++)
  {
    if(!nodes[i] || !nodes[i]->grid || !nodes[i]->grid->valid())
      return refuse("tsd_fleet_create: a node is not initialised");
    members.push_back({nodes[i]->grid, nodes[i]->node->get_parameter("x_offset").as_double(),
                       nodes[i]->node->get_parameter("y_offset").as_double()});
  }
  tsd_fleet* f = new tsd_fleet();
  f->nodes.assign(nodes, nodes + n);
  try
  {
    f->group = new ThreadGridGroup(nodes[0]->node, members);
  }
  catch(const std::exception& e)
  {
    delete f;
    return refuse(e.what());
  }
  return f;
}

void tsd_fleet_destroy(tsd_fleet* f)
{
  if(!f)
    return;
  if(f->group)
  {
    f->group->terminateThread();
    while(!f->group->alive(1)) {}
    delete f->group;
  }
  delete f->fused;
  delete f;
}

// TSD-level fusion of the nodes' grids (ThreadGridGroup::fuse) into a grid the fleet owns: as large as node 0's and where node 0's
// lies.  Returns its context (an ordinary grid: ray cast, localise, push, store, colour image), NULL on failure with the code in *rc.
tsd_ctx* tsd_fleet_fuse_tsd(tsd_fleet* f, int* rc)
{
  int dummy;
  if(!rc)
    rc = &dummy;
  *rc = TSD_E_ARG;
  if(!f || !f->group || f->nodes.empty())
    return nullptr;
  obvious::TsdGrid* g0 = f->nodes[0]->grid;
  if(!f->fused)
  {
    int log2 = 0;
    while((1u << log2) < g0->getCellsX())
      log2++;
    f->fused = new obvious::TsdGrid(g0->getCellSize(), obvious::LAYOUT_32x32, static_cast<obvious::EnumTsdGridLayout>(log2),
                                    tsd_device(g0->context()));
    if(!f->fused->valid())
    {
      delete f->fused;
      f->fused = nullptr;
      *rc = TSD_E_NODEVICE;
      return nullptr;
    }
  }
  f->fused->setMaxTruncation(g0->getMaxTruncation());
  *rc = f->group->fuse(f->fused);
  return *rc == TSD_OK ? f->fused->context() : nullptr;
}

// ThreadGridGroup::setTransforms: T33s holds one 3x3 row-major transform per node (9n doubles), T[i] = node i's grid coordinates into
// node 0's.  TSD_OK, or TSD_E_ARG with the reason in err (the group stays as it was).
int tsd_fleet_set_transforms(tsd_fleet* f, const double* T33s, char* err, int cap)
{
  auto refuse = [&](const char* what) {
    if(err && cap > 0) std::snprintf(err, (size_t)cap, "%s", what);
    return TSD_E_ARG;
  };
  if(!f || !f->group || !T33s)
    return refuse("tsd_fleet_set_transforms: no fleet or no transforms");
  std::vector<std::array<double, 9>> T(f->nodes.size());
  for(size_t i = 0; i < T.size(); i++)
    std::memcpy(T[i].data(), T33s + 9 * i, 9 * sizeof(double));
  try
  {
    f->group->setTransforms(T);
  }
  catch(const std::exception& e)
  {
    return refuse(e.what());
  }
  return TSD_OK;
}

void tsd_fleet_fused_lock(tsd_fleet* f) { if(f && f->fused) f->fused->mutex().lock(); }
void tsd_fleet_fused_unlock(tsd_fleet* f) { if(f && f->fused) f->fused->mutex().unlock(); }

// the colour image of the fused grid as ThreadGrid would publish it (sensor_msgs/Image, rgb8, one pixel per cell): tsd_node_map_image_msg's
// layout; data_out NULL: the sizes only.  TSD_OK or the error code (TSD_E_ARG before the first fusion).
int tsd_fleet_fused_image_msg(tsd_fleet* f, uint8_t* data_out, double* out5, char* text, int cap)
{
  if(!f || !f->fused || !out5)
    return TSD_E_ARG;
  const unsigned int w = f->fused->getCellsX(), h = f->fused->getCellsY();
  out5[0] = h; out5[1] = w; out5[2] = 3.0 * w; out5[3] = 0.0;
  const builtin_interfaces::msg::Time now = f->nodes[0]->node->get_clock()->now();
  out5[4] = (double)now.sec * 1e9 + (double)now.nanosec;
  if(text && cap > 0)
    std::snprintf(text, (size_t)cap, "%s|%s", sensor_msgs::image_encodings::RGB8.c_str(), "map");
  if(!data_out)
    return TSD_OK;
  std::lock_guard<std::mutex> g(f->fused->mutex());
  return tsd_color_image(f->fused->context(), data_out, w, h);
}

// one merge and publication now, on the caller's thread (what a wake-up of the worker does); TSD_OK or the error
int tsd_fleet_publish_merged(tsd_fleet* f) { return (f && f->group) ? f->group->publish() : TSD_E_ARG; }

// The frontiers of the merged map published last with one seed per node: robot 0's last estimated pose, taken from the map frame into
// the node's grid coordinates by the node's own map origin and carried on by the group (ThreadGridGroup::frontiers).  Kept for
// tsd_fleet_frontiers_fetch.  seeds_out: 2 int32 per node, *n_seeds_out: the nodes; origin_cs: the merged map's origin x, y and its
// resolution.  At most TSD_FRONTIER_MAX_SEEDS nodes (TSD_E_ARG beyond).
static std::vector<double> fleet_grid_xy(tsd_fleet* f);
int tsd_fleet_frontiers(tsd_fleet* f, unsigned min_size, int* count, int* seeds_used, int32_t* seeds_out, int* n_seeds_out, double* origin_cs)
{
  if(!f || !f->group || !count)
    return TSD_E_ARG;
  const std::vector<double> xy = fleet_grid_xy(f);
  const int rc = f->group->frontiers(xy.data(), min_size ? min_size : 1u, &f->frontiers, seeds_used, seeds_out, origin_cs);
  if(rc != TSD_OK)
    return rc;
  *count = static_cast<int>(f->frontiers.size());
  if(n_seeds_out)
    *n_seeds_out = static_cast<int>(f->nodes.size());
  return TSD_OK;
}

// The same with the routes (ThreadGridGroup::explorePlan), kept for tsd_fleet_explore_plan_fetch: counts and info as
// tsd_node_explore_plan; a goal's seed is the index of the node nearest to that frontier.
int tsd_fleet_explore_plan(tsd_fleet* f, unsigned min_size, int max_len, int* counts, tsd_route_info* info, int32_t* seeds_out, int* n_seeds_out,
                           double* origin_cs)
{
  if(!f || !f->group || !counts || !info)
    return TSD_E_ARG;
  const std::vector<double> xy = fleet_grid_xy(f);
  const int rc = f->group->explorePlan(xy.data(), min_size ? min_size : 1u, max_len, &f->plan, seeds_out, origin_cs);
  if(rc != TSD_OK)
    return rc;
  plan_counts(f->plan, counts);
  *info = f->plan.route;
  if(n_seeds_out)
    *n_seeds_out = static_cast<int>(f->nodes.size());
  return TSD_OK;
}

void tsd_fleet_explore_plan_fetch(tsd_fleet* f, tsd_frontier* rec, tsd_route_goal* goals, int32_t* lens, uint32_t* paths)
{
  if(f)
    plan_fetch(f->plan, rec, goals, lens, paths);
}

// Which node takes which goal of the plan made last (ThreadGridGroup::exploreAssign): goal_of_robot and picked hold one entry per node.
int tsd_fleet_explore_assign(tsd_fleet* f, double view_radius_m, unsigned gain_weight, int unknown_depth, int32_t* goal_of_robot,
                             tsd_view_gain* picked, int* rounds, int* radius_cells)
{
  if(!f || !f->group)
    return TSD_E_ARG;
  return f->group->exploreAssign(f->plan.goals.data(), f->plan.goals.size(), view_radius_m, gain_weight, unknown_depth, goal_of_robot, picked,
                                 rounds, radius_cells);
}

// Frontiers, a field per node, the goal matrix, the assignment across nodes and each node's waypoints in one call on the merged map
// published last (ThreadGridGroup::exploreDispatch), kept for tsd_fleet_explore_dispatch_fetch.  counts: the frontiers, the nodes, the
// rounds, the view radius and the look-ahead in cells, the seeds used; seeds_out: 2 int32 per node; origin_cs as tsd_fleet_frontiers.
int tsd_fleet_explore_dispatch(tsd_fleet* f, unsigned min_size, double view_radius_m, unsigned gain_weight, int unknown_depth, double lookahead_m,
                               unsigned slack, int max_len, int max_way, int* counts, tsd_route_fields_info* info, int32_t* seeds_out, double* origin_cs)
{
  if(!f || !f->group || !counts || !info)
    return TSD_E_ARG;
  ExploreDispatch& d = f->dispatch;
  d.frames = 0;
  d.viewRadius = view_radius_m;
  d.lookahead = lookahead_m;
  d.gainWeight = gain_weight;
  d.slack = slack;
  d.unknownDepth = unknown_depth;
  d.maxLen = max_len;
  d.maxWay = max_way;
  const std::vector<double> xy = fleet_grid_xy(f);
  const int rc = f->group->exploreDispatch(xy.data(), min_size ? min_size : 1u, &d, seeds_out, origin_cs);
  if(rc != TSD_OK)
    return rc;
  counts[0] = static_cast<int>(d.frontiers.size());
  counts[1] = static_cast<int>(f->nodes.size());
  counts[2] = d.rounds;
  counts[3] = d.radiusCells;
  counts[4] = d.lookaheadCells;
  counts[5] = d.seedsUsed;
  *info = d.fields;
  return TSD_OK;
}

// The result of the last tsd_fleet_explore_dispatch: rec [frontiers], goals [nodes * frontiers], goal_of_robot and picked [nodes],
// way [nodes * max_way], way_info [nodes]; each pointer may be NULL.  TSD_E_ARG without a result and once the merged map has been
// published again: the result is then of a map that is no longer the published one.
int tsd_fleet_explore_dispatch_fetch(tsd_fleet* f, tsd_frontier* rec, tsd_route_goal* goals, int32_t* goal_of_robot, tsd_view_gain* picked,
                                     uint32_t* way, tsd_waypoint_info* way_info)
{
  if(!f || !f->group)
    return TSD_E_ARG;
  const ExploreDispatch& d = f->dispatch;
  if(d.frames == 0 || d.frames != f->group->frames())
    return TSD_E_ARG;
  if(rec && !d.frontiers.empty()) std::memcpy(rec, d.frontiers.data(), d.frontiers.size() * sizeof(tsd_frontier));
  if(goals && !d.goals.empty()) std::memcpy(goals, d.goals.data(), d.goals.size() * sizeof(tsd_route_goal));
  if(goal_of_robot) std::memcpy(goal_of_robot, d.goalOfRobot.data(), d.goalOfRobot.size() * sizeof(int32_t));
  if(picked) std::memcpy(picked, d.picked.data(), d.picked.size() * sizeof(tsd_view_gain));
  if(way) std::memcpy(way, d.way.data(), d.way.size() * sizeof(uint32_t));
  if(way_info) std::memcpy(way_info, d.wayInfo.data(), d.wayInfo.size() * sizeof(tsd_waypoint_info));
  return TSD_OK;
}

// Every node's next velocity towards the goal the last tsd_fleet_explore_dispatch gave it (ThreadGridGroup::exploreDrive): poses_xyt
// three doubles per node in the merged map's frame; out8 eight doubles per node as tsd_node_explore_drive, choice one record per node.
int tsd_fleet_explore_drive(tsd_fleet* f, const double* poses_xyt, const double* limits, const int* ints, const double* footprint_xy, int n_foot,
                            double* out8, tsd_drive_choice* choice, int* shape4, double* dt)
{
  DriveRequest q;
  if(!f || !f->group || !poses_xyt || !out8 || !drive_request(limits, ints, footprint_xy, n_foot, &q))
    return TSD_E_ARG;
  std::vector<DriveAnswer> a(f->nodes.size());
  DriveSamples s;
  const int rc = f->group->exploreDrive(f->dispatch, poses_xyt, q, a.data(), &s);
  if(rc != TSD_OK)
    return rc;
  for(size_t r = 0; r < a.size(); r++)
    drive_answer(a[r], out8 + 8 * r, choice ? choice + r : nullptr);
  drive_shape(s, shape4, dt);
  return TSD_OK;
}

// tsd_fleet_explore_drive with the nodes keeping `separation_m` [m] off each other (ThreadGridGroup::exploreDrive with a
// FleetDriveRequest): priority n_priority node indices, the first decides first, or NULL / 0 for the default; order_out and
// blocked_out one int per node, tracks_out (steps + 1) pairs (x, y) [m] per node, node after node, where tracks_cap doubles hold them.
int tsd_fleet_explore_drive_apart(tsd_fleet* f, const double* poses_xyt, const double* limits, const int* ints, const double* footprint_xy, int n_foot,
                                  double separation_m, const int32_t* priority, int n_priority, double* out8, tsd_drive_choice* choice, int* shape4,
                                  double* dt, int32_t* order_out, int32_t* blocked_out, double* tracks_out, int tracks_cap)
{
  DriveRequest q;
  if(!f || !f->group || !poses_xyt || !out8 || !drive_request(limits, ints, footprint_xy, n_foot, &q) || !(separation_m > 0.0) || n_priority < 0 ||
     (n_priority > 0 && !priority))
    return TSD_E_ARG;
  FleetDriveRequest fq;
  fq.separation = separation_m;
  fq.priority.assign(priority, priority + n_priority);
  FleetDriveAnswer fa;
  std::vector<DriveAnswer> a(f->nodes.size());
  DriveSamples s;
  const int rc = f->group->exploreDrive(f->dispatch, poses_xyt, q, a.data(), &s, &fq, &fa);
  if(rc != TSD_OK)
    return rc;
  if(tracks_out && (size_t)std::max(tracks_cap, 0) < fa.tracks.size())
    return TSD_E_ARG;
  for(size_t r = 0; r < a.size(); r++)
    drive_answer(a[r], out8 + 8 * r, choice ? choice + r : nullptr);
  drive_shape(s, shape4, dt);
  if(order_out) std::memcpy(order_out, fa.order.data(), fa.order.size() * sizeof(int32_t));
  if(blocked_out) std::memcpy(blocked_out, fa.blocked.data(), fa.blocked.size() * sizeof(int32_t));
  if(tracks_out) std::memcpy(tracks_out, fa.tracks.data(), fa.tracks.size() * sizeof(double));
  return TSD_OK;
}

// tsd_fleet_explore_drive (separation_m == 0) or tsd_fleet_explore_drive_apart (separation_m > 0) with the current scans' end points of
// all nodes as one live layer (ThreadGridGroup::exploreDrive with a LiveRequest; a skip disc at every node's pose): live_kept the
// points no disc dropped, blocked_live_out one int per node, the samples refused by reason 7.  order_out, blocked_out and tracks_out
// are written with a separation only.
int tsd_fleet_explore_drive_live(tsd_fleet* f, const double* poses_xyt, const double* limits, const int* ints, const double* footprint_xy, int n_foot,
                                 double separation_m, const int32_t* priority, int n_priority, const double* live_xy, int n_live,
                                 double live_radius_m, double live_skip_m, double* out8, tsd_drive_choice* choice, int* shape4, double* dt,
                                 int32_t* order_out, int32_t* blocked_out, double* tracks_out, int tracks_cap, int* live_kept,
                                 int32_t* blocked_live_out)
{
  DriveRequest q;
  LiveRequest l;
  if(!f || !f->group || !poses_xyt || !out8 || !drive_request(limits, ints, footprint_xy, n_foot, &q) || !(separation_m >= 0.0) || n_priority < 0 ||
     (n_priority > 0 && (!priority || !(separation_m > 0.0))) || !live_request(live_xy, n_live, live_radius_m, live_skip_m, &l))
    return TSD_E_ARG;
  const bool apart = separation_m > 0.0;
  FleetDriveRequest fq;
  fq.separation = separation_m;
  fq.priority.assign(priority, priority + n_priority);
  FleetDriveAnswer fa;
  LiveAnswer la;
  std::vector<DriveAnswer> a(f->nodes.size());
  DriveSamples s;
  const int rc = f->group->exploreDrive(f->dispatch, poses_xyt, q, a.data(), &s, apart ? &fq : nullptr, apart ? &fa : nullptr, &l, &la);
  if(rc != TSD_OK)
    return rc;
  if(apart && tracks_out && (size_t)std::max(tracks_cap, 0) < fa.tracks.size())
    return TSD_E_ARG;
  for(size_t r = 0; r < a.size(); r++)
    drive_answer(a[r], out8 + 8 * r, choice ? choice + r : nullptr);
  drive_shape(s, shape4, dt);
  if(apart && order_out) std::memcpy(order_out, fa.order.data(), fa.order.size() * sizeof(int32_t));
  if(apart && blocked_out) std::memcpy(blocked_out, fa.blocked.data(), fa.blocked.size() * sizeof(int32_t));
  if(apart && tracks_out) std::memcpy(tracks_out, fa.tracks.data(), fa.tracks.size() * sizeof(double));
  if(live_kept) *live_kept = la.kept;
  if(blocked_live_out) std::memcpy(blocked_live_out, la.blocked.data(), la.blocked.size() * sizeof(int32_t));
  return TSD_OK;
}

// The merged plan's paths straightened into waypoints (ThreadGridGroup::exploreWaypoints), as tsd_node_explore_waypoints.
int tsd_fleet_explore_waypoints(tsd_fleet* f, double lookahead_m, unsigned slack, int max_len, int max_way, uint32_t* way, tsd_waypoint_info* info,
                                int* lookahead_cells)
{
  if(!f || !f->group || ((!way || !info) && !f->plan.goals.empty()))
    return TSD_E_ARG;
  return f->group->exploreWaypoints(f->plan.goals.data(), f->plan.goals.size(), lookahead_m, slack, max_len, max_way, way, info, lookahead_cells);
}

// every node's position (robot 0's last estimated pose) in ITS grid's coordinates, NaN without a pose: what the group's calls take
static std::vector<double> fleet_grid_xy(tsd_fleet* f)
{
  std::vector<double> xy(2 * f->nodes.size());
  for(size_t i = 0; i < f->nodes.size(); i++)
  {
    tsd_node* n = f->nodes[i];
    const double nan = std::nan("");
    xy[2 * i] = xy[2 * i + 1] = nan;
    if(n->localizers.empty() || !n->gridThread)
      continue;
    const auto pose = n->localizers[0]->posePublisher()->last();
    if(n->localizers[0]->posePublisher()->count() == 0)
      continue;
    // (the origin a node's map carries is fixed by its parameters: -(W / 2 + offset), whether or not a map was published yet)
    const double W = (double)n->grid->getCellsX() * (double)n->grid->getCellSize();
    const double ox = -(W * 0.5 + n->node->get_parameter("x_offset").as_double()), oy = -(W * 0.5 + n->node->get_parameter("y_offset").as_double());
    xy[2 * i] = pose.pose.position.x - ox;
    xy[2 * i + 1] = pose.pose.position.y - oy;
  }
  return xy;
}

void tsd_fleet_frontiers_fetch(tsd_fleet* f, tsd_frontier* out)
{
  if(f && out && !f->frontiers.empty())
    std::memcpy(out, f->frontiers.data(), f->frontiers.size() * sizeof(tsd_frontier));
}
unsigned long long tsd_fleet_merged_frames(tsd_fleet* f) { return (f && f->group) ? f->group->frames() : 0; }

// last message on <node>/merged_map (map_out layout); returns the publish count
unsigned long long tsd_fleet_merged_map_msg(tsd_fleet* f, int8_t* data_out, double* out12, char* frame_id, int cap)
{
  auto pub = f->group->gridPublisher();
  map_out(pub->last(), data_out, out12, frame_id, cap);
  return pub->count();
}

// <node>/get_merged_map: the last merged map with a fresh stamp (map_out layout); 1 if the service answered
int tsd_fleet_get_merged_map(tsd_fleet* f, int8_t* data_out, double* out12, char* frame_id, int cap)
{
  auto req = std::make_shared<nav_msgs::srv::GetMap::Request>();
  auto res = std::make_shared<nav_msgs::srv::GetMap::Response>();
  if(!f->group->getMapServCallBack(req, res))
    return 0;
  map_out(res->map, data_out, out12, frame_id, cap);
  return 1;
}

tsd_ctx* tsd_node_grid_ctx(tsd_node* n) { return n->grid ? n->grid->context() : nullptr; }
// the facade's grid mutex (obvious::TsdGrid::mutex()): whoever talks to the context through the raw tsd_* ABI while the
// node's worker threads may be running takes it around each call, like the facade's own classes do
void tsd_node_grid_lock(tsd_node* n) { if(n && n->grid) n->grid->mutex().lock(); }
void tsd_node_grid_unlock(tsd_node* n) { if(n && n->grid) n->grid->mutex().unlock(); }
// obvious::TsdGrid::frontierMutex for a caller that runs tsd_frontiers_* on the node's context itself: taken BEFORE tsd_node_grid_lock,
// held until the result is fetched
void tsd_node_frontier_lock(tsd_node* n) { if(n && n->grid) n->grid->frontierMutex().lock(); }
void tsd_node_frontier_unlock(tsd_node* n) { if(n && n->grid) n->grid->frontierMutex().unlock(); }

// SlamNode::~SlamNode shutdown order (SlamNode.cpp:131-152): localisers, then ThreadGrid (its timer first), then the mapper
void tsd_node_destroy(tsd_node* n)
{
  if(!n)
    return;
  for(auto* l : n->localizers)
  {
    l->terminateThread();
    while(!l->alive(1)) {}
    delete l;
  }
  if(n->timer.joinable())
  {
    {
      std::lock_guard<std::mutex> lk(n->timerMutex);
      n->timerStop = true;
    }
    n->timerCond.notify_all();
    n->timer.join();
  }
  if(n->gridThread)
  {
    n->gridThread->terminateThread();
    while(!n->gridThread->alive(1)) {}
    delete n->gridThread;
  }
  if(n->mapping)
  {
    n->mapping->terminateThread();
    while(!n->mapping->alive(1)) {}
    delete n->mapping;
  }
  delete n->grid;
  delete n;
}

// host-only helpers for the CPU unit tests of the sensor model and gates ------------------------
void tsd_host_sensor_ingest_f32(const float* ranges, int n, double ang_res, double phi_min, double max_range,
                                double* data_out, unsigned char* mask_out, int remask)
{
  obvious::SensorPolar2D s((unsigned)n, ang_res, phi_min, max_range, 0.001, 2.0);
  s.setRealMeasurementData(std::vector<float>(ranges, ranges + n));
  s.setStandardMask();
  if(remask == 2)   // the shortcut the fused scan path uses
  {
    std::vector<uint8_t> m;
    s.maskForMapping(m);
    std::memcpy(data_out, s.getRealMeasurementData(), sizeof(double) * (size_t)n);
    std::memcpy(mask_out, m.data(), (size_t)n);
    return;
  }
  if(remask)
  {
    std::unique_ptr<obvious::SensorPolar2D> c(s.copyForMapping());
    std::memcpy(data_out, c->getRealMeasurementData(), sizeof(double) * (size_t)n);
    std::memcpy(mask_out, c->maskBytes(), (size_t)n);
    return;
  }
  std::memcpy(data_out, s.getRealMeasurementData(), sizeof(double) * (size_t)n);
  std::memcpy(mask_out, s.maskBytes(), (size_t)n);
}

// pose after `transform(T1)` then `transform(T2)`, world rays scaled to `norm`, scene points
void tsd_host_sensor_chain(int n, double ang_res, double phi_min, const double* T1, const double* T2, double norm,
                           const float* ranges, double* pose_out, double* rays_out, double* rays_local_out,
                           double* scene_out, unsigned char* scene_mask_out, int* valid_out)
{
  obvious::SensorPolar2D s((unsigned)n, ang_res, phi_min, 30.0, 0.001, 2.0);
  obvious::Matrix A(3, 3, T1), B(3, 3, T2);
  s.setRealMeasurementData(std::vector<float>(ranges, ranges + n));
  s.setStandardMask();
  s.transform(&A);
  const double* r = s.getNormalizedRayMap(norm);
  (void)r;
  s.transform(&B);
  r = s.getNormalizedRayMap(norm);
  s.getTransformation().getData(pose_out);
  std::memcpy(rays_out, r, sizeof(double) * 2 * (size_t)n);
  std::memcpy(rays_local_out, s.getLocalRayMap(), sizeof(double) * 2 * (size_t)n);
  std::vector<char> m((size_t)n);
  *valid_out = (int)s.dataToCartesianVectorMask(scene_out, reinterpret_cast<bool*>(m.data()));
  for(int i = 0; i < n; i++) scene_mask_out[i] = m[(size_t)i] ? 1 : 0;
}

double tsd_host_calc_angle(const double* T) { obvious::Matrix M(3, 3, T); return ThreadLocalize::calcAngle(&M); }
int tsd_host_is_registration_error(const double* T, double trs, double rot)
{
  obvious::Matrix M(3, 3, T);
  return ThreadLocalize::isRegistrationError(&M, trs, rot) ? 1 : 0;
}
int tsd_host_is_pose_change_significant(const double* last, const double* cur)
{
  obvious::Matrix A(3, 3, last), B(3, 3, cur);
  return ThreadLocalize::isPoseChangeSignificant(&A, &B) ? 1 : 0;
}
void tsd_host_mat3_inv(const double* A, double* out) { obvious::Matrix M(3, 3, A); M.invert(); M.getData(out); }
int tsd_host_backproject(const double* pose, double x, double y, int n, double ang_res, double phi_min)
{
  obvious::SensorPolar2D s((unsigned)n, ang_res, phi_min, 30.0, 0.001, 2.0);
  s.setTransformation(obvious::Matrix(3, 3, pose));
  double p[2] = {x, y};
  return s.backProject(p);
}

}  // extern "C"
