// ThreadGrid.h -- the occupancy-grid worker; public surface of the reference's ThreadGrid (src/ThreadGrid.h:24-129,
// src/ThreadGrid.cpp).  Every wake-up publishes one frame of the device (tsd_map_frame_begin / _wait: the occupancy map and the
// colour image from one pass over the tiles) on <node>/map and <node>/map/image; <node>/get_map answers with the last map.
// With the parameter publish_map_updates (not in the reference; default false) only the first publication, and every one the device
// cannot take as a window, is a full map: the others are windowed frames (tsd_map_update_begin / _wait) published as
// map_msgs/OccupancyGridUpdate on <node>/map_updates, the form rviz and nav2's static layer listen for.
// With the parameter publish_surface_cloud (not in the reference; default false) every publication is followed by the map's surface
// (tsd_surface_extract: calcCoords' sub-cell points with their normals) as sensor_msgs/PointCloud2 on <node>/surface, in the map's frame.
// With the parameter publish_costmap (not in the reference; default false) every publication is followed by the cost map nav2's
// inflation layer would compute from the map just published (tsd_costmap_begin / _wait: the exact Euclidean clearance on the device):
// a full map is followed by a nav_msgs/OccupancyGrid on <node>/costmap, an update by a map_msgs/OccupancyGridUpdate on
// <node>/costmap_updates for the update's window grown by the inflation radius.  costmap_inflation_radius [m], costmap_inscribed_radius
// [m] and costmap_cost_scaling_factor are nav2's inflation_radius, the robot's inscribed radius and cost_scaling_factor.
// With the parameter publish_frontiers (not in the reference; default false) every publication, full or update, is followed by the
// frontiers of the map just published (tsd_frontiers_frame: the free cells that border unknown space as 8-connected components, on
// the device) as sensor_msgs/PointCloud2 on <node>/frontiers, one point per frontier of at least frontier_min_size cells (default 8).
#pragma once
#include <cstdint>
#include <memory>
#include <vector>
#include <mutex>

#include "ThreadSLAM.h"
#include "ros_shim.h"

namespace ohm_tsd_slam
{

/** What an explorer asks of a map in one call (ThreadGrid::explorePlan, ThreadGridGroup::explorePlan): the frontiers, for each the
 *  cheapest cell to drive to with its cost and the seed (robot) it is cheapest from, and the path to it. */
struct ExplorePlan
{
  std::vector<tsd_frontier> frontiers;
  std::vector<tsd_route_goal> goals;     // one per frontier, in the frontiers' order
  std::vector<int32_t> lens;             // one per frontier: the path's full length in cells (0: no goal; -1: the field did not converge)
  std::vector<uint32_t> paths;           // the paths one after the other, min(len, maxLen) linear cell indices each, goal first, seed last
  tsd_route_info route;
  int seedsUsed;
};

/** Route, goals and paths (tsd_route_*) on a context whose frontier result is in place, into out->goals, lens, paths and route.
 *  mapDev nullptr: the frame form from `source`, else the generic form on mapDev (width x height, rows of width bytes).  The caller
 *  holds the context's frontierMutex, and for the generic form the grid's mutex.  TSD_E_ARG where the device library has no routes. */
int routePlan(tsd_ctx* ctx, const void* mapDev, int width, int height, int source, const tsd_route_params& prm, int maxLen, ExplorePlan* out);
/** A view radius [m] in cells: rounded to the nearest, at least 1 and at most TSD_VIEW_MAX_RADIUS. */
int viewRadiusCells(double viewRadius, double cellSize);
/** A waypoint look-ahead [m] in path cells: rounded to the nearest, at least 1 and at most TSD_WAYPOINT_MAX_LOOKAHEAD. */
int waypointLookaheadCells(double lookahead, double cellSize);
/** The waypoints (tsd_route_waypoints) of `n` goals of a plan on the context that holds the plan's route result, in chunks the entry
 *  takes: way[i * prm.max_way + k], k < min(info[i].n_way, prm.max_way), seed first and goal last; a goal without a cell gets a record
 *  of len 0 and n_way 0.  The caller holds the context's frontierMutex, and for a route made by the generic form the grid's mutex.
 *  TSD_E_ARG where the device library has no waypoints. */
int routeWaypoints(tsd_ctx* ctx, const tsd_route_goal* goals, size_t n, const tsd_waypoint_params& prm, uint32_t* way, tsd_waypoint_info* info);

/** What exploreDrive is asked (ThreadGrid::exploreDrive, ThreadGridGroup::exploreDrive): the robot's limits, its footprint and the
 *  rollout's coefficients. */
struct DriveRequest
{
  double vMax = 0.0, wMax = 0.0, horizon = 0.0;   // [m/s], [rad/s], [s]
  int nSpeeds = 5;                                // V: v_max * i / (V - 1), the fastest first
  std::vector<double> footprint;                  // pairs (x, y) [m] in the robot's frame, x forward; empty: the centre alone
  int aEnd = 1, aNose = 1, aCost = 0, aTurn = 0;  // tsd_drive_params' coefficients
  double nose = 0.0;                              // [m]
  uint32_t noseMiss = 0;
  uint32_t margin = 0;                            // added to the goal's dist for the field's limit
};
/** The sample lists made of a request at a cell size: dt = cellSize / vMax (the top speed is one cell per step), T = min(256,
 *  ceil(horizon / dt)), the speeds vMax * i / (V - 1) fastest first, the turns 0, 1, -1, .. n, -n with n = round(wMax * dt * H / 2 pi). */
struct DriveSamples
{
  std::vector<int32_t> step, turn, body;
  tsd_drive_params prm;                           // points into the vectors
  double dt = 0.0;
};
/** What exploreDrive answers per robot: the command, where its arc ends and the pose to expect after one step, in the map's frame. */
struct DriveAnswer
{
  double v = 0.0, w = 0.0;                        // [m/s], [rad/s]; 0 without an admissible sample
  double endXy[2] = {0.0, 0.0};                   // the end cell's centre [m]; NaN without an admissible sample
  double next[3] = {0.0, 0.0, 0.0};               // x, y [m] and yaw [rad] after one step of the chosen arc (the pose itself without one)
  tsd_drive_choice choice;
};
/** TSD_E_ARG for limits that are not positive and finite, V outside 2 .. TSD_DRIVE_MAX_SPEEDS, a turn list beyond TSD_DRIVE_HEADINGS / 8
 *  or TSD_DRIVE_MAX_TURNS entries, more than TSD_DRIVE_MAX_BODY footprint points, a point or the nose beyond 64 cells, a coefficient
 *  outside 0 .. 255. */
int driveSamples(double cellSize, const DriveRequest& q, DriveSamples* s);
/** A pose x, y [m], yaw [rad] in the map's frame (origin, resolution) as cell, Q16 offset and heading index; false for a pose that is
 *  not finite or outside width x height. */
bool drivePose(const double* originRes, const double* xyt, int width, int height, int layer, tsd_drive_pose* p);
/** The answer of one robot from its choice: velocities from the chosen indices, the end cell in metres, tsd_drive_advance by one step. */
int driveAnswer(const DriveSamples& s, const double* originRes, int width, const tsd_drive_pose& pose, const tsd_drive_choice& c, DriveAnswer* out);

/** What exploreDrive is asked beside the DriveRequest where the current scans are to keep the arcs off what is not on the map yet
 *  (tsd_drive_live_set): the scans' end points and how far to stay away from them. */
struct LiveRequest
{
  std::vector<double> points;                     // pairs (x, y) [m] in the map's frame
  double radius = 0.0;                            // [m], to the nearest cell: every cell that close to a point refuses an arc
  double skipRadius = 0.0;                        // [m], rounded up to cells: points that close to a robot's own pose are dropped
};
/** ... and what it answers beside the DriveAnswers: the points no robot's disc dropped, and per robot the samples refused by reason 7. */
struct LiveAnswer
{
  int kept = 0;
  std::vector<int32_t> blocked;
};
/** The request in cells of the map (origin, resolution) -- a point's cell is taken as a pose's, floor((x - origin) / resolution) --
 *  with a skip disc at every pose of `poses`, and the layer set on `ctx` for a width x height image.  TSD_E_ARG where the device
 *  library has no live layer, for a point, radius or skip radius that is not finite or negative, and for what tsd_drive_live_set
 *  refuses. */
int liveSet(tsd_ctx* ctx, const double* originRes, const LiveRequest& live, const tsd_drive_pose* poses, size_t nPoses, int width, int height,
            int* kept);
/** tsd_drive_live_clear, and the samples of each of n robots whose `why` holds reason 7. */
void liveDone(tsd_ctx* ctx, const uint16_t* why, size_t nRobots, size_t samples, std::vector<int32_t>* blocked);

class ThreadGrid : public ThreadSLAM
{
public:
  ThreadGrid(obvious::TsdGrid* grid, const std::shared_ptr<rclcpp::Node>& node, const double xOffset, const double yOffset);
  virtual ~ThreadGrid();

  /** one publication on the caller's thread, what every wake-up of the event loop does (not in the reference: deterministic tests).
   *  Returns TSD_OK or the frame's error code. */
  int publish(void);
  /** frames published so far */
  uint64_t frames(void);
  /** update messages published so far (publish_map_updates) */
  uint64_t updates(void);

  std::shared_ptr<rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>> gridPublisher() { return _gridPub; }
  std::shared_ptr<rclcpp::Publisher<sensor_msgs::msg::Image>> imagePublisher() { return _pubColorImage; }
  /** <node>/map_updates; nullptr unless publish_map_updates is set */
  std::shared_ptr<rclcpp::Publisher<map_msgs::msg::OccupancyGridUpdate>> updatePublisher() { return _updatePub; }
  /** the last update message (width 0 before the first one) */
  map_msgs::msg::OccupancyGridUpdate lastUpdate(void);
  /** <node>/surface; nullptr unless publish_surface_cloud is set */
  std::shared_ptr<rclcpp::Publisher<sensor_msgs::msg::PointCloud2>> surfacePublisher() { return _surfacePub; }
  /** the last surface message (no fields before the first one) and the number published */
  sensor_msgs::msg::PointCloud2 lastSurface(void);
  uint64_t surfaces(void);
  std::shared_ptr<rclcpp::Service<nav_msgs::srv::GetMap>> mapService() { return _getMapServ; }
  /** <node>/costmap and <node>/costmap_updates; nullptr unless publish_costmap is set (the latter also needs publish_map_updates) */
  std::shared_ptr<rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>> costmapPublisher() { return _costmapPub; }
  std::shared_ptr<rclcpp::Publisher<map_msgs::msg::OccupancyGridUpdate>> costmapUpdatePublisher() { return _costmapUpdatePub; }
  /** the last cost map update message (width 0 before the first one), the messages published on the two topics together, and the
   *  inflation radius in cells (0 with the parameter off) */
  map_msgs::msg::OccupancyGridUpdate lastCostmapUpdate(void);
  uint64_t costmaps(void);
  int costmapRadiusCells(void) const { return _publishCostmap ? _costPrm.radius_cells : 0; }
  /** <node>/frontiers; nullptr unless publish_frontiers is set */
  std::shared_ptr<rclcpp::Publisher<sensor_msgs::msg::PointCloud2>> frontierPublisher() { return _frontierPub; }
  /** the last frontier message (no fields before the first one), the number published, and frontier_min_size */
  sensor_msgs::msg::PointCloud2 lastFrontiers(void);
  uint64_t frontierClouds(void);
  uint32_t frontierMinSize(void) const { return _frontierMinSize; }
  /** The frontiers of the map published last (tsd_frontiers_frame), between two publications: records of at least minSize cells in
   *  ascending root index, reachability from the n seed cells seedsXy (x, y pairs; n == 0: -1 everywhere), the number of seeds that
   *  counted, and in originRes the origin x, y and the resolution (a float32) <node>/map carries.  Holds the publish mutex, so the map
   *  is the one the records belong to, and the grid's frontierMutex for the call.  TSD_E_ARG before the first publication. */
  int frontiers(const int32_t* seedsXy, int n, uint32_t minSize, std::vector<tsd_frontier>* out, int* seedsUsed, double* originRes);
  /** frontiers(), then the cost-to-go field from the same seeds (tsd_route_frame on `source`: TSD_ROUTE_MAP with unit weights, or
   *  TSD_ROUTE_COSTMAP -- the cost map of the last publication, parameter publish_costmap -- with free_max 98 and
   *  tsd_route_weights(98, maxWeight)), the goal of every frontier and the paths to them, cut at maxLen cells.  n is 1 ..
   *  TSD_FRONTIER_MAX_SEEDS.  Holds the publish mutex and, from the frontier call to the last fetch, the grid's frontierMutex (the
   *  goals read the frontier result).  TSD_E_ARG before the first publication. */
  int explorePlan(const int32_t* seedsXy, int n, uint32_t minSize, int source, int maxWeight, int maxLen, ExplorePlan* out, double* originRes);
  /** What a scanner standing on each of `n` goals of the plan made last would see within viewRadius [m] (tsd_view_gains on the staged
   *  map, free_max 0; the radius rounded to cells, at least 1 and at most TSD_VIEW_MAX_RADIUS, returned in *radiusCells): one record
   *  per goal, zeros for a goal without a cell.  Holds the publish mutex and the grid's frontierMutex.  TSD_E_ARG without a plan, where
   *  the map has been published again since the plan was made, and where the device library has no views. */
  int exploreGains(const tsd_route_goal* goals, size_t n, double viewRadius, int unknownDepth, tsd_view_gain* out, int* radiusCells);
  /** The paths to `n` goals of the plan made last, straightened into waypoints joined by straight drivable segments
   *  (tsd_route_waypoints on the plan's route result): segments span at most `lookahead` [m] of path -- rounded to cells, at least 1 and
   *  at most TSD_WAYPOINT_MAX_LOOKAHEAD, returned in *lookaheadCells -- and may cost `slack` more than the field's difference; paths
   *  longer than maxLen cells are not straightened; way[i * maxWay + k], seed first, goal last.  Holds the publish mutex and the grid's
   *  frontierMutex.  TSD_E_ARG without a plan, where the map has been published again since the plan was made, and where the device
   *  library has no waypoints. */
  int exploreWaypoints(const tsd_route_goal* goals, size_t n, double lookahead, uint32_t slack, int maxLen, int maxWay, uint32_t* way,
                       tsd_waypoint_info* info, int* lookaheadCells);
  /** The velocity of the next step towards `goal` of the plan made last, for a robot at poseXyt (x, y [m], yaw [rad] in the map's
   *  frame): a route call seeded at the goal's cell on the plan's source with the plan's weights (tsd_route_frame; limit: the goal's
   *  dist plus q.margin), then tsd_drive_rollout with the lists of driveSamples.  The goal-seeded field REPLACES the plan's route
   *  result on the context, so exploreWaypoints is refused from then on until the next explorePlan (the plan's goals and paths have
   *  been fetched by then); exploreDrive itself may be called again.  Holds the locks explorePlan holds.  TSD_E_ARG without a plan,
   *  once the map has been published again, for a goal without a cell, a pose outside the map, what driveSamples refuses, and where
   *  the device library has no rollout.
   *  With `live` the current scans' end points refuse arcs as well (reason 7 of the rule): the layer is set behind the route call --
   *  the skip disc is the robot's own pose --, the rollout runs with it and it is cleared again before the locks are given up, so no
   *  other caller of the context ever meets it.  liveOut gets the points kept and the samples the layer refused.  TSD_E_ARG also
   *  for a NULL liveOut, what liveSet refuses and where the device library has no live layer. */
  int exploreDrive(const tsd_route_goal& goal, const double* poseXyt, const DriveRequest& q, DriveAnswer* out, DriveSamples* samples,
                   const LiveRequest* live = nullptr, LiveAnswer* liveOut = nullptr);
  /** origin x, y and resolution of <node>/map: fixed by the parameters at construction, the same before and after a publication */
  void mapPlacement(double* originRes);

  /** the get_map service (ThreadGrid.cpp:135-142): the last map with a fresh stamp */
  bool getMapServCallBack(const std::shared_ptr<nav_msgs::srv::GetMap::Request> req,
                          std::shared_ptr<nav_msgs::srv::GetMap::Response> res);

protected:
  virtual void eventLoop(void);

private:
  int publishUpdate(const tsd_map_window& win);
  int publishSurface(const std_msgs::msg::Header& header);
  int publishCostmap(const tsd_map_window* mapWin);
  int publishFrontiers(const std_msgs::msg::Header& header);

private:
  std::shared_ptr<rclcpp::Node> _node;
  std::shared_ptr<nav_msgs::msg::OccupancyGrid> _occGrid;
  sensor_msgs::msg::Image _image;
  std::shared_ptr<rclcpp::Service<nav_msgs::srv::GetMap>> _getMapServ;
  std::shared_ptr<rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>> _gridPub;
  std::shared_ptr<rclcpp::Publisher<sensor_msgs::msg::Image>> _pubColorImage;
  std::shared_ptr<rclcpp::Publisher<map_msgs::msg::OccupancyGridUpdate>> _updatePub;
  map_msgs::msg::OccupancyGridUpdate _lastUpdate;     // (kept here: a real publisher does not keep its messages)
  bool _publishUpdates;
  std::shared_ptr<rclcpp::Publisher<sensor_msgs::msg::PointCloud2>> _surfacePub;
  sensor_msgs::msg::PointCloud2 _lastSurface;         // (likewise)
  bool _publishSurface;
  std::shared_ptr<rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>> _costmapPub;
  std::shared_ptr<rclcpp::Publisher<map_msgs::msg::OccupancyGridUpdate>> _costmapUpdatePub;
  map_msgs::msg::OccupancyGridUpdate _lastCostmapUpdate;   // (likewise)
  bool _publishCostmap;
  tsd_costmap_params _costPrm;
  int8_t* _hCost;                // page-locked: the full current cost map
  uint64_t _costmaps;
  std::shared_ptr<rclcpp::Publisher<sensor_msgs::msg::PointCloud2>> _frontierPub;
  sensor_msgs::msg::PointCloud2 _lastFrontiers;       // (likewise)
  bool _publishFrontiers;
  uint32_t _frontierMinSize;
  uint64_t _frontierClouds;
  unsigned int _width;
  unsigned int _height;
  double _cellSize;
  unsigned int _objInflateFactor;
  bool _objectInflation;
  // page-locked landing buffers of the frames (the persistent _occGridContent lives on the device)
  int8_t* _hOcc;
  uint8_t* _hRgb;
  std::mutex _publishMutex;      // one publication at a time (event loop, publish())
  std::mutex _msgMutex;          // _occGrid between a publication and the get_map service
  uint64_t _frames;
  uint64_t _updates;
  uint64_t _planStamp;           // _frames + _updates when explorePlan last succeeded (under _publishMutex; ~0: no plan)
  int _planSource, _planMaxWeight;   // what the plan was made on: exploreDrive's field is made on the same
  bool _planRouteReplaced;       // exploreDrive has put a goal-seeded field in the place of the plan's route result
  uint64_t _surfaces;
};

} /* namespace ohm_tsd_slam */
