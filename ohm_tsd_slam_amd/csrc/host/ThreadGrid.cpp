#include "ThreadGrid.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace ohm_tsd_slam
{

ThreadGrid::ThreadGrid(obvious::TsdGrid* grid, const std::shared_ptr<rclcpp::Node>& node, const double xOffset, const double yOffset):
    ThreadSLAM(*grid),
    _node(node),
    _occGrid(std::make_shared<nav_msgs::msg::OccupancyGrid>()),
    _publishCostmap(false),
    _hCost(nullptr),
    _costmaps(0),
    _publishFrontiers(false),
    _frontierMinSize(8),
    _frontierClouds(0),
    _width(grid->getCellsX()),
    _height(grid->getCellsY()),
    _cellSize(grid->getCellSize()),
    _hOcc(nullptr),
    _hRgb(nullptr),
    _frames(0),
    _updates(0),
    _planStamp(~(uint64_t)0),
    _planSource(TSD_ROUTE_MAP),
    _planMaxWeight(1),
    _planRouteReplaced(false),
    _surfaces(0)
{
  // (ThreadGrid.cpp:16-40)
  _occGrid->info.resolution           = static_cast<double>(_grid.getCellSize());
  _occGrid->info.width                = _grid.getCellsX();
  _occGrid->info.height               = _grid.getCellsY();
  _occGrid->info.origin.orientation.w = 1.0;
  _occGrid->info.origin.orientation.x = 0.0;
  _occGrid->info.origin.orientation.y = 0.0;
  _occGrid->info.origin.orientation.z = 0.0;
  _occGrid->info.origin.position.x    = -(static_cast<double>(_grid.getCellsX()) * static_cast<double>(_grid.getCellSize()) * 0.5 + xOffset);
  _occGrid->info.origin.position.y    = -(static_cast<double>(_grid.getCellsY()) * static_cast<double>(_grid.getCellSize()) * 0.5 + yOffset);
  _occGrid->info.origin.position.z    = 0.0;
  _occGrid->data.resize((size_t)_width * _height);

  // pub_tsd_color_map / object_inflation_factor / use_object_inflation are declared with the node's parameters
  // (facade_capi.cpp: declare_node_parameters), so they are only read here (ThreadGrid.cpp:42-53).  The reference never reads
  // pub_tsd_color_map: the image is published with every map.
  _occGrid->header.frame_id = node->get_parameter("tf_map_frame").as_string();
  _objectInflation = node->get_parameter("use_object_inflation").as_bool();
  _objInflateFactor = static_cast<unsigned int>(node->get_parameter("object_inflation_factor").as_int());

  // not in the reference: declared here, with the worker it belongs to (a launch file's or YAML's value is kept)
#if OHM_TSD_SLAM_HAVE_ROS
  if(!node->has_parameter("publish_map_updates"))
    node->declare_parameter<bool>("publish_map_updates", false);
#else
  node->declare_parameter("publish_map_updates", false);
#endif
  _publishUpdates = node->get_parameter("publish_map_updates").as_bool();
#if OHM_TSD_SLAM_HAVE_ROS
  if(!node->has_parameter("publish_surface_cloud"))
    node->declare_parameter<bool>("publish_surface_cloud", false);
#else
  node->declare_parameter("publish_surface_cloud", false);
#endif
  _publishSurface = node->get_parameter("publish_surface_cloud").as_bool();
#if OHM_TSD_SLAM_HAVE_ROS
  if(!node->has_parameter("publish_costmap"))
    node->declare_parameter<bool>("publish_costmap", false);
  if(!node->has_parameter("costmap_inflation_radius"))
    node->declare_parameter<double>("costmap_inflation_radius", 0.55);
  if(!node->has_parameter("costmap_inscribed_radius"))
    node->declare_parameter<double>("costmap_inscribed_radius", 0.25);
  if(!node->has_parameter("costmap_cost_scaling_factor"))
    node->declare_parameter<double>("costmap_cost_scaling_factor", 10.0);
#else
  node->declare_parameter("publish_costmap", false);
  node->declare_parameter("costmap_inflation_radius", 0.55);
  node->declare_parameter("costmap_inscribed_radius", 0.25);
  node->declare_parameter("costmap_cost_scaling_factor", 10.0);
#endif
  _publishCostmap = node->get_parameter("publish_costmap").as_bool();
  // R = ceil(radius / cell size), where a quotient that is whole up to rounding stays whole (0.55 / 0.025 is 22, not 23)
  double cellsR = std::ceil(node->get_parameter("costmap_inflation_radius").as_double() / _cellSize - 1e-9);
  if(!(cellsR >= 1.0))
    cellsR = 1.0;
  if(cellsR > (double)TSD_CLEARANCE_MAX_RADIUS)
  {
    if(_publishCostmap)
      std::fprintf(stderr, "ThreadGrid: costmap_inflation_radius is %.0f cells, clamped to %d\n", cellsR, TSD_CLEARANCE_MAX_RADIUS);
    cellsR = (double)TSD_CLEARANCE_MAX_RADIUS;
  }
  _costPrm.radius_cells = static_cast<int32_t>(cellsR);
  _costPrm.want_dist2 = 0;
  _costPrm.inscribed_radius_m = node->get_parameter("costmap_inscribed_radius").as_double();
  _costPrm.cost_scaling = node->get_parameter("costmap_cost_scaling_factor").as_double();
#if OHM_TSD_SLAM_HAVE_ROS
  if(!node->has_parameter("publish_frontiers"))
    node->declare_parameter<bool>("publish_frontiers", false);
  if(!node->has_parameter("frontier_min_size"))
    node->declare_parameter<int>("frontier_min_size", 8);
#else
  node->declare_parameter("publish_frontiers", false);
  node->declare_parameter("frontier_min_size", 8);
#endif
  _publishFrontiers = node->get_parameter("publish_frontiers").as_bool();
  const int64_t minSize = node->get_parameter("frontier_min_size").as_int();
  _frontierMinSize = minSize < 1 ? 1u : (minSize > 0x7FFFFFFF ? 0x7FFFFFFFu : static_cast<uint32_t>(minSize));

  const std::string node_name = _node->get_name();
  _gridPub = node->create_publisher<nav_msgs::msg::OccupancyGrid>(node_name + "/map", rclcpp::QoS(1).reliable().transient_local());
  _pubColorImage = node->create_publisher<sensor_msgs::msg::Image>(node_name + "/map/image", rclcpp::QoS(1).best_effort());
  if(_publishUpdates)
    _updatePub = node->create_publisher<map_msgs::msg::OccupancyGridUpdate>(node_name + "/map_updates",
                                                                            rclcpp::QoS(10).reliable().durability_volatile());
  if(_publishSurface)
    _surfacePub = node->create_publisher<sensor_msgs::msg::PointCloud2>(node_name + "/surface", rclcpp::QoS(1).reliable().durability_volatile());
  if(_publishCostmap)        // (the map's QoS on both topics)
  {
    _costmapPub = node->create_publisher<nav_msgs::msg::OccupancyGrid>(node_name + "/costmap", rclcpp::QoS(1).reliable().transient_local());
    if(_publishUpdates)
      _costmapUpdatePub = node->create_publisher<map_msgs::msg::OccupancyGridUpdate>(node_name + "/costmap_updates",
                                                                                     rclcpp::QoS(10).reliable().durability_volatile());
  }
  if(_publishFrontiers)
    _frontierPub = node->create_publisher<sensor_msgs::msg::PointCloud2>(node_name + "/frontiers", rclcpp::QoS(1).reliable().durability_volatile());
  _getMapServ = node->create_service<nav_msgs::srv::GetMap>(
    node_name + "/get_map",
    std::bind(&ThreadGrid::getMapServCallBack, this, std::placeholders::_1, std::placeholders::_2));

  // (ThreadGrid.cpp:64-68)
  _image.header.frame_id = "map";
  _image.step = _grid.getCellsY() * 3;
  _image.data.resize((size_t)_width * _height * 3);
  startThread();
}

ThreadGrid::~ThreadGrid()
{
  // (a publication in progress finishes first: publish() waits for its frame before it returns)
  terminateThread();
  joinThread();
  tsd_host_free(_hOcc);
  tsd_host_free(_hRgb);
  tsd_host_free(_hCost);
}

map_msgs::msg::OccupancyGridUpdate ThreadGrid::lastCostmapUpdate(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _lastCostmapUpdate;
}

uint64_t ThreadGrid::costmaps(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _costmaps;
}

sensor_msgs::msg::PointCloud2 ThreadGrid::lastFrontiers(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _lastFrontiers;
}

uint64_t ThreadGrid::frontierClouds(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _frontierClouds;
}

uint64_t ThreadGrid::frames(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _frames;
}

uint64_t ThreadGrid::updates(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _updates;
}

map_msgs::msg::OccupancyGridUpdate ThreadGrid::lastUpdate(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _lastUpdate;
}

sensor_msgs::msg::PointCloud2 ThreadGrid::lastSurface(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _lastSurface;
}

uint64_t ThreadGrid::surfaces(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _surfaces;
}

void ThreadGrid::eventLoop(void)
{
  while(_stayActive)
  {
    waitForWork();
    if(!_stayActive)
      break;
    publish();
  }
}

int ThreadGrid::publish(void)
{
  std::lock_guard<std::mutex> lk(_publishMutex);
  const size_t cells = (size_t)_width * _height;
  if(!_hOcc)                   // (allocated at the first publication: a node that never publishes pins nothing)
  {
    _hOcc = static_cast<int8_t*>(tsd_host_alloc(cells));
    _hRgb = static_cast<uint8_t*>(tsd_host_alloc(3 * cells));
  }
  if(!_hOcc || !_hRgb)
    return TSD_E_ARG;
  tsd_ctx* ctx = _grid.context();
  tsd_map_params prm;
  prm.inflate = _objectInflation ? 1 : 0;
  prm.inflate_factor = static_cast<int32_t>(_objInflateFactor);
  tsd_map_window win = {0, 0, 0, 0};
  int rc;
  {
    // the grid's mutex only while the frame is enqueued: the localisers go on while it is computed and copied
    std::lock_guard<std::mutex> g(_grid.mutex());
    rc = _publishUpdates ? tsd_map_update_begin(ctx, &prm, _hOcc, _hRgb, &win) : tsd_map_frame_begin(ctx, &prm, _hOcc, _hRgb);
  }
  if(rc != TSD_OK)
    return rc;
  int mapSize2 = 0;          // calcCoords' mapSize / 2 (of an update: of the window's tiles)
  rc = _publishUpdates ? tsd_map_update_wait(ctx, &mapSize2) : tsd_map_frame_wait(ctx, &mapSize2);
  if(rc != TSD_OK)
    return rc;
  if(_publishUpdates && win.width == 0)      // nothing was pushed since the last publication
    return TSD_OK;
  if(_publishUpdates && !((size_t)win.width == _width && (size_t)win.height == _height))
  {
    rc = publishUpdate(win);
    if(rc == TSD_OK && _publishCostmap)
      rc = publishCostmap(&win);
    if(rc == TSD_OK && _publishFrontiers)
      rc = publishFrontiers(_lastUpdate.header);
    if(rc == TSD_OK && _publishSurface)
      rc = publishSurface(_lastUpdate.header);
    return rc;
  }
  if(mapSize2 == 0)
  {
#if OHM_TSD_SLAM_HAVE_ROS
    RCLCPP_WARN(_node->get_logger(), "OccupancyGridThread: Warning! Raycasting returned with no coordinates, map contains no data yet!\n");
#else
    std::fprintf(stderr, "OccupancyGridThread: Warning! Raycasting returned with no coordinates, map contains no data yet!\n");
#endif
  }
  nav_msgs::msg::OccupancyGrid msg;
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    _occGrid->header.stamp       = _node->get_clock()->now();
    _occGrid->info.map_load_time = _node->get_clock()->now();
    std::memcpy(_occGrid->data.data(), _hOcc, cells);
    msg = *_occGrid;
    _frames++;
  }
  _gridPub->publish(msg);
  // (ThreadGrid.cpp:120-131)
  _image.header.stamp = msg.header.stamp;
  _image.height = msg.info.height;
  _image.width = msg.info.width;
  _image.encoding = sensor_msgs::image_encodings::RGB8;
  std::memcpy(_image.data.data(), _hRgb, 3 * cells);
  _pubColorImage->publish(_image);
  if(_publishCostmap)
  {
    rc = publishCostmap(nullptr);
    if(rc != TSD_OK)
      return rc;
  }
  if(_publishFrontiers)
  {
    rc = publishFrontiers(msg.header);
    if(rc != TSD_OK)
      return rc;
  }
  if(_publishSurface)
    return publishSurface(msg.header);
  return TSD_OK;
}

// The frontiers of the frame staged last.  The call runs on the context's copy stream and waits for it; the grid's mutex is not
// needed (the grid is not read).  The caller holds _publishMutex, so the staging is not replaced meanwhile; the grid's frontierMutex
// keeps the context's frontier scratch and result to one call at a time, this worker's or a ThreadGridGroup's on the same context,
// from the call to the fetch.
static int frameFrontiersLocked(obvious::TsdGrid& grid, const int32_t* seedsXy, int n, uint32_t minSize, std::vector<tsd_frontier>* out, int* seedsUsed)
{
  tsd_ctx* ctx = grid.context();
  tsd_frontier_params prm;
  prm.free_max = 0;
  prm.min_size = minSize;
  prm.n_seeds = n;
  prm.reserved = 0;
  prm.seeds_xy = n > 0 ? seedsXy : nullptr;
  int count = 0, used = 0;
  int rc = tsd_frontiers_frame(ctx, &prm, &count, &used);
  if(rc != TSD_OK)
    return rc;
  out->resize((size_t)count);
  if(count > 0)
    rc = tsd_frontiers_fetch(ctx, 0, count, out->data());
  if(seedsUsed)
    *seedsUsed = used;
  return rc;
}

static int frameFrontiers(obvious::TsdGrid& grid, const int32_t* seedsXy, int n, uint32_t minSize, std::vector<tsd_frontier>* out, int* seedsUsed)
{
  std::lock_guard<std::mutex> fl(grid.frontierMutex());
  return frameFrontiersLocked(grid, seedsXy, n, minSize, out, seedsUsed);
}

// The route entry points are weak references in the facade's workers: they also link against stand-ins of the device ABI that have
// no routes (tests/frontier_lock.cpp), where routePlan answers TSD_E_ARG.
#pragma weak tsd_route_weights
#pragma weak tsd_route_dev
#pragma weak tsd_route_frame
#pragma weak tsd_route_goals
#pragma weak tsd_route_goals_fetch
#pragma weak tsd_route_trace

int routePlan(tsd_ctx* ctx, const void* mapDev, int width, int height, int source, const tsd_route_params& prm, int maxLen, ExplorePlan* out)
{
  if(!tsd_route_dev || !tsd_route_frame || !tsd_route_goals || !tsd_route_goals_fetch || !tsd_route_trace)
    return TSD_E_ARG;
  if(!out || maxLen < 1 || maxLen > (1 << 24))
    return TSD_E_ARG;
  int rc = mapDev ? tsd_route_dev(ctx, mapDev, width, height, width, &prm, &out->route) : tsd_route_frame(ctx, source, &prm, &out->route);
  if(rc != TSD_OK)
    return rc;
  int count = 0;
  rc = tsd_route_goals(ctx, &count);
  if(rc != TSD_OK)
    return rc;
  out->goals.resize((size_t)count);
  out->lens.assign((size_t)count, 0);
  out->paths.clear();
  if(count == 0)
    return TSD_OK;
  rc = tsd_route_goals_fetch(ctx, 0, count, out->goals.data());
  if(rc != TSD_OK)
    return rc;
  // the goals with a cell, traced in chunks the trace call takes (at most TSD_ROUTE_MAX_GOALS goals and 1 << 24 path cells)
  std::vector<uint32_t> cells, buf;
  std::vector<int32_t> lens;
  std::vector<size_t> which;
  const size_t chunk = std::min<size_t>(TSD_ROUTE_MAX_GOALS, ((size_t)1 << 24) / (size_t)maxLen);
  for(size_t i = 0; i <= (size_t)count; i++)
  {
    if(i < (size_t)count && out->goals[i].cell != TSD_ROUTE_NONE)
    {
      cells.push_back(out->goals[i].cell);
      which.push_back(i);
    }
    if(cells.empty() || (cells.size() < chunk && i < (size_t)count))
      continue;
    buf.resize(cells.size() * (size_t)maxLen);
    lens.resize(cells.size());
    rc = tsd_route_trace(ctx, cells.data(), static_cast<int>(cells.size()), maxLen, buf.data(), lens.data());
    if(rc != TSD_OK)
      return rc;
    for(size_t g = 0; g < cells.size(); g++)
    {
      out->lens[which[g]] = lens[g];
      const size_t kept = (size_t)std::min(std::max(lens[g], 0), maxLen);
      out->paths.insert(out->paths.end(), buf.begin() + (ptrdiff_t)(g * (size_t)maxLen), buf.begin() + (ptrdiff_t)(g * (size_t)maxLen + kept));
    }
    cells.clear();
    which.clear();
  }
  return TSD_OK;
}

int ThreadGrid::explorePlan(const int32_t* seedsXy, int n, uint32_t minSize, int source, int maxWeight, int maxLen, ExplorePlan* out,
                            double* originRes)
{
  if(!out || !seedsXy || n < 1 || n > TSD_FRONTIER_MAX_SEEDS || (source != TSD_ROUTE_MAP && source != TSD_ROUTE_COSTMAP))
    return TSD_E_ARG;
  uint8_t weights[100];
  const int freeMax = source == TSD_ROUTE_COSTMAP ? 98 : 0;
  if(!tsd_route_weights || tsd_route_weights(freeMax, source == TSD_ROUTE_COSTMAP ? maxWeight : 1, weights) != TSD_OK)
    return TSD_E_ARG;
  std::lock_guard<std::mutex> lk(_publishMutex);
  if(originRes)
    mapPlacement(originRes);
  // the goals read the frontier result: one lock from the frontier call to the last fetch
  std::lock_guard<std::mutex> fl(_grid.frontierMutex());
  int rc = frameFrontiersLocked(_grid, seedsXy, n, minSize, &out->frontiers, &out->seedsUsed);
  if(rc != TSD_OK)
    return rc;
  tsd_route_params prm;
  prm.free_max = freeMax;
  prm.n_seeds = n;
  prm.seeds_xy = seedsXy;
  prm.weights = weights;
  prm.limit = 0;
  prm.max_rounds = 0;
  _planStamp = ~(uint64_t)0;
  rc = routePlan(_grid.context(), nullptr, 0, 0, source, prm, maxLen, out);
  if(rc == TSD_OK)
  {
    _planStamp = _frames + _updates;
    _planSource = source;
    _planMaxWeight = maxWeight;
    _planRouteReplaced = false;
  }
  return rc;
}

// The view entry points are weak references like the routes'.
#pragma weak tsd_view_gains
#pragma weak tsd_view_assign

int viewRadiusCells(double viewRadius, double cellSize)
{
  if(!(viewRadius > 0.0) || !(cellSize > 0.0))
    return 1;
  const double cells = std::floor(viewRadius / cellSize + 0.5);
  return cells < 1.0 ? 1 : cells > (double)TSD_VIEW_MAX_RADIUS ? TSD_VIEW_MAX_RADIUS : static_cast<int>(cells);
}

int ThreadGrid::exploreGains(const tsd_route_goal* goals, size_t n, double viewRadius, int unknownDepth, tsd_view_gain* out, int* radiusCells)
{
  if(!tsd_view_gains || (n > 0 && (!goals || !out)) || unknownDepth < 0)
    return TSD_E_ARG;
  std::lock_guard<std::mutex> lk(_publishMutex);
  if(_planStamp != _frames + _updates)
    return TSD_E_ARG;                  // no plan, or one of a map that has been published over
  tsd_view_params prm;
  prm.free_max = 0;
  prm.radius = viewRadiusCells(viewRadius, static_cast<double>(_grid.getCellSize()));
  prm.unknown_depth = unknownDepth;
  prm.use_claims = 0;
  if(radiusCells)
    *radiusCells = prm.radius;
  std::lock_guard<std::mutex> fl(_grid.frontierMutex());
  std::vector<uint32_t> cells(n);
  for(size_t i = 0; i < n; i++)
    cells[i] = goals[i].cell;          // (TSD_ROUTE_NONE lies outside every map: a record of zeros)
  for(size_t first = 0; first < n; first += TSD_VIEW_MAX_CELLS)
  {
    const int count = static_cast<int>(std::min<size_t>(TSD_VIEW_MAX_CELLS, n - first));
    const int rc = tsd_view_gains(_grid.context(), nullptr, 0, 0, 0, &prm, cells.data() + first, count, out + first);
    if(rc != TSD_OK)
      return rc;
  }
  return TSD_OK;
}

// The waypoint entry point is a weak reference like the routes'.
#pragma weak tsd_route_waypoints

int waypointLookaheadCells(double lookahead, double cellSize)
{
  if(!(lookahead > 0.0) || !(cellSize > 0.0))
    return 1;
  const double cells = std::floor(lookahead / cellSize + 0.5);
  return cells < 1.0 ? 1 : cells > (double)TSD_WAYPOINT_MAX_LOOKAHEAD ? TSD_WAYPOINT_MAX_LOOKAHEAD : static_cast<int>(cells);
}

int routeWaypoints(tsd_ctx* ctx, const tsd_route_goal* goals, size_t n, const tsd_waypoint_params& prm, uint32_t* way, tsd_waypoint_info* info)
{
  if(!tsd_route_waypoints || (n > 0 && (!goals || !way || !info)) || prm.max_len < 1 || prm.max_len > (1 << 24) || prm.max_way < 1 ||
     prm.max_way > (1 << 24))
    return TSD_E_ARG;
  std::vector<uint32_t> cells(n);
  for(size_t i = 0; i < n; i++)
    cells[i] = goals[i].cell;            // (TSD_ROUTE_NONE lies outside every map: a record of len 0, n_way 0)
  const size_t chunk = std::min<size_t>(TSD_ROUTE_MAX_GOALS, ((size_t)1 << 24) / (size_t)std::max(prm.max_len, prm.max_way));
  for(size_t first = 0; first < n; first += chunk)
  {
    const int count = static_cast<int>(std::min(chunk, n - first));
    const int rc = tsd_route_waypoints(ctx, cells.data() + first, count, &prm, way + first * (size_t)prm.max_way, info + first);
    if(rc != TSD_OK)
      return rc;
  }
  return TSD_OK;
}

int ThreadGrid::exploreWaypoints(const tsd_route_goal* goals, size_t n, double lookahead, uint32_t slack, int maxLen, int maxWay, uint32_t* way,
                                 tsd_waypoint_info* info, int* lookaheadCells)
{
  std::lock_guard<std::mutex> lk(_publishMutex);
  if(_planStamp != _frames + _updates || _planRouteReplaced)
    return TSD_E_ARG;                  // no plan, one of a map that has been published over, or its field replaced by exploreDrive's
  tsd_waypoint_params prm;
  prm.lookahead = waypointLookaheadCells(lookahead, static_cast<double>(_grid.getCellSize()));
  prm.slack = slack;
  prm.max_len = maxLen;
  prm.max_way = maxWay;
  if(lookaheadCells)
    *lookaheadCells = prm.lookahead;
  std::lock_guard<std::mutex> fl(_grid.frontierMutex());
  return routeWaypoints(_grid.context(), goals, n, prm, way, info);
}

// The rollout entry points are weak references like the routes'.
#pragma weak tsd_drive_rollout
#pragma weak tsd_drive_advance

static const double kTwoPi = 6.283185307179586476925286766559;

int driveSamples(double cellSize, const DriveRequest& q, DriveSamples* s)
{
  if(!s || !(cellSize > 0.0) || !(q.vMax > 0.0) || !(q.wMax >= 0.0) || !(q.horizon > 0.0) || !std::isfinite(q.vMax) || !std::isfinite(q.wMax) ||
     !std::isfinite(q.horizon) || q.nSpeeds < 2 || q.nSpeeds > TSD_DRIVE_MAX_SPEEDS || (q.footprint.size() & 1u) ||
     q.footprint.size() > 2u * TSD_DRIVE_MAX_BODY || !(q.nose >= 0.0) || q.noseMiss > TSD_ROUTE_MAX_DIST)
    return TSD_E_ARG;
  for(const int c : {q.aEnd, q.aNose, q.aCost, q.aTurn})
    if(c < 0 || c > 255)
      return TSD_E_ARG;
  s->dt = cellSize / q.vMax;
  const double steps = std::ceil(q.horizon / s->dt);
  const int T = steps < 1.0 ? 1 : steps > (double)TSD_DRIVE_MAX_STEPS ? TSD_DRIVE_MAX_STEPS : static_cast<int>(steps);
  const double turns = std::floor(q.wMax * s->dt * (double)TSD_DRIVE_HEADINGS / kTwoPi + 0.5);
  if(turns > (double)(TSD_DRIVE_HEADINGS / 8) || 2.0 * turns + 1.0 > (double)TSD_DRIVE_MAX_TURNS)
    return TSD_E_ARG;
  s->step.clear();
  for(int i = 0; i < q.nSpeeds; i++)
    s->step.push_back(static_cast<int32_t>(std::lrint(65536.0 * (double)(q.nSpeeds - 1 - i) / (double)(q.nSpeeds - 1))));
  s->turn.assign(1, 0);
  for(int m = 1; m <= static_cast<int>(turns); m++)
  {
    s->turn.push_back(m);
    s->turn.push_back(-m);
  }
  s->body.clear();
  for(const double v : q.footprint)
  {
    const double cells = v / cellSize;
    if(!(std::fabs(cells) <= 64.0))
      return TSD_E_ARG;
    s->body.push_back(static_cast<int32_t>(std::lrint(cells * 65536.0)));
  }
  const double nose = q.nose / cellSize;
  if(!(nose <= 64.0))
    return TSD_E_ARG;
  tsd_drive_params& p = s->prm;
  p.steps = T;
  p.n_speeds = q.nSpeeds;
  p.n_turns = static_cast<int32_t>(s->turn.size());
  p.n_body = static_cast<int32_t>(s->body.size() / 2);
  p.step_q16 = s->step.data();
  p.turn = s->turn.data();
  p.body_q16 = s->body.empty() ? nullptr : s->body.data();
  p.a_end = q.aEnd; p.a_nose = q.aNose; p.a_cost = q.aCost; p.a_turn = q.aTurn;
  p.nose_q16 = static_cast<int32_t>(std::lrint(nose * 65536.0));
  p.nose_miss = q.noseMiss;
  return TSD_OK;
}

bool drivePose(const double* originRes, const double* xyt, int width, int height, int layer, tsd_drive_pose* p)
{
  if(!std::isfinite(xyt[0]) || !std::isfinite(xyt[1]) || !std::isfinite(xyt[2]))
    return false;
  const double ux = (xyt[0] - originRes[0]) / originRes[2], uy = (xyt[1] - originRes[1]) / originRes[2];
  const double cx = std::floor(ux), cy = std::floor(uy);
  if(!(cx >= 0.0 && cx < (double)width && cy >= 0.0 && cy < (double)height))
    return false;
  p->x = static_cast<int32_t>(cx);
  p->y = static_cast<int32_t>(cy);
  p->fx = std::min(65535, std::max(0, static_cast<int>(std::floor((ux - cx) * 65536.0))));
  p->fy = std::min(65535, std::max(0, static_cast<int>(std::floor((uy - cy) * 65536.0))));
  const long long h = std::llrint(std::remainder(xyt[2], kTwoPi) * (double)TSD_DRIVE_HEADINGS / kTwoPi);
  p->heading = static_cast<int32_t>(((h % TSD_DRIVE_HEADINGS) + TSD_DRIVE_HEADINGS) % TSD_DRIVE_HEADINGS);
  p->layer = layer;
  return true;
}

int driveAnswer(const DriveSamples& s, const double* originRes, int width, const tsd_drive_pose& pose, const tsd_drive_choice& c, DriveAnswer* out)
{
  if(!tsd_drive_advance || !out)
    return TSD_E_ARG;
  const double res = originRes[2];
  out->choice = c;
  tsd_drive_pose next = pose;
  if(c.speed >= 0 && c.turn >= 0)
  {
    // host arithmetic on the chosen indices: a step of s cells takes dt, a turn of t headings per step likewise
    out->v = (double)s.step[(size_t)c.speed] / 65536.0 * res / s.dt;
    out->w = (double)s.turn[(size_t)c.turn] * kTwoPi / ((double)TSD_DRIVE_HEADINGS * s.dt);
    out->endXy[0] = ((double)(c.end_cell % (uint32_t)width) + 0.5) * res + originRes[0];
    out->endXy[1] = ((double)(c.end_cell / (uint32_t)width) + 0.5) * res + originRes[1];
    if(tsd_drive_advance(&pose, s.step[(size_t)c.speed], s.turn[(size_t)c.turn], 1, &next) != TSD_OK)
      return TSD_E_ARG;
  }
  else
  {
    out->v = out->w = 0.0;
    out->endXy[0] = out->endXy[1] = std::nan("");
  }
  out->next[0] = ((double)next.x + (double)next.fx / 65536.0) * res + originRes[0];
  out->next[1] = ((double)next.y + (double)next.fy / 65536.0) * res + originRes[1];
  out->next[2] = (double)next.heading * kTwoPi / (double)TSD_DRIVE_HEADINGS;
  return TSD_OK;
}

// The live layer's entry points are weak references too: a device library without them answers TSD_E_ARG.
#pragma weak tsd_drive_live_set
#pragma weak tsd_drive_live_clear

int liveSet(tsd_ctx* ctx, const double* originRes, const LiveRequest& live, const tsd_drive_pose* poses, size_t nPoses, int width, int height,
            int* kept)
{
  if(!tsd_drive_live_set || !tsd_drive_live_clear || !poses || nPoses > (size_t)TSD_DRIVE_LIVE_MAX_SKIP || (live.points.size() & 1u) ||
     live.points.size() > 2u * TSD_DRIVE_LIVE_MAX_POINTS || !(live.radius >= 0.0) || !(live.skipRadius >= 0.0) || !std::isfinite(live.radius) ||
     !std::isfinite(live.skipRadius))
    return TSD_E_ARG;
  const double radius = std::floor(live.radius / originRes[2] + 0.5), skipRadius = std::ceil(live.skipRadius / originRes[2]);
  if(!(radius <= (double)TSD_DRIVE_LIVE_MAX_RADIUS) || !(skipRadius <= 32768.0))
    return TSD_E_ARG;
  std::vector<int32_t> cells(live.points.size());
  for(size_t i = 0; i < live.points.size(); i++)
  {
    const double c = std::floor((live.points[i] - originRes[i & 1u]) / originRes[2]);      // (as drivePose takes a pose's cell)
    if(!(std::fabs(c) <= 1073741824.0))
      return TSD_E_ARG;                  // not finite, or beyond 1 << 30 cells
    cells[i] = static_cast<int32_t>(c);
  }
  std::vector<int32_t> skip;
  for(size_t r = 0; r < nPoses; r++)
  {
    skip.push_back(poses[r].x);
    skip.push_back(poses[r].y);
    skip.push_back(static_cast<int32_t>(skipRadius));
  }
  tsd_drive_live_params prm;
  prm.radius = static_cast<int32_t>(radius);
  prm.n_skip = static_cast<int32_t>(nPoses);
  prm.skip = skip.empty() ? nullptr : skip.data();
  return tsd_drive_live_set(ctx, &prm, cells.empty() ? nullptr : cells.data(), static_cast<int>(cells.size() / 2), width, height, kept);
}

void liveDone(tsd_ctx* ctx, const uint16_t* why, size_t nRobots, size_t samples, std::vector<int32_t>* blocked)
{
  tsd_drive_live_clear(ctx);
  blocked->assign(nRobots, 0);
  for(size_t r = 0; r < nRobots; r++)
    for(size_t i = 0; i < samples; i++)
      (*blocked)[r] += (why[r * samples + i] >> 12) == 7;
}

int ThreadGrid::exploreDrive(const tsd_route_goal& goal, const double* poseXyt, const DriveRequest& q, DriveAnswer* out, DriveSamples* samples,
                             const LiveRequest* live, LiveAnswer* liveOut)
{
  if(!tsd_drive_rollout || !tsd_drive_advance || !tsd_route_frame || !tsd_route_weights || !poseXyt || !out || !samples ||
     goal.cell == TSD_ROUTE_NONE || goal.dist == TSD_ROUTE_NONE || (live && (!liveOut || !tsd_drive_live_set || !tsd_drive_live_clear)))
    return TSD_E_ARG;
  std::lock_guard<std::mutex> lk(_publishMutex);
  if(_planStamp != _frames + _updates)
    return TSD_E_ARG;                  // no plan, or one of a map that has been published over
  double place[3];
  mapPlacement(place);
  const int W = static_cast<int>(_width), H = static_cast<int>(_height);
  if(goal.cell >= (uint32_t)W * (uint32_t)H)
    return TSD_E_ARG;
  int rc = driveSamples(place[2], q, samples);
  if(rc != TSD_OK)
    return rc;
  tsd_drive_pose pose;
  if(!drivePose(place, poseXyt, W, H, 0, &pose))
    return TSD_E_ARG;
  uint8_t weights[100];
  const int freeMax = _planSource == TSD_ROUTE_COSTMAP ? 98 : 0;
  if(tsd_route_weights(freeMax, _planSource == TSD_ROUTE_COSTMAP ? _planMaxWeight : 1, weights) != TSD_OK)
    return TSD_E_ARG;
  const int32_t seed[2] = {static_cast<int32_t>(goal.cell % (uint32_t)W), static_cast<int32_t>(goal.cell / (uint32_t)W)};
  tsd_route_params prm;
  prm.free_max = freeMax;
  prm.n_seeds = 1;
  prm.seeds_xy = seed;
  prm.weights = weights;
  prm.limit = static_cast<uint32_t>(std::min<uint64_t>(TSD_ROUTE_MAX_DIST, (uint64_t)goal.dist + q.margin));
  prm.max_rounds = 0;
  std::lock_guard<std::mutex> fl(_grid.frontierMutex());
  // the field seeded AT the goal (the navigation potential) takes the place of the plan's robot-seeded route result
  _planRouteReplaced = true;
  tsd_route_info info;
  rc = tsd_route_frame(_grid.context(), _planSource, &prm, &info);
  if(rc != TSD_OK)
    return rc;
  tsd_drive_choice choice;
  if(!live)
    rc = tsd_drive_rollout(_grid.context(), &samples->prm, &pose, 1, &choice, nullptr, nullptr);
  else
  {
    rc = liveSet(_grid.context(), place, *live, &pose, 1, W, H, &liveOut->kept);
    if(rc != TSD_OK)
      return rc;                         // (the layer before it, if any, was nobody's: none outlives a call)
    std::vector<uint16_t> why((size_t)samples->prm.n_speeds * samples->prm.n_turns, 0);
    rc = tsd_drive_rollout(_grid.context(), &samples->prm, &pose, 1, &choice, nullptr, why.data());
    liveDone(_grid.context(), why.data(), 1, why.size(), &liveOut->blocked);
  }
  if(rc != TSD_OK)
    return rc;
  return driveAnswer(*samples, place, W, pose, choice, out);
}

void ThreadGrid::mapPlacement(double* originRes)
{
  std::lock_guard<std::mutex> m(_msgMutex);
  originRes[0] = _occGrid->info.origin.position.x;
  originRes[1] = _occGrid->info.origin.position.y;
  originRes[2] = static_cast<double>(_occGrid->info.resolution);
}

int ThreadGrid::frontiers(const int32_t* seedsXy, int n, uint32_t minSize, std::vector<tsd_frontier>* out, int* seedsUsed, double* originRes)
{
  if(!out || (n > 0 && !seedsXy))
    return TSD_E_ARG;
  std::lock_guard<std::mutex> lk(_publishMutex);
  if(originRes)
    mapPlacement(originRes);
  return frameFrontiers(_grid, seedsXy, n, minSize, out, seedsUsed);
}

// The frontiers of the map just published as a cloud, one point per frontier of at least frontier_min_size cells in ascending root
// index: float32 x y z -- the centroid of the frontier's cell centres in the map's frame,
//   x = (float)(((double)sum_x / (double)size + 0.5) * (double)info.resolution + origin.x), y likewise, z = 0
// with the resolution (a float32, as a subscriber reads it) and the origin <node>/map carries -- then uint32 size and int32 min_x min_y max_x max_y (cells).  No seeds: ThreadGrid knows no poses.
int ThreadGrid::publishFrontiers(const std_msgs::msg::Header& header)
{
  std::vector<tsd_frontier> recs;
  const int rc = frameFrontiers(_grid, nullptr, 0, _frontierMinSize, &recs, nullptr);
  if(rc != TSD_OK)
    return rc;
  sensor_msgs::msg::PointCloud2 cloud;
  cloud.header = header;
  cloud.height = 1;
  cloud.width = static_cast<uint32_t>(recs.size());
  static const char* const names[8] = {"x", "y", "z", "size", "min_x", "min_y", "max_x", "max_y"};
  cloud.fields.resize(8);
  for(unsigned i = 0; i < 8; i++)
  {
    cloud.fields[i].name = names[i];
    cloud.fields[i].offset = 4 * i;
    cloud.fields[i].datatype = i < 3 ? sensor_msgs::msg::PointField::FLOAT32
                                     : (i == 3 ? sensor_msgs::msg::PointField::UINT32 : sensor_msgs::msg::PointField::INT32);
    cloud.fields[i].count = 1;
  }
  cloud.is_bigendian = false;
  cloud.point_step = 32;
  cloud.row_step = cloud.point_step * cloud.width;
  cloud.is_dense = true;
  cloud.data.resize((size_t)cloud.row_step);
  double ox, oy, res;
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    ox = _occGrid->info.origin.position.x;
    oy = _occGrid->info.origin.position.y;
    res = static_cast<double>(_occGrid->info.resolution);
  }
  for(size_t i = 0; i < recs.size(); i++)
  {
    const tsd_frontier& f = recs[i];
    const float c[3] = {static_cast<float>(((double)f.sum_x / (double)f.size + 0.5) * res + ox),
                        static_cast<float>(((double)f.sum_y / (double)f.size + 0.5) * res + oy), 0.f};
    const int32_t box[4] = {f.min_x, f.min_y, f.max_x, f.max_y};
    uint8_t* p = cloud.data.data() + i * cloud.point_step;
    std::memcpy(p, c, 12);
    std::memcpy(p + 12, &f.size, 4);
    std::memcpy(p + 16, box, 16);
  }
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    _lastFrontiers = cloud;
    _frontierClouds++;
  }
  _frontierPub->publish(cloud);
  return TSD_OK;
}

// The cost map of the map just published, from the device copy of that very frame.  mapWin == nullptr: behind a full map, a full
// nav_msgs/OccupancyGrid with the map's info and header.  Otherwise behind the update of window *mapWin: the update's window grown by
// the inflation radius (what tsd_costmap_begin recomputed and copied into _hCost, which holds the full current cost map) as a
// map_msgs/OccupancyGridUpdate.
int ThreadGrid::publishCostmap(const tsd_map_window* mapWin)
{
  const size_t cells = (size_t)_width * _height;
  if(!_hCost)
    _hCost = static_cast<int8_t*>(tsd_host_alloc(cells));
  if(!_hCost)
    return TSD_E_ARG;
  tsd_ctx* ctx = _grid.context();
  tsd_map_window out = {0, 0, 0, 0};
  int rc;
  {
    // the grid's mutex only while the call is enqueued, as for the frame
    std::lock_guard<std::mutex> g(_grid.mutex());
    rc = tsd_costmap_begin(ctx, &_costPrm, _hCost, nullptr, mapWin, &out);
  }
  if(rc != TSD_OK)
    return rc;
  rc = tsd_costmap_wait(ctx);
  if(rc != TSD_OK)
    return rc;
  if(!mapWin)
  {
    nav_msgs::msg::OccupancyGrid msg;
    {
      std::lock_guard<std::mutex> m(_msgMutex);
      msg.header = _occGrid->header;
      msg.info = _occGrid->info;
      _costmaps++;
    }
    msg.data.resize(cells);
    std::memcpy(msg.data.data(), _hCost, cells);
    _costmapPub->publish(msg);
    return TSD_OK;
  }
  if(out.width == 0 || out.height == 0 || !_costmapUpdatePub)
    return TSD_OK;
  map_msgs::msg::OccupancyGridUpdate upd;
  upd.x = out.x;
  upd.y = out.y;
  upd.width = static_cast<uint32_t>(out.width);
  upd.height = static_cast<uint32_t>(out.height);
  upd.data.resize((size_t)out.width * out.height);
  for(int32_t r = 0; r < out.height; r++)
    std::memcpy(upd.data.data() + (size_t)r * out.width, _hCost + (size_t)(out.y + r) * _width + (size_t)out.x, (size_t)out.width);
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    upd.header = _occGrid->header;
    _lastCostmapUpdate = upd;
    _costmaps++;
  }
  _costmapUpdatePub->publish(upd);
  return TSD_OK;
}

// The map's surface beside the map: calcCoords' sub-cell points (tsd_surface_extract) as float32 x y z normal_x normal_y normal_z, z =
// normal_z = 0, moved into the map's frame by the origin <node>/map carries; a point whose normal failed keeps a zero normal.  The
// header is the map's (or the update's).
int ThreadGrid::publishSurface(const std_msgs::msg::Header& header)
{
  tsd_ctx* ctx = _grid.context();
  int n = 0;
  std::vector<double> xy, nr;
  std::vector<uint8_t> ok;
  {
    // the grid's mutex for the whole extraction: the call waits for its count, and the grid must not be written meanwhile
    std::lock_guard<std::mutex> g(_grid.mutex());
    int rc = tsd_surface_extract(ctx, nullptr, &n);
    if(rc != TSD_OK)
      return rc;
    xy.resize(2 * (size_t)n + 2); nr.resize(2 * (size_t)n + 2); ok.resize((size_t)n + 1);
    rc = tsd_surface_fetch(ctx, 0, n, xy.data(), nr.data(), ok.data());
    if(rc != TSD_OK)
      return rc;
  }
  sensor_msgs::msg::PointCloud2 cloud;
  cloud.header = header;
  cloud.height = 1;
  cloud.width = static_cast<uint32_t>(n);
  static const char* const names[6] = {"x", "y", "z", "normal_x", "normal_y", "normal_z"};
  cloud.fields.resize(6);
  for(unsigned i = 0; i < 6; i++)
  {
    cloud.fields[i].name = names[i];
    cloud.fields[i].offset = 4 * i;
    cloud.fields[i].datatype = sensor_msgs::msg::PointField::FLOAT32;
    cloud.fields[i].count = 1;
  }
  cloud.is_bigendian = false;
  cloud.point_step = 24;
  cloud.row_step = cloud.point_step * cloud.width;
  cloud.is_dense = true;
  cloud.data.resize((size_t)cloud.row_step);
  double ox, oy;
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    ox = _occGrid->info.origin.position.x;
    oy = _occGrid->info.origin.position.y;
  }
  for(int i = 0; i < n; i++)
  {
    const float p[6] = {static_cast<float>(xy[2 * (size_t)i] + ox), static_cast<float>(xy[2 * (size_t)i + 1] + oy), 0.f,
                        ok[(size_t)i] ? static_cast<float>(nr[2 * (size_t)i]) : 0.f, ok[(size_t)i] ? static_cast<float>(nr[2 * (size_t)i + 1]) : 0.f, 0.f};
    std::memcpy(cloud.data.data() + (size_t)i * cloud.point_step, p, sizeof(p));
  }
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    _lastSurface = cloud;
    _surfaces++;
  }
  _surfacePub->publish(cloud);
  return TSD_OK;
}

// a windowed frame: _hOcc / _hRgb hold the full current frame, of which the window's rows are new
int ThreadGrid::publishUpdate(const tsd_map_window& win)
{
  map_msgs::msg::OccupancyGridUpdate upd;
  upd.x = win.x;
  upd.y = win.y;
  upd.width = static_cast<uint32_t>(win.width);
  upd.height = static_cast<uint32_t>(win.height);
  upd.data.resize((size_t)win.width * win.height);
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    _occGrid->header.stamp = _node->get_clock()->now();
    upd.header = _occGrid->header;
    for(int32_t r = 0; r < win.height; r++)
    {
      const size_t o = (size_t)(win.y + r) * _width + (size_t)win.x;
      std::memcpy(_occGrid->data.data() + o, _hOcc + o, (size_t)win.width);
      std::memcpy(upd.data.data() + (size_t)r * win.width, _hOcc + o, (size_t)win.width);
    }
    _lastUpdate = upd;
    _updates++;
  }
  _updatePub->publish(upd);
  // the image stays a full message (ThreadGrid.cpp:120-131), patched by the window's rows
  _image.header.stamp = upd.header.stamp;
  _image.height = _height;
  _image.width = _width;
  _image.encoding = sensor_msgs::image_encodings::RGB8;
  for(int32_t r = 0; r < win.height; r++)
  {
    const size_t o = 3 * ((size_t)(win.y + r) * _width + (size_t)win.x);
    std::memcpy(_image.data.data() + o, _hRgb + o, 3 * (size_t)win.width);
  }
  _pubColorImage->publish(_image);
  return TSD_OK;
}

bool ThreadGrid::getMapServCallBack(const std::shared_ptr<nav_msgs::srv::GetMap::Request>,
                                    std::shared_ptr<nav_msgs::srv::GetMap::Response> res)
{
  std::lock_guard<std::mutex> m(_msgMutex);
  res->map = *_occGrid;
  res->map.header.stamp = _node->get_clock()->now();
  _occGrid->info.map_load_time = _node->get_clock()->now();
  return true;
}

} /* namespace ohm_tsd_slam */
