#include "ThreadGridGroup.h"
#include "ThreadGrid.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace ohm_tsd_slam
{

bool ThreadGridGroup::cellOffset(double origin, double originRef, double cellSize, int32_t* cells)
{
  const double d = (origin - originRef) / cellSize;
  const double r = std::round(d);
  if(!(std::fabs(d - r) <= 1e-6) || std::fabs(r) > 16777216.0)
    return false;
  *cells = static_cast<int32_t>(r);
  return true;
}

static double mapOrigin(obvious::TsdGrid* grid, unsigned int cells, double offset)
{
  // (ThreadGrid.cpp:28-29)
  return -(static_cast<double>(cells) * static_cast<double>(grid->getCellSize()) * 0.5 + offset);
}

ThreadGridGroup::ThreadGridGroup(const std::shared_ptr<rclcpp::Node>& node, const std::vector<Member>& members):
    ThreadSLAM(*members.at(0).grid),
    _node(node),
    _members(members),
    _group(nullptr),
    _occGrid(std::make_shared<nav_msgs::msg::OccupancyGrid>()),
    _width(0),
    _height(0),
    _hOcc(nullptr),
    _frames(0),
    _planFrames(0)
{
  const double cs = static_cast<double>(_grid.getCellSize());
  // the merged window's origin is the smallest origin along each axis; every grid lies a whole number of cells from grid 0
  std::vector<int32_t> off(2 * _members.size());
  std::vector<tsd_ctx*> ctxs(_members.size());
  const double ox0 = mapOrigin(_members[0].grid, _members[0].grid->getCellsX(), _members[0].xOffset);
  const double oy0 = mapOrigin(_members[0].grid, _members[0].grid->getCellsY(), _members[0].yOffset);
  double originX = ox0, originY = oy0;
  for(size_t i = 0; i < _members.size(); i++)
  {
    obvious::TsdGrid* g = _members[i].grid;
    ctxs[i] = g->context();
    const double ox = mapOrigin(g, g->getCellsX(), _members[i].xOffset), oy = mapOrigin(g, g->getCellsY(), _members[i].yOffset);
    if(!cellOffset(ox, ox0, cs, &off[2 * i]) || !cellOffset(oy, oy0, cs, &off[2 * i + 1]))
    {
      char text[256];
      std::snprintf(text, sizeof(text), "ThreadGridGroup: the map origins of grid 0 (%.9g, %.9g) and grid %zu (%.9g, %.9g) do not differ by "
                    "whole cells of %.9g m", ox0, oy0, i, ox, oy, cs);
      throw std::invalid_argument(text);
    }
    if(ox < originX) originX = ox;
    if(oy < originY) originY = oy;
  }
  _group = tsd_group_create(static_cast<int>(_members.size()), ctxs.data(), off.data(), 0, 0);
  if(!_group)
    throw std::invalid_argument("ThreadGridGroup: the device refused the group (one device, one cell size, at most 64 grids)");
  _width = static_cast<unsigned int>(tsd_group_width(_group));
  _height = static_cast<unsigned int>(tsd_group_height(_group));

  _occGrid->info.resolution           = cs;
  _occGrid->info.width                = _width;
  _occGrid->info.height               = _height;
  _occGrid->info.origin.orientation.w = 1.0;
  _occGrid->info.origin.orientation.x = 0.0;
  _occGrid->info.origin.orientation.y = 0.0;
  _occGrid->info.origin.orientation.z = 0.0;
  _occGrid->info.origin.position.x    = originX;
  _occGrid->info.origin.position.y    = originY;
  _occGrid->info.origin.position.z    = 0.0;
  _occGrid->data.resize((size_t)_width * _height);

  _occGrid->header.frame_id = node->get_parameter("tf_map_frame").as_string();
  _objectInflation = node->get_parameter("use_object_inflation").as_bool();
  _objInflateFactor = static_cast<unsigned int>(node->get_parameter("object_inflation_factor").as_int());

  const std::string node_name = _node->get_name();
  _gridPub = node->create_publisher<nav_msgs::msg::OccupancyGrid>(node_name + "/merged_map", rclcpp::QoS(1).reliable().transient_local());
  _getMapServ = node->create_service<nav_msgs::srv::GetMap>(
    node_name + "/get_merged_map",
    std::bind(&ThreadGridGroup::getMapServCallBack, this, std::placeholders::_1, std::placeholders::_2));
  startThread();
}

ThreadGridGroup::~ThreadGridGroup()
{
  terminateThread();
  joinThread();
  tsd_group_destroy(_group);
  tsd_host_free(_hOcc);
}

uint64_t ThreadGridGroup::frames(void)
{
  std::lock_guard<std::mutex> lk(_msgMutex);
  return _frames;
}

void ThreadGridGroup::eventLoop(void)
{
  while(_stayActive)
  {
    waitForWork();
    if(!_stayActive)
      break;
    publish();
  }
}

int ThreadGridGroup::publish(void)
{
  std::lock_guard<std::mutex> lk(_publishMutex);
  const size_t cells = (size_t)_width * _height;
  if(!_hOcc)
    _hOcc = static_cast<int8_t*>(tsd_host_alloc(cells));
  if(!_hOcc)
    return TSD_E_ARG;
  tsd_map_params prm;
  prm.inflate = _objectInflation ? 1 : 0;
  prm.inflate_factor = static_cast<int32_t>(_objInflateFactor);
  for(size_t i = 0; i < _members.size(); i++)
  {
    // one grid's mutex at a time, and only while that grid's extraction is enqueued: the localisers go on while the maps are merged
    std::lock_guard<std::mutex> g(_members[i].grid->mutex());
    const int rc = tsd_group_extract_begin(_group, static_cast<int>(i), &prm);
    if(rc != TSD_OK)
      return rc;
  }
  int rc = tsd_group_merge_maps_begin(_group, nullptr, _hOcc);
  if(rc != TSD_OK)
    return rc;
  rc = tsd_group_merge_wait(_group, nullptr);
  if(rc != TSD_OK)
    return rc;
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
  return TSD_OK;
}

int ThreadGridGroup::frontiers(const double* gridXy, uint32_t minSize, std::vector<tsd_frontier>* out, int* seedsUsed, int32_t* seedsXy,
                               double* originCs)
{
  return frontiersAndPlan(gridXy, minSize, out, seedsUsed, seedsXy, originCs, nullptr, 0);
}

int ThreadGridGroup::explorePlan(const double* gridXy, uint32_t minSize, int maxLen, ExplorePlan* out, int32_t* seedsXy, double* originCs)
{
  if(!out || maxLen < 1)
    return TSD_E_ARG;
  return frontiersAndPlan(gridXy, minSize, &out->frontiers, &out->seedsUsed, seedsXy, originCs, out, maxLen);
}

// frontiers(); with `plan` also the routes from the same seeds on the same map (unit weights, free_max 0), under the same two locks:
// the goals read the frontier result
int ThreadGridGroup::frontiersAndPlan(const double* gridXy, uint32_t minSize, std::vector<tsd_frontier>* out, int* seedsUsed, int32_t* seedsXy,
                                      double* originCs, ExplorePlan* plan, int maxLen, ExploreDispatch* dispatch)
{
  if(!gridXy || !out || _members.size() > (size_t)TSD_FRONTIER_MAX_SEEDS)
    return TSD_E_ARG;
  std::lock_guard<std::mutex> lk(_publishMutex);      // (the merged map on the device stays as the last publication left it)
  const double cs = static_cast<double>(_grid.getCellSize());
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    if(_frames == 0)
      return TSD_E_ARG;
    if(originCs)
    {
      originCs[0] = _occGrid->info.origin.position.x;
      originCs[1] = _occGrid->info.origin.position.y;
      originCs[2] = static_cast<double>(_occGrid->info.resolution);
    }
  }
  int32_t x0 = 0, y0 = 0;
  if(tsd_group_corner(_group, &x0, &y0) != TSD_OK)
    return TSD_E_ARG;
  std::vector<int32_t> seeds(2 * _members.size(), -1);
  for(size_t i = 0; i < _members.size(); i++)
  {
    double T[9];
    if(tsd_group_member_transform(_group, static_cast<int>(i), T) != TSD_OK)
      return TSD_E_ARG;
    const double x = gridXy[2 * i], y = gridXy[2 * i + 1];
    const double fx = std::floor((T[0] * x + T[1] * y + T[2]) / cs) - (double)x0, fy = std::floor((T[3] * x + T[4] * y + T[5]) / cs) - (double)y0;
    if(fx >= 0.0 && fx < (double)_width && fy >= 0.0 && fy < (double)_height)       // (false for a NaN)
    {
      seeds[2 * i] = static_cast<int32_t>(fx);
      seeds[2 * i + 1] = static_cast<int32_t>(fy);
    }
  }
  if(seedsXy)
    std::memcpy(seedsXy, seeds.data(), seeds.size() * sizeof(int32_t));
  tsd_frontier_params prm;
  prm.free_max = 0;
  prm.min_size = minSize < 1u ? 1u : minSize;
  prm.n_seeds = static_cast<int32_t>(_members.size());
  prm.reserved = 0;
  prm.seeds_xy = seeds.data();
  int count = 0, used = 0, rc;
  {
    // member 0's context and stream carry the call: its frontierMutex, because that context's frontier scratch also serves member
    // 0's own ThreadGrid (whose frame-form calls do not take the grid's mutex), then its grid's mutex, as for every call on that stream
    std::lock_guard<std::mutex> fl(_members[0].grid->frontierMutex());
    std::lock_guard<std::mutex> g(_members[0].grid->mutex());
    tsd_ctx* ctx = _members[0].grid->context();
    rc = tsd_frontiers_dev(ctx, tsd_group_map_dev(_group), static_cast<int>(_width), static_cast<int>(_height), static_cast<int>(_width),
                           &prm, &count, &used);
    if(rc == TSD_OK)
    {
      out->resize((size_t)count);
      if(count > 0)
        rc = tsd_frontiers_fetch(ctx, 0, count, out->data());
    }
    if(rc == TSD_OK && plan)
    {
      tsd_route_params rp;
      rp.free_max = 0;
      rp.n_seeds = prm.n_seeds;
      rp.seeds_xy = seeds.data();
      rp.weights = nullptr;
      rp.limit = 0;
      rp.max_rounds = 0;
      rc = routePlan(ctx, tsd_group_map_dev(_group), static_cast<int>(_width), static_cast<int>(_height), TSD_ROUTE_MAP, rp, maxLen, plan);
    }
    if(rc == TSD_OK && dispatch)
      rc = dispatchLocked(ctx, seeds, dispatch);
  }
  if(dispatch)
    dispatch->frames = rc == TSD_OK ? _frames : 0;
  if(seedsUsed)
    *seedsUsed = used;
  if(plan)
    _planFrames = rc == TSD_OK ? _frames : 0;
  return rc;
}

#pragma weak tsd_route_fields_dev
#pragma weak tsd_route_fields_goals
#pragma weak tsd_route_fields_goals_fetch
#pragma weak tsd_route_fields_waypoints
#pragma weak tsd_view_assign_fields

int ThreadGridGroup::exploreDispatch(const double* gridXy, uint32_t minSize, ExploreDispatch* d, int32_t* seedsXy, double* originCs)
{
  if(!tsd_route_fields_dev || !tsd_route_fields_goals || !tsd_route_fields_goals_fetch || !tsd_route_fields_waypoints || !tsd_view_assign_fields ||
     !d || d->unknownDepth < 0 || d->maxLen < 1 || d->maxWay < 1)
    return TSD_E_ARG;
  return frontiersAndPlan(gridXy, minSize, &d->frontiers, &d->seedsUsed, seedsXy, originCs, nullptr, 0, d);
}

// exploreDispatch behind the frontiers, on the same context and under the same locks: fields, matrix, assignment, waypoints
int ThreadGridGroup::dispatchLocked(tsd_ctx* ctx, const std::vector<int32_t>& seeds, ExploreDispatch* d)
{
  const int L = static_cast<int>(_members.size()), W = static_cast<int>(_width), H = static_cast<int>(_height);
  const double cs = static_cast<double>(_grid.getCellSize());
  if(d->frontiers.size() > (size_t)TSD_VIEW_MAX_CELLS)
    return TSD_E_ARG;
  tsd_route_params rp;
  rp.free_max = 0;
  rp.n_seeds = L;
  rp.seeds_xy = seeds.data();
  rp.weights = nullptr;
  rp.limit = 0;
  rp.max_rounds = 0;
  int rc = tsd_route_fields_dev(ctx, tsd_group_map_dev(_group), W, H, W, &rp, &d->fields);
  if(rc != TSD_OK)
    return rc;
  int n = 0;
  rc = tsd_route_fields_goals(ctx, &n);
  if(rc != TSD_OK)
    return rc;
  d->goals.assign((size_t)L * n, tsd_route_goal{TSD_ROUTE_NONE, TSD_ROUTE_NONE, -1, 0u});
  for(int r = 0; r < L && n > 0; r++)
    if((rc = tsd_route_fields_goals_fetch(ctx, r, 0, n, d->goals.data() + (size_t)r * n)) != TSD_OK)
      return rc;
  tsd_view_params vp;
  vp.free_max = 0;
  vp.radius = viewRadiusCells(d->viewRadius, cs);
  vp.unknown_depth = d->unknownDepth;
  vp.use_claims = 0;
  d->radiusCells = vp.radius;
  d->goalOfRobot.assign((size_t)L, -1);
  d->picked.assign((size_t)L, tsd_view_gain{TSD_ROUTE_NONE, 0u, 0u, 0u});
  rc = tsd_view_assign_fields(ctx, tsd_group_map_dev(_group), W, H, W, &vp, d->goals.data(), n, L, d->gainWeight, d->goalOfRobot.data(),
                              d->picked.data(), &d->rounds);
  if(rc != TSD_OK)
    return rc;
  tsd_waypoint_params wp;
  wp.lookahead = waypointLookaheadCells(d->lookahead, cs);
  wp.slack = d->slack;
  wp.max_len = d->maxLen;
  wp.max_way = d->maxWay;
  d->lookaheadCells = wp.lookahead;
  d->way.assign((size_t)L * d->maxWay, 0u);
  d->wayInfo.assign((size_t)L, tsd_waypoint_info{0, 0, 0u, TSD_ROUTE_NONE});
  // the members with a goal, each on its own layer, in one call
  std::vector<uint32_t> cells, way;
  std::vector<uint8_t> layers;
  for(int r = 0; r < L; r++)
    if(d->goalOfRobot[r] >= 0)
    {
      cells.push_back(d->goals[(size_t)r * n + d->goalOfRobot[r]].cell);
      layers.push_back(static_cast<uint8_t>(r));
    }
  if(cells.empty())
    return TSD_OK;
  way.assign(cells.size() * d->maxWay, 0u);
  std::vector<tsd_waypoint_info> info(cells.size());
  rc = tsd_route_fields_waypoints(ctx, cells.data(), layers.data(), static_cast<int>(cells.size()), &wp, way.data(), info.data());
  if(rc != TSD_OK)
    return rc;
  for(size_t k = 0; k < cells.size(); k++)
  {
    d->wayInfo[layers[k]] = info[k];
    std::memcpy(d->way.data() + (size_t)layers[k] * d->maxWay, way.data() + k * d->maxWay, (size_t)d->maxWay * sizeof(uint32_t));
  }
  return TSD_OK;
}

#pragma weak tsd_drive_fields_rollout
#pragma weak tsd_drive_fleet_rollout
#pragma weak tsd_drive_fields_togo
#pragma weak tsd_drive_live_set
#pragma weak tsd_drive_live_clear

int ThreadGridGroup::exploreDrive(const ExploreDispatch& d, const double* posesXyt, const DriveRequest& q, DriveAnswer* out, DriveSamples* samples,
                                  const FleetDriveRequest* fleet, FleetDriveAnswer* fleetOut, const LiveRequest* live, LiveAnswer* liveOut)
{
  const size_t L = _members.size();
  if(!tsd_drive_fields_rollout || !tsd_route_fields_dev || !posesXyt || !out || !samples || L < 1 || L > (size_t)TSD_DRIVE_MAX_ROBOTS ||
     d.goalOfRobot.size() != L)
    return TSD_E_ARG;
  const bool apart = fleet && fleet->separation > 0.0;
  if(apart && (!tsd_drive_fleet_rollout || !tsd_drive_fields_togo || !fleetOut || !std::isfinite(fleet->separation) ||
               (!fleet->priority.empty() && fleet->priority.size() != L)))
    return TSD_E_ARG;
  if(live && (!liveOut || !tsd_drive_live_set || !tsd_drive_live_clear))
    return TSD_E_ARG;
  std::lock_guard<std::mutex> lk(_publishMutex);
  if(d.frames == 0 || d.frames != _frames)
    return TSD_E_ARG;                  // no dispatch, or one of a merged map that has been published over
  double place[3];
  {
    std::lock_guard<std::mutex> m(_msgMutex);
    place[0] = _occGrid->info.origin.position.x;
    place[1] = _occGrid->info.origin.position.y;
    place[2] = static_cast<double>(_occGrid->info.resolution);
  }
  const int W = static_cast<int>(_width), H = static_cast<int>(_height);
  int rc = driveSamples(place[2], q, samples);
  if(rc != TSD_OK)
    return rc;
  const size_t n = d.goals.size() / L;
  std::vector<int32_t> seeds(2 * L, -1);
  std::vector<tsd_drive_pose> poses(L);
  uint32_t far = 0;
  for(size_t r = 0; r < L; r++)
  {
    if(!drivePose(place, posesXyt + 3 * r, W, H, static_cast<int>(r), &poses[r]))
      return TSD_E_ARG;
    if(d.goalOfRobot[r] < 0 || (size_t)d.goalOfRobot[r] >= n)
      continue;
    const tsd_route_goal& g = d.goals[r * n + (size_t)d.goalOfRobot[r]];
    if(g.cell == TSD_ROUTE_NONE || g.cell >= (uint32_t)W * (uint32_t)H)
      continue;
    seeds[2 * r] = static_cast<int32_t>(g.cell % (uint32_t)W);
    seeds[2 * r + 1] = static_cast<int32_t>(g.cell / (uint32_t)W);
    far = std::max(far, g.dist);
  }
  tsd_route_params rp;
  rp.free_max = 0;
  rp.n_seeds = static_cast<int32_t>(L);
  rp.seeds_xy = seeds.data();
  rp.weights = nullptr;
  rp.limit = static_cast<uint32_t>(std::min<uint64_t>(TSD_ROUTE_MAX_DIST, (uint64_t)far + q.margin));
  rp.max_rounds = 0;
  std::vector<tsd_drive_choice> choice(L);
  tsd_drive_fleet_params fp;
  std::vector<int32_t> order;
  std::vector<uint16_t> why;
  std::vector<int64_t> tracks;
  const size_t S = (size_t)samples->prm.n_speeds * samples->prm.n_turns, T1 = (size_t)samples->prm.steps + 1;
  if(apart)
  {
    const double sep = std::floor(fleet->separation / place[2] * 65536.0 + 0.5);
    if(!(sep <= (double)TSD_DRIVE_MAX_SEP))
      return TSD_E_ARG;
    fp.sep_q16 = static_cast<int32_t>(sep);
    fp.reserved = 0;
    order = fleet->priority;
    std::vector<bool> seen(L, false);
    for(const int32_t r : order)
    {
      if(r < 0 || (size_t)r >= L || seen[(size_t)r])
        return TSD_E_ARG;
      seen[(size_t)r] = true;
    }
    for(size_t r = 0; r < L; r++)
      if(seeds[2 * r] < 0)
        poses[r].layer = -1;             // no goal: parked where it stands
    tracks.resize(L * T1 * 2);
  }
  if(apart || live)
    why.resize(L * S);
  {
    // as for the dispatch: member 0's context and stream carry the call
    std::lock_guard<std::mutex> fl(_members[0].grid->frontierMutex());
    std::lock_guard<std::mutex> g(_members[0].grid->mutex());
    tsd_ctx* ctx = _members[0].grid->context();
    tsd_route_fields_info info;
    // layer r seeded AT member r's goal: this replaces the dispatch's robot-seeded fields result, whose answers have been fetched
    rc = tsd_route_fields_dev(ctx, tsd_group_map_dev(_group), W, H, W, &rp, &info);
    bool layer = false;                  // the live layer stands: it goes before the locks do
    if(rc == TSD_OK && live)
    {
      rc = liveSet(ctx, place, *live, poses.data(), L, W, H, &liveOut->kept);
      layer = rc == TSD_OK;
    }
    if(rc == TSD_OK && !apart)
      rc = tsd_drive_fields_rollout(ctx, &samples->prm, poses.data(), static_cast<int>(L), choice.data(), nullptr, live ? why.data() : nullptr);
    if(rc == TSD_OK && apart && order.empty())
    {
      // the cost-to-go of each member at its pose, from its own layer, in one round trip: 0xFFFFFFFF (no key, or no goal) sorts
      // last.  Two members' keys never tie -- the low bits of layer r's keys hold the seed index r --, so equal cost goes to the lower
      // index by the keys themselves; the stable sort settles the members without a key.
      std::vector<uint32_t> togo(L, TSD_ROUTE_NONE);
      rc = tsd_drive_fields_togo(ctx, poses.data(), static_cast<int>(L), togo.data());
      order.resize(L);
      for(size_t r = 0; r < L; r++)
        order[r] = static_cast<int32_t>(r);
      std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return togo[(size_t)a] < togo[(size_t)b]; });
    }
    if(rc == TSD_OK && apart)
    {
      fp.order = order.data();
      rc = tsd_drive_fleet_rollout(ctx, &samples->prm, &fp, poses.data(), static_cast<int>(L), choice.data(), nullptr, why.data(), tracks.data());
    }
    if(layer)
      liveDone(ctx, why.data(), L, S, &liveOut->blocked);
  }
  for(size_t r = 0; r < L && rc == TSD_OK; r++)
    rc = driveAnswer(*samples, place, W, poses[r], choice[r], out + r);
  if(rc == TSD_OK && apart)
  {
    fleetOut->order = order;
    fleetOut->steps = samples->prm.steps;
    fleetOut->blocked.assign(L, 0);
    for(size_t r = 0; r < L; r++)
      for(size_t i = 0; i < S; i++)
        fleetOut->blocked[r] += (why[r * S + i] >> 12) == 6;
    fleetOut->tracks.resize(L * T1 * 2);
    for(size_t i = 0; i < L * T1; i++)
      for(size_t a = 0; a < 2; a++)
        fleetOut->tracks[2 * i + a] = static_cast<double>(tracks[2 * i + a]) / 65536.0 * place[2] + place[a];
  }
  return rc;
}

#pragma weak tsd_view_assign

int ThreadGridGroup::exploreAssign(const tsd_route_goal* goals, size_t n, double viewRadius, uint32_t gainWeight, int unknownDepth,
                                   int32_t* goalOfRobot, tsd_view_gain* picked, int* rounds, int* radiusCells)
{
  if(!tsd_view_assign || (n > 0 && !goals) || n > (size_t)TSD_VIEW_MAX_CELLS || !goalOfRobot || !rounds || unknownDepth < 0 ||
     _members.size() > (size_t)TSD_FRONTIER_MAX_SEEDS)
    return TSD_E_ARG;
  std::lock_guard<std::mutex> lk(_publishMutex);
  if(_planFrames == 0 || _planFrames != _frames)
    return TSD_E_ARG;                  // no plan, or one of a merged map that has been published over
  tsd_view_params prm;
  prm.free_max = 0;
  prm.radius = viewRadiusCells(viewRadius, static_cast<double>(_grid.getCellSize()));
  prm.unknown_depth = unknownDepth;
  prm.use_claims = 0;
  if(radiusCells)
    *radiusCells = prm.radius;
  // as for the plan: member 0's context and stream carry the call
  std::lock_guard<std::mutex> fl(_members[0].grid->frontierMutex());
  std::lock_guard<std::mutex> g(_members[0].grid->mutex());
  return tsd_view_assign(_members[0].grid->context(), tsd_group_map_dev(_group), static_cast<int>(_width), static_cast<int>(_height),
                         static_cast<int>(_width), &prm, goals, static_cast<int>(n), static_cast<int>(_members.size()), gainWeight, goalOfRobot,
                         picked, rounds);
}

int ThreadGridGroup::exploreWaypoints(const tsd_route_goal* goals, size_t n, double lookahead, uint32_t slack, int maxLen, int maxWay,
                                      uint32_t* way, tsd_waypoint_info* info, int* lookaheadCells)
{
  std::lock_guard<std::mutex> lk(_publishMutex);
  if(_planFrames == 0 || _planFrames != _frames)
    return TSD_E_ARG;                  // no plan, or one of a merged map that has been published over
  tsd_waypoint_params prm;
  prm.lookahead = waypointLookaheadCells(lookahead, static_cast<double>(_grid.getCellSize()));
  prm.slack = slack;
  prm.max_len = maxLen;
  prm.max_way = maxWay;
  if(lookaheadCells)
    *lookaheadCells = prm.lookahead;
  // as for the plan: member 0's context and stream carry the call
  std::lock_guard<std::mutex> fl(_members[0].grid->frontierMutex());
  std::lock_guard<std::mutex> g(_members[0].grid->mutex());
  return routeWaypoints(_members[0].grid->context(), goals, n, prm, way, info);
}

int ThreadGridGroup::fuse(obvious::TsdGrid* dst)
{
  if(!dst || !dst->valid())
    return TSD_E_ARG;
  std::vector<int32_t> cellOff(2 * _members.size());
  {
    // (setTransforms may replace the group between two calls)
    std::lock_guard<std::mutex> lk(_publishMutex);
    if(tsd_group_cell_offsets(_group, cellOff.data()) != TSD_OK)
      return TSD_E_ARG;           // a member is rotated or lies a fraction of a cell off: the TSD-level fusion shifts by whole cells
  }
  std::vector<tsd_ctx*> ctxs(_members.size());
  for(size_t i = 0; i < _members.size(); i++)
  {
    if(_members[i].grid == dst)
      return TSD_E_ARG;
    ctxs[i] = _members[i].grid->context();
  }
  int rc;
  {
    // every grid involved, and only while the fusion is enqueued: the localisers go on while it runs
    std::vector<std::unique_lock<std::mutex>> held;
    held.reserve(_members.size() + 1);
    for(size_t i = 0; i < _members.size(); i++)
      held.emplace_back(_members[i].grid->mutex());
    held.emplace_back(dst->mutex());
    rc = tsd_fuse_begin(dst->context(), static_cast<int>(ctxs.size()), ctxs.data(), cellOff.data());
  }
  if(rc != TSD_OK)
    return rc;
  std::lock_guard<std::mutex> g(dst->mutex());
  return tsd_fuse_wait(dst->context(), nullptr);
}

void ThreadGridGroup::setTransforms(const std::vector<std::array<double, 9>>& T)
{
  if(T.size() != _members.size())
    throw std::invalid_argument("ThreadGridGroup::setTransforms: one transform per grid");
  static const std::array<double, 9> identity = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  if(T[0] != identity)
    throw std::invalid_argument("ThreadGridGroup::setTransforms: T[0] must be the identity (the frame is grid 0's)");
  const double cs = static_cast<double>(_grid.getCellSize());
  std::vector<tsd_ctx*> ctxs(_members.size());
  std::vector<double> flat;
  for(size_t i = 0; i < _members.size(); i++)
  {
    ctxs[i] = _members[i].grid->context();
    flat.insert(flat.end(), T[i].begin(), T[i].end());
  }
  std::lock_guard<std::mutex> lk(_publishMutex);
  tsd_group* group = tsd_group_create_rigid(static_cast<int>(ctxs.size()), ctxs.data(), flat.data(), 0, 0);
  if(!group)
    throw std::invalid_argument("ThreadGridGroup::setTransforms: the device refused the transforms (rigid, finite, within 65536 cells)");
  tsd_group_destroy(_group);
  _group = group;
  _planFrames = 0;               // (a plan's cells are those of the window that goes)
  if(_hOcc)
    tsd_host_free(_hOcc);
  _hOcc = nullptr;               // (publish() allocates the landing buffer for the new window)
  _width = static_cast<unsigned int>(tsd_group_width(_group));
  _height = static_cast<unsigned int>(tsd_group_height(_group));
  int32_t x0 = 0, y0 = 0;
  tsd_group_corner(_group, &x0, &y0);
  std::lock_guard<std::mutex> m(_msgMutex);
  _occGrid->info.width             = _width;
  _occGrid->info.height            = _height;
  _occGrid->info.origin.position.x = mapOrigin(_members[0].grid, _members[0].grid->getCellsX(), _members[0].xOffset) + static_cast<double>(x0) * cs;
  _occGrid->info.origin.position.y = mapOrigin(_members[0].grid, _members[0].grid->getCellsY(), _members[0].yOffset) + static_cast<double>(y0) * cs;
  _occGrid->data.assign((size_t)_width * _height, -1);
}

bool ThreadGridGroup::getMapServCallBack(const std::shared_ptr<nav_msgs::srv::GetMap::Request>,
                                         std::shared_ptr<nav_msgs::srv::GetMap::Response> res)
{
  std::lock_guard<std::mutex> m(_msgMutex);
  res->map = *_occGrid;
  res->map.header.stamp = _node->get_clock()->now();
  _occGrid->info.map_load_time = _node->get_clock()->now();
  return true;
}

} /* namespace ohm_tsd_slam */
