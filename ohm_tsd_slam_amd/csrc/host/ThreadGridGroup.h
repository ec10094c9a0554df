// ThreadGridGroup.h -- the merged-map worker of several grids on ONE GPU (not in the reference, whose robots share one TsdGrid): every
// wake-up extracts each grid's occupancy map on that grid's own stream, merges them on the device (tsd_group_*: the signed maximum,
// each grid shifted by the whole-cell difference of the map origins) and publishes one nav_msgs/OccupancyGrid on <node>/merged_map;
// <node>/get_merged_map answers with the last one.  setTransforms() places the grids by rigid transforms instead (tsd_group_create_rigid):
// grids turned against each other or a fraction of a cell apart.  Across GPUs the merge is include/tsd_comm.h's; this one never maps RCCL.
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ThreadSLAM.h"
#include "ros_shim.h"

namespace ohm_tsd_slam
{

struct ExplorePlan;      // ThreadGrid.h
struct DriveRequest;
struct DriveSamples;
struct DriveAnswer;
struct LiveRequest;
struct LiveAnswer;

/** What ThreadGridGroup::exploreDrive is asked beside the DriveRequest where the members have to keep off each other, and what it
 *  answers beside the DriveAnswers. */
struct FleetDriveRequest
{
  double separation = 0.0;             // [m] centre to centre; 0: every member is rolled out as if it were alone on the map
  std::vector<int32_t> priority;       // a permutation of the members' indices, the first decides first; empty: see exploreDrive
};
struct FleetDriveAnswer
{
  std::vector<int32_t> order;          // the priority used
  std::vector<int32_t> blocked;        // per member: the samples refused because of another member's arc (reason 6)
  std::vector<double> tracks;          // per member T + 1 pairs (x, y) [m]: the chosen arc step by step, the pose itself without one
  int steps = 0;                       // T
};

/** What ThreadGridGroup::exploreDispatch is asked and what it answers. */
struct ExploreDispatch
{
  // the request
  double viewRadius = 0.0, lookahead = 0.0;  // [m]
  uint32_t gainWeight = 0, slack = 0;
  int unknownDepth = 0, maxLen = 4096, maxWay = 256;
  // the answer
  std::vector<tsd_frontier> frontiers;
  int seedsUsed = 0;
  tsd_route_fields_info fields = {};
  std::vector<tsd_route_goal> goals;         // the matrix, [member * frontiers + frontier]
  std::vector<int32_t> goalOfRobot;          // per member a frontier index, -1: none
  std::vector<tsd_view_gain> picked;
  int rounds = 0, radiusCells = 0, lookaheadCells = 0;
  std::vector<uint32_t> way;                 // [member * maxWay + i]
  std::vector<tsd_waypoint_info> wayInfo;    // per member
  uint64_t frames = 0;                       // the publication it was made on (0: none)
};

class ThreadGridGroup : public ThreadSLAM
{
public:
  struct Member
  {
    obvious::TsdGrid* grid;
    double xOffset;       // the grid's x_offset / y_offset: its map origin is -(W / 2 + offset) (ThreadGrid.cpp:28-29)
    double yOffset;
  };

  /** whole-cell offset of a map at `origin` relative to one at `originRef`; false unless within 1e-6 cells of an integer */
  static bool cellOffset(double origin, double originRef, double cellSize, int32_t* cells);

  /** throws std::invalid_argument when two grids' origins do not differ by whole cells (the message names them) or the device
   *  refuses the group */
  ThreadGridGroup(const std::shared_ptr<rclcpp::Node>& node, const std::vector<Member>& members);
  virtual ~ThreadGridGroup();

  /** one merge and publication on the caller's thread, what every wake-up of the event loop does.  TSD_OK or the error code. */
  int publish(void);
  /** merged maps published so far */
  uint64_t frames(void);

  /** TSD-level fusion of the members' grids into `dst` (tsd_fuse_*), on the caller's thread: `dst` lies where grid 0 lies and
   *  member i is shifted by the whole-cell offset the group holds for it (the occupancy merge's own placement).  `dst`
   *  (same cell size and truncation as the members, not one of them) is an ordinary grid afterwards.  The fusion must not run
   *  beside a grid write of a member enqueued in between, so the mutexes of ALL grids involved are held while it is enqueued -- in
   *  member order, then dst's; nothing else holds two grids -- and none of the members' while it runs.  TSD_OK or the error code. */
  int fuse(obvious::TsdGrid* dst);

  /** Places the members by rigid transforms instead of the whole-cell distances of their map origins: T[i] (3x3 row-major) carries
   *  member i's grid coordinates into member 0's, what tsd_map_align(grid 0, grid i) returns; T[0] must be the identity.  The group
   *  is replaced by a rigid one (tsd_group_create_rigid, bounding box) between two publications; the merged map's origin becomes
   *  member 0's map origin plus the window's corner, its orientation stays the identity.  fuse() asks the group for the members'
   *  whole-cell offsets (tsd_group_cell_offsets) and returns TSD_E_ARG where it has none: a member turned or a fraction of a cell off.
   *  Throws std::invalid_argument (the group stays as it was) on a wrong count, a T[0] other than the identity or a transform the
   *  device library refuses. */
  void setTransforms(const std::vector<std::array<double, 9>>& T);

  /** The frontiers of the merged map published last (tsd_frontiers_dev on the group's device map, on member 0's context), with one
   *  seed per member: gridXy[2i], gridXy[2i + 1] is member i's current position in ITS grid's coordinates [m] (NaN: no pose yet, the
   *  seed lies outside the map), carried into the merged map by the group's placement -- tsd_group_member_transform, then
   *  floor(. / cell size) minus the window's corner (tsd_group_corner).  out: the records of at least minSize cells in ascending root
   *  index (member 0's frontierMutex and grid mutex are held from the call to the fetch: its ThreadGrid uses the same scratch); seedsXy
   *  (2 per member): the seed cells; originCs: the merged map's origin x, y and its resolution (the message's float32).  TSD_E_ARG before the
   *  first publication. */
  int frontiers(const double* gridXy, uint32_t minSize, std::vector<tsd_frontier>* out, int* seedsUsed, int32_t* seedsXy, double* originCs);
  /** frontiers(), then on the same merged map and from the same seeds the cost-to-go field (tsd_route_dev: unit weights, free_max 0),
   *  the goal of every frontier -- its `seed` is the member nearest to that frontier, what an allocator starts from -- and the paths,
   *  cut at maxLen cells.  The two locks of frontiers() are held to the last fetch. */
  int explorePlan(const double* gridXy, uint32_t minSize, int maxLen, ExplorePlan* out, int32_t* seedsXy, double* originCs);
  /** Which member drives to which goal of the plan made last (tsd_view_assign on the merged map, free_max 0, one robot per member):
   *  a goal's worth is the unknown cells a scanner there would see within viewRadius [m] (rounded to cells, at least 1 and at most
   *  TSD_VIEW_MAX_RADIUS, returned in *radiusCells), and what one member is about to see is no longer worth a visit by another.
   *  goalOfRobot and picked hold one entry per member.  A member is only ever offered the goals it is nearest to (exploreDispatch
   *  plans on a field per member and lifts that).  Holds the publish
   *  mutex and member 0's frontierMutex and grid mutex.  TSD_E_ARG without a plan, where the merged map has been published again or
   *  re-placed since the plan was made, and where the device library has no views. */
  int exploreAssign(const tsd_route_goal* goals, size_t n, double viewRadius, uint32_t gainWeight, int unknownDepth, int32_t* goalOfRobot,
                    tsd_view_gain* picked, int* rounds, int* radiusCells);
  /** ThreadGrid::exploreWaypoints for the plan made last on the merged map: the paths to its goals straightened into waypoints
   *  (tsd_route_waypoints on member 0's context, which holds the plan's route result).  Holds the publish mutex and member 0's
   *  frontierMutex and grid mutex.  TSD_E_ARG without a plan, where the merged map has been published again or re-placed since the plan
   *  was made, and where the device library has no waypoints. */
  int exploreWaypoints(const tsd_route_goal* goals, size_t n, double lookahead, uint32_t slack, int maxLen, int maxWay, uint32_t* way,
                       tsd_waypoint_info* info, int* lookaheadCells);
  /** One call from the merged map to every member's way: the frontiers of the merged map published last with one seed per member
   *  (frontiers()), a cost-to-go field PER MEMBER on the same map (tsd_route_fields_dev: unit weights, free_max 0), the goal matrix
   *  (member r's cheapest cell of frontier f), the assignment across members (tsd_view_assign_fields: a member may be given a frontier
   *  another member is nearer to) and the waypoints of each member's goal on that member's own field (tsd_route_fields_waypoints).
   *  d's request fields are read, its results filled: goals[r * n + f]; goalOfRobot[r] a frontier index or -1; way[r * maxWay + i],
   *  i < min(wayInfo[r].n_way, maxWay), seed first -- a member without a goal has a record of len 0 and n_way 0.  Holds the locks
   *  explorePlan holds, from the frontiers to the last fetch.  Refuses as exploreAssign refuses: TSD_E_ARG before the first
   *  publication, for a negative unknownDepth, for more than TSD_FRONTIER_MAX_SEEDS members or TSD_VIEW_MAX_CELLS frontiers, and where
   *  the device library has no fields. */
  int exploreDispatch(const double* gridXy, uint32_t minSize, ExploreDispatch* d, int32_t* seedsXy, double* originCs);
  /** The velocity of every member's next step towards the goal the dispatch `d` gave it, for members at posesXyt (x, y [m], yaw [rad]
   *  per member in the merged map's frame): one fields call on the merged map seeded at the members' goal cells (tsd_route_fields_dev:
   *  unit weights, free_max 0 as exploreDispatch plans; limit: the largest goal dist plus q.margin; a member without a goal gets a
   *  seed outside the map, a layer without keys and no command), then one tsd_drive_fields_rollout, member r on layer r.  The
   *  goal-seeded layers REPLACE the robot-seeded fields result of the dispatch on member 0's context; the dispatch's answers have been
   *  fetched by then.  Holds the locks explorePlan holds.  TSD_E_ARG for a dispatch of another publication, a pose outside the map,
   *  what driveSamples refuses, and where the device library has no rollout.
   *  With fleet->separation > 0 the members keep off each other (tsd_drive_fleet_rollout instead): they decide in the order
   *  fleet->priority, each against the arcs chosen before it, and a member without a goal goes in as a parked robot the others keep
   *  clear of.  Without a priority list: the members with a goal in ascending cost-to-go at their pose (the one nearer its goal
   *  decides first; read from the goal-seeded layers), ties by index, then the others.  fleetOut gets the order used, the samples
   *  each member lost to the others and the chosen arcs in metres.  TSD_E_ARG also for a priority that is no permutation, a
   *  separation beyond TSD_DRIVE_MAX_SEP cells, a NULL fleetOut and where the device library has no fleet rollout.
   *  With `live` the current scans' end points refuse arcs as well, as in ThreadGrid::exploreDrive: one layer for all members, a
   *  skip disc at every member's pose (one member's scanner sees the other's body), set behind the fields call and cleared before
   *  the locks are given up. */
  int exploreDrive(const ExploreDispatch& d, const double* posesXyt, const DriveRequest& q, DriveAnswer* out, DriveSamples* samples,
                   const FleetDriveRequest* fleet = nullptr, FleetDriveAnswer* fleetOut = nullptr, const LiveRequest* live = nullptr,
                   LiveAnswer* liveOut = nullptr);
  size_t members(void) const { return _members.size(); }

  std::shared_ptr<rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>> gridPublisher() { return _gridPub; }
  std::shared_ptr<rclcpp::Service<nav_msgs::srv::GetMap>> mapService() { return _getMapServ; }
  bool getMapServCallBack(const std::shared_ptr<nav_msgs::srv::GetMap::Request> req,
                          std::shared_ptr<nav_msgs::srv::GetMap::Response> res);

protected:
  virtual void eventLoop(void);

private:
  int frontiersAndPlan(const double* gridXy, uint32_t minSize, std::vector<tsd_frontier>* out, int* seedsUsed, int32_t* seedsXy, double* originCs,
                       ExplorePlan* plan, int maxLen, ExploreDispatch* dispatch = nullptr);
  int dispatchLocked(tsd_ctx* ctx, const std::vector<int32_t>& seeds, ExploreDispatch* d);

  std::shared_ptr<rclcpp::Node> _node;
  std::vector<Member> _members;
  tsd_group* _group;
  std::shared_ptr<nav_msgs::msg::OccupancyGrid> _occGrid;
  std::shared_ptr<rclcpp::Service<nav_msgs::srv::GetMap>> _getMapServ;
  std::shared_ptr<rclcpp::Publisher<nav_msgs::msg::OccupancyGrid>> _gridPub;
  unsigned int _width;
  unsigned int _height;
  unsigned int _objInflateFactor;
  bool _objectInflation;
  int8_t* _hOcc;                 // page-locked landing buffer of the merged map
  std::mutex _publishMutex;      // one merge at a time (event loop, publish())
  std::mutex _msgMutex;          // _occGrid between a publication and the get_merged_map service
  uint64_t _frames;
  uint64_t _planFrames;          // _frames when explorePlan last succeeded (under _publishMutex; 0: no plan)
};

} /* namespace ohm_tsd_slam */
