// map_source_rule.hpp -- what the products of an int8 map (clearance.hip, frontier.hip, route.hip, view.hip) are handed and when they
// refuse: the map as a kernel argument, the seed list, the rule for a caller's map, the rule for a call on the last published frame
// and the range of a fetch.  Plain host logic, no HIP and nothing of the context: tests/map_source_check.cpp runs it on the CPU.
// map_product.hpp applies it to a context.
#pragma once
#include <cstddef>
#include <cstdint>

#include "tsd_hip.h"

namespace tsd {

// The map as the kernels take it: W x H cells, `stride` bytes from row to row.
struct MapView { const int8_t* map; int W, H; size_t stride; };

// Up to TSD_FRONTIER_MAX_SEEDS seed cells, by value; the entries past n are 0, so the bytes that reach the device are defined ones.
struct MapSeeds { int n; int xy[2 * TSD_FRONTIER_MAX_SEEDS]; };

inline MapSeeds map_seeds(int n, const int32_t* xy)      // (the caller has checked 0 <= n <= TSD_FRONTIER_MAX_SEEDS, xy non-null where n > 0)
{
  MapSeeds sd{};
  sd.n = n;
  for (int k = 0; k < 2 * n; k++) sd.xy[k] = xy[k];
  return sd;
}

// A map of the caller's: nullptr, or why it is refused.  One wording for every caller.
inline const char* caller_map_wrong(const void* map, int w, int h, int stride, int max_side)
{
  if (!map || w < 1 || h < 1 || w > max_side || h > max_side || stride < w)
    return "a null map, a side outside 1 .. TSD_FRONTIER_MAX_SIDE, or stride < width";
  return nullptr;
}

// What the frame rule reads of a context.
struct FrameState {
  bool cost_inflight;          // tsd_costmap_begin without its tsd_costmap_wait
  bool frame_inflight;         // tsd_map_frame_begin / tsd_map_update_begin without its wait
  bool frame_map_valid;        // the staging holds the complete map of the frame enqueued last
  bool staged;                 // there is a staging
  int N;                       // the grid's side
  bool have_cost;              // there is a cost map ...
  size_t cost_cells;           // ... of this many cells
};

// A call on the map of the last published frame (want_cost: on the cost map made of it): nullptr, or why it is refused.  The staging
// and the cost map are written on the copy stream by a frame / a cost map in flight, so both must have been waited for.
inline const char* frame_map_wrong(const FrameState& s, int max_side, bool want_cost)
{
  if (s.cost_inflight) return "a cost map is in flight (tsd_costmap_wait first)";
  if (s.frame_inflight) return "a frame is in flight (tsd_map_frame_wait first)";
  if (!s.frame_map_valid || !s.staged) return "no completed frame to read";
  if (s.N > max_side) return "the grid's side is above TSD_FRONTIER_MAX_SIDE";
  if (want_cost && (!s.have_cost || s.cost_cells != (size_t)s.N * (size_t)s.N)) return "no completed cost map of the grid's size to read";
  return nullptr;
}

// Records first .. first + count - 1 of n into `out`: nullptr, or why the fetch is refused.  count == 0 needs no `out`.
inline const char* fetch_range_wrong(int first, int count, int n, const void* out)
{
  if (first < 0 || count < 0 || first > n || count > n - first || (count > 0 && !out)) return "the range is outside [0, n) or out is NULL";
  return nullptr;
}

}  // namespace tsd
