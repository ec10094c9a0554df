// map_source_check.cpp -- the map products' rule header (csrc/map_source_rule.hpp) on the CPU: when a call on a caller's map, a call on
// the last published frame and a fetch are refused, and the seed list the kernels are handed.  What each case must return is written
// out below by hand, as tables, from the rule as include/tsd_hip.h states it -- none of it is computed by the header.  Built and run
// by tests/test_cpu_map_source.py under -fsanitize=address,undefined.  Prints "ok <case>" per case, "map_source: all cases ok" at the end.
#include "map_source_rule.hpp"

#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>

using namespace tsd;

static int failures = 0;
static void done(const char* name, int bad)
{
  if (bad) { std::printf("FAIL %s: %d wrong\n", name, bad); failures++; }
  else std::printf("ok %s\n", name);
}
static bool same(const char* got, const char* want) { return (!got && !want) || (got && want && std::strcmp(got, want) == 0); }

static const char* const COST_FLIGHT = "a cost map is in flight (tsd_costmap_wait first)";
static const char* const FRAME_FLIGHT = "a frame is in flight (tsd_map_frame_wait first)";
static const char* const NO_FRAME = "no completed frame to read";
static const char* const SIDE = "the grid's side is above TSD_FRONTIER_MAX_SIDE";
static const char* const NO_COST = "no completed cost map of the grid's size to read";
static const char* const CALLER = "a null map, a side outside 1 .. TSD_FRONTIER_MAX_SIDE, or stride < width";
static const char* const RANGE = "the range is outside [0, n) or out is NULL";

// ---- frame_map_wrong.  The order of the conditions: cost map in flight, frame in flight, no completed frame, the side, the cost map.
static void frame_rule()
{
  // bit 3: a cost map in flight, bit 2: a frame in flight, bit 1: the frame's map valid, bit 0: a staging exists.  nullptr: the flags
  // let the call through to the side
  static const char* const by_flags[16] = {
    /* 0000 */ NO_FRAME,    /* 0001 */ NO_FRAME,    /* 0010 */ NO_FRAME,    /* 0011 */ nullptr,
    /* 0100 */ FRAME_FLIGHT, /* 0101 */ FRAME_FLIGHT, /* 0110 */ FRAME_FLIGHT, /* 0111 */ FRAME_FLIGHT,
    /* 1000 */ COST_FLIGHT, /* 1001 */ COST_FLIGHT, /* 1010 */ COST_FLIGHT, /* 1011 */ COST_FLIGHT,
    /* 1100 */ COST_FLIGHT, /* 1101 */ COST_FLIGHT, /* 1110 */ COST_FLIGHT, /* 1111 */ COST_FLIGHT,
  };
  // behind the flags: [N at the limit, N above][want_cost][cost map absent, of N * N cells, of N * N - 1 cells]
  static const char* const behind[2][2][3] = {
    {{nullptr, nullptr, nullptr}, {NO_COST, nullptr, NO_COST}},
    {{SIDE, SIDE, SIDE}, {SIDE, SIDE, SIDE}},
  };
  int bad = 0, accepted[2] = {0, 0}, accepted_flags_and_side[2] = {0, 0};
  for (int flags = 0; flags < 16; flags++)
    for (int above = 0; above < 2; above++)
      for (int want = 0; want < 2; want++) {
        int any = 0;
        for (int cost = 0; cost < 3; cost++) {
          const int N = TSD_FRONTIER_MAX_SIDE + above;
          FrameState s{};
          s.cost_inflight = (flags & 8) != 0; s.frame_inflight = (flags & 4) != 0; s.frame_map_valid = (flags & 2) != 0; s.staged = (flags & 1) != 0;
          s.N = N;
          s.have_cost = cost != 0;
          s.cost_cells = cost == 0 ? 0 : (size_t)N * (size_t)N - (cost == 2 ? 1 : 0);
          const char* want_text = by_flags[flags] ? by_flags[flags] : behind[above][want][cost];
          const char* got = frame_map_wrong(s, TSD_FRONTIER_MAX_SIDE, want != 0);
          if (!same(got, want_text)) {
            std::printf("  frame_map_wrong flags %d N %d want_cost %d cost %d: got \"%s\", want \"%s\"\n", flags, N, want, cost, got ? got : "(accepted)",
                        want_text ? want_text : "(accepted)");
            bad++;
          }
          if (!got) { accepted[want]++; any = 1; }
        }
        accepted_flags_and_side[want] += any;
      }
  // one combination of flags and side per want_cost lets a call through: nothing in flight, a valid staged frame, the side at the
  // limit.  Without want_cost the cost map's state is not looked at (all 3 states pass), with it only the cost map of N * N cells does.
  if (accepted_flags_and_side[0] != 1 || accepted_flags_and_side[1] != 1 || accepted[0] != 3 || accepted[1] != 1) {
    std::printf("  accepted: %d %d combinations of flags and side, %d %d cases\n", accepted_flags_and_side[0], accepted_flags_and_side[1], accepted[0], accepted[1]);
    bad++;
  }
  // a limit of the caller's own (the cost map passes 65536): the same grid passes there
  FrameState s{false, false, true, true, TSD_FRONTIER_MAX_SIDE + 1, false, 0};
  if (frame_map_wrong(s, 65536, false) != nullptr) bad++;
  s.N = 65537;
  if (!same(frame_map_wrong(s, 65536, false), SIDE)) bad++;
  done("frame_map_wrong", bad);
}

// ---- caller_map_wrong
static void caller_rule()
{
  static const int limits[2] = {TSD_FRONTIER_MAX_SIDE, 65536};
  // sides 0, 1, max_side, max_side + 1; strides w - 1, w, w + 1
  static const bool side_ok[4] = {false, true, true, false};
  static const bool stride_ok[3] = {false, true, true};
  const int8_t cell = 0;
  int bad = 0, n_ok = 0;
  for (int l = 0; l < 2; l++)
    for (int wi = 0; wi < 4; wi++)
      for (int hi = 0; hi < 4; hi++)
        for (int si = 0; si < 3; si++)
          for (int have = 0; have < 2; have++) {
            const int max_side = limits[l];
            const int sides[4] = {0, 1, max_side, max_side + 1};
            const int w = sides[wi], h = sides[hi], stride = w - 1 + si;
            const bool ok = have && side_ok[wi] && side_ok[hi] && stride_ok[si];
            const char* got = caller_map_wrong(have ? &cell : nullptr, w, h, stride, max_side);
            if (!same(got, ok ? nullptr : CALLER)) { std::printf("  caller_map_wrong map %d w %d h %d stride %d limit %d: got \"%s\"\n", have, w, h, stride, max_side, got ? got : "(accepted)"); bad++; }
            n_ok += got ? 0 : 1;
          }
  if (n_ok != 2 * 2 * 2 * 2) { std::printf("  caller_map_wrong accepted %d of 192, want 16\n", n_ok); bad++; }     // per limit: 2 widths x 2 heights x 2 strides
  done("caller_map_wrong", bad);
}

// ---- fetch_range_wrong
static void fetch_rule()
{
  // per n and first, the counts -1, 0, 1, n - first, n - first + 1, INT_MAX: R refused, A accepted with or without `out`, O accepted
  // only with `out`
  struct Row { int n, first; const char* by_count; };
  static const Row rows[] = {
    {5, -1, "RRRRRR"},     // (n - first = 6, 7)
    {5, 0, "RAOORR"},      // (n - first = 5: the whole list; 6: one too many)
    {5, 5, "RARARR"},      // (first == n: the empty range at the end, and n - first = 0 is it again)
    {5, 6, "RRRRRR"},      // (n - first = -1; n - first + 1 = 0 records, but from beyond the end)
    {0, -1, "RRRRRR"},
    {0, 0, "RARARR"},      // (first == n == 0: an empty result has its empty range)
    {0, 1, "RRRRRR"},
  };
  const int8_t cell = 0;
  int bad = 0;
  for (const Row& r : rows) {
    const int counts[6] = {-1, 0, 1, r.n - r.first, r.n - r.first + 1, INT_MAX};
    for (int ci = 0; ci < 6; ci++)
      for (int have = 0; have < 2; have++) {
        const char c = r.by_count[ci];
        const bool ok = c == 'A' || (c == 'O' && have);
        const char* got = fetch_range_wrong(r.first, counts[ci], r.n, have ? &cell : nullptr);
        if (!same(got, ok ? nullptr : RANGE)) { std::printf("  fetch_range_wrong n %d first %d count %d out %d: got \"%s\"\n", r.n, r.first, counts[ci], have, got ? got : "(accepted)"); bad++; }
      }
  }
  done("fetch_range_wrong", bad);
}

// ---- map_seeds, and the two kernel arguments' layout
static void seeds()
{
  int bad = 0;
  int32_t xy[2 * TSD_FRONTIER_MAX_SEEDS];
  for (int k = 0; k < 2 * TSD_FRONTIER_MAX_SEEDS; k++) xy[k] = 1000 + k;
  const int ns[3] = {0, 1, 16};
  for (int n : ns) {
    const MapSeeds sd = map_seeds(n, n ? xy : nullptr);
    if (sd.n != n) bad++;
    for (int k = 0; k < 2 * TSD_FRONTIER_MAX_SEEDS; k++)
      if (sd.xy[k] != (k < 2 * n ? 1000 + k : 0)) { std::printf("  map_seeds n %d: xy[%d] = %d\n", n, k, sd.xy[k]); bad++; }
  }
  static_assert(TSD_FRONTIER_MAX_SEEDS == 16, "the cases above are written for 16 seeds");
  static_assert(sizeof(MapSeeds) == 4 + 8 * TSD_FRONTIER_MAX_SEEDS, "MapSeeds: n, then the pairs");
  static_assert(sizeof(MapView) == 24 && offsetof(MapView, map) == 0 && offsetof(MapView, W) == 8 && offsetof(MapView, H) == 12 && offsetof(MapView, stride) == 16,
                "MapView: the layout the kernels were built with");
  done("map_seeds", bad);
}

int main()
{
  frame_rule();
  caller_rule();
  fetch_rule();
  seeds();
  if (failures) { std::printf("map_source: %d case(s) FAILED\n", failures); return 1; }
  std::printf("map_source: all cases ok\n");
  return 0;
}
