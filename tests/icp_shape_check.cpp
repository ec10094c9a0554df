// icp_shape_check.cpp -- the registration's launch decision (csrc/icp_shape.hpp) on the CPU: icp_shape_for, icp_helpers and
// icp_with_shape against rows written out by hand from the table of DESIGN 3.3 (family, threads, capacity, node shape, helper
// workgroups, errors), and against tests/golden/icp_shapes.txt for what is not to be invented: the LDS bytes, the one or two halves of
// the slot array and which shapes do not fit 160 KiB -- recorded once from the arithmetic as it stood before the header existed.
//   icp_shape_check <golden file>   the check: "ok <case>" per group, "icp_shape: all cases ok" at the end
//   icp_shape_check --rows          "name cap T ptl" of every row that reaches the LDS arithmetic (what the golden file is keyed by)
// Built and run by tests/test_cpu_icp_shape.py under -fsanitize=address,undefined.
#include "icp_shape.hpp"

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace tsd;

static const char* const E_POINTS = "icp points > TSD_MAX_ICP_POINTS";
static const char* const E_SHAPE = "icp workgroup shape";
static const char* const E_LDS = "registration does not fit the LDS of one CU";
static const char* const E_LDS_PTL = "registration does not fit the LDS of one CU (point-to-line: model normals too)";

struct Row {
  std::string name;
  int n_cap, n_thr; bool ptl; int forced;      // the call
  int R, MAXT, T, cap; bool node;              // the shape it must give ...
  int helpers;                                 // ... and the helper workgroups of n_thr points in it, helpers switched on
  const char* error;                           // or: the TSD_E_CAPACITY it must give (nullptr: whatever the golden file says about the LDS)
};

static Row ok(const std::string& name, int n_cap, int n_thr, bool ptl, int forced, int R, int MAXT, int T, int cap, bool node, int helpers)
{
  return Row{name, n_cap, n_thr, ptl, forced, R, MAXT, T, cap, node, helpers, nullptr};
}
static Row bad(const std::string& name, int n_cap, int n_thr, bool ptl, int forced, const char* error)
{
  return Row{name, n_cap, n_thr, ptl, forced, 0, 0, 0, 0, false, 0, error};
}

// the fused scan, TSD_ICP_SHAPE unset: n beams size the arrays and decide the threads
static std::vector<Row> fused(bool ptl)
{
  struct F { int n, R, MAXT, T, cap; bool node; int helpers; };
  static const F rows[] = {
    {1, 3, 512, 64, 64, false, 1},         {192, 3, 512, 64, 192, false, 3},     {193, 3, 512, 128, 256, false, 2},
    {768, 3, 512, 256, 768, false, 3},     {769, 3, 512, 320, 832, false, 4},    {960, 3, 512, 448, 960, false, 4},
    {961, 3, 512, 512, 1024, false, 4},    {1024, 3, 512, 512, 1024, false, 4},  {1025, 3, 512, 512, 1088, true, 5},
    {1081, 3, 512, 512, 1088, true, 5},    {1088, 3, 512, 512, 1088, true, 5},   {1089, 3, 512, 512, 1152, false, 5},
    {1536, 3, 512, 512, 1536, false, 6},   {1537, 8, 256, 256, 1600, false, 7},  {2048, 8, 256, 256, 2048, false, 8},
  };
  std::vector<Row> v;
  const std::string prefix = ptl ? "fused_ptl_" : "fused_";
  for (const F& f : rows) v.push_back(ok(prefix + std::to_string(f.n), f.n, f.n, ptl, 0, f.R, f.MAXT, f.T, f.cap, f.node && !ptl, f.helpers));
  v.push_back(bad(prefix + "2049", 2049, 2049, ptl, 0, E_POINTS));
  return v;
}
static std::vector<Row> forced_shapes()
{
  return {
    ok("forced8_1081", 1081, 1081, false, 8, 8, 256, 192, 1088, false, 6),
    ok("forced8_40", 40, 40, false, 8, 8, 256, 64, 64, false, 1),
    ok("forced512_300", 300, 300, false, 512, 3, 512, 512, 320, false, 2),
    bad("forced576_300", 300, 300, false, 576, E_SHAPE),
    ok("forced64_1081", 1081, 1081, false, 64, 3, 512, 512, 1088, true, 5),
  };
}
// direct mode: the larger of model and scene sizes the arrays, the scene decides the threads
static std::vector<Row> direct_mode()
{
  auto d = [](int n_model, int n_scene, int R, int MAXT, int T, int cap, bool node, int helpers) {
    return ok("direct_" + std::to_string(n_model) + "_" + std::to_string(n_scene), n_model > n_scene ? n_model : n_scene, n_scene, false, 0,
              R, MAXT, T, cap, node, helpers);
  };
  return {d(1088, 961, 3, 512, 512, 1088, true, 4), d(1088, 960, 3, 512, 448, 1088, false, 4), d(2048, 10, 3, 512, 64, 2048, false, 1),
          d(10, 2048, 8, 256, 256, 2048, false, 8)};
}

struct Golden { int cap, T, ptl; unsigned long long lds; int halves, fits; };
static std::map<std::string, Golden> golden;

static bool read_golden(const char* path)
{
  std::FILE* f = std::fopen(path, "r");
  if (!f) return false;
  char line[256], name[64];
  while (std::fgets(line, sizeof(line), f)) {
    Golden g;
    if (line[0] == '#' || std::sscanf(line, "%63s %d %d %d %llu %d %d", name, &g.cap, &g.T, &g.ptl, &g.lds, &g.halves, &g.fits) != 7) continue;
    golden[name] = g;
  }
  std::fclose(f);
  return true;
}

// what icp_with_shape hands its functor
struct Tags { int R, MAXT, ptl, fcap, ft; };
struct Recorder {
  std::vector<Tags>* calls;
  template <class S> int operator()(S) const { calls->push_back(Tags{S::R, S::MAXT, S::PTL, S::FCAP, S::FT}); return 7; }
};

static int failures = 0;

static void run(const char* group, const std::vector<Row>& rows)
{
  int bad = 0;
  auto fail = [&](const Row& r, const char* msg) { std::printf("FAIL %s %s: %s\n", group, r.name.c_str(), msg); bad++; };
  for (const Row& r : rows) {
    const IcpShape s = icp_shape_for(r.n_cap, r.n_thr, r.ptl, r.forced, 0);
    std::printf("  %s: rc %d (%s) <%d,%d> T %d cap %d ptl %d node %d lds %zu\n", r.name.c_str(), s.rc, s.rc ? s.why : "", s.R, s.MAXT, s.T,
                s.cap, (int)s.ptl, (int)s.node, s.lds);
    const char* want_error = r.error;
    const Golden* g = nullptr;
    if (!want_error) {
      auto it = golden.find(r.name);
      if (it == golden.end()) { fail(r, "no line in the golden file"); continue; }
      g = &it->second;
      if (g->cap != r.cap || g->T != r.T || g->ptl != (int)r.ptl) { fail(r, "the golden line was recorded for another shape"); continue; }
      if (!g->fits) want_error = r.ptl ? E_LDS_PTL : E_LDS;
    }
    if (want_error) {
      if (s.rc != TSD_E_CAPACITY || !s.why || std::strcmp(s.why, want_error) != 0) fail(r, "wanted TSD_E_CAPACITY with the row's message");
      continue;
    }
    if (s.rc != TSD_OK) { fail(r, "an error where a shape was wanted"); continue; }
    if (s.R != r.R || s.MAXT != r.MAXT) fail(r, "family");
    if (s.T != r.T) fail(r, "threads");
    if (s.cap != r.cap) fail(r, "capacity");
    if (s.ptl != r.ptl) fail(r, "estimator");
    if (s.node != r.node) fail(r, "node shape");
    if ((unsigned long long)s.lds != g->lds) fail(r, "LDS bytes");
    if (icp_slot_halves(s.cap, s.T, s.ptl) != g->halves) fail(r, "halves of the slot array");
    if (icp_shape_for(r.n_cap, r.n_thr, r.ptl, r.forced, 4096).lds != s.lds + 4096) fail(r, "extra LDS is added on top");
    if (icp_helpers(true, r.n_thr, s.T) != r.helpers) { std::printf("  got %d helpers\n", icp_helpers(true, r.n_thr, s.T)); fail(r, "helpers"); }
    if (icp_helpers(false, r.n_thr, s.T) != 0) fail(r, "helpers switched off");
    std::vector<Tags> calls;
    if (icp_with_shape(s, Recorder{&calls}) != 7) fail(r, "the dispatcher returns what the functor returned");
    const Tags want = r.node ? Tags{3, 512, 0, 1088, 512} : Tags{r.R, r.MAXT, (int)r.ptl, 0, 0};
    if (calls.size() != 1) { fail(r, "the dispatcher calls the functor exactly once"); continue; }
    const Tags& c = calls[0];
    if (c.R != want.R || c.MAXT != want.MAXT || c.ptl != want.ptl || c.fcap != want.fcap || c.ft != want.ft) {
      std::printf("  got tags <%d,%d,%d,%d,%d>\n", c.R, c.MAXT, c.ptl, c.fcap, c.ft);
      fail(r, "the dispatcher's tags");
    }
  }
  if (bad) failures += bad; else std::printf("ok %s\n", group);
}

int main(int argc, char** argv)
{
  std::vector<std::pair<const char*, std::vector<Row>>> groups = {
    {"fused_closed_form", fused(false)}, {"fused_point_to_line", fused(true)}, {"forced_shapes", forced_shapes()}, {"direct_mode", direct_mode()}};
  if (argc == 2 && std::strcmp(argv[1], "--rows") == 0) {
    for (const auto& g : groups)
      for (const Row& r : g.second)
        if (!r.error) std::printf("%s %d %d %d\n", r.name.c_str(), r.cap, r.T, (int)r.ptl);
    return 0;
  }
  if (argc != 2 || !read_golden(argv[1])) { std::printf("usage: icp_shape_check <tests/golden/icp_shapes.txt> | --rows\n"); return 2; }
  for (const auto& g : groups) run(g.first, g.second);

  // a batch of two sensors, 1081 and 360 beams, closed form: the widest decides the shape, each entry's helpers are its own beams in
  // that shape's threads, the grid is entries x (1 + the most helpers of any entry).  TSD_ICP_SHAPE has no way in.
  {
    const IcpShape s = icp_batch_shape(1081, false);
    const IcpShape f = icp_shape_for(1081, 1081, false, 0, 0);
    const int h0 = icp_helpers(true, 1081, s.T), h1 = icp_helpers(true, 360, s.T);
    const int grid = 2 * (1 + (h0 > h1 ? h0 : h1));
    const bool good = s.rc == TSD_OK && s.node && s.R == f.R && s.MAXT == f.MAXT && s.T == f.T && s.cap == f.cap && s.lds == f.lds && h0 == 5 && h1 == 2 &&
                      grid == 12 && icp_batch_shape(1081, true).rc == TSD_OK && !icp_batch_shape(1081, true).node &&
                      icp_batch_shape(2049, false).rc == TSD_E_CAPACITY;
    if (good) std::printf("ok batch\n"); else { std::printf("FAIL batch: node %d helpers %d %d grid %d\n", (int)s.node, h0, h1, grid); failures++; }
  }
  // more points than sixteen helpers reach: none at all
  {
    const bool good = icp_helpers(true, 16 * 64, 64) == 16 && icp_helpers(true, 16 * 64 + 1, 64) == 0 && icp_helpers(true, 2048, 128) == 16 &&
                      icp_helpers(true, 2048, 64) == 0;
    if (good) std::printf("ok helpers_limit\n"); else { std::printf("FAIL helpers_limit\n"); failures++; }
  }
  if (failures) { std::printf("icp_shape: %d failures\n", failures); return 1; }
  std::printf("icp_shape: all cases ok\n");
  return 0;
}
