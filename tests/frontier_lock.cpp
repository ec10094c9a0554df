// frontier_lock.cpp -- who may use a context's frontier scratch, on a box without a GPU (built by tests/test_cpu_frontier_lock.py with
// -fsanitize=thread).  Links the facade's own ThreadGrid / ThreadGridGroup sources against tests/stub_tsd_hip.c and the stand-ins
// below for the calls those two make.  A context's frontier scratch and result serve one call at a time, from the call to the fetch;
// a node's ThreadGrid (tsd_frontiers_frame, under its own publish mutex, without the grid's mutex) and a ThreadGridGroup that borrows
// member 0's context (tsd_frontiers_dev) meet there.  The stand-ins record every overlap of two calls on one context and every fetch
// that reads another thread's result; three threads -- publications with publish_frontiers on, ThreadGrid::frontiers, the group's
// frontiers -- run against each other.  Prints "ok"; exit code = number of failed checks.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "ThreadGrid.h"
#include "ThreadGridGroup.h"

using namespace ohm_tsd_slam;

// ---- stand-ins.  A context is an opaque pointer here; what belongs to it is kept by its address.
namespace {
struct Scratch
{
  std::atomic<int> inside{0};
  std::atomic<long> calls{0}, overlaps{0}, foreignFetches{0};
  std::mutex m;
  std::thread::id owner;         // the thread whose result the scratch holds
};
std::mutex g_tableMutex;
std::map<const void*, std::unique_ptr<Scratch>> g_table;
Scratch& scratchOf(const void* ctx)
{
  std::lock_guard<std::mutex> lk(g_tableMutex);
  auto& p = g_table[ctx];
  if(!p)
    p.reset(new Scratch());
  return *p;
}
int frontierCall(const void* ctx, int* n, int* used)
{
  Scratch& s = scratchOf(ctx);
  if(s.inside.fetch_add(1) != 0)
    s.overlaps++;
  s.calls++;
  std::this_thread::sleep_for(std::chrono::microseconds(300));      // (the kernels and the two waits)
  {
    std::lock_guard<std::mutex> lk(s.m);
    s.owner = std::this_thread::get_id();
  }
  s.inside.fetch_sub(1);
  *n = 3;
  if(used)
    *used = 0;
  return TSD_OK;
}
struct Group { int width, height; std::vector<int8_t> map; };
}  // namespace

extern "C" {
int tsd_frontiers_frame(tsd_ctx* ctx, const tsd_frontier_params*, int* n, int* used) { return frontierCall(ctx, n, used); }
int tsd_frontiers_dev(tsd_ctx* ctx, const void*, int, int, int, const tsd_frontier_params*, int* n, int* used) { return frontierCall(ctx, n, used); }
int tsd_frontiers_fetch(tsd_ctx* ctx, int, int count, tsd_frontier* out)
{
  Scratch& s = scratchOf(ctx);
  {
    std::lock_guard<std::mutex> lk(s.m);
    if(s.owner != std::this_thread::get_id())
      s.foreignFetches++;
  }
  std::memset(out, 0, (size_t)count * sizeof(tsd_frontier));
  for(int i = 0; i < count; i++)
    out[i].size = 10u + (uint32_t)i;
  return TSD_OK;
}
void* tsd_host_alloc(uint64_t bytes) { return std::calloc(1, (size_t)bytes); }
void tsd_host_free(void* p) { std::free(p); }
int tsd_map_frame_begin(tsd_ctx*, const tsd_map_params*, int8_t*, uint8_t*) { return TSD_OK; }
int tsd_map_frame_wait(tsd_ctx*, int* n) { if(n) *n = 1; return TSD_OK; }
int tsd_map_update_begin(tsd_ctx*, const tsd_map_params*, int8_t*, uint8_t*, tsd_map_window* w) { w->x = w->y = w->width = w->height = 0; return TSD_OK; }
int tsd_map_update_wait(tsd_ctx*, int* n) { if(n) *n = 0; return TSD_OK; }
int tsd_costmap_begin(tsd_ctx*, const tsd_costmap_params*, int8_t*, uint16_t*, const tsd_map_window*, tsd_map_window*) { return TSD_E_ARG; }
int tsd_costmap_wait(tsd_ctx*) { return TSD_E_ARG; }
int tsd_surface_extract(tsd_ctx*, const tsd_surface_params*, int*) { return TSD_E_ARG; }
int tsd_surface_fetch(tsd_ctx*, int, int, double*, double*, uint8_t*) { return TSD_E_ARG; }
int tsd_fuse_begin(tsd_ctx*, int, tsd_ctx* const*, const int32_t*) { return TSD_E_ARG; }
int tsd_fuse_wait(tsd_ctx*, tsd_fuse_stats*) { return TSD_E_ARG; }
tsd_group* tsd_group_create(int, tsd_ctx* const*, const int32_t*, int, int)
{
  Group* g = new Group{64, 64, std::vector<int8_t>(64 * 64, 0)};
  return reinterpret_cast<tsd_group*>(g);
}
tsd_group* tsd_group_create_rigid(int, tsd_ctx* const*, const double*, int, int) { return nullptr; }
void tsd_group_destroy(tsd_group* g) { delete reinterpret_cast<Group*>(g); }
int tsd_group_width(const tsd_group* g) { return reinterpret_cast<const Group*>(g)->width; }
int tsd_group_height(const tsd_group* g) { return reinterpret_cast<const Group*>(g)->height; }
void* tsd_group_map_dev(tsd_group* g) { return reinterpret_cast<Group*>(g)->map.data(); }
int tsd_group_extract_begin(tsd_group*, int, const tsd_map_params*) { return TSD_OK; }
int tsd_group_merge_maps_begin(tsd_group*, const void* const*, int8_t*) { return TSD_OK; }
int tsd_group_merge_wait(tsd_group*, int* n) { if(n) *n = 0; return TSD_OK; }
int tsd_group_cell_offsets(const tsd_group*, int32_t*) { return TSD_E_ARG; }
int tsd_group_corner(const tsd_group*, int32_t* x0, int32_t* y0) { if(x0) *x0 = 0; if(y0) *y0 = 0; return TSD_OK; }
int tsd_group_member_transform(const tsd_group*, int, double T[9])
{
  static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::memcpy(T, I, sizeof(I));
  return TSD_OK;
}
}  // extern "C"

static int g_failed = 0;
#define CHECK(cond, ...) do { if(!(cond)) { g_failed++; std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
                                           std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } while(0)

int main()
{
  auto node = std::make_shared<rclcpp::Node>("tsd_slam");
  node->declare_parameter("tf_map_frame", std::string("map"));
  node->declare_parameter("object_inflation_factor", 2);
  node->declare_parameter("use_object_inflation", false);
  node->set_parameter("publish_frontiers", true);
  std::vector<obvious::TsdGrid*> grids;
  for(int i = 0; i < 2; i++)
    grids.push_back(new obvious::TsdGrid(0.05, obvious::LAYOUT_32x32, static_cast<obvious::EnumTsdGridLayout>(6), 0));
  {
    ThreadGrid worker(grids[0], node, 0.0, 0.0);                     // member 0's own publisher, publish_frontiers on
    ThreadGridGroup group(node, {{grids[0], 0.0, 0.0}, {grids[1], 0.0, 0.0}});
    CHECK(worker.publish() == TSD_OK && worker.frontierClouds() == 1, "the first publication carries no frontier cloud");
    CHECK(group.publish() == TSD_OK, "the group's first merge failed");
    const int rounds = 60;
    std::atomic<int> bad{0};
    std::thread a([&] { for(int k = 0; k < rounds; k++) if(worker.publish() != TSD_OK) bad++; });
    std::thread b([&] {
      std::vector<tsd_frontier> out;
      const int32_t seed[2] = {1, 1};
      double place[3];
      for(int k = 0; k < rounds; k++) { int used = -1; if(worker.frontiers(seed, 1, 1u, &out, &used, place) != TSD_OK || out.size() != 3) bad++; }
    });
    std::thread c([&] {
      std::vector<tsd_frontier> out;
      const double xy[4] = {0.5, 0.5, 1.0, 1.0};
      int32_t seeds[4];
      double place[3];
      for(int k = 0; k < rounds; k++) { int used = -1; if(group.frontiers(xy, 1u, &out, &used, seeds, place) != TSD_OK || out.size() != 3) bad++; }
    });
    a.join(); b.join(); c.join();
    CHECK(bad == 0, "%d calls failed", bad.load());
    Scratch& s0 = scratchOf(grids[0]->context());
    CHECK(s0.calls == 1 + 3 * rounds, "member 0's context carried %ld frontier calls, expected %d", s0.calls.load(), 1 + 3 * rounds);
    CHECK(s0.overlaps == 0, "%ld frontier calls ran beside another on member 0's context", s0.overlaps.load());
    CHECK(s0.foreignFetches == 0, "%ld fetches read a result another thread's call had replaced", s0.foreignFetches.load());
    CHECK(worker.frontierClouds() == 1 + (uint64_t)rounds, "%llu clouds", (unsigned long long)worker.frontierClouds());
  }
  for(obvious::TsdGrid* g : grids)
    delete g;
  if(!g_failed)
    std::printf("ok\n");
  return g_failed;
}
