// group.hip -- the same-device merge group of include/tsd_hip.h (tsd_group_*): N grid contexts of ONE process on ONE GPU, each shifted by
// whole cells, merged into one int8 occupancy map by a local kernel -- the signed maximum ncclAllReduce(int8, max) gives across GPUs
// (comm.hip), without RCCL.  Part of libtsd_hip.so; uses the contexts only through the public C ABI (tsd_stream,
// tsd_occupancy_dev_async), like comm.hip does.
//
// Ordering (events only; nothing waits on the host before tsd_group_merge_wait, nothing spins on the device):
//   member i's stream :  [wait ev_merged]  extraction into d_member[i]  record ev_extracted[i]
//   group stream      :  wait ev_extracted[*]  clear count  k_group_merge  record ev_merged  copy count (+ map) to the host
// The group's stream is non-blocking and created before anything else touches the device: the legacy NULL stream stays unused (it
// would take one of the few hardware queues the scans' streams are mapped onto, see comm.hip).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/tsd_hip.h"

#define TSD_GROUP_MAX 64
#define TSD_GROUP_MAX_SIDE 65536

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));      // a row of a window whose width is no multiple of 16
typedef short s16x2 __attribute__((ext_vector_type(2)));

// The count of occupied cells is one atomic per wave, and 16 384 waves adding to ONE address are handed through at ~88 per microsecond
// (the rate occupancy_device.hpp's work list is sharded for): 190 us for a kernel that streams its bytes in ~15.  The waves add to 32
// counters on lines of their own, in turn; tsd_group_merge_wait sums them.
constexpr int GROUP_COUNT_SHARDS = 32, GROUP_COUNT_STRIDE = 32;

struct GroupMember {
  const int8_t* map;      // w * h bytes, row = y, 16-byte aligned, w a multiple of 16
  int ox, oy, w, h;       // the member's cell (x, y) is the window's cell (x + ox, y + oy)
};
struct GroupArgs {        // by value: the member table is read with scalar loads from the kernel-argument segment
  int8_t* out;            // W * H bytes, row = y
  int* count;             // GROUP_COUNT_SHARDS counters, one per 128-byte line: their sum += cells equal to 100
  int W, H, n, chunks;    // chunks: 16-byte pieces per output row, (W + 15) / 16
  GroupMember m[TSD_GROUP_MAX];
};

// bytes s .. s + 15 of the 32 bytes lo | hi (s = 1 .. 15, the same in every lane): four v_alignbit-class instructions
__device__ __forceinline__ u32x4 funnel16(u32x4 lo, u32x4 hi, int s)
{
  const unsigned r = (unsigned)s & 3u;
  u32x4 o;
  switch (s >> 2) {
    case 0:
      o.x = __builtin_amdgcn_alignbyte(lo.y, lo.x, r); o.y = __builtin_amdgcn_alignbyte(lo.z, lo.y, r);
      o.z = __builtin_amdgcn_alignbyte(lo.w, lo.z, r); o.w = __builtin_amdgcn_alignbyte(hi.x, lo.w, r);
      break;
    case 1:
      o.x = __builtin_amdgcn_alignbyte(lo.z, lo.y, r); o.y = __builtin_amdgcn_alignbyte(lo.w, lo.z, r);
      o.z = __builtin_amdgcn_alignbyte(hi.x, lo.w, r); o.w = __builtin_amdgcn_alignbyte(hi.y, hi.x, r);
      break;
    case 2:
      o.x = __builtin_amdgcn_alignbyte(lo.w, lo.z, r); o.y = __builtin_amdgcn_alignbyte(hi.x, lo.w, r);
      o.z = __builtin_amdgcn_alignbyte(hi.y, hi.x, r); o.w = __builtin_amdgcn_alignbyte(hi.z, hi.y, r);
      break;
    default:
      o.x = __builtin_amdgcn_alignbyte(hi.x, lo.w, r); o.y = __builtin_amdgcn_alignbyte(hi.y, hi.x, r);
      o.z = __builtin_amdgcn_alignbyte(hi.z, hi.y, r); o.w = __builtin_amdgcn_alignbyte(hi.w, hi.z, r);
      break;
  }
  return o;
}

__device__ __forceinline__ uint32_t pk_max_i16(uint32_t a, uint32_t b)
{
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ uint32_t pk_shl8_b16(uint32_t a)
{
  return __builtin_bit_cast(uint32_t, (s16x2)(__builtin_bit_cast(s16x2, a) << (s16x2)(8)));
}

// The packed signed-byte maximum.  gfx950 has no packed 8-bit maximum; it has v_pk_max_i16.  The four bytes of a dword are kept as two
// pairs of 16-bit lanes whose HIGH byte is the map byte: `hi` takes the dword as it is (bytes 1 and 3 are in place; what sits below
// them can only decide between two values whose high bytes are equal, i.e. nothing), `lo` takes it shifted left by 8 inside each
// 16-bit lane (v_pk_lshlrev_b16: bytes 0 and 2).  Per member and dword: v_pk_max_i16, v_pk_lshlrev_b16, v_pk_max_i16.
struct Acc4 {
  uint32_t hi[4], lo[4];
  __device__ __forceinline__ void init()
  {
#pragma unroll
    for (int k = 0; k < 4; k++) hi[k] = lo[k] = 0x80008000u;         // -128 in every high byte
  }
  __device__ __forceinline__ void take(u32x4 v)
  {
#pragma unroll
    for (int k = 0; k < 4; k++) { hi[k] = pk_max_i16(hi[k], v[k]); lo[k] = pk_max_i16(lo[k], pk_shl8_b16(v[k])); }
  }
  // bytes 3, 1 from hi's high bytes, bytes 2, 0 from lo's: one v_perm_b32
  __device__ __forceinline__ uint32_t dword(int k) const { return __builtin_amdgcn_perm(hi[k], lo[k], 0x07030501u); }
};

// bytes of w that equal 100 (exact per-byte zero test of w ^ 0x64646464)
__device__ __forceinline__ int count100(uint32_t w)
{
  const uint32_t x = w ^ 0x64646464u;
  const uint32_t t = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;
  return __popc(~t & 0x80808080u);
}

// One lane per 16 bytes of an output row.  Per lane: for every member whose rows cover y and whose columns touch the piece, one aligned
// 16-byte load (x offset a multiple of 16) or two aligned 16-byte loads funnelled by the offset's low four bits (the same shift in
// every lane: member rows and output pieces both start on multiples of 16); a member that does not cover the row costs a scalar
// compare.  -128 is the maximum's identity, and since -128 is also a legal map value the covered bytes are tracked beside it: what no
// member covers becomes -1.  ROWS16: W is a multiple of 16 -- every piece is whole and its store is one aligned 16-byte store.
template <bool ROWS16>
__global__ void __launch_bounds__(256) k_group_merge(const GroupArgs a)
{
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  const unsigned chunks = (unsigned)a.chunks;
  const int y = (int)(t / chunks);
  const int x0 = (int)(t - (unsigned)y * chunks) * 16;
  int n100 = 0;
  if (y < a.H) {
    Acc4 acc;
    acc.init();
    u32x4 cov = (u32x4)(0u);
    for (int i = 0; i < a.n; i++) {
      const int ox = a.m[i].ox, oy = a.m[i].oy, w = a.m[i].w, h = a.m[i].h;
      const int my = y - oy, mx0 = x0 - ox;
      if ((unsigned)my >= (unsigned)h || mx0 <= -16 || mx0 >= w) continue;
      const int8_t* row = a.m[i].map + (size_t)my * (size_t)w;
      const int s = (-ox) & 15;                 // = mx0 & 15, from scalars only: uniform
      const int b0 = mx0 - s;                   // the aligned 16 bytes that hold the piece's first byte: -16 <= b0 < w
      if (s == 0) {                             // (then mx0 = b0 >= 0: the piece is one whole aligned block of the member)
        acc.take(*reinterpret_cast<const u32x4*>(row + b0));
        cov = (u32x4)(~0u);
        continue;
      }
      const bool in0 = b0 >= 0, in1 = b0 + 16 < w;
      u32x4 lo = (u32x4)(0u), hi = (u32x4)(0u);
      if (in0) lo = *reinterpret_cast<const u32x4*>(row + b0);
      if (in1) hi = *reinterpret_cast<const u32x4*>(row + b0 + 16);
      u32x4 v = funnel16(lo, hi, s);
      if (in0 && in1) { acc.take(v); cov = (u32x4)(~0u); continue; }
      // the member ends inside this piece: the bytes beyond it take the identity and stay uncovered
      const u32x4 c = funnel16(in0 ? (u32x4)(~0u) : (u32x4)(0u), in1 ? (u32x4)(~0u) : (u32x4)(0u), s);
      v = (v & c) | ((u32x4)(0x80808080u) & ~c);
      acc.take(v);
      cov |= c;
    }
    u32x4 r;
#pragma unroll
    for (int k = 0; k < 4; k++) { r[k] = acc.dword(k) | ~cov[k]; }      // uncovered: 0x80 | 0xFF = -1
    int8_t* o = a.out + (size_t)y * (size_t)a.W + (size_t)x0;
    if (ROWS16) {
      *reinterpret_cast<u32x4*>(o) = r;
#pragma unroll
      for (int k = 0; k < 4; k++) n100 += count100(r[k]);
    } else if (x0 + 16 <= a.W) {
      *reinterpret_cast<u32x4_u*>(o) = r;
#pragma unroll
      for (int k = 0; k < 4; k++) n100 += count100(r[k]);
    } else {                                     // the row's last, partial piece
      for (int j = 0; x0 + j < a.W; j++) {
        const int8_t b = (int8_t)(r[j >> 2] >> (8 * (j & 3)));
        o[j] = b;
        n100 += b == 100;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n100 += __shfl_down(n100, off, 64);
  if ((threadIdx.x & 63) == 0 && n100)                                // one atomic per wave at most
    atomicAdd(a.count + (((blockIdx.x << 2) | (threadIdx.x >> 6)) & (GROUP_COUNT_SHARDS - 1)) * GROUP_COUNT_STRIDE, n100);
}

}  // namespace

struct tsd_group {
  int n = 0, W = 0, H = 0, device = 0;
  int x0 = 0, y0 = 0;                          // the window's corner in the offsets' frame (bounding box: the smallest offsets)
  std::vector<tsd_ctx*> ctx;
  std::vector<int> ox, oy, side;               // offsets relative to the window's corner; cells per side of each member
  std::vector<int8_t*> d_member;
  std::vector<hipEvent_t> ev_extracted;        // member i's map written (its context's stream)
  std::vector<char> extracted_pending;
  int8_t* d_merged = nullptr;
  int* d_count = nullptr;                      // GROUP_COUNT_SHARDS counters, GROUP_COUNT_STRIDE ints apart
  int* h_count = nullptr;                      // pinned copy of them
  hipStream_t gstream = nullptr;               // the merge's stream
  hipEvent_t ev_merged = nullptr;              // the merge kernel has read the member maps (group stream)
  bool merged_pending = false;
  // tsd_group_profile: HIP events around every member's extraction and around the merge kernel
  bool profile = false;
  struct Timed { hipEvent_t t0, t1; bool merge; };
  std::vector<Timed> pending;
  std::vector<hipEvent_t> pool;
  double extract_ms = 0.0, merge_ms = 0.0;
  int merges_timed = 0;
  std::string err;
};

static constexpr size_t kCountBytes = (size_t)GROUP_COUNT_SHARDS * GROUP_COUNT_STRIDE * sizeof(int);

static hipEvent_t group_event(tsd_group* g)
{
  if (!g->pool.empty()) { hipEvent_t e = g->pool.back(); g->pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

static int group_fail(tsd_group* g, const char* what, hipError_t e)
{
  g->err = std::string(what) + ": " + (e != hipSuccess ? hipGetErrorString(e) : "");
  return TSD_E_HIP;
}

static void group_release(tsd_group* g)
{
  for (auto& t : g->pending) { hipEventDestroy(t.t0); hipEventDestroy(t.t1); }
  for (hipEvent_t e : g->pool) hipEventDestroy(e);
  for (hipEvent_t e : g->ev_extracted) if (e) hipEventDestroy(e);
  if (g->ev_merged) hipEventDestroy(g->ev_merged);
  for (int8_t* p : g->d_member) if (p) hipFree(p);
  if (g->d_merged) hipFree(g->d_merged);
  if (g->d_count) hipFree(g->d_count);
  if (g->h_count) hipHostFree(g->h_count);
  if (g->gstream) hipStreamDestroy(g->gstream);
  delete g;
}

extern "C" {

tsd_group* tsd_group_create(int n, tsd_ctx* const* ctxs, const int32_t* cell_off_xy, int width, int height)
{
  auto refuse = [](const char* what) -> tsd_group* { std::fprintf(stderr, "tsd_group_create: %s\n", what); return nullptr; };
  // ---- argument checks: nothing here touches the HIP runtime
  if (n < 1 || n > TSD_GROUP_MAX) return refuse("the number of members must be 1 .. 64");
  if (!ctxs) return refuse("no contexts");
  for (int i = 0; i < n; i++) if (!ctxs[i]) return refuse("a member context is NULL");
  if ((width == 0) != (height == 0) || width < 0 || height < 0 || width > TSD_GROUP_MAX_SIDE || height > TSD_GROUP_MAX_SIDE)
    return refuse("width and height are both 0 (bounding box) or both 1 .. 65536");
  const int device = tsd_device(ctxs[0]);
  const double cs = tsd_cell_size(ctxs[0]);
  for (int i = 1; i < n; i++) {
    if (tsd_device(ctxs[i]) != device) return refuse("the members must be on one device (across devices: include/tsd_comm.h)");
    const double c = tsd_cell_size(ctxs[i]);
    if (std::memcmp(&c, &cs, sizeof(double)) != 0) return refuse("the members must have the same cell size");
    for (int j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) return refuse("a context is listed twice");
  }
  tsd_group* g = new (std::nothrow) tsd_group();
  if (!g) return nullptr;
  g->n = n; g->device = device;
  g->ctx.assign(ctxs, ctxs + n);
  g->ox.resize(n); g->oy.resize(n); g->side.resize(n);
  int64_t lo_x = INT64_MAX, lo_y = INT64_MAX, hi_x = INT64_MIN, hi_y = INT64_MIN;
  for (int i = 0; i < n; i++) {
    g->side[i] = tsd_cells(ctxs[i]);
    const int64_t x = cell_off_xy ? cell_off_xy[2 * i] : 0, y = cell_off_xy ? cell_off_xy[2 * i + 1] : 0;
    if (g->side[i] <= 0 || g->side[i] % 16 != 0 || x < -(1 << 24) || x > (1 << 24) || y < -(1 << 24) || y > (1 << 24)) {
      delete g;
      return refuse("a member's size or offset is out of range");
    }
    g->ox[i] = (int)x; g->oy[i] = (int)y;
    lo_x = x < lo_x ? x : lo_x; lo_y = y < lo_y ? y : lo_y;
    hi_x = x + g->side[i] > hi_x ? x + g->side[i] : hi_x; hi_y = y + g->side[i] > hi_y ? y + g->side[i] : hi_y;
  }
  if (width == 0) {
    if (hi_x - lo_x > TSD_GROUP_MAX_SIDE || hi_y - lo_y > TSD_GROUP_MAX_SIDE) { delete g; return refuse("the bounding box exceeds 65536 cells"); }
    g->x0 = (int)lo_x; g->y0 = (int)lo_y; g->W = (int)(hi_x - lo_x); g->H = (int)(hi_y - lo_y);
    for (int i = 0; i < n; i++) { g->ox[i] -= g->x0; g->oy[i] -= g->y0; }
  } else {
    g->W = width; g->H = height;
  }
  // ---- device objects; the group's stream first
  auto fail = [&](const char* what) -> tsd_group* { std::fprintf(stderr, "tsd_group_create: %s\n", what); group_release(g); return nullptr; };
  g->d_member.assign(n, nullptr); g->ev_extracted.assign(n, nullptr); g->extracted_pending.assign(n, 0);
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&g->gstream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&g->ev_merged, hipEventDisableTiming) != hipSuccess)
    return fail("stream / events");
  for (int i = 0; i < n; i++) {
    const size_t bytes = (size_t)g->side[i] * (size_t)g->side[i];
    if (hipEventCreateWithFlags(&g->ev_extracted[i], hipEventDisableTiming) != hipSuccess) return fail("events");
    if (hipMalloc(&g->d_member[i], bytes) != hipSuccess) return fail("no device memory for a member's map");
    if (hipMemsetAsync(g->d_member[i], 0xFF, bytes, g->gstream) != hipSuccess) return fail("clearing a member's map");    // -1 = unknown
  }
  const size_t out_bytes = (size_t)g->W * (size_t)g->H;
  if (hipMalloc(&g->d_merged, out_bytes) != hipSuccess || hipMalloc(&g->d_count, kCountBytes) != hipSuccess ||
      hipHostMalloc(&g->h_count, kCountBytes, hipHostMallocDefault) != hipSuccess)
    return fail("no memory for the merged map");
  std::memset(g->h_count, 0, kCountBytes);
  if (hipMemsetAsync(g->d_merged, 0xFF, out_bytes, g->gstream) != hipSuccess || hipStreamSynchronize(g->gstream) != hipSuccess)
    return fail("clearing the merged map");
  return g;
}

void tsd_group_destroy(tsd_group* g)
{
  if (!g) return;
  hipSetDevice(g->device);
  // (the members' streams may still hold extractions into the group's buffers)
  for (int i = 0; i < g->n; i++) if (g->extracted_pending[i]) hipEventSynchronize(g->ev_extracted[i]);
  if (g->gstream) hipStreamSynchronize(g->gstream);
  group_release(g);
}

int tsd_group_size(const tsd_group* g) { return g ? g->n : 0; }
int tsd_group_width(const tsd_group* g) { return g ? g->W : 0; }
int tsd_group_height(const tsd_group* g) { return g ? g->H : 0; }
int tsd_group_corner(const tsd_group* g, int32_t* x0, int32_t* y0)
{
  if (!g) return TSD_E_ARG;
  if (x0) *x0 = g->x0;
  if (y0) *y0 = g->y0;
  return TSD_OK;
}
const char* tsd_group_last_error(const tsd_group* g) { return g ? g->err.c_str() : "null group"; }
void* tsd_group_map_dev(tsd_group* g) { return g ? g->d_merged : nullptr; }
void* tsd_group_member_map_dev(tsd_group* g, int i) { return (g && i >= 0 && i < g->n) ? g->d_member[i] : nullptr; }

int tsd_group_extract_begin(tsd_group* g, int i, const tsd_map_params* params)
{
  if (!g || i < 0 || i >= g->n || !params) return TSD_E_ARG;
  if (hipSetDevice(g->device) != hipSuccess) return group_fail(g, "hipSetDevice", hipGetLastError());
  hipStream_t ms = static_cast<hipStream_t>(tsd_stream(g->ctx[i]));
  // the previous merge may still be reading this member's map: the extraction waits for it on the device
  if (g->merged_pending && hipStreamWaitEvent(ms, g->ev_merged, 0) != hipSuccess) return group_fail(g, "hipStreamWaitEvent", hipGetLastError());
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (g->profile) { t0 = group_event(g); t1 = group_event(g); if (t0) hipEventRecord(t0, ms); }
  const int rc = tsd_occupancy_dev_async(g->ctx[i], g->d_member[i], params->inflate, params->inflate_factor);
  if (rc != TSD_OK) {
    g->err = tsd_last_error(g->ctx[i]);
    if (t0) g->pool.push_back(t0);
    if (t1) g->pool.push_back(t1);
    return rc;
  }
  if (t0 && t1) { hipEventRecord(t1, ms); g->pending.push_back({t0, t1, false}); }
  if (hipEventRecord(g->ev_extracted[i], ms) != hipSuccess) return group_fail(g, "hipEventRecord", hipGetLastError());
  g->extracted_pending[i] = 1;
  return TSD_OK;
}

int tsd_group_member_map_upload(tsd_group* g, int i, const int8_t* map_host)
{
  if (!g || i < 0 || i >= g->n || !map_host) return TSD_E_ARG;
  if (hipSetDevice(g->device) != hipSuccess) return group_fail(g, "hipSetDevice", hipGetLastError());
  if (g->extracted_pending[i] && hipStreamWaitEvent(g->gstream, g->ev_extracted[i], 0) != hipSuccess)
    return group_fail(g, "hipStreamWaitEvent", hipGetLastError());
  const hipError_t e = hipMemcpyAsync(g->d_member[i], map_host, (size_t)g->side[i] * (size_t)g->side[i], hipMemcpyHostToDevice, g->gstream);
  if (e != hipSuccess) return group_fail(g, "hipMemcpyAsync", e);
  return TSD_OK;
}

int tsd_group_merge_maps_begin(tsd_group* g, const void* const* member_maps_dev, int8_t* merged_host)
{
  if (!g) return TSD_E_ARG;
  GroupArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int i = 0; i < g->n; i++) {
    const void* p = member_maps_dev ? member_maps_dev[i] : g->d_member[i];
    if (!p || (reinterpret_cast<uintptr_t>(p) & 15u)) { g->err = "a member map is NULL or not 16-byte aligned"; return TSD_E_ARG; }
    a.m[i] = GroupMember{static_cast<const int8_t*>(p), g->ox[i], g->oy[i], g->side[i], g->side[i]};
  }
  if (hipSetDevice(g->device) != hipSuccess) return group_fail(g, "hipSetDevice", hipGetLastError());
  for (int i = 0; i < g->n; i++)
    if (g->extracted_pending[i]) {
      if (hipStreamWaitEvent(g->gstream, g->ev_extracted[i], 0) != hipSuccess) return group_fail(g, "hipStreamWaitEvent", hipGetLastError());
      g->extracted_pending[i] = 0;
    }
  a.out = g->d_merged; a.count = g->d_count; a.W = g->W; a.H = g->H; a.n = g->n; a.chunks = (g->W + 15) / 16;
  hipError_t e = hipMemsetAsync(g->d_count, 0, kCountBytes, g->gstream);
  if (e != hipSuccess) return group_fail(g, "hipMemsetAsync", e);
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (g->profile) { t0 = group_event(g); t1 = group_event(g); if (t0) hipEventRecord(t0, g->gstream); }
  const unsigned long long pieces = (unsigned long long)a.chunks * (unsigned long long)g->H;      // <= 2^28
  const unsigned blocks = (unsigned)((pieces + 255) / 256);
  if (g->W % 16 == 0) hipLaunchKernelGGL(k_group_merge<true>, dim3(blocks), dim3(256), 0, g->gstream, a);
  else hipLaunchKernelGGL(k_group_merge<false>, dim3(blocks), dim3(256), 0, g->gstream, a);
  e = hipGetLastError();
  if (e != hipSuccess) { if (t0) g->pool.push_back(t0); if (t1) g->pool.push_back(t1); return group_fail(g, "k_group_merge", e); }
  if (t0 && t1) { hipEventRecord(t1, g->gstream); g->pending.push_back({t0, t1, true}); }
  if (hipEventRecord(g->ev_merged, g->gstream) != hipSuccess) return group_fail(g, "hipEventRecord", hipGetLastError());
  g->merged_pending = true;
  e = hipMemcpyAsync(g->h_count, g->d_count, kCountBytes, hipMemcpyDeviceToHost, g->gstream);
  if (e == hipSuccess && merged_host)
    e = hipMemcpyAsync(merged_host, g->d_merged, (size_t)g->W * (size_t)g->H, hipMemcpyDeviceToHost, g->gstream);
  if (e != hipSuccess) return group_fail(g, "hipMemcpyAsync", e);
  return TSD_OK;
}

int tsd_group_merge_begin(tsd_group* g, const tsd_map_params* params, int8_t* merged_host)
{
  if (!g || !params) return TSD_E_ARG;
  for (int i = 0; i < g->n; i++) {
    const int rc = tsd_group_extract_begin(g, i, params);
    if (rc != TSD_OK) return rc;
  }
  return tsd_group_merge_maps_begin(g, nullptr, merged_host);
}

int tsd_group_merge_wait(tsd_group* g, int* n_occupied)
{
  if (!g) return TSD_E_ARG;
  if (hipSetDevice(g->device) != hipSuccess) return group_fail(g, "hipSetDevice", hipGetLastError());
  const hipError_t e = hipStreamSynchronize(g->gstream);
  if (e != hipSuccess) return group_fail(g, "hipStreamSynchronize", e);
  if (n_occupied) {
    int n = 0;
    for (int k = 0; k < GROUP_COUNT_SHARDS; k++) n += g->h_count[k * GROUP_COUNT_STRIDE];
    *n_occupied = n;
  }
  return TSD_OK;
}

int tsd_group_profile(tsd_group* g, int on)
{
  if (!g) return TSD_E_ARG;
  g->profile = on != 0;
  return TSD_OK;
}

int tsd_group_merge_times(tsd_group* g, double* extract_ms_total, double* merge_ms_total, int* merges)
{
  if (!g) return TSD_E_ARG;
  if (hipSetDevice(g->device) != hipSuccess) return group_fail(g, "hipSetDevice", hipGetLastError());
  for (auto& t : g->pending) {
    float ms = 0.f;
    if (hipEventSynchronize(t.t1) == hipSuccess && hipEventElapsedTime(&ms, t.t0, t.t1) == hipSuccess) {
      if (t.merge) { g->merge_ms += (double)ms; g->merges_timed++; }
      else g->extract_ms += (double)ms;
    }
    g->pool.push_back(t.t0); g->pool.push_back(t.t1);
  }
  g->pending.clear();
  if (extract_ms_total) *extract_ms_total = g->extract_ms;
  if (merge_ms_total) *merge_ms_total = g->merge_ms;
  if (merges) *merges = g->merges_timed;
  return TSD_OK;
}

}  // extern "C"
