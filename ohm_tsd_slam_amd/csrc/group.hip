// group.hip -- the same-device merge group of include/tsd_hip.h (tsd_group_*): N grid contexts of ONE process on ONE GPU, each shifted by
// whole cells, merged into one int8 occupancy map by a local kernel -- the signed maximum ncclAllReduce(int8, max) gives across GPUs
// (comm.hip), without RCCL.  Part of libtsd_hip.so; uses the contexts only through the public C ABI (tsd_stream,
// tsd_occupancy_dev_async), like comm.hip does.  A group made by tsd_group_create_rigid is the same group with its members placed by
// rigid transforms: same buffers, events and ordering, k_group_merge_rigid in k_group_merge's place.
//
// Both kernels share the step per member and 16-byte piece (take_shifted), the end (store_piece, count_flush) and the arguments
// (group_args); both constructors share group_new and one form of placement: the window and, per member, T, `whole`, ox / oy.
//
// Ordering (events only; nothing waits on the host before tsd_group_merge_wait, nothing spins on the device):
//   member i's stream :  [wait ev_merged]  extraction into d_member[i]  record ev_extracted[i]
//   group stream      :  wait ev_extracted[*]  clear count  k_group_merge  record ev_merged  copy count (+ map) to the host
// The group's stream is non-blocking and created before anything else touches the device: the legacy NULL stream stays unused (it
// would take one of the few hardware queues the scans' streams are mapped onto, see comm.hip).
#include <hip/hip_runtime.h>

#include <cmath>
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

// One member record and one argument struct, filled by group_args() for either kernel
struct GroupMember {
  const int8_t* map;      // side * side bytes, row = y, 16-byte aligned, side a multiple of 16
  int side;
  int whole;              // T is a whole-cell shift: the member's cell (x, y) is the window's cell (x + ox, y + oy)
  int ox, oy;
  double c, s, tx, ty;    // T = [c -s tx; s c ty]: the member's grid coordinates (metres) into the frame
};
struct GroupArgs {        // by value: the member table is read with scalar loads from the kernel-argument segment
  int8_t* out;            // W * H bytes, row = y
  int* count;             // GROUP_COUNT_SHARDS counters, one per 128-byte line: their sum += cells equal to 100
  int W, H, n;
  int x0, y0, chunks;     // (x0, y0): the window's corner in frame cells; chunks: 16-byte pieces per output row, (W + 15) / 16
  double cs;
  GroupMember m[TSD_GROUP_MAX];
};
static_assert(sizeof(GroupArgs) <= 4096, "the kernel-argument segment holds 4 KiB");
// k_group_merge takes the part of GroupArgs it reads, 24 bytes per member.  Its lanes walk the table with one dependent pair of scalar
// loads per member, and with the 56-byte records -- the same instructions, the stride apart -- it measured 0.2 / 0.9 us slower at
// N = 2 / 8 (15.7 -> 15.9, 31.0 -> 32.0 us; profiles/group_refactor_ab.txt).
struct ShiftArgs {
  int8_t* out;
  int* count;
  int W, H, n, chunks;
  struct Member { const int8_t* map; int side, ox, oy, reserved; } m[TSD_GROUP_MAX];
  explicit ShiftArgs(const GroupArgs& a) : out(a.out), count(a.count), W(a.W), H(a.H), n(a.n), chunks(a.chunks)
  {
    for (int i = 0; i < TSD_GROUP_MAX; i++) m[i] = Member{a.m[i].map, a.m[i].side, a.m[i].ox, a.m[i].oy, 0};
  }
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

// The step for one member and one 16-byte piece of window row y that starts at column x0 (a multiple of 16): the member's bytes go
// into the accumulator, the bytes it covers into cov.  One aligned 16-byte load (x offset a multiple of 16) or two aligned 16-byte
// loads funnelled by the offset's low four bits (the same shift in every lane: member rows and output pieces both start on multiples
// of 16); a member that does not cover the row costs a scalar compare.
__device__ __forceinline__ void take_shifted(Acc4& acc, u32x4& cov, const int8_t* map, int side, int ox, int oy, int y, int x0)
{
  const int my = y - oy, mx0 = x0 - ox;
  if ((unsigned)my >= (unsigned)side || mx0 <= -16 || mx0 >= side) return;
  const int8_t* row = map + (size_t)my * (size_t)side;
  const int s = (-ox) & 15;                     // = mx0 & 15, from scalars only: uniform
  const int b0 = mx0 - s;                       // the aligned 16 bytes that hold the piece's first byte: -16 <= b0 < side
  if (s == 0) {                                 // (then mx0 = b0 >= 0: the piece is one whole aligned block of the member)
    acc.take(*reinterpret_cast<const u32x4*>(row + b0));
    cov = (u32x4)(~0u);
    return;
  }
  const bool in0 = b0 >= 0, in1 = b0 + 16 < side;
  u32x4 lo = (u32x4)(0u), hi = (u32x4)(0u);
  if (in0) lo = *reinterpret_cast<const u32x4*>(row + b0);
  if (in1) hi = *reinterpret_cast<const u32x4*>(row + b0 + 16);
  u32x4 v = funnel16(lo, hi, s);
  if (in0 && in1) { acc.take(v); cov = (u32x4)(~0u); return; }
  // the member ends inside this piece: the bytes beyond it take the identity and stay uncovered
  const u32x4 c = funnel16(in0 ? (u32x4)(~0u) : (u32x4)(0u), in1 ? (u32x4)(~0u) : (u32x4)(0u), s);
  acc.take((v & c) | ((u32x4)(0x80808080u) & ~c));
  cov |= c;
}

// Both kernels' end, part one: the piece of window row y at column x0 is stored, what no member covers as -1; returns how many of
// the stored bytes equal 100.  ROWS16: W is a multiple of 16 -- every piece is whole and its store is one aligned 16-byte store.
template <bool ROWS16>
__device__ __forceinline__ int store_piece(int8_t* out, int W, int y, int x0, const Acc4& acc, u32x4 cov)
{
  u32x4 r;
#pragma unroll
  for (int k = 0; k < 4; k++) r[k] = acc.dword(k) | ~cov[k];            // uncovered: 0x80 | 0xFF = -1
  int8_t* o = out + (size_t)y * (size_t)W + (size_t)x0;
  int n100 = 0;
  if (ROWS16 || x0 + 16 <= W) {
    if (ROWS16) *reinterpret_cast<u32x4*>(o) = r;
    else *reinterpret_cast<u32x4_u*>(o) = r;
#pragma unroll
    for (int k = 0; k < 4; k++) n100 += count100(r[k]);
  } else {                                       // the row's last, partial piece
    for (int j = 0; x0 + j < W; j++) {
      const int8_t b = (int8_t)(r[j >> 2] >> (8 * (j & 3)));
      o[j] = b;
      n100 += b == 100;
    }
  }
  return n100;
}

// Part two: the wave's sum of n100 goes to the counter that the wave's index selects, one atomic per wave at most
__device__ __forceinline__ void count_flush(int* count, unsigned wave, int n100)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n100 += __shfl_down(n100, off, 64);
  if ((threadIdx.x & 63) == 0 && n100) atomicAdd(count + (wave & (GROUP_COUNT_SHARDS - 1)) * GROUP_COUNT_STRIDE, n100);
}

// One lane per 16 bytes of an output row; per lane take_shifted() for every member.  -128 is the maximum's identity, and since -128 is
// also a legal map value the covered bytes are tracked beside it: what no member covers becomes -1.
template <bool ROWS16>
__global__ void __launch_bounds__(256) k_group_merge(const ShiftArgs a)
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
    for (int i = 0; i < a.n; i++) take_shifted(acc, cov, a.m[i].map, a.m[i].side, a.m[i].ox, a.m[i].oy, y, x0);
    n100 = store_piece<ROWS16>(a.out, a.W, y, x0, acc, cov);
  }
  count_flush(a.count, (blockIdx.x << 2) | (threadIdx.x >> 6), n100);
}

// ---- members under rigid transforms (tsd_group_create_rigid; the rule is stated in include/tsd_hip.h) ------------------------------
// A workgroup owns 64 x 64 window cells.  Their back-projected centres span at most 63 (|c| + |s|) <= 89.1 member cells per axis, the
// footprints 1.5 more: at most 91 rows of at most 7 aligned 16-byte pieces.  One spare piece per row keeps rows 4 banks apart.
constexpr int RIGID_BLOCK = 64, RIGID_ROWS = 96, RIGID_PIECES = 8, RIGID_STRIDE = RIGID_PIECES * 16 + 16;

// u, v of the header for window cell (X, Y).  Every operation is monotone in its operands after rounding as before it, so u and v are
// monotone in X and in Y: over a block of cells their extremes are taken at the block's corners, exactly.
__device__ __forceinline__ double rigid_centre(int k0, int K, double cs) { return ((double)(k0 + K) + 0.5) * cs; }

// One lane per 16 cells of a window row, four lanes per row, 64 rows per workgroup.  Per member: the box of member cells the block's
// footprints can touch, from the block's four corners (wave-uniform); a member it misses costs that and nothing else.  Otherwise the
// box is staged in LDS with aligned 16-byte loads (take_shifted's loads) and every lane takes its cells' footprint maxima from there:
// a wave walking a window row walks a slanted line through the member, up to 64 |s| rows of it, a few bytes from each.
// A member whose transform is a whole-cell shift (the frame's owner, as a rule) takes k_group_merge's step instead: with c = 1, s = 0
// and a translation within 1e-6 cells of whole cells, u and v lie within 2e-6 of (cell + 0.5), a quarter cell from both thresholds,
// so the footprint is that one cell -- no fp64, no LDS (measured: profiles/group_merge_rigid.txt).
template <bool ROWS16>
__global__ void __launch_bounds__(256) k_group_merge_rigid(const GroupArgs a)
{
  __shared__ __attribute__((aligned(16))) int8_t tile[RIGID_ROWS * RIGID_STRIDE];
  const int bX = (int)blockIdx.x * RIGID_BLOCK, bY = (int)blockIdx.y * RIGID_BLOCK;
  const int Y = bY + (int)(threadIdx.x >> 2), X0 = bX + (int)(threadIdx.x & 3u) * 16;
  const bool live = Y < a.H && X0 < a.W;
  const double cs = a.cs;
  const double py = rigid_centre(a.y0, Y, cs);
  Acc4 acc;
  acc.init();
  u32x4 cov = (u32x4)(0u);
  for (int i = 0; i < a.n; i++) {
    const int side = a.m[i].side;
    if (a.m[i].whole) {
      if (live) take_shifted(acc, cov, a.m[i].map, side, a.m[i].ox, a.m[i].oy, Y, X0);
      continue;
    }
    const double c = a.m[i].c, s = a.m[i].s, tx = a.m[i].tx, ty = a.m[i].ty;
    int lox = INT32_MAX, loy = INT32_MAX, hix = INT32_MIN, hiy = INT32_MIN;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double dx = rigid_centre(a.x0, bX + ((k & 1) ? RIGID_BLOCK - 1 : 0), cs) - tx;
      const double dy = rigid_centre(a.y0, bY + ((k & 2) ? RIGID_BLOCK - 1 : 0), cs) - ty;
      const double u = (c * dx + s * dy) / cs, v = (c * dy - s * dx) / cs;
      lox = min(lox, (int)ceil(u - 1.25)); hix = max(hix, (int)floor(u + 0.25));
      loy = min(loy, (int)ceil(v - 1.25)); hiy = max(hiy, (int)floor(v + 0.25));
    }
    lox = __builtin_amdgcn_readfirstlane(max(lox, 0)); hix = __builtin_amdgcn_readfirstlane(min(hix, side - 1));
    loy = __builtin_amdgcn_readfirstlane(max(loy, 0)); hiy = __builtin_amdgcn_readfirstlane(min(hiy, side - 1));
    if (lox > hix || loy > hiy) continue;        // the block misses the member (uniform: every lane computed the same box)
    const int ax = lox & ~15;
    const int pieces = min(((hix - ax) >> 4) + 1, RIGID_PIECES), rows = min(hiy - loy + 1, RIGID_ROWS);
    __syncthreads();                             // the previous member's reads of the tile
    const int8_t* src = a.m[i].map + (size_t)loy * (size_t)side + (size_t)ax;
    for (int k = (int)threadIdx.x; k < rows * pieces; k += 256) {
      const int r = k / pieces, p = k - r * pieces;
      *reinterpret_cast<u32x4*>(tile + r * RIGID_STRIDE + p * 16) = *reinterpret_cast<const u32x4*>(src + (size_t)r * (size_t)side + p * 16);
    }
    __syncthreads();
    if (!live) continue;
    const double dy = py - ty, sdy = s * dy, cdy = c * dy;
    const int xmax = ax + pieces * 16 - 1, ymax = loy + rows - 1;
    u32x4 val = (u32x4)(0u), msk = (u32x4)(0u);  // the member's 16 values (-128, the maximum's identity, where it does not cover) and the bytes it covers
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const double dx = rigid_centre(a.x0, X0 + j, cs) - tx;
      const double u = (c * dx + sdy) / cs, v = (cdy - s * dx) / cs;
      int kx0 = max((int)ceil(u - 1.25), 0), kx1 = min((int)floor(u + 0.25), side - 1);
      int ky0 = max((int)ceil(v - 1.25), 0), ky1 = min((int)floor(v + 0.25), side - 1);
      int m = -128;
      if (kx0 <= kx1 && ky0 <= ky1) {            // (otherwise the footprint lies outside the member)
        // inside the staged box by the corners' argument; clamped all the same, so that no index can leave the tile
        kx0 = min(max(kx0, ax), xmax) - ax; kx1 = min(max(kx1, ax), xmax) - ax;
        const int8_t* r0 = tile + (min(max(ky0, loy), ymax) - loy) * RIGID_STRIDE;
        const int8_t* r1 = tile + (min(max(ky1, loy), ymax) - loy) * RIGID_STRIDE;
        m = max(max((int)r0[kx0], (int)r0[kx1]), max((int)r1[kx0], (int)r1[kx1]));
        msk[j >> 2] |= 0xFFu << (8 * (j & 3));
      }
      val[j >> 2] |= (uint32_t)(uint8_t)m << (8 * (j & 3));
    }
    acc.take(val);
    cov |= msk;
  }
  const int n100 = live ? store_piece<ROWS16>(a.out, a.W, Y, X0, acc, cov) : 0;
  count_flush(a.count, ((blockIdx.y * gridDim.x + blockIdx.x) << 2) | (threadIdx.x >> 6), n100);
}

}  // namespace

struct tsd_group {
  int n = 0, device = 0;
  // the placement, one form for every group: the window, W x H cells with its corner at (x0, y0) in frame cells (the offsets' frame of
  // tsd_group_create), and per member its transform into the frame, whether that is a whole-cell shift and, where it is, the shift
  int W = 0, H = 0, x0 = 0, y0 = 0;
  bool rigid = false;                          // k_group_merge_rigid is launched (tsd_group_create_rigid), k_group_merge otherwise
  std::vector<double> T;                       // 9 per member
  std::vector<int> whole, ox, oy;              // T[i] is a whole-cell shift: ox / oy hold it, relative to the window's corner
  std::vector<tsd_ctx*> ctx;
  std::vector<int> side;                       // cells per side of each member
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

static const char kOutOfRange[] = "a member's size or offset is out of range";

// what either constructor asks before it looks at a context; the refusal's text or nullptr
static const char* members_listed(int n, tsd_ctx* const* ctxs)
{
  if (n < 1 || n > TSD_GROUP_MAX) return "the number of members must be 1 .. 64";
  if (!ctxs) return "no contexts";
  for (int i = 0; i < n; i++) if (!ctxs[i]) return "a member context is NULL";
  return nullptr;
}

// The one constructor: the checks of the members and of an explicit window (worded as tsd_group_create's for either caller), then
// place(g) -- the caller's placement of the checked members: T, whole, ox / oy and, for a bounding box, the window; it returns a
// refusal's text or nullptr --, then every device object.  Nothing before the device objects touches the HIP runtime.
template <class Place>
static tsd_group* group_new(int n, tsd_ctx* const* ctxs, int width, int height, Place place)
{
  auto refuse = [](const char* what) -> tsd_group* { std::fprintf(stderr, "tsd_group_create: %s\n", what); return nullptr; };
  if (const char* what = members_listed(n, ctxs)) return refuse(what);
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
  g->n = n; g->device = device; g->W = width; g->H = height;
  g->ctx.assign(ctxs, ctxs + n);
  g->T.assign((size_t)9 * (size_t)n, 0.0); g->whole.assign(n, 0); g->ox.assign(n, 0); g->oy.assign(n, 0); g->side.resize(n);
  const char* what = nullptr;
  for (int i = 0; i < n && !what; i++) {
    g->side[i] = tsd_cells(ctxs[i]);
    if (g->side[i] <= 0 || g->side[i] % 16 != 0) what = kOutOfRange;
  }
  if (!what) what = place(*g);
  if (what) { delete g; return refuse(what); }
  // ---- device objects; the group's stream first
  auto fail = [&](const char* step) -> tsd_group* { group_release(g); return refuse(step); };
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

// the kernels' arguments from the placement and the members' maps (NULL: the group's own buffers)
static int group_args(tsd_group* g, const void* const* member_maps_dev, GroupArgs& a)
{
  std::memset(&a, 0, sizeof(a));
  a.out = g->d_merged; a.count = g->d_count; a.W = g->W; a.H = g->H; a.n = g->n; a.chunks = (g->W + 15) / 16;
  a.x0 = g->x0; a.y0 = g->y0; a.cs = tsd_cell_size(g->ctx[0]);
  for (int i = 0; i < g->n; i++) {
    const void* p = member_maps_dev ? member_maps_dev[i] : g->d_member[i];
    if (!p || (reinterpret_cast<uintptr_t>(p) & 15u)) { g->err = "a member map is NULL or not 16-byte aligned"; return TSD_E_ARG; }
    const double* t = &g->T[(size_t)9 * (size_t)i];
    a.m[i] = GroupMember{static_cast<const int8_t*>(p), g->side[i], g->whole[i], g->ox[i], g->oy[i], t[0], t[3], t[2], t[5]};
  }
  return TSD_OK;
}

extern "C" {

tsd_group* tsd_group_create(int n, tsd_ctx* const* ctxs, const int32_t* cell_off_xy, int width, int height)
{
  // every member a whole-cell shift; the bounding box's corner is the smallest offsets
  return group_new(n, ctxs, width, height, [&](tsd_group& g) -> const char* {
    const double cs = tsd_cell_size(ctxs[0]);
    int64_t lo_x = INT64_MAX, lo_y = INT64_MAX, hi_x = INT64_MIN, hi_y = INT64_MIN;
    for (int i = 0; i < n; i++) {
      const int64_t x = cell_off_xy ? cell_off_xy[2 * i] : 0, y = cell_off_xy ? cell_off_xy[2 * i + 1] : 0;
      if (x < -(1 << 24) || x > (1 << 24) || y < -(1 << 24) || y > (1 << 24)) return kOutOfRange;
      g.whole[i] = 1; g.ox[i] = (int)x; g.oy[i] = (int)y;
      const double T[9] = {1.0, 0.0, (double)x * cs, 0.0, 1.0, (double)y * cs, 0.0, 0.0, 1.0};
      std::memcpy(&g.T[(size_t)9 * (size_t)i], T, sizeof(T));
      lo_x = x < lo_x ? x : lo_x; lo_y = y < lo_y ? y : lo_y;
      hi_x = x + g.side[i] > hi_x ? x + g.side[i] : hi_x; hi_y = y + g.side[i] > hi_y ? y + g.side[i] : hi_y;
    }
    if (width == 0) {
      if (hi_x - lo_x > TSD_GROUP_MAX_SIDE || hi_y - lo_y > TSD_GROUP_MAX_SIDE) return "the bounding box exceeds 65536 cells";
      g.x0 = (int)lo_x; g.y0 = (int)lo_y; g.W = (int)(hi_x - lo_x); g.H = (int)(hi_y - lo_y);
      for (int i = 0; i < n; i++) { g.ox[i] -= g.x0; g.oy[i] -= g.y0; }
    }
    return nullptr;
  });
}

tsd_group* tsd_group_create_rigid(int n, tsd_ctx* const* ctxs, const double* T33, int width, int height)
{
  auto refuse = [](const char* what) -> tsd_group* { std::fprintf(stderr, "tsd_group_create_rigid: %s\n", what); return nullptr; };
  // ---- the transforms and the window, ahead of the members' own checks.  Nothing here touches HIP.
  if (const char* what = members_listed(n, ctxs)) return refuse(what);
  const double cs = tsd_cell_size(ctxs[0]);
  std::vector<double> T((size_t)9 * (size_t)n);
  double lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
  for (int i = 0; i < n; i++) {
    double* t = &T[(size_t)9 * (size_t)i];
    for (int k = 0; k < 9; k++) t[k] = T33 ? T33[9 * i + k] : (k % 4 == 0 ? 1.0 : 0.0);
    for (int k = 0; k < 9; k++) if (!std::isfinite(t[k])) return refuse("a transform has an entry that is not finite");
    if (t[6] != 0.0 || t[7] != 0.0 || t[8] != 1.0) return refuse("a transform's last row is not (0, 0, 1)");
    if (std::fabs(t[0] - t[4]) > 1e-12 || std::fabs(t[1] + t[3]) > 1e-12) return refuse("a transform is no rotation (shear or reflection)");
    const double c = t[0], s = t[3];
    if (std::fabs(c * c + s * s - 1.0) > 1e-9) return refuse("a transform is no rotation (scale)");
    if (!(std::fabs(t[2] / cs) <= 16777216.0) || !(std::fabs(t[5] / cs) <= 16777216.0)) return refuse("a translation exceeds 2^24 cells");
    const double L = (double)tsd_cells(ctxs[i]) * cs;
    for (int k = 0; k < 4; k++) {
      const double x = (k & 1) ? L : 0.0, y = (k & 2) ? L : 0.0;
      const double X = (c * x - s * y) + t[2], Y = (s * x + c * y) + t[5];
      lo_x = X < lo_x ? X : lo_x; hi_x = X > hi_x ? X : hi_x;
      lo_y = Y < lo_y ? Y : lo_y; hi_y = Y > hi_y ? Y : hi_y;
    }
  }
  int x0 = 0, y0 = 0;
  if (width == 0 && height == 0) {
    const double fx0 = std::floor(lo_x / cs + 1e-9), fx1 = std::ceil(hi_x / cs - 1e-9);
    const double fy0 = std::floor(lo_y / cs + 1e-9), fy1 = std::ceil(hi_y / cs - 1e-9);
    if (!(fx1 - fx0 >= 1.0 && fx1 - fx0 <= (double)TSD_GROUP_MAX_SIDE && fy1 - fy0 >= 1.0 && fy1 - fy0 <= (double)TSD_GROUP_MAX_SIDE))
      return refuse("the bounding box exceeds 65536 cells");
    x0 = (int)fx0; y0 = (int)fy0; width = (int)(fx1 - fx0); height = (int)(fy1 - fy0);
  }
  return group_new(n, ctxs, width, height, [&](tsd_group& g) -> const char* {
    g.rigid = true; g.x0 = x0; g.y0 = y0;
    g.T.swap(T);
    // a member shifted by whole cells (within 1e-6 of a cell) is merged as tsd_group_create's members are
    for (int i = 0; i < n; i++) {
      const double* t = &g.T[(size_t)9 * (size_t)i];
      const double dx = t[2] / cs, dy = t[5] / cs, rx = std::rint(dx), ry = std::rint(dy);
      if (t[0] == 1.0 && t[4] == 1.0 && t[1] == 0.0 && t[3] == 0.0 && std::fabs(dx - rx) <= 1e-6 && std::fabs(dy - ry) <= 1e-6) {
        g.whole[i] = 1; g.ox[i] = (int)rx - x0; g.oy[i] = (int)ry - y0;
      }
    }
    return nullptr;
  });
}

int tsd_group_member_transform(const tsd_group* g, int i, double T33[9])
{
  if (!g || i < 0 || i >= g->n || !T33) return TSD_E_ARG;
  std::memcpy(T33, &g->T[(size_t)9 * (size_t)i], 9 * sizeof(double));
  return TSD_OK;
}

int tsd_group_cell_offsets(const tsd_group* g, int32_t* cell_off_xy)
{
  if (!g || !cell_off_xy) return TSD_E_ARG;
  for (int i = 0; i < g->n; i++) if (!g->whole[i]) return TSD_E_ARG;
  for (int i = 0; i < g->n; i++) { cell_off_xy[2 * i] = g->ox[i] + g->x0; cell_off_xy[2 * i + 1] = g->oy[i] + g->y0; }
  return TSD_OK;
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
  const int rc = group_args(g, member_maps_dev, a);
  if (rc != TSD_OK) return rc;
  if (hipSetDevice(g->device) != hipSuccess) return group_fail(g, "hipSetDevice", hipGetLastError());
  for (int i = 0; i < g->n; i++)
    if (g->extracted_pending[i]) {
      if (hipStreamWaitEvent(g->gstream, g->ev_extracted[i], 0) != hipSuccess) return group_fail(g, "hipStreamWaitEvent", hipGetLastError());
      g->extracted_pending[i] = 0;
    }
  hipError_t e = hipMemsetAsync(g->d_count, 0, kCountBytes, g->gstream);
  if (e != hipSuccess) return group_fail(g, "hipMemsetAsync", e);
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (g->profile) { t0 = group_event(g); t1 = group_event(g); if (t0) hipEventRecord(t0, g->gstream); }
  const unsigned long long pieces = (unsigned long long)a.chunks * (unsigned long long)g->H;      // <= 2^28
  const unsigned blocks = (unsigned)((pieces + 255) / 256);
  if (g->rigid) {
    const dim3 grid((unsigned)((g->W + RIGID_BLOCK - 1) / RIGID_BLOCK), (unsigned)((g->H + RIGID_BLOCK - 1) / RIGID_BLOCK));   // <= 1024 x 1024
    if (g->W % 16 == 0) hipLaunchKernelGGL(k_group_merge_rigid<true>, grid, dim3(256), 0, g->gstream, a);
    else hipLaunchKernelGGL(k_group_merge_rigid<false>, grid, dim3(256), 0, g->gstream, a);
  }
  else if (g->W % 16 == 0) hipLaunchKernelGGL(k_group_merge<true>, dim3(blocks), dim3(256), 0, g->gstream, ShiftArgs(a));
  else hipLaunchKernelGGL(k_group_merge<false>, dim3(blocks), dim3(256), 0, g->gstream, ShiftArgs(a));
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
