// reloc_shared.hpp -- the pose-lattice search on the TSD, which relocalisation (reloc.hip, tsd_relocalize) and map alignment (align.hip,
// tsd_align_points / tsd_map_align) both run: score every candidate of a lattice, pick the peaks, refine them.  Said once, here:
//   device  lattice_score<GATE>, the body of both score kernels (k_reloc_score = <true>, k_align_score = <false>), and the peak-key
//           codec: key <-> (score, idx), idx -> pose on a lattice
//   host    the lattice of a call (LatticeSpec) with its refusals and its rotation table, the one launch of the search
//           (launch_lattice_search, reloc.hip) and the stage events of a profiled call
// The score volume's type is tsd_ctx.hpp's ScoreVolume; each search keeps an instance of its own.
#pragma once
#include "capi_internal.hpp"

namespace tsd {

constexpr int RELOC_WAVES = 4;             // rotations a workgroup has in flight
constexpr int RELOC_BATCH = 4;             // look-ups per lane in flight together
constexpr unsigned int RELOC_ONE = 1048576u;    // 2^20: the weight of a point that lies exactly on a surface
constexpr int PK_KEEP = TSD_RELOC_MAX_PEAKS;

struct RelocLattice { double x0, y0, step; int nx, ny, ntheta; };

// One lane's share of a candidate's score: the points lane, lane + 64, .. of the P points staged in LDS ([P] x | [P] y), carried to the
// pose (c, s, tx, ty), RELOC_BATCH look-ups in flight.  Integer terms: the wave's sum of these does not depend on its order.
__device__ __forceinline__ unsigned int reloc_lane_score(const GridDev& g, const double* s_pts, int P, int lane, double c, double s,
                                                         double tx, double ty)
{
  unsigned int acc = 0u;
  for (int i0 = 0; i0 < P; i0 += 64 * RELOC_BATCH) {
    Lookup l[RELOC_BATCH];
#pragma unroll
    for (int b = 0; b < RELOC_BATCH; b++) {
      const int i = i0 + 64 * b + lane, ic = i < P ? i : 0;
      const double px = s_pts[ic], py = s_pts[P + ic];
      l[b] = lookup_issue(g, (c * px - s * py) + tx, (s * px + c * py) + ty, i < P);
    }
#pragma unroll
    for (int b = 0; b < RELOC_BATCH; b++) {
      double v;
      const bool ok = lookup_value(l[b], v);
      acc += ok ? RELOC_ONE - (unsigned int)rint(fabs(v) * 1048576.0) : 0u;
    }
  }
  return acc;
}

// The score kernels' body.  A workgroup = one lattice position (blockIdx.x) and a run of rot_per_block of its rotations (blockIdx.y),
// the coarse points -- every stride-th of pts, minus the pivot -- staged in LDS once, a wave per rotation, lanes over points.  One
// uint32 per candidate: the sum of 2^20 - rint(|tsd| * 2^20) over the look-ups that succeed.  GATE: 0 for every candidate whose
// position does not lie in seen free space (a look-up there that succeeds with a value > 0), decided by one look-up per workgroup
// whose round trip runs beside the staging.
template <bool GATE>
__device__ __forceinline__ void lattice_score(const GridDev& g, const RelocLattice& L, const double* __restrict__ pts, int P, int stride,
                                              double pvx, double pvy, const double* __restrict__ cos_sin, uint32_t* __restrict__ scores,
                                              int rot_per_block)
{
  extern __shared__ __attribute__((aligned(16))) double s_pts[];      // [P] x | [P] y, relative to the pivot
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ix = (int)blockIdx.x % L.nx, iy = (int)blockIdx.x / L.nx;
  const double tx = L.x0 + (double)ix * L.step, ty = L.y0 + (double)iy * L.step;
  Lookup gl;
  if constexpr (GATE) gl = lookup_issue(g, tx, ty);
  for (int i = threadIdx.x; i < P; i += 64 * RELOC_WAVES) {
    const size_t at = (size_t)i * (size_t)stride;
    s_pts[i] = pts[2 * at] - pvx; s_pts[P + i] = pts[2 * at + 1] - pvy;
  }
  const int k0 = (int)blockIdx.y * rot_per_block;
  const int k1 = k0 + rot_per_block < L.ntheta ? k0 + rot_per_block : L.ntheta;
  const size_t plane = (size_t)L.nx * (size_t)L.ny, at = (size_t)iy * (size_t)L.nx + (size_t)ix;
  if constexpr (GATE) {
    double gv;
    if (!(lookup_value(gl, gv) && gv > 0.0)) {                        // (the same for every thread)
      for (int k = k0 + (int)threadIdx.x; k < k1; k += 64 * RELOC_WAVES) scores[(size_t)k * plane + at] = 0u;
      return;
    }
  }
  __syncthreads();
  for (int k = k0 + wave; k < k1; k += RELOC_WAVES) {                 // (whole waves: no barrier below)
    const double c = cos_sin[2 * k], s = cos_sin[2 * k + 1];
    unsigned int acc = reloc_lane_score(g, s_pts, P, lane, c, s, tx, ty);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += (unsigned int)__shfl_down((int)acc, off, 64);
    if (lane == 0) scores[(size_t)k * plane + at] = acc;
  }
}

// the two kernels, each in its search's file; launch_lattice_search launches either
__global__ void __launch_bounds__(64 * RELOC_WAVES)
k_reloc_score(GridDev g, RelocLattice L, const double* __restrict__ pts, int P, const double* __restrict__ cos_sin,
              uint32_t* __restrict__ scores, int rot_per_block);
__global__ void __launch_bounds__(64 * RELOC_WAVES)
k_align_score(GridDev g, RelocLattice L, const double* __restrict__ pts, int P, int stride, double pvx, double pvy,
              const double* __restrict__ cos_sin, uint32_t* __restrict__ scores, int rot_per_block);

// ---- the peak keys: score << 32 | ~idx, so that a larger key is a better score, then a lower candidate index; 0 = no peak ----------------
struct Peak { unsigned int score, idx; };
__host__ __device__ inline unsigned long long peak_key(unsigned int score, unsigned int idx)
{
  return ((unsigned long long)score << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}
__host__ __device__ inline Peak peak_of(unsigned long long key)
{
  return Peak{(unsigned int)(key >> 32), 0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull)};
}
// candidate idx = (k * ny + iy) * nx + ix of lattice L with the rotation table t (on the side that calls)
struct LatticePose { double x, y, c, s; };
__host__ __device__ inline LatticePose lattice_pose(const RelocLattice& L, const double* t, unsigned int idx)
{
  const unsigned int per = (unsigned int)(L.nx * L.ny), k = idx / per, rem = idx % per, iy = rem / (unsigned int)L.nx, ix = rem % (unsigned int)L.nx;
  return LatticePose{L.x0 + (double)ix * L.step, L.y0 + (double)iy * L.step, t[2 * k], t[2 * k + 1]};
}

// ---- host: the lattice of one call -----------------------------------------------------------------------------------------------------------
// what tsd_reloc_params and tsd_align_params have in common, filled field by field from either
struct LatticeSpec { RelocLattice L; int theta_wraps; const double* cos_sin; double theta0, dtheta; int K; };
template <typename Params>
inline LatticeSpec lattice_spec(const Params& p)
{
  return LatticeSpec{RelocLattice{p.x0, p.y0, p.step_xy, p.nx, p.ny, p.ntheta}, p.theta_wraps ? 1 : 0, p.cos_sin, p.theta0, p.dtheta, p.K};
}
// a refusal in the name of the entry point `who`
inline int refuse(tsd_ctx* ctx, const char* who, int code, const char* what)
{
  return set_error(ctx, code, (std::string(who) + ": " + what).c_str(), hipSuccess);
}
// the lattice's refusals, in this order: shape >= 1, x0 / y0 / step_xy, capacity, reach, theta0 / dtheta without a table
int lattice_check(tsd_ctx* ctx, const LatticeSpec& lat, const char* who);
// the rotation table of the call (the caller's, or libm's cos / sin of theta0 + k * dtheta); false when an entry is not finite
bool lattice_table(const LatticeSpec& lat, std::vector<double>& table);
// Every lattice position within TSD_RELOC_MAX_REACH grid widths of the grid, every point within as many of the sensor / the pivot: a
// carried point then lies within a dozen grid widths, (int)floor(x / cellSize) of coord2cell is defined and equals the restatement's int64.
double reloc_reach(const GridDev& g);
bool points_in_reach(const GridDev& g, const double* points_xy, int n);     // n host points x0 y0 x1 y1 ..; NaN fails too
bool reloc_scan_in_flight(const tsd_ctx* ctx);

// ---- host: the search ------------------------------------------------------------------------------------------------------------------------
// the context's search buffers that both searches use: the scan points' block, the peak keys, room for `rotations` table entries
int reloc_ensure(tsd_ctx* ctx, size_t rotations);
// The search on the context's stream: the score kernel (gate: k_reloc_score, else k_align_score with stride and pivot) over the lattice
// with the table in ctx->reloc.d_cos_sin into `vol`, whose shape it records, then the two peak kernels.  The merged keys and their count
// arrive in ctx->reloc.h_keys[0 .. PK_KEEP] once the stream is waited for, and stay in reloc_merged_keys(ctx) on the device.
int launch_lattice_search(tsd_ctx* ctx, ScoreVolume& vol, const LatticeSpec& lat, bool gate, const double* d_pts, int P, int stride,
                          double pvx, double pvy);
const unsigned long long* reloc_merged_keys(const tsd_ctx* ctx);

// The stage events of one call, local to it: created when the context profiles, destroyed with the scope.
struct StageEvents {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t stream = nullptr;
  ~StageEvents() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
  int open(tsd_ctx* ctx, int n, const char* who)
  {
    stream = ctx->stream;
    for (int i = 0; ctx->profile && i < n; i++) {
      const hipError_t e = hipEventCreate(&ev[i]);
      if (e != hipSuccess) { ev[i] = nullptr; return set_error(ctx, TSD_E_HIP, (std::string(who) + ": hipEventCreate").c_str(), e); }
    }
    return TSD_OK;
  }
  void record(int i) { if (ev[i]) hipEventRecord(ev[i], stream); }
  // milliseconds between two recorded events into `ms`, once the later one has passed
  void measure(int from, int to, double& ms) const
  {
    float f = 0.f;
    if (ev[to] && hipEventSynchronize(ev[to]) == hipSuccess && hipEventElapsedTime(&f, ev[from], ev[to]) == hipSuccess) ms = (double)f;
  }
};

}  // namespace tsd
