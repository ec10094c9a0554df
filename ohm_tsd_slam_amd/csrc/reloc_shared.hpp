// reloc_shared.hpp -- what the two pose-lattice searches share: relocalisation of a scan (reloc.hip, tsd_relocalize) and alignment of
// a map's surface points (align.hip, tsd_align_points / tsd_map_align).  The look-up loop of a candidate's score exists once, here; the
// peak kernels and their launcher live in reloc.hip and are called from both.
#pragma once
#include "capi_internal.hpp"

namespace tsd {

constexpr int RELOC_WAVES = 4;             // rotations a workgroup has in flight
constexpr int RELOC_BATCH = 4;             // look-ups per lane in flight together
constexpr int RELOC_MIN_BLOCKS = 2048;     // a lattice of few positions is cut along its rotations until the launch has about this many workgroups
constexpr unsigned int RELOC_ONE = 1048576u;    // 2^20: the weight of a point that lies exactly on a surface
constexpr size_t RELOC_KEEP_CANDIDATES = (size_t)1 << 23;   // a score volume up to this (32 MiB) stays with the context for the next search
constexpr int PK_KEEP = TSD_RELOC_MAX_PEAKS;

struct RelocLattice { double x0, y0, step; int nx, ny, ntheta; };

// One lane's share of a candidate's score: the points lane, lane + 64, .. of the P points staged in LDS ([P] x | [P] y), carried to the
// pose (c, s, tx, ty), RELOC_BATCH look-ups in flight with the tile flag and the four cells of each issued together (ld_pinned /
// load_quad: not behind the flag test).  Integer terms: the wave's sum of these does not depend on its order.
__device__ __forceinline__ unsigned int reloc_lane_score(const GridDev& g, const double* s_pts, int P, int lane, double c, double s,
                                                         double tx, double ty)
{
  unsigned int acc = 0u;
  for (int i0 = 0; i0 < P; i0 += 64 * RELOC_BATCH) {
    uint8_t fl[RELOC_BATCH]; Quad qv[RELOC_BATCH]; double wx[RELOC_BATCH], wy[RELOC_BATCH]; bool inside[RELOC_BATCH];
#pragma unroll
    for (int b = 0; b < RELOC_BATCH; b++) {
      const int i = i0 + 64 * b + lane, ic = i < P ? i : 0;
      const double px = s_pts[ic], py = s_pts[P + ic];
      const double x = (c * px - s * py) + tx;
      const double y = (s * px + c * py) + ty;
      int p = 0, lx = 0, ly = 0; double dx = 0.0, dy = 0.0;
      inside[b] = coord2cell(g, x, y, p, lx, ly, dx, dy) && i < P;
      if (!inside[b]) { p = 0; lx = 0; ly = 0; }
      fl[b] = ld_pinned(&g.flags[p]);
      qv[b] = load_quad(g.tsd + (size_t)p * TILE_STRIDE, lx, ly);
      wx[b] = fabs((x - dx) * g.inv_cs); wy[b] = fabs((y - dy) * g.inv_cs);
    }
#pragma unroll
    for (int b = 0; b < RELOC_BATCH; b++) {
      // TsdGrid::interpolateBilinear (TsdGrid.h:284-304), interpolate_bilinear's expression
      const double v = qv[b].t00 * (1. - wy[b]) * (1. - wx[b]) + qv[b].t10 * wy[b] * (1. - wx[b])
                     + qv[b].t01 * (1. - wy[b]) * wx[b] + qv[b].t11 * wy[b] * wx[b];
      const bool ok = inside[b] && fl[b] != 0 && !isnan(v);
      acc += ok ? RELOC_ONE - (unsigned int)rint(fabs(v) * 1048576.0) : 0u;
    }
  }
  return acc;
}

// how a lattice of nx * ny positions and nt rotations is cut into workgroups of RELOC_WAVES waves: (rotations per workgroup, grid.y)
inline void reloc_cut(int nx, int ny, int nt, int& rot_per_block, int& blocks_y)
{
  const long long positions = (long long)nx * ny;
  long long cuts = (RELOC_MIN_BLOCKS + positions - 1) / positions;                 // along the rotations, whole rounds of RELOC_WAVES at least
  cuts = std::max<long long>(1, std::min<long long>(cuts, (nt + RELOC_WAVES - 1) / RELOC_WAVES));
  cuts = std::min<long long>(cuts, 65535);
  rot_per_block = (int)((nt + cuts - 1) / cuts);
  blocks_y = (nt + rot_per_block - 1) / rot_per_block;
}

// ---- reloc.hip's host side, shared with align.hip ----
// the context's search buffers: room for `rotations` table entries and (candidates > 0) a score volume of tsd_ctx::reloc
int reloc_ensure(tsd_ctx* ctx, size_t rotations, size_t candidates);
// the two peak kernels on the context's stream over a volume on the device; the merged keys (score << 32 | ~idx) and their count
// arrive in ctx->reloc.h_keys[0 .. PK_KEEP] once the stream is waited for, and stay in reloc_merged_keys(ctx) on the device
int launch_reloc_peaks(tsd_ctx* ctx, const uint32_t* d_scores, int nx, int ny, int nt, int wraps, int K);
const unsigned long long* reloc_merged_keys(const tsd_ctx* ctx);
bool reloc_lattice_ok(int nx, int ny, int nt);
bool reloc_lattice_fits(int nx, int ny, int nt);
double reloc_reach(const GridDev& g);
bool reloc_lattice_near(const GridDev& g, double a0, int n, double step);
bool reloc_scan_in_flight(const tsd_ctx* ctx);

}  // namespace tsd
