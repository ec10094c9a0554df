// icp_shape.hpp -- the workgroup shape of a registration as a value: which instantiation of the kernels runs, with how many threads, how
// much LDS and how many helper workgroups.  icp_shape_for() is the only statement of that decision (DESIGN 3.3 has it as a table); the
// launchers of icp_kernels.hip reach the kernels through icp_with_shape() and nothing else.  The LDS arithmetic is the one text the
// host and the kernels share.  Plain arithmetic, no HIP: tests/icp_shape_check.cpp runs it on the CPU.
#pragma once

#include <cstddef>

#include "tsd_hip.h"

#ifdef __HIPCC__
#define ICP_HD __host__ __device__
#else
#define ICP_HD
namespace tsd { struct alignas(16) double2 { double x, y; }; }
#endif

namespace tsd {

constexpr int ICP_MAXW = 16;                    // waves per workgroup at most
constexpr int ICP_PAD = 96;                     // wrapped copies of the model at both ends of its LDS array
constexpr int ICP_HELPER_POINTS = 256;              // scene points per helper workgroup: one per lane of its waves 0-3 (one wave per SIMD)
constexpr int ICP_MAX_HELPERS = 16;
constexpr size_t ICP_TAIL_BYTES = 288;             // sizeof(IcpTail), what the kernel parks in LDS until the last step (icp_kernels.hip asserts it)

// (up to the node's shape -- 1081 beams, capacity 1088 -- the list holds every point: one pass, always)
ICP_HD inline int icp_list_cap(int cap) { return cap <= 1088 ? cap : 1024; }
// bytes of the region shared by the work list (48 B per entry), the setup staging and the transpose buffer
ICP_HD inline size_t icp_region_bytes(int cap, int threads)
{
  size_t b = 48u * (size_t)icp_list_cap(cap);
  const size_t tr = (size_t)threads * 11u * sizeof(double);      // nsum_pitch(NSUM_PTL): the wider of the two
  if (tr > b) b = tr;
  return (b + 15u) & ~(size_t)15u;
}
// a half of the reciprocal filter's slot array: a whole number of entries per thread, so that giving a half back is the same stores in every
// thread (no bound to test: a test is a branch)
ICP_HD inline int icp_slot_cap(int cap, int threads) { return (cap + threads - 1) / threads * threads; }
ICP_HD inline size_t icp_lds_base_bytes(int cap, int threads, bool normals)      // with ONE half of the slot array
{
  // the staging (cap double2 + cap int) aliases the list + result arrays: 40 * lc >= 20 * cap
  return sizeof(double2) * 2 * (size_t)cap + sizeof(double2) * 2 * ICP_PAD + sizeof(unsigned long long) * (size_t)icp_slot_cap(cap, threads) + sizeof(int) * 2 * (size_t)cap +
         icp_region_bytes(cap, threads) + sizeof(double) * (2 * ICP_MAXW * 16 + 16) + ((ICP_TAIL_BYTES + 15) & ~(size_t)15) +
         sizeof(int) * 64 + 64 + (normals ? sizeof(double2) * (size_t)cap : 0);
}
#ifdef TSD_ICP_TIMELINE
#ifndef TSD_ICP_TL_FIRST
#define TSD_ICP_TL_FIRST 19
#define TSD_ICP_TL_STEPS 4
#endif
constexpr size_t ICP_TL_BYTES = (size_t)TSD_ICP_TL_STEPS * 8 * 16 * sizeof(long long);     // the timeline build's stamp buffer behind the kernel's LDS (<= 8 waves)
#else
constexpr size_t ICP_TL_BYTES = 0;
#endif
// The reciprocal filter's slot array has two halves used by alternate steps wherever the CU's 160 KB hold them (every shape the node
// runs; not the largest point counts of tsd_icp with the point-to-line estimator's normals): see the loop.  Same rule on both sides.
ICP_HD inline int icp_slot_halves(int cap, int threads, bool normals)
{
  return icp_lds_base_bytes(cap, threads, normals) + sizeof(unsigned long long) * (size_t)icp_slot_cap(cap, threads) + ICP_TL_BYTES <= 160u * 1024u ? 2 : 1;
}
ICP_HD inline size_t icp_lds_bytes_for(int cap, int threads, bool normals = false)
{
  return icp_lds_base_bytes(cap, threads, normals) + sizeof(unsigned long long) * (size_t)icp_slot_cap(cap, threads) * (size_t)(icp_slot_halves(cap, threads, normals) - 1);
}

inline int icp_cap_for(int n)
{
  int cap = (n + 63) & ~63;
  if (cap < 64) cap = 64;
  return cap;
}

// threads of a registration of n points with R register slots per lane (four "old" waves take R blocks of 64 points each,
// younger waves one block each where the blocks left allow it)
inline int icp_threads_for(int n, int R, int maxt)
{
  int T = ((n + R - 1) / R + 63) & ~63;
  if (T < 64) T = 64;
  const int B = (n + 63) / 64;
  if (B > 4 * R) {
    int W = 4 + (B - 4 * R);
    if (W > maxt / 64) W = maxt / 64;
    if (64 * W > T) T = 64 * W;
  }
  return T;
}

// helper workgroups of a registration with `points` scene points in workgroups of T threads (see ICP_HELPER_POINTS)
inline int icp_helpers(bool enabled, int points, int T)
{
  if (!enabled) return 0;
  const int per = T < ICP_HELPER_POINTS ? T : ICP_HELPER_POINTS;
  const int h = (points + per - 1) / per;
  return h > ICP_MAX_HELPERS ? 0 : h;                // (more points than the helpers reach: the registration searches itself)
}

// Workgroup shape: R scene points per thread, T <= MAXT threads, LDS arrays of `cap` points.  One CU runs the whole registration and is
// issue bound, so few waves (per-wave reduction / control cost paid once per SIMD) win.  rc != TSD_OK: no such shape, `why` says why.
struct IcpShape { int R, MAXT, T, cap; bool ptl, node; size_t lds; int rc; const char* why; };

// n_cap points size the LDS arrays, n_thr scene points decide family and thread count (the fused scan and a batch: the beams for both;
// direct mode: the larger set and the scene).  forced: tsd_ctx::icp_shape where the caller honours TSD_ICP_SHAPE (8 = <8,256>,
// >= 64 = at least that many threads of <3,512>), else 0.  extra_lds: what the caller's kernel keeps behind the registration's LDS.
inline IcpShape icp_shape_for(int n_cap, int n_thr, bool ptl, int forced, size_t extra_lds)
{
  IcpShape s{};
  s.ptl = ptl;
  auto fail = [&s](const char* why) { s.rc = TSD_E_CAPACITY; s.why = why; return s; };
  if (n_cap > TSD_MAX_ICP_POINTS) return fail("icp points > TSD_MAX_ICP_POINTS");
  s.cap = icp_cap_for(n_cap);
  // (the experimental shapes <2,576>, <5,512> and <5,256> are gone -- measured no faster, and the first spilled 21-27 registers per lane)
  const bool three = forced != 8 && n_thr <= 3 * 512;
  s.R = three ? 3 : 8; s.MAXT = three ? 512 : 256;
  s.T = icp_threads_for(n_thr, s.R, s.MAXT);
  if (three && forced >= 64 && forced > s.T) s.T = forced;
  if (s.T > s.MAXT) return fail("icp workgroup shape");
  s.lds = icp_lds_bytes_for(s.cap, s.T, ptl) + extra_lds;
  if (s.lds > 160u * 1024u)
    return fail(ptl ? "registration does not fit the LDS of one CU (point-to-line: model normals too)" : "registration does not fit the LDS of one CU");
  // The default scanner's shape (1081 beams: capacity 1088, 512 threads, closed form) has an instantiation of its own in which the
  // capacity and the thread count are compile-time constants: the twenty offsets of the LDS layout then cost no scalar registers
  // (spilled scalars of the loop 166 -> 56; -0.7 us per registration, profiles/r5_icp_helpers_ab.txt)
  s.node = s.R == 3 && s.MAXT == 512 && !ptl && s.cap == 1088 && s.T == 512;
  return s;
}

// a batch's registrations all run in the shape of its widest sensor (`beams`); TSD_ICP_SHAPE does not reach them.  launch_icp_batch and
// the entries' helper counts (icp_batch_seed_args) both take it from here.
inline IcpShape icp_batch_shape(int beams, bool ptl) { return icp_shape_for(beams, beams, ptl, 0, 0); }

// the template arguments of k_icp / k_icp_batch for a shape (k_icp_pairs: R and MAXT only); FCAP, FT != 0: the node's compile-time layout
template <int R_, int MAXT_, bool PTL_, int FCAP_ = 0, int FT_ = 0>
struct IcpTags { static constexpr int R = R_, MAXT = MAXT_, FCAP = FCAP_, FT = FT_; static constexpr bool PTL = PTL_; };

// f(IcpTags<...>{}) for the instantiation a shape runs in: two families x two estimators (the estimator is a compile-time choice: the
// node's closed form does not pay for the other one's tenth sum) and the node's.  These five are all there are.
template <class F>
inline auto icp_with_shape(const IcpShape& s, F&& f)
{
  if (s.node) return f(IcpTags<3, 512, false, 1088, 512>{});
  if (s.R == 3) return s.ptl ? f(IcpTags<3, 512, true>{}) : f(IcpTags<3, 512, false>{});
  return s.ptl ? f(IcpTags<8, 256, true>{}) : f(IcpTags<8, 256, false>{});
}

}  // namespace tsd
