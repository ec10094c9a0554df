// push_kernels.hip -- TsdGrid::push (TsdGrid.cpp:217-284) on gfx950:
//
//   k_push_tables   (one workgroup, off the critical path in the fused scan) range-query tables of the
//                   scan: the two beam-range tests of TsdGridComponent::isInRange become O(1) look-ups.
//   k_push_classify isInRange for every tile of the launch window, one LANE per tile (range cull, four corner
//                   back-projections, table look-ups): the reference's `#pragma omp for` over all partitions
//                   (TsdGrid.cpp:228-277) without its load imbalance.  Tiles that need a workgroup go to a
//                   work list (one atomic per wave) with the beam interval their cells can project to.
//   k_push_update   one 256-thread workgroup per listed tile: scan window staged in LDS, 4 cells per thread,
//                   row-major => coalesced 8-byte RMW; beam index from a fp32 estimate proven by two fp64
//                   cross products (exact atan2 fallback); lazy TsdGridPartition::init
//                   (TsdGridPartition.cpp:88-134) folded in; TsdGridPartition::increaseEmptiness
//                   (TsdGridPartition.cpp:136-164) for EMPTY tiles.  No same-address atomics: every tile
//                   leaves a 4-byte record (what happened, cells updated) and running totals.
//   k_push_halo     TsdGrid::propagateBorders (TsdGrid.cpp:372-427) restricted to what can have
//                   changed: for every listed tile (touched, or freeFootprint's dirty mark) refresh its
//                   own halo from R/U/UR and the halos of L/D/DL that mirror its first column/row/cell.
//                   Equal to the reference's full sweep by induction (untouched pairs are already
//                   consistent).  One wave per tile.
//
// HBM-bound integer/fp64 work: no MFMA.  Roofline accounting in DESIGN.md.
#include "push_device.hpp"

namespace tsd {

__device__ __forceinline__ void
push_tables_body(const double* __restrict__ ranges, const uint8_t* __restrict__ mask, int B, char* __restrict__ buf,
                 double phi_min, double ang_res)
{
  // LDS: values (2 x Bp doubles) + two levels of both index tables (ping-pong); each finished level is
  // streamed to global memory, so 4096 beams need 96 KB whatever the number of levels
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RmqView gv = rmq_view(buf, B);
  const int Bp = gv.Bp;
  double* sA = reinterpret_cast<double*>(smem);
  double* sB = sA + Bp;
  unsigned short* lv = reinterpret_cast<unsigned short*>(sB + Bp);      // [2][2][Bp]: parity, max/min
  double* gA = const_cast<double*>(gv.A); double* gB = const_cast<double*>(gv.Bv);
  unsigned short* ginf = const_cast<unsigned short*>(gv.inf);
  unsigned short* gmax = const_cast<unsigned short*>(gv.tmax); unsigned short* gmin = const_cast<unsigned short*>(gv.tmin);
  const int tid = threadIdx.x, T = blockDim.x;
  {
    double2* gb = const_cast<double2*>(gv.bdir);
    for (int j = tid; j <= B; j += T) {
      const double beta = phi_min + ((double)j - 0.5) * ang_res;
      gb[j] = make_double2(cos(beta), sin(beta));
    }
    double2* gr = const_cast<double2*>(gv.rot);
    for (int k = tid; k < ROT_N; k += T) { const double al = (double)k * ang_res; gr[k] = make_double2(cos(al), sin(al)); }
  }
  for (int i = tid; i < B; i += T) {
    const double d = ranges[i];
    const bool mk = mask[i] != 0;
    const double a = mk ? d : -__builtin_inf();
    const double b = isinf(d) ? __builtin_inf() : (mk ? d : -__builtin_inf());
    sA[i] = a; sB[i] = b; gA[i] = a; gB[i] = b;
    lv[i] = (unsigned short)i; lv[Bp + i] = (unsigned short)i;
    gmax[i] = (unsigned short)i; gmin[i] = (unsigned short)i;
  }
  if (tid < 64) {
    // prefix count of infinite readings by one wave (B <= 4096: 64 lanes x 64 beams)
    const int per = (B + 63) / 64;
    const int j0 = tid * per;
    int c = 0;
    for (int j = j0; j < j0 + per && j < B; j++) c += isinf(ranges[j]) ? 1 : 0;
    int incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off, 64); if (tid >= off) incl += t; }
    int run = incl - c;
    if (tid == 0) ginf[0] = 0;
    for (int j = j0; j < j0 + per && j < B; j++) { run += isinf(ranges[j]) ? 1 : 0; ginf[j + 1] = (unsigned short)run; }
  }
  __syncthreads();
  for (int k = 1; k < gv.levels; k++) {
    const int half = 1 << (k - 1), span = 1 << k;
    const unsigned short* pmax = lv + (size_t)((k - 1) & 1) * 2 * Bp; const unsigned short* pmin = pmax + Bp;
    unsigned short* cmax = lv + (size_t)(k & 1) * 2 * Bp; unsigned short* cmin = cmax + Bp;
    for (int j = tid; j + span <= B; j += T) {
      const unsigned short a0 = pmax[j], a1 = pmax[j + half];
      const unsigned short am = sA[a1] > sA[a0] ? a1 : a0;
      const unsigned short b0 = pmin[j], b1 = pmin[j + half];
      const unsigned short bm = sB[b1] < sB[b0] ? b1 : b0;
      cmax[j] = am; cmin[j] = bm;
      gmax[(size_t)k * Bp + j] = am; gmin[(size_t)k * Bp + j] = bm;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(1024)
k_push_tables(const double* __restrict__ ranges, const uint8_t* __restrict__ mask, int B, char* __restrict__ buf,
              double phi_min, double ang_res)
{
  push_tables_body(ranges, mask, B, buf, phi_min, ang_res);
}

// the tables of a batch of scans in ONE launch (tsd_batch_begin): workgroup x builds the tables of scan x
__global__ void __launch_bounds__(1024)
k_push_tables_batch(const TablesBatchEntry* __restrict__ entries)
{
  const TablesBatchEntry e = entries[blockIdx.x];
  push_tables_body(e.ranges, e.mask, e.beams, e.rmq, e.phi_min, e.ang_res);
}

// isInRange for every tile of the launch window, one LANE per tile (TsdGridComponent.cpp:43-124: range cull,
// four corner back-projections, the two beam-range tests as O(1) table look-ups).  Tiles that need work go
// to the list (one atomic per wave); increaseEmptiness of a tile that was never materialised is done here
// (TsdGridPartition.cpp:157-162).  Every tile of the window gets its record.
// CLASSIFY_BLOCK threads = CLASSIFY_BLOCK / 4 tiles per workgroup (four lanes each).  Two sizes: the kernel is a chain of fp64 atan2
// and dependent look-ups per wave, so a small window wants its waves spread over many compute units (256 threads), while a large one
// is bound by the list counters' atomic rate and wants as few atomics as possible (1024 threads: one pair per 256 tiles).
template <int CLASSIFY_BLOCK>
__global__ void __launch_bounds__(CLASSIFY_BLOCK)
k_push_classify(GridDev g, const PushArgs* __restrict__ a_dev, const char* __restrict__ rmq_buf,
                uint32_t* __restrict__ tile_rec, const uint8_t* __restrict__ dirty, uint32_t* __restrict__ tile_totals,
                uint32_t* __restrict__ list, PushListAux* __restrict__ list_aux, uint32_t* __restrict__ list_h,
                unsigned int* __restrict__ list_cnt /* [2][CNT_WORDS] */, int parity, int tx0, int ty0, int ntx, int nty)
{
  // FOUR lanes per tile, one corner each: the four back-projections (an fp64 atan2 apiece, by far the longest chain of this
  // kernel, and the kernel a pure latency chain: a few dozen waves on the whole chip) run side by side instead of one after
  // the other.  The quad shares everything else (same values in its four lanes); its first lane owns the tile's side effects.
  const PushArgs a = *a_dev;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int corner = lane & 3;
  const bool owner = corner == 0;
  const int t = blockIdx.x * (CLASSIFY_BLOCK / 4) + ((int)threadIdx.x >> 2);
  if (t < 16 && owner) {      // the next push's counters (nobody uses them now)
    if (t < 4) list_cnt[CNT_WORDS * (parity ^ 1) + t] = 0u;        // (U, O, H and HDONE)
    list_cnt[CNT_WORDS * (parity ^ 1) + CNT_TICKET + TICKET_STRIDE * t] = 0u;
    list_cnt[CNT_WORDS * (parity ^ 1) + CNT_TICKET + TICKET_STRIDE * (t + 16)] = 0u;
  }
  const bool in_window = t < ntx * nty;
  const int p = in_window ? (ty0 + t / ntx) * g.PX + tx0 + t % ntx : 0;
  uint32_t rec = 0u, kind = 0u;
  // the tile's state, requested before anything else: it travels in the list record of an UPDATE tile (k_push_update then needs no
  // dependent read for it) and decides the increaseEmptiness case below
  // (unconditional reads -- p is 0 outside the window: the compiler waits for a predicated read on the spot, and this kernel is a
  // chain of memory round trips: every one of them that rides along with another is ~0.6 us off the kernel)
  // ld_pinned: the optimiser otherwise SINKS a read into the conditional block of its only use, behind that block's other waits.
  const uint8_t t_flag = ld_pinned(&g.flags[p]), t_dirty = ld_pinned(&dirty[p]);      // (used inside `in_window` regions only)
  // which of the left / lower / diagonal neighbours hold data BEFORE this push: k_push_update mirrors the edge cells it changes into
  // their halos (a neighbour materialised by this very push gets its halo from k_push_halo)
  unsigned nbr = 0u;
  {
    const int ppx = p % g.PX, ppy = p / g.PX;
    const bool hL = ppx > 0, hD = ppy > 0;
    const uint8_t nL = ld_pinned(&g.flags[hL ? p - 1 : p]), nD = ld_pinned(&g.flags[hD ? p - g.PX : p]), nDL = ld_pinned(&g.flags[(hL && hD) ? p - g.PX - 1 : p]);
    nbr = ((hL && nL) ? 2u : 0u) | ((hD && nD) ? 4u : 0u) | ((hL && hD && nDL) ? 8u : 0u);
  }
  const double t_iw = ld_pinned(&g.init_weight[p]);
  TileRange tr{};                                           // (read for UPDATE tiles only)
  if (in_window && a.enabled) {
    tr = tile_in_range(g, a, rmq_view(const_cast<char*>(rmq_buf), a.beams), p, corner);
    if (tr.pass) {
      rec = REC_RANGE_PASS;
      if (tr.action == ACT_UPDATE) kind = KIND_UPDATE;
      else if (tr.action == ACT_EMPTY) {
        // TsdGridPartition::increaseEmptiness (TsdGridPartition.cpp:136-164), isInRange then returns false
        if (t_flag) kind = KIND_EMPTY;
        else {
          if (owner) {
            double v = t_iw + 1.0; v = fmin(v, MAX_WEIGHT); g.init_weight[p] = v;
            atomicAdd(&tile_totals[(size_t)p * TOT_FIELDS + 6], 1u);      // (no-return atomics: nothing waits for them; += is a read, a wait and a write)
          }
          rec |= REC_EMPTIED_UNINIT;
        }
      }
      if (owner) atomicAdd(&tile_totals[(size_t)p * TOT_FIELDS + 1], 1u);
    }
    if (kind == 0u && t_dirty != 0) { kind = KIND_HALO; rec |= REC_LISTED; }       // written by freeFootprint since the last push
  }
  if (in_window && owner && (kind == 0u || kind == KIND_HALO)) tile_rec[p] = rec;   // UPDATE / EMPTY: the workgroup writes the final record
  if (!owner) kind = 0u;
  // List slots: the waves' counts meet in LDS and ONE lane of the workgroup draws the slots of all 256 tiles with one atomic per
  // list.  (One atomic per wave, round 2: every wave of the grid hit the same word with a RETURNING atomic, and one word hands out
  // ~88 of those per microsecond -- the 2 400 waves of a cfg 3 window spent 20 us of the kernel's 21 queueing for list slots.)
  // (hb: the UPDATE tiles k_push_halo has work for -- materialised by this push, or written by freeFootprint since the last one; what a
  // plain UPDATE tile changes of its edges its own workgroup mirrors into the neighbours' halos.  That kernel walks list_h + the others.)
  const unsigned long long ub = __ballot(kind == KIND_UPDATE), ob = __ballot(kind != 0u && kind != KIND_UPDATE);
  const unsigned long long hb = __ballot(kind == KIND_UPDATE && (t_flag == 0 || t_dirty != 0));
  __shared__ unsigned int s_wu[CLASSIFY_BLOCK / 64], s_wo[CLASSIFY_BLOCK / 64], s_wh[CLASSIFY_BLOCK / 64], s_base[3];
  if (lane == 0) { s_wu[wave] = (unsigned int)__popcll(ub); s_wo[wave] = (unsigned int)__popcll(ob); s_wh[wave] = (unsigned int)__popcll(hb); }
  lds_barrier();             // (LDS only: a __syncthreads() would also sit out every wave's stores and counters above)
  if (lane == 0 && wave < 3) {
    // lane 0 of wave 0 draws the UPDATE slots, lane 0 of wave 1 the others', lane 0 of wave 2 the halo list's: the returning atomics are in flight together
    const unsigned int* cnt_w = wave == 0 ? s_wu : (wave == 1 ? s_wo : s_wh);
    unsigned int tot = 0u;
    for (int w = 0; w < CLASSIFY_BLOCK / 64; w++) tot += cnt_w[w];
    s_base[wave] = tot ? atomicAdd(&list_cnt[CNT_WORDS * parity + (wave == 0 ? CNT_U : (wave == 1 ? CNT_O : CNT_H))], tot) : 0u;
  }
  lds_barrier();
  if (ub | ob) {
    unsigned int base_u = s_base[0], base_o = s_base[1], base_h = s_base[2];
    for (int w = 0; w < wave; w++) { base_u += s_wu[w]; base_o += s_wo[w]; base_h += s_wh[w]; }
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t word = (uint32_t)p | tr.far_flag | (kind << KIND_SHIFT);
    if (kind != 0u && kind != KIND_UPDATE) list[(unsigned)g.tiles - 1u - (base_o + (unsigned)__popcll(ob & lt))] = word;
    if (kind == KIND_UPDATE && (t_flag == 0 || t_dirty != 0)) list_h[base_h + (unsigned)__popcll(hb & lt)] = word;
    if (kind == KIND_UPDATE) {
      const unsigned int slot = base_u + (unsigned)__popcll(ub & lt);
      list[slot] = word;
      // flag bit 0: the tile's _initialized; bits 1 / 2 / 3: left / lower / diagonal neighbour holds data
      static_cast<PushListAuxBody&>(list_aux[slot]) = make_update_record(g, a, word, tr, t_iw, (uint32_t)t_flag | nbr);
    }
  }
}


// One workgroup per resident slot of the device, each taking UPDATE tiles off a queue (TsdGrid.cpp:237-274).  Per tile:
//   phase A  fp32 only, 4 cells per thread: beam coordinate from the estimate above, classification, and for decided cells the
//            candidate test -- one LDS read and one compare against the beam's limit (beam_limit).  Candidates are COMPACTED into an
//            LDS list (cell | beam << 10), one LDS atomic per wave; cells within IDX_MARGIN of a boundary go to a wave-local list
//   fix-up   (same wave, no barrier) the undecided cells, densely, one lane each: the side of the boundary direction beta_jb the
//            cell's fp64 sensor-frame vector lies on -- the sign of |l| sin(angle - beta) = bx ly - by lx, good to 1e-16 where
//            the reference's own rounding chain is good to 1e-15 -- names the reference's beam unless |sin| < 1e-11; those cells,
//            and cells at the +-pi cut, take the reference's formulation itself (fp64 atan2), an out-of-line cold path
//   phase C  the exact part over the COMPACTED candidates, full waves, up to 4 cells per lane: tsd / weight reads, the IEEE
//            distance, signed distance, addTsd (TsdGridPartition.h:170-212), the writes
// SOFTWARE PIPELINE over the workgroup's tiles: the cell reads of tile n are issued, then phase A of tile n + 1 runs while they are
// in flight, then the exact part of tile n -- so a tile costs max(memory latency, phase A) + the exact arithmetic instead of their
// sum, with ONE workgroup barrier per tile.  Everything a phase hands to the next lives in LDS, double / triple buffered by tile
// number (candidate lists and distance tables x2, counters x3); the registers carried across phase A are the cells in flight.
// Tiles come off a device-wide ticket counter (the first one is the workgroup's own index): a workgroup that drew cheap tiles takes
// more of them.  Lazy TsdGridPartition::init (TsdGridPartition.cpp:88-134) is folded in (a fresh tile's old value is known:
// non-candidates get the init value from phase A / the fix-up, candidates start from it in phase C).  increaseEmptiness of
// materialised tiles (TsdGridPartition.cpp:136-164, the `other` list) follows the tile queue.
__global__ void __launch_bounds__(UPDATE_BLOCK, UPDATE_WPS)
k_push_update(GridDev g, const PushArgs* __restrict__ a_dev, const double* __restrict__ ranges,
              const uint8_t* __restrict__ mask, uint32_t* __restrict__ tile_rec, uint32_t* __restrict__ tile_totals,
              const uint32_t* __restrict__ list, const PushListAux* __restrict__ list_aux,
              unsigned int* __restrict__ list_cnt, int parity, const double2* __restrict__ bdir, const double2* __restrict__ rot,
              double* __restrict__ dbg)
{
  static_assert(UPDATE_BLOCK == 256 && UPD_CPT == 4, "phase A: 4 cells per thread, 32 x 2 cells per wave and pass");
#ifdef TSD_PUSH_STAMPS   // diagnostic build (tools/push_stamps_r3.sh): shader cycles per phase, summed over the tiles of every 8th workgroup (thread 0)
  long long st_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; long long st_t = clock64(); const long long st_w0 = wall_clock64(); int st_tiles = 0;
#define PSTAMP(i) do { const long long now_ = clock64(); st_acc[i] += now_ - st_t; st_t = now_; } while (0)
#else
#define PSTAMP(i) do {} while (0)
#endif
  unsigned int* const cntw = list_cnt + CNT_WORDS * parity;
  const unsigned int n_upd_tiles = cntw[CNT_U], n_other = cntw[CNT_O];
  const int tid = threadIdx.x, lane = tid & 63;
  // A tile's list record travels as ONE vector register per wave (lane i holds dword i of the 64-byte record) from the request to
  // the tile's turn, its boundary direction likewise: requested a tile ahead, unpacked by v_readlane when the tile starts.  (As
  // scalar loads the compiler moves the requests to the point of first use and, short of scalar registers, waits for them on the
  // spot -- two memory round trips at the head of every tile, ~1.3 us of a tile's ~7 at cfg 3.)
  auto rec_request = [&](unsigned i) { return reinterpret_cast<const uint32_t*>(list_aux + i)[lane & 31]; };
  auto rec_word = [&](uint32_t v, int k) { return (uint32_t)__builtin_amdgcn_readlane((int)v, k); };
  auto rec_unpack = [&](uint32_t v) {
    PushListAux x;
    x.entry = rec_word(v, 0); x.win = rec_word(v, 1);
    x.pw = __hiloint2double((int)rec_word(v, 3), (int)rec_word(v, 2));
    x.A = __uint_as_float(rec_word(v, 4)); x.B = __uint_as_float(rec_word(v, 5)); x.C = __uint_as_float(rec_word(v, 6)); x.D = __uint_as_float(rec_word(v, 7));
    x.lc2 = __uint_as_float(rec_word(v, 8)); x.th_c = __uint_as_float(rec_word(v, 9)); x.lcx = __uint_as_float(rec_word(v, 10)); x.lcy = __uint_as_float(rec_word(v, 11));
    x.iw = __hiloint2double((int)rec_word(v, 13), (int)rec_word(v, 12));
    x.flag = rec_word(v, 14); x.jb0 = rec_word(v, 15);
    return x;
  };
  auto bd_unpack = [&](uint32_t v) {
    double2 d;
    d.x = __hiloint2double((int)rec_word(v, 17), (int)rec_word(v, 16)); d.y = __hiloint2double((int)rec_word(v, 19), (int)rec_word(v, 18));
    return d;
  };
  const uint32_t first_v = rec_request(blockIdx.x);             // read speculatively: arrives with the list lengths and the arguments
  const PushArgs a = *a_dev;
  // ... and, for a workgroup that will take several tiles, so does the whole scan (the first STAGE_R x 256 beams: a UTM-30LX scan in
  // one round) and the rotation table: one memory round trip.  (A single-tile workgroup stages only the beams its tile can project
  // to, behind the record: 1 read per thread instead of 5 -- measured 0.7 us better at cfg 2 than staging everything up front.)
  const bool more_than_one = n_upd_tiles > gridDim.x;
  const bool stage_all = more_than_one;
  constexpr int STAGE_R = 5;
  double st_r[STAGE_R]; unsigned st_m[STAGE_R];
#pragma unroll
  for (int i = 0; i < STAGE_R; i++) { st_r[i] = 0.0; st_m[i] = 0u; }
  if (stage_all) {
#pragma unroll
    for (int i = 0; i < STAGE_R; i++) {       // (unconditional reads of a clamped index: a predicated read is waited for on the spot)
      const int j = tid + i * UPDATE_BLOCK, jc = j < a.beams ? j : 0;
      st_r[i] = ranges[jc]; st_m[i] = (unsigned)mask[jc];
    }
  }
  const double2 st_rot = rot[tid < ROT_N ? tid : 0];
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Bp = (a.beams + 3) & ~3;
  double* s_ranges = reinterpret_cast<double*>(smem);                      // [Bp]
  double* s_d2 = s_ranges + Bp;                                            // [2][2][32] by tile number & 1: (ccx - trx)^2 per column, (ccy - try)^2 per row
  double2* s_rot = reinterpret_cast<double2*>(s_d2 + 4 * TILE_DIM);        // [ROT_N] (cos, sin)(k * res)
  float* s_lim = reinterpret_cast<float*>(s_rot + ROT_N);                  // [Bp] beam_limit of every staged beam
  uint32_t* s_cand = reinterpret_cast<uint32_t*>(s_lim + Bp);              // [2][1024] candidates by tile number & 1: cell | beam << 10
  __shared__ unsigned long long s_cu[3];                                   // by tile number % 3: candidates listed (low word) | undecided cells listed (high word)
  __shared__ unsigned int s_upd[3];                                        // cells updated
  __shared__ unsigned long long s_neg[3];                                  // groups of the tile that received a negative value
  __shared__ unsigned int s_tk[4];                                         // list index of tile number n at [n & 3]
  // the tile's edge cells that this push changed (slot y: cell (0, y); slot 32 + x: cell (x, 0), x > 0): value, weight, "changed"
  // (a NaN weight = unchanged: weights are never NaN)
  __shared__ __attribute__((aligned(16))) double2 s_edge[2 * TILE_DIM];
  const double max_trunc = g.max_trunc;

  if (blockIdx.x < n_upd_tiles) {
    TileA ta;
    ta.phi_min = (float)a.phi_min; ta.inv_res = (float)a.ang_res_inv; ta.beams = a.beams;
    ta.mt = (float)max_trunc;
    ta.low2 = (float)(a.low_refl * a.low_refl) * 1.00001f;
    ta.axx = (float)(a.Pi[0] * g.cs); ta.axy = (float)(a.Pi[1] * g.cs); ta.ayx = (float)(a.Pi[3] * g.cs); ta.ayy = (float)(a.Pi[4] * g.cs);
    ta.cs2 = (float)(g.cs * g.cs);
    // the queue: tile 0 of this workgroup is its own index, the others come off its ticket head, requested two tiles ahead
    // (a grid smaller than TICKET_HEADS -- a small compute partition, a CU mask -- uses as many heads as it has workgroups: a head
    // nobody owns would leave its residue class of the list unprocessed)
    const unsigned int n_heads = gridDim.x < (unsigned)TICKET_HEADS ? gridDim.x : (unsigned)TICKET_HEADS;
    unsigned int* const head = cntw + CNT_TICKET + TICKET_STRIDE * (blockIdx.x % n_heads);
    const unsigned int head_first = gridDim.x + blockIdx.x % n_heads;
    // (the RAW counter value is carried to where the ticket is needed: nothing may consume the returning atomic early, or thread 0's
    // wave sits out a device-scope round trip in the middle of its step; csrc/Makefile switches the compiler's atomic optimiser off for
    // this file for the same reason -- it would turn the one-lane atomic into a wave scan that needs the result at once)
    auto draw = [&]() { return atomicAdd(head, 1u); };
    auto ticket_of = [&](unsigned raw) { return head_first + n_heads * raw; };
    unsigned int tk_pending = 0u;                  // (thread 0) the ticket requested during the previous step
    if (tid == 0) {
      s_tk[0] = blockIdx.x;
      s_tk[1] = more_than_one ? ticket_of(draw()) : ~0u;        // tile 1; tile n's step requests tile n + 2
    }
    // The scan is staged once per workgroup: all of it when the workgroup may take several tiles (from the reads issued at the top),
    // only the beams the tile can project to when it has a single one.  Beams outside the staged window: see phase A.
    uint32_t xc_v = first_v;                              // tile n's record
    PushListAux xc = rec_unpack(xc_v);
    int wlo = 0, whi = a.beams - 1;
    if (stage_all) {
#pragma unroll
      for (int i = 0; i < STAGE_R; i++) { const int j = tid + i * UPDATE_BLOCK; if (j <= whi) { s_ranges[j] = st_r[i]; s_lim[j] = beam_limit(st_r[i], st_m[i], ta.mt, ta.low2); } }
      // (longer scans: further rounds, every read of a round issued before its first LDS write)
      for (int j0 = STAGE_R * UPDATE_BLOCK; j0 <= whi; j0 += 4 * UPDATE_BLOCK) {
        double rr[4]; unsigned mm[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { const int j = j0 + tid + i * UPDATE_BLOCK, jc = j <= whi ? j : 0; rr[i] = ranges[jc]; mm[i] = (unsigned)mask[jc]; }
#pragma unroll
        for (int i = 0; i < 4; i++) { const int j = j0 + tid + i * UPDATE_BLOCK; if (j <= whi) { s_ranges[j] = rr[i]; s_lim[j] = beam_limit(rr[i], mm[i], ta.mt, ta.low2); } }
      }
    } else {
      wlo = (int)(xc.win & 0xFFFFu) - 1; whi = (int)(xc.win >> 16) + 1;
      if (wlo < 0) wlo = 0;
      if (whi > a.beams - 1) whi = a.beams - 1;
      for (int j0 = wlo; j0 <= whi; j0 += 4 * UPDATE_BLOCK) {      // (the usual tile, seen from outside: a few dozen beams, one round)
        double rr[4]; unsigned mm[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { const int j = j0 + tid + i * UPDATE_BLOCK, jc = j <= whi ? j : wlo; rr[i] = ranges[jc]; mm[i] = (unsigned)mask[jc]; }
#pragma unroll
        for (int i = 0; i < 4; i++) { const int j = j0 + tid + i * UPDATE_BLOCK; if (j <= whi) { s_ranges[j] = rr[i]; s_lim[j] = beam_limit(rr[i], mm[i], ta.mt, ta.low2); } }
      }
    }
    ta.wlo = wlo; ta.whi = whi;
    if (tid < ROT_N) s_rot[tid] = st_rot;
    if (tid < 3) { s_cu[tid] = 0ull; s_upd[tid] = 0u; s_neg[tid] = 0ull; }
    if (tid < 2 * TILE_DIM) s_edge[tid] = make_double2(0.0, __builtin_nan(""));
    lds_barrier();                     // scan staged, counters zeroed, first tickets in place
    PSTAMP(0);

    const unsigned ix = (unsigned)tid & 31u, iy0 = (unsigned)tid >> 5;
    const int c0 = (int)(iy0 * 32u + ix);                                  // phase A: cell k of this thread is c0 + 256 k = (ix, iy0 + 8 k)
    const float dxc = (float)ix - 16.0f;

    // ---- phase A of tile number `n` (list record `x`): fills candidate list / counters / distance tables of that tile number
    auto phase_a = [&](unsigned n, const PushListAux& x, const TileC& tc, const unsigned x0, const unsigned y0) {
      uint32_t* cand_list = s_cand + (n & 1u) * UPD_CAND_MAX;
      unsigned long long* cnt = &s_cu[n % 3u];
      const double t_init = (tc.iw > 0.0) ? 1.0 : __builtin_nan("");      // TsdGridPartition::init values (TsdGridPartition.cpp:98-120)
      // the two squares of the exact cell distance depend on the column / the row only: one lane each, once per tile
      if (tid < 2 * TILE_DIM) {
        const bool col = tid < TILE_DIM;
        const unsigned i = (unsigned)tid & 31u;
        const double cc = ((double)((col ? x0 : y0) + i) + 0.5) * g.cs;       // TsdGridPartition.cpp:127-128
        const double dw = cc - (col ? a.trx : a.try_);
        s_d2[(n & 1u) * 2 * TILE_DIM + tid] = dw * dw;
      }
      CellsA cs;
      classify_cells(ta, x, dxc, iy0, cs);
      PSTAMP(6);     // (sub-phase: d2 table, setup, classification)
      cell_limits(ta, s_lim, cs);
#pragma unroll
      for (int k = 0; k < UPD_CPT; k++) {
        cs.cand[k] = is_candidate(cs, k);
        // a freshly materialised tile: cells that addTsd will not touch get the init value here
        if (tc.fresh && !cs.cand[k] && !cs.uns[k]) st_cell(tc.T, tc.W, c0 + UPDATE_BLOCK * k, t_init, tc.iw);
#ifdef TSD_PUSH_VERIFY_INDEX   // diagnostic build: every decided cell against the exact formulation
        {
          const double ccx = ((double)(x0 + ix) + 0.5) * g.cs, ccy = ((double)(y0 + iy0 + 8u * (unsigned)k) + 0.5) * g.cs;
          const int ex = backproject(a.Pi, ccx, ccy, a.phi_min, a.ang_res_inv, a.phi_lower, a.phi_upper);
          const int index = cs.in[k] ? cs.idx[k] : -1;
          if (!cs.uns[k] && (index < 0 ? ex >= 0 : ex != index)) atomicAdd(reinterpret_cast<unsigned long long*>(dbg + 1000), 1ull);
          if (cs.uns[k]) atomicAdd(reinterpret_cast<unsigned long long*>(dbg + 1001), 1ull);
          atomicAdd(reinterpret_cast<unsigned long long*>(dbg + 1002), 1ull);
        }
#endif
      }
      PSTAMP(7);     // (sub-phase: limits, candidate test, fresh stores)
      compact_cells(cs, c0, lane, cnt, cand_list);
      PSTAMP(8);     // (sub-phase: compaction)
      if (tc.fresh) {
        // halo cells of a freshly materialised tile keep the init value until k_push_halo
        for (int h = tid; h < 2 * TILE_DIM + 1; h += UPDATE_BLOCK) {      // the halo strip: column 32, then row 32
          st_tsd(tc.T + HALO_COL + h, t_init); st_w(tc.W + HALO_COL + h, tc.iw);
        }
      }
    };
    auto tile_of = [&](const PushListAux& x) {
      TileC tc;
      tc.p = (int)(x.entry & LIST_TILE_MASK);
      tc.T = g.tsd + (size_t)tc.p * TILE_STRIDE; tc.W = g.weight + (size_t)tc.p * TILE_STRIDE;
      tc.pw = x.pw; tc.iw = x.iw; tc.fresh = (x.flag & 1u) == 0u;
      return tc;
    };

    // ---- the tile loop: phase A -> barrier -> exact part -> barrier -> record.  (Measured alternative, round 3: a software pipeline
    // that issues the cell reads of tile n, runs phase A of tile n + 1 while they are in flight and then the exact part of tile n --
    // one barrier per tile, the cells of a tile held in registers across phase A.  It removes the memory wait from the exact part
    // but needs 128 registers (4 workgroups per compute unit instead of 6) and the kernel is bound by VALU issue either way: 75.6 us
    // against 75.0 us at cfg3 / comb, 16.9 against 14.5 us at cfg2.  profiles/r3_push_update_structure.txt.)
    const double inv_max_trunc = 1.0 / max_trunc;
    unsigned i_cur = blockIdx.x, i_next = s_tk[1];        // list indices of tiles n / n + 1 (>= n_upd_tiles: none)
    uint32_t xn_v = rec_request(i_next < n_upd_tiles ? i_next : 0u);        // tile n + 1's record, in flight
    for (unsigned n = 0u; i_cur < n_upd_tiles; n++) {
      const unsigned slot = n % 3u;
      // thread 0: the ticket of tile n + 2, consumed at the end of this tile
      if (tid == 0 && more_than_one) tk_pending = draw();
      const TileC tcur = tile_of(xc);
      const unsigned x0 = (unsigned)(tcur.p % g.PX) * TILE_DIM, y0 = (unsigned)(tcur.p / g.PX) * TILE_DIM;

      phase_a(n, xc, tcur, x0, y0);
      PSTAMP(1);
      // tile n + 1's record and the ticket of tile n + 2 were requested a whole phase A ago: the wave takes delivery HERE, where that
      // costs nothing -- at their points of use (behind the exact part) the same wait would also sit out the tile's own stores
      asm volatile("" : "+v"(xn_v), "+v"(tk_pending));
      lds_barrier();
      PSTAMP(2);
      const unsigned long long cu = s_cu[slot];
      const unsigned n_cand = (unsigned)cu, n_uns = (unsigned)(cu >> 32);
      const unsigned n_tot = n_cand + n_uns;
      uint32_t* cand_list = s_cand + (n & 1u) * UPD_CAND_MAX;
      const double* d2x = s_d2 + (n & 1u) * 2 * TILE_DIM;
      const double t_init = (tcur.iw > 0.0) ? 1.0 : __builtin_nan("");
      // ---- fix-up of the tile's undecided cells (~4 % of the cells: one partly filled wave per tile), one lane each, in place: entry
      // n_cand + u of the exact part below lives at list[1023 - u] and is settled here BY THE THREAD THAT WILL READ IT there (an LDS
      // hand-off inside one lane: no barrier).  resolve_undecided names the cell's beam.
      for (unsigned u = ((unsigned)tid - n_cand) & (unsigned)(UPDATE_BLOCK - 1); u < n_uns; u += UPDATE_BLOCK) {
        const uint32_t e = cand_list[(unsigned)(UPD_CAND_MAX - 1) - u];
        const int c = (int)(e & 1023u);
        const int jbq = (int)(e >> 10);
        const double ccx = ((double)(x0 + ((unsigned)c & 31u)) + 0.5) * g.cs;   // TsdGridPartition.cpp:127-128
        const double ccy = ((double)(y0 + ((unsigned)c >> 5)) + 0.5) * g.cs;
        // (near tiles see the whole scan: beyond the LDS rotation table, the global boundary table)
        const UndecidedBeam beam = resolve_undecided(a, a_dev, xc.jb0, bd_unpack(xc_v), s_rot, bdir, ccx, ccy, jbq);
        const int index = beam.index;
#ifdef TSD_PUSH_VERIFY_INDEX
        {
          const int ex = backproject(a.Pi, ccx, ccy, a.phi_min, a.ang_res_inv, a.phi_lower, a.phi_upper);
          if (index < 0 ? ex >= 0 : ex != index) atomicAdd(reinterpret_cast<unsigned long long*>(dbg + 1003), 1ull);
          if (beam.cold) atomicAdd(reinterpret_cast<unsigned long long*>(dbg + 1004), 1ull);
        }
#endif
        bool cand = false;
        if (index >= 0) {
          const int il = min(max(index, wlo), whi);
          float lm = s_lim[il];
          asm volatile("" : "+v"(lm));
          if (__builtin_expect(il != index, 0)) { lm = beam_limit(ranges[index], (unsigned)mask[index], ta.mt, ta.low2); asm volatile("" : "+v"(lm)); }
          cand = !((float)beam.l2 > lm * 1.00001f);      // (|l|^2 from the fp64 vector here: within 1e-7 of phase A's fp32 form; the margin covers it)
        }
        if (tcur.fresh && !cand) st_cell(tcur.T, tcur.W, c, t_init, tcur.iw);
        cand_list[(unsigned)(UPD_CAND_MAX - 1) - u] = cand ? ((uint32_t)c | ((uint32_t)index << 10)) : 0xFFFFFFFFu;
      }
      PSTAMP(9);     // (sub-phase: fix-up)
      // the exact part: UPD_CB cells per lane and pass, their reads in flight together; a wave skips the cells of a pass none of its
      // lanes has (a tile's last pass is rarely full)
      unsigned long long wrote_neg = 0ull;
      unsigned n_upd = 0u;                                  // cells this WAVE updated (a scalar: population counts of the lane masks)
      const double w_meas = tcur.pw;                        // 0.01 * partition weight (TsdGridPartition.h:193-196), from the tile's record
      for (unsigned q0 = (unsigned)tid; q0 < n_tot; q0 += UPD_CB * UPDATE_BLOCK) {
        uint32_t ce[UPD_CB]; double tv[UPD_CB], wv[UPD_CB];
#pragma unroll
        for (int j = 0; j < UPD_CB; j++) {
          const unsigned q = q0 + (unsigned)(j * UPDATE_BLOCK);
          ce[j] = q < n_tot ? cand_list[q < n_cand ? q : ((unsigned)(UPD_CAND_MAX - 1) + n_cand) - q] : 0xFFFFFFFFu;
          tv[j] = t_init; wv[j] = tcur.iw;
          if (ce[j] != 0xFFFFFFFFu && !tcur.fresh) { tv[j] = ld_tsd(tcur.T + (ce[j] & 1023u)); wv[j] = ld_w(tcur.W + (ce[j] & 1023u)); }
        }
#pragma unroll
        for (int j = 0; j < UPD_CB; j++) {
          // (lanes leave the loop from the top down: the first active lane is the wave's lane 0)
          if (j > 0 && !((unsigned)__builtin_amdgcn_readfirstlane((int)q0) + (unsigned)(j * UPDATE_BLOCK) < n_tot)) break;
          const bool on = ce[j] != 0xFFFFFFFFu;
          const int c = (int)(ce[j] & 1023u);
          const int index = on ? (int)(ce[j] >> 10) : wlo;
          const int il = min(max(index, wlo), whi);
          double r = s_ranges[il];
          const double dx2 = d2x[c & 31], dy2 = d2x[TILE_DIM + (c >> 5)];
          asm volatile("" : "+v"(r));
          // (a beam outside the staged window -- rounding at the window's ends, rare: read AND delivered inside the branch.  Left to the
          // compiler, the wait for this read sits behind the branch, on every pass, as s_waitcnt vmcnt(0) -- which is also a wait for
          // the previous cell's stores)
          if (__builtin_expect(il != index, 0)) { r = ranges[index]; asm volatile("" : "+v"(r)); }
          const double dist = sqrt_normal(dx2 + dy2);                // (ccx - trx)^2 + (ccy - try)^2, then the IEEE root
          // Every cell read of the pass is taken delivery of HERE -- behind the first root, ahead of the first store.  The cells'
          // values are consumed inside branches, so left to the compiler each later use (and each reuse of their registers) is
          // guarded by s_waitcnt vmcnt(0), which on this hardware is also a wait for the stores issued in between: the second
          // cell of a pass then sits out the first cell's store round trip.
          if (j == 0) {
#pragma unroll
            for (int jj = 0; jj < UPD_CB; jj++) asm volatile("" : "+v"(tv[jj]), "+v"(wv[jj]));
          }
          double sd;
          const bool hit = cell_signed_distance(r, dist, a.low_refl, max_trunc, sd);
          bool touched = false;
          if (on && hit) touched = add_tsd(tv[j], wv[j], sd, w_meas, max_trunc, inv_max_trunc);
          n_upd += (unsigned)__popcll(__ballot(touched));
          if (touched && tv[j] < 0.0) wrote_neg |= neg_bit((unsigned)c & 31u, (unsigned)c >> 5);
          if (on && (touched || tcur.fresh)) st_cell(tcur.T, tcur.W, c, tv[j], wv[j]);
          // a changed cell of column 0 / row 0 is also a halo cell of the left / lower / diagonal neighbour: parked for the mirror pass
          // (a fresh tile's surroundings are refreshed by k_push_halo)
          if (touched && !tcur.fresh && ((c & 31) == 0 || (c >> 5) == 0))
            s_edge[(c & 31) == 0 ? (c >> 5) : TILE_DIM + (c & 31)] = make_double2(tv[j], wv[j]);
        }
      }
      if (wrote_neg) atomicOr(&s_neg[slot], wrote_neg);               // (LDS; folded into the tile's mask below)
      if (lane == 0 && n_upd) atomicAdd(&s_upd[slot], n_upd);
      if (tid == 0) s_tk[(n + 2u) & 3u] = more_than_one ? ticket_of(tk_pending) : ~0u;
      PSTAMP(3);
      lds_barrier();               // tile n done by every wave; the next ticket in place
      PSTAMP(4);
      {
      if (tid >= 64 && tid < 128) {
        // TsdGrid::propagateBorders (TsdGrid.cpp:372-427) for what THIS tile changed: its column 0 is the left neighbour's halo column,
        // its row 0 the lower neighbour's halo row, its cell (0, 0) the diagonal neighbour's corner -- written from here, 64 lanes at
        // once, instead of being gathered by k_push_halo line by line (32 lines for 32 cells).  Only where the neighbour holds data;
        // untouched cells are in place from earlier pushes.
        const int l = lane;
        const double2 e = s_edge[l == TILE_DIM ? 0 : l];                // (cell (0, 0) heads both the column and the row)
        const double2 e0 = s_edge[0];
        const unsigned nf = xc.flag >> 1;                                // bits 0 / 1 / 2: left / lower / diagonal neighbour held data before this push
        {
          // (the "unchanged" marker is built HERE from a scalar the compiler cannot hoist: as a loop invariant it was kept in four
          // vector registers, spilled, and reloaded from scratch memory once per tile)
          unsigned nan_hi = 0x7ff80000u;
          asm volatile("" : "+s"(nan_hi));
          s_edge[l] = make_double2(0.0, __hiloint2double((int)nan_hi, 0));      // (this wave's reads above precede this write: in order)
        }
        const bool f = !isnan(e.y), f0 = !isnan(e0.y);
        const size_t PXs = (size_t)g.PX;
        if (l < TILE_DIM) {
          if (f && (nf & 1u)) { const size_t o = ((size_t)tcur.p - 1) * TILE_STRIDE + HALO_COL + l; st_tsd(g.tsd + o, e.x); st_w(g.weight + o, e.y); }
        } else {
          if (f && (nf & 2u)) { const size_t o = ((size_t)tcur.p - PXs) * TILE_STRIDE + HALO_ROW + (l - TILE_DIM); st_tsd(g.tsd + o, e.x); st_w(g.weight + o, e.y); }
        }
        if (l == 0 && f0 && (nf & 4u)) { const size_t o = ((size_t)tcur.p - PXs - 1) * TILE_STRIDE + HALO_ROW + TILE_DIM; st_tsd(g.tsd + o, e0.x); st_w(g.weight + o, e0.y); }
      }
      }
      if (tid == 0) {
        // the record of tile n (this slot's counters are next used by tile n + 3: behind two more barriers)
        const unsigned cells = s_upd[slot];
        const unsigned long long nm = s_neg[slot];
        s_cu[slot] = 0ull; s_upd[slot] = 0u; s_neg[slot] = 0ull;
        uint32_t rec = REC_RANGE_PASS | REC_UPDATE | REC_LISTED;
        if (tcur.fresh) rec |= REC_NEW | (tcur.iw > 0.0 ? REC_NEW_FROM_EMPTY : 0u);
        tile_rec[tcur.p] = rec | (cells << REC_CELLS_SHIFT);
        // The tile's running totals and mask: NO-RETURN atomics (fire and forget; every tile has its own words, so nothing contends).
        uint32_t* tot = tile_totals + (size_t)tcur.p * TOT_FIELDS;
        if (nm) atomicOr(&g.negmask[tcur.p], nm);
        atomicAdd(&tot[0], cells); atomicAdd(&tot[2], 1u);
        if (tcur.fresh) { atomicAdd(&tot[3], 1u); if (tcur.iw > 0.0) atomicAdd(&tot[4], 1u); }
        if (tcur.fresh) g.flags[tcur.p] = 1;   // publish the tile
      }
      PSTAMP(10);    // (sub-phase: the tile's record)
#ifdef TSD_PUSH_STAMPS
      st_tiles++;
#endif
      // advance: the record of tile n + 2 is requested now, one tile ahead of its phase A
      i_cur = i_next; i_next = s_tk[(n + 2u) & 3u];
      xc_v = xn_v; xc = rec_unpack(xc_v); xn_v = rec_request(i_next < n_upd_tiles ? i_next : 0u);
      PSTAMP(0);
    }
  }

  // ---- the other list: increaseEmptiness of materialised tiles, all 33 x 33 cells, halo included; the average uses the NEW weight
  for (unsigned int k = blockIdx.x; k < n_other; k += gridDim.x) {
    const uint32_t entry = list[(unsigned)g.tiles - 1u - k];
    if ((entry >> KIND_SHIFT) != KIND_EMPTY) continue;
    const int p = (int)(entry & LIST_TILE_MASK);
    tsd_cell_t* __restrict__ T = g.tsd + (size_t)p * TILE_STRIDE;
    w_cell_t* __restrict__ W = g.weight + (size_t)p * TILE_STRIDE;
    for (int i = tid; i < TILE_CELLS; i += UPDATE_BLOCK) {      // (interior, halo column, halo row: offsets 0..1088)
      double t = ld_tsd(T + i), w = ld_w(W + i);
      empty_cell(t, w);
      st_cell(T, W, i, t, w);
    }
    if (tid == 0) { tile_rec[p] = REC_RANGE_PASS | REC_EMPTIED_INIT | REC_LISTED; atomicAdd(&tile_totals[(size_t)p * TOT_FIELDS + 5], 1u); }
  }
#ifdef TSD_PUSH_STAMPS
  if (threadIdx.x == 0 && (blockIdx.x & 7) == 0 && (blockIdx.x >> 3) < 256) {
    double* o = dbg + (blockIdx.x >> 3) * 8;
    PSTAMP(5);
    o[0] = (double)st_w0; o[1] = (double)wall_clock64(); o[2] = (double)st_tiles;
    for (int i = 0; i < 5; i++) o[3 + i] = (double)st_acc[i];
    double* o2 = dbg + 2048 + (blockIdx.x >> 3) * 8;      // (the trace buffer is followed by the stamp build's own 16 KB)
    for (int i = 0; i < 5; i++) o2[i] = (double)st_acc[6 + i];
  }
#endif
}

// TsdGrid::propagateBorders (TsdGrid.cpp:372-427), incremental form, as a kernel of its own behind k_push_update: one wave per listed
// tile (push_device.hpp: halo_tile_job).  The fused scan does not launch it: there the next scan's ray cast follows the push at
// once and its first waves do this pass (raycast_kernels.hip).
__global__ void __launch_bounds__(256)
k_push_halo(GridDev g, HaloArgs h)
{
  const int lane = threadIdx.x & 63;
  const unsigned int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv == 0 && lane == 0) halo_bookkeeping(h.pushes, h.a_dev, h.cx, h.cy, h.slack);
  // the tiles with work here: UPDATE tiles materialised by this push or written by freeFootprint (list_h), emptied and halo-only tiles
  // (the back of `list`).  A plain UPDATE tile's edge changes were mirrored by its own workgroup.
  const unsigned int n_u = h.cnt[CNT_H], n_list = n_u + h.cnt[CNT_O];
  const uint32_t first = h.list_h[wv];                          // speculative: arrives with the list lengths
  for (unsigned int li = wv; li < n_list; li += gridDim.x * 4) {
    // UPDATE tiles from the halo list, the others (emptied, dirtied) from the back of the work list
    const uint32_t entry = li < n_u ? ((li == wv) ? first : h.list_h[li]) : h.list[(unsigned)g.tiles - 1u - (li - n_u)];
    halo_tile_job(g, h.dirty, h.tile_rec, entry, lane);
  }
}

// TsdGrid::freeFootprint (TsdGrid.cpp:609-638): lazily initialise touched tiles, set tsd = 1.0
// (weight untouched).  One 256-thread block per tile of the rectangle's tile range.
__global__ void __launch_bounds__(256)
k_free_footprint(GridDev g, unsigned minX, unsigned maxX, unsigned minY, unsigned maxY,
                 unsigned tx0, unsigned ty0, unsigned ntx, uint8_t* __restrict__ dirty)
{
  const unsigned tx = tx0 + blockIdx.x % ntx, ty = ty0 + blockIdx.x / ntx;
  const int p = (int)(ty * (unsigned)g.PX + tx);
  const int tid = threadIdx.x;
  tsd_cell_t* T = g.tsd + (size_t)p * TILE_STRIDE;
  w_cell_t* W = g.weight + (size_t)p * TILE_STRIDE;
  const bool fresh = g.flags[p] == 0;
  const double iw = g.init_weight[p];
  const double t_init = (iw > 0.0) ? 1.0 : __builtin_nan("");
  for (int i = tid; i < TILE_CELLS; i += 256) {
    const int can = canonical_of_off(i);                       // i is the device offset
    const unsigned lx = (unsigned)(can % TILE_PITCH), ly = (unsigned)(can / TILE_PITCH);
    const unsigned col = tx * TILE_DIM + lx, row = ty * TILE_DIM + ly;
    const bool inside = lx < TILE_DIM && ly < TILE_DIM && col >= minX && col < maxX && row >= minY && row < maxY;
    if (inside) { st_tsd(T + i, 1.0); if (fresh) st_w(W + i, iw); }
    else if (fresh) { st_tsd(T + i, t_init); st_w(W + i, iw); }
  }
  __syncthreads();            // every thread has read `fresh`
  if (tid == 0) {
    if (fresh) g.flags[p] = 1;
    dirty[p] = 1;             // its halo (and its neighbours') are refreshed by the next push
  }
}

// PMC calibration (MI355X_MICROARCH.md, HBM: FETCH_SIZE / WRITE_SIZE are only calibrated for 16 B/lane
// streams): a read-modify-write of n doubles with the push kernel's access shape, 8 B per lane, two
// arrays, so that the counters of a known byte count (16 n read, 16 n written) can be compared with
// what rocprofv3 reports for k_push_tiles.
__global__ void __launch_bounds__(256)
k_calib_rmw(double* __restrict__ t, double* __restrict__ w, size_t n)
{
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double a = t[i], b = w[i];
    t[i] = a * 0.5 + b; w[i] = b + 1.0;
  }
}

int launch_calibrate(tsd_ctx* ctx, double* t, double* w, size_t n)
{
  hipLaunchKernelGGL(k_calib_rmw, dim3(2048), dim3(256), 0, ctx->stream, t, w, n);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

// ------------------------------------------------------------------------------------------------
// exact `negmask` of a grid whose cells were written by the host (tsd_upload_tiles): one workgroup per tile;
// a negative halo cell is charged to the tile that owns the cell (uploaded halos may be stale)
__global__ void __launch_bounds__(256)
k_neg_scan(GridDev g)
{
  const int p = blockIdx.x;
  if (!g.flags[p]) return;
  const int PX = g.PX, px = p % PX, py = p / PX;
  const tsd_cell_t* T = g.tsd + (size_t)p * TILE_STRIDE;
  for (int i = threadIdx.x; i < TILE_CELLS; i += 256) {
    if (!(ld_tsd(T + i) < 0.0)) continue;
    const int can = canonical_of_off(i);
    const unsigned ix = (unsigned)can % TILE_PITCH, iy = (unsigned)can / TILE_PITCH;
    const int qx = px + (ix == TILE_DIM ? 1 : 0), qy = py + (iy == TILE_DIM ? 1 : 0);
    if (qx >= PX || qy >= PX) continue;                        // (no tile owns the outermost halo)
    atomicOr(&g.negmask[qy * PX + qx], neg_bit(ix & 31u, iy & 31u));
  }
}

// ------------------------------------------------------------------------------------------------
// Canonical tile I/O (tsd_download_tiles / tsd_upload_tiles): the C ABI and the oracle speak 33 x 33 row-major fp64
// tiles (TsdGridPartition::_grid); the device layout (interior + halo strip, fp64 or Q32 cells) is converted here.
// One workgroup per tile of the chunk [t0, t0 + n).
__global__ void __launch_bounds__(256)
k_export_tiles(GridDev g, int t0, double* __restrict__ out_t, double* __restrict__ out_w)
{
  const int p = t0 + blockIdx.x;
  const bool init = g.flags[p] != 0;
  const tsd_cell_t* T = g.tsd + (size_t)p * TILE_STRIDE;
  const w_cell_t* W = g.weight + (size_t)p * TILE_STRIDE;
  double* ot = out_t + (size_t)blockIdx.x * TILE_CELLS;
  double* ow = out_w + (size_t)blockIdx.x * TILE_CELLS;
  for (int i = threadIdx.x; i < TILE_CELLS; i += 256) {
    const int can = canonical_of_off(i);
    ot[can] = init ? ld_tsd(T + i) : __builtin_nan("");      // uninitialised tiles read back NaN / 0
    ow[can] = init ? ld_w(W + i) : 0.0;
  }
}
__global__ void __launch_bounds__(256)
k_import_tiles(GridDev g, int t0, const double* __restrict__ in_t, const double* __restrict__ in_w)
{
  const int p = t0 + blockIdx.x;
  if (!g.flags[p]) return;
  tsd_cell_t* T = g.tsd + (size_t)p * TILE_STRIDE;
  w_cell_t* W = g.weight + (size_t)p * TILE_STRIDE;
  const double* it = in_t + (size_t)blockIdx.x * TILE_CELLS;
  const double* iw = in_w + (size_t)blockIdx.x * TILE_CELLS;
  for (int i = threadIdx.x; i < TILE_CELLS; i += 256) {
    const int can = canonical_of_off(i);
    st_cell(T, W, i, it[can], iw[can]);
  }
}
int launch_export_tiles(tsd_ctx* ctx, int t0, int n, double* d_t, double* d_w)
{
  hipLaunchKernelGGL(k_export_tiles, dim3(n), dim3(256), 0, ctx->stream, ctx->grid, t0, d_t, d_w);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}
int launch_import_tiles(tsd_ctx* ctx, int t0, int n, const double* d_t, const double* d_w)
{
  hipLaunchKernelGGL(k_import_tiles, dim3(n), dim3(256), 0, ctx->stream, ctx->grid, t0, d_t, d_w);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

// Digest of the canonical dump (tsd_grid_digest): an order-free 64-bit hash of (tile flag, initWeight, every cell's
// tsd and weight bit patterns, NaN and -0.0 canonicalised) plus sums over the valid cells -- what the cfg 1-3 golden
// fixtures pin without shipping a 4.6 GB dump.  One workgroup per tile; out[p] = {hash, n_valid} as
// u64, sums[p] = {sum tsd, sum weight}; the host adds the per-tile records in tile order.
__device__ __forceinline__ unsigned long long digest_mix(unsigned long long k, unsigned long long a, unsigned long long b)
{
  unsigned long long x = k * 0x9E3779B97F4A7C15ull + a;
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  x += b;
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  return x;
}
__device__ __forceinline__ unsigned long long digest_bits(double v)
{
  if (isnan(v)) return 0x7FF8000000000000ull;
  return (unsigned long long)__double_as_longlong(v + 0.0);      // -0.0 -> +0.0
}
__global__ void __launch_bounds__(256)
k_grid_digest(GridDev g, unsigned long long* __restrict__ out, double* __restrict__ sums)
{
  const int p = blockIdx.x;
  const bool init = g.flags[p] != 0;
  const tsd_cell_t* T = g.tsd + (size_t)p * TILE_STRIDE;
  const w_cell_t* W = g.weight + (size_t)p * TILE_STRIDE;
  unsigned long long h = 0ull, nv = 0ull; double st = 0.0, sw = 0.0;
  if (init) {
    for (int i = threadIdx.x; i < TILE_CELLS; i += 256) {
      const double t = ld_tsd(T + i), w = ld_w(W + i);
      h += digest_mix((unsigned long long)p * 2048ull + 1ull + (unsigned long long)canonical_of_off(i), digest_bits(t), digest_bits(w));
      if (!isnan(t)) { nv++; st += t; sw += w; }
    }
  }
  __shared__ unsigned long long s_h[256], s_n[256]; __shared__ double s_t[256], s_w[256];
  s_h[threadIdx.x] = h; s_n[threadIdx.x] = nv; s_t[threadIdx.x] = st; s_w[threadIdx.x] = sw;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      s_h[threadIdx.x] += s_h[threadIdx.x + k]; s_n[threadIdx.x] += s_n[threadIdx.x + k];
      s_t[threadIdx.x] += s_t[threadIdx.x + k]; s_w[threadIdx.x] += s_w[threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[2 * p] = s_h[0] + digest_mix((unsigned long long)p * 2048ull, init ? 1ull : 0ull, digest_bits(g.init_weight[p]));
    out[2 * p + 1] = s_n[0];
    sums[2 * p] = s_t[0]; sums[2 * p + 1] = s_w[0];
  }
}
int launch_grid_digest(tsd_ctx* ctx, unsigned long long* d_out, double* d_sums)
{
  hipLaunchKernelGGL(k_grid_digest, dim3(ctx->grid.tiles), dim3(256), 0, ctx->stream, ctx->grid, d_out, d_sums);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

int launch_neg_scan(tsd_ctx* ctx)
{
  const GridDev& g = ctx->grid;
  TSD_HIP_CHECK(ctx, hipMemsetAsync(g.negmask, 0, (size_t)g.tiles * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_neg_scan, dim3(g.tiles), dim3(256), 0, ctx->stream, g);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

int launch_free_footprint(tsd_ctx* ctx, unsigned minX, unsigned maxX, unsigned minY, unsigned maxY)
{
  if (maxX <= minX || maxY <= minY) { ctx->ledger.footprint(TileBox{}); return TSD_OK; }    // (nothing to write; the call still counts)
  const unsigned tx0 = minX / TILE_DIM, tx1 = (maxX - 1) / TILE_DIM;
  const unsigned ty0 = minY / TILE_DIM, ty1 = (maxY - 1) / TILE_DIM;
  const unsigned ntx = tx1 - tx0 + 1, nty = ty1 - ty0 + 1;
  hipLaunchKernelGGL(k_free_footprint, dim3(ntx * nty), dim3(256), 0, ctx->stream, ctx->grid, minX,
                     maxX, minY, maxY, tx0, ty0, ntx, ctx->d_dirty);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  TileBox b; b.x0 = (int)tx0; b.y0 = (int)ty0; b.x1 = (int)tx1; b.y1 = (int)ty1;
  ctx->ledger.footprint(b);
  return TSD_OK;
}

size_t push_rmq_bytes(int beams) { return rmq_bytes(beams); }
size_t push_list_aux_bytes() { return sizeof(PushListAux); }
size_t push_list_cnt_bytes() { return 2 * CNT_WORDS * sizeof(unsigned int); }

int launch_push_tables(tsd_ctx* ctx, hipStream_t stream, int beams, const double* d_ranges, const uint8_t* d_mask, char* rmq,
                       double phi_min, double ang_res)
{
  const size_t bp = (size_t)((beams + 3) & ~3);
  const size_t lds = 2 * bp * sizeof(double) + 4 * bp * 2 + 64;
  if (int rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(k_push_tables), lds)) return rc;
  hipLaunchKernelGGL(k_push_tables, dim3(1), dim3(1024), lds, stream, d_ranges, d_mask, beams, rmq, phi_min, ang_res);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

int launch_push_tables_batch(tsd_ctx* ctx, hipStream_t stream, const TablesBatchEntry* d_entries, int n, int max_beams)
{
  const size_t bp = (size_t)((max_beams + 3) & ~3);
  const size_t lds = 2 * bp * sizeof(double) + 4 * bp * 2 + 64;
  if (int rc = ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(k_push_tables_batch), lds)) return rc;
  hipLaunchKernelGGL(k_push_tables_batch, dim3(n), dim3(1024), lds, stream, d_entries);
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

// the tables of this scan must already be in job.rmq (launch_push_tables, ordered before this)
int launch_push(tsd_ctx* ctx, hipStream_t stream, const PushJob& job, HaloArgs* defer_halo)
{
  const GridDev& g = ctx->grid;
  const PushArgs* const a_dev = job.a_dev;
  if (!a_dev) return set_error(ctx, TSD_E_ARG, "launch_push: the arguments must be on the device", hipSuccess);
  char* const rmq = job.rmq;
  const double cx = job.cx, cy = job.cy, slack = job.slack;
  // Tile window: the push's own (push_tile_window), widened by the ledger to the previous push and what freeFootprint touched since.
  const TileBox box = ctx->ledger.push_window(push_tile_window(g, cx, cy, job.max_range, slack));
  const int ntx = box.x1 - box.x0 + 1, nty = box.y1 - box.y0 + 1;
  const int parity = (int)(ctx->push_parity & 1u);
  ctx->push_parity++;
  const int n_window = ntx * nty;
  {
    ScopedKernelTimer t(ctx, "push_classify");
    if (n_window <= 12288)
      hipExtLaunchKernelGGL((k_push_classify<256>), dim3((n_window + 63) / 64), dim3(256), 0, stream, t.a, t.b, 0, g, a_dev, rmq,
                         ctx->d_tile_rec, ctx->d_dirty, ctx->d_tile_totals, ctx->d_list, reinterpret_cast<PushListAux*>(ctx->d_list_aux), ctx->d_list_h, ctx->d_list_cnt, parity,
                         box.x0, box.y0, ntx, nty);
    else
      hipExtLaunchKernelGGL((k_push_classify<1024>), dim3((n_window + 255) / 256), dim3(1024), 0, stream, t.a, t.b, 0, g, a_dev, rmq,
                         ctx->d_tile_rec, ctx->d_dirty, ctx->d_tile_totals, ctx->d_list, reinterpret_cast<PushListAux*>(ctx->d_list_aux), ctx->d_list_h, ctx->d_list_cnt, parity,
                         box.x0, box.y0, ntx, nty);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  // as many workgroups as are RESIDENT at once (UPDATE_WPS per compute unit), never more: every workgroup loops over the
  // list with that stride, and a second round of workgroups would start its whole share of the list when the first round is done
  int per_cu = UPDATE_WPS;
  { const size_t lds_wg = update_lds_bytes(job.beams) + 64; const int by_lds = (int)((160u * 1024u) / lds_wg); if (by_lds < per_cu) per_cu = by_lds < 1 ? 1 : by_lds; }
  const int resident = ctx->n_cus * per_cu;
  const int n_groups = n_window < resident ? n_window : resident;
  {
    ScopedKernelTimer t(ctx, "push_update");
    size_t lds = update_lds_bytes(job.beams);
    hipExtLaunchKernelGGL(k_push_update, dim3(n_groups), dim3(UPDATE_BLOCK), lds, stream, t.a, t.b, 0, g, a_dev, job.ranges, job.mask,
                       ctx->d_tile_rec, ctx->d_tile_totals, ctx->d_list, reinterpret_cast<const PushListAux*>(ctx->d_list_aux), ctx->d_list_cnt, parity,
                       rmq_view(rmq, job.beams).bdir, rmq_view(rmq, job.beams).rot, ctx->d_icp_trace);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  HaloArgs h;
  h.dirty = ctx->d_dirty; h.pushes = ctx->d_pushes; h.a_dev = a_dev; h.list = ctx->d_list; h.list_h = ctx->d_list_h; h.tile_rec = ctx->d_tile_rec;
  h.cnt = ctx->d_list_cnt + CNT_WORDS * parity; h.cx = cx; h.cy = cy; h.slack = slack + g.cs; h.on = 1;
  if (defer_halo) {
    // (the caller launches the ray cast that carries this pass -- launch_raycast(.., &halo) -- right behind this push, or, if it cannot,
    // launch_push_halo(): the grid's halos are not consistent until one of the two has run)
    *defer_halo = h;
    return TSD_OK;
  }
  return launch_push_halo(ctx, stream, h, n_window);
}

int launch_push_halo(tsd_ctx* ctx, hipStream_t stream, const HaloArgs& h, int n_window)
{
  {
    ScopedKernelTimer t(ctx, "push_halo");
    // one wave per tile of the halo list (tiles materialised / emptied / written by freeFootprint: a few dozen per push once the map
    // stands, every tile of the window in the first push); a longer list is looped over.  (Round 4 launched one wave per WINDOW tile:
    // 6 745 waves to move 0.35 MB at cfg 2.)
    constexpr int HALO_WAVES = 2048;
    if (n_window > ctx->grid.tiles) n_window = ctx->grid.tiles;        // (every wave reads its first list entry speculatively: stay inside the list)
    const int n_waves = n_window < HALO_WAVES ? (n_window < 1 ? 1 : n_window) : HALO_WAVES;
    hipExtLaunchKernelGGL(k_push_halo, dim3((n_waves + 3) / 4), dim3(256), 0, stream, t.a, t.b, 0, ctx->grid, h);
  }
  TSD_HIP_CHECK(ctx, hipGetLastError());
  return TSD_OK;
}

}  // namespace tsd
