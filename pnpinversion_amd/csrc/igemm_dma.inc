// igemm_dma_kernel: the LDS-DMA implicit-GEMM kernel template (included by gemm.hip; tools/isa_probe.hip instantiates single
// configurations of it to read their ISA without rebuilding every variant).
#pragma once
#include "ops.h"
#include "igemm_epilogue.inc"
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

// A 16-byte LDS read the compiler does not track (ds_read_b128 in inline asm): the caller waits with its own counted
// `s_waitcnt lgkmcnt(N)` + sched_barrier(0) before the first use (cdna_hip_programming.md 5.7, form iii).  hipcc's own waits are
// always lgkmcnt(0) in this loop -- it cannot keep a younger k-step's reads in flight across an older k-step's MFMAs.
__device__ __forceinline__ half8 lds_read_b128_async(unsigned addr, int imm) {
  half8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(imm) : "memory");
  return v;
}

// ABL: 0 = product kernel, main loop scheduled by the compiler; 4 = product kernel, hand-scheduled main loop (fragment reads two k-steps
// ahead behind counted lgkmcnt waits, the next chunk's DMA instructions spread between the MFMAs); 1 = DMA only (no fragment reads / MFMA); 2 = compute only (no DMA); 3 = activation operand loaded for
// the first filter tap only -- bottleneck ablations for tools/ (1-3 produce garbage).
//
// Tile geometry: WGM x 2 wavefronts (NT = 128 * WGM threads); a wave owns (BM / WGM) x (BN / 2) of the block tile as 32x32 MFMA
// tiles.  Instantiated shapes (BM x BN, wave tile): 64x64 (32x32), 128x128 (64x64), 128x256 (64x128), 128x320 (64x160: 20
// MFMAs per 32-deep k-chunk and barrier, 91 FLOP per operand byte -- the N = 320 / 640 / 1280 layers tile exactly), 256x128.
//
// WK > 1: K-parallel wave groups.  The block holds WK groups of WGM x 2 waves; group g owns its own LDS ring and walks the g-th
// contiguous slice of the block's k-range into its own accumulators (the groups run in lock step on the one workgroup barrier per
// chunk), then groups 1 .. WK-1 hand their fp32 accumulators to group 0 through LDS in a FIXED order and exit; group 0 runs the
// epilogue.  A launch with at most one tile per CU (the one-row inversion forwards, the 16 x 16 / 8 x 8 levels) puts WK times the
// MFMA-issuing waves on every CU this way -- split-K with the partial sums in LDS instead of slabs + a reduce launch.
template <int BM, int BN, int BKT, int NST, int WGM = 2, int ABL = 0, int WK = 1>
struct IgemmGeom {
  static constexpr int NW = 2 * WGM, NT = 64 * NW;              // waves / threads of ONE k-group (= the epilogue's threads)
  static constexpr int NT_ALL = NT * WK;
  static constexpr int WM = BM / WGM, WN = BN / 2, MI = WM / 32, NI = WN / 32;
  static constexpr int RPI = 1024 / (BKT * 2);                 // tile rows per 1-KiB DMA instruction (8 or 16)
  static constexpr int AV = BM / RPI / NW, WV = BN / RPI / NW;  // DMA instructions per wave per chunk and operand
  static constexpr int ROWB = BKT * 2;                          // bytes per tile row
  static constexpr int STAGE = (BM + BN) * ROWB;                // bytes
  static constexpr int RING = NST * STAGE;
  // LDS epilogue: the output tile is staged as [rows][BN + 8] halfs in the idle ring, EPASS passes of EROWS rows (one row of
  // waves per pass when the whole tile does not fit), then written as full rows; G row groups of VPR 16-byte vectors.
  static constexpr int OLD = BN + 8, VPR = BN / 8, G = NT / VPR;
  static constexpr int STATS_B = G * BN * 2 * 4;
  static constexpr int EPASS = (BM * OLD * 2 + STATS_B <= RING) ? 1 : WGM;
  static constexpr int EROWS = BM / EPASS;
  static constexpr int TOLD = EROWS + 8;                        // halfs per staged row of a TRANSPOSED tile ([BN][EROWS + 8])
  static constexpr int EPI_PLAIN = EROWS * OLD * 2 + STATS_B, EPI_TR = BN * TOLD * 2;
  static constexpr int EPI = EPI_PLAIN > EPI_TR ? EPI_PLAIN : EPI_TR;
  static constexpr int RED = (WK - 1) * BM * BN * 4;            // fp32 accumulators of groups 1 .. WK-1 on their way to group 0
  static constexpr int LDS0 = WK * RING > EPI ? WK * RING : EPI;
  static constexpr int LDS = LDS0 > RED ? LDS0 : RED;
  static_assert(LDS <= 160 * 1024, "LDS");
  static_assert(BM % (RPI * NW) == 0 && BN % (RPI * NW) == 0, "DMA instructions must divide evenly over the waves");
  static_assert(WM % 32 == 0 && WN % 32 == 0 && BN % 64 == 0, "wave tile");
};

template <int BM, int BN, int BKT, int NST, int WGM = 2, int ABL = 0, int WK = 1>
__global__ void __launch_bounds__(128 * WGM * WK, (IgemmGeom<BM, BN, BKT, NST, WGM, ABL, WK>::LDS * 2 <= 160 * 1024 && BN <= 320 && WK == 1) ? (2 * 2 * WGM / 4) : (2 * WGM * WK / 4))
igemm_dma_kernel(GemmP p_in, const half_t* __restrict__ zero_page) {
  GemmP p = p_in;
  static_assert(BKT == 64 || BKT == 32, "BKT");
  using GEO = IgemmGeom<BM, BN, BKT, NST, WGM, ABL, WK>;
  constexpr int NT = GEO::NT, NW = GEO::NW;
  constexpr int WM = GEO::WM, WN = GEO::WN, MI = GEO::MI, NI = GEO::NI;
  constexpr int AV = GEO::AV, WV = GEO::WV, ROWB = GEO::ROWB, STAGE = GEO::STAGE;
  constexpr int T32 = 32 * ROWB;                       // bytes per 32-row MFMA tile
  extern __shared__ __attribute__((aligned(1024))) char smem_all[];

  const int tid = threadIdx.x & (NT - 1), lane = tid & 63;                    // thread / wave index inside the k-group
  const int kgrp = WK == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x / NT);
  char* smem_raw = smem_all + kgrp * GEO::RING;                                 // this group's ring
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave >> 1) * WM, wn0 = (wave & 1) * WN;
  // XCD-aware tile order.  Consecutive workgroup ids are dealt round-robin to the 8 XCDs (each with a private L2), so the
  // launch is 1-D and XCD x takes the x-th contiguous eighth of the tile list.  The list is ordered so that the operand
  // that is expensive to re-fetch crosses the fabric once: tile_order 0 = n fastest (an XCD owns a band of m-tiles: the
  // activation is read once, the weight by every XCD), 1 = m fastest (an XCD owns a band of (n, k-split) weight slices:
  // the weight is read once -- the low-resolution 1280-channel convolutions, where the weight is 10x the activation).
  int bx, by, bz;
  {
    const int T = p.gx * p.gy * p.gz, per = (T + 7) >> 3;
    const int tix = p.tile_order == 2 ? (int)blockIdx.x : (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);   // 2: ablation
    if (tix >= T) return;
    if (p.tile_order == 0) { by = tix % p.gy; const int t = tix / p.gy; bx = t % p.gx; bz = t / p.gx; }
    else { bx = tix % p.gx; const int t = tix / p.gx; by = t % p.gy; bz = t / p.gy; }
  }
  const int m0 = bx * BM, n0 = by * BN;
  if (p.nbatch > 1) {                 // batched launch: bz is the problem index (the launcher never combines it with split-K)
    p.x1 += (size_t)bz * p.sx1;
    p.w += (size_t)bz * p.sw;
    if (p.out) p.out += (size_t)bz * p.sout;
    if (p.outT) p.outT = (char*)p.outT + (size_t)bz * p.soutT;
  }
  const int Cin = p.C1 + p.C2;
  const int HoWo = p.Ho * p.Wo;

  // ---- DMA lane roles.  A wave-level DMA instruction fills 1 KiB lane-linearly; the (row, chunk) a lane fetches is the
  // inverse of the swizzled LDS layout:
  //   BKT = 64: 128-byte rows, byte(R, s) = (R>>4)*2048 + (R&7)*256 + ((R>>3)&1)*128 + ((s ^ (R&7)) * 16)
  //   BKT = 32:  64-byte rows, byte(R, s) = (R>>4)*1024 + ((R>>2)&3)*256 + (R&3)*64 + ((s ^ ((R>>2)&3)) * 16)
  // Everything of the gather that does not depend on the k-chunk is precomputed per row; the per-chunk address is pure
  // arithmetic (no selects that could turn into divergent control flow, no runtime-indexed arrays -> no scratch).
  int d_row, d_chunk;   // row within the instruction's row group, logical 16-byte chunk
  if (BKT == 64) {
    const int line_lo = lane >> 4, half = (lane >> 3) & 1;
    d_row = half * 8 + line_lo;         // + 4 * (j & 1) added below
    d_chunk = lane & 7;                 // ^ line below
  } else {
    d_row = (lane >> 4) * 4 + ((lane >> 2) & 3);
    d_chunk = (lane & 3) ^ (lane >> 4);
  }
  int a_y0[AV], a_x0[AV], a_bh[AV], a_chunk[AV];
#pragma unroll
  for (int i = 0; i < AV; ++i) {
    const int j = wave * AV + i;
    int R, ch;
    if (BKT == 64) { const int line = 4 * (j & 1) + (lane >> 4); R = (j >> 1) * 16 + ((lane >> 3) & 1) * 8 + line; ch = (lane & 7) ^ line; }
    else { R = j * 16 + d_row; ch = d_chunk; }
    a_chunk[i] = ch * 8;
    const int m = m0 + R;
    int b = m / HoWo;
    int rr = m - b * HoWo;
    int yo = rr / p.Wo;
    int xo = rr - yo * p.Wo;
    a_bh[i] = b * p.H;
    a_y0[i] = m < p.M ? yo * p.stride - p.pad : -(1 << 20);   // rows past M fail the bounds test for every tap
    a_x0[i] = xo * p.stride - p.pad;
  }
  const int lim_y = p.ups ? 2 * p.H : p.H, lim_x = p.ups ? 2 * p.W : p.W, ups_sh = p.ups ? 1 : 0;
  const int nchunks = p.K / BKT;
  int kc0 = 0, kc1 = nchunks;
  if (p.splitk > 1) {   // kchunks_per_split is given in 64-wide chunks
    kc0 = bz * p.kchunks_per_split * (64 / BKT);
    kc1 = min(nchunks, kc0 + p.kchunks_per_split * (64 / BKT));
  }
  int iters = kc1 > kc0 ? kc1 - kc0 : 0;      // loop trips: the same for every k-group (they share the barrier)
  if (WK > 1) {
    iters = (iters + WK - 1) / WK;
    kc0 = min(kc1, kc0 + kgrp * iters);
    kc1 = min(kc1, kc0 + iters);
  }
  // Weight rows: one pointer per DMA instruction, bumped by BKT per chunk.  Rows past N read the zero page, which is as long
  // as the longest K this kernel is launched with, so they are bumped like the others (no select in the loop).
  const half_t* w_cur[WV];
#pragma unroll
  for (int i = 0; i < WV; ++i) {
    const int j = wave * WV + i;
    int R, ch;
    if (BKT == 64) { const int line = 4 * (j & 1) + (lane >> 4); R = (j >> 1) * 16 + ((lane >> 3) & 1) * 8 + line; ch = (lane & 7) ^ line; }
    else { R = j * 16 + d_row; ch = d_chunk; }
    const int n = n0 + R;
    w_cur[i] = (n < p.N ? p.w + (size_t)n * p.ldw : zero_page) + ch * 8 + kc0 * BKT;
  }

  // Activation rows: the (tap, source, bounds) part of the gather address changes only when the k-chunk walks into a new
  // filter tap or from the first concat source into the second; inside a tap consecutive chunks are consecutive channels.
  // So the full address (bounds test, 64-bit multiply, zero-page select) is rebuilt under a wave-uniform branch on those
  // boundaries only, and the per-chunk work is one pointer bump per DMA instruction.
  int is_tap = (kc0 * BKT) / Cin;              // wave-uniform scalars
  int is_c0 = kc0 * BKT - is_tap * Cin;
  bool retap = true;
  const half_t* a_cur[AV];
#pragma unroll
  for (int i = 0; i < AV; ++i) a_cur[i] = zero_page;

  auto issue = [&](int buf) {
    char* sA = smem_raw + buf * STAGE;
    char* sW = sA + BM * ROWB;
    if (retap) {
      int r = 0, s = 0;
      if (p.ksize == 3) { r = is_tap / 3; s = is_tap - 3 * r; }
      const half_t* src; int ld, cc;
      if (is_c0 < p.C1) { src = p.x1; ld = p.ldx1; cc = is_c0; } else { src = p.x2; ld = p.ldx2; cc = is_c0 - p.C1; }
      const long zoff = zero_page - src;   // element distance to the zero page (plain integer arithmetic on addresses)
#pragma unroll
      for (int i = 0; i < AV; ++i) {
        const int yi = a_y0[i] + r, xi = a_x0[i] + s;
        const bool ok = (unsigned)yi < (unsigned)lim_y && (unsigned)xi < (unsigned)lim_x;
        const long off = (long)((a_bh[i] + (yi >> ups_sh)) * p.W + (xi >> ups_sh)) * ld + (cc + a_chunk[i]);
        const long mask = -(long)ok;                       // all ones when in range: select without control flow
        a_cur[i] = src + ((off & mask) | ((zoff + a_chunk[i]) & ~mask));
      }
      retap = false;
    }
    if (ABL != 3 || (is_tap == 0)) {   // ABL 3: the activation operand only for the first filter tap (bound of tap-reuse schemes)
#pragma unroll
      for (int i = 0; i < AV; ++i) {
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)a_cur[i], (lds_ptr_t)(sA + (wave * AV + i) * 1024), 16, 0, 0);
        a_cur[i] += BKT;
      }
    }
#pragma unroll
    for (int i = 0; i < WV; ++i) {
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)w_cur[i], (lds_ptr_t)(sW + (wave * WV + i) * 1024), 16, 0, 0);
      w_cur[i] += BKT;
    }
    is_c0 += BKT;
    if (is_c0 >= Cin) { is_c0 = 0; ++is_tap; retap = true; }
    else if (is_c0 == p.C1) retap = true;
  };

  // The same, split for the hand-scheduled loop (ABL == 4): issue_prep() rebuilds the gather addresses when the k-walk entered a new tap /
  // concat source, issue_piece(stage, p) issues the p-th DMA instruction of the chunk (activation rows first, then weight rows) and bumps
  // its pointer, issue_done() advances the k-walk.
  auto issue_prep = [&]() {
    if (retap) {
      int r = 0, s = 0;
      if (p.ksize == 3) { r = is_tap / 3; s = is_tap - 3 * r; }
      const half_t* src; int ld, cc;
      if (is_c0 < p.C1) { src = p.x1; ld = p.ldx1; cc = is_c0; } else { src = p.x2; ld = p.ldx2; cc = is_c0 - p.C1; }
      const long zoff = zero_page - src;
#pragma unroll
      for (int i = 0; i < AV; ++i) {
        const int yi = a_y0[i] + r, xi = a_x0[i] + s;
        const bool ok = (unsigned)yi < (unsigned)lim_y && (unsigned)xi < (unsigned)lim_x;
        const long off = (long)((a_bh[i] + (yi >> ups_sh)) * p.W + (xi >> ups_sh)) * ld + (cc + a_chunk[i]);
        const long mask = -(long)ok;
        a_cur[i] = src + ((off & mask) | ((zoff + a_chunk[i]) & ~mask));
      }
      retap = false;
    }
  };
  auto issue_piece = [&](char* stage, int pidx) {
    if (pidx < AV) {
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)a_cur[pidx], (lds_ptr_t)(stage + (wave * AV + pidx) * 1024), 16, 0, 0);
      a_cur[pidx] += BKT;
    } else {
      const int i = pidx - AV;
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)w_cur[i], (lds_ptr_t)(stage + BM * ROWB + (wave * WV + i) * 1024), 16, 0, 0);
      w_cur[i] += BKT;
    }
  };
  auto issue_done = [&]() {
    is_c0 += BKT;
    if (is_c0 >= Cin) { is_c0 = 0; ++is_tap; retap = true; }
    else if (is_c0 == p.C1) retap = true;
  };

  // Accumulators.  With alpha == 1 the bias is the accumulator's INITIAL value (p.bias_init, set by the launcher): 4 * NI
  // unconditional 16-byte loads per lane, issued before the first DMA instruction and landed long before the first MFMA needs
  // them -- instead of 16 * MI * NI dependent 4-byte loads in the epilogue, each with its own wait, which cost the short-K
  // layers (10 ... 40 k-chunks per tile) more than their whole main loop.  A lane holds columns n .. n + 3 of every 8-column
  // group, the same for every mi.
  floatx16 acc[MI][NI];
  const float* ebias = p.bias_init ? nullptr : p.bias;   // what the epilogue still has to add
  if (p.bias_init && kgrp == 0) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn0 + ni * 32 + 8 * g + 4 * (lane >> 5);
        floatx4 b = *reinterpret_cast<const floatx4*>(p.bias + min(n, p.N - 4));   // N % 4 == 0: a group is all in or all out
        if (n >= p.N) b = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[0][ni][4 * g + j] = b[j];
      }
#pragma unroll
    for (int mi = 1; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = acc[0][ni];
  } else {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
  }

  // byte address of this k-group's ring inside the workgroup's LDS allocation (for the asm fragment reads of the hand-scheduled loop)
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem_raw;
  // fragment read addressing (same involution as the DMA source permutation)
  const int lr = lane & 31, hk = lane >> 5;
  int lane_row_off, xk;
  if (BKT == 64) { lane_row_off = (lr >> 4) * 2048 + (lr & 7) * 256 + ((lr >> 3) & 1) * 128; xk = lr & 7; }
  else { lane_row_off = (lr >> 4) * 1024 + ((lr >> 2) & 3) * 256 + (lr & 3) * 64; xk = (lr >> 2) & 3; }

  // NST-deep LDS ring.  Chunk k+NST-1 is issued while chunk k is computed; each wave waits for ITS loads of chunk k with a
  // counted vmcnt (the newer chunks stay in flight across the barrier), then one raw barrier per chunk makes every wave's
  // part of chunk k visible and, at the same time, frees the stage that was read in the previous iteration.
  constexpr int LPS = AV + WV;   // DMA instructions per wave per chunk
  if constexpr (ABL == 4 || ABL == 5) {
    // ---- hand-scheduled main loop (ABL == 5: the DMA instructions as one block in front of the MFMAs, as the compiler-scheduled loop has them).  Same ring protocol as below (counted vmcnt for the oldest chunk, one raw barrier per chunk), but
    //   * the fragments of k-step kk + 2 are read (inline asm, untracked by the compiler) right after the MFMAs of k-step kk were
    //     issued, and each k-step waits with a COUNTED lgkmcnt for its own fragments only: the LDS latency of every read hides under
    //     MI * NI MFMAs (hipcc's own schedule waits lgkmcnt(0) four times per chunk with the reads issued two MFMAs earlier);
    //   * the next chunk's DMA instructions are issued one at a time BETWEEN the MFMAs (their ~60-100 issue cycles overlap the matrix
    //     pipe) instead of as one block in front of them;
    //   * the loop is peeled into a steady-state part (always issues) and a drain part (never does): no per-chunk control flow around
    //     the MFMAs, and the accumulators stay in place.
    static_assert(WK == 1, "hand-scheduled loop: one k-group");
    constexpr int KS = BKT / 16, NR = MI + NI, NM = MI * NI;
    const int total = iters;
    int issued = 0;
#pragma unroll
    for (int st = 0; st < NST - 1; ++st)
      if (issued < total) { issue(st); ++issued; }
    int rd = 0, wr = NST - 1;
    half8 fa[3][MI], fw[3][NI];      // three fragment sets in rotation: in use (k-step kk), landed or landing (kk + 1), being read (kk + 2)
    auto chunk = [&](auto more_c, int ahead) {
      constexpr bool MORE = decltype(more_c)::value;
      static_assert((NST - 2) * LPS <= 63, "vmcnt holds 6 bits");
      if (NST == 2 || ahead <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
      else if (ahead == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPS) : "memory");
      else if (ahead == 3 || NST <= 5) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST > 4 ? 3 : 0) * LPS) : "memory");
      else if (ahead == 4 || NST <= 6) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST > 5 ? 4 : 0) * LPS) : "memory");
      else if (ahead == 5 || NST <= 7) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST > 6 ? 5 : 0) * LPS) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST > 7 ? 6 : 0) * LPS) : "memory");
      __builtin_amdgcn_s_barrier();
      const unsigned aA = lds_base + (unsigned)(rd * STAGE + (wm0 >> 5) * T32 + lane_row_off);
      const unsigned aW = lds_base + (unsigned)(rd * STAGE + BM * ROWB + (wn0 >> 5) * T32 + lane_row_off);
      // the r-th fragment read of k-step kk (activation tiles first, then weight tiles) into set `slot`
      auto rd_one = [&](auto slot_c, int kk, int r) {
        constexpr int slot = decltype(slot_c)::value;
        const unsigned ko = (unsigned)(((kk * 2 + hk) ^ xk) * 16);
        if (r < MI) fa[slot][r] = lds_read_b128_async(aA + ko, r * T32);
        else fw[slot][r - MI] = lds_read_b128_async(aW + ko, (r - MI) * T32);
      };
      auto rd_slot = [&](int slot, int kk, int r) {
        if (slot == 0) rd_one(std::integral_constant<int, 0>{}, kk, r);
        else if (slot == 1) rd_one(std::integral_constant<int, 1>{}, kk, r);
        else rd_one(std::integral_constant<int, 2>{}, kk, r);
      };
#pragma unroll
      for (int r = 0; r < NR; ++r) rd_slot(0, 0, r);
      if (MORE) issue_prep();
      char* const stW = smem_raw + wr * STAGE;
      if (ABL == 5 && MORE) {
#pragma unroll
        for (int pidx = 0; pidx < LPS; ++pidx) issue_piece(stW, pidx);
      }
      if (KS > 1) {
#pragma unroll
        for (int r = 0; r < NR; ++r) rd_slot(1, 1, r);
      }
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        if (kk + 1 < KS) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NR) : "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        const int p0 = (kk * LPS) / KS, p1 = ((kk + 1) * LPS) / KS, np = (MORE && ABL == 4) ? p1 - p0 : 0;   // this k-step's share of the DMA instructions
        const int nrd = kk + 2 < KS ? NR : 0;                                                               // reads of k-step kk + 2, between the MFMAs
        int pc = 0, rc = 0;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const int mi = m / NI, ni = m % NI;
          acc[mi][ni] = mfma32(fw[kk % 3][ni], fa[kk % 3][mi], acc[mi][ni]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (; rc < ((m + 1) * nrd) / NM; ++rc) rd_slot((kk + 2) % 3, kk + 2, rc);
          if (np > 0 && ((m + 1) * np) / NM > pc) { issue_piece(stW, p0 + pc); ++pc; }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (MORE) { issue_done(); wr = wr + 1 == NST ? 0 : wr + 1; }
      rd = rd + 1 == NST ? 0 : rd + 1;
    };
    int it = 0;
    for (; it + (NST - 1) < total; ++it) chunk(std::true_type{}, NST - 2);          // steady state: NST - 2 younger chunks in flight
    for (; it < total; ++it) chunk(std::false_type{}, total - it - 1);              // drain
  } else
  if (iters > 0) {
    const int total = kc1 - kc0;   // this group's chunks (<= iters; a short last group idles through its tail but keeps the barrier)
    int issued = 0;
#pragma unroll
    for (int st = 0; st < NST - 1; ++st)
      if (issued < total) { if (ABL != 2) issue(st); ++issued; }
    int rd = 0, wr = NST - 1;
    for (int it = 0; it < iters; ++it) {
      const int ahead = issued - it - 1;           // chunks issued after the one needed now (0 .. NST-2)
      static_assert((NST - 2) * LPS <= 63, "vmcnt holds 6 bits");
      if (NST == 2 || ahead <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
      else if (ahead == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPS) : "memory");
      else if (ahead == 3 || NST <= 5) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST > 4 ? 3 : 0) * LPS) : "memory");
      else if (ahead == 4 || NST <= 6) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST > 5 ? 4 : 0) * LPS) : "memory");
      else if (ahead == 5 || NST <= 7) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST > 6 ? 5 : 0) * LPS) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST > 7 ? 6 : 0) * LPS) : "memory");
      __builtin_amdgcn_s_barrier();
      if (WK > 1 && it >= total) continue;         // wave-uniform: this group has run out of chunks
      if (ABL == 1) {
        if (issued < total) { issue(wr); ++issued; wr = wr + 1 == NST ? 0 : wr + 1; }
        rd = rd + 1 == NST ? 0 : rd + 1;
        continue;
      }
      const char* sA = smem_raw + rd * STAGE + (wm0 >> 5) * T32 + lane_row_off;
      const char* sW = smem_raw + rd * STAGE + BM * ROWB + (wn0 >> 5) * T32 + lane_row_off;
      // Software pipeline inside the chunk: the fragments of k-step kk+1 are read while the MFMAs of k-step kk run, and the
      // first k-step's reads are issued BEFORE the next chunk's DMA instructions (their issue slots -- ~100 cycles each -- then
      // overlap the LDS latency instead of preceding it).  One exposed LDS round trip per chunk instead of one per k-step.
      constexpr int KS = BKT / 16;
      half8 wf[2][NI], af[2][MI];
      auto frag_load = [&](int slot, int kk) {
        const int ko = ((kk * 2 + hk) ^ xk) * 16;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) af[slot][mi] = *reinterpret_cast<const half8*>(sA + mi * T32 + ko);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) wf[slot][ni] = *reinterpret_cast<const half8*>(sW + ni * T32 + ko);
      };
      frag_load(0, 0);
      if (issued < total) { if (ABL != 2) issue(wr); ++issued; wr = wr + 1 == NST ? 0 : wr + 1; }
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        if (kk + 1 < KS) frag_load((kk + 1) & 1, kk + 1);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = mfma32(wf[kk & 1][ni], af[kk & 1][mi], acc[mi][ni]);
      }
      rd = rd + 1 == NST ? 0 : rd + 1;
    }
  }

  if (WK > 1) {
    // k-groups 1 .. WK-1 -> group 0, through LDS (the rings are idle: every issued chunk has been waited for and read).  Register r
    // of lane l of wave w travels as one float at [(g-1)][w][tile][r][l]: lane-contiguous, conflict-free; group 0 adds the groups in
    // ascending order, so the sum is bit-reproducible.
    float* sRed = reinterpret_cast<float*>(smem_all);
    constexpr int PER_WAVE = MI * NI * 16 * 64, PER_GRP = NW * PER_WAVE;
    __syncthreads();
    if (kgrp > 0) {
      float* dst = sRed + (size_t)(kgrp - 1) * PER_GRP + wave * PER_WAVE + lane;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r) dst[((mi * NI + ni) * 16 + r) * 64] = acc[mi][ni][r];
    }
    __syncthreads();
    if (kgrp > 0) return;              // whole waves exit: s_barrier counts the surviving waves only
#pragma unroll
    for (int g = 1; g < WK; ++g) {
      const float* src = sRed + (size_t)(g - 1) * PER_GRP + wave * PER_WAVE + lane;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[mi][ni][r] += src[((mi * NI + ni) * 16 + r) * 64];
    }
    smem_raw = smem_all;               // the epilogue stages from the start of LDS
  }

  if (p.epi_lds && p.splitk <= 1) {
    // Coalesced epilogue: the output tile is assembled in LDS (the ring is idle now) and written as full rows, 16 bytes per
    // lane.  The residual tile is staged the same way, so out = fp16(alpha*acc + bias + residual) with a single rounding.
    // EPASS passes of EROWS rows (pass e = the waves of wave-row e when the tile is staged in parts).  Store loop: thread t owns
    // the fixed 16-byte vector v = t % VPR of row group g = t / VPR and walks rows g, g + G, ...: per-channel sums for the
    // GroupNorm that consumes this tensor fall out of it (fp32 sums of the rounded fp16 values the consumer will read), and every
    // partial is combined in a FIXED order (rows ascending per thread, then groups ascending): bit-reproducible statistics.
    constexpr int OLD = GEO::OLD, VPR = GEO::VPR, G = GEO::G, EPASS = GEO::EPASS, EROWS = GEO::EROWS;
    half_t* sOut = reinterpret_cast<half_t*>(smem_raw);
    const bool tr_tile = p.outT != nullptr && n0 >= p.vt_col0;      // block-uniform (the launcher aligns vt_col0 to the tile width)
    const int sv = tid % VPR, sg = tid / VPR;
    const bool s_active = sg < G;
    float cs[8], cq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { cs[j] = 0.f; cq[j] = 0.f; }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPASS; ++e) {
      const int r0 = e * EROWS;                         // first tile row of this pass
      const bool res_staged = p.res && !p.res_late;
      if (res_staged) {
        if (s_active) {
          // clamped addresses instead of predicated loads: the loads of an unrolled group issue back to back (rows past M / columns
          // past N stage finite junk that is never stored)
          const int nres = min(n0 + sv * 8, p.N - 8);
#pragma unroll 8
          for (int r = sg; r < EROWS; r += G) {
            const int m = min(m0 + r0 + r, p.M - 1);
            *reinterpret_cast<half8*>(sOut + r * OLD + sv * 8) = ldg_half8(p.res + (size_t)m * p.ldres + nres);
          }
        }
        __syncthreads();
      }
      if (tr_tile) {
        // V^T-style output (columns >= vt_col0 are written transposed per batch item): the tile is staged TRANSPOSED, [BN][EROWS + 8],
        // and leaves as 16-byte runs of 8 consecutive tokens of one output channel
        constexpr int TOLD = GEO::TOLD, VPT = EROWS / 8;
        if (EPASS == 1 || (wave >> 1) == e) {
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            const int ml = wm0 - r0 + mi * 32 + (lane & 31);
            const int mlp = p.vt_perm16 ? vt_perm16_pos(ml) : ml;      // tiles start on multiples of 16 tokens: permute inside the tile
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const int nl = wn0 + ni * 32 + 8 * g + 4 * (lane >> 5);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  float o = acc[mi][ni][4 * g + j] * p.alpha;
                  if (ebias && n0 + nl + j < p.N) o += ebias[n0 + nl + j];
                  sOut[(nl + j) * TOLD + mlp] = (half_t)o;
                }
              }
            }
          }
        }
        __syncthreads();
        const int ncol = p.N - p.vt_col0;
        for (int idx = tid; idx < BN * VPT; idx += NT) {
          const int nl = idx / VPT, v = idx - nl * VPT;
          const int n = n0 + nl, m = m0 + r0 + v * 8;
          if (n < p.N && m < p.M) {
            const int b = m / p.rows_per_batch, tok = m - b * p.rows_per_batch;
            half_t* dst = (half_t*)p.outT + ((size_t)b * ncol + (n - p.vt_col0)) * p.vt_ld + tok;
            *reinterpret_cast<half8*>(dst) = *reinterpret_cast<const half8*>(sOut + nl * TOLD + v * 8);
          }
        }
        if (e + 1 < EPASS) __syncthreads();
        continue;
      }
      if (EPASS == 1 || (wave >> 1) == e) {
        // two copies, selected by a block-uniform branch: with the bias already in the accumulators (the usual case) the staging
        // loop has no per-element control flow at all
        auto stage = [&](auto has_bias) {
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            const int ml = wm0 - r0 + mi * 32 + (lane & 31);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
              half4* slot0 = reinterpret_cast<half4*>(sOut + ml * OLD + wn0 + ni * 32 + 4 * (lane >> 5));   // slot of group g: + 2 * g
              half4 r4[4];
              if (res_staged) {                  // the four residual slots of this 32-column tile in flight together
#pragma unroll
                for (int g = 0; g < 4; ++g) r4[g] = slot0[2 * g];
              }
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn0 + ni * 32 + 8 * g + 4 * (lane >> 5);
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  o[j] = acc[mi][ni][4 * g + j] * p.alpha;
                  if constexpr (decltype(has_bias)::value) { if (n + j < p.N) o[j] += ebias[n + j]; }
                }
                if (res_staged) {
#pragma unroll
                  for (int j = 0; j < 4; ++j) o[j] += (float)r4[g][j];
                }
                half4 h4 = {(half_t)o[0], (half_t)o[1], (half_t)o[2], (half_t)o[3]};
                slot0[2 * g] = h4;
              }
            }
          }
        };
        if (ebias) stage(std::true_type{}); else stage(std::false_type{});
      }
      __syncthreads();
      if (!p.geglu) {
        const int n = n0 + sv * 8;
        if (s_active && n < p.N) {
#pragma unroll 4
          for (int r = sg; r < EROWS; r += G) {
            const int m = m0 + r0 + r;
            half8 val = *reinterpret_cast<const half8*>(sOut + r * OLD + sv * 8);
            if (m < p.M) {
              if (p.res && p.res_late) {   // residual added on the way out (coalesced 16-byte reads, no staging pass / barrier)
                const half8 rv = ldg_half8(p.res + (size_t)m * p.ldres + n);
#pragma unroll
                for (int j = 0; j < 8; ++j) val[j] = (half_t)((float)val[j] + (float)rv[j]);
              }
              *reinterpret_cast<half8*>(p.out + (size_t)m * p.ldo + n) = val;
              if (p.stats) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { float f = (float)val[j]; cs[j] += f; cq[j] += f * f; }
              }
            }
          }
        }
      } else {
        constexpr int VPO = BN / 16;
        for (int idx = tid; idx < EROWS * VPO; idx += NT) epilogue_geglu_vec<BN, OLD>(p, sOut, m0 + r0, n0, idx);
      }
      if (e + 1 < EPASS) __syncthreads();               // the next pass overwrites the staging rows
    }
    if (p.stats && !p.geglu) {
      float* sSt = reinterpret_cast<float*>(sOut + EROWS * OLD);       // [G][BN][2]
      if (s_active) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          sSt[(sg * BN + sv * 8 + j) * 2 + 0] = cs[j];
          sSt[(sg * BN + sv * 8 + j) * 2 + 1] = cq[j];
        }
      }
      __syncthreads();
      for (int c = tid; c < BN; c += NT) {
        if (n0 + c < p.N) {
          float s = 0.f, q = 0.f;
#pragma unroll
          for (int g = 0; g < G; ++g) { s += sSt[(g * BN + c) * 2]; q += sSt[(g * BN + c) * 2 + 1]; }
          float* dst = p.stats + ((size_t)bx * p.N + n0 + c) * 2;
          dst[0] = s;
          dst[1] = q;
        }
      }
    }
    return;
  }

#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = m0 + wm0 + mi * 32 + (lane & 31);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int nb = n0 + wn0 + ni * 32 + 8 * g + 4 * (lane >> 5);
        float v[4] = {acc[mi][ni][4 * g + 0], acc[mi][ni][4 * g + 1], acc[mi][ni][4 * g + 2], acc[mi][ni][4 * g + 3]};
        if (p.splitk > 1) {
          if (m < p.M) {
            float* dst = p.slab + ((size_t)bz * p.M + m) * p.N + nb;
            if (nb + 3 < p.N) *reinterpret_cast<floatx4*>(dst) = floatx4{v[0], v[1], v[2], v[3]};
            else {
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (nb + j < p.N) dst[j] = v[j];
            }
          }
        } else {
          epilogue_store4(p, m, nb, v, ebias);
        }
      }
    }
  }
}

