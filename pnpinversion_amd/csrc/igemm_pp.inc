// igemm_pp_kernel: the 8-wave "ping-pong" LDS-DMA implicit-GEMM kernel (included by gemm.hip).
//
// Same operator as igemm_dma_kernel (igemm_dma.inc: conv 3x3 / 1x1 / linear of resnet.py:289-358 and attention.py:125-333 as one
// gather-GEMM with fused epilogues), built for ONE workgroup of 8 wavefronts per CU instead of 2-3 workgroups of 4:
//
//   * tile BM x BN x 64 with BM x BN = 256 x 256 or 192 x 320 (128 / 120 FLOP per operand byte against 64 for 128 x 128: the LDS-DMA
//     path, which paces the 4-wave kernels, carries half the bytes per FLOP), v_mfma_f32_16x16x32_f16 (tiles are multiples of 16, so
//     192 x 320 exists: (49152, 320), (12288, 640) x split 2, (3072, 1280) x split 4 all give exactly 256 workgroups);
//   * each BN also has a shorter tile, 128 x 320 and 192 x 256 (91 / 110 FLOP per operand byte), for the launches whose row count
//     leaves the taller tile with a part-filled round of workgroups (the 8-row lock step: (32768, 320) is 171 tiles of 192 rows but
//     exactly 256 of 128).  An output element's K walk (K-tiles in order, two k-steps each) and its split-K ranges do not depend on
//     BM, and the GroupNorm partial sums keep one reduction tree per BN (PpGeom::GPS), so the tiles of one BN are interchangeable
//     bit for bit; launch_igemm picks the row height on the launched M (pp_rowtile_pick in gemm.hip, tuning "pp_rowtile");
//   * the two waves that share a SIMD (wave w and w + 4) run half a phase apart: while one issues its MFMAs (s_setprio 1) the
//     other reads its fragments and issues its DMA instructions, then they swap -- the matrix pipe of every SIMD always has a wave in
//     its MFMA section.  Two raw s_barriers per phase keep the two groups in that order (group 1 starts one barrier late);
//   * a K-tile (64 deep, 128-byte rows) is walked in 4 phases = the 4 quadrants of the wave tile (a0 w0, a1 w0, a1 w1, a0 w1), so
//     the regions of the K-tile buffer fall idle one after the other and the NEXT use of the buffer (K-tile t + 2) is re-staged
//     region by region while K-tile t + 1 is computed: two K-tile buffers (128 KB), every DMA instruction is issued four phases
//     (one whole K-tile of MFMA time) before the counted `s_waitcnt vmcnt(N)` that retires it and five before its first read;
//     vmcnt never reaches 0 inside the loop;
//   * LDS layout: 16-row fragment blocks of 128-byte rows, 16-byte chunk c of row r stored at chunk c ^ ((r >> 1) & 7); the DMA
//     destination is lane-linear, so the permutation is applied to the per-lane SOURCE address and again on the fragment read
//     (conflict-free for the 4 x 16 lane groups of ds_read_b128, MI355X_MICROARCH.md "LDS").
//
// Protocol (p = phase counter, one DMA batch per phase; batches b1..b4 of a K-tile are the slots of its buffer in storage order
// [W0 | A0 | A1 | W1]):  batch issued in phase p  ->  `vmcnt` in phase p + 4 retires it (every wave waits for its own part, the
// phase's first barrier publishes it)  ->  first fragment read in phase p + 5 or later (RAW: one phase after the wait, which also
// covers the one-barrier stagger between the groups);  a region is re-staged two or more phases after its last read (WAR).
//
// Unequal batches.  The shorter tiles have 7 slots per K-tile ([W0 W0 | A0 | A1 | W1 W1 W1] and [W0 W0 | A0 | A1 A1 | W1 W1]), split
// 1, 2, 2, 2 (CB = 1, 3, 5, 7; PpGeom's static_assert: W0 and A0 end inside batch 2, A1 inside batch 3, A1 starts in batch >= 2, W1 in
// batch >= 3).  Every wave issues exactly one instruction per slot, in a fixed order, so with N1..N4 the batch sizes and
// NALL = N1 + N2 + N3 + N4 each counted wait is "the instructions issued BEHIND the batch that must have landed" -- never more (more
// would let that batch stay in flight: a race), and written in N1..N4, not in NALL / 4:
//   prologue      issued T0 b1 b2 b3 b4 [T1 b1 b2]; needs T0 b1 b2; behind them: N3 + N4 [+ N1 + N2 = NALL].
//   phase 1       (rem >= 1) issues T(t+1) b3; needs T(t) b3; behind it: T(t) b4, T(t+1) b1 b2 b3 = NALL -- T(t+1) b1 b2 were issued by
//                 the prologue (t = 0) or by phases 3, 4 of K-tile t - 1, where rem was >= 2.  (rem = 0) nothing issued since T(t) b4: N4.
//   phase 2       (rem >= 1) issues T(t+1) b4; needs T(t) b4; behind it: T(t+1) b1 b2 b3 b4 = NALL.  (rem = 0) the queue's tail: 0.
//   phase 3       issues T(t+2) b1 when rem >= 2; no wait (phase 4 reads nothing new).
//   phase 4       (rem >= 2) issues T(t+2) b2; needs T(t+1) b1 b2; behind them: T(t+1) b3 b4, T(t+2) b1 b2 = NALL.  (rem = 1) phases
//                 3, 4 issued nothing: behind them T(t+1) b3 b4 = N3 + N4.  (rem = 0) nothing left.
// nt = 1: prologue N3 + N4, then N4, 0.  nt = 2: prologue NALL; t = 0: NALL, NALL, -, N3 + N4; t = 1: N4, 0.  nt = 3: t = 0 runs the
// steady state (rem = 2), t = 1 as nt = 2's t = 0, t = 2 as its t = 1; odd / even nt differ only in the buffer a K-tile lands in.
// The counts hold for any batch sizes; what unequal batches change is only which slots share a batch (the RAW / WAR assert above).
#pragma once
#include "igemm_dma.inc"

// a pointer the compiler computed on the VALU (64-bit multiplies have no scalar form) back into SGPRs: buffer descriptors must be wave-uniform
__device__ __forceinline__ const half_t* uniform_ptr(const half_t* q) {
  const unsigned long long v = (unsigned long long)q;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return (const half_t*)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ floatx4 mfma16(half8 a, half8 b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

constexpr int pp_pow2_floor(int v) { int r = 1; while (2 * r <= v) r *= 2; return r; }

template <int BM, int BN, int MI0, int NI0>
struct PpGeom {
  static constexpr int WGM = 4, WGN = 2, NWV = 8, NT = 512;
  static constexpr int WM = BM / WGM, WN = BN / WGN, MI = WM / 16, NI = WN / 16, MI1 = MI - MI0, NI1 = NI - NI0;
  // K-tile buffer regions (rows), storage order [W0 | A0 | A1 | W1]; every region a multiple of 64 rows = one DMA slot (8 waves x 8 rows)
  static constexpr int RW0 = WGN * NI0 * 16, RA0 = WGM * MI0 * 16, RA1 = WGM * MI1 * 16, RW1 = WGN * NI1 * 16;
  static constexpr int SW0 = RW0 / 64, SA0 = RA0 / 64, SA1 = RA1 / 64, SW1 = RW1 / 64;     // slots per region
  static constexpr int OW0 = 0, OA0 = RW0, OA1 = RW0 + RA0, OW1 = RW0 + RA0 + RA1;          // first row of each region
  static constexpr int NPW = (BM + BN) / 64, NAS = BM / 64, NWS = BN / 64;                  // slots per K-tile: all / activation / weight
  static constexpr int KT_BYTES = (BM + BN) * 128, RING = 2 * KT_BYTES;
  // DMA batches: slots [CB[b-1], CB[b]) are issued together; NPW = 8: four batches of two instructions per wave; NPW = 7 (the 128 x 320
  // and 192 x 256 tiles): CB = 1, 3, 5, 7, batches of 1, 2, 2, 2 ("Unequal batches" in the header comment)
  static constexpr int CB0 = 0, CB1 = NPW / 4, CB2 = NPW / 2, CB3 = (3 * NPW) / 4, CB4 = NPW;
  static_assert(RW0 % 64 == 0 && RA0 % 64 == 0 && RA1 % 64 == 0 && RW1 % 64 == 0, "regions are whole DMA slots");
  static_assert(MI0 > 0 && MI1 > 0 && NI0 > 0 && NI1 > 0 && WM % 16 == 0 && WN % 16 == 0, "quadrants");
  // RAW: what phase 1 reads (W0, A0) lies in batches 1-2, A1 (phase 2) in batches <= 3.  WAR: A1 (last read in phase 2) in batches >= 2,
  // W1 (phase 3) in batches >= 3.
  static_assert(SW0 + SA0 <= CB2 && SW0 + SA0 + SA1 <= CB3 && SW0 + SA0 >= CB1 && SW0 + SA0 + SA1 >= CB2, "batch / region schedule");
  // Epilogue: the output tile staged as [rows][BN + 8] halfs, EPASS passes of EROWS rows; G row groups of VPR 16-byte vectors; GroupNorm
  // statistics per 64-row sub-block (64 divides every H*W of the UNet, 192 does not), GPS row groups per sub-block.
  static constexpr int OLD = BN + 8, VPR = BN / 8, G = NT / VPR;
  static constexpr int STATS_B = G * BN * 2 * 4;
  static constexpr int EPASS = (BM * OLD * 2 + STATS_B <= 160 * 1024) ? 1 : 2;
  // GPS = the largest power of two the row groups allow: GA = SB * GPS of the G groups store (8 of 12 in the 128 x 320 tile), so that
  // the reduction tree of a sub-block's statistics (RPT rows per thread, then GPS groups) is the same for every BM of one BN
  static constexpr int EROWS = BM / EPASS, SB = EROWS / 64, GPS = pp_pow2_floor(G / SB), RPT = 64 / GPS, GA = SB * GPS;   // sub-blocks per pass, groups per sub-block, rows per thread, storing groups
  static constexpr int TOLD = EROWS + 8;
  static constexpr int EPI_PLAIN = EROWS * OLD * 2 + STATS_B, EPI_TR = BN * TOLD * 2;
  static constexpr int EPI = EPI_PLAIN > EPI_TR ? EPI_PLAIN : EPI_TR;
  static constexpr int LDS = RING > EPI ? RING : EPI;
  static_assert(LDS <= 160 * 1024, "LDS");
  static_assert(EROWS % 64 == 0 && GA <= G && GPS >= 1 && 64 % GPS == 0 && (WGM / EPASS) * WM == EROWS, "epilogue geometry");
};

template <int BM, int BN, int MI0, int NI0, int ABL = 0>
__global__ void __launch_bounds__(512, 2)
igemm_pp_kernel(GemmP p_in) {
  GemmP p = p_in;
  using GEO = PpGeom<BM, BN, MI0, NI0>;
  constexpr int WGN = GEO::WGN, NT = GEO::NT;
  constexpr int WM = GEO::WM, WN = GEO::WN, MI = GEO::MI, NI = GEO::NI, MI1 = GEO::MI1, NI1 = GEO::NI1;
  constexpr int SW0 = GEO::SW0, SA0 = GEO::SA0, SA1 = GEO::SA1, NPW = GEO::NPW, NAS = GEO::NAS, NWS = GEO::NWS;
  constexpr int KT_BYTES = GEO::KT_BYTES;
  constexpr int NIX = NI0 > NI1 ? NI0 : NI1;
  extern __shared__ __attribute__((aligned(1024))) char smem_raw[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int wm0 = wm * WM, wn0 = wn * WN;
  const int grp = wave >> 2;                       // waves w and w + 4 share a SIMD: one of each group per SIMD
  int bx, by, bz;
  {   // XCD-aware tile order, as igemm_dma_kernel
    const int T = p.gx * p.gy * p.gz, per = (T + 7) >> 3;
    const int tix = p.tile_order == 2 ? (int)blockIdx.x : (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (tix >= T) return;
    if (p.tile_order == 0) { by = tix % p.gy; const int t = tix / p.gy; bx = t % p.gx; bz = t / p.gx; }
    else { bx = tix % p.gx; const int t = tix / p.gx; by = t % p.gy; bz = t / p.gy; }
  }
  const int m0 = bx * BM, n0 = by * BN;
  if (p.nbatch > 1) {
    p.x1 += (size_t)bz * p.sx1;
    p.w += (size_t)bz * p.sw;
    if (p.out) p.out += (size_t)bz * p.sout;
    if (p.outT) p.outT = (char*)p.outT + (size_t)bz * p.soutT;
  }
  const int Cin = p.C1 + p.C2;
  const int HoWo = p.Ho * p.Wo;
  const int nchunks = p.K / 64;
  int kc0 = 0, kc1 = nchunks;
  if (p.splitk > 1) { kc0 = bz * p.kchunks_per_split; kc1 = min(nchunks, kc0 + p.kchunks_per_split); }
  const int nt = kc1 > kc0 ? kc1 - kc0 : 0;

  // ---- DMA lane roles.  A wave-level instruction fills 8 rows x 128 bytes lane-linearly: lane l lands at row (l >> 3), chunk (l & 7) of
  // its half fragment block, so it FETCHES logical chunk (l & 7) ^ swz with swz = ((row in the 16-row block) >> 1) & 7 = 4 * half + (l >> 4).
  const int d_half = wave & 1;                                        // slot bases are multiples of 64 rows: the half is the wave's parity
  const int d_chunk = ((lane & 7) ^ (4 * d_half + (lane >> 4))) * 8;  // halfs
  const int d_row = d_half * 8 + (lane >> 3);                         // row inside the fragment block
  // tile row of this lane for activation slot i / weight slot i (slots in region order A0, A1 / W0, W1)
  auto a_tile_row = [&](int i) {
    const int f = (i < SA0 ? i : i - SA0) * 4 + (wave >> 1);          // fragment block inside its region
    return i < SA0 ? (f / MI0) * WM + (f % MI0) * 16 + d_row : (f / MI1) * WM + (MI0 + f % MI1) * 16 + d_row;
  };
  auto w_tile_row = [&](int i) {
    const int f = (i < SW0 ? i : i - SW0) * 4 + (wave >> 1);
    return i < SW0 ? (f / NI0) * WN + (f % NI0) * 16 + d_row : (f / NI1) * WN + (NI0 + f % NI1) * 16 + d_row;
  };
  // Addressing through buffer descriptors (buffer_load_dwordx4 ... offen lds): one 32-bit byte offset per DMA slot in a VGPR, the k-walk
  // in the descriptor's (wave-uniform) base address, and an offset >= num_records (2 GiB) makes the lane read zeros -- conv padding and
  // rows past M without a zero page.  Weight rows past N are clamped to row N - 1 (their products land in columns that are never stored).
  int a_y0[NAS], a_x0[NAS], a_bh[NAS];      // yo * stride - pad, xo * stride - pad (a linear layer is one image row of M pixels: x runs to M), batch index * H
#pragma unroll
  for (int i = 0; i < NAS; ++i) {
    const int m = m0 + a_tile_row(i);
    const int b = m / HoWo;
    const int rr = m - b * HoWo;
    const int yo = rr / p.Wo;
    const int xo = rr - yo * p.Wo;
    a_bh[i] = b * p.H;
    a_y0[i] = m < p.M ? yo * p.stride - p.pad : -(1 << 20);      // rows past M fail the bounds test for every tap
    a_x0[i] = xo * p.stride - p.pad;
  }
  const int lim_y = p.ups ? 2 * p.H : p.H, lim_x = p.ups ? 2 * p.W : p.W, ups_sh = p.ups ? 1 : 0;
  unsigned w_voff[NWS];
#pragma unroll
  for (int i = 0; i < NWS; ++i) {
    const int n = min(n0 + w_tile_row(i), p.N - 1);
    w_voff[i] = (unsigned)(n * p.ldw + d_chunk) * 2u;
  }
  const half_t* w_base = uniform_ptr(p.w + (size_t)kc0 * 64);   // wave-uniform: advanced by one K-tile at the first weight slot of every K-tile after the first
  bool w_first = true;
  // k-walk.  Default order = the weight layout's (tap-major: all channels of filter tap 0, then tap 1, ...).  p.k_order = 1 (3 x 3
  // convolutions): channel-slab-major -- the nine taps of one 64-channel slab in a row, so that the activation lines a tile reads for
  // tap (r, s) are re-read for the next tap one K-tile later (still in L2) instead of Cin / 64 K-tiles later.  K-tile q of this order is
  // k = (q % 9) * Cin + (q / 9) * 64; any partition of the q axis is a valid split-K.
  const bool tap_inner = p.k_order == 1 && p.ksize == 3;
  int is_tap = tap_inner ? kc0 % 9 : (kc0 * 64) / Cin;
  int is_c0 = tap_inner ? (kc0 / 9) * 64 : kc0 * 64 - is_tap * Cin;
  int wq_tap = is_tap, wq_c0 = is_c0;                 // the weight operand's own position of the same walk (its slots are issued first)
  bool retap = true;
  const half_t* a_base = p.x1;
  unsigned a_voff[NAS];
#pragma unroll
  for (int i = 0; i < NAS; ++i) a_voff[i] = 0x80000000u;
  constexpr int SRD_FLAGS = 0x00020000;            // raw buffer, 32-bit data format (gfx90a / gfx942 / gfx950)

  // the gather offsets of the NEXT K-tile's activation slots (rebuilt only when the k-walk enters a new filter tap / concat source),
  // called at that K-tile's first activation slot; then the k-walk moves on
  auto prep_a = [&]() {
    if (retap) {
      int r = 0, s = 0;
      if (p.ksize == 3) { r = is_tap / 3; s = is_tap - 3 * r; }
      int ld;
      if (is_c0 < p.C1) { a_base = uniform_ptr(p.x1 + is_c0); ld = p.ldx1; } else { a_base = uniform_ptr(p.x2 + (is_c0 - p.C1)); ld = p.ldx2; }
#pragma unroll
      for (int i = 0; i < NAS; ++i) {
        const int yi = a_y0[i] + r, xi = a_x0[i] + s;
        const bool ok = (unsigned)yi < (unsigned)lim_y && (unsigned)xi < (unsigned)lim_x;
        const unsigned off = (unsigned)(((a_bh[i] + (yi >> ups_sh)) * p.W + (xi >> ups_sh)) * ld + d_chunk) * 2u;
        a_voff[i] = ok ? off : 0x80000000u;
      }
      retap = false;
    } else {
      a_base += 64;
    }
    if (tap_inner) {
      ++is_tap; retap = true;
      if (is_tap == 9) { is_tap = 0; is_c0 += 64; }
    } else {
      is_c0 += 64;
      if (is_c0 >= Cin) { is_c0 = 0; ++is_tap; retap = true; }
      else if (is_c0 == p.C1) retap = true;
    }
  };
  // slot k (storage order) of K-tile buffer `buf`
  auto issue_slot = [&](auto kc, char* buf) {
    constexpr int k = decltype(kc)::value;
    char* dst = buf + (64 * k + 8 * wave) * 128;
    if constexpr (k >= SW0 && k < SW0 + SA0 + SA1) {
      constexpr int i = k - SW0;
      if constexpr (i == 0) prep_a();
      if (ABL != 2 && ABL != 4)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(__builtin_amdgcn_make_buffer_rsrc((void*)a_base, 0, (int)0x80000000, SRD_FLAGS), (lds_ptr_t)dst, 16,
                                                 (int)a_voff[i], 0, 0, 0);
    } else {
      constexpr int i = k < SW0 ? k : k - SA0 - SA1;
      if constexpr (k == 0) {
        if (tap_inner) {
          w_base = uniform_ptr(p.w + (size_t)(wq_tap * Cin + wq_c0));
          if (++wq_tap == 9) { wq_tap = 0; wq_c0 += 64; }
        } else {
          if (!w_first) w_base += 64;
          w_first = false;
        }
      }
      if (ABL != 2 && ABL != 4)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(__builtin_amdgcn_make_buffer_rsrc((void*)w_base, 0, (int)0x80000000, SRD_FLAGS), (lds_ptr_t)dst, 16,
                                                 (int)w_voff[i], 0, 0, 0);
    }
  };
  auto issue_batch = [&](auto bc, char* buf) {
    constexpr int b = decltype(bc)::value;
    constexpr int lo = b == 1 ? GEO::CB0 : b == 2 ? GEO::CB1 : b == 3 ? GEO::CB2 : GEO::CB3;
    constexpr int hi = b == 1 ? GEO::CB1 : b == 2 ? GEO::CB2 : b == 3 ? GEO::CB3 : GEO::CB4;
    if constexpr (hi - lo > 0) issue_slot(std::integral_constant<int, lo>{}, buf);
    if constexpr (hi - lo > 1) issue_slot(std::integral_constant<int, lo + 1>{}, buf);
    if constexpr (hi - lo > 2) issue_slot(std::integral_constant<int, lo + 2>{}, buf);
    if constexpr (hi - lo > 3) issue_slot(std::integral_constant<int, lo + 3>{}, buf);
    static_assert(hi - lo <= 4, "batch");
  };
  constexpr int N1 = GEO::CB1 - GEO::CB0, N2 = GEO::CB2 - GEO::CB1, N3 = GEO::CB3 - GEO::CB2, N4 = GEO::CB4 - GEO::CB3;

  floatx4 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};

  // ---- fragment read addressing: lane l reads row (l & 15), logical chunk 4 * ks + (l >> 4) of a 16-row block; k-step 1 = address ^ 64
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem_raw;
  const unsigned fr = lane & 15;
  const unsigned lane_off = fr * 128 + ((((unsigned)lane >> 4) ^ ((fr >> 1) & 7)) << 4);
  const unsigned rA0 = lds_base + (GEO::OA0 + wm * MI0 * 16) * 128 + lane_off;
  const unsigned rA1 = lds_base + (GEO::OA1 + wm * MI1 * 16) * 128 + lane_off;
  const unsigned rW0 = lds_base + (GEO::OW0 + wn * NI0 * 16) * 128 + lane_off;
  const unsigned rW1 = lds_base + (GEO::OW1 + wn * NI1 * 16) * 128 + lane_off;

  half8 fa0[MI0][2], fa1[MI1][2], fw[NIX][2];
  if (ABL >= 3) {      // ablations without fragment reads: defined operands
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
      for (int i = 0; i < MI0; ++i) fa0[i][k] = zero_half8() + (half_t)(float)lane;
#pragma unroll
      for (int i = 0; i < MI1; ++i) fa1[i][k] = zero_half8() + (half_t)1.f;
#pragma unroll
      for (int i = 0; i < NIX; ++i) fw[i][k] = zero_half8() + (half_t)(float)(lane & 7);
    }
  }
  auto wait_vm = [&](auto nc) {
    constexpr int n = decltype(nc)::value;
    static_assert(n <= 63, "vmcnt");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory");
  };
  auto mfma_begin = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
  };
  auto mfma_end = [&]() {
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  auto read_a0 = [&](unsigned boff) {
    if (ABL >= 3) return;
#pragma unroll
    for (int mi = 0; mi < MI0; ++mi) { fa0[mi][0] = lds_read_b128_async(rA0 + boff, mi * 2048); fa0[mi][1] = lds_read_b128_async((rA0 + boff) ^ 64, mi * 2048); }
  };
  auto read_a1 = [&](unsigned boff) {
    if (ABL >= 3) return;
#pragma unroll
    for (int mi = 0; mi < MI1; ++mi) { fa1[mi][0] = lds_read_b128_async(rA1 + boff, mi * 2048); fa1[mi][1] = lds_read_b128_async((rA1 + boff) ^ 64, mi * 2048); }
  };
  auto read_w0 = [&](unsigned boff) {
    if (ABL >= 3) return;
#pragma unroll
    for (int ni = 0; ni < NI0; ++ni) { fw[ni][0] = lds_read_b128_async(rW0 + boff, ni * 2048); fw[ni][1] = lds_read_b128_async((rW0 + boff) ^ 64, ni * 2048); }
  };
  auto read_w1 = [&](unsigned boff) {
    if (ABL >= 3) return;
#pragma unroll
    for (int ni = 0; ni < NI1; ++ni) { fw[ni][0] = lds_read_b128_async(rW1 + boff, ni * 2048); fw[ni][1] = lds_read_b128_async((rW1 + boff) ^ 64, ni * 2048); }
  };
  constexpr int NALL = N1 + N2 + N3 + N4;

  if (nt > 0) {
    // prologue: the whole first K-tile and the first half of the second
    issue_batch(std::integral_constant<int, 1>{}, smem_raw);
    issue_batch(std::integral_constant<int, 2>{}, smem_raw);
    issue_batch(std::integral_constant<int, 3>{}, smem_raw);
    issue_batch(std::integral_constant<int, 4>{}, smem_raw);
    if (nt > 1) {
      issue_batch(std::integral_constant<int, 1>{}, smem_raw + KT_BYTES);
      issue_batch(std::integral_constant<int, 2>{}, smem_raw + KT_BYTES);
      wait_vm(std::integral_constant<int, NALL>{});
    } else {
      wait_vm(std::integral_constant<int, N3 + N4>{});
    }
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();       // group 1 runs one barrier behind group 0 from here on
    // K-tile t computes from buffer t & 1 and issues batches 3, 4 of K-tile t + 1 (the other buffer) and 1, 2 of K-tile t + 2 (its own).
    // The vmcnt of a phase = the instructions of the batches that may stay in flight behind the one the NEXT phase reads (wave-uniform
    // branches pick the drain values of the last two K-tiles).
    for (int t = 0; t < nt; ++t) {
      const int rem = nt - 1 - t;                                   // K-tiles after this one
      const unsigned boff = (t & 1) ? (unsigned)KT_BYTES : 0u;
      char* const bsame = smem_raw + boff;
      char* const bnext = smem_raw + (KT_BYTES - boff);
      // ---------------- phase 1: a0 x w0
      read_a0(boff);
      read_w0(boff);
      if (rem >= 1) { issue_batch(std::integral_constant<int, 3>{}, bnext); wait_vm(std::integral_constant<int, NALL>{}); }   // retires batch 3 of this K-tile (phase 2 reads A1)
      else wait_vm(std::integral_constant<int, N4>{});
      mfma_begin();
      if (ABL != 1 && ABL != 3) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int mi = 0; mi < MI0; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI0; ++ni) acc[mi][ni] = mfma16(fw[ni][ks], fa0[mi][ks], acc[mi][ni]);
      }
      mfma_end();
      // ---------------- phase 2: a1 x w0
      read_a1(boff);
      if (rem >= 1) { issue_batch(std::integral_constant<int, 4>{}, bnext); wait_vm(std::integral_constant<int, NALL>{}); }   // retires batch 4 of this K-tile (phase 3 reads W1)
      else wait_vm(std::integral_constant<int, 0>{});
      mfma_begin();
      if (ABL != 1 && ABL != 3) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int mi = 0; mi < MI1; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI0; ++ni) acc[MI0 + mi][ni] = mfma16(fw[ni][ks], fa1[mi][ks], acc[MI0 + mi][ni]);
      }
      mfma_end();
      // ---------------- phase 3: a1 x w1 (nothing new is read in phase 4: no wait)
      read_w1(boff);
      if (rem >= 2) issue_batch(std::integral_constant<int, 1>{}, bsame);
      mfma_begin();
      if (ABL != 1 && ABL != 3) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int mi = 0; mi < MI1; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI1; ++ni) acc[MI0 + mi][NI0 + ni] = mfma16(fw[ni][ks], fa1[mi][ks], acc[MI0 + mi][NI0 + ni]);
      }
      mfma_end();
      // ---------------- phase 4: a0 x w1 (a0 is still in registers)
      if (rem >= 2) { issue_batch(std::integral_constant<int, 2>{}, bsame); wait_vm(std::integral_constant<int, NALL>{}); }    // retires batches 1, 2 of the next K-tile (its phase 1)
      else if (rem == 1) wait_vm(std::integral_constant<int, N3 + N4>{});
      mfma_begin();
      if (ABL != 1 && ABL != 3) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int mi = 0; mi < MI0; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI1; ++ni) acc[mi][NI0 + ni] = mfma16(fw[ni][ks], fa0[mi][ks], acc[mi][NI0 + ni]);
      }
      mfma_end();
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();       // group 0 catches the last barrier of group 1
  }
  // ---- epilogue (the formats of igemm_dma_kernel's: LDS-staged full-row stores with residual / GEGLU / GroupNorm statistics / V^T, or
  // split-K slabs / the scalar fallback).  Accumulator j of fragment (mi, ni): pixel m = mi * 16 + (lane & 15), channel n = ni * 16 +
  // 4 * (lane >> 4) + j -- four consecutive channels of one pixel per lane.
  const float* ebias = p.bias;
  const int fl = lane & 15, fq = lane >> 4;
  if (p.epi_lds && p.splitk <= 1) {
    constexpr int OLD = GEO::OLD, VPR = GEO::VPR, EPASS = GEO::EPASS, EROWS = GEO::EROWS, GPS = GEO::GPS, RPT = GEO::RPT, SB = GEO::SB;
    half_t* sOut = reinterpret_cast<half_t*>(smem_raw);
    const bool tr_tile = p.outT != nullptr && n0 >= p.vt_col0;      // block-uniform (the launcher aligns vt_col0 to the tile width)
    const int sv = tid % VPR, sg = tid / VPR;
    const bool s_active = sg < GEO::GA;                             // the 128 x 320 tile: 8 of its 12 row groups
    const int srow0 = (sg / GPS) * 64 + (sg % GPS);                 // store loop: rows srow0 + GPS * k of the pass, all inside one 64-row sub-block
    floatx4 bv[NI];
    if (ebias) {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int n = n0 + wn0 + ni * 16 + 4 * fq;
        bv[ni] = *reinterpret_cast<const floatx4*>(ebias + min(n, p.N - 4));     // N % 4 == 0 (epi_lds needs N % 8 == 0)
        if (n >= p.N) bv[ni] = floatx4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) bv[ni] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPASS; ++e) {
      const int r0 = e * EROWS;
      const bool mine = EPASS == 1 || (wm / (GEO::WGM / EPASS)) == e;
      const bool res_staged = p.res && !p.res_late;
      float cs[8], cq[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { cs[j] = 0.f; cq[j] = 0.f; }
      if (res_staged) {
        if (s_active) {
          const int nres = min(n0 + sv * 8, p.N - 8);
#pragma unroll 8
          for (int k = 0; k < RPT; ++k) {
            const int r = srow0 + GPS * k;
            const int m = min(m0 + r0 + r, p.M - 1);
            *reinterpret_cast<half8*>(sOut + r * OLD + sv * 8) = ldg_half8(p.res + (size_t)m * p.ldres + nres);
          }
        }
        __syncthreads();
      }
      if (tr_tile) {
        constexpr int TOLD = GEO::TOLD, VPT = EROWS / 8;
        if (mine) {
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            const int ml = wm0 - r0 + mi * 16 + fl;
            const int mlp = p.vt_perm16 ? vt_perm16_pos(ml) : ml;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
              const int nl = wn0 + ni * 16 + 4 * fq;
#pragma unroll
              for (int j = 0; j < 4; ++j) sOut[(nl + j) * TOLD + mlp] = (half_t)(acc[mi][ni][j] * p.alpha + bv[ni][j]);
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
      if (mine) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const int ml = wm0 - r0 + mi * 16 + fl;
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            half4* slot = reinterpret_cast<half4*>(sOut + ml * OLD + wn0 + ni * 16 + 4 * fq);
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = acc[mi][ni][j] * p.alpha + bv[ni][j];
            if (res_staged) {
              const half4 r4 = *slot;
#pragma unroll
              for (int j = 0; j < 4; ++j) o[j] += (float)r4[j];
            }
            const half4 h4 = {(half_t)o[0], (half_t)o[1], (half_t)o[2], (half_t)o[3]};
            *slot = h4;
          }
        }
      }
      __syncthreads();
      if (!p.geglu) {
        const int n = n0 + sv * 8;
        if (s_active && n < p.N) {
#pragma unroll 4
          for (int k = 0; k < RPT; ++k) {
            const int r = srow0 + GPS * k;
            const int m = m0 + r0 + r;
            half8 val = *reinterpret_cast<const half8*>(sOut + r * OLD + sv * 8);
            if (m < p.M) {
              if (p.res && p.res_late) {
                const half8 rv = ldg_half8(p.res + (size_t)m * p.ldres + n);
#pragma unroll
                for (int j = 0; j < 8; ++j) val[j] = (half_t)((float)val[j] + (float)rv[j]);
              }
              *reinterpret_cast<half8*>(p.out + (size_t)m * p.ldo + n) = val;
              if (p.stats) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float f = (float)val[j]; cs[j] += f; cq[j] += f * f; }
              }
            }
          }
        }
      } else {
        constexpr int VPO = BN / 16;
        for (int idx = tid; idx < EROWS * VPO; idx += NT) epilogue_geglu_vec<BN, OLD>(p, sOut, m0 + r0, n0, idx);
      }
      if (p.stats && !p.geglu) {
        // per (64-row sub-block, channel) sum / sum of squares of the stored fp16 values, combined in a FIXED order (rows ascending per
        // thread, then the sub-block's row groups ascending): bit-reproducible; partial index = (first row of the sub-block) / 64
        float* sSt = reinterpret_cast<float*>(sOut + EROWS * OLD);       // [G][BN][2]
        if (s_active) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            sSt[(sg * BN + sv * 8 + j) * 2 + 0] = cs[j];
            sSt[(sg * BN + sv * 8 + j) * 2 + 1] = cq[j];
          }
        }
        __syncthreads();
        for (int idx = tid; idx < SB * BN; idx += NT) {
          const int sb = idx / BN, c = idx - sb * BN;
          const int mrow = m0 + r0 + sb * 64;
          if (n0 + c < p.N && mrow < p.M) {
            float s_ = 0.f, q_ = 0.f;
#pragma unroll
            for (int g = 0; g < GPS; ++g) { s_ += sSt[((sb * GPS + g) * BN + c) * 2]; q_ += sSt[((sb * GPS + g) * BN + c) * 2 + 1]; }
            float* dst = p.stats + ((size_t)(mrow >> 6) * p.N + n0 + c) * 2;
            dst[0] = s_;
            dst[1] = q_;
          }
        }
        if (e + 1 < EPASS) __syncthreads();
      } else if (e + 1 < EPASS) {
        __syncthreads();
      }
    }
    return;
  }

#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = m0 + wm0 + mi * 16 + fl;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int nb = n0 + wn0 + ni * 16 + 4 * fq;
      float v[4] = {acc[mi][ni][0], acc[mi][ni][1], acc[mi][ni][2], acc[mi][ni][3]};
      {   // split-K slabs (the launcher gives this kernel only launches that take the LDS epilogue or write slabs)
        if (m < p.M) {
          float* dst = p.slab + ((size_t)bz * p.M + m) * p.N + nb;
          if (nb + 3 < p.N) *reinterpret_cast<floatx4*>(dst) = floatx4{v[0], v[1], v[2], v[3]};
          else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (nb + j < p.N) dst[j] = v[j];
          }
        }
      }
    }
  }
}
