// Implicit-GEMM conv3x3 / conv1x1 / linear on v_mfma_f32_32x32x16_f16 (gfx950).
//
// Restates, as one kernel family, what the reference executes through torch.nn.Conv2d / torch.nn.Linear in
//   models/edict/my_diffusers/models/resnet.py:289,298,346,358 (3x3 convs), :30,48 (upsample conv), :74,95 (stride-2 conv),
//   models/edict/my_diffusers/models/attention.py:125,134 (1x1 proj_in/out), :230-234 (to_q/k/v/out), :303-333 (GEGLU FF).
//
// Tiling: 256 threads = 4 wavefronts (2 x 2); block tile BM x BN x 64; each wave owns (BM/2) x (BN/2) as 32x32 MFMA tiles.
// The weight tile is the MFMA "A" operand and the activation tile the "B" operand, so that an accumulator register
// group holds 4 consecutive output channels of one pixel (8-byte NHWC stores, vector bias loads).
// global -> registers -> LDS staging (the conv gather needs per-lane predication, which LDS-DMA cannot do), LDS rows
// padded by 16 B so that ds_read_b128 fragment reads are bank-conflict free (stride 144 B = 36 banks).
#include <stdlib.h>
#include <type_traits>
#include <string.h>

#include "ops.h"
#include "tuning.h"
#include "igemm_dma.inc"
#include "igemm_pp.inc"

static constexpr int BK = 64;
static constexpr int LDS_LD = BK + 8;  // halfs

// problem z of a batched launch (GemmP::nbatch): the operand / output pointers of that problem
__device__ __forceinline__ void gemm_batch_offsets(GemmP& p, int z) {
  p.x1 += (size_t)z * p.sx1;
  p.w += (size_t)z * p.sw;
  if (p.out) p.out += (size_t)z * p.sout;
  if (p.outT) p.outT = (char*)p.outT + (size_t)z * p.soutT;
}

template <int BM, int BN, bool FASTK>
__global__ void __launch_bounds__(256) igemm_kernel(GemmP p_in) {
  GemmP p = p_in;
  if (p.nbatch > 1) gemm_batch_offsets(p, (int)blockIdx.z);
  constexpr int WM = BM / 2, WN = BN / 2, MI = WM / 32, NI = WN / 32;
  constexpr int AV = BM / 32, WV = BN / 32;  // 16-byte vectors per thread per k-chunk
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  half_t* sA = reinterpret_cast<half_t*>(smem_raw);  // [2][BM][LDS_LD]
  half_t* sW = sA + 2 * BM * LDS_LD;                 // [2][BN][LDS_LD]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm0 = (wave >> 1) * WM, wn0 = (wave & 1) * WN;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int kvec = tid & 7, lrow = tid >> 3;
  const int Cin = p.C1 + p.C2;
  const int HoWo = p.Ho * p.Wo;

  int a_y[AV], a_x[AV], a_b[AV];
  bool a_ok[AV];
#pragma unroll
  for (int i = 0; i < AV; ++i) {
    int m = m0 + lrow + 32 * i;
    a_ok[i] = m < p.M;
    int b = m / HoWo;
    int r = m - b * HoWo;
    int yo = r / p.Wo;
    int xo = r - yo * p.Wo;
    a_b[i] = b;
    a_y[i] = yo * p.stride - p.pad;
    a_x[i] = xo * p.stride - p.pad;
  }

  const int nchunks = (p.K + BK - 1) / BK;
  int kc0 = 0, kc1 = nchunks;
  if (p.splitk > 1) {
    kc0 = blockIdx.z * p.kchunks_per_split;
    kc1 = min(nchunks, kc0 + p.kchunks_per_split);
  }

  half8 ra[AV], rw[WV];

  auto load_tiles = [&](int kc) {
    const int k = kc * BK + kvec * 8;
    const bool kok = k < p.K;
#pragma unroll
    for (int i = 0; i < WV; ++i) {
      int n = n0 + lrow + 32 * i;
      rw[i] = (kok && n < p.N) ? ldg_half8(p.w + (size_t)n * p.ldw + k) : zero_half8();
    }
    int tap, c;
    if (FASTK) {
      int kk = kc * BK;
      tap = kk / Cin;
      c = kk - tap * Cin + kvec * 8;
    } else {
      tap = k / Cin;
      c = k - tap * Cin;
    }
    int r = 0, s = 0;
    if (p.ksize == 3) { r = tap / 3; s = tap - 3 * r; }
    const half_t* src; int ld, cc;
    if (c < p.C1) { src = p.x1; ld = p.ldx1; cc = c; } else { src = p.x2; ld = p.ldx2; cc = c - p.C1; }
#pragma unroll
    for (int i = 0; i < AV; ++i) {
      int yi = a_y[i] + r, xi = a_x[i] + s;
      bool ok = a_ok[i] && kok && yi >= 0 && xi >= 0;
      if (p.ups) { ok = ok && yi < 2 * p.H && xi < 2 * p.W; yi >>= 1; xi >>= 1; }
      else { ok = ok && yi < p.H && xi < p.W; }
      ra[i] = ok ? ldg_half8(src + ((size_t)(a_b[i] * p.H + yi) * p.W + xi) * ld + cc) : zero_half8();
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AV; ++i)
      *reinterpret_cast<half8*>(sA + (size_t)(buf * BM + lrow + 32 * i) * LDS_LD + kvec * 8) = ra[i];
#pragma unroll
    for (int i = 0; i < WV; ++i)
      *reinterpret_cast<half8*>(sW + (size_t)(buf * BN + lrow + 32 * i) * LDS_LD + kvec * 8) = rw[i];
  };

  floatx16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  if (kc0 < kc1) {
    load_tiles(kc0);
    store_tiles(0);
    __syncthreads();
    for (int kc = kc0; kc < kc1; ++kc) {
      const int buf = (kc - kc0) & 1;
      const bool more = kc + 1 < kc1;
      if (more) load_tiles(kc + 1);
      const half_t* bA = sA + (size_t)(buf * BM + wm0 + (lane & 31)) * LDS_LD + (lane >> 5) * 8;
      const half_t* bW = sW + (size_t)(buf * BN + wn0 + (lane & 31)) * LDS_LD + (lane >> 5) * 8;
#pragma unroll
      for (int kk = 0; kk < BK / 16; ++kk) {
        half8 wf[NI], af[MI];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) wf[ni] = *reinterpret_cast<const half8*>(bW + ni * 32 * LDS_LD + kk * 16);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) af[mi] = *reinterpret_cast<const half8*>(bA + mi * 32 * LDS_LD + kk * 16);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = mfma32(wf[ni], af[mi], acc[mi][ni]);
      }
      if (more) store_tiles(buf ^ 1);
      __syncthreads();
    }
  }

  // epilogue: accumulator register r of lane l is (n = tile_n + acc_row(r,l), m = tile_m + (l & 31))
  if (p.epi_lds && p.splitk <= 1) {
    // Coalesced epilogue: the output tile is assembled in LDS (the ring is idle now) and written as full rows, 16 bytes per
    // lane.  The residual tile is staged the same way, so out = fp16(alpha*acc + bias + residual) with a single rounding.
    constexpr int OLD = BN + 8;                         // halfs per staged row
    constexpr int VPR = BN / 8;                         // 16-byte vectors per row
    half_t* sOut = reinterpret_cast<half_t*>(smem_raw);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (p.res) {
      for (int idx = tid; idx < BM * VPR; idx += 256) {
        const int r = idx / VPR, v = idx - r * VPR;
        const int m = m0 + r, n = n0 + v * 8;
        half8 val = (m < p.M && n < p.N) ? ldg_half8(p.res + (size_t)m * p.ldres + n) : zero_half8();
        *reinterpret_cast<half8*>(sOut + r * OLD + v * 8) = val;
      }
      __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int ml = wm0 + mi * 32 + (lane & 31);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int nl = wn0 + ni * 32 + 8 * g + 4 * (lane >> 5);
          const int n = n0 + nl;
          half4* slot = reinterpret_cast<half4*>(sOut + ml * OLD + nl);
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = acc[mi][ni][4 * g + j] * p.alpha;
            if (p.bias && n + j < p.N) o[j] += p.bias[n + j];
          }
          if (p.res) {
            half4 r4 = *slot;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += (float)r4[j];
          }
          half4 h4 = {(half_t)o[0], (half_t)o[1], (half_t)o[2], (half_t)o[3]};
          *slot = h4;
        }
      }
    }
    __syncthreads();
    // plain rows only: GEGLU and GroupNorm statistics launches never reach this kernel (igemm_plan gives them a DMA-family tile or fails)
    for (int idx = tid; idx < BM * VPR; idx += 256) {
      const int r = idx / VPR, v = idx - r * VPR;
      const int m = m0 + r, n = n0 + v * 8;
      if (m < p.M && n < p.N)
        *reinterpret_cast<half8*>(p.out + (size_t)m * p.ldo + n) = *reinterpret_cast<const half8*>(sOut + r * OLD + v * 8);
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
            float* dst = p.slab + ((size_t)blockIdx.z * p.M + m) * p.N + nb;
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (nb + j < p.N) dst[j] = v[j];
          }
        } else {
          epilogue_store4(p, m, nb, v, p.bias);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// v2: asynchronous LDS-DMA staging (global_load_lds_dwordx4), no staging registers, no ds_write pass.
//   * each wave-level DMA instruction fills 1 KiB of LDS lane-linearly, so the bank-conflict-free layout is obtained by
//     permuting the per-lane SOURCE address and applying the same involution on the fragment read:
//       logical (row R, 16-byte chunk s)  ->  byte  (R>>4)*2048 + (R&7)*256 + ((R>>3)&1)*128 + ((s ^ (R&7)) * 16)
//     (a ds_read_b128 lane group then touches 16 distinct 16-byte slots of the 256-byte bank row);
//   * conv zero padding / M,N tails: out-of-range lanes read from a zeroed page instead of being masked (a masked DMA lane
//     would leave stale LDS bytes);
//   * two LDS stages (64 KiB at 128x128 -> two blocks per CU); the DMA of chunk k+1 flies under the MFMAs of chunk k and is
//     drained by the vmcnt(0) the compiler puts in front of the one barrier per chunk.
// Requires (C1 + C2) % 64 == 0 and C1 % 64 == 0 (every SD-1.x layer but the 4/3-channel stems, which stay on v1).
// ------------------------------------------------------------------------------------------------------------------
static half_t* g_zero_page = nullptr;   // out-of-range lanes of igemm_dma_kernel read it (igemm_init)

static thread_local int g_last_geom[7] = {0, 0, 0, 0, 0, 0, 0};   // geom of the most recent launch's instance (kInstances; all 0: the v1 kernel)
// What launch_dma and launch_pp share: the logical grid and the XCD traversal order into p, the launch grid flattened and rounded up
// to 8 workgroups, the kernel's dynamic-LDS attribute once per device.
static int dma_launch_prep(GemmP& p, dim3& grid, DeviceOnce& attr_once, const void* kernel, int lds) {
  p.gx = grid.x; p.gy = grid.y; p.gz = grid.z;
  const double bytes_a = 2.0 * p.B * p.H * p.W * (p.C1 + p.C2), bytes_w = 2.0 * (double)p.N * p.K;
  p.tile_order = (bytes_a + 8 * bytes_w <= 8 * bytes_a + bytes_w) ? 0 : 1;
  if (g_tile_order >= 0) p.tile_order = g_tile_order;
  const int total = (int)(grid.x * grid.y * grid.z);
  grid = dim3((unsigned)(((total + 7) / 8) * 8), 1, 1);
  return once_per_device(attr_once, [&]() { return (int)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
}

template <int BM, int BN, int BKT, int NST, int WGM = 2, int ABL = 0, int WK = 1>
static int launch_dma(GemmP p, dim3 grid, hipStream_t st) {
  using GEO = IgemmGeom<BM, BN, BKT, NST, WGM, ABL, WK>;
  static DeviceOnce attr_once;
  if (int r = dma_launch_prep(p, grid, attr_once, (const void*)igemm_dma_kernel<BM, BN, BKT, NST, WGM, ABL, WK>, GEO::LDS)) return r;
  igemm_dma_kernel<BM, BN, BKT, NST, WGM, ABL, WK><<<grid, GEO::NT_ALL, GEO::LDS, st>>>(p, g_zero_page);
  return 0;
}

// The 8-wave ping-pong kernel (igemm_pp.inc): one workgroup per CU, same tile-order / grid conventions as launch_dma.  Its out-of-range
// lanes read zeros through the buffer descriptor's bounds check: no zero page.
template <int BM, int BN, int MI0, int NI0, int ABL = 0>
static int launch_pp(GemmP p, dim3 grid, hipStream_t st) {
  using GEO = PpGeom<BM, BN, MI0, NI0>;
  static DeviceOnce attr_once;
  if (int r = dma_launch_prep(p, grid, attr_once, (const void*)igemm_pp_kernel<BM, BN, MI0, NI0, ABL>, GEO::LDS)) return r;
  igemm_pp_kernel<BM, BN, MI0, NI0, ABL><<<grid, GEO::NT, GEO::LDS, st>>>(p);
  return 0;
}

// The register-staged v1 kernel: its launch, and its dynamic-LDS attribute (igemm_init sets it).
static constexpr size_t lds_bytes(int BM, int BN) { return (size_t)(2 * BM + 2 * BN) * LDS_LD * sizeof(half_t); }
template <int BM, int BN, bool FASTK>
static int launch_v1(GemmP p, dim3 grid, hipStream_t st) {
  igemm_kernel<BM, BN, FASTK><<<grid, 256, lds_bytes(BM, BN), st>>>(p);
  return 0;
}
template <int BM, int BN, bool FASTK>
static int init_v1() {
  return (int)hipFuncSetAttribute((const void*)igemm_kernel<BM, BN, FASTK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(BM, BN));
}

// Deterministic split-K combine: fixed slab order, then the common epilogue.
__global__ void __launch_bounds__(256) splitk_reduce_kernel(GemmP p) {
  const int groups_per_row = (p.N + 3) / 4;
  const size_t total = (size_t)p.M * groups_per_row;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    int m = (int)(idx / groups_per_row);
    int nb = (int)(idx - (size_t)m * groups_per_row) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < p.splitk; ++z) {
      const float* src = p.slab + ((size_t)z * p.M + m) * p.N + nb;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (nb + j < p.N) v[j] += src[j];
    }
    epilogue_store4(p, m, nb, v, p.bias);
  }
}

// The same combine for the layouts every layer of the UNet has (N % 4 == 0, plain row-major output, 16-byte aligned bias, 8-byte
// aligned rows): one thread per 4 columns, unconditional 16-byte slab loads unrolled over the slabs (the generic kernel's
// predicated scalar loads each carry their own wait), same summation order -> same bits.
__global__ void __launch_bounds__(256) splitk_reduce_vec_kernel(GemmP p) {
  const int gpr = p.N >> 2;
  const size_t total = (size_t)p.M * gpr;
  const size_t slab_stride = (size_t)p.M * p.N;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(idx / gpr);
    const int nb = (int)(idx - (size_t)m * gpr) * 4;
    const float* src = p.slab + (size_t)m * p.N + nb;
    floatx4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int z = 0; z < p.splitk; ++z) v += *reinterpret_cast<const floatx4*>(src + (size_t)z * slab_stride);
    v *= p.alpha;
    if (p.bias) v += *reinterpret_cast<const floatx4*>(p.bias + nb);
    if (p.res) {
      const half4 r4 = *reinterpret_cast<const half4*>(p.res + (size_t)m * p.ldres + nb);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += (float)r4[j];
    }
    half4 h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
    *reinterpret_cast<half4*>(p.out + (size_t)m * p.ldo + nb) = h;
  }
}

void gemm_defaults(GemmP& p) {
  p.x1 = nullptr; p.x2 = nullptr; p.C1 = 0; p.C2 = 0; p.ldx1 = 0; p.ldx2 = 0;
  p.B = 1; p.H = 1; p.W = 1; p.Ho = 1; p.Wo = 1; p.ksize = 1; p.stride = 1; p.pad = 0; p.ups = 0;
  p.w = nullptr; p.ldw = 0; p.M = 0; p.N = 0; p.K = 0; p.bias = nullptr; p.res = nullptr; p.ldres = 0; p.alpha = 1.f;
  p.out = nullptr; p.ldo = 0; p.outT = nullptr; p.vt_col0 = 1 << 30; p.vt_ld = 0; p.vt_f32 = 0; p.rows_per_batch = 1; p.vt_perm16 = 0;
  p.slab = nullptr; p.splitk = 1; p.kchunks_per_split = 0; p.geglu = 0; p.epi_lds = 0; p.stats = nullptr; p.res_late = 0; p.bias_init = 0;
  p.k_order = 0; p.nbatch = 1; p.sx1 = 0; p.sw = 0; p.sout = 0; p.soutT = 0;
}

static constexpr size_t ZERO_PAGE_BYTES = 128 << 10;   // >= 2 * (longest K + one chunk): out-of-range rows walk it like real rows
static thread_local int g_last_cfg = -1, g_last_split = 1;   // per thread: two contexts may launch from two threads   // what the most recent launch_igemm used (profiling dumps)
void igemm_last_launch(int* cfg, int* split, int* geom) { *cfg = g_last_cfg; *split = g_last_split; for (int i = 0; i < 7; ++i) geom[i] = g_last_geom[i]; }

// product tile configurations with one k-group: compiler-scheduled main loop, or (tuning "igemm_sched", in a `build --ablations` library:
// tools/pp_ablate.py, tools/profile_pp.sh) the hand-scheduled ones
#ifdef PNPI_ABLATIONS
static constexpr bool kAblations = true;
#else
static constexpr bool kAblations = false;
#endif
template <int BM, int BN, int BKT, int NST>
static int launch_dma_s(GemmP p, dim3 grid, hipStream_t st) {
#ifdef PNPI_ABLATIONS      // in place of the row's instance: the launch record shows the ABL that ran
  if (g_sched == 1) { g_last_geom[5] = 4; return launch_dma<BM, BN, BKT, NST, 2, 4>(p, grid, st); }
  if (g_sched == 2) { g_last_geom[5] = 5; return launch_dma<BM, BN, BKT, NST, 2, 5>(p, grid, st); }
#endif
  return launch_dma<BM, BN, BKT, NST>(p, grid, st);
}

// ------------------------------------------------------------------------------------------------------------------
// Kernel instances: one row per instance a build can launch.  igemm_plan names the row (kInstRules), launch_igemm calls its launch
// function and records its geom (igemm_last_launch), pnpi_igemm_instance_info hands the table to the tests.
//   name    "dma<BM,BN,BKT,NST[,wgmW][,kgK]>" (WGM = 2 and one k-group are left out), "pp<BM,BN>", "v1<BM,BN,fast|generic>"; an ablation
//           instance adds ",ablA", A the kernel's ABL argument: "dma<128,128,32,3,abl1>", "pp<256,256,abl3>"
//   geom    igemm_dma_kernel's <BM, BN, BKT, NST, WGM, ABL, WK>; igemm_pp_kernel's <BM, BN, MI0, NI0, ABL>, 0, -1; the v1 kernel: all 0
//   launch  launch_dma_s: the instance, or under tuning "igemm_sched" (ablation library) its hand-scheduled form, which has no row
//   init    igemm_init calls it (the v1 kernels' LDS attribute; the other kernels set theirs at their first launch on a device)
// Product rows first; the instances of a `build --ablations` library in one block at the end.
// ------------------------------------------------------------------------------------------------------------------
using LaunchFn = int (*)(GemmP, dim3, hipStream_t);
struct Instance { const char* name; int geom[7]; bool ablation_only; LaunchFn launch; int (*init)(); };
template <int BM, int BN, int BKT, int NST, int WGM = 2, int ABL = 0, int WK = 1>
static constexpr Instance dma_row(const char* name) { return {name, {BM, BN, BKT, NST, WGM, ABL, WK}, ABL != 0, launch_dma<BM, BN, BKT, NST, WGM, ABL, WK>, nullptr}; }
template <int BM, int BN, int BKT, int NST>
static constexpr Instance dma_s_row(const char* name) { return {name, {BM, BN, BKT, NST, 2, 0, 1}, false, launch_dma_s<BM, BN, BKT, NST>, nullptr}; }
template <int BM, int BN, int MI0, int NI0, int ABL = 0>
static constexpr Instance pp_row(const char* name) { return {name, {BM, BN, MI0, NI0, ABL, 0, -1}, ABL != 0, launch_pp<BM, BN, MI0, NI0, ABL>, nullptr}; }
template <int BM, int BN, bool FASTK>
static constexpr Instance v1_row(const char* name) { return {name, {0, 0, 0, 0, 0, 0, 0}, false, launch_v1<BM, BN, FASTK>, init_v1<BM, BN, FASTK>}; }
static constexpr Instance kInstances[] = {
  v1_row<128, 128, true>("v1<128,128,fast>"), v1_row<128, 128, false>("v1<128,128,generic>"),
  v1_row<64, 64, true>("v1<64,64,fast>"), v1_row<64, 64, false>("v1<64,64,generic>"),
  dma_s_row<128, 128, 64, 2>("dma<128,128,64,2>"),
  dma_row<128, 128, 64, 3>("dma<128,128,64,3>"),
  dma_s_row<128, 128, 32, 2>("dma<128,128,32,2>"),
  dma_s_row<128, 128, 32, 3>("dma<128,128,32,3>"),
  dma_row<128, 128, 32, 4>("dma<128,128,32,4>"),
  dma_row<128, 128, 32, 8>("dma<128,128,32,8>"),        // 128 KB ring: sparse launches
  dma_row<64, 64, 64, 2>("dma<64,64,64,2>"),
  dma_s_row<64, 64, 64, 3>("dma<64,64,64,3>"),
  dma_row<64, 64, 64, 4>("dma<64,64,64,4>"),
  dma_row<64, 64, 64, 8>("dma<64,64,64,8>"),            // 128 KB ring: sparse launches
  dma_row<64, 64, 32, 4>("dma<64,64,32,4>"),
  dma_row<256, 128, 32, 2>("dma<256,128,32,2>"),
  dma_row<256, 128, 32, 3>("dma<256,128,32,3>"),
  dma_s_row<128, 320, 32, 2>("dma<128,320,32,2>"),      // 56 KB ring, two-pass epilogue, 2 blocks / CU
  dma_row<128, 320, 32, 3>("dma<128,320,32,3>"),        // 84 KB ring = whole-tile epilogue, 1 block / CU
  dma_row<128, 320, 32, 5>("dma<128,320,32,5>"),
  dma_row<128, 320, 64, 2>("dma<128,320,64,2>"),        // 128-byte rows, 112 KB, 1 block / CU
  dma_s_row<128, 256, 32, 2>("dma<128,256,32,2>"),      // 48 KB: two-pass epilogue, 3 blocks / CU by LDS
  dma_row<128, 256, 32, 3>("dma<128,256,32,3>"),        // 72 KB, 2 blocks / CU
  dma_row<128, 256, 32, 6>("dma<128,256,32,6>"),
  dma_row<128, 256, 64, 2>("dma<128,256,64,2>"),
  dma_row<256, 320, 64, 2, 4>("dma<256,320,64,2,wgm4>"),
  dma_row<256, 256, 64, 2, 4>("dma<256,256,64,2,wgm4>"),
  dma_row<64, 64, 64, 2, 2, 0, 4>("dma<64,64,64,2,kg4>"),
  dma_row<128, 128, 32, 3, 2, 0, 2>("dma<128,128,32,3,kg2>"),
  dma_row<128, 128, 64, 2, 2, 0, 2>("dma<128,128,64,2,kg2>"),
  dma_row<64, 64, 64, 2, 2, 0, 2>("dma<64,64,64,2,kg2>"),
  dma_row<64, 320, 32, 2>("dma<64,320,32,2>"),
  pp_row<256, 256, 2, 4>("pp<256,256>"), pp_row<192, 320, 1, 4>("pp<192,320>"), pp_row<128, 320, 1, 4>("pp<128,320>"), pp_row<192, 256, 1, 4>("pp<192,256>"),
#ifdef PNPI_ABLATIONS
  dma_row<128, 128, 32, 3, 2, 1>("dma<128,128,32,3,abl1>"),      // DMA only
  dma_row<128, 128, 32, 3, 2, 2>("dma<128,128,32,3,abl2>"),      // compute only
  dma_row<128, 128, 32, 3, 2, 3>("dma<128,128,32,3,abl3>"),      // activation loads for tap 0 only
  dma_row<128, 320, 32, 2, 2, 1>("dma<128,320,32,2,abl1>"),      // DMA only
  dma_row<128, 320, 32, 2, 2, 2>("dma<128,320,32,2,abl2>"),      // compute only
  // the tall ping-pong tiles without their MFMAs (1), without their DMA (2), DMA only (3), MFMAs only (4)
  pp_row<256, 256, 2, 4, 1>("pp<256,256,abl1>"), pp_row<256, 256, 2, 4, 2>("pp<256,256,abl2>"), pp_row<256, 256, 2, 4, 3>("pp<256,256,abl3>"), pp_row<256, 256, 2, 4, 4>("pp<256,256,abl4>"),
  pp_row<192, 320, 1, 4, 1>("pp<192,320,abl1>"), pp_row<192, 320, 1, 4, 2>("pp<192,320,abl2>"), pp_row<192, 320, 1, 4, 3>("pp<192,320,abl3>"), pp_row<192, 320, 1, 4, 4>("pp<192,320,abl4>"),
#endif
};
static constexpr int kNumInstances = (int)(sizeof(kInstances) / sizeof(kInstances[0]));
static constexpr bool str_eq(const char* a, const char* b) { for (; *a && *a == *b; ++a, ++b) {} return *a == *b; }
static constexpr int inst(const char* name) {      // the row of that name; -1: none
  for (int i = 0; i < kNumInstances; ++i)
    if (str_eq(kInstances[i].name, name)) return i;
  return -1;
}
int igemm_instance_info(int index, const char** name, int* geom7, int* ablation_only) {
  if (index < 0 || index >= kNumInstances) return -1;
  if (name) *name = kInstances[index].name;
  if (ablation_only) *ablation_only = kInstances[index].ablation_only;
  for (int i = 0; geom7 && i < 7; ++i) geom7[i] = kInstances[index].geom[i];
  return 0;
}

int igemm_init() {
  if (!g_zero_page) {
    HIP_CHECK_RET(hipMalloc((void**)&g_zero_page, ZERO_PAGE_BYTES));
    HIP_CHECK_RET(hipMemset(g_zero_page, 0, ZERO_PAGE_BYTES));
  }
  for (const Instance& in : kInstances)
    if (in.init)
      if (int r = in.init()) return r;
  return 0;
}

// Which instance a plan runs: the first row that matches the tile id, the kernel path (the register-staged kernels by FASTK, or LDS-DMA),
// the tile's knob (kTileDesc; DEF: whatever it holds) and the plan's occupancy class (`sparse`; ANY: whatever).  `reports` is what the
// plan's variant field then shows (KEEP: the knob's value): ids 0 / 1 take their deep rings only from the default variant and report the
// variant that names the same ring directly.  A variant without a row fails the plan (-10): the ping-pong tiles have rows for igemm_vpp
// = 0 only, and in an ablation library the tall ones for 1 ... 4 and a default.
enum { DEF = INT_MIN, KEEP = INT_MIN, ANY = -1 };
enum InstPath { V1_FAST, V1_GENERIC, DMA };
struct InstRule { int id; InstPath path; int variant, sparse, reports, inst; };
static constexpr InstRule kInstRules[] = {
  // id, path, variant, sparse, reports, instance
#ifdef PNPI_ABLATIONS
  {0, DMA, 11, ANY, KEEP, inst("dma<128,128,32,3,abl1>")}, {0, DMA, 12, ANY, KEEP, inst("dma<128,128,32,3,abl2>")}, {0, DMA, 15, ANY, KEEP, inst("dma<128,128,32,3,abl3>")},
  {4, DMA, 11, ANY, KEEP, inst("dma<128,320,32,2,abl1>")}, {4, DMA, 12, ANY, KEEP, inst("dma<128,320,32,2,abl2>")},
  {16, DMA, 1, ANY, KEEP, inst("pp<256,256,abl1>")}, {16, DMA, 2, ANY, KEEP, inst("pp<256,256,abl2>")}, {16, DMA, 3, ANY, KEEP, inst("pp<256,256,abl3>")},
  {16, DMA, 4, ANY, KEEP, inst("pp<256,256,abl4>")}, {16, DMA, DEF, ANY, KEEP, inst("pp<256,256>")},
  {17, DMA, 1, ANY, KEEP, inst("pp<192,320,abl1>")}, {17, DMA, 2, ANY, KEEP, inst("pp<192,320,abl2>")}, {17, DMA, 3, ANY, KEEP, inst("pp<192,320,abl3>")},
  {17, DMA, 4, ANY, KEEP, inst("pp<192,320,abl4>")}, {17, DMA, DEF, ANY, KEEP, inst("pp<192,320>")},
#endif
  {0, V1_FAST, DEF, ANY, KEEP, inst("v1<128,128,fast>")}, {0, V1_GENERIC, DEF, ANY, KEEP, inst("v1<128,128,generic>")},
  {1, V1_FAST, DEF, ANY, KEEP, inst("v1<64,64,fast>")}, {1, V1_GENERIC, DEF, ANY, KEEP, inst("v1<64,64,generic>")},
  // the default variants of ids 0 / 1 by occupancy (igemm_plan: "Ring depth by occupancy")
  {0, DMA, 2, 2, 8, inst("dma<128,128,32,8>")}, {0, DMA, 2, 1, 3, inst("dma<128,128,32,4>")}, {0, DMA, 2, ANY, KEEP, inst("dma<128,128,32,3>")},
  {0, DMA, 1, ANY, KEEP, inst("dma<128,128,64,3>")}, {0, DMA, 3, ANY, KEEP, inst("dma<128,128,32,4>")}, {0, DMA, 4, ANY, KEEP, inst("dma<128,128,32,2>")},
  {0, DMA, 8, ANY, KEEP, inst("dma<128,128,32,8>")}, {0, DMA, DEF, ANY, KEEP, inst("dma<128,128,64,2>")},
  {1, DMA, 0, 2, 8, inst("dma<64,64,64,8>")}, {1, DMA, 0, 1, 2, inst("dma<64,64,64,4>")},
  {1, DMA, 1, ANY, KEEP, inst("dma<64,64,64,2>")}, {1, DMA, 2, ANY, KEEP, inst("dma<64,64,64,4>")}, {1, DMA, 3, ANY, KEEP, inst("dma<64,64,32,4>")},
  {1, DMA, 8, ANY, KEEP, inst("dma<64,64,64,8>")}, {1, DMA, DEF, ANY, KEEP, inst("dma<64,64,64,3>")},
  {3, DMA, 1, ANY, KEEP, inst("dma<256,128,32,2>")}, {3, DMA, DEF, ANY, KEEP, inst("dma<256,128,32,3>")},
  {4, DMA, 1, 2, KEEP, inst("dma<128,320,32,5>")}, {4, DMA, 0, ANY, KEEP, inst("dma<128,320,32,3>")}, {4, DMA, 2, ANY, KEEP, inst("dma<128,320,64,2>")},
  {4, DMA, DEF, ANY, KEEP, inst("dma<128,320,32,2>")},
  {5, DMA, 1, 2, KEEP, inst("dma<128,256,32,6>")}, {5, DMA, 0, ANY, KEEP, inst("dma<128,256,32,3>")}, {5, DMA, 2, ANY, KEEP, inst("dma<128,256,64,2>")},
  {5, DMA, DEF, ANY, KEEP, inst("dma<128,256,32,2>")},
  {6, DMA, DEF, ANY, KEEP, inst("dma<256,320,64,2,wgm4>")}, {7, DMA, DEF, ANY, KEEP, inst("dma<256,256,64,2,wgm4>")},
  {8, DMA, DEF, ANY, KEEP, inst("dma<64,64,64,2,kg4>")}, {9, DMA, DEF, ANY, KEEP, inst("dma<128,128,32,3,kg2>")},
  {10, DMA, DEF, ANY, KEEP, inst("dma<128,128,64,2,kg2>")}, {11, DMA, DEF, ANY, KEEP, inst("dma<64,64,64,2,kg2>")},
  {12, DMA, DEF, ANY, KEEP, inst("dma<64,320,32,2>")}, {13, DMA, DEF, ANY, KEEP, inst("dma<128,128,32,2>")},
  {14, DMA, DEF, ANY, KEEP, inst("dma<128,128,64,2>")}, {15, DMA, DEF, ANY, KEEP, inst("dma<128,256,64,2>")},
  {18, DMA, DEF, ANY, KEEP, inst("dma<128,128,64,3>")},
  {16, DMA, 0, ANY, KEEP, inst("pp<256,256>")}, {17, DMA, 0, ANY, KEEP, inst("pp<192,320>")},
  {19, DMA, 0, ANY, KEEP, inst("pp<128,320>")}, {20, DMA, 0, ANY, KEEP, inst("pp<192,256>")},
};
static constexpr const InstRule* inst_rule(int id, InstPath path, int variant, int sparse) {
  for (const InstRule& r : kInstRules)
    if (r.id == id && r.path == path && (r.variant == DEF || r.variant == variant) && (r.sparse == ANY || r.sparse == sparse)) return &r;
  return nullptr;
}
static_assert(inst_rule(0, DMA, 7, 2)->inst == inst("dma<128,128,64,2>") && inst_rule(0, DMA, 3, 2)->reports == KEEP, "an unnamed variant is the default; deep rings only from the default variant");
static_assert(!inst_rule(19, DMA, 1, 0) && !inst_rule(20, DMA, 4, 2) && (inst_rule(16, DMA, 1, 0) != nullptr) == kAblations && (inst_rule(17, DMA, 7, 0) != nullptr) == kAblations,
              "igemm_vpp: the short ping-pong tiles have no ablation instance, the tall ones in an ablation library only");

// ------------------------------------------------------------------------------------------------------------------
// Tile descriptors: one row per tile id (launch_igemm's force_cfg, the tools' CFG / NAME maps, csrc/tile_table.inc).  Everything the
// launcher needs to know about a tile is a field here: a new tile is a row of this table, its kInstances rows and its kInstRules rows.
// Id 2 is no tile: it is the caller's alias for "id 1 with split-K chosen by the launcher".
//   fam       FAM_V1: 4-wave LDS-DMA kernel that also exists as the register-staged v1 kernel (shapes the DMA kernels cannot take);
//             FAM_DMA: 4-wave LDS-DMA kernel only (WGM x 2 waves per k-group); FAM_PP: the 8-wave ping-pong kernel (igemm_pp.inc)
//   kgroups   K-parallel wave groups (intra-block split-K for launches with at most one tile per CU)
//   wide      left out by tuning "igemm_wide" = 0 (table entries and the cost model)
//   cls       kernel class reported through cfg_used when the launch has no split-K (0 igemm128, 1 igemm64, 9 igemm_wide; split-K: 2)
//   stat_rows rows per GroupNorm statistics partial: the ping-pong kernel writes them per 64-row sub-block, the others per tile
//   alt       ping-pong tiles: the id of the other row height of the same BN (pp_rowtile_pick); -1 otherwise
//   splits    takes split-K;  stats: takes a launch that produces statistics (the 192 x 256 tile cannot reproduce the 256 x 256 tile's
//             statistics tree: 16 row groups over 3 sub-blocks)
//   knob      the tuning knob that holds the tile's variant (kInstRules); nullptr: the tile has one instance
// ------------------------------------------------------------------------------------------------------------------
enum TileFam { FAM_V1, FAM_DMA, FAM_PP };
struct TileDesc { int id, bm, bn; TileFam fam; int kgroups; bool wide; int cls, stat_rows, alt; bool splits, stats; const int* knob; };
static constexpr TileDesc kTileDesc[] = {
  // id, bm, bn, fam, kgroups, wide, cls, stat_rows, alt, splits, stats, knob
  {0, 128, 128, FAM_V1, 1, false, 0, 128, -1, true, true, &g_var128},     // 64-byte rows x 3 stages; deeper rings on sparse launches (igemm_v128)
  {1, 64, 64, FAM_V1, 1, false, 1, 64, -1, true, true, &g_var64},        // (igemm_v64)
  {3, 256, 128, FAM_DMA, 1, false, 0, 256, -1, false, true, &g_var256},   // ablation: too few tiles at these sizes
  {4, 128, 320, FAM_DMA, 1, true, 9, 128, -1, true, true, &g_var320},     // (igemm_v320)
  {5, 128, 256, FAM_DMA, 1, true, 9, 128, -1, true, true, &g_var256n},     // (igemm_v256n)
  {6, 256, 320, FAM_DMA, 1, true, 9, 256, -1, true, true, nullptr},     // 6 / 7: 8 waves, 128-byte rows, two stages, one block per CU
  {7, 256, 256, FAM_DMA, 1, true, 9, 256, -1, true, true, nullptr},
  {8, 64, 64, FAM_DMA, 4, true, 1, 64, -1, true, true, nullptr},        // 16 waves: 4 k-groups
  {9, 128, 128, FAM_DMA, 2, true, 0, 128, -1, true, true, nullptr},     // 8 waves: 2 k-groups, 96 KB
  {10, 128, 128, FAM_DMA, 2, true, 0, 128, -1, true, true, nullptr},    // 8 waves: 2 k-groups, 128-byte rows, 128 KB
  {11, 64, 64, FAM_DMA, 2, true, 1, 64, -1, true, true, nullptr},       // 8 waves: 2 k-groups, 64 KB (2 blocks / CU)
  {12, 64, 320, FAM_DMA, 1, true, 9, 64, -1, true, true, nullptr},      // 768 tiles on the 12-row 64 x 64 level = 3 per CU
  {13, 128, 128, FAM_DMA, 1, false, 0, 128, -1, true, true, nullptr},   // 32 KB two-stage ring (two-pass epilogue): 4 blocks / CU for the short-K layers
  {14, 128, 128, FAM_DMA, 1, false, 0, 128, -1, true, true, nullptr},   // 128-byte rows, half the barriers per k: 64 KB, 2 blocks / CU
  {15, 128, 256, FAM_DMA, 1, true, 9, 128, -1, true, true, nullptr},    // the same for the 128 x 256 tile: 96 KB, 1 block / CU
  {16, 256, 256, FAM_PP, 1, true, 9, 64, 20, true, true, &g_varpp},
  {17, 192, 320, FAM_PP, 1, true, 9, 64, 19, true, true, &g_varpp},
  {18, 128, 128, FAM_DMA, 1, false, 0, 128, -1, true, true, nullptr},   // 128-byte rows, three stages (96 KB, 1 block / CU): the one-wave launches of the 16 x 16 level
  {19, 128, 320, FAM_PP, 1, true, 9, 64, 17, true, true, &g_varpp},      // 19 / 20: the shorter ping-pong tiles: force_cfg or pp_rowtile_pick, never the table
  {20, 192, 256, FAM_PP, 1, true, 9, 64, 16, true, false, &g_varpp},
};
static constexpr const TileDesc* tile_desc(int id) {      // nullptr: no such tile (id 2 included)
  return (id < 0 || id == 2 || id > 20) ? nullptr : &kTileDesc[id < 2 ? id : id - 1];
}
// the one-k-group tile of the same shape class that every launch can fall back to (it also exists as a v1 kernel)
static const TileDesc* plain_twin(const TileDesc* d) { return tile_desc(d->bm == 64 && d->bn == 64 ? 1 : 0); }

// Cost-model constants of the tiles the model chooses among.  rate: FLOP/s of the whole chip with every CU full; t_fix: per-tile
// prologue + epilogue seconds; bpc: co-resident blocks per CU
struct TileCost { int id; double rate, t_fix; int bpc; };
static const TileCost kTiles[] = {
  {0, 868e12, 1.22e-6, 3},
  {1, 572e12, 0.25e-6, 4},
  {4, 1228e12, 5.15e-6, 2},
  {5, 1178e12, 3.61e-6, 2},
};
// Measured choices for the SD-1.x layer shapes at the row counts of the benchmarked schedule (1-row inversion, 12-row lock step):
// per-shape best of every tile / split-K / k-group configuration (tools/autotune2.py -> tools/gen_tile_table.py).  The cost model
// below covers every other shape (other row counts, other model widths).
struct TileEntry { int M, N, K, ks, cfg, split; };
static constexpr TileEntry kTileTable[] = {
#include "tile_table.inc"
};
static constexpr bool tile_tables_consistent() {      // every id finds its own row; every table entry names a tile
  for (const TileDesc& d : kTileDesc)
    if (tile_desc(d.id) != &d) return false;
  for (const TileEntry& e : kTileTable)
    if (!tile_desc(e.cfg)) return false;
  return sizeof(kTileDesc) / sizeof(kTileDesc[0]) == 20;
}
static_assert(tile_tables_consistent(), "kTileDesc rows out of place, or tile_table.inc names an id without a row");
// every rule names a tile and an instance; every instance has a rule; every tile has an instance at every occupancy whatever its knob
// holds (a ping-pong tile: at igemm_vpp = 0), and a FAM_V1 tile both register-staged ones
static constexpr bool inst_tables_consistent() {
  bool used[kNumInstances] = {};
  for (const InstRule& r : kInstRules) {
    if (!tile_desc(r.id) || r.inst < 0) return false;
    used[r.inst] = true;
  }
  for (bool u : used)
    if (!u) return false;
  for (const TileDesc& d : kTileDesc) {
    for (int sparse = 0; sparse <= 2; ++sparse)
      if (!inst_rule(d.id, DMA, d.fam == FAM_PP ? 0 : DEF, sparse)) return false;
    if (d.fam == FAM_V1 && !(inst_rule(d.id, V1_FAST, DEF, 0) && inst_rule(d.id, V1_GENERIC, DEF, 0))) return false;
  }
  return true;
}
static_assert(inst_tables_consistent(), "kInstRules names no tile or no kInstances row, a row has no rule, or a tile has no default rule");
// Table lookup: the exact {M, N, K, ksize}; else -- the same layer (N, K, ksize) at another row count, e.g. --batch_size 2 ... 7 of the
// sweep driver -- the entry whose M is nearest in ratio, up to 4x away.  Held out of the table one row count at a time, the nearest
// entry's configuration costs 13.3 / 10.1 / 6.7 / 5.2 ms per 12- / 8- / 4- / 3-row forward against 15.3 / 10.4 / 6.9 / 6.1 ms for the
// cost model's pick (per-shape best 12.5 / 9.4 / 6.0 / 5.1; profiles/round2_fwd_tune_b*.json).  how: 1 exact, 2 nearest, 0 none.
static const TileEntry* tile_table_lookup(int M, int N, int K, int ks, int* how) {
  const TileEntry* near = nullptr;
  double near_ratio = 4.0 + 1e-9;
  for (const TileEntry& e : kTileTable) {
    if (e.N != N || e.K != K || e.ks != ks) continue;
    if (e.M == M) { if (how) *how = 1; return &e; }
    const double r = e.M > M ? (double)e.M / M : (double)M / e.M;
    if (r < near_ratio) { near_ratio = r; near = &e; }      // ties: the first (smaller M) entry of the sorted table
  }
  if (!g_table_near) near = nullptr;
  if (how) *how = near ? 2 : 0;
  return near;
}
int igemm_table_lookup(int M, int N, int K, int ks, int* cfg, int* split, int* entry_m) {
  int how = 0;
  const TileEntry* e = (M > 0 && N > 0 && K > 0) ? tile_table_lookup(M, N, K, ks, &how) : nullptr;
  if (e) { if (cfg) *cfg = e->cfg; if (split) *split = e->split; if (entry_m) *entry_m = e->M; }
  return how;
}

// Row height of a ping-pong launch (tuning "pp_rowtile").  Tile and split-K are chosen first, as ever (table entry at sel_M); this
// only swaps the tile for the other row height of the same BN (17 <-> 19: 192 / 128 x 320; 16 <-> 20: 256 / 192 x 256), which changes no
// output bit (igemm_pp.inc), using the LAUNCHED M.  W(bm) = ceil(M / bm) * ceil(N / BN) * split workgroups run in ceil(W / 256) rounds
// of one workgroup per CU.  The shorter tile runs when it needs no more rounds than the taller one: each round is then shorter and
// more CUs take part.  (49152, 320) stays 192 (256 tiles, one round, against two); (32768, 320) becomes 128 (171 tiles on two thirds
// of the chip -> 256); (2048, 1280) x 4 becomes 192 x 256 (160 -> 220 workgroups).  Not "the smaller rounds x bm": a round of the
// 128-row tile was measured at 0.91 of a 192-row round, not 0.67 (the weight panel's bytes and the prologue / epilogue do not shrink
// with BM), so four rounds of 128 lose to three of 192 -- (8192, 5120): 688 workgroups 77.7 us against 1024 workgroups 83.6 us
// (profiles/pp_rowtile_ab.json).  Returns the tile to launch.
static bool pp_is_tall(const TileDesc* d) { return d->bm > tile_desc(d->alt)->bm; }
static const TileDesc* pp_rowtile_pick(const TileDesc* d, int M, int N, int split) {
  const TileDesc* tall = pp_is_tall(d) ? d : tile_desc(d->alt);
  const TileDesc* shrt = tile_desc(tall->alt);
  auto rounds = [&](int bm) { const long w = (long)((M + bm - 1) / bm) * ((N + tall->bn - 1) / tall->bn) * (split > 1 ? split : 1); return (w + 255) / 256; };
  return rounds(shrt->bm) > rounds(tall->bm) ? tall : shrt;
}
// host-only query (tests): rows of the tile pp_rowtile_pick launches for a ping-pong configuration; 0: cfg is no ping-pong tile
int igemm_pp_rowtile_query(int cfg, int M, int N, int split) {
  const TileDesc* d = tile_desc(cfg);
  if (!d || d->fam != FAM_PP || M <= 0 || N <= 0) return 0;
  return pp_rowtile_pick(d, M, N, split)->bm;
}

// Which epilogue a launch on tiles BN wide takes.  vt_lds: the transposed (V^T) columns go through the LDS epilogue too -- whole tiles
// are either plain or transposed and 8-token runs stay inside one batch item.  epi_lds: the coalesced LDS-staged epilogue with 16-byte
// row stores applies (never under split-K: the kernel writes slabs).  pp_ok: the ping-pong kernel, which has no scalar epilogue, can
// take the launch: slabs, or the LDS epilogue with a 16-byte aligned bias and whole 16-token groups under vt_perm16.
struct EpiSel { bool vt_none, vt_lds, epi_lds, pp_ok; };
static EpiSel epi_select(const GemmP& p, int bn, int split, bool dma_ok) {
  EpiSel e;
  e.vt_none = p.vt_col0 >= p.N;
  e.vt_lds = !e.vt_none && dma_ok && p.outT && !p.vt_f32 && p.vt_col0 % bn == 0 && p.rows_per_batch % 8 == 0 && p.vt_ld % 8 == 0 &&
             p.M % 8 == 0 && !p.res && !p.geglu && g_vt_lds;
  const bool rows16 = (e.vt_none || e.vt_lds) && (p.N % 8 == 0) && (p.vt_col0 == 0 || p.ldo % 8 == 0) && (!p.res || p.ldres % 8 == 0);
  e.epi_lds = rows16 && split == 1;
  e.pp_ok = split > 1 || (rows16 && (!p.bias || ((uintptr_t)p.bias & 15) == 0) && (!p.vt_perm16 || p.rows_per_batch % 16 == 0));
  return e;
}
// Can the ping-pong tile d take this launch?  Beyond its epilogue (epi_select): its DMA addresses are 32-bit byte offsets under a 2 GiB
// buffer descriptor (operands beyond that stay on the 64-bit-pointer kernels); its split-K slabs are written four columns at a time;
// batched launches stay on the 4-wave kernels; d->stats.
static bool pp_eligible(const GemmP& p, const TileDesc* d, int split, bool dma_ok) {
  if (!d->stats && p.stats && split == 1) return false;
  const double lim = 2147483648.0 - 1048576.0;
  const bool off32_ok = 2.0 * p.B * p.H * p.W * (double)(p.ldx1 > p.ldx2 ? p.ldx1 : p.ldx2) < lim && 2.0 * (double)p.N * p.ldw < lim;
  return dma_ok && off32_ok && epi_select(p, d->bn, split, dma_ok).pp_ok && !(split > 1 && p.N % 4 != 0) && p.nbatch <= 1;
}

// Selection as a pure function of the launch description and the tuning globals: no HIP call, no g_last_* state, no operand is
// dereferenced (pointers are looked at for null / alignment only).  Order of decisions: forced tile (caller's force_cfg, else tuning
// "igemm_force_cfg") | measured table at sel_M | cost model; then the fall-backs -- batched launches lose split-K and k-groups, shapes
// the DMA kernels cannot take go to the v1 tiles, split-K is clamped to the workspace, a ping-pong tile the launch is not eligible for
// becomes 128 x 128 -- then the ping-pong row height on the launched M, the epilogue, the grid, the occupancy class and the instance.
IgemmPlan igemm_plan(GemmP p, bool have_ws, size_t ws_bytes, int force_cfg, int force_split, int sel_M) {
  IgemmPlan pl = {};
  pl.id = -1; pl.split = 1; pl.stats_tile_rows = -1; pl.instance = -1;
  auto fail = [&](int err) { pl.err = err; return pl; };
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return fail(-2);
  const int Cin = p.C1 + p.C2;
  if ((Cin & 7) || (p.K & 7) || (p.C1 & 7) || (p.ldw & 7) || (p.ldx1 & 7) || (p.C2 && (p.ldx2 & 7))) return fail(-3);
  if (p.K != p.ksize * p.ksize * Cin) return fail(-4);
  if (p.vt_col0 > p.N) p.vt_col0 = p.N;
  pl.vt_col0 = p.vt_col0;
  const bool fast = (Cin % BK == 0) && (p.C1 % BK == 0);
  const int nchunks = (p.K + BK - 1) / BK;
  const bool dma_ok = fast && g_use_dma && (p.K % BK == 0) && (p.ldw % 8 == 0) && ((size_t)p.K * 2 + 1024 <= ZERO_PAGE_BYTES);
  pl.fastk = fast; pl.dma = dma_ok;
  // sel_M > 0: tile, split-K and ring depth are chosen as for a launch of sel_M rows (the same layer at another row count: the
  // deduplicated UNet prefix pinned to its full-row configuration); the launch itself covers p.M rows
  const int selM = sel_M > 0 ? sel_M : p.M;
  auto tiles_of = [&](int bm, int bn) { return (long)((selM + bm - 1) / bm) * ((p.N + bn - 1) / bn); };
  // the slabs are written for the launched rows: a launch configured as at FEWER rows than it has must still fit them
  const int slabM = selM > p.M ? selM : p.M;
  auto slabs_fit = [&](int s) { return have_ws && (size_t)s * slabM * p.N * sizeof(float) <= ws_bytes; };
  int cfg = force_cfg;
  int split = 1;
  if (cfg < 0 && g_force_cfg >= 0) { cfg = g_force_cfg == 2 ? 1 : g_force_cfg; if (force_split <= 0) force_split = g_force_split; }
  const bool cfg_forced = cfg >= 0;      // a caller's force_cfg or tuning "igemm_force_cfg" names its tile and keeps it
  if (cfg_forced && cfg != 2 && !tile_desc(cfg)) return fail(-2);
  if (cfg < 0 && g_use_table && dma_ok) {
    if (const TileEntry* e = tile_table_lookup(selM, p.N, p.K, p.ksize, nullptr)) {
      const TileDesc* ed = tile_desc(e->cfg);
      const bool pp = ed->fam == FAM_PP;
      const bool split_ok = e->split == 1 || (!p.geglu && slabs_fit(e->split));
      const bool vt_ok = p.vt_col0 >= p.N || p.vt_col0 % ed->bn == 0;
      const bool pp_masked = pp && ((g_pp_only_n > 0 && p.N != g_pp_only_n) || (g_pp_only_k > 0 && p.K != g_pp_only_k) ||
                                    (g_pp_only_m > 0 && selM != g_pp_only_m) || g_pp_only_n < 0);
      // a ping-pong entry (tile and split tuned together) applies only to a launch that kernel can take: otherwise the cost model
      // picks tile AND split for the 4-wave kernels (not the entry's split on a 128 x 128 tile)
      const bool pp_ok = !pp || pp_eligible(p, ed, e->split, dma_ok);
      if (split_ok && vt_ok && !pp_masked && pp_ok && (g_wide || !ed->wide)) { cfg = e->cfg; split = e->split; }
    }
  }
  if (cfg < 0) {
    // Tile / split-K selection by a small cost model (constants fitted to per-shape timings on MI355X, tools/fit_cost_model.py):
    //   time ~ (units on the busiest CU) x (padded FLOPs of one unit) / (per-CU rate of the tile x co-residency factor)
    //          + split-K slab traffic + the reduce launch.
    // Wider tiles move fewer operand bytes per FLOP through the LDS-DMA path (the limiter), but need split-K on the
    // low-resolution layers to put work on all 256 CUs.
    double best = 1e30;
    static const int splits[] = {1, 2, 3, 4, 6, 8, 12, 16};
    for (const TileCost& tc : kTiles) {
      const TileDesc* td = tile_desc(tc.id);
      if (td->wide && !(dma_ok && g_wide)) continue;     // the wide tiles exist only as LDS-DMA kernels
      const long tiles = tiles_of(td->bm, td->bn);
      for (int s : splits) {
        if (s > 1 && (nchunks / s < 4 || !slabs_fit(s))) continue;
        if (s > 1 && p.geglu) continue;
        // constants: tools/fit_cost_model2.py on tools/autotune2.py timings of every configuration per layer shape (rms log error
        // 0.10; the picks cost 1 % more than the per-shape best over a 12-row forward)
        const double unit = tc.t_fix + (double)((nchunks + s - 1) / s) * (2.0 * td->bm * td->bn * BK) / (tc.rate / 256.0);   // padded tiles do real work
        const long units = tiles * s;
        const long on_busiest = (units + 255) / 256;
        const double per_cu = (double)units / 256.0;
        // co-resident blocks cover each other's exposed loads: a lone block on a CU runs below the tile's full rate
        const double fill = per_cu >= tc.bpc ? 1.0 : (per_cu <= 1.0 ? 0.0 : (per_cu - 1.0) / (tc.bpc - 1.0));
        const double resid = 0.82 + 0.18 * fill;
        double t = (double)on_busiest * unit / resid;
        if (s > 1) t += (double)(2 * s + 1) * selM * p.N * 4.0 / 8.14e12 + 4.97e-6;   // slabs written, re-read, output + the reduce launch
        if (p.vt_col0 < p.N && p.vt_col0 % td->bn != 0) t *= 1.3;   // transposed columns not tile-aligned: scalar epilogue
        if (t < best) { best = t; cfg = tc.id; split = s; }
      }
    }
  } else if (cfg == 2) {
    const long t64 = tiles_of(64, 64);
    cfg = 1;
    split = force_split > 0 ? force_split : (int)((512 + t64 - 1) / t64);
    if (split > 16) split = 16;
    if (split > nchunks) split = nchunks;
    while (split > 1 && nchunks / split < 4) --split;
  } else if (force_split > 1) {
    split = force_split;
  }
  const TileDesc* d = tile_desc(cfg);
  if (p.nbatch > 1) { split = 1; if (d->kgroups > 1) d = plain_twin(d); }   // no split-K / k-groups across problems
  if (!dma_ok && d->fam != FAM_V1) d = plain_twin(d);                      // every other tile exists only as an LDS-DMA kernel
  // whatever chose the split (cost model or a caller-forced value): the slabs must fit the workspace and each split needs work
  if (split > 1) {
    if (split > nchunks) split = nchunks;
    if (!slabs_fit(split) || p.geglu || !d->splits) split = 1;
  }
  if (d->fam == FAM_PP && !pp_eligible(p, d, split, dma_ok)) d = tile_desc(0);     // forced configurations (tests, sweeps): the 128 x 128 kernel instead
  // the row height follows the launched M
  if (d->fam == FAM_PP && g_pp_rowtile && !cfg_forced && !g_varpp) {      // forced tiles keep theirs; the ablation instances (igemm_vpp) exist for the tall tiles only
    const TileDesc* o = pp_rowtile_pick(d, p.M, p.N, split);
    if (o != d && pp_eligible(p, o, split, dma_ok)) d = o;
  }
  const bool cpp = d->fam == FAM_PP;
  pl.id = d->id; pl.split = split; pl.bm = d->bm; pl.bn = d->bn;
  pl.cls = split > 1 ? 2 : d->cls;
  pl.kchunks_per_split = (nchunks + split - 1) / split;
  const EpiSel epi = epi_select(p, d->bn, split, dma_ok);
  pl.epi_lds = epi.epi_lds;
  pl.res_late = g_res_late;
  pl.bias_init = (dma_ok && split == 1 && p.bias && p.alpha == 1.f && p.N % 4 == 0 && ((uintptr_t)p.bias & 15) == 0 && g_bias_init && !cpp) ? 1 : 0;
  pl.k_order = cpp ? ((g_tapin && p.ksize == 3) ? 1 : 0) : p.k_order;
  if (p.vt_perm16 && (p.rows_per_batch % 16 != 0 || p.vt_f32)) return fail(-9);   // permuted V^T: whole 16-token groups, fp16
  if (p.geglu && !(pl.epi_lds && dma_ok && p.N % 64 == 0)) return fail(-7);   // GEGLU exists only in the LDS epilogue
  // statistics come only from the DMA kernels' LDS epilogue, and not from a launch whose V^T columns take it
  pl.stats = p.stats && !epi.vt_lds && pl.epi_lds && dma_ok && !p.geglu;
  pl.stats_tile_rows = pl.stats ? d->stat_rows : 0;
  if (p.nbatch > 1 && (split != 1 || p.bias || p.res || pl.stats || p.geglu || p.x2)) return fail(-8);     // batched launches: plain products only
  pl.gx = (p.M + d->bm - 1) / d->bm; pl.gy = (p.N + d->bn - 1) / d->bn; pl.gz = p.nbatch > 1 ? p.nbatch : split;
  // Ring depth by occupancy: with at most one block per CU nothing else covers the HBM latency of the weight stream (cold in a
  // forward: 1.7 GB of weights pass through per UNet call), and the whole 160 KB of LDS is free -- so sparse launches take an
  // 8-deep ring (7 chunks in flight per block); two blocks per CU a 4-deep one; fuller launches the shallow rings that fit 3 blocks.
  const long units = (long)((selM + d->bm - 1) / d->bm) * pl.gy * pl.gz;
  pl.sparse = !g_deep_rings ? 0 : (units <= 256 ? 2 : (units <= 512 ? 1 : 0));
  // The instance (kInstRules): by the tile's knob and the occupancy class.  A variant without a row: -10
  int variant = dma_ok && d->knob ? *d->knob : 0;
  // 128-byte rows with 2 stages (64 KB, 2 blocks / CU) beat 64-byte rows with 3 stages (48 KB, 3 blocks / CU) once every CU
  // holds two blocks that cover for each other's exposed loads; below that the deeper ring wins
  if (d->id == 0 && g_v128_bk64_tiles > 0 && variant == 2 && units >= g_v128_bk64_tiles) variant = 0;
  const InstRule* r = inst_rule(d->id, dma_ok ? DMA : (fast ? V1_FAST : V1_GENERIC), variant, pl.sparse);
  if (!r) return fail(-10);
  pl.variant = r->reports == KEEP ? variant : r->reports;
  pl.instance = r->inst;
  return pl;
}

int launch_igemm(GemmP p, float* ws, size_t ws_bytes, hipStream_t st, int force_cfg, int force_split, int* cfg_used,
                 int* stats_tile_rows, int sel_M) {
  const IgemmPlan pl = igemm_plan(p, ws != nullptr, ws_bytes, force_cfg, force_split, sel_M);
  if (pl.id < 0) return pl.err;      // rejected before a tile was chosen
  if (cfg_used) *cfg_used = pl.cls;
  g_last_cfg = pl.id; g_last_split = pl.split;
  for (int i = 0; i < 7; ++i) g_last_geom[i] = pl.instance < 0 ? 0 : kInstances[pl.instance].geom[i];
  if (stats_tile_rows && pl.stats_tile_rows >= 0) *stats_tile_rows = pl.stats_tile_rows;
  if (pl.err) return pl.err;
  p.vt_col0 = pl.vt_col0; p.splitk = pl.split; p.kchunks_per_split = pl.kchunks_per_split; p.slab = ws;
  p.epi_lds = pl.epi_lds; p.bias_init = pl.bias_init; p.res_late = pl.res_late; p.k_order = pl.k_order;
  if (!pl.stats) p.stats = nullptr;
  if (int r = kInstances[pl.instance].launch(p, dim3(pl.gx, pl.gy, pl.gz), st)) return r;
  if (pl.split > 1) {
    size_t total = (size_t)p.M * ((p.N + 3) / 4);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    const bool vec = p.N % 4 == 0 && p.vt_col0 >= p.N && p.ldo % 4 == 0 && (!p.res || p.ldres % 4 == 0) && (!p.bias || ((uintptr_t)p.bias & 15) == 0) &&
                     ((uintptr_t)p.out & 7) == 0 && (!p.res || ((uintptr_t)p.res & 7) == 0) && ((uintptr_t)ws & 15) == 0;
    if (vec) splitk_reduce_vec_kernel<<<blocks, 256, 0, st>>>(p);
    else splitk_reduce_kernel<<<blocks, 256, 0, st>>>(p);
  }
  return (int)hipGetLastError();
}
