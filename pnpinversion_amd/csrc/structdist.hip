// DINO structure distance kernels for gfx950 (evaluation/matrics_calculator.py:385-405 -> :237-246 -> :154-171): the tensor Resize +
// ImageNet Normalize on 0..255 values written straight into the patch rows of the patch-embedding GEMM, token assembly with the
// convolution's bias, the exact GELU of DINO's MLP, and the metric's own arithmetic: the mean squared difference of the two key
// self-similarity maps, formed tile by tile on the matrix pipe and reduced in a fixed order without either map reaching memory.
#include "ops.h"

// ---------------------------------------------------------------------------------------------------------------
// torchvision 0.13 Resize on a tensor = torch.nn.functional.interpolate(mode="bilinear", align_corners=False), no antialiasing: two taps
// per axis.  The taps (idx0, idx1, lambda1 per output index: pnpi_dino_resize_taps, PyTorch's fp32 index arithmetic) come from the
// host.  The four products and three sums of one output value are carried in double and rounded to fp32 once: half an ulp from the
// exact value of the fp32-weight formula (evaluated in fp32 with FMAs it can be 3 ulp off -- two roundings in each row's value, scaled
// by a weight near 1 into a result one binade lower, and two more).  Then Normalize((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)) on
// the 0..255 value, as the reference applies it (a white pixel is ~1.1e3), in fp32.
// One workgroup per output row, two horizontally adjacent outputs of one channel per thread (4-byte patch-row stores).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dino_normalise(float v, int c) {
  const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
  const float sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
  return (v - mean) / sd;
}

__global__ void __launch_bounds__(256) dino_preprocess_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, int S, int out,
                                                              const int* __restrict__ idx0, const int* __restrict__ idx1,
                                                              const float* __restrict__ lam, int patch, float* __restrict__ resized,
                                                              half_t* __restrict__ patches) {
  const int oy = blockIdx.x, b = blockIdx.y;
  const int y0 = idx0[oy], y1 = idx1[oy];
  const double wy1 = (double)lam[oy], wy0 = (double)(1.0f - lam[oy]);      // lambda0 = 1 - lambda1 in fp32, as PyTorch forms it
  const uint8_t* r0 = img + ((size_t)b * S + y0) * S * 3;
  const uint8_t* r1 = img + ((size_t)b * S + y1) * S * 3;
  const uint8_t* m0 = mask ? mask + ((size_t)b * S + y0) * S : nullptr;
  const uint8_t* m1 = mask ? mask + ((size_t)b * S + y1) * S : nullptr;
  const int half_out = out >> 1, G = out / patch, pp = patch * patch, K = 3 * pp;
  const int py = oy / patch, ky = oy - py * patch;
  for (int it = threadIdx.x; it < 3 * half_out; it += 256) {
    const int c = it / half_out, ox = 2 * (it - c * half_out);
    float v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int x0 = idx0[ox + j], x1 = idx1[ox + j];
      const double wx1 = (double)lam[ox + j], wx0 = (double)(1.0f - lam[ox + j]);
      // img * mask: a cleared source pixel is 0 in every channel
      const double p00 = (m0 && m0[x0] == 0) ? 0.0 : (double)r0[x0 * 3 + c], p01 = (m0 && m0[x1] == 0) ? 0.0 : (double)r0[x1 * 3 + c];
      const double p10 = (m1 && m1[x0] == 0) ? 0.0 : (double)r1[x0 * 3 + c], p11 = (m1 && m1[x1] == 0) ? 0.0 : (double)r1[x1 * 3 + c];
      v[j] = (float)(wy0 * (wx0 * p00 + wx1 * p01) + wy1 * (wx0 * p10 + wx1 * p11));
    }
    if (resized) {
      float* dst = resized + (((size_t)b * 3 + c) * out + oy) * out + ox;
      dst[0] = v[0]; dst[1] = v[1];
    }
    if (patches) {
      const int px = ox / patch, kx = ox - px * patch;      // ox and patch are even: both outputs lie in one patch, at an even column
      const half2v h = {(half_t)dino_normalise(v[0], c), (half_t)dino_normalise(v[1], c)};
      *reinterpret_cast<half2v*>(patches + ((size_t)b * G * G + (size_t)py * G + px) * K + c * pp + ky * patch + kx) = h;
    }
  }
}

int launch_dino_preprocess(const uint8_t* img, const uint8_t* mask, int n, int S, int out, const int* idx0, const int* idx1, const float* lam,
                           int patch, float* resized, half_t* patches, hipStream_t st) {
  if (!img || !idx0 || !idx1 || !lam || n <= 0 || S <= 0 || out <= 0 || (!resized && !patches)) return -3;
  if (patch <= 0 || (patch & 1) || out % patch || n > 65535) return -3;
  dino_preprocess_kernel<<<dim3(out, n), 256, 0, st>>>(img, mask, S, out, idx0, idx1, lam, patch, resized, patches);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// torch.nn.GELU() (erf form) in place, eight values per thread (n % 8 == 0: rows of a multiple-of-8 width)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gelu_erf_kernel(half_t* __restrict__ x, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    half8 h = *reinterpret_cast<const half8*>(x + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (half_t)gelu_f((float)h[j]);
    *reinterpret_cast<half8*>(x + i * 8) = h;
  }
}
int launch_gelu_erf(half_t* x, size_t n, hipStream_t st) {
  if (!x || n == 0 || (n & 7) || ((uintptr_t)x & 15)) return -3;
  const size_t n8 = n >> 3;
  int blocks = (int)((n8 + 255) / 256); if (blocks > 4096) blocks = 4096;
  gelu_erf_kernel<<<blocks, 256, 0, st>>>(x, n8);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Key self-similarity distance (VitExtractor.attn_cosine_sim + F.mse_loss):
//   sim[i][j] = (x_i . x_j) / max(|x_i| |x_j|, 1e-8),   distance = mean over the T^2 entries of (sim_a - sim_b)^2.
// 1. row norms of every key matrix in fp32, one wavefront per row.
// 2. one workgroup per 64 x 64 tile of the T x T index space and pair: the tile's i rows and j rows of both matrices go through LDS in
//    chunks of 64 columns (the next chunk's global loads are in flight while the matrix pipe works on this one), each of the four
//    waves forms its 32 x 32 block of Ka Ka^T and of Kb Kb^T with v_mfma_f32_32x32x16_f16 -- the same (i, j) of both maps in the same
//    accumulator slot of the same lane -- divides by the clamped norm products, squares the difference and reduces: wave shuffle, then
//    the four wave sums in a fixed order, one partial per workgroup.  Rows and columns beyond T are left out by predicate.
// 3. one workgroup per pair sums the partials in a fixed order and divides by T^2.  No atomics: the same inputs give the same bits.
// MAP = true is the same tile body on one matrix, writing its map in fp32 (kernel tests, and the unfused composition tools/time_structure_distance.py times).
// LDS rows are 64 + 8 halves (144 B): the 16 lanes of a ds_read_b128 group read 16 different rows at one column, 9 r mod 16 puts them
// on the 16 different 16-byte slots of the bank row.
// ---------------------------------------------------------------------------------------------------------------
static constexpr int SS_TILE = 64, SS_KC = 64, SS_LD = SS_KC + 8;

__global__ void __launch_bounds__(256) key_norms_kernel(const half_t* __restrict__ ka, const half_t* __restrict__ kb, size_t rows, int D,
                                                        float* __restrict__ norms) {
  const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // rows of ka, then rows of kb
  const int lane = threadIdx.x & 63;
  const size_t total = kb ? 2 * rows : rows;
  if (r >= total) return;
  const half_t* p = r < rows ? ka + r * D : kb + (r - rows) * D;
  float s = 0.f;
  for (int c = lane * 8; c < D; c += 64 * 8) {
    const half8 h = ldg_half8(p + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) s = __builtin_fmaf((float)h[j], (float)h[j], s);
  }
  s = wave_sum(s);
  if (lane == 0) norms[r] = sqrtf(s);
}

template <bool MAP>
__global__ void __launch_bounds__(256) selfsim_tile_kernel(const half_t* __restrict__ ka, const half_t* __restrict__ kb, int T, int D,
                                                           const float* __restrict__ norms_a, const float* __restrict__ norms_b,
                                                           float* __restrict__ partial, float* __restrict__ map) {
  constexpr int NM = MAP ? 1 : 2;                                 // matrices in flight
  __shared__ __attribute__((aligned(16))) half_t s_k[NM * 2][SS_TILE][SS_LD];      // [matrix][i rows | j rows]
  __shared__ float s_n[NM * 2][SS_TILE];
  __shared__ float s_red[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j0 = blockIdx.x * SS_TILE, i0 = blockIdx.y * SS_TILE, pair = blockIdx.z;
  const half_t* base[2] = {ka + (size_t)pair * T * D, MAP ? nullptr : kb + (size_t)pair * T * D};
  if (tid < NM * 2 * SS_TILE) {
    const int reg = tid >> 6, r = tid & 63, g = ((reg & 1) ? j0 : i0) + r;
    const float* nr = (reg >> 1) ? norms_b : norms_a;
    s_n[reg][r] = g < T ? nr[(size_t)pair * T + g] : 0.f;
  }
  // global -> registers: region reg = 2 * matrix + (0: i rows, 1: j rows), 64 rows x 8 sixteen-byte segments, two per thread
  half8 stage[NM * 2][2];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int reg = 0; reg < NM * 2; ++reg)
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int idx = tid + it * 256, r = idx >> 3, col = k0 + (idx & 7) * 8;
        const int g = ((reg & 1) ? j0 : i0) + r;
        stage[reg][it] = (g < T && col < D) ? ldg_half8(base[reg >> 1] + (size_t)g * D + col) : zero_half8();
      }
  };
  floatx16 acc[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;          // this wave's 32 x 32 block of the tile
  load_chunk(0);
  for (int k0 = 0; k0 < D; k0 += SS_KC) {
#pragma unroll
    for (int reg = 0; reg < NM * 2; ++reg)
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int idx = tid + it * 256;
        *reinterpret_cast<half8*>(&s_k[reg][idx >> 3][(idx & 7) * 8]) = stage[reg][it];
      }
    __syncthreads();
    if (k0 + SS_KC < D) load_chunk(k0 + SS_KC);
#pragma unroll
    for (int kk = 0; kk < SS_KC; kk += 16) {
      const int kc = kk + (lane >> 5) * 8;
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const half8 fi = *reinterpret_cast<const half8*>(&s_k[2 * m][wr + (lane & 31)][kc]);
        const half8 fj = *reinterpret_cast<const half8*>(&s_k[2 * m + 1][wc + (lane & 31)][kc]);
        acc[m] = mfma32(fi, fj, acc[m]);
      }
    }
    __syncthreads();
  }
  // accumulator slot r of lane l: row wr + acc_row(r, l), column wc + (l & 31)
  const int jl = wc + (lane & 31), j = j0 + jl;
  float local = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int il = wr + acc_row(r, lane), i = i0 + il;
    const float sa = acc[0][r] / fmaxf(s_n[0][il] * s_n[1][jl], 1e-8f);
    if constexpr (MAP) {
      if (i < T && j < T) map[((size_t)pair * T + i) * T + j] = sa;
    } else {
      const float sb = acc[1][r] / fmaxf(s_n[2][il] * s_n[3][jl], 1e-8f);
      const float d = sa - sb;
      if (i < T && j < T) local = __builtin_fmaf(d, d, local);
    }
  }
  if constexpr (!MAP) {
    local = wave_sum(local);
    if (lane == 0) s_red[wave] = local;
    __syncthreads();
    if (tid == 0) partial[((size_t)pair * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  }
}

__global__ void __launch_bounds__(256) selfsim_reduce_kernel(const float* __restrict__ partial, int nblk, int T, float* __restrict__ out) {
  __shared__ float s[256];
  const int pair = blockIdx.x, tid = threadIdx.x;
  float v = 0.f;
  for (int i = tid; i < nblk; i += 256) v += partial[(size_t)pair * nblk + i];
  s[tid] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) s[tid] += s[tid + off];
    __syncthreads();
  }
  if (tid == 0) out[pair] = s[0] / (float)((double)T * (double)T);
}

size_t keys_selfsim_scratch_floats(int n, int T) {
  const size_t nt = (size_t)(T + SS_TILE - 1) / SS_TILE;
  return 2 * (size_t)n * T + (size_t)n * nt * nt;
}

// keys_a / keys_b fp16 [n][T][D]; scratch: keys_selfsim_scratch_floats(n, T) floats; dist (nullable) fp32 [n]; sim_a (nullable) fp32
// [n][T][T] = the map of keys_a
int launch_keys_selfsim_mse(const half_t* keys_a, const half_t* keys_b, int n, int T, int D, float* scratch, float* dist, float* sim_a,
                            hipStream_t st) {
  if (!keys_a || !scratch || n <= 0 || n > 65535 || T <= 0 || D <= 0 || (D & 31) || (!dist && !sim_a) || (dist && !keys_b)) return -3;
  if (((uintptr_t)keys_a | (uintptr_t)keys_b) & 15) return -3;
  const int nt = (T + SS_TILE - 1) / SS_TILE;
  if (nt > 65535) return -3;
  const size_t rows = (size_t)n * T;
  float* norms = scratch;
  float* partial = scratch + 2 * rows;
  const half_t* kb = dist ? keys_b : nullptr;
  const size_t nrows = kb ? 2 * rows : rows;
  key_norms_kernel<<<(unsigned)((nrows + 3) / 4), 256, 0, st>>>(keys_a, kb, rows, D, norms);
  HIP_CHECK_RET(hipGetLastError());
  if (dist) {
    selfsim_tile_kernel<false><<<dim3(nt, nt, n), 256, 0, st>>>(keys_a, keys_b, T, D, norms, norms + rows, partial, nullptr);
    HIP_CHECK_RET(hipGetLastError());
    selfsim_reduce_kernel<<<n, 256, 0, st>>>(partial, nt * nt, T, dist);
    HIP_CHECK_RET(hipGetLastError());
  }
  if (sim_a) {
    selfsim_tile_kernel<true><<<dim3(nt, nt, n), 256, 0, st>>>(keys_a, nullptr, T, D, norms, nullptr, nullptr, sim_a);
    HIP_CHECK_RET(hipGetLastError());
  }
  return 0;
}
