// LPIPS (SqueezeNet) kernels for gfx950 (evaluation/matrics_calculator.py:324-342 -> torchmetrics >= 1.0
// LearnedPerceptualImagePatchSimilarity(net_type = "squeeze")): the metric's preprocessing fused into the first convolution, the
// ceil-mode max pool and the in-place ReLU of torchvision's squeezenet1_1().features, and the metric's own arithmetic: per tap the
// channel-normalised difference, weighted, squared and averaged over the pixels in a fixed order, without a normalised map reaching
// memory.  The Fire convolutions are implicit GEMMs (gemm.hip).  No atomics anywhere: the same inputs give the same bits.
#include "ops.h"

// ---------------------------------------------------------------------------------------------------------------
// features.0 + features.1 with the input transform in front: u8 [n][S][S][3] (* mask [n][S][S] 0 / 1) -> ((u8 / 255) * mask) * 2 - 1
// (a cleared pixel is -1, not 0) -> ScalingLayer (x - shift_c) / scale_c -> Conv2d(3, 64, 3, stride 2, no padding) -> ReLU -> fp16 NHWC
// [n][Ho][Ho][64], Ho = (S - 3) / 2 + 1.  K = 27: no matrix pipe, no padded image buffer.  The transform of one input value is carried
// in double and rounded to fp32 once (half an ulp from the exact value).  There are only 3 x 256 distinct ones -- a cleared pixel is the
// value of u8 = 0 -- so every workgroup forms them once into an LDS table, three per thread; the 27 products are accumulated by FMAs
// on the bias in (ky, kx, c) order.  256 threads = 32 output pixels x 8 groups of 8 output channels: one 16-byte
// store per thread, 128 contiguous bytes per pixel.  The weights [64][27] fp16 sit in LDS as fp32 [27][64].
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lpips_input(int u8, int c) {
  const double shift = c == 0 ? -0.030 : (c == 1 ? -0.088 : -0.188);
  const double scale = c == 0 ? 0.458 : (c == 1 ? 0.448 : 0.450);
  return (float)(((double)u8 / 255.0 * 2.0 - 1.0 - shift) / scale);
}

__global__ void __launch_bounds__(256) lpips_conv1_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, int S, int Ho,
                                                          const half_t* __restrict__ w, const float* __restrict__ bias,
                                                          half_t* __restrict__ out) {
  __shared__ float s_w[27][64];
  __shared__ float s_b[64];
  __shared__ float s_in[3][256];
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int i = tid; i < 3 * 256; i += 256) s_in[i >> 8][i & 255] = lpips_input(i & 255, i >> 8);
  for (int i = tid; i < 64 * 27; i += 256) s_w[i % 27][i / 27] = (float)w[i];
  if (tid < 64) s_b[tid] = bias[tid];
  __syncthreads();
  const int pix = blockIdx.x * 32 + (tid >> 3), c0 = (tid & 7) * 8;
  if (pix >= Ho * Ho) return;
  const int oy = pix / Ho, ox = pix - oy * Ho;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = s_b[c0 + j];
#pragma unroll 1      // one row of taps at a time: unrolled whole, the 216 weights of a thread are all fetched up front (249 VGPRs)
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const size_t at = ((size_t)b * S + (2 * oy + ky)) * S + (2 * ox + kx);      // 2 (Ho - 1) + 2 <= S - 1
      const int keep = mask ? mask[at] != 0 : 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = s_in[c][keep ? img[at * 3 + c] : 0];
        const float* wr = &s_w[(ky * 3 + kx) * 3 + c][c0];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(wr[j], v, acc[j]);
      }
    }
  half8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (half_t)fmaxf(acc[j], 0.f);
  *reinterpret_cast<half8*>(out + ((size_t)b * Ho * Ho + pix) * 64 + c0) = h;
}

int lpips_conv1_out(int S) { return S < 3 ? 0 : (S - 3) / 2 + 1; }

int launch_lpips_conv1(const uint8_t* img, const uint8_t* mask, int n, int S, const half_t* w, const float* bias, half_t* out, hipStream_t st) {
  if (!img || !w || !bias || !out || n <= 0 || n > 65535 || S < 3 || S > 8192 || ((uintptr_t)out & 15)) return -3;
  const int Ho = lpips_conv1_out(S);
  lpips_conv1_kernel<<<dim3((Ho * Ho + 31) / 32, n), 256, 0, st>>>(img, mask, S, Ho, w, bias, out);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// MaxPool2d(3, stride 2, ceil_mode = True) on fp16 NHWC, 16-byte vectors over the channels.  A window that overhangs the input is
// clipped to it; the last window starts inside the input (PyTorch's pooling_output_shape).  One thread per (output pixel, 8 channels).
// ---------------------------------------------------------------------------------------------------------------
int maxpool3s2_ceil_out(int H) {
  if (H < 2) return 0;                      // PyTorch: "Output size is too small"
  int Ho = (H - 2) / 2 + 1;                 // ceil((H - 3) / 2) + 1
  if ((Ho - 1) * 2 >= H) --Ho;
  return Ho;
}

__global__ void __launch_bounds__(256) maxpool3s2_ceil_kernel(const half_t* __restrict__ x, int H, int Ho, int C8, size_t total,
                                                              half_t* __restrict__ out) {
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cv = (int)(idx % C8);
    size_t r = idx / C8;
    const int ox = (int)(r % Ho); r /= Ho;
    const int oy = (int)(r % Ho);
    const size_t b = r / Ho;
    const int y1 = min(2 * oy + 3, H), x1 = min(2 * ox + 3, H);
    half8 m = ldg_half8(x + ((b * H + 2 * oy) * H + 2 * ox) * C8 * 8 + cv * 8);
    for (int y = 2 * oy; y < y1; ++y)
      for (int xx = 2 * ox; xx < x1; ++xx) {
        const half8 v = ldg_half8(x + ((b * H + y) * H + xx) * C8 * 8 + cv * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = v[j] > m[j] ? v[j] : m[j];
      }
    *reinterpret_cast<half8*>(out + idx * 8) = m;
  }
}

int launch_maxpool3s2_ceil(const half_t* x, int n, int H, int C, half_t* out, hipStream_t st) {
  if (!x || !out || n <= 0 || H < 2 || H > 8192 || C <= 0 || (C & 7) || ((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return -3;
  const int Ho = maxpool3s2_ceil_out(H);
  const size_t total = (size_t)n * Ho * Ho * (C / 8);
  int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  maxpool3s2_ceil_kernel<<<blocks, 256, 0, st>>>(x, H, Ho, C / 8, total, out);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// ReLU in place, eight values per thread (n % 8 == 0): one pass over a Fire block's concat buffer, whose two halves the expand
// convolutions wrote side by side
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) relu_f16_kernel(half_t* __restrict__ x, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    half8 h = *reinterpret_cast<const half8*>(x + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = h[j] > (half_t)0.f ? h[j] : (half_t)0.f;
    *reinterpret_cast<half8*>(x + i * 8) = h;
  }
}
int launch_relu_f16(half_t* x, size_t n, hipStream_t st) {
  if (!x || n == 0 || (n & 7) || ((uintptr_t)x & 15)) return -3;
  const size_t n8 = n >> 3;
  int blocks = (int)((n8 + 255) / 256); if (blocks > 8192) blocks = 8192;
  relu_f16_kernel<<<blocks, 256, 0, st>>>(x, n8);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// One tap of the LPIPS score: a, b fp16 [n][HW][C], w fp32 [C] (the 1 x 1 `lin` layer: no bias, any sign):
//   per pixel  an = sqrt(1e-8 + sum_c a_c^2), bn likewise,  d = sum_c w_c (a_c / an - b_c / bn)^2;   tap[p] = mean over the pixels of d
// (torchmetrics >= 1.0's _normalize_tensor: the eps sits under the root).  All of it in fp32.
// 1. a group of G = 2^k lanes (the smallest with 8 G >= C, at most 64) owns a pixel: 16-byte loads, the three sums by xor shuffles
//    inside the group; a workgroup walks LP_PIX pixels, group 0's lane adds its pixels' d in walk order, then the 256 lanes' sums go
//    through a fixed tree: one partial per (pair, workgroup).  The grid depends on HW alone, so a pair's partials do not depend on n.
// 2. one workgroup per pair adds the partials in a fixed order, divides by HW and writes or adds to out[pair].
// Identical a and b take identical arithmetic: every difference is exactly 0.  A zero vector normalises to zeros (an = 1e-4).
// ---------------------------------------------------------------------------------------------------------------
static constexpr int LP_PIX = 256;

__global__ void __launch_bounds__(256) lpips_layer_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, const float* __restrict__ w,
                                                          int HW, int C, int G, float* __restrict__ partial) {
  __shared__ float s[256];
  const int tid = threadIdx.x, g = tid & (G - 1), grp = tid / G, ngrp = 256 / G;
  const int pair = blockIdx.y, p0 = blockIdx.x * LP_PIX, p1 = min(p0 + LP_PIX, HW);
  float local = 0.f;
  for (int pb = p0; pb < p1; pb += ngrp) {      // every lane of the workgroup takes every turn (the shuffles below)
    const int pix = pb + grp;
    const bool on = pix < p1;
    const half_t* pa = a + ((size_t)pair * HW + (on ? pix : p0)) * C;
    const half_t* pq = b + ((size_t)pair * HW + (on ? pix : p0)) * C;
    float sa = 0.f, sb = 0.f;
    for (int c = g * 8; c < C; c += G * 8) {
      const half8 ha = ldg_half8(pa + c), hb = ldg_half8(pq + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sa = __builtin_fmaf((float)ha[j], (float)ha[j], sa);
        sb = __builtin_fmaf((float)hb[j], (float)hb[j], sb);
      }
    }
    for (int off = G >> 1; off > 0; off >>= 1) { sa += __shfl_xor(sa, off, 64); sb += __shfl_xor(sb, off, 64); }
    const float na = sqrtf(1e-8f + sa), nb = sqrtf(1e-8f + sb);
    float d = 0.f;
    for (int c = g * 8; c < C; c += G * 8) {      // the second read of the pixel's 2 C bytes comes from the cache
      const half8 ha = ldg_half8(pa + c), hb = ldg_half8(pq + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float df = (float)ha[j] / na - (float)hb[j] / nb;
        d = __builtin_fmaf(w[c + j], df * df, d);
      }
    }
    for (int off = G >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
    if (on && g == 0) local += d;
  }
  s[tid] = local;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) s[tid] += s[tid + off];
    __syncthreads();
  }
  if (tid == 0) partial[(size_t)pair * gridDim.x + blockIdx.x] = s[0];
}

__global__ void __launch_bounds__(256) lpips_reduce_kernel(const float* __restrict__ partial, int nblk, int HW, float* __restrict__ out,
                                                           int accumulate) {
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
  if (tid == 0) {
    const float m = s[0] / (float)HW;
    out[pair] = accumulate ? out[pair] + m : m;
  }
}

size_t lpips_layer_scratch_floats(int n, int HW) { return (size_t)n * ((HW + LP_PIX - 1) / LP_PIX); }

int launch_lpips_layer(const half_t* a, const half_t* b, const float* w, int n, int HW, int C, float* scratch, float* out, int accumulate,
                       hipStream_t st) {
  if (!a || !b || !w || !scratch || !out || n <= 0 || n > 65535 || HW <= 0 || HW > (1 << 26) || C <= 0 || (C & 7)) return -3;
  if (((uintptr_t)a | (uintptr_t)b) & 15) return -3;
  int G = 1;
  while (G < 64 && G * 8 < C) G <<= 1;
  const int nblk = (HW + LP_PIX - 1) / LP_PIX;
  lpips_layer_kernel<<<dim3(nblk, n), 256, 0, st>>>(a, b, w, HW, C, G, scratch);
  HIP_CHECK_RET(hipGetLastError());
  lpips_reduce_kernel<<<n, 256, 0, st>>>(scratch, nblk, HW, out, accumulate);
  return (int)hipGetLastError();
}
