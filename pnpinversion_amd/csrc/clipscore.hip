// CLIP similarity kernels for gfx950: the preprocessing of transformers' CLIPProcessor (PIL bicubic resize, rescale, normalise) straight
// into the patch rows the patch-embedding GEMM reads, token assembly, the pooled-row gather of both towers and the cosine score.
// Reference semantics: torchmetrics CLIPScore + CLIPProcessor as evaluation/matrics_calculator.py:290-302 calls them.
#include <limits.h>

#include "ops.h"

// ---------------------------------------------------------------------------------------------------------------
// PIL Image.resize(size, BICUBIC) for 8-bit RGB (libImaging/Resample.c): per output pixel a window of `taps` source pixels from
// `first`, weights in 22-bit fixed point that were normalised in double and rounded half away from zero on the host; every pass starts
// its accumulator at 2^21, shifts right by 22 and clamps to 0 .. 255.  Horizontal pass, then vertical pass on its uint8 result.
// ---------------------------------------------------------------------------------------------------------------
static constexpr int CLIP_PREC = 22;

__device__ __forceinline__ unsigned clip_u8(int acc) {
  const int v = acc >> CLIP_PREC;      // arithmetic shift, as PIL's lookup of (in >> PRECISION_BITS)
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// row copies between global memory and LDS: 16-byte vectors over the aligned body, bytes over the tail (or over everything when the
// global pointer is not 16-byte aligned)
__device__ __forceinline__ void row_g2s(uint8_t* s, const uint8_t* g, int nbytes, int tid) {
  const int nv = (((uintptr_t)g & 15) == 0) ? nbytes >> 4 : 0;
  for (int i = tid; i < nv; i += 256) reinterpret_cast<uint4*>(s)[i] = reinterpret_cast<const uint4*>(g)[i];
  for (int i = nv * 16 + tid; i < nbytes; i += 256) s[i] = g[i];
}
__device__ __forceinline__ void row_s2g(uint8_t* g, const uint8_t* s, int nbytes, int tid) {
  const int nv = (((uintptr_t)g & 15) == 0) ? nbytes >> 4 : 0;
  for (int i = tid; i < nv; i += 256) reinterpret_cast<uint4*>(g)[i] = reinterpret_cast<const uint4*>(s)[i];
  for (int i = nv * 16 + tid; i < nbytes; i += 256) g[i] = s[i];
}

// one workgroup per source row: the row (times its mask) in LDS, one output pixel (three channels) per thread
__global__ void __launch_bounds__(256) clip_resize_h_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, int S, int out,
                                                            const int* __restrict__ bounds, const int* __restrict__ coef, int ksize,
                                                            uint8_t* __restrict__ tmp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t clip_smem[];
  const int y = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int rowb = S * 3, orowb = out * 3;
  uint8_t* srow = clip_smem;
  uint8_t* orow = clip_smem + ((rowb + 15) & ~15);
  row_g2s(srow, img + ((size_t)b * S + y) * rowb, rowb, tid);
  __syncthreads();
  if (mask) {      // uint8(img * mask), the mask broadcast over the channels: 0 clears the pixel, 1 keeps it
    const uint8_t* m = mask + ((size_t)b * S + y) * S;
    const int nv = (((uintptr_t)m & 15) == 0) ? S >> 4 : 0;
    for (int i = tid; i < nv; i += 256) {
      const uint4 mv = reinterpret_cast<const uint4*>(m)[i];
      const unsigned w[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (((w[q] >> (8 * j)) & 255u) == 0) {
            uint8_t* p = srow + (i * 16 + q * 4 + j) * 3;
            p[0] = 0; p[1] = 0; p[2] = 0;
          }
    }
    for (int x = nv * 16 + tid; x < S; x += 256)
      if (m[x] == 0) { uint8_t* p = srow + x * 3; p[0] = 0; p[1] = 0; p[2] = 0; }
    __syncthreads();
  }
  for (int ox = tid; ox < out; ox += 256) {
    const int first = bounds[2 * ox], taps = bounds[2 * ox + 1];
    const int* k = coef + (size_t)ox * ksize;
    const uint8_t* p = srow + first * 3;
    int s0 = 1 << (CLIP_PREC - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < taps; ++j) {
      const int w = k[j];
      s0 += (int)p[3 * j] * w; s1 += (int)p[3 * j + 1] * w; s2 += (int)p[3 * j + 2] * w;
    }
    orow[3 * ox] = (uint8_t)clip_u8(s0); orow[3 * ox + 1] = (uint8_t)clip_u8(s1); orow[3 * ox + 2] = (uint8_t)clip_u8(s2);
  }
  __syncthreads();
  row_s2g(tmp + ((size_t)b * S + y) * orowb, orow, orowb, tid);
}

__device__ __forceinline__ float clip_normalise(unsigned v, int c) {
  // CLIPImageProcessor: rescale by 1 / 255, then (x - mean) / std with OPENAI_CLIP_MEAN / OPENAI_CLIP_STD
  const float mean = c == 0 ? 0.48145466f : (c == 1 ? 0.4578275f : 0.40821073f);
  const float sd = c == 0 ? 0.26862954f : (c == 1 ? 0.26130258f : 0.27577711f);
  return ((float)v / 255.f - mean) / sd;
}

// one workgroup per output row: four bytes of the row per thread (32-bit loads down the window of tmp rows), the row in LDS, then the
// resized image row and / or the row's 3 * G runs of `patch` normalised pixels in the patch rows
__global__ void __launch_bounds__(256) clip_resize_v_kernel(const uint8_t* __restrict__ tmp, int S, int out, const int* __restrict__ bounds,
                                                            const int* __restrict__ coef, int ksize, int patch, int Kp,
                                                            uint8_t* __restrict__ resized, half_t* __restrict__ patches) {
  extern __shared__ __attribute__((aligned(16))) uint8_t clip_smem[];
  uint8_t* res = clip_smem;
  const int oy = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int orowb = out * 3;
  const int first = bounds[2 * oy], taps = bounds[2 * oy + 1];
  const int* k = coef + (size_t)oy * ksize;
  const uint8_t* base = tmp + ((size_t)b * S + first) * orowb;
  if ((orowb & 3) == 0 && ((uintptr_t)tmp & 3) == 0) {
    for (int q = tid; q < (orowb >> 2); q += 256) {
      int s0 = 1 << (CLIP_PREC - 1), s1 = s0, s2 = s0, s3 = s0;
      for (int j = 0; j < taps; ++j) {
        const unsigned v = *reinterpret_cast<const unsigned*>(base + (size_t)j * orowb + 4 * q);
        const int w = k[j];
        s0 += (int)(v & 255u) * w; s1 += (int)((v >> 8) & 255u) * w; s2 += (int)((v >> 16) & 255u) * w; s3 += (int)(v >> 24) * w;
      }
      reinterpret_cast<unsigned*>(res)[q] = clip_u8(s0) | (clip_u8(s1) << 8) | (clip_u8(s2) << 16) | (clip_u8(s3) << 24);
    }
  } else {
    for (int e = tid; e < orowb; e += 256) {
      int s0 = 1 << (CLIP_PREC - 1);
      for (int j = 0; j < taps; ++j) s0 += (int)base[(size_t)j * orowb + e] * k[j];
      res[e] = (uint8_t)clip_u8(s0);
    }
  }
  __syncthreads();
  if (resized) row_s2g(resized + ((size_t)b * out + oy) * orowb, res, orowb, tid);
  if (!patches) return;
  const int G = out / patch, py = oy / patch, ky = oy - py * patch, pp = patch * patch, K = 3 * pp;
  half_t* prow0 = patches + ((size_t)b * G * G + (size_t)py * G) * Kp;      // patch (py, 0) of this image
  if ((patch & 1) == 0) {      // element offsets c * pp + ky * patch + kx are even with kx: 4-byte stores
    const int hp = patch >> 1, items = G * 3 * hp;
    for (int it = tid; it < items; it += 256) {
      const int kx = 2 * (it % hp), c = (it / hp) % 3, px = it / (hp * 3);
      const int ox = px * patch + kx;
      half2v h = {(half_t)clip_normalise(res[ox * 3 + c], c), (half_t)clip_normalise(res[(ox + 1) * 3 + c], c)};
      *reinterpret_cast<half2v*>(prow0 + (size_t)px * Kp + c * pp + ky * patch + kx) = h;
    }
    if (ky == 0) {             // the pad columns of this patch row's G patches
      const int hz = (Kp - K) >> 1;
      const half2v z = {(half_t)0.f, (half_t)0.f};
      for (int it = tid; it < G * hz; it += 256) *reinterpret_cast<half2v*>(prow0 + (size_t)(it / hz) * Kp + K + 2 * (it % hz)) = z;
    }
  } else {
    const int items = G * 3 * patch;
    for (int it = tid; it < items; it += 256) {
      const int kx = it % patch, c = (it / patch) % 3, px = it / (patch * 3);
      prow0[(size_t)px * Kp + c * pp + ky * patch + kx] = (half_t)clip_normalise(res[(px * patch + kx) * 3 + c], c);
    }
    if (ky == 0) {
      const int nz = Kp - K;
      for (int it = tid; it < G * nz; it += 256) prow0[(size_t)(it / nz) * Kp + K + it % nz] = (half_t)0.f;
    }
  }
}

static constexpr int CLIP_LDS_MAX = 48 << 10;

int launch_clip_resize_h(const uint8_t* img, const uint8_t* mask, int n, int S, int out, const int* bounds, const int* coef, int ksize,
                         uint8_t* tmp, hipStream_t st) {
  if (!img || !bounds || !coef || !tmp || n <= 0 || S <= 0 || out <= 0 || out > S || ksize <= 0) return -3;
  const size_t lds = (size_t)((S * 3 + 15) & ~15) + (size_t)((out * 3 + 15) & ~15);
  if (lds > (size_t)CLIP_LDS_MAX) return -3;
  clip_resize_h_kernel<<<dim3(S, n), 256, lds, st>>>(img, mask, S, out, bounds, coef, ksize, tmp);
  return (int)hipGetLastError();
}
int launch_clip_resize_v(const uint8_t* tmp, int n, int S, int out, const int* bounds, const int* coef, int ksize, int patch, int Kp,
                         uint8_t* resized, half_t* patches, hipStream_t st) {
  if (!tmp || !bounds || !coef || n <= 0 || S <= 0 || out <= 0 || out > S || ksize <= 0 || (!resized && !patches)) return -3;
  if (patches && (patch <= 0 || out % patch || Kp < 3 * patch * patch || (Kp & 7))) return -3;
  const size_t lds = (size_t)((out * 3 + 15) & ~15);
  if (lds > (size_t)CLIP_LDS_MAX) return -3;
  clip_resize_v_kernel<<<dim3(out, n), 256, lds, st>>>(tmp, S, out, bounds, coef, ksize, patch, Kp, resized, patches);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// A ViT's token assembly: cat([class token, patch embeddings]) + position embedding, where pe is the bias-free GEMM over the patch
// rows.  bias (nullable) is the convolution's: CLIP's patch embedding has none, DINO's is added here.  (pe [+ bias]) + pos in fp32,
// one rounding to fp16; the class row takes no bias.  Eight channels per thread, 16-byte loads (W % 8 == 0, 16-byte aligned rows).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ldg_float8(const float* __restrict__ p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__global__ void __launch_bounds__(256) vit_assemble_tokens_kernel(const half_t* __restrict__ pe, const float* __restrict__ bias,
                                                                  const float* __restrict__ cls, const float* __restrict__ pos, int n, int NP,
                                                                  int W, half_t* __restrict__ x) {
  const int W8 = W >> 3, T = NP + 1;
  const size_t total = (size_t)n * T * W8;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % W8) * 8;
    const size_t row = i / W8;
    const int t = (int)(row % T), b = (int)(row / T);
    float v[8], pv[8];
    if (t == 0) {
      ldg_float8(cls + c, v);
    } else {
      const half8 h = ldg_half8(pe + ((size_t)b * NP + (t - 1)) * W + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
      if (bias) {
        float bv[8];
        ldg_float8(bias + c, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += bv[j];
      }
    }
    ldg_float8(pos + (size_t)t * W + c, pv);
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)(v[j] + pv[j]);
    *reinterpret_cast<half8*>(x + row * W + c) = o;
  }
}
int launch_vit_assemble_tokens(const half_t* pe, const float* bias, const float* cls, const float* pos, int n, int NP, int W, half_t* x,
                               hipStream_t st) {
  if (!pe || !cls || !pos || !x || n <= 0 || NP <= 0 || W <= 0 || (W & 7)) return -3;
  const size_t total = (size_t)n * (NP + 1) * (W >> 3);
  int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
  vit_assemble_tokens_kernel<<<blocks, 256, 0, st>>>(pe, bias, cls, pos, n, NP, W, x);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// The pooled row of each sequence: token 0 (image tower: the class token) or the first position of the row's largest id (text tower:
// transformers' input_ids.argmax(-1), the EOS token of CLIP's vocabulary).  One workgroup per sequence.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) clip_gather_rows_kernel(const half_t* __restrict__ x, int T, int H, const int* __restrict__ ids,
                                                               half_t* __restrict__ out) {
  __shared__ int s_val[256], s_pos[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  int tok = 0;
  if (ids) {
    int bv = INT_MIN, bp = 0x7fffffff;
    for (int t = tid; t < T; t += 256) {
      const int v = ids[(size_t)b * T + t];
      if (v > bv) { bv = v; bp = t; }      // ascending t per thread: the first position of the thread's maximum
    }
    s_val[tid] = bv; s_pos[tid] = bp;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) {
        const int ov = s_val[tid + off], op = s_pos[tid + off];
        if (ov > s_val[tid] || (ov == s_val[tid] && op < s_pos[tid])) { s_val[tid] = ov; s_pos[tid] = op; }
      }
      __syncthreads();
    }
    tok = s_pos[0];
  }
  const half_t* src = x + ((size_t)b * T + tok) * H;
  for (int c = tid * 8; c < H; c += 256 * 8) *reinterpret_cast<half8*>(out + (size_t)b * H + c) = ldg_half8(src + c);
}
int launch_clip_gather_rows(const half_t* x, int n, int T, int H, const int* ids, half_t* out, hipStream_t st) {
  if (!x || !out || n <= 0 || T <= 0 || H <= 0 || (H & 7)) return -3;
  clip_gather_rows_kernel<<<n, 256, 0, st>>>(x, T, H, ids, out);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// CLIPScore: 100 * cos(image, text) clamped at 0; the two squared norms and the dot product in fp32, one wavefront per pair
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) clip_cosine_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, int D,
                                                          float* __restrict__ out) {
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pair >= n) return;
  const float* pa = a + (size_t)pair * D;
  const float* pb = b + (size_t)pair * D;
  float aa = 0.f, bb = 0.f, ab = 0.f;
  if ((D & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0) {
    for (int i = lane * 4; i < D; i += 64 * 4) {
      const float4 u = *reinterpret_cast<const float4*>(pa + i), v = *reinterpret_cast<const float4*>(pb + i);
      aa += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
      bb += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
      ab += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
    }
  } else {
    for (int i = lane; i < D; i += 64) { aa += pa[i] * pa[i]; bb += pb[i] * pb[i]; ab += pa[i] * pb[i]; }
  }
  aa = wave_sum(aa); bb = wave_sum(bb); ab = wave_sum(ab);
  if (lane == 0) out[pair] = fmaxf(100.f * (ab / (sqrtf(aa) * sqrtf(bb))), 0.f);
}
int launch_clip_cosine(const float* a, const float* b, int n, int D, float* out, hipStream_t st) {
  if (!a || !b || !out || n <= 0 || D <= 0) return -3;
  clip_cosine_kernel<<<(n + 3) / 4, 256, 0, st>>>(a, b, n, D, out);
  return (int)hipGetLastError();
}
