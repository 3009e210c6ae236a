// What the implicit-GEMM kernels share after the last MFMA, once each: epilogue_store4, the scalar fallback store of four columns of one
// output row (igemm_kernel, igemm_dma_kernel and the split-K combine in gemm.hip), and epilogue_geglu_vec, one output vector of the GEGLU
// drain of an LDS-staged pass (igemm_dma_kernel, igemm_pp_kernel).  Loops, barriers and the accumulator -> LDS staging stay in the kernels.
#pragma once
#include "ops.h"

__device__ __forceinline__ void epilogue_store4(const GemmP& p, int m, int nb, const float* v, const float* bias) {
  if (m >= p.M) return;
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int n = nb + j;
    float x = v[j] * p.alpha;
    if (n < p.N) {
      if (bias) x += bias[n];
      if (p.res) x += (float)p.res[(size_t)m * p.ldres + n];
    }
    o[j] = x;
  }
  if (nb + 3 < p.vt_col0 && nb + 3 < p.N && (p.ldo & 3) == 0) {
    half4 h;
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = (half_t)o[j];
    *reinterpret_cast<half4*>(p.out + (size_t)m * p.ldo + nb) = h;
    return;
  }
  int b = 0, tok = m;
  if (nb + 3 >= p.vt_col0) { b = m / p.rows_per_batch; tok = m - b * p.rows_per_batch; }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int n = nb + j;
    if (n >= p.N) continue;
    if (n < p.vt_col0) {
      p.out[(size_t)m * p.ldo + n] = (half_t)o[j];
    } else {
      size_t idx = ((size_t)b * (p.N - p.vt_col0) + (n - p.vt_col0)) * p.vt_ld + (p.vt_perm16 ? vt_perm16_pos(tok) : tok);
      if (p.vt_f32) ((float*)p.outT)[idx] = o[j];
      else ((half_t*)p.outT)[idx] = (half_t)o[j];
    }
  }
}

// GEGLU: columns come in [x(32) | gate(32)] groups; the block's BN columns hold BN/2 outputs starting at column n0/2; idx = one
// 8-column output vector of the pass's EROWS * (BN / 16), staged as [EROWS][OLD]
template <int BN, int OLD>
__device__ __forceinline__ void epilogue_geglu_vec(const GemmP& p, const half_t* sOut, int mrow0, int n0, int idx) {
  constexpr int VPO = BN / 16;
  const int r = idx / VPO, v = idx - r * VPO;
  const int m = mrow0 + r;
  const int xc = (v >> 2) * 64 + (v & 3) * 8;     // local column of the x vector; its gate sits 32 columns further
  const int no = (n0 >> 1) + v * 8;
  if (m < p.M && no < (p.N >> 1)) {
    const half8 x = *reinterpret_cast<const half8*>(sOut + r * OLD + xc);
    const half8 gt = *reinterpret_cast<const half8*>(sOut + r * OLD + xc + 32);
    half8 o8;
#pragma unroll
    for (int j = 0; j < 8; ++j) o8[j] = (half_t)((float)x[j] * gelu_f((float)gt[j]));
    *reinterpret_cast<half8*>(p.out + (size_t)m * p.ldo + no) = o8;
  }
}
