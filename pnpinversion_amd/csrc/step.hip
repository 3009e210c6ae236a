// Latent-space step kernels: DDIM invert / denoise update, classifier-free guidance, the direct-inversion "3 lines",
// and LocalBlend. fp32 NCHW latents, coalesced, wavefront-uniform scalars; every multiply/add is an explicit
// round-to-nearest op in the reference's order (no FMA contraction), so these kernels are bit-exact against the
// reference formulas given the same eps.
//
// Reference: DirectInversion.next_step models/p2p/inversion.py:262-270, prev_step :247-260,
//   DDIMSchedulerDev.step models/p2p/scheduler_dev.py:38-95 (eta = 0, epsilon prediction, no clipping),
//   CFG + offset lines inversion.py:383-389 and p2p_guidance_forward.py:110-114,
//   LocalBlend.__call__/get_mask models/p2p/attention_control.py:97-121.
#include "ops.h"

// The reference evaluates each multiply / add / divide as a separately rounded fp32 op (eager PyTorch).  hipcc would
// contract a*b+c into one FMA (single rounding) by default, so contraction is switched off for this file.
#pragma clang fp contract(off)

__device__ __forceinline__ float ddim_update(float x, float e, float sqrt_a_from, float sqrt_b_from, float sqrt_a_to,
                                             float sqrt_b_to) {
  // pred_x0 = (x - sqrt(1-a_from) * e) / sqrt(a_from);  dir = sqrt(1-a_to) * e;  out = sqrt(a_to) * pred_x0 + dir
  float x0 = __fdiv_rn(__fsub_rn(x, __fmul_rn(sqrt_b_from, e)), sqrt_a_from);
  float dir = __fmul_rn(sqrt_b_to, e);
  return __fadd_rn(__fmul_rn(sqrt_a_to, x0), dir);
}

__global__ void ddim_move_kernel(const float* __restrict__ x, const float* __restrict__ eps, float sa_f, float sb_f, float sa_t,
                                 float sb_t, size_t n, float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = ddim_update(x[i], eps[i], sa_f, sb_f, sa_t, sb_t);
}

int launch_ddim_move(const float* x, const float* eps, float a_from, float a_to, size_t n, float* out, hipStream_t st) {
  // torch computes `t ** 0.5` on 0-dim fp32 tensors: correctly rounded fp32 sqrt of fp32 operands
  float sa_f = sqrtf(a_from), sb_f = sqrtf(1.0f - a_from), sa_t = sqrtf(a_to), sb_t = sqrtf(1.0f - a_to);
  int blocks = (int)((n + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  ddim_move_kernel<<<blocks, 256, 0, st>>>(x, eps, sa_f, sb_f, sa_t, sb_t, n, out);
  return (int)hipGetLastError();
}

// DDIMSchedulerDev.step with the reconstruction pull (scheduler_dev.py:68-76), level-1 form: ref / mask already expanded to the sample's
// shape.  pred_x0 = (x - sqrt(1-a_t) e) / sqrt(a_t);  pred_x0 -= lr * (pred_x0 - ref) [* mask];  prev = sqrt(a_p) pred_x0 + sqrt(1-a_p) e.
// pred_x0_out (nullable) receives the pulled pred_original_sample (the reference returns it).
__global__ void ddim_prev_recon_kernel(const float* __restrict__ x, const float* __restrict__ eps, float sa_f, float sb_f, float sa_t, float sb_t,
                                       const float* __restrict__ ref, float lr, const float* __restrict__ mask, size_t n,
                                       float* __restrict__ out, float* __restrict__ x0_out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float e = eps[i];
    float x0 = __fdiv_rn(__fsub_rn(x[i], __fmul_rn(sb_f, e)), sa_f);
    if (ref) {
      float pull = __fmul_rn(lr, __fsub_rn(x0, ref[i]));
      if (mask) pull = __fmul_rn(pull, mask[i]);
      x0 = __fsub_rn(x0, pull);
    }
    if (x0_out) x0_out[i] = x0;
    out[i] = __fadd_rn(__fmul_rn(sa_t, x0), __fmul_rn(sb_t, e));
  }
}
int launch_ddim_prev_recon(const float* x, const float* eps, float a_from, float a_to, const float* ref, float lr, const float* mask, size_t n,
                           float* out, float* x0_out, hipStream_t st) {
  float sa_f = sqrtf(a_from), sb_f = sqrtf(1.0f - a_from), sa_t = sqrtf(a_to), sb_t = sqrtf(1.0f - a_to);
  int blocks = (int)((n + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  ddim_prev_recon_kernel<<<blocks, 256, 0, st>>>(x, eps, sa_f, sb_f, sa_t, sb_t, ref, lr, mask, n, out, x0_out);
  return (int)hipGetLastError();
}

// proximal guidance (proximal_guidance_forward.py:39-62): score_delta -= clamp(score_delta, -thr, thr); 'l1' then shrinks the
// survivors by thr once more on each side
__device__ __forceinline__ float prox_shrink(float d, float th, int mode) {
  d = __fsub_rn(d, fminf(fmaxf(d, -th), th));
  if (mode == 2) {
    if (d > 0.f) d = __fsub_rn(d, th);
    if (d < 0.f) d = __fadd_rn(d, th);
  }
  return d;
}

// eps: [nimg][2R][E] (first R rows unconditional, next R conditional); x: [nimg][R][E]
//   e   = eps_u + g * (eps_c - eps_u)
//   prev = ddim(x, e)
//   target != null  (offset_calculate):  loss = (target[img] - prev) * oscale ; offset_out = loss ; x_out = prev + loss
//   else noise_loss != null            :  x_out = prev + noise_loss[img][r]  for r < offset_rows, prev otherwise
// recon_ref != null (reconstruction guidance, proximal_guidance_forward.py:48-51,60-72 + DDIMSchedulerDev.step scheduler_dev.py:68-76):
//   mask_edit = |shrunk delta| > thr, dilated by a (2*dil+1)^2 max-pool over each [h][w] plane (in-bounds neighbours only);
//   pred_x0 -= recon_lr * (pred_x0 - ref[img]) * (1 - mask_edit)   before the step's second half
// inv_ref != null (inversion guidance, proximal_guidance_forward.py:73-75): the step's RESULT is pulled towards the inversion trajectory
//   outside the same mask: x_out -= recon_lr * (x_out - inv_ref[img]) * (1 - mask_edit), inv_ref = x*_{t-1} for both rows of the image
__global__ void cfg_ddim_prev_kernel(const float* __restrict__ eps, const float* __restrict__ x, int nimg, int R, size_t E, float g,
                                     float sa_f, float sb_f, float sa_t, float sb_t, const float* __restrict__ noise_loss,
                                     int offset_rows, const float* __restrict__ target, float oscale,
                                     float* __restrict__ offset_out, float* __restrict__ x_out, const float* __restrict__ prox_thr,
                                     int prox_mode, const float* __restrict__ recon_ref, float recon_lr, int dil, int lat_h, int lat_w,
                                     const float* __restrict__ inv_ref) {
  const size_t total = (size_t)nimg * R * E;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    size_t e_idx = i % E;
    size_t ir = i / E;
    int r = (int)(ir % R);
    int img = (int)(ir / R);
    const float* eu_row = eps + ((size_t)img * 2 * R + r) * E;
    const float* ec_row = eps + ((size_t)img * 2 * R + R + r) * E;
    float eu = eu_row[e_idx];
    float ec = ec_row[e_idx];
    float d = __fsub_rn(ec, eu);
    const float th = prox_mode ? prox_thr[img] : 0.f;
    if (prox_mode) d = prox_shrink(d, th, prox_mode);
    float e = __fadd_rn(eu, __fmul_rn(g, d));
    float prev;
    if ((recon_ref || inv_ref) && prox_mode) {
      float mask_edit = fabsf(d) > th ? 1.f : 0.f;
      if (dil > 0 && mask_edit == 0.f) {
        const int hw = lat_h * lat_w;
        const int pl = (int)(e_idx / hw), py = (int)(e_idx % hw) / lat_w, px = (int)(e_idx % hw) % lat_w;
        for (int dy = -dil; dy <= dil && mask_edit == 0.f; ++dy)
          for (int dx = -dil; dx <= dil; ++dx) {
            const int yy = py + dy, xx = px + dx;
            if (yy < 0 || yy >= lat_h || xx < 0 || xx >= lat_w) continue;
            const size_t j = (size_t)pl * hw + (size_t)yy * lat_w + xx;
            const float dn = prox_shrink(__fsub_rn(ec_row[j], eu_row[j]), th, prox_mode);
            if (fabsf(dn) > th) { mask_edit = 1.f; break; }
          }
      }
      const float recon_mask = __fsub_rn(1.f, mask_edit);
      if (recon_ref) {
        float x0 = __fdiv_rn(__fsub_rn(x[i], __fmul_rn(sb_f, e)), sa_f);
        x0 = __fsub_rn(x0, __fmul_rn(__fmul_rn(recon_lr, __fsub_rn(x0, recon_ref[(size_t)img * E + e_idx])), recon_mask));
        prev = __fadd_rn(__fmul_rn(sa_t, x0), __fmul_rn(sb_t, e));
      } else {
        prev = ddim_update(x[i], e, sa_f, sb_f, sa_t, sb_t);
      }
      if (inv_ref) prev = __fsub_rn(prev, __fmul_rn(__fmul_rn(recon_lr, __fsub_rn(prev, inv_ref[(size_t)img * E + e_idx])), recon_mask));
    } else {
      prev = ddim_update(x[i], e, sa_f, sb_f, sa_t, sb_t);
    }
    float outv = prev;
    if (target) {
      // loss = (x*_{t-1} - prev) * scale: scale is 1 on the paper's path, `scale` / 0-or-1 in the not_full / skip_step ablations
      // (inversion.py:491-492, 512-515)
      float loss = __fmul_rn(__fsub_rn(target[(size_t)img * E + e_idx], prev), oscale);
      offset_out[i] = loss;
      outv = __fadd_rn(prev, loss);
    } else if (noise_loss && r < offset_rows) {
      outv = __fadd_rn(prev, noise_loss[i]);
    }
    x_out[i] = outv;
  }
}

int launch_cfg_ddim_prev(const CfgStepP& p, hipStream_t st) {
  float sa_f = sqrtf(p.a_t), sb_f = sqrtf(1.0f - p.a_t), sa_t = sqrtf(p.a_prev), sb_t = sqrtf(1.0f - p.a_prev);
  size_t total = (size_t)p.nimg * p.rows_per_img * p.row_elems;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  if ((p.recon_ref || p.inv_ref) && (p.lat_h <= 0 || p.lat_w <= 0 || p.row_elems % ((size_t)p.lat_h * p.lat_w))) return -3;
  cfg_ddim_prev_kernel<<<blocks, 256, 0, st>>>(p.eps, p.x, p.nimg, p.rows_per_img, p.row_elems, p.gscale, sa_f, sb_f, sa_t, sb_t, p.noise_loss,
                                               p.offset_rows, p.target, p.offset_scale, p.offset_out, p.x_out, p.prox_thr, p.prox_mode,
                                               p.recon_ref, p.recon_lr, p.dilate, p.lat_h, p.lat_w, p.inv_ref);
  return (int)hipGetLastError();
}

// torch.quantile(|eps_c - eps_u|, q) over all R rows of one image (proximal_guidance_forward.py:41,53: the threshold of the
// proximal step), default 'linear' interpolation: sort, pos = q * (n - 1), lerp(x[floor], x[floor + 1], frac).  One block per
// image; the n <= 32768 magnitudes are sorted in LDS (bitonic, padded with +inf to a power of two).
__global__ void __launch_bounds__(1024) quantile_abs_diff_kernel(const float* __restrict__ eps, int R, size_t E, float q, int npow2,
                                                                 float* __restrict__ thr_out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* s = reinterpret_cast<float*>(smem_raw);
  const int img = blockIdx.x, tid = threadIdx.x;
  const int n = (int)(R * E);
  const float* base = eps + (size_t)img * 2 * R * E;
  for (int i = tid; i < npow2; i += blockDim.x)
    s[i] = i < n ? fabsf(__fsub_rn(base[(size_t)R * E + i], base[i])) : INFINITY;
  __syncthreads();
  for (int k = 2; k <= npow2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npow2; i += blockDim.x) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & k) == 0;
          const float a = s[i], b = s[l];
          if ((a > b) == up) { s[i] = b; s[l] = a; }
        }
      }
      __syncthreads();
    }
  if (tid == 0) {
    const float pos = __fmul_rn(q, (float)(n - 1));
    const int lo = (int)floorf(pos);
    const int hi = lo + 1 < n ? lo + 1 : n - 1;
    const float w = __fsub_rn(pos, (float)lo);
    const float a = s[lo], b = s[hi];
    // torch.lerp: a + w * (b - a) for w < 0.5, b - (b - a) * (1 - w) otherwise
    thr_out[img] = w < 0.5f ? __fadd_rn(a, __fmul_rn(w, __fsub_rn(b, a))) : __fsub_rn(b, __fmul_rn(__fsub_rn(b, a), __fsub_rn(1.f, w)));
  }
}

int launch_quantile_abs_diff(const float* eps, int nimg, int rows_per_img, size_t row_elems, float q, float* thr_out, hipStream_t st) {
  const size_t n = (size_t)rows_per_img * row_elems;
  int npow2 = 1;
  while ((size_t)npow2 < n) npow2 <<= 1;
  if (npow2 > 32768) return -6;
  static DeviceOnce attr_once;
  if (int r = once_per_device(attr_once, [&]() { return (int)hipFuncSetAttribute((const void*)quantile_abs_diff_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4); })) return r;
  quantile_abs_diff_kernel<<<nimg, 1024, (size_t)npow2 * sizeof(float), st>>>(eps, rows_per_img, row_elems, q, npow2, thr_out);
  return (int)hipGetLastError();
}

__global__ void fill_f32_kernel(float* p, int n, float v) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
int launch_fill_f32(float* p, int n, float v, hipStream_t st) {
  fill_f32_kernel<<<(n + 255) / 256, 256, 0, st>>>(p, n, v);
  return (int)hipGetLastError();
}

// One block per image. lb_acc: [nimg][nslots][planes][map_hw*map_hw] accumulated (summed over steps) selector-weighted maps; planes 0, 1 =
// the blend words of the source / target prompt, planes 2, 3 (planes == 4) = the substruct words.
// blend maps   -> mean over slots -> 3x3 max-pool (stride 1, pad 1) -> nearest resize to lat_hw -> / max -> > th      (get_mask, use_pool)
// substruct    -> mean over slots ->              (no pooling)      -> nearest resize          -> / max -> > th_sub  (attention_control.py:97-118)
// mask_tgt = (mask_src | mask_tgt) & ~(sub_src | sub_tgt);  x_tgt = x_src + mask_tgt * (x_tgt - x_src)   (latents [nimg][2][C][lat_hw^2])
__global__ void __launch_bounds__(256) local_blend_kernel(const float* __restrict__ lb_acc, int nslots, int mhw, int lhw, int C,
                                                          float th, float* __restrict__ latents, int planes, float th_sub) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int MP = mhw * mhw;
  float* s_map = reinterpret_cast<float*>(smem_raw);  // [4][MP]   mean maps
  float* s_pool = s_map + 4 * MP;                     // [4][MP]   pooled (planes 0, 1) / copied (planes 2, 3)
  float* s_red = s_pool + 4 * MP;                     // [4][256]
  const int img = blockIdx.x, tid = threadIdx.x;
  for (int idx = tid; idx < planes * MP; idx += blockDim.x) {
    int which = idx / MP, pix = idx - which * MP;
    float s = 0.f;
    for (int sl = 0; sl < nslots; ++sl) s += lb_acc[(((size_t)img * nslots + sl) * planes + which) * MP + pix];
    s_map[idx] = s / (float)nslots;
  }
  __syncthreads();
  float lmax[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int idx = tid; idx < planes * MP; idx += blockDim.x) {
    int which = idx / MP, pix = idx - which * MP;
    int y = pix / mhw, x = pix - y * mhw;
    float m = -INFINITY;
    if (which < 2) {
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          int yy = y + dy, xx = x + dx;
          if (yy >= 0 && yy < mhw && xx >= 0 && xx < mhw) m = fmaxf(m, s_map[which * MP + yy * mhw + xx]);
        }
    } else {
      m = s_map[idx];
    }
    s_pool[idx] = m;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if (w == which) lmax[w] = fmaxf(lmax[w], m);
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) s_red[w * 256 + tid] = lmax[w];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int w = 0; w < 4; ++w) s_red[w * 256 + tid] = fmaxf(s_red[w * 256 + tid], s_red[w * 256 + tid + off]);
    }
    __syncthreads();
  }
  const float mx0 = s_red[0], mx1 = s_red[256], mx2 = s_red[512], mx3 = s_red[768];
  const int LP = lhw * lhw;
  float* xs = latents + (size_t)img * 2 * C * LP;
  float* xt = xs + (size_t)C * LP;
  for (int pix = tid; pix < LP; pix += blockDim.x) {
    int y = pix / lhw, x = pix - y * lhw;
    // torch 'nearest': src = floor(dst * in / out)
    int sy = (int)floorf((float)y * ((float)mhw / (float)lhw)), sx = (int)floorf((float)x * ((float)mhw / (float)lhw));
    if (sy > mhw - 1) sy = mhw - 1;
    if (sx > mhw - 1) sx = mhw - 1;
    float v0 = __fdiv_rn(s_pool[sy * mhw + sx], mx0);
    float v1 = __fdiv_rn(s_pool[MP + sy * mhw + sx], mx1);
    bool m = (v0 > th) || (v1 > th);
    if (planes == 4) {
      float u0 = __fdiv_rn(s_pool[2 * MP + sy * mhw + sx], mx2);
      float u1 = __fdiv_rn(s_pool[3 * MP + sy * mhw + sx], mx3);
      m = m && !((u0 > th_sub) || (u1 > th_sub));
    }
    float mf = m ? 1.f : 0.f;
    for (int c = 0; c < C; ++c) {
      float a = xs[(size_t)c * LP + pix], b = xt[(size_t)c * LP + pix];
      xt[(size_t)c * LP + pix] = __fadd_rn(a, __fmul_rn(mf, __fsub_rn(b, a)));
    }
  }
}

int launch_local_blend(const float* lb_acc, int nslots, int map_hw, int lat_hw, int C, float th, float* latents, int nimg,
                       hipStream_t st, int planes, float th_sub) {
  if (planes != 2 && planes != 4) return -3;
  size_t lds = (size_t)(8 * map_hw * map_hw + 1024) * sizeof(float);
  local_blend_kernel<<<nimg, 256, lds, st>>>(lb_acc, nslots, map_hw, lat_hw, C, th, latents, planes, th_sub);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- edit-friendly DDPM (eta > 0)
// Reference: models/edit_friendly_ddm/inversion_utils.py -- sample_xts_from_x0 :31-55, inversion_forward_process :151-171,
// get_variance :91-98, reverse_step :179-208.  The per-step scalars are the reference's 0-dim fp32 torch ops, evaluated here on the host
// in the same order (this file is compiled without FMA contraction, host code included):
//   ab_p  = ab[t - ratio] (final_alpha_cumprod below 0)
//   var   = ((1 - ab_p) / (1 - ab_t)) * (1 - ab_t / ab_p)
//   dcoef = ((1 - ab_p) - eta * var) ** 0.5        sigma = eta * var ** 0.5
// out: [sa_t, sb_t, sa_p, dcoef, sigma, var]
void ef_step_scalars(float ab_t, float ab_p, float eta, float* out) {
  const float bt = 1.0f - ab_t, bp = 1.0f - ab_p;
  const float var = (bp / bt) * (1.0f - ab_t / ab_p);
  out[0] = sqrtf(ab_t);
  out[1] = sqrtf(bt);
  out[2] = sqrtf(ab_p);
  out[3] = sqrtf(bp - eta * var);
  out[4] = eta * sqrtf(var);
  out[5] = var;
}

// xts[1 + k][img] = x0[img] * sqrt(ab[t_k]) + noise[k][img] * sqrt(1 - ab[t_k])   (inversion_utils.py:53), k = 0 .. nlev-1 in draw order.
// lev: [nlev][2] = (sqrt(ab), sqrt(1 - ab)) per level.  xts[0] is not written.
__global__ void ef_sample_xts_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const float* __restrict__ lev, int nlev,
                                     size_t per_lev, float* __restrict__ xts) {
  const size_t total = (size_t)nlev * per_lev;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / per_lev);
    const size_t r = i - (size_t)k * per_lev;
    xts[per_lev + i] = __fadd_rn(__fmul_rn(x0[r], lev[2 * k]), __fmul_rn(noise[i], lev[2 * k + 1]));
  }
}
int launch_ef_sample_xts(const float* x0, const float* noise, const float* lev_dev, int nlev, size_t per_lev, float* xts, hipStream_t st) {
  size_t total = (size_t)nlev * per_lev;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  ef_sample_xts_kernel<<<blocks, 256, 0, st>>>(x0, noise, lev_dev, nlev, per_lev, xts);
  return (int)hipGetLastError();
}

// One step of inversion_forward_process (:151-171) for nimg images.  eps: [nimg][2][E] (uncond, cond) when cfg, else [nimg][1][E];
// xt = xts[idx+1], xprev = xts[idx] (read, then overwritten with the corrected value), z_out = zs[idx]:
//   e = eu + g * (ec - eu);  x0 = (xt - sb_t e) / sa_t;  mu = sa_p x0 + dcoef e;  z = (xprev - mu) / sigma;  xprev = mu + sigma z
// var_zero (the t = 0 step, ab_p == ab_t): z = 0 and xprev is left as sampled.  The reference divides by zero there and its xts[0] is
// NaN; nothing reads either (zs[0] is zeroed at :173-174).
__global__ void ef_noise_map_kernel(const float* __restrict__ eps, int cfg, float g, const float* __restrict__ xt, float* __restrict__ xprev,
                                    float* __restrict__ z_out, int nimg, size_t E, float sa_t, float sb_t, float sa_p, float dcoef, float sigma,
                                    int var_zero) {
  const size_t total = (size_t)nimg * E;
  const int rpi = cfg ? 2 : 1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / E, e_idx = i - img * E;
    const float eu = eps[(img * rpi) * E + e_idx];
    const float e = cfg ? __fadd_rn(eu, __fmul_rn(g, __fsub_rn(eps[(img * rpi + 1) * E + e_idx], eu))) : eu;
    const float x0 = __fdiv_rn(__fsub_rn(xt[i], __fmul_rn(sb_t, e)), sa_t);
    const float mu = __fadd_rn(__fmul_rn(sa_p, x0), __fmul_rn(dcoef, e));
    if (var_zero) {
      z_out[i] = 0.f;
    } else {
      const float z = __fdiv_rn(__fsub_rn(xprev[i], mu), sigma);
      z_out[i] = z;
      xprev[i] = __fadd_rn(mu, __fmul_rn(sigma, z));
    }
  }
}
int launch_ef_noise_map(const float* eps, int cfg, float g, const float* xt, float* xprev, float* z_out, int nimg, size_t E, const float* sc,
                        hipStream_t st) {
  size_t total = (size_t)nimg * E;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  ef_noise_map_kernel<<<blocks, 256, 0, st>>>(eps, cfg, g, xt, xprev, z_out, nimg, E, sc[0], sc[1], sc[2], sc[3], sc[4], sc[5] == 0.0f);
  return (int)hipGetLastError();
}

// One reverse_step (:179-208) after the per-row CFG of inversion_reverse_process (:254-258), P prompt rows per image:
// eps: [nimg][2P][E] (P uncond rows, then P cond rows), x / out: [nimg][P][E] (may alias), z: [nimg][E] (one noise map per image, expanded
// over its prompt rows as at :252), g0 / g1: the guidance scale of prompt row 0 / 1.
//   e = eu + g_r (ec - eu);  x0 = (x - sb_t e) / sa_t;  prev = sa_p x0 + dcoef e;  prev += sigma z   (only when eta > 0, :203-206)
__global__ void ef_reverse_step_kernel(const float* __restrict__ eps, const float* x, const float* __restrict__ z, int nimg, int P, size_t E,
                                       float g0, float g1, float sa_t, float sb_t, float sa_p, float dcoef, float sigma, int add_noise,
                                       float* out) {
  const size_t total = (size_t)nimg * P * E;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e_idx = i % E, ir = i / E;
    const int r = (int)(ir % P);
    const size_t img = ir / P;
    const float eu = eps[(img * 2 * P + r) * E + e_idx], ec = eps[(img * 2 * P + P + r) * E + e_idx];
    const float e = __fadd_rn(eu, __fmul_rn(r == 0 ? g0 : g1, __fsub_rn(ec, eu)));
    const float x0 = __fdiv_rn(__fsub_rn(x[i], __fmul_rn(sb_t, e)), sa_t);
    float prev = __fadd_rn(__fmul_rn(sa_p, x0), __fmul_rn(dcoef, e));
    if (add_noise) prev = __fadd_rn(prev, __fmul_rn(sigma, z[img * E + e_idx]));
    out[i] = prev;
  }
}
int launch_ef_reverse_step(const float* eps, const float* x, const float* z, int nimg, int P, size_t E, float g0, float g1, const float* sc,
                           int add_noise, float* out, hipStream_t st) {
  if (P != 1 && P != 2) return -3;
  size_t total = (size_t)nimg * P * E;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  ef_reverse_step_kernel<<<blocks, 256, 0, st>>>(eps, x, z, nimg, P, E, g0, g1, sc[0], sc[1], sc[2], sc[3], sc[4], add_noise, out);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- Blended Latent Diffusion
// Reference: run_editing_blended_latent_diffusion.py, BlendedLatnetDiffusion.edit_image :110-139 with diffusers' DDIMScheduler.step
// (eta = 0, no clipping) and add_noise.  One step for nimg images in one launch:
//   e      = eu + g * (ec - eu)                                        (:127-130)   eps: [nimg][2][E] (uncond, cond)
//   prev   = sa_p * ((x - sb_t * e) / sa_t) + sb_p * e                 (:133)       scheduler.step, t -> t - ratio
//   noised = sa_t * src + sb_t * noise                                 (:136-138)   add_noise at the step's OWN t (not t - ratio)
//   out    = prev * m + noised * (1 - m)                               (:139)       m = mask[img][e % HW]: broadcast over the channels
// The blend is evaluated as written (two multiplies and an add, 1 - m computed), every operation rounded on its own.  x / x_out may
// alias: a thread reads element i of x before it writes element i of x_out, and no other thread touches it.
__global__ void bld_step_kernel(const float* __restrict__ eps, const float* x, const float* __restrict__ src,
                                const float* __restrict__ noise, const float* __restrict__ mask, int nimg, size_t E, size_t HW, float g,
                                float sa_t, float sb_t, float sa_p, float sb_p, float* x_out) {
  const size_t total = (size_t)nimg * E;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / E, e_idx = i - img * E;
    const float eu = eps[(img * 2) * E + e_idx], ec = eps[(img * 2 + 1) * E + e_idx];
    const float e = __fadd_rn(eu, __fmul_rn(g, __fsub_rn(ec, eu)));
    const float prev = ddim_update(x[i], e, sa_t, sb_t, sa_p, sb_p);
    const float noised = __fadd_rn(__fmul_rn(sa_t, src[i]), __fmul_rn(sb_t, noise[i]));
    const float m = mask[img * HW + e_idx % HW];
    x_out[i] = __fadd_rn(__fmul_rn(prev, m), __fmul_rn(noised, __fsub_rn(1.0f, m)));
  }
}
int launch_bld_step(const float* eps, const float* x, const float* src, const float* noise, const float* mask, int nimg, size_t E, size_t HW,
                    float g, float a_t, float a_prev, float* x_out, hipStream_t st) {
  if (nimg <= 0 || E == 0 || HW == 0 || E % HW) return -3;
  // alphas_cumprod[t] ** 0.5 / (1 - alphas_cumprod[t]) ** 0.5 on 0-dim fp32 tensors: correctly rounded fp32 sqrt of fp32 operands
  const float sa_t = sqrtf(a_t), sb_t = sqrtf(1.0f - a_t), sa_p = sqrtf(a_prev), sb_p = sqrtf(1.0f - a_prev);
  size_t total = (size_t)nimg * E;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  bld_step_kernel<<<blocks, 256, 0, st>>>(eps, x, src, noise, mask, nimg, E, HW, g, sa_t, sb_t, sa_p, sb_p, x_out);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- Plug-and-Play
// Reference: run_editing_pnp.py, PNP.denoise_step :351-369 with diffusers' DDIMScheduler.step (eta = 0, no clipping).  One step for nimg
// images in one launch, eps [nimg][3][E] = (source row: unread, negative prompt, target prompt):
//   e    = eu + g * (ec - eu)                              (:364-365)
//   prev = sa_p * ((x - sb_t * e) / sa_t) + sb_p * e       (:368)        scheduler.step, t -> t - ratio
// rows_next (nullable) [nimg][3][E]: the next launch's input rows [src_next, prev, prev] (:353; src_next [nimg][E] is the source latent
// of the next level, NULL: row 0 is left alone).  x / x_out may alias (element i is read before it is written, by one thread).
__global__ void pnp_step_kernel(const float* __restrict__ eps, const float* x, const float* __restrict__ src_next, int nimg, size_t E, float g,
                                float sa_t, float sb_t, float sa_p, float sb_p, float* x_out, float* __restrict__ rows_next) {
  const size_t total = (size_t)nimg * E;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / E, e_idx = i - img * E;
    const float eu = eps[(img * 3 + 1) * E + e_idx], ec = eps[(img * 3 + 2) * E + e_idx];
    const float e = __fadd_rn(eu, __fmul_rn(g, __fsub_rn(ec, eu)));
    const float prev = ddim_update(x[i], e, sa_t, sb_t, sa_p, sb_p);
    x_out[i] = prev;
    if (rows_next) {
      float* r = rows_next + img * 3 * E + e_idx;
      if (src_next) r[0] = src_next[i];
      r[E] = prev;
      r[2 * E] = prev;
    }
  }
}
int launch_pnp_step(const float* eps, const float* x, const float* src_next, int nimg, size_t E, float g, float a_t, float a_prev, float* x_out,
                    float* rows_next, hipStream_t st) {
  if (nimg <= 0 || E == 0) return -3;
  // alpha_prod_t ** 0.5 / beta_prod_t ** 0.5 on 0-dim fp32 tensors: correctly rounded fp32 sqrt of fp32 operands
  const float sa_t = sqrtf(a_t), sb_t = sqrtf(1.0f - a_t), sa_p = sqrtf(a_prev), sb_p = sqrtf(1.0f - a_prev);
  size_t total = (size_t)nimg * E;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  pnp_step_kernel<<<blocks, 256, 0, st>>>(eps, x, src_next, nimg, E, g, sa_t, sb_t, sa_p, sb_p, x_out, rows_next);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- InstructPix2Pix, InstructDiffusion
// Reference: run_editing_instructpix2pix.py, CFGDenoiser :33-46 around k-diffusion's CompVisDenoiser, and sample_euler_ancestral (and
// run_editing_instructdiffusion.py :32-48: another third row and another combine, see ip2p_move; everything else below is shared).  One step
// for nimg images in one launch, eps [nimg][3][E] = (edit text + image, null text + image, null text + zero image), sc = the step's host
// scalars [sigma, sigma_down - sigma, sigma_up]:
//   den_k = z + eps_k * (-sigma)                                                  CompVisDenoiser.forward: input + eps * c_out
//   den   = den_2 + g_text * (den_0 - den_1) + g_image * (den_1 - den_2)          (:46), summed left to right
//   d     = (z - den) / sigma;   z' = z + d * (sigma_down - sigma);   z' = z' + noise * sigma_up   (only when sigma_next > 0)
// eps == NULL: no step, z' = z (the loop's first launch, which only forms the inputs).  in_next (nullable) [nimg][2][2 E]: the two distinct
// 8-channel inputs of the next launch, [z' * c_in_next | image] and [z' * c_in_next | 0] (only z is scaled, :43).  z / z_out may alias
// (element i is read before it is written, by one thread).  V = 4: E % 4 == 0 and every pointer 16-byte aligned.
struct Ip2pStepP {
  const float *eps, *z, *noise, *image;
  int nimg; size_t E;
  float g_text, g_image, neg_sigma, sigma, dt, up, c_in_next;
  int add_noise;
  float *z_out, *in_next;
};
// COMBINE: how the three denoised rows become one (the rest of the step is shared).
//   IP2P_CHAIN      run_editing_instructpix2pix.py :46, rows (text + image, null + image, null + zero image): a chain from the unconditional row
//                     den_2 + g_text * (den_0 - den_1) + g_image * (den_1 - den_2)
//   IP2P_SYMMETRIC  run_editing_instructdiffusion.py :46-48, rows (text + image, null + image, text + zero image): around the mean of the
//                   two single-condition rows
//                     0.5 * (den_1 + den_2) + g_text * (den_0 - den_1) + g_image * (den_0 - den_2)
// both summed left to right as the reference's expression is evaluated.
template <int COMBINE>
__device__ __forceinline__ float ip2p_move(const Ip2pStepP& p, float z, float e0, float e1, float e2, float nz) {
  const float d0 = __fadd_rn(z, __fmul_rn(e0, p.neg_sigma)), d1 = __fadd_rn(z, __fmul_rn(e1, p.neg_sigma)), d2 = __fadd_rn(z, __fmul_rn(e2, p.neg_sigma));
  float den;
  if (COMBINE == IP2P_CHAIN)
    den = __fadd_rn(__fadd_rn(d2, __fmul_rn(p.g_text, __fsub_rn(d0, d1))), __fmul_rn(p.g_image, __fsub_rn(d1, d2)));
  else
    den = __fadd_rn(__fadd_rn(__fmul_rn(0.5f, __fadd_rn(d1, d2)), __fmul_rn(p.g_text, __fsub_rn(d0, d1))), __fmul_rn(p.g_image, __fsub_rn(d0, d2)));
  const float d = __fdiv_rn(__fsub_rn(z, den), p.sigma);
  float zn = __fadd_rn(z, __fmul_rn(d, p.dt));
  if (p.add_noise) zn = __fadd_rn(zn, __fmul_rn(nz, p.up));
  return zn;
}
template <int V, int COMBINE>
__global__ void ip2p_step_kernel(const Ip2pStepP p) {
  const size_t EV = p.E / V, total = (size_t)p.nimg * EV;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / EV, e_idx = (i - img * EV) * V, at = img * p.E + e_idx;
    alignas(16) float z[V], zn[V], sc[V], im[V], zero[V];
    if (V == 4) *(float4*)z = *(const float4*)(p.z + at);
    else z[0] = p.z[at];
    if (p.eps) {
      alignas(16) float e0[V], e1[V], e2[V], nz[V];
      const float* e = p.eps + img * 3 * p.E + e_idx;
      if (V == 4) {
        *(float4*)e0 = *(const float4*)e; *(float4*)e1 = *(const float4*)(e + p.E); *(float4*)e2 = *(const float4*)(e + 2 * p.E);
        if (p.add_noise) *(float4*)nz = *(const float4*)(p.noise + at);
      } else {
        e0[0] = e[0]; e1[0] = e[p.E]; e2[0] = e[2 * p.E];
        if (p.add_noise) nz[0] = p.noise[at];
      }
      for (int k = 0; k < V; ++k) zn[k] = ip2p_move<COMBINE>(p, z[k], e0[k], e1[k], e2[k], p.add_noise ? nz[k] : 0.f);
    } else {
      for (int k = 0; k < V; ++k) zn[k] = z[k];
    }
    if (V == 4) *(float4*)(p.z_out + at) = *(const float4*)zn;
    else p.z_out[at] = zn[0];
    if (p.in_next) {
      for (int k = 0; k < V; ++k) { sc[k] = __fmul_rn(zn[k], p.c_in_next); zero[k] = 0.f; }
      float* r = p.in_next + img * 4 * p.E + e_idx;      // [row 0: z part, image part][row 1: z part, zero part]
      if (V == 4) {
        *(float4*)im = *(const float4*)(p.image + at);
        *(float4*)r = *(const float4*)sc; *(float4*)(r + p.E) = *(const float4*)im;
        *(float4*)(r + 2 * p.E) = *(const float4*)sc; *(float4*)(r + 3 * p.E) = *(const float4*)zero;
      } else {
        r[0] = sc[0]; r[p.E] = p.image[at]; r[2 * p.E] = sc[0]; r[3 * p.E] = 0.f;
      }
    }
  }
}
int launch_ip2p_step(int combine, const float* eps, const float* z, const float* noise, const float* image, int nimg, size_t E, float g_text,
                     float g_image, const float* sc, int add_noise, float c_in_next, float* z_out, float* in_next, hipStream_t st) {
  if (combine != IP2P_CHAIN && combine != IP2P_SYMMETRIC) return -3;
  if (nimg <= 0 || E == 0 || !z || !z_out || (in_next && !image) || (eps && !sc) || (eps && add_noise && !noise)) return -3;
  if (eps && !(sc[0] > 0.f)) return -3;
  Ip2pStepP p;
  p.eps = eps; p.z = z; p.noise = noise; p.image = image; p.nimg = nimg; p.E = E; p.g_text = g_text; p.g_image = g_image;
  p.sigma = eps ? sc[0] : 1.f; p.neg_sigma = -p.sigma; p.dt = eps ? sc[1] : 0.f; p.up = eps ? sc[2] : 0.f; p.c_in_next = c_in_next;
  p.add_noise = eps && add_noise ? 1 : 0; p.z_out = z_out; p.in_next = in_next;
  const uintptr_t al = (uintptr_t)eps | (uintptr_t)z | (uintptr_t)(p.add_noise ? noise : nullptr) | (uintptr_t)(in_next ? image : nullptr) |
                       (uintptr_t)z_out | (uintptr_t)in_next;
  const bool vec = E % 4 == 0 && al % 16 == 0;
  const size_t total = (size_t)nimg * (vec ? E / 4 : E);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  if (combine == IP2P_CHAIN) {
    if (vec) ip2p_step_kernel<4, IP2P_CHAIN><<<blocks, 256, 0, st>>>(p);
    else ip2p_step_kernel<1, IP2P_CHAIN><<<blocks, 256, 0, st>>>(p);
  } else {
    if (vec) ip2p_step_kernel<4, IP2P_SYMMETRIC><<<blocks, 256, 0, st>>>(p);
    else ip2p_step_kernel<1, IP2P_SYMMETRIC><<<blocks, 256, 0, st>>>(p);
  }
  return (int)hipGetLastError();
}

// BlendedLatnetDiffusion._read_mask (:164-173): PIL NEAREST resize of the [H][W] mask to [h][w], then `mask < 0.5 -> 0, else 1` (for
// uint8 values: non-zero -> 1).  PIL's nearest filter reads source pixel floor((i + 0.5) * H / h) (the centre of the destination pixel,
// scaled): in integers floor((2 i + 1) H / (2 h)), clamped to the image.
__global__ void bld_mask_kernel(const uint8_t* __restrict__ in, int n, int H, int W, int h, int w, float* __restrict__ out) {
  const size_t total = (size_t)n * h * w;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % w), yo = (int)(i / w % h);
    const size_t img = i / ((size_t)h * w);
    int ys = (int)(((long long)(2 * yo + 1) * H) / (2 * h)), xs = (int)(((long long)(2 * xo + 1) * W) / (2 * w));
    if (ys > H - 1) ys = H - 1;
    if (xs > W - 1) xs = W - 1;
    out[i] = in[(img * H + ys) * W + xs] != 0 ? 1.0f : 0.0f;
  }
}
int launch_bld_mask(const uint8_t* in, int n, int H, int W, int h, int w, float* out, hipStream_t st) {
  if (n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return -3;
  size_t total = (size_t)n * h * w;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  bld_mask_kernel<<<blocks, 256, 0, st>>>(in, n, H, W, h, w, out);
  return (int)hipGetLastError();
}

// Mask-guided MasaCtrl: the (h, w) source / target masks at one self-attention level, as the reference resizes them in every hooked
// forward (masactrl.py:149, :187: F.interpolate(mask, (H, W)), mode "nearest").  torch's nearest index is
// min(floor(dst * scale), in - 1) with scale = (float)in / out evaluated in fp32 (aten UpSampleNearest): the same expression here.
__global__ void masa_mask_level_kernel(const uint8_t* __restrict__ in, int n, int H, int W, int h, int w, uint8_t* __restrict__ out) {
  const size_t total = (size_t)n * h * w;
  const float sy = (float)H / (float)h, sx = (float)W / (float)w;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % w), yo = (int)(i / w % h);
    const size_t img = i / ((size_t)h * w);
    int ys = (int)floorf((float)yo * sy), xs = (int)floorf((float)xo * sx);
    if (ys > H - 1) ys = H - 1;
    if (xs > W - 1) xs = W - 1;
    out[i] = in[(img * H + ys) * W + xs] != 0 ? 1 : 0;
  }
}
int launch_masa_mask_level(const uint8_t* in, int n, int H, int W, int h, int w, uint8_t* out, hipStream_t st) {
  if (n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return -3;
  size_t total = (size_t)n * h * w;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  masa_mask_level_kernel<<<blocks, 256, 0, st>>>(in, n, H, W, h, w, out);
  return (int)hipGetLastError();
}
