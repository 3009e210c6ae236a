// libpnpi: C-ABI entry points + the static SD-1.x UNet / VAE graph executor and the device-resident DI / P2P loops.
// See include/pnpi.h for the reference interface each entry point replaces.
// One translation unit in ten files: this one (error helpers, the C ABI: context life cycle, level-1 operators, the CLIP text encoder,
// kernel-level test hooks) includes, in order,
//   api_weights.inc   weight slots of the packed arena and the model builder
//   api_graph.inc     profiling records, activation tape, op wrappers, ResNet / transformer blocks, unet_fwd
//   api_backward.inc  reverse walk over the tape (gradient w.r.t. the unconditional embedding)
//   api_vae.inc       AutoencoderKL encoder / decoder graph
//   api_ctrl.inc      per-loop text K / V cache, controller descriptor -> device tables
//   api_clipscore.inc CLIP similarity: the image tower attached to a context, projections, preprocessing, score
//   api_structdist.inc DINO structure distance: the ViT attached to a context, preprocessing, keys, the fused distance
//   api_lpips.inc     LPIPS: SqueezeNet 1.1 features attached to a context, the seven taps, the fused tap distance
//   api_loops.inc     (last) the loop scaffold and the level-2 loops: DDIM / direct inversion, edit loops, edit-friendly DDPM, null-text
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <string>

#include "model.h"
#include "tuning.h"

// ---------------------------------------------------------------------------------------------------- error helpers
// explicit status + message
static int fail(pnpi_ctx* c, int status, const char* what) {
  c->err = what;
  return status;
}
// raw launch result: > 0 is a hipError_t, < 0 an argument/shape rejection by a launch wrapper
static int fail_launch(pnpi_ctx* c, int code, const char* what) {
  char buf[640];
  if (code > 0) {
    snprintf(buf, sizeof(buf), "HIP error %d (%s) in %s", code, hipGetErrorString((hipError_t)code), what);
    c->err = buf;
    return PNPI_EHIP;
  }
  snprintf(buf, sizeof(buf), "launch wrapper rejected arguments (code %d) in %s", code, what);
  c->err = buf;
  return PNPI_ESHAPE;
}
// CK: raw launch codes.  CKP: propagate an already-mapped pnpi_status (message already set).
#define CK(x)                                 \
  do {                                        \
    int _r = (x);                             \
    if (_r) return fail_launch(c, _r, #x);    \
  } while (0)
#define CKP(x)                \
  do {                        \
    int _r = (x);             \
    if (_r) return _r;        \
  } while (0)
#define CKH(x)                                     \
  do {                                             \
    hipError_t _e = (x);                           \
    if (_e != hipSuccess) return fail_launch(c, (int)_e, #x); \
  } while (0)

#include "api_weights.inc"
#include "api_graph.inc"
#include "api_backward.inc"
#include "api_vae.inc"
#include "api_ctrl.inc"

// ---------------------------------------------------------------------------------------------------- C ABI
extern "C" {

void pnpi_config_sd1(pnpi_model_config* g) {
  memset(g, 0, sizeof(*g));
  g->in_channels = 4; g->out_channels = 4; g->n_blocks = 4;
  int boc[4] = {320, 640, 1280, 1280}, att[4] = {1, 1, 1, 0}, vb[4] = {128, 256, 512, 512};
  for (int i = 0; i < 4; ++i) { g->block_out_channels[i] = boc[i]; g->block_has_attn[i] = att[i]; g->vae_block_out_channels[i] = vb[i]; }
  g->layers_per_block = 2; g->heads = 8; g->cross_dim = 768; g->ctx_len = 77; g->sample_size = 64; g->norm_groups = 32;
  g->n_train_timesteps = 1000; g->vae_in_channels = 3; g->vae_latent_channels = 4; g->vae_n_blocks = 4;
  g->vae_layers_per_block = 2; g->vae_norm_groups = 32;
  g->clip_layers = 12; g->clip_heads = 12; g->clip_intermediate = 3072; g->clip_vocab = 49408;   /* CLIP ViT-L/14 text model */
}

const char* pnpi_last_error(const pnpi_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

static int validate_config(pnpi_ctx* c) {
  const pnpi_model_config& g = c->cfg;
  if (g.n_blocks < 2 || g.n_blocks > 4 || g.vae_n_blocks < 2 || g.vae_n_blocks > 4) return fail(c, PNPI_ESHAPE, "n_blocks must be 2..4");
  for (int i = 0; i < g.n_blocks; ++i) {
    int ch = g.block_out_channels[i];
    if (ch % g.norm_groups || ch % 8 || ch % g.heads) return fail(c, PNPI_ESHAPE, "block_out_channels must divide by groups, heads and 8");
    int dh = ch / g.heads;
    if (g.block_has_attn[i] && (dh % 4 || dh > 160)) return fail(c, PNPI_ESHAPE, "head dim must be a multiple of 4 and <= 160");
  }
  for (int i = 0; i < g.vae_n_blocks; ++i)
    if (g.vae_block_out_channels[i] % g.vae_norm_groups || g.vae_block_out_channels[i] % 8) return fail(c, PNPI_ESHAPE, "vae channels");
  if (g.cross_dim % 8 || g.ctx_len > 96 || g.in_channels > 8 || g.vae_latent_channels > 4 || g.vae_in_channels != 3)
    return fail(c, PNPI_ESHAPE, "cross_dim/ctx_len/in_channels unsupported");
  if (g.sample_size % (1 << (g.n_blocks - 1))) return fail(c, PNPI_ESHAPE, "sample_size must divide by 2^(n_blocks-1)");
  if (g.block_out_channels[0] % 2) return fail(c, PNPI_ESHAPE, "C0 must be even");
  if (g.clip_layers < 0 || g.clip_layers > 48) return fail(c, PNPI_ESHAPE, "clip_layers out of range");
  if (g.clip_layers > 0) {
    if (g.clip_heads <= 0 || g.cross_dim % g.clip_heads) return fail(c, PNPI_ESHAPE, "cross_dim must divide by clip_heads");
    const int dh = g.cross_dim / g.clip_heads;
    if (dh % 32 || dh > 160) return fail(c, PNPI_ESHAPE, "CLIP head dim must be a multiple of 32 and <= 160");
    if (g.clip_intermediate <= 0 || g.clip_intermediate % 8 || g.clip_vocab <= 0) return fail(c, PNPI_ESHAPE, "clip_intermediate / clip_vocab invalid");
  }
  return 0;
}

static int clip_fwd(pnpi_ctx* c, const int* ids, int n, float* out, half_t** y16_out = nullptr);
static void clipv_free(pnpi_ctx* c);
static void dino_free(pnpi_ctx* c);
static void lpips_free(pnpi_ctx* c);

static int create_impl(pnpi_ctx** out, const pnpi_model_config* cfg, int device, void* hip_stream, int max_unet_rows, int max_vae_images, pnpi_ctx* parent);
int pnpi_create(pnpi_ctx** out, const pnpi_model_config* cfg, int device, void* hip_stream, int max_unet_rows, int max_vae_images) {
  if (!out || !cfg) return PNPI_EINVAL;
  return create_impl(out, cfg, device, hip_stream, max_unet_rows, max_vae_images, nullptr);
}
// A further context on the SAME packed weights: the new context borrows the parent's weight arena (read-only from here on) instead of
// holding a copy -- several images in flight on one GPU (own stream, own workspaces, own caches) then share one 1.9 GB arena in the
// Infinity Cache / L2 instead of competing with N copies of it.  The parent must outlive the child and its weights must not be
// reloaded while children exist (a child refuses pnpi_load_weights).
int pnpi_create_shared(pnpi_ctx** out, pnpi_ctx* parent, void* hip_stream, int max_unet_rows, int max_vae_images) {
  if (!out || !parent) return PNPI_EINVAL;
  if (parent->warena_borrowed) return fail(parent, PNPI_ESTATE, "pnpi_create_shared: the parent itself borrows its weights; share from the owner");
  return create_impl(out, &parent->cfg, parent->device, hip_stream, max_unet_rows, max_vae_images, parent);
}
// dry runs of every graph at the context's row limits: the peaks of the two activation workspaces
static int size_workspaces(pnpi_ctx* c, size_t* ppeak, size_t* tpeak) {
  DryScope dry(c);
  auto fresh = [c]() { c->persist = Bump(); c->temp = Bump(); };
  auto keep = [&]() { *ppeak = std::max(*ppeak, c->persist.peak); *tpeak = std::max(*tpeak, c->temp.peak); };
  *ppeak = *tpeak = 0;
  if (c->max_rows > 0) {
    fresh();
    UNetCall k; k.rows = c->max_rows;
    CKP(unet_fwd(c, k));
    keep();
  }
  if (!c->clip.layers.empty()) {
    fresh();
    CKP(clip_fwd(c, nullptr, c->rows_ident_n, nullptr));
    keep();
  }
  if (c->max_vae > 0) {
    const int S = c->cfg.sample_size, F = 1 << (c->cfg.vae_n_blocks - 1);
    fresh();
    (void)palloc(c, (size_t)c->max_vae * S * F * S * F * 8);
    CKP(vae_encode_fwd(c, nullptr, c->max_vae, S * F, S * F, nullptr));
    keep();
    fresh();
    (void)palloc(c, (size_t)c->max_vae * S * S * 8);
    (void)c->persist.alloc((size_t)c->max_vae * 3 * S * F * S * F * sizeof(float));
    CKP(vae_decode_fwd(c, nullptr, c->max_vae, S, S, nullptr));
    keep();
  }
  return 0;
}
static int create_impl(pnpi_ctx** out, const pnpi_model_config* cfg, int device, void* hip_stream, int max_unet_rows, int max_vae_images, pnpi_ctx* parent) {
  pnpi_ctx* c = new pnpi_ctx();
  *out = c;
  c->cfg = *cfg; c->device = device; c->st = (hipStream_t)hip_stream; c->max_rows = max_unet_rows; c->max_vae = max_vae_images;
  c->sched_set = false; c->final_alpha = 0.f;
  c->splitk_ws = nullptr; c->gn_partial = nullptr; c->temb_table = nullptr;
  memset(&c->ctr, 0, sizeof(c->ctr));
  CKP(validate_config(c));
  CKH(hipSetDevice(device));
  CK(igemm_init());
  const pnpi_model_config& g = c->cfg;
  // pass 1: measure the weight arena; pass 2: real pointers
  build_model(c);
  const size_t wbytes = align_up(c->warena.peak + 4096, 4096);
  if (parent) {
    if (parent->warena.cap != wbytes) return fail(c, PNPI_ESTATE, "pnpi_create_shared: the parent's weight arena has another size");
    c->warena.base = parent->warena.base; c->warena_borrowed = true;
    c->warena_ref = parent->warena_ref; c->warena_ref->refs.fetch_add(1);      // the arena lives until its last user is destroyed
  } else {
    CKH(hipMalloc((void**)&c->warena.base, wbytes));
    c->warena_ref = new pnpi_ctx::ArenaRef{c->warena.base, {1}};
    CKH(hipMemsetAsync(c->warena.base, 0, wbytes, c->st));
  }
  c->warena.cap = wbytes; c->warena.reset(); c->warena.peak = 0;
  build_model(c);
  if (parent)      // the same deterministic layout: every slot points at the parent's packed tensor and is loaded iff the parent's is
    for (auto& kv : c->slots) { auto it = parent->slots.find(kv.first); kv.second.loaded = it != parent->slots.end() && it->second.loaded; }
  else
    for (const pnpi_ctx::AugBias& ab : c->aug_biases) {      // constants of the arena (not part of any checkpoint): the memset above left zeros
      std::vector<float> hb((size_t)3 * ab.heads * ab.Dp, 0.f);
      for (int part = 1; part < 3; ++part)
        for (int hh = 0; hh < ab.heads; ++hh) hb[(size_t)part * ab.heads * ab.Dp + hh * ab.Dp + ab.dh] = 1.f;
      CKH(hipMemcpyAsync(ab.p, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice, c->st));
      CKH(hipStreamSynchronize(c->st));                        // hb is a temporary
    }
  // small persistent buffers
  const int C0 = g.block_out_channels[0], TE = 4 * C0;
  c->splitk_bytes = ((size_t)96 << 20) + (size_t)(max_unet_rows > 12 ? max_unet_rows - 12 : 0) * ((size_t)8 << 20);   // grows with the rows per launch
  CKH(hipMalloc((void**)&c->splitk_ws, c->splitk_bytes));
  size_t gnp = (size_t)(max_unet_rows > max_vae_images ? max_unet_rows : max_vae_images) * (128 * 64 * 2 + 4096 * 2) * sizeof(float);
  CKH(hipMalloc((void**)&c->gn_partial, gnp));
  c->gn_partial_floats = gnp / sizeof(float);
  CKH(hipMalloc((void**)&c->temb_h, TE * sizeof(float)));
  CKH(hipMalloc((void**)&c->temb_row, C0 * sizeof(float)));
  CKH(hipMalloc((void**)&c->temb_emb, TE * sizeof(float)));
  CKH(hipMalloc((void**)&c->bias_scratch, (size_t)c->unet.temb_total * sizeof(float)));
  if (max_unet_rows > 0) {
    // per-timestep (conv1 bias + time embedding) table: [n_train][temb_total] fp32 (81 MB for SD-1.x), rows filled on first use
    CKH(hipMalloc((void**)&c->bias_tab, (size_t)g.n_train_timesteps * c->unet.temb_total * sizeof(float)));
    c->bias_valid.assign(g.n_train_timesteps, 0);
    c->tkv.cap = text_kv_bytes(c, max_unet_rows);
    CKH(hipMalloc((void**)&c->tkv.base, c->tkv.cap));
    CKH(hipMemset(c->tkv.base, 0, c->tkv.cap));   // (text_kv_precompute clears each V^T block again: the layout depends on the row count)
  }
  // sinusoidal timestep table, get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0), fp64 -> fp32
  // (my_diffusers/models/embeddings.py:21-60)
  {
    const int half = C0 / 2;
    std::vector<float> tab((size_t)g.n_train_timesteps * C0);
    for (int t = 0; t < g.n_train_timesteps; ++t)
      for (int i = 0; i < half; ++i) {
        double e = exp(-log(10000.0) * (double)i / (double)half);
        double a = (double)t * e;
        tab[(size_t)t * C0 + i] = (float)cos(a);          // flipped: cos first
        tab[(size_t)t * C0 + half + i] = (float)sin(a);
      }
    CKH(hipMalloc((void**)&c->temb_table, tab.size() * sizeof(float)));
    CKH(hipMemcpy(c->temb_table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  // controller / loop arena
  {
    const size_t E = (size_t)g.in_channels * g.sample_size * g.sample_size;
    size_t cap = ((size_t)8 << 20) + (size_t)max_unet_rows * E * sizeof(float) * 8 +
                 (size_t)max_unet_rows * (96 * 96 * 2 + 64 * 2 * 96 * 4 * 2 + (size_t)c->unet.lb_nslots * 4 * c->unet.lb_tokens * 4);
    CKH(hipMalloc((void**)&c->ctrl_arena.base, cap));
    c->ctrl_arena.cap = cap;
  }
  {
    c->rows_ident_n = max_unet_rows > 8 ? max_unet_rows : 8;
    std::vector<int> idt((size_t)c->rows_ident_n * 4);
    for (int r = 0; r < c->rows_ident_n; ++r) idt[4 * r] = idt[4 * r + 1] = idt[4 * r + 2] = idt[4 * r + 3] = r;
    CKH(hipMalloc((void**)&c->rows_ident, idt.size() * sizeof(int)));
    CKH(hipMemcpy(c->rows_ident, idt.data(), idt.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  size_t ppeak, tpeak;
  CKP(size_workspaces(c, &ppeak, &tpeak));
  ppeak = align_up(ppeak + (1 << 20), 4096); tpeak = align_up(tpeak + (1 << 20), 4096);
  CKH(hipMalloc((void**)&c->persist.base, ppeak));
  CKH(hipMalloc((void**)&c->temp.base, tpeak));
  c->persist.cap = ppeak; c->temp.cap = tpeak; c->persist.reset(); c->temp.reset();
  memset(&c->ctr, 0, sizeof(c->ctr));
  // identity attention-row table for the controller-free path
  CKP(setup_ctrl(c, nullptr, 0, max_unet_rows > 0 ? max_unet_rows : 1));
  CKH(hipStreamSynchronize(c->st));
  return 0;
}

void pnpi_destroy(pnpi_ctx* c) {
  if (!c) return;
  (void)hipStreamSynchronize(c->st);
  // the weight arena is shared with the contexts pnpi_create_shared made from this one (or borrowed from the one this was made from):
  // whoever is destroyed last frees it -- destroying the owner first does not pull the weights from under a running child
  void* arena = nullptr;
  if (c->warena_ref && c->warena_ref->refs.fetch_sub(1) == 1) { arena = c->warena_ref->base; delete c->warena_ref; }
  void* bufs[] = {arena, c->persist.base, c->temp.base, c->ctrl_arena.base, c->splitk_ws, c->gn_partial, c->gn_bwd_ws,
                  c->temb_table, c->temb_row, c->temb_h, c->temb_emb, c->bias_scratch, c->bias_tab, c->tkv.base, c->rows_ident, c->mm.base, c->mm.stage};
  for (void* b : bufs) (void)hipFree(b);
  if (c->tape) {
    (void)hipFree(c->tape->garena.base); (void)hipFree(c->tape->d_ctx); (void)hipFree(c->tape->attn_scratch);
    for (auto& kv : c->tape->wd) (void)hipFree(kv.second);
    delete c->tape;
  }
  clipv_free(c);
  dino_free(c);
  lpips_free(c);
  (void)hipFree(c->ss_ws);
  (void)hipFree(c->lp_ws);
  delete c;
}

static void invalidate_derived(pnpi_ctx* c) {     // caches of functions of the weights
  std::fill(c->bias_valid.begin(), c->bias_valid.end(), 0);
  c->tkv.rows = 0;
  if (c->tape) { for (auto& kv : c->tape->wd) (void)hipFree(kv.second); c->tape->wd.clear(); }     // dgrad repacks of the old weights
}

int pnpi_load_weights(pnpi_ctx* c, const pnpi_named_tensor* ts, int n) {
  if (!c || !ts) return PNPI_EINVAL;
  if (c->warena_borrowed) return fail(c, PNPI_ESTATE, "this context borrows its weights (pnpi_create_shared): load them into the owning context");
  invalidate_derived(c);
  bool fold_src = false;
  for (int i = 0; i < n; ++i) {
    const pnpi_named_tensor& t = ts[i];
    std::string name = t.name;
    // diffusers 0.3-0.10 register the stride-2 conv twice ("conv" and "Conv2d_0"): accept either spelling
    size_t pos = name.find(".downsamplers.0.Conv2d_0.");
    if (pos != std::string::npos) name.replace(pos, strlen(".downsamplers.0.Conv2d_0."), ".downsamplers.0.conv.");
    if (name.compare(0, 16, "clip.text_model.") == 0) name = "clip." + name.substr(16);   // transformers < 5 key spelling
    auto it = c->slots.find(name);
    if (it == c->slots.end()) continue;  // unknown keys are ignored (e.g. buffers)
    Slot& s = it->second;
    size_t numel = 1;
    for (int d = 0; d < t.ndim; ++d) numel *= (size_t)t.shape[d];
    if (s.kind == 0) {
      if (numel != (size_t)s.rows * s.cols * s.taps) { c->err = "shape mismatch for " + name; return PNPI_ESHAPE; }
      CK(launch_repack_matrix(t.data, t.dtype, s.rows, s.cols, s.taps, (half_t*)s.dst, s.dst_ld, s.cin_pad, s.row0, s.dh, s.Dp, c->st,
                              s.ilv_half));
    } else {
      if (numel != (size_t)s.n) { c->err = "shape mismatch for " + name; return PNPI_ESHAPE; }
      CK(launch_repack_vec(t.data, t.dtype, s.n, (float*)s.dst, c->st, s.ilv_half));
    }
    s.loaded = true;
    if (!fold_src && ff_fold_source(c, name)) { fold_src = true; c->warena_ref->ff_fold_ready = false; }
  }
  if (fold_src) CK(build_ff_fold(c));     // the folded ff2 + proj_out weights follow their sources (same stream: ordered behind the repacks)
  return 0;
}

int pnpi_missing_weights(const pnpi_ctx* c, char* names_out, size_t cap) {
  int missing = 0;
  size_t used = 0;
  if (names_out && cap) names_out[0] = 0;
  for (auto& kv : c->slots)
    if (!kv.second.loaded && kv.first.compare(0, 5, "clip.") != 0 && kv.first.compare(0, 6, "clipv.") != 0 && kv.first.compare(0, 5, "dino.") != 0 && kv.first.compare(0, 6, "lpips.") != 0) {   // the text encoder reports through pnpi_text_encode, the image tower through pnpi_clip_*, the DINO ViT through pnpi_dino_*, LPIPS through pnpi_lpips*
      ++missing;
      if (names_out && used + kv.first.size() + 2 < cap) {
        memcpy(names_out + used, kv.first.c_str(), kv.first.size());
        used += kv.first.size();
        names_out[used++] = '\n';
        names_out[used] = 0;
      }
    }
  return missing;
}

int pnpi_weight_arena(pnpi_ctx* c, void** ptr, size_t* bytes) {
  if (!c || !ptr || !bytes) return PNPI_EINVAL;
  *ptr = c->warena.base; *bytes = c->warena.cap;
  // after a broadcast every slot of the receiving ranks is populated
  return 0;
}

int pnpi_mark_all_loaded(pnpi_ctx* c) {
  invalidate_derived(c);            // the arena was just overwritten by the broadcast
  for (auto& kv : c->slots)
    if (kv.first.compare(0, 6, "clipv.") != 0 && kv.first.compare(0, 5, "dino.") != 0 && kv.first.compare(0, 6, "lpips.") != 0) kv.second.loaded = true;      // the image tower, the DINO ViT and the LPIPS network are no part of the arena
  CK(build_ff_fold(c));             // derived after the broadcast, from the weights it delivered (a borrowing context leaves it to the owner)
  return 0;
}

int pnpi_set_scheduler(pnpi_ctx* c, const float* ac, int n_train, float final_alpha) {
  if (!c || !ac || n_train != c->cfg.n_train_timesteps) return PNPI_EINVAL;
  c->ac.assign(ac, ac + n_train);
  c->final_alpha = final_alpha;
  c->sched_set = true;
  return 0;
}

int pnpi_get_counters(const pnpi_ctx* c, pnpi_counters* out) { if (!c || !out) return PNPI_EINVAL; *out = c->ctr; return 0; }
int pnpi_reset_counters(pnpi_ctx* c) { if (!c) return PNPI_EINVAL; memset(&c->ctr, 0, sizeof(c->ctr)); return 0; }

// Matrix-pipe clock calibration (bench.py's `clock` object): every SIMD of the chip issues v_mfma_f32_32x32x16_f16 back to back on register
// operands with pseudo-random fp16 values (two waves per SIMD, four independent accumulators each): 32 matrix-pipe cycles per instruction
// (MI355X_MICROARCH.md, "Per-instruction cycle constants"), so cycles / elapsed = the clock the part holds under a pure MFMA load.
__global__ void __launch_bounds__(512, 2) mfma_clock_kernel(int iters, float* sink) {
  const int lane = threadIdx.x & 63;
  unsigned h = (unsigned)(blockIdx.x * 512 + threadIdx.x) * 2654435761u;
  half8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13;
    a[j] = (half_t)((float)(h & 0xffff) * (2.f / 65536.f) - 1.f);
    b[j] = (half_t)((float)(h >> 16) * (2.f / 65536.f) - 1.f);
  }
  floatx16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
  for (int t = 0; t < iters; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = mfma32(a, b, acc[i]);
  }
  float s_ = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) s_ += acc[i][0] + acc[i][15];
  if (s_ == 12345.678f) sink[blockIdx.x * 64 + lane] = s_;      // never true in practice: keeps the accumulators live
}

int pnpi_clock_probe(pnpi_ctx* c, int iters, float* ghz_out, float* ms_out) {
  if (!c || iters <= 0 || iters > (1 << 24) || !ghz_out) return PNPI_EINVAL;
  int dev = 0, cus = 0;
  CKH(hipGetDevice(&dev));
  CKH(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  hipEvent_t e0, e1;
  CKH(hipEventCreate(&e0));
  CKH(hipEventCreate(&e1));
  CKH(hipEventRecord(e0, c->st));
  hipLaunchKernelGGL(mfma_clock_kernel, dim3(cus), dim3(512), 0, c->st, iters, (float*)c->gn_partial);
  CKH(hipGetLastError());
  CKH(hipEventRecord(e1, c->st));
  CKH(hipEventSynchronize(e1));
  float ms = 0.f;
  CKH(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  // one workgroup of 8 waves per CU = 2 waves per SIMD, 16 MFMAs per wave and iteration, 32 pipe cycles each
  *ghz_out = ms > 0.f ? (float)(2.0 * 16.0 * 32.0 * (double)iters / ((double)ms * 1e6)) : 0.f;
  if (ms_out) *ms_out = ms;
  return 0;
}

int pnpi_profile_begin(pnpi_ctx* c) {
  if (!c) return PNPI_EINVAL;
  CKH(hipStreamSynchronize(c->st));
  c->prof.clear();
  c->prof_on = true;
  return 0;
}
int pnpi_profile_end(pnpi_ctx* c, pnpi_kernel_stats* out) {
  if (!c || !out) return PNPI_EINVAL;
  c->prof_on = false;
  CKH(hipStreamSynchronize(c->st));
  if (const char* path = getenv("PNPI_PROFILE_DUMP")) {   // per-launch records for tools/ (class, M, N, K, ksize, us)
    if (FILE* f = fopen(path, "w")) {
      fprintf(f, "cls,M,N,K,ksize,us,flops,cfg,split,kernel,bytes\n");
      for (ProfRec& r : c->prof) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.a, r.b);
        char kn[96] = "-";     // the kernel template a rocprofv3 kernel trace shows for this launch
        if (r.geom[0] && r.geom[6] == -1) snprintf(kn, sizeof kn, "igemm_pp_kernel<%d %d %d %d %d>", r.geom[0], r.geom[1], r.geom[2], r.geom[3], r.geom[4]);
        else if (r.geom[0]) snprintf(kn, sizeof kn, "igemm_dma_kernel<%d %d %d %d %d %d %d>", r.geom[0], r.geom[1], r.geom[2], r.geom[3], r.geom[4], r.geom[5], r.geom[6]);
        else if (r.cfg >= 0) snprintf(kn, sizeof kn, "igemm_kernel");
        fprintf(f, "%d,%d,%d,%d,%d,%.3f,%.0f,%d,%d,%s,%.0f\n", r.cls, r.M, r.N, r.K, r.ksize, ms * 1e3, r.flops, r.cfg, r.split, kn, r.bytes);
      }
      fclose(f);
    }
  }
  memset(out, 0, sizeof(pnpi_kernel_stats) * PNPI_KC_COUNT);
  for (ProfRec& r : c->prof) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    if (r.cls >= 0 && r.cls < PNPI_KC_COUNT) {
      out[r.cls].launches += 1; out[r.cls].total_ms += ms; out[r.cls].flops += r.flops; out[r.cls].bytes += r.bytes;
    }
    (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
  }
  c->prof.clear();
  return 0;
}

static bool is_clipv_slot(const std::string& name) { return name.compare(0, 6, "clipv.") == 0; }      // image tower + projections (pnpi_clipv_attach)
static bool is_clip_slot(const std::string& name) { return name.compare(0, 5, "clip.") == 0 || is_clipv_slot(name); }
static bool is_dino_slot(const std::string& name) { return name.compare(0, 5, "dino.") == 0 || name.compare(0, 6, "lpips.") == 0; }      // DINO ViT (pnpi_dino_attach), LPIPS network (pnpi_lpips_attach)
static int check_ready(pnpi_ctx* c) {   // UNet / VAE entry points: the text encoder's weights are optional for them
  for (auto& kv : c->slots)
    if (!kv.second.loaded && !is_clip_slot(kv.first) && !is_dino_slot(kv.first)) { c->err = "weights not loaded: " + kv.first; return PNPI_ESTATE; }
  return 0;
}
// Level-2 entry points (whole loops in one call): they drive unet_fwd directly with kernel descriptors, so a host attention callback
// left installed by an earlier level-1 forward would silently replace the descriptor edits (and run during inversion).  Fail loudly.
static int check_loop_ready(pnpi_ctx* c) {
  CKP(check_ready(c));
  if (c->attn_cb) return fail(c, PNPI_ESTATE, "an attention callback is installed (pnpi_set_attention_callback): the loop entry points take kernel "
                                               "descriptors only -- remove the callback first (callback controllers run through pnpi_unet_forward)");
  return 0;
}
static int check_clip_ready(pnpi_ctx* c) {
  if (c->clip.layers.empty()) return fail(c, PNPI_ESTATE, "this context was built without a text encoder (clip_layers = 0)");
  for (auto& kv : c->slots)
    if (!kv.second.loaded && is_clip_slot(kv.first) && !is_clipv_slot(kv.first)) { c->err = "weights not loaded: " + kv.first; return PNPI_ESTATE; }
  return 0;
}

int pnpi_set_attention_callback(pnpi_ctx* c, pnpi_attn_callback cb, void* user, float* attn_buf, size_t attn_buf_bytes) {
  if (!c || (cb && (!attn_buf || !attn_buf_bytes))) return PNPI_EINVAL;
  c->attn_cb = cb; c->attn_cb_user = user; c->attn_buf = cb ? attn_buf : nullptr; c->attn_buf_bytes = cb ? attn_buf_bytes : 0;
  return 0;
}

int pnpi_text_kv_precompute(pnpi_ctx* c, const float* context, int rows) {
  if (!c || !context) return PNPI_EINVAL;
  CKP(check_ready(c));
  return text_kv_precompute(c, context, rows);
}

// the level-1 forwards' call: context == NULL reads the text K/V cache, which must hold this row count
static int level1_call(pnpi_ctx* c, const float* latents, int rows, const float* context, float* eps_out, UNetCall& k) {
  if (!context && c->tkv.rows != rows) return fail(c, PNPI_ESTATE, "context is NULL: call pnpi_text_kv_precompute for this row count first");
  k.latents = latents; k.rows = rows; k.context = context; k.cached_kv = context == nullptr; k.eps_out = eps_out;
  return 0;
}
int pnpi_unet_forward(pnpi_ctx* c, const float* latents, int rows, int rows_per_image, int t, const float* context,
                      const pnpi_ctrl_desc* ctrl_host, int cur_step, float* eps_out) {
  if (!c || !latents || !eps_out) return PNPI_EINVAL;
  CKP(check_ready(c));
  UNetCall k; CKP(level1_call(c, latents, rows, context, eps_out, k));
  if (c->attn_cb && (!context || ctrl_host)) return fail(c, PNPI_EINVAL, "attention callback: pass the context, and no controller descriptor");
  if (ctrl_host) {
    if (rows_per_image != 4 || rows % 4) return fail(c, PNPI_EINVAL, "controllers need rows_per_image == 4");
    if (cur_step == 0 || c->cd.nimg != rows / 4) CKP(setup_ctrl(c, ctrl_host, rows / 4, rows));
  } else if (c->cd.any_edit || c->cd.nimg != 0) {
    CKP(setup_ctrl(c, nullptr, 0, c->max_rows));
  }
  k.t = t; k.use_ctrl = ctrl_host != nullptr; k.cur_step = cur_step;
  return unet_fwd(c, k);
}

/* LocalBlend step_callback for level-1 drivers (attention_control.py:253-256): latents [nimg][2][4][h][w] in place */
int pnpi_local_blend(pnpi_ctx* c, float* latents, int nimg, int step_index) {
  if (!c || !latents || nimg != c->cd.nimg) return PNPI_EINVAL;
  return apply_local_blend(c, latents, step_index);
}

int pnpi_vae_encode(pnpi_ctx* c, const float* x, int n, int height, int width, float* mean_out) {
  if (!c || !x || !mean_out || n <= 0 || n > c->max_vae) return PNPI_EINVAL;
  CKP(check_ready(c));
  c->persist.reset(); c->temp.reset();
  half_t* xin = palloc(c, (size_t)n * height * width * 8);
  CK(launch_nchw_f32_to_nhwc_f16(x, n, 3, height * width, 8, xin, c->st));
  CKP(vae_encode_fwd(c, xin, n, height, width, mean_out));
  c->ctr.vae_encodes += n;
  if (c->persist.overflow || c->temp.overflow) return fail(c, PNPI_ENOMEM, "workspace overflow (vae encode)");
  return 0;
}

int pnpi_image2latent(pnpi_ctx* c, const uint8_t* img, int n, int height, int width, float* z_out) {
  if (!c || !img || !z_out || n <= 0 || n > c->max_vae) return PNPI_EINVAL;
  CKP(check_ready(c));
  c->persist.reset(); c->temp.reset();
  half_t* xin = palloc(c, (size_t)n * height * width * 8);
  CK(launch_img_u8_to_nhwc(img, n, height * width, 8, xin, c->st));
  CKP(vae_encode_fwd(c, xin, n, height, width, z_out));
  const int F = 1 << (c->cfg.vae_n_blocks - 1);
  size_t ne = (size_t)n * c->cfg.vae_latent_channels * (height / F) * (width / F);
  CK(launch_scale_f32(z_out, ne, 0.18215f, z_out, c->st));
  c->ctr.vae_encodes += n;
  if (c->persist.overflow || c->temp.overflow) return fail(c, PNPI_ENOMEM, "workspace overflow (vae encode)");
  return 0;
}

static int decode_common(pnpi_ctx* c, const float* z, int n, int lh, int lw, float zscale, float* sample_out, uint8_t* u8_out) {
  CKP(check_ready(c));
  c->persist.reset(); c->temp.reset();
  const int L = c->cfg.vae_latent_channels, F = 1 << (c->cfg.vae_n_blocks - 1);
  const float* zin = z;
  if (zscale != 1.0f) {
    float* zs = (float*)c->persist.alloc((size_t)n * L * lh * lw * sizeof(float));
    CK(launch_scale_f32(z, (size_t)n * L * lh * lw, zscale, zs, c->st));
    zin = zs;
  }
  half_t* z16 = palloc(c, (size_t)n * lh * lw * 8);
  CK(launch_nchw_f32_to_nhwc_f16(zin, n, L, lh * lw, 8, z16, c->st));
  float* dst = sample_out;
  if (!dst) dst = (float*)c->persist.alloc((size_t)n * 3 * lh * F * lw * F * sizeof(float));
  CKP(vae_decode_fwd(c, z16, n, lh, lw, dst));
  if (u8_out) CK(launch_dec_to_u8(dst, n, lh * F * lw * F, u8_out, c->st));
  c->ctr.vae_decodes += n;
  if (c->persist.overflow || c->temp.overflow) return fail(c, PNPI_ENOMEM, "workspace overflow (vae decode)");
  return 0;
}

int pnpi_vae_decode(pnpi_ctx* c, const float* z, int n, int lh, int lw, float* sample_out) {
  if (!c || !z || !sample_out || n <= 0 || n > c->max_vae) return PNPI_EINVAL;
  return decode_common(c, z, n, lh, lw, 1.0f, sample_out, nullptr);
}
int pnpi_latent2image(pnpi_ctx* c, const float* z, int n, int lh, int lw, uint8_t* img_out) {
  if (!c || !z || !img_out || n <= 0 || n > c->max_vae) return PNPI_EINVAL;
  // utils/utils.py:60: latents = 1 / 0.18215 * latents  (python float 1/0.18215 rounded to fp32 by the tensor multiply)
  return decode_common(c, z, n, lh, lw, (float)(1.0 / 0.18215), nullptr, img_out);
}

static int alphas_for(pnpi_ctx* c, int t, int ratio, bool forward, float* a_from, float* a_to) {
  if (!c->sched_set) return fail(c, PNPI_ESTATE, "pnpi_set_scheduler not called");
  const int n = c->cfg.n_train_timesteps;
  if (t < 0 || t >= n) return fail(c, PNPI_EINVAL, "timestep out of range");
  if (forward) {  // next_step: (min(t - ratio, 999)) -> t
    int tp = t - ratio; if (tp > n - 1) tp = n - 1;
    *a_from = tp >= 0 ? c->ac[tp] : c->final_alpha;
    *a_to = c->ac[t];
  } else {        // prev_step: t -> t - ratio
    int tp = t - ratio;
    *a_from = c->ac[t];
    *a_to = tp >= 0 ? c->ac[tp] : c->final_alpha;
  }
  return 0;
}

int pnpi_ddim_next_step(pnpi_ctx* c, const float* eps, int t, int ratio, const float* sample, size_t n, float* out) {
  float af, at; CKP(alphas_for(c, t, ratio, true, &af, &at));
  CK(launch_ddim_move(sample, eps, af, at, n, out, c->st));
  return 0;
}
int pnpi_ddim_prev_step(pnpi_ctx* c, const float* eps, int t, int ratio, const float* sample, size_t n, float* out) {
  float af, at; CKP(alphas_for(c, t, ratio, false, &af, &at));
  CK(launch_ddim_move(sample, eps, af, at, n, out, c->st));
  return 0;
}
// DDIMSchedulerDev.step(model_output, t, sample, ref_image=, recon_lr=, recon_mask=) (scheduler_dev.py:38-95 with :68-76): one launch.
// ref / mask (nullable) are full-shape like the sample; pred_x0_out nullable.
int pnpi_ddim_prev_step_recon(pnpi_ctx* c, const float* eps, int t, int ratio, const float* sample, size_t n, const float* ref_image,
                              float recon_lr, const float* recon_mask, float* out, float* pred_x0_out) {
  if (!c || !eps || !sample || !out) return PNPI_EINVAL;
  float af, at; CKP(alphas_for(c, t, ratio, false, &af, &at));
  const bool on = ref_image && recon_lr > 0.f;
  CK(launch_ddim_prev_recon(sample, eps, af, at, on ? ref_image : nullptr, recon_lr, on ? recon_mask : nullptr, n, out, pred_x0_out, c->st));
  return 0;
}
// the recon_t window of proximal_guidance_forward.py:48,60 (and :73 for the inversion pull).  Inside it the pred-x0 pull towards ref_image
// runs for recon_lr > 0 (scheduler_dev.py:68), the pull of the step's result towards x*_{t-1} for any recon_lr != 0 (:75 has no such test)
static bool recon_window(const pnpi_recon_desc* rc, int t) {
  return rc && ((rc->recon_t > 0 && t < rc->recon_t) || (rc->recon_t < 0 && t > -rc->recon_t));
}
static const float* recon_ref_at(const pnpi_recon_desc* rc, int t) { return (recon_window(rc, t) && rc->recon_lr > 0.f) ? rc->ref_image : nullptr; }
static bool recon_inv_at(const pnpi_recon_desc* rc, int t) { return recon_window(rc, t) && rc->inv_x_stars && rc->recon_lr != 0.f; }
static int recon_check(pnpi_ctx* c, const pnpi_recon_desc* rc) {
  if (rc && rc->struct_size != (uint32_t)sizeof(pnpi_recon_desc)) return fail(c, PNPI_EINVAL, "pnpi_recon_desc.struct_size is not sizeof(pnpi_recon_desc) of this library");
  return 0;
}

int pnpi_cfg_ddim_prev(pnpi_ctx* c, const float* eps, const float* x, int nimg, int rpi, size_t row_elems, float gs, int t, int ratio,
                       const float* noise_loss, int offset_rows, const float* target, float offset_scale, float* offset_out,
                       float* x_out, const float* prox_threshold, int prox, const pnpi_recon_desc* recon) {
  if (prox < 0 || prox > 2 || (prox && !prox_threshold)) return fail(c, PNPI_EINVAL, "prox must be 0, or 1 / 2 with a threshold");
  float af, at; CKP(alphas_for(c, t, ratio, false, &af, &at));
  CKP(recon_check(c, recon));
  CfgStepP s;
  s.eps = eps; s.x = x; s.x_out = x_out; s.nimg = nimg; s.rows_per_img = rpi; s.row_elems = row_elems; s.gscale = gs; s.a_t = af; s.a_prev = at;
  s.noise_loss = noise_loss; s.offset_rows = offset_rows; s.target = target; s.offset_scale = offset_scale; s.offset_out = offset_out;
  s.prox_thr = prox_threshold; s.prox_mode = prox;
  if (prox) {
    s.recon_ref = recon_ref_at(recon, t);
    if (recon_inv_at(recon, t)) s.inv_ref = recon->inv_x_stars;     // level 1: the caller points inv_x_stars at this step's x*_{t-1} [nimg][...]
  }
  if (s.recon_ref || s.inv_ref) { s.recon_lr = recon->recon_lr; s.dilate = recon->dilate_mask; }
  s.lat_h = s.lat_w = c->cfg.sample_size;
  CK(launch_cfg_ddim_prev(s, c->st));
  return 0;
}

int pnpi_prox_threshold(pnpi_ctx* c, const float* eps, int nimg, int rpi, size_t row_elems, float quantile, float* thr_out) {
  if (!c || !eps || !thr_out || nimg <= 0 || !(quantile > 0.f && quantile <= 1.f)) return PNPI_EINVAL;
  int r = launch_quantile_abs_diff(eps, nimg, rpi, row_elems, quantile, thr_out, c->st);
  if (r == -6) return fail(c, PNPI_ESHAPE, "proximal threshold: more than 32768 elements per image");
  CK(r);
  return 0;
}

// One CLIPEncoderLayer (transformers modeling_clip.py), shared by the two towers: pre-LN self-attention (causal in the text tower, full in
// the image tower) and the quick_gelu MLP, each with its residual; x [n * T][H] is updated in place.  rows: identity row table [n][4].
// DINO's Block (vision_transformer.py) is the same layer with ln_eps = 1e-6 and the erf-form GELU (gelu_erf = 1).
static int clip_encoder_layer(pnpi_ctx* c, const ClipLayerW& L, half_t* x, int n, int T, int H, int heads, int I, int causal, const int* rows,
                              float ln_eps = 1e-5f, int gelu_erf = 0) {
  const int M = n * T, dh = H / heads, ldv = round_up_i(T, 8);
  const size_t mk = c->temp.mark();
  half_t* h1 = talloc(c, (size_t)M * H);
  if (!c->dry) PROF(PNPI_KC_LAYERNORM, 0.0, 2.0 * M * (double)H * 2.0, launch_layernorm(x, M, H, ln_eps, L.ln1.g, L.ln1.b, h1, c->st));
  half_t* qk = talloc(c, (size_t)M * 2 * H);
  half_t* vt = talloc(c, (size_t)n * H * ldv);
  {
    VtOut v; v.outT = vt; v.col0 = 2 * H; v.ld = ldv; v.f32 = 0; v.rpb = T;
    CK(op_gemm(c, h1, H, M, H, L.w_qkv, H, 3 * H, L.b_qkv, nullptr, 0, qk, 2 * H, 1.f, &v));
  }
  half_t* ao = talloc(c, (size_t)M * H);
  {
    AttnP a; a.q = qk; a.ldq = 2 * H; a.q_off = 0; a.k = qk; a.ldk = 2 * H; a.k_off = H; a.vt = vt; a.ldv = ldv;
    a.o = ao; a.ldo = H; a.heads = heads; a.Nq = T; a.Nk = T; a.Dp = dh; a.dh = dh; a.scale = 1.0f / sqrtf((float)dh);
    a.rows = rows; a.nrows = n; a.causal = causal;
    if (!c->dry) PROFD(PNPI_KC_ATTN_FLASH, 4.0 * n * heads * (double)T * T * dh, 0.0, T, T, dh, launch_attn_flash(a, c->st));
  }
  half_t* x1 = talloc(c, (size_t)M * H);
  CK(op_gemm(c, ao, H, M, H, L.out.w, H, H, L.out.b, x, H, x1, H));
  half_t* h2 = talloc(c, (size_t)M * H);
  if (!c->dry) PROF(PNPI_KC_LAYERNORM, 0.0, 2.0 * M * (double)H * 2.0, launch_layernorm(x1, M, H, ln_eps, L.ln2.g, L.ln2.b, h2, c->st));
  half_t* f = talloc(c, (size_t)M * I);
  CK(op_gemm(c, h2, H, M, H, L.fc1.w, H, I, L.fc1.b, nullptr, 0, f, I));
  if (!c->dry) CK(gelu_erf ? launch_gelu_erf(f, (size_t)M * I, c->st) : launch_quick_gelu(f, (size_t)M * I, c->st));
  CK(op_gemm(c, f, I, M, I, L.fc2.w, I, H, L.fc2.b, x1, H, x, H));    // x <- x1 + mlp (x's old value is dead)
  c->temp.release(mk);
  return 0;
}

// CLIPTextModel.forward -> last_hidden_state (transformers modeling_clip.py: CLIPTextEmbeddings, CLIPEncoderLayer x L with a
// causal mask, final_layer_norm); pre-LN blocks, quick_gelu MLP.  ids: device int32 [n][T]; out fp32 [n][T][H] (nullable);
// y16_out (nullable): the same rows in fp16, in the persistent workspace until the next forward resets it.
static int clip_fwd(pnpi_ctx* c, const int* ids, int n, float* out, half_t** y16_out) {
  const ClipW& t = c->clip;
  const int H = t.H, T = t.T, M = n * T;
  c->persist.reset(); c->temp.reset();
  half_t* x = palloc(c, (size_t)M * H);
  if (!c->dry) CK(launch_embed_tokens(ids, M, T, H, t.vocab, t.tok, t.pos, x, c->st));
  for (const ClipLayerW& L : t.layers) CKP(clip_encoder_layer(c, L, x, n, T, H, t.heads, t.I, 1, c->rows_ident));
  half_t* y = palloc(c, (size_t)M * H);
  if (!c->dry) {
    PROF(PNPI_KC_LAYERNORM, 0.0, 2.0 * M * (double)H * 2.0, launch_layernorm(x, M, H, 1e-5f, t.final_ln.g, t.final_ln.b, y, c->st));
    if (out) CK(launch_f16_to_f32(y, (size_t)M * H, out, c->st));
  }
  if (y16_out) *y16_out = y;
  return 0;
}

int pnpi_text_encode(pnpi_ctx* c, const int32_t* input_ids, int n, float* hidden_out) {
  if (!c || !input_ids || !hidden_out || n <= 0) return PNPI_EINVAL;
  CKP(check_clip_ready(c));
  if (n > c->rows_ident_n) return fail(c, PNPI_EINVAL, "more prompts than max(max_unet_rows, 8)");
  return clip_fwd(c, (const int*)input_ids, n, hidden_out);
}

#include "api_vit.inc"
#include "api_clipscore.inc"
#include "api_structdist.inc"
#include "api_lpips.inc"

// ---------------------------------------------------------------------------------------------------- kernel-level ops
static int conv_hook(pnpi_ctx* c, const void* x1, const void* x2, int C1, int C2, int B, int H, int W, int ksize, int stride, int pad, int ups,
                     int Ho, int Wo, const void* w, const float* bias, const void* res, int N, void* out, int force_cfg, int force_split,
                     float* stats_out, int* tile_rows_out) {
  GemmP p; gemm_defaults(p);
  p.x1 = (const half_t*)x1; p.x2 = (const half_t*)x2; p.C1 = C1; p.C2 = C2; p.ldx1 = C1; p.ldx2 = C2;
  p.B = B; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.ksize = ksize; p.stride = stride; p.pad = pad; p.ups = ups;
  p.K = ksize * ksize * (C1 + C2); p.w = (const half_t*)w; p.ldw = p.K; p.M = B * Ho * Wo; p.N = N;
  p.bias = bias; p.res = (const half_t*)res; p.ldres = N; p.out = (half_t*)out; p.ldo = N; p.stats = stats_out;
  CK(launch_igemm(p, c->splitk_ws, c->splitk_bytes, c->st, force_cfg, force_split, nullptr, tile_rows_out));
  return 0;
}
int pnpi_op_conv(pnpi_ctx* c, const void* x1, const void* x2, int C1, int C2, int B, int H, int W, int ksize, int stride, int pad,
                 int ups, int Ho, int Wo, const void* w, const float* bias, const void* res, int N, void* out, int force_cfg,
                 int force_split) {
  return conv_hook(c, x1, x2, C1, C2, B, H, W, ksize, stride, pad, ups, Ho, Wo, w, bias, res, N, out, force_cfg, force_split, nullptr, nullptr);
}
/* conv + the per-(m-tile, channel) GroupNorm partial sums its epilogue produces (the statistics fusion of resnet_fwd): stats_out
 * [ceil(M / tile_rows)][N][2] fp32 = (sum, sum of squares) of the stored fp16 values; *tile_rows_out = rows per m-tile, 0 when the
 * launch configuration produced no statistics (split-K, non-DMA shapes). */
int pnpi_op_conv_stats(pnpi_ctx* c, const void* x1, const void* x2, int C1, int C2, int B, int H, int W, int ksize, int stride, int pad,
                       int ups, int Ho, int Wo, const void* w, const float* bias, const void* res, int N, void* out, int force_cfg,
                       int force_split, float* stats_out, int* tile_rows_out) {
  if (!c || !stats_out || !tile_rows_out) return PNPI_EINVAL;
  return conv_hook(c, x1, x2, C1, C2, B, H, W, ksize, stride, pad, ups, Ho, Wo, w, bias, res, N, out, force_cfg, force_split, stats_out, tile_rows_out);
}
/* host-only queries of tile selection (pnpi_set_tuning and its kin: tuning.hip) */
int pnpi_tile_table_lookup(int M, int N, int K, int ksize, int* cfg, int* split, int* entry_m) {
  return igemm_table_lookup(M, N, K, ksize, cfg, split, entry_m);
}
int pnpi_pp_rowtile_query(int cfg, int M, int N, int split) { return igemm_pp_rowtile_query(cfg, M, N, split); }
int pnpi_igemm_plan_query(const pnpi_igemm_launch_desc* d, pnpi_igemm_plan* plan) {
  static_assert(sizeof(pnpi_igemm_plan) == sizeof(IgemmPlan), "pnpi_igemm_plan mirrors IgemmPlan field for field");
  if (!d || !plan) return PNPI_EINVAL;
  half_t* const some = (half_t*)(uintptr_t)4096;      // operands are never dereferenced: only null / alignment are looked at
  GemmP p;
  gemm_defaults(p);
  p.x1 = some; p.w = some; p.out = some; p.x2 = d->C2 ? some : nullptr;
  p.M = d->M; p.N = d->N; p.K = d->K; p.ksize = d->ksize; p.pad = d->ksize / 2; p.C1 = d->C1; p.C2 = d->C2;
  p.B = 1; p.H = d->M; p.W = 1; p.Ho = d->M; p.Wo = 1;      // rows only: B * H * W = M
  p.ldx1 = d->ldx1; p.ldx2 = d->ldx2; p.ldw = d->ldw; p.ldo = d->ldo; p.ldres = d->ldres;
  if (d->bias) p.bias = (const float*)((uintptr_t)some + (d->bias_aligned16 ? 0 : 4));
  if (d->residual) p.res = some;
  if (d->stats) p.stats = (float*)some;
  p.geglu = d->geglu;
  p.vt_col0 = d->vt_col0; p.vt_ld = d->vt_ld; p.vt_f32 = d->vt_f32; p.rows_per_batch = d->rows_per_batch; p.vt_perm16 = d->vt_perm16;
  if (d->vt_col0 < d->N) p.outT = some;
  p.nbatch = d->nbatch;
  const IgemmPlan pl = igemm_plan(p, d->ws_bytes > 0, d->ws_bytes > 0 ? (size_t)d->ws_bytes : 0, d->force_cfg, d->force_split, d->sel_M);
  memcpy(plan, &pl, sizeof pl);
  return 0;
}
int pnpi_igemm_instance_info(int index, const char** name, int* geom7, int* ablation_only) {
  return igemm_instance_info(index, name, geom7, ablation_only) ? PNPI_EINVAL : 0;
}
int pnpi_op_gemm(pnpi_ctx* c, const void* a, int lda, const void* w, int ldw, int M, int N, int K, float alpha, const float* bias,
                 const void* res, void* out, int ldo, int vt_col0, void* outT, int vt_ld, int vt_f32, int rpb, int force_cfg,
                 int force_split) {
  GemmP p; gemm_defaults(p);
  p.x1 = (const half_t*)a; p.C1 = K; p.ldx1 = lda; p.B = 1; p.H = 1; p.W = M; p.Ho = 1; p.Wo = M; p.ksize = 1;
  p.w = (const half_t*)w; p.ldw = ldw; p.M = M; p.N = N; p.K = K; p.alpha = alpha; p.bias = bias; p.res = (const half_t*)res;
  p.ldres = N; p.out = (half_t*)out; p.ldo = ldo;
  if (outT) { p.outT = outT; p.vt_col0 = vt_col0; p.vt_ld = vt_ld; p.vt_f32 = vt_f32; p.rows_per_batch = rpb; p.vt_perm16 = g_op_gemm_vt_perm16; }
  CK(launch_igemm(p, c->splitk_ws, c->splitk_bytes, c->st, force_cfg, force_split));
  return 0;
}
int pnpi_op_gemm_geglu(pnpi_ctx* c, const void* a, int lda, const void* w, int ldw, int M, int N, int K, const float* bias, void* out,
                       int ldo) {
  GemmP p; gemm_defaults(p);
  p.x1 = (const half_t*)a; p.C1 = K; p.ldx1 = lda; p.B = 1; p.H = 1; p.W = M; p.Ho = 1; p.Wo = M; p.ksize = 1;
  p.w = (const half_t*)w; p.ldw = ldw; p.M = M; p.N = N; p.K = K; p.bias = bias; p.out = (half_t*)out; p.ldo = ldo; p.geglu = 1;
  CK(launch_igemm(p, c->splitk_ws, c->splitk_bytes, c->st));
  return 0;
}
int pnpi_op_groupnorm(pnpi_ctx* c, const void* x1, const void* x2, int C1, int C2, int B, int HW, int G, float eps, const float* gamma,
                      const float* beta, int silu, void* out) {
  if (!c || !x1 || !gamma || !beta || !out || B <= 0 || HW <= 0 || G <= 0) return PNPI_EINVAL;
  if (groupnorm_scratch_floats(C1, C2, B, HW, G, false) > c->gn_partial_floats)
    return fail(c, PNPI_ESHAPE, "groupnorm: the context's statistics scratch is sized for max_unet_rows batch items");
  CK(launch_groupnorm((const half_t*)x1, (const half_t*)x2, C1, C2, B, HW, G, eps, gamma, beta, silu, (half_t*)out, c->gn_partial, c->st));
  return 0;
}
/* the statistics-fed GroupNorm of op_gn: the producers' partials instead of a statistics pass, refused where op_gn would recompute */
int pnpi_op_groupnorm_stats(pnpi_ctx* c, const void* x1, const void* x2, int C1, int C2, int B, int HW, int G, float eps, const float* gamma,
                            const float* beta, int silu, void* out, const float* st1, int rows1, const float* st2, int rows2) {
  if (!c || !x1 || !gamma || !beta || !out || !st1 || B <= 0 || HW <= 0 || G <= 0 || C1 <= 0 || C2 < 0) return PNPI_EINVAL;
  if ((x2 != nullptr) != (C2 > 0) || (x2 && !st2)) return PNPI_EINVAL;
  if (!gn_stats_usable(HW, rows1) || (x2 && !gn_stats_usable(HW, rows2)))
    return fail(c, PNPI_ESHAPE, "groupnorm_stats: partials need rows > 0, HW % rows == 0 and HW / rows <= 256 (op_gn recomputes the statistics here)");
  if (groupnorm_scratch_floats(C1, C2, B, HW, G, true) > c->gn_partial_floats)
    return fail(c, PNPI_ESHAPE, "groupnorm_stats: the context's statistics scratch is sized for max_unet_rows batch items");
  CK(launch_groupnorm_fused((const half_t*)x1, (const half_t*)x2, C1, C2, B, HW, G, eps, gamma, beta, silu, (half_t*)out, st1, HW / rows1, st2,
                            x2 ? HW / rows2 : 1, c->gn_partial, c->st));
  return 0;
}
int pnpi_op_layernorm(pnpi_ctx* c, const void* x, int M, int C, float eps, const float* gamma, const float* beta, void* out) {
  CK(launch_layernorm((const half_t*)x, M, C, eps, gamma, beta, (half_t*)out, c->st));
  return 0;
}
int pnpi_op_geglu(pnpi_ctx* c, const void* x, int M, int inner, void* out) {
  if (!c || !x || !out || M <= 0 || inner <= 0) return PNPI_EINVAL;      // (a zero-block grid otherwise)
  CK(launch_geglu((const half_t*)x, M, inner, (half_t*)out, c->st));
  return 0;
}
int pnpi_op_softmax_rows(pnpi_ctx* c, void* x, int M, int N, int ld) {
  if (!c || !x || M <= 0 || N <= 0) return PNPI_EINVAL;
  if (ld < N) return fail(c, PNPI_ESHAPE, "softmax_rows: ld < N");
  CK(launch_softmax_rows((half_t*)x, M, N, ld, c->st));
  return 0;
}
/* kernel-level forms of three launchers no other entry point reaches on their own (tests/test_gpu_norm_fwd_instances.py): the fp32 row
 * softmax and the padded fp16 conversion of the materialised attention path (controller call-back, attention backward), and the GEMV of
 * the time-embedding MLP. */
int pnpi_op_softmax_rows_f32(pnpi_ctx* c, float* x, int M, int N) {
  if (!c || !x || M <= 0 || N <= 0) return PNPI_EINVAL;
  CK(launch_softmax_rows_f32(x, (size_t)M, N, c->st));
  return 0;
}
int pnpi_op_f32_rows_to_f16_padded(pnpi_ctx* c, const float* in, int M, int N, int ld, void* out) {
  if (!c || !in || !out || M <= 0 || N <= 0) return PNPI_EINVAL;
  if (ld < N) return fail(c, PNPI_ESHAPE, "f32_rows_to_f16_padded: ld < N");
  CK(launch_f32_rows_to_f16_padded(in, (size_t)M, N, ld, (half_t*)out, c->st));
  return 0;
}
int pnpi_op_gemv(pnpi_ctx* c, const float* x, int K, const void* w, int N, const float* bias, const float* bias2, int silu_in, float* out) {
  if (!c || !x || !w || !out || K <= 0 || N <= 0) return PNPI_EINVAL;
  CK(launch_gemv(x, K, (const half_t*)w, N, bias, bias2, silu_in, out, c->st));
  return 0;
}
/* pnpi_op_attention_bwd with what the recording forward left (kernel tests of the hand-over): lse_fwd [B][heads][Nq] log2-domain
 * log-sum-exp and o_fwd [B*Nq][ld_ofwd] the forward's output -- the flash dQ then skips its first pass over the keys.  Both nullable. */
int pnpi_op_attention_bwd_fwd(pnpi_ctx* c, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* v, int ldv, int v_off,
                              const void* d_o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, int B, void* dq, void* dk, void* dv,
                              void* scratch, size_t scratch_bytes, const float* lse_fwd, const void* o_fwd, int ld_ofwd) {
  if (!c || !q || !k || !v || !d_o || !dq || !dk || !dv) return PNPI_EINVAL;
  CKP(attn_bwd(c, (const half_t*)q, ldq, q_off, (const half_t*)k, ldk, k_off, (const half_t*)v, ldv, v_off, (const half_t*)d_o, ldo,
               heads, Nq, Nk, Dp, dh, scale, B, (half_t*)dq, (half_t*)dk, (half_t*)dv, scratch, scratch_bytes, lse_fwd, (const half_t*)o_fwd, ld_ofwd));
  return 0;
}
int pnpi_op_attention_bwd(pnpi_ctx* c, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* v, int ldv, int v_off,
                          const void* d_o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, int B, void* dq, void* dk, void* dv,
                          void* scratch, size_t scratch_bytes) {
  return pnpi_op_attention_bwd_fwd(c, q, ldq, q_off, k, ldk, k_off, v, ldv, v_off, d_o, ldo, heads, Nq, Nk, Dp, dh, scale, B, dq, dk, dv, scratch,
                                   scratch_bytes, nullptr, nullptr, 0);
}
size_t pnpi_op_attention_bwd_scratch_bytes(int Nq, int Nk, int dh) { return attn_bwd_scratch_bytes(Nq, Nk, dh); }
/* host-only: what attn_bwd decides for this shape under the tuning in force (scratch_bytes < 0: as much as the form asks for) */
int pnpi_attn_bwd_plan_query(int heads, int Nq, int Nk, int Dp, int dh, long long scratch_bytes, int have_fwd, pnpi_attn_bwd_plan* plan) {
  if (!plan || heads <= 0 || Nq <= 0 || Nk <= 0 || Dp <= 0 || dh <= 0) return PNPI_EINVAL;
  const AttnBwdPlan pl = attn_bwd_plan(heads, Nq, Nk, Dp, dh, scratch_bytes < 0 ? SIZE_MAX : (size_t)scratch_bytes, have_fwd != 0);
  plan->flash = pl.flash; plan->lt = pl.lt; plan->nsplit = pl.nsplit;
  plan->pf_dq = pl.pf[0]; plan->pf_dk = pl.pf[1]; plan->pf_dv = pl.pf[2];
  plan->one_pass = pl.one_pass; plan->share_rows = pl.share_rows; plan->empty_shares = pl.empty_shares;
  plan->scratch_bytes = pl.scratch_bytes;
  return 0;
}
// ---- activation-gradient kernels (null-text path groundwork; tests/test_gpu_backward.py)
int pnpi_op_layernorm_bwd(pnpi_ctx* c, const void* x, const void* dy, int M, int C, float eps, const float* gamma, void* dx) {
  CK(launch_layernorm_bwd((const half_t*)x, (const half_t*)dy, M, C, eps, gamma, (half_t*)dx, c->st));
  return 0;
}
int pnpi_op_groupnorm_bwd(pnpi_ctx* c, const void* x1, const void* x2, int C1, int C2, int B, int HW, int G, float eps, const float* gamma,
                          const float* beta, int silu, const void* dy, void* dx) {
  const int C = C1 + C2;
  if (!(C & 7) && !(C1 & 7) && G <= 64) {      // the product path: three chip-wide phases (here with one dense destination)
    float* ws = nullptr;
    CKP(gn_bwd_workspace(c, B, HW, G, &ws));
    CK(launch_groupnorm_bwd2((const half_t*)x1, (const half_t*)x2, C1, C2, B, HW, G, eps, gamma, beta, silu, (const half_t*)dy,
                             GnbOut{(half_t*)dx, C, 0}, GnbOut{(half_t*)dx + C1, C, 0}, ws, c->st));
    return 0;
  }
  CK(launch_groupnorm_bwd((const half_t*)x1, (const half_t*)x2, C1, C2, B, HW, G, eps, gamma, beta, silu, (const half_t*)dy, (half_t*)dx, c->st));
  return 0;
}
/* kernel-level forms of what tape_backward launches (tests/test_gpu_bwd_walk_ops.py).  groupnorm_bwd_split: the three-phase kernel with
 * the walk's two separate destinations (ld, accumulate, or none); scratch NULL = the context's workspace, else the caller's buffer of
 * scratch_floats floats.  groupnorm_bwd_ref: always the one-block-per-group kernel the walk falls back to. */
size_t pnpi_op_groupnorm_bwd_scratch_floats(int B, int HW, int G) {
  if (B <= 0 || HW <= 0 || G <= 0) return 0;
  return groupnorm_bwd2_scratch_floats(B, HW, G);
}
int pnpi_op_groupnorm_bwd_split(pnpi_ctx* c, const void* x1, const void* x2, int C1, int C2, int B, int HW, int G, float eps, const float* gamma,
                                const float* beta, int silu, const void* dy, void* dx1, int ld1, int acc1, void* dx2, int ld2, int acc2,
                                float* scratch, size_t scratch_floats) {
  if (!c || !x1 || !gamma || !beta || !dy || B <= 0 || HW <= 0 || G <= 0 || C1 <= 0 || C2 < 0) return PNPI_EINVAL;
  if ((dx1 && ld1 < C1) || (dx2 && ld2 < C2))
    return fail(c, PNPI_ESHAPE, "groupnorm_bwd_split: a destination's row stride is shorter than its channel count");
  float* ws = scratch;
  if (!ws) CKP(gn_bwd_workspace(c, B, HW, G, &ws));
  else if (scratch_floats < groupnorm_bwd2_scratch_floats(B, HW, G))
    return fail(c, PNPI_ESHAPE, "groupnorm_bwd_split: scratch is smaller than pnpi_op_groupnorm_bwd_scratch_floats(B, HW, G)");
  CK(launch_groupnorm_bwd2((const half_t*)x1, (const half_t*)x2, C1, C2, B, HW, G, eps, gamma, beta, silu, (const half_t*)dy,
                           GnbOut{(half_t*)dx1, ld1, acc1 ? 1 : 0}, GnbOut{C2 ? (half_t*)dx2 : nullptr, ld2, acc2 ? 1 : 0}, ws, c->st));
  return 0;
}
int pnpi_op_groupnorm_bwd_ref(pnpi_ctx* c, const void* x1, const void* x2, int C1, int C2, int B, int HW, int G, float eps, const float* gamma,
                              const float* beta, int silu, const void* dy, void* dx) {
  if (!c || !x1 || !gamma || !beta || !dy || !dx || G <= 0 || C1 <= 0 || C2 < 0) return PNPI_EINVAL;
  CK(launch_groupnorm_bwd((const half_t*)x1, (const half_t*)x2, C1, C2, B, HW, G, eps, gamma, beta, silu, (const half_t*)dy, (half_t*)dx, c->st));
  return 0;
}
int pnpi_op_strided_add(pnpi_ctx* c, void* dst, const void* src, int ld, int off, size_t R, int C, int accumulate) {
  if (!c || !dst || !src || ld <= 0 || off < 0 || C <= 0) return PNPI_EINVAL;
  if (off + C > ld) return fail(c, PNPI_ESHAPE, "strided_add: columns off .. off + C reach past the source row (ld)");
  CK(launch_strided_add_f16((half_t*)dst, (const half_t*)src, ld, off, R, C, accumulate, c->st));
  return 0;
}
int pnpi_op_pad_heads(pnpi_ctx* c, const void* src, size_t R, int heads, int dh, int Dp, void* dst) {
  if (!c || !src || !dst || heads <= 0 || dh <= 0) return PNPI_EINVAL;
  if (Dp < dh) return fail(c, PNPI_ESHAPE, "pad_heads: Dp < dh");
  CK(launch_pad_heads_f16((const half_t*)src, R, heads, dh, Dp, (half_t*)dst, c->st));
  return 0;
}
int pnpi_op_add_f16_to_f32(pnpi_ctx* c, float* dst, const void* src, size_t n, float scale) {
  if (!c || !dst || !src) return PNPI_EINVAL;
  CK(launch_add_f16_to_f32(dst, (const half_t*)src, n, scale, c->st));
  return 0;
}
int pnpi_op_transpose(pnpi_ctx* c, const void* src, int ld_src, int R, int Cc, void* dst, int ld_dst, int nbatch, long s_src, long s_dst) {
  if (!c || !src || !dst) return PNPI_EINVAL;
  CK(launch_transpose_f16((const half_t*)src, ld_src, R, Cc, (half_t*)dst, ld_dst, c->st, nbatch, s_src, s_dst));
  return 0;
}
int pnpi_op_repack_dgrad_pad(pnpi_ctx* c, const void* w, int N, int Npad, int taps, int Cin, void* wd) {
  if (!c || !w || !wd || N <= 0 || taps <= 0 || Cin <= 0) return PNPI_EINVAL;
  CK(launch_repack_dgrad((const half_t*)w, N, Npad, taps, Cin, (half_t*)wd, c->st));
  return 0;
}
int pnpi_op_geglu_bwd(pnpi_ctx* c, const void* h, const void* dy, int M, int inner, void* dh) {
  CK(launch_geglu_bwd((const half_t*)h, (const half_t*)dy, M, inner, (half_t*)dh, c->st));
  return 0;
}
int pnpi_op_softmax_bwd_rows(pnpi_ctx* c, const float* P, const float* dP, int R, int N, int ld, float scale, void* dS) {
  CK(launch_softmax_bwd_rows(P, dP, (size_t)R, N, ld, scale, (half_t*)dS, c->st));
  return 0;
}
int pnpi_op_accumulate(pnpi_ctx* c, void* dst, const void* src, size_t n) {
  CK(launch_accumulate_f16((half_t*)dst, (const half_t*)src, n, c->st));
  return 0;
}
int pnpi_op_sumpool2x2(pnpi_ctx* c, const void* dup, int B, int H, int W, int C, void* dx) {
  CK(launch_sumpool2x2((const half_t*)dup, B, H, W, C, (half_t*)dx, c->st));
  return 0;
}
int pnpi_op_zero_stuff2(pnpi_ctx* c, const void* dy, int B, int Ho, int Wo, int C, void* out) {
  CK(launch_zero_stuff2((const half_t*)dy, B, Ho, Wo, C, (half_t*)out, c->st));
  return 0;
}
int pnpi_op_repack_dgrad(pnpi_ctx* c, const void* w, int N, int taps, int Cin, void* wd) {
  CK(launch_repack_dgrad((const half_t*)w, N, N, taps, Cin, (half_t*)wd, c->st));
  return 0;
}
int pnpi_op_null_text_loss(pnpi_ctx* c, const float* eps_u, const float* eps_c, const float* x, const float* target, int n, float w, float c_x,
                           float c_e, float grad_scale, void* d_eps_u, float* loss) {
  CK(launch_null_text_loss(eps_u, eps_c, x, target, n, w, c_x, c_e, grad_scale, (float*)d_eps_u, loss, c->st));
  return 0;
}
int pnpi_op_adam_step(pnpi_ctx* c, float* p, float* m, float* v, const float* g, int n, int k, float lr, float inv_scale) {
  CK(launch_adam_step(p, m, v, g, n, k, lr, inv_scale, c->st));
  return 0;
}
/* pnpi_op_attention with the two AttnP fields only the model sets: causal (CLIP text encoder) and lse_dev [nrows_out][heads][Nq], the
 * log2-domain log-sum-exp the recording forward leaves for the backward (nullable).  The tuning keys apply as in pnpi_op_attention. */
int pnpi_op_attention_ex(pnpi_ctx* c, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* vt, int ldv,
                         void* o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, const int* rows_dev, int nrows, int causal,
                         float* lse_dev) {
  if (!c || !q || !k || !vt || !o || !rows_dev) return PNPI_EINVAL;
  AttnP a; a.q = (const half_t*)q; a.ldq = ldq; a.q_off = q_off; a.k = (const half_t*)k; a.ldk = ldk; a.k_off = k_off;
  a.vt = (const half_t*)vt; a.ldv = ldv; a.o = (half_t*)o; a.ldo = ldo; a.heads = heads; a.Nq = Nq; a.Nk = Nk; a.Dp = Dp; a.dh = dh;
  a.scale = scale; a.rows = rows_dev; a.nrows = nrows;
  a.causal = causal ? 1 : 0; a.lse = lse_dev;
  a.vt_perm = (g_op_attention_vt_perm && attn_flash_uses_dma64(Dp, Nk, a.causal)) ? 1 : 0;
  a.aug = g_op_attention_aug;
  CK(launch_attn_flash(a, c->st));
  return 0;
}
int pnpi_op_attention(pnpi_ctx* c, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* vt, int ldv,
                      void* o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, const int* rows_dev, int nrows) {
  return pnpi_op_attention_ex(c, q, ldq, q_off, k, ldk, k_off, vt, ldv, o, ldo, heads, Nq, Nk, Dp, dh, scale, rows_dev, nrows, 0, nullptr);
}
/* pnpi_op_attention over class-restricted keys (attn.hip attn_flash_masked_kernel): kcls_dev [nmask][Nk], qcls_dev [nmask][Nq] class bytes,
 * mrow_dev [nrows] the class row of each entry of rows_dev.  The tuning key "op_attention_vt_perm" applies as in pnpi_op_attention. */
int pnpi_op_attention_masked(pnpi_ctx* c, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* vt, int ldv,
                             void* o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, const int* rows_dev, int nrows,
                             const uint8_t* kcls_dev, const uint8_t* qcls_dev, const int* mrow_dev) {
  if (!c || !q || !k || !vt || !o || !rows_dev || !kcls_dev || !qcls_dev || !mrow_dev) return PNPI_EINVAL;
  AttnP a; a.q = (const half_t*)q; a.ldq = ldq; a.q_off = q_off; a.k = (const half_t*)k; a.ldk = ldk; a.k_off = k_off;
  a.vt = (const half_t*)vt; a.ldv = ldv; a.o = (half_t*)o; a.ldo = ldo; a.heads = heads; a.Nq = Nq; a.Nk = Nk; a.Dp = Dp; a.dh = dh;
  a.scale = scale; a.rows = rows_dev; a.nrows = nrows;
  a.vt_perm = (g_op_attention_vt_perm && attn_flash_uses_dma64(Dp, Nk, 0)) ? 1 : 0;
  AttnMaskP mk; mk.kcls = kcls_dev; mk.qcls = qcls_dev; mk.mrow = mrow_dev;
  CK(launch_attn_flash_masked(a, mk, c->st));
  return 0;
}
/* F.interpolate(mode="nearest") of n uint8 masks [n][H][W] to [n][h][w] class bytes (device pointers): the per-level resize of pnpi_masa_set_masks */
int pnpi_op_masa_mask_level(pnpi_ctx* c, const uint8_t* in_dev, int n, int H, int W, int h, int w, uint8_t* out_dev) {
  if (!c || !in_dev || !out_dev) return PNPI_EINVAL;
  CK(launch_masa_mask_level(in_dev, n, H, W, h, w, out_dev, c->st));
  return 0;
}
int pnpi_masa_set_masks(pnpi_ctx* c, const uint8_t* mask_s_host, const uint8_t* mask_t_host, int nimg, int h, int w) {
  if (!c) return PNPI_EINVAL;
  MasaMasks& mm = c->mm;
  if (!mask_s_host && !mask_t_host) { mm.nimg = 0; return 0; }      // cleared: kind-2 controllers run plain MasaCtrl again
  if (!mask_s_host || !mask_t_host) return fail(c, PNPI_EINVAL, "pnpi_masa_set_masks: mask_s and mask_t come together (NULL, NULL clears them)");
  const pnpi_model_config& g = c->cfg;
  const int cap = c->max_rows / 4;
  if (nimg <= 0 || nimg > cap) return fail(c, PNPI_EINVAL, "pnpi_masa_set_masks: nimg must be 1 .. max_unet_rows / 4");
  if (h <= 0 || w <= 0 || h > 4096 || w > 4096) return fail(c, PNPI_EINVAL, "pnpi_masa_set_masks: mask sides must be 1 .. 4096");
  const size_t n = (size_t)nimg * h * w;
  for (size_t i = 0; i < n; ++i)
    if (mask_s_host[i] > 1 || mask_t_host[i] > 1)
      return fail(c, PNPI_EINVAL, "pnpi_masa_set_masks: masks must be binary (0 / 1); the two-pass blend of fractional masks is not built");
  if (!mm.base) {      // once per context: the level buffers keep their addresses
    mm.cap_img = cap; mm.side.clear(); mm.off.clear();
    size_t total = 0;
    for (int i = 0; i < g.n_blocks; ++i) {
      const int sd = g.sample_size >> i;
      mm.side.push_back(sd); mm.off.push_back(total);
      total += align_up((size_t)2 * cap * sd * sd, 256);
    }
    CKH(hipMalloc((void**)&mm.base, total));
  }
  if (mm.stage_bytes < 2 * n) {
    CKH(hipStreamSynchronize(c->st));
    if (mm.stage) CKH(hipFree(mm.stage));
    mm.stage = nullptr; mm.stage_bytes = 0;
    CKH(hipMalloc((void**)&mm.stage, 2 * n));
    mm.stage_bytes = 2 * n;
  }
  mm.nimg = 0;
  CKP(upload(c, mm.stage, mask_s_host, n));
  CKP(upload(c, mm.stage + n, mask_t_host, n));
  for (size_t l = 0; l < mm.side.size(); ++l) {
    const int sd = mm.side[l];
    CK(launch_masa_mask_level(mm.stage, nimg, h, w, sd, sd, mm.base + mm.off[l], c->st));
    CK(launch_masa_mask_level(mm.stage + n, nimg, h, w, sd, sd, mm.base + mm.off[l] + (size_t)mm.cap_img * sd * sd, c->st));
  }
  mm.nimg = nimg;
  return 0;
}
/* the resized masks of level `level` (side = sample_size >> level) as pnpi_masa_set_masks left them: [nimg][side][side] class bytes each */
int pnpi_masa_get_level_masks(pnpi_ctx* c, int level, uint8_t* mask_s_out_host, uint8_t* mask_t_out_host, int* side_out) {
  if (!c || !mask_s_out_host || !mask_t_out_host) return PNPI_EINVAL;
  const MasaMasks& mm = c->mm;
  if (mm.nimg <= 0) return fail(c, PNPI_ESTATE, "pnpi_masa_get_level_masks: no masks are set");
  if (level < 0 || level >= (int)mm.side.size()) return fail(c, PNPI_EINVAL, "pnpi_masa_get_level_masks: level out of range");
  const size_t n = (size_t)mm.nimg * mm.side[level] * mm.side[level];
  CKH(hipStreamSynchronize(c->st));
  CKH(hipMemcpy(mask_s_out_host, mm.s_at(level), n, hipMemcpyDeviceToHost));
  CKH(hipMemcpy(mask_t_out_host, mm.t_at(level), n, hipMemcpyDeviceToHost));
  if (side_out) *side_out = mm.side[level];
  return 0;
}
int pnpi_op_cross_edit(pnpi_ctx* c, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* vt, int ldv,
                       void* o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, const int* pairs_dev, int npairs,
                       const void* mmatT, const float* c1, const float* c2, const float* lb_alpha, float* lb_acc, int lb_slot0,
                       int lb_nslots) {
  CrossEditP e; e.q = (const half_t*)q; e.ldq = ldq; e.q_off = q_off; e.k = (const half_t*)k; e.ldk = ldk; e.k_off = k_off;
  e.vt = (const half_t*)vt; e.ldv = ldv; e.o = (half_t*)o; e.ldo = ldo; e.heads = heads; e.Nq = Nq; e.Nk = Nk; e.Dp = Dp; e.dh = dh;
  e.scale = scale; e.pairs = pairs_dev; e.npairs = npairs; e.mmatT = (const half_t*)mmatT; e.c1 = c1; e.c2 = c2;
  e.lb_alpha = lb_alpha; e.lb_acc = lb_acc; e.lb_slot0 = lb_slot0; e.lb_nslots = lb_nslots; e.write_src = 1;
  CK(launch_attn_cross_edit(e, c->st));
  return 0;
}
int pnpi_op_local_blend(pnpi_ctx* c, const float* lb_acc, int nslots, int map_hw, int lat_hw, int C, float th, float* latents, int nimg) {
  CK(launch_local_blend(lb_acc, nslots, map_hw, lat_hw, C, th, latents, nimg, c->st));
  return 0;
}
int pnpi_op_local_blend_sub(pnpi_ctx* c, const float* lb_acc, int nslots, int map_hw, int lat_hw, int C, float th, float th_sub,
                            float* latents, int nimg) {
  CK(launch_local_blend(lb_acc, nslots, map_hw, lat_hw, C, th, latents, nimg, c->st, 4, th_sub));
  return 0;
}

#include "api_loops.inc"

}  // extern "C"
