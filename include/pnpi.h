/*
 * pnpi.h -- C ABI of libpnpi.so: the MI355X (gfx950) implementation of PnPInversion's direct-inversion +
 * Prompt-to-Prompt hot path.  Plain pointers and sizes only; no C++ / torch types cross this boundary.
 *
 * The reference (cure-lab/PnPInversion) is pure Python and has no FFI of its own; its "operator API" for this path is the
 * duck-typed pipeline object used by the modules under models/p2p/.  Each entry point below names the reference interface it
 * replaces (file:line in /root/reference).  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative pnpi_status otherwise; pnpi_last_error() gives the message.
 *   - all tensor arguments are DEVICE pointers to contiguous memory unless the name ends in _host.
 *   - public layouts are the reference's: latents / eps fp32 NCHW, context fp32 [rows,77,768], images uint8 HWC.
 *   - all work is enqueued on the HIP stream given to pnpi_create(); nothing synchronises the device.
 *   - one pnpi_ctx per (process, GPU); a ctx is not thread-safe.
 *   - UNet batch-row convention (models/p2p/p2p_guidance_forward.py:108,170; inversion.py:305,382), per image:
 *       rows_per_image = 4 : [uncond_src, uncond_tgt, cond_src, cond_tgt]   (controllers act on rows 2,3 only)
 *       rows_per_image = 1 : DDIM inversion (cond_src only)
 */
#ifndef PNPI_H
#define PNPI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pnpi_ctx pnpi_ctx;

typedef enum {
  PNPI_OK = 0,
  PNPI_EINVAL = -1,  /* bad argument */
  PNPI_ESHAPE = -2,  /* unsupported shape / configuration */
  PNPI_EHIP = -3,    /* HIP runtime error */
  PNPI_ESTATE = -4,  /* call sequence error (e.g. weights not loaded) */
  PNPI_ENOMEM = -5
} pnpi_status;

/* Architecture of the Stable-Diffusion-1.x UNet / VAE (diffusers UNet2DConditionModel / AutoencoderKL constructor args,
 * models/edict/my_diffusers/models/unet_2d_condition.py:57-82, vae.py:508-519).  SD-1.x: see pnpi_config_sd1(). */
typedef struct {
  int in_channels, out_channels;   /* 4, 4 */
  int n_blocks;                    /* 4 */
  int block_out_channels[4];       /* 320, 640, 1280, 1280 */
  int block_has_attn[4];           /* 1, 1, 1, 0  (CrossAttnDownBlock2D x3, DownBlock2D) */
  int layers_per_block;            /* 2 */
  int heads;                       /* 8  (diffusers' "attention_head_dim") */
  int cross_dim;                   /* 768 */
  int ctx_len;                     /* 77 */
  int sample_size;                 /* 64 (latent H = W) */
  int norm_groups;                 /* 32 */
  int n_train_timesteps;           /* 1000 */
  int vae_in_channels;             /* 3 */
  int vae_latent_channels;         /* 4 */
  int vae_n_blocks;                /* 4 */
  int vae_block_out_channels[4];   /* 128, 256, 512, 512 */
  int vae_layers_per_block;        /* 2 */
  int vae_norm_groups;             /* 32 */
  /* CLIP text encoder (transformers CLIPTextModel: hidden = cross_dim, positions = ctx_len); clip_layers = 0: not built */
  int clip_layers;                 /* 12 */
  int clip_heads;                  /* 12 */
  int clip_intermediate;           /* 3072 */
  int clip_vocab;                  /* 49408 */
} pnpi_model_config;

void pnpi_config_sd1(pnpi_model_config* cfg);

typedef struct {
  const char* name;   /* diffusers state-dict key prefixed with "unet." or "vae."; transformers CLIPTextModel key (with or
                         without its "text_model." prefix) prefixed with "clip." */
  const void* data;   /* device pointer, contiguous, PyTorch layout ([out,in,kh,kw] / [out,in] / [n]) */
  int dtype;          /* 0 = fp32, 1 = fp16 */
  int ndim;
  int64_t shape[4];
} pnpi_named_tensor;

/* Declarative Prompt-to-Prompt controller (one per image).  Replaces the per-layer Python callback
 * controller(attn, is_cross, place_in_unet) of models/p2p/attention_control.py:44,178-190 for the controller classes
 * AttentionStore (:214), AttentionReplace (:301), AttentionRefine (:317), AttentionReweight (:338) and LocalBlend (:95).
 * All pointers are HOST pointers; tables are copied at the call. */
typedef struct {
  int kind;                        /* 0 = none / AttentionStore (no effect on the output), 1 = Prompt-to-Prompt edit,
                                      2 = MasaCtrl mutual self-attention (models/masactrl/masactrl.py:14-72) */
  int n_alpha_rows;                /* rows of cross_alpha (num_steps + 1 = 51) */
  const float* cross_alpha_host;   /* [n_alpha_rows][77]  get_time_words_attention_alpha, utils/utils.py:117-135 */
  const float* mapper_host;        /* [77][77] source-token w -> target-token j weights (Replace: seq_aligner.py:152-185;
                                      Refine: one-hot of mapper[j]==w, seq_aligner.py:107-118; Reweight alone: identity) */
  const float* alphas_host;        /* [77] Refine blend weights (1 for Replace)            attention_control.py:319-321 */
  const float* equalizer_host;     /* [77] Reweight scales (1 if none)                     attention_control.py:84-92,343 */
  int self_replace_lo, self_replace_hi;  /* num_self_replace = (0, 30)                     attention_control.py:295-297 */
  int self_replace_max_tokens;     /* 1024 (32**2)                                          attention_control.py:259 */
  int lb_enabled;                  /* LocalBlend                                            attention_control.py:95-147 */
  int lb_start;                    /* start_blend = int(0.2 * steps) = 10 */
  float lb_threshold;              /* 0.3 */
  const float* lb_alpha_host;      /* [2][77] alpha_layers one-hot rows (src prompt, tgt prompt) */
  int masa_start_step;             /* kind 2: steps >= start_step (4) ...                   masactrl.py:36,61 */
  int masa_start_layer;            /* ... and transformer blocks >= start_layer (10, execution order 0..15): the target rows'
                                      self-attention reads K and V of the source row of their CFG half (masactrl.py:63-69) */
  const float* lb_sub_alpha_host;  /* LocalBlend substruct_words: [2][77] substruct_layers one-hot rows, or NULL (none).  The blend mask
                                      becomes mask & ~mask_sub, mask_sub = the same maps weighted by these rows, NOT max-pooled, thresholded
                                      at lb_threshold_sub                                    attention_control.py:97-106,114-116,134-143 */
  float lb_threshold_sub;          /* th[1] = 0.3 */
  /* kind 2 with explicit lists (MutualSelfAttentionControl(layer_idx=, step_idx=), masactrl.py:24-37: membership tests at :61).  Both
   * optional; when given they REPLACE the corresponding window above. */
  unsigned masa_layer_mask;        /* bit b set: transformer block b (execution order 0..15) is in layer_idx; 0 = the start_layer window.
                                      Bit 31 = "a list was given": alone it is the EMPTY list (no block matches, control off) */
  int masa_n_steps;                /* length of masa_step_on_host; 0 = the start_step window (an empty step_idx list: one 0 byte) */
  const unsigned char* masa_step_on_host;   /* [masa_n_steps]: 1 where the denoising step is in step_idx (steps past the end: off) */
} pnpi_ctrl_desc;

/* Reconstruction guidance of the proximal-guidance loop (models/p2p/proximal_guidance_forward.py:48-51,60-72 with
 * DDIMSchedulerDev.step's ref_image / recon_lr / recon_mask branch, models/p2p/scheduler_dev.py:68-76): at the steps with
 * (recon_t > 0 and t < recon_t) or (recon_t < 0 and t > -recon_t) the predicted x0 is pulled towards the encoded source image where
 * the (shrunk) CFG difference is not above the proximal threshold:  mask_edit = dilate(|delta| > thr, kernel 2*dilate_mask+1);
 * pred_x0 -= recon_lr * (pred_x0 - ref_image) * (1 - mask_edit).  Only meaningful with prox != 0. */
typedef struct {
  uint32_t struct_size;            /* = sizeof(pnpi_recon_desc), set by the caller: the struct grew a field in round 5 and may grow again; an
                                      entry point answers any other value with PNPI_EINVAL instead of reading past what the caller filled */
  const float* ref_image;          /* device [nimg][4][h][w]: image_enc_latent (0.18215 * VAE posterior mean of the source image) */
  float recon_lr;
  int recon_t;
  int dilate_mask;                 /* radius of the max-pool dilation of mask_edit; 0 = none */
  /* inversion guidance (proximal_guidance_forward.py:73-75): inv_x_stars = the inversion trajectory x*_0 .. x*_nsteps, device fp32
   * [nsteps+1][nimg][4][h][w] (nullable = off); at step i inside the recon_t window the step's result is pulled towards
   * x*_{nsteps-1-i} outside the edit mask with recon_lr.  ref_image may then be NULL (no pred-x0 pull).  pnpi_cfg_ddim_prev (level 1,
   * one step, no step index): inv_x_stars points at THIS step's x*_{t-1}, [nimg][4][h][w].
   * recon_lr: the pred-x0 pull runs for recon_lr > 0 only (scheduler_dev.py:68), the inversion pull for any recon_lr != 0 (the
   * reference applies `latents - recon_lr * (...)` unconditionally inside the window, proximal_guidance_forward.py:75). */
  const float* inv_x_stars;
} pnpi_recon_desc;

typedef struct {
  uint64_t unet_sample_forwards;   /* number of UNet batch rows evaluated (x 803.27 GFLOP each for SD-1.x) */
  uint64_t unet_calls;
  uint64_t vae_encodes, vae_decodes;
  double executed_gemm_flops;      /* 2*M*N*K over every MFMA GEMM/conv launch, padding included */
  double executed_attn_flops;
  uint64_t text_kv_rows;           /* context rows whose 16 cross-attention K / V projections were computed by a precompute (2.95 GFLOP
                                      each for SD-1.x); a forward that reads the cache does NOT execute them: its sample-forward is
                                      803.27 - 2.95 GFLOP */
  uint64_t unet_sample_forwards_cached_kv;   /* of unet_sample_forwards, the rows that read the text K / V cache */
  uint64_t unet_backward_rows;     /* reverse walks (d loss / d context through one UNet row: null-text / null-latent inversion); the
                                      recording forward of each is counted in unet_sample_forwards */
  uint64_t unet_dedup_prefix_rows; /* rows the text-independent UNet prefix ran on in forwards that deduplicated it (tuning "cfg_dedup":
                                      one per distinct latent of the launch); forwards without deduplication add nothing.  Under
                                      "src_share" the distinct latents of the logical rows (rows served, as unet_sample_forwards) */
  uint64_t unet_shared_rows;       /* tuning "src_share": of unet_sample_forwards, the rows that were NOT launched because another row of
                                      the same launch computes them bit for bit (pnpi_direct_edit: 4 * nimg per step at npass = 2).
                                      unet_sample_forwards, unet_sample_forwards_cached_kv and unet_dedup_prefix_rows count rows served;
                                      rows launched = unet_sample_forwards - unet_shared_rows */
} pnpi_counters;

/* ---- lifetime ------------------------------------------------------------------------------------------------ */
/* replaces StableDiffusionPipeline.from_pretrained(...).to(device)             models/p2p_editor.py:23-25 */
int pnpi_create(pnpi_ctx** out, const pnpi_model_config* cfg, int device, void* hip_stream, int max_unet_rows, int max_vae_images);
/* A further context on the SAME packed weights (same device, same model configuration): own stream, workspaces and caches, the
 * parent's weight arena borrowed read-only instead of copied (several images in flight on one GPU: one 1.9 GB arena in the caches
 * instead of N).  The arena is reference-counted: it is freed by the last pnpi_destroy among the parent and its children, in whatever
 * order they are destroyed.  A failed pnpi_create / pnpi_create_shared leaves a context in *out that only pnpi_last_error and
 * pnpi_destroy accept (call both).  Reloading the parent's weights while children exist is the caller's error
 * (call pnpi_mark_all_loaded on each child afterwards); pnpi_load_weights on a child fails with PNPI_ESTATE.  There is no
 * counterpart in the reference (one pipeline object per process, models/p2p_editor.py:18-25). */
int pnpi_create_shared(pnpi_ctx** out, pnpi_ctx* parent, void* hip_stream, int max_unet_rows, int max_vae_images);
void pnpi_destroy(pnpi_ctx* ctx);
const char* pnpi_last_error(const pnpi_ctx* ctx);
int pnpi_load_weights(pnpi_ctx* ctx, const pnpi_named_tensor* tensors, int n);
int pnpi_missing_weights(const pnpi_ctx* ctx, char* names_out, size_t cap);   /* returns count of unloaded slots */
/* packed fp16/fp32 weight arena, for the one start-up RCCL broadcast */
int pnpi_weight_arena(pnpi_ctx* ctx, void** ptr, size_t* bytes);
/* receiving ranks of that broadcast call this instead of pnpi_load_weights */
int pnpi_mark_all_loaded(pnpi_ctx* ctx);
/* DDIMScheduler tables: alphas_cumprod[n_train] (fp32) and final_alpha_cumprod    models/p2p_editor.py:18-22 */
int pnpi_set_scheduler(pnpi_ctx* ctx, const float* alphas_cumprod_host, int n_train, float final_alpha_cumprod);
int pnpi_get_counters(const pnpi_ctx* ctx, pnpi_counters* out);
int pnpi_reset_counters(pnpi_ctx* ctx);

/* Per-kernel-class timing with HIP events on the ctx stream (used by bench.py for the `roofline` object).
 * Between begin and end every kernel launch of the graph executor is bracketed by two events. */
enum { PNPI_KC_IGEMM128 = 0, PNPI_KC_IGEMM64 = 1, PNPI_KC_IGEMM64_SPLITK = 2, PNPI_KC_ATTN_FLASH = 3, PNPI_KC_ATTN_EDIT = 4,
       PNPI_KC_GROUPNORM = 5, PNPI_KC_LAYERNORM = 6, PNPI_KC_GEGLU = 7, PNPI_KC_SOFTMAX = 8, PNPI_KC_IGEMM_WIDE = 9 /* 128x320, 128x256 tiles */,
       PNPI_KC_COUNT = 10 };
typedef struct {
  uint64_t launches;
  double total_ms;      /* sum of per-launch durations */
  double flops;         /* algorithmic FLOPs (2*M*N*K of the logical problem, head padding excluded for attention) */
  double bytes;         /* algorithmic HBM bytes for the bandwidth-bound classes */
} pnpi_kernel_stats;
int pnpi_profile_begin(pnpi_ctx* ctx);
int pnpi_profile_end(pnpi_ctx* ctx, pnpi_kernel_stats* out /* [PNPI_KC_COUNT] */);

/* Matrix-pipe clock calibration for bench.py's `clock` object (no reference counterpart: it protects the one number the driver times):
 * every SIMD issues `iters` x 16 v_mfma_f32_32x32x16_f16 back to back (2 waves per SIMD, register operands, pseudo-random values), timed
 * with HIP events on the ctx stream; *ghz_out = matrix-pipe cycles / elapsed = the clock the part holds under a pure MFMA load. */
int pnpi_clock_probe(pnpi_ctx* ctx, int iters, float* ghz_out, float* ms_out /* nullable */);

/* ---- level 1: operator boundary (keeps the loops under models/p2p/ usable unmodified) ---------------------------- */
/* model.unet(latents, t, encoder_hidden_states=context)["sample"]    inversion.py:273, p2p_guidance_forward.py:109 */
int pnpi_unet_forward(pnpi_ctx* ctx, const float* latents, int rows, int rows_per_image, int t, const float* context,
                      const pnpi_ctrl_desc* ctrl_host /* nullable, [rows/4] */, int cur_step, float* eps_out);
/* Level-1 fallback for attention controllers the library has no descriptor for: the hooked attention forward of
 * models/p2p/attention_control.py:20-47 executed literally.  While a callback is set, every attention site of pnpi_unet_forward
 * materialises attn = softmax(q k^T * scale) as fp32 [rows*heads][Nq][Nk] (rows outer, heads inner: the reference's
 * reshape_heads_to_batch_dim order) in `attn_buf`, calls cb -- which may rewrite the tensor in place with device work on the
 * library's stream, as `attn = controller(attn, is_cross, place_in_unet)` does -- and then forms out = attn v.  place: 0 down,
 * 1 mid, 2 up; layer: attention site 0..31 in call order.  A non-zero return from cb aborts the forward (PNPI_ESTATE).  Slow by
 * construction (score tensors in HBM, one GEMM pair per (row, head)); the fused descriptor path is the product path.
 * cb = NULL restores the fused path.  attn_buf must hold, for the largest site, rows*heads*Nq*Nk floats + Nq*round_up(Nk, 8) halfs. */
typedef int (*pnpi_attn_callback)(void* user, float* attn, int rows, int heads, int Nq, int Nk, int is_cross, int place, int layer);
int pnpi_set_attention_callback(pnpi_ctx* ctx, pnpi_attn_callback cb, void* user, float* attn_buf, size_t attn_buf_bytes);
/* Cross-attention keys / values of the 16 transformer blocks for `rows` context rows (device fp32 [rows][77][768]); they depend on
 * the text only (CrossAttention.to_k / to_v on encoder_hidden_states, my_diffusers/models/attention.py:230-234, evaluated by the
 * reference inside every one of its 650 UNet calls per image).  pnpi_unet_forward(..., context = NULL, ...) then reads the cache
 * (rows must match); the level-2 loops below precompute it themselves once per loop and drop it at their end (a loop call
 * therefore also invalidates a cache filled here). */
int pnpi_text_kv_precompute(pnpi_ctx* ctx, const float* context, int rows);
/* controller.step_callback -> LocalBlend.__call__ (attention_control.py:108-121,253-256) for level-1 drivers:
 * latents [nimg][2][4][h][w] updated in place, using the maps accumulated by the preceding pnpi_unet_forward calls */
int pnpi_local_blend(pnpi_ctx* ctx, float* latents, int nimg, int step_index);
/* model.vae.encode(x)['latent_dist'].mean  (x fp32 NCHW in [-1,1])                     utils/utils.py:78 */
int pnpi_vae_encode(pnpi_ctx* ctx, const float* x_nchw, int n, int height, int width, float* mean_out);
/* model.vae.decode(z)['sample']                                                        utils/utils.py:61 */
int pnpi_vae_decode(pnpi_ctx* ctx, const float* z_nchw, int n, int lat_h, int lat_w, float* sample_out);
/* image2latent: uint8 HWC -> 0.18215 * mean                                             utils/utils.py:68-80 */
int pnpi_image2latent(pnpi_ctx* ctx, const uint8_t* img_hwc, int n, int height, int width, float* z_out);
/* latent2image: decode(z / 0.18215) -> (x/2+.5).clamp(0,1)*255 -> uint8 HWC              utils/utils.py:58-66 */
int pnpi_latent2image(pnpi_ctx* ctx, const float* z_nchw, int n, int lat_h, int lat_w, uint8_t* img_hwc_out);
/* DirectInversion.next_step (inversion.py:262-270): alpha values are taken from the scheduler table */
int pnpi_ddim_next_step(pnpi_ctx* ctx, const float* eps, int t, int step_ratio, const float* sample, size_t n, float* out);
/* DirectInversion.prev_step (inversion.py:247-260) == DDIMSchedulerDev.step (scheduler_dev.py:38-95), eta = 0 */
int pnpi_ddim_prev_step(pnpi_ctx* ctx, const float* eps, int t, int step_ratio, const float* sample, size_t n, float* out);
/* DDIMSchedulerDev.step with the reconstruction pull          models/p2p/scheduler_dev.py:68-76
 * (kwargs ref_image / recon_lr / recon_mask): pred_x0 -= recon_lr * (pred_x0 - ref_image) [* recon_mask] between the step's two halves.
 * ref_image / recon_mask are device fp32 arrays of the sample's shape (the caller expands them), recon_mask and pred_x0_out nullable. */
int pnpi_ddim_prev_step_recon(pnpi_ctx* ctx, const float* eps, int t, int ratio, const float* sample, size_t n, const float* ref_image,
                              float recon_lr, const float* recon_mask, float* out, float* pred_x0_out);
/* fused CFG + prev_step + direct-inversion offset (inversion.py:383-389; p2p_guidance_forward.py:110-114).
 *   eps [nimg][2R][E]; x [nimg][R][E]; target (nullable) [nimg][E] -> offset_out = (target - prev) * offset_scale (1 on
 *   the paper's path; the not_full / skip_step ablations scale or zero it, inversion.py:491-492,512-515), x_out = prev + offset;
 *   else noise_loss (nullable) [nimg][R][E] added to the first offset_rows rows. */
int pnpi_cfg_ddim_prev(pnpi_ctx* ctx, const float* eps, const float* x, int nimg, int rows_per_img, size_t row_elems,
                       float guidance_scale, int t, int step_ratio, const float* noise_loss, int offset_rows,
                       const float* target, float offset_scale, float* offset_out, float* x_out,
                       const float* prox_threshold /*[nimg] device, nullable*/, int prox /*0 none, 1 l0, 2 l1*/,
                       const pnpi_recon_desc* recon /* nullable; applied when its recon_t window contains t */);
/* threshold of the proximal-guidance step (proximal_guidance_forward.py:41,53): torch.quantile(|eps_c - eps_u|, q) with the
 * default linear interpolation over the rows of each image; eps [nimg][2R][E] -> thr_out [nimg] (device) */
int pnpi_prox_threshold(pnpi_ctx* ctx, const float* eps, int nimg, int rows_per_img, size_t row_elems, float quantile,
                        float* thr_out);

/* model.text_encoder(input_ids)[0] (inversion.py:290-306, p2p_guidance_forward.py:151-164): transformers CLIPTextModel
 * last_hidden_state.  ids: device int32 [n][ctx_len]; out: fp32 [n][ctx_len][cross_dim].  Needs the "clip." weights; the UNet /
 * VAE entry points do not. */
int pnpi_text_encode(pnpi_ctx* ctx, const int32_t* input_ids, int n, float* hidden_out);

/* ---- CLIP similarity (evaluation/matrics_calculator.py:290-302: torchmetrics CLIPScore("openai/clip-vit-large-patch14") on
 * uint8(img * mask)) ---------------------------------------------------------------------------------------------------------
 * The image tower (transformers CLIPVisionTransformer), visual_projection and text_projection attached to a context that has the
 * text tower: pnpi_model_config, pnpi_create and the shared weight arena are untouched, the tower's weights, tables and workspaces
 * are an allocation of their own, freed by pnpi_destroy.  Weights arrive through pnpi_load_weights under the prefix "clipv." with
 * transformers CLIPModel keys: vision_model.embeddings.{class_embedding, patch_embedding.weight, position_embedding.weight},
 * vision_model.pre_layrnorm.* (upstream's spelling), vision_model.encoder.layers.N.*, vision_model.post_layernorm.*,
 * visual_projection.weight, text_projection.weight.  Neither pnpi_missing_weights nor the UNet / VAE entry points look at them; the
 * entry points below name every missing one in pnpi_last_error.  pnpi_mark_all_loaded does not mark them (they are not in the arena).
 * Every entry point refuses, with a status and a message and before anything is launched: no tower attached (PNPI_ESTATE), missing
 * weights (PNPI_ESTATE), n outside 1 .. max_images (PNPI_EINVAL), an S other than a square side with image_size <= S <= 8192
 * (PNPI_ESHAPE), a mask byte other than 0 / 1 (PNPI_EINVAL; the masks are read back to the host for this check). */
typedef struct {
  int struct_size;                 /* = sizeof(pnpi_clipv_config), set by pnpi_clipv_config_vitl14 / the caller; a mismatch is PNPI_EINVAL */
  int image_size;                  /* 224 */
  int patch;                       /* 14 */
  int width;                       /* 1024 */
  int layers;                      /* 24 */
  int heads;                       /* 16 */
  int intermediate;                /* 4096 */
  int proj_dim;                    /* 768 */
} pnpi_clipv_config;
void pnpi_clipv_config_vitl14(pnpi_clipv_config* cfg);
/* PNPI_ESTATE if the context has no text tower (clip_layers = 0) or already has an image tower */
int pnpi_clipv_attach(pnpi_ctx* ctx, const pnpi_clipv_config* cfg, int max_images);
/* CLIPModel.get_image_features of CLIPProcessor(images): img_hwc device uint8 [n][S][S][3], mask_hw nullable device uint8 [n][S][S]
 * (0 / 1, broadcast over the channels: uint8(img * mask) first); PIL's Image.resize(BICUBIC) to image_size (antialiased two-pass
 * filter in PIL's 22-bit fixed point, a uint8 rounding after each pass: bit-exact), / 255, CLIP mean / std; patch embedding, class
 * token, positions, pre_layrnorm, the encoder layers, post_layernorm on the class token, visual_projection.
 * embed_out device fp32 [n][proj_dim], not normalised. */
int pnpi_clip_image_embed(pnpi_ctx* ctx, const uint8_t* img_hwc, const uint8_t* mask_hw, int n, int S, float* embed_out);
/* CLIPModel.get_text_features: the text tower's output (final LayerNorm included) at each row's EOS position -- the FIRST position
 * holding the row's largest id, which is argmax(input_ids) of transformers for CLIP's vocabulary (EOS = vocab - 1) -- through
 * text_projection.  input_ids device int32 [n][ctx_len]; embed_out device fp32 [n][proj_dim]. */
int pnpi_clip_text_embed(pnpi_ctx* ctx, const int32_t* input_ids, int n, float* embed_out);
/* CLIPScore per pair: score_out[i] = max(100 * cos(image_i, text_i), 0), device fp32 [n] */
int pnpi_clip_score(pnpi_ctx* ctx, const uint8_t* img_hwc, const uint8_t* mask_hw, const int32_t* input_ids, int n, int S, float* score_out);
/* kernel-level: the preprocessing alone, to out_size (a multiple of the attached tower's patch, <= S).  resized_out (nullable) device
 * uint8 [n][out][out][3]: what PIL's resize gives; patches_f16_out (nullable) device fp16 [n][(out / patch)^2][Kp], Kp = 3 * patch^2
 * rounded up to a multiple of 64: the normalised pixels as patch rows in the patch-embedding weight's (c, ky, kx) order, pad columns
 * zero.  Needs no weights. */
int pnpi_op_clip_preprocess(pnpi_ctx* ctx, const uint8_t* img_hwc, const uint8_t* mask_hw, int n, int S, int out_size,
                            uint8_t* resized_out, void* patches_f16_out);
/* Host-only, no context: the per-output-pixel tables the preprocessing kernels apply for in_size -> out_size (both passes use the same
 * table for square images), as PIL's precompute_coeffs + normalize_coeffs_8bpc give them for BICUBIC.  Returns ksize (taps reserved per
 * output pixel; 1 for in_size == out_size, where PIL copies) or PNPI_ESHAPE for out_size > in_size or in_size > 8192; bounds_out
 * (nullable) [out_size][2] = (first source index, taps used), coef_out (nullable) [out_size][ksize] 22-bit fixed point.  Call once with
 * NULLs for ksize.  One pass: acc = 2^21 + sum_j src[first + j] * coef[j];  out = clamp(acc >> 22, 0, 255). */
int pnpi_clip_resize_tables(int in_size, int out_size, int* bounds_out, int* coef_out);

/* ---- DINO structure distance (evaluation/matrics_calculator.py:385-405 -> LossG.calculate_global_ssim_loss :237-246 ->
 * VitExtractor.get_keys_self_sim_from_input(layer_num = 11) :154-171, dino_vitb8) ---------------------------------------------
 * The DINO ViT (facebookresearch/dino vision_transformer.py) attached to a context, which needs nothing else: no text tower, no UNet
 * rows, no VAE images.  Weights, tables and workspaces are an allocation of their own, freed by pnpi_destroy; a context that never
 * attaches is unchanged.  Weights arrive through pnpi_load_weights under the prefix "dino." with DINO's own state-dict keys: cls_token,
 * pos_embed, patch_embed.proj.{weight, bias}, blocks.N.{norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2}.{weight, bias}, norm.*.
 * The metric reads the output of the LAST block's attn.qkv: of that block only norm1 and the K third of attn.qkv (rows width ..
 * 2 * width - 1) are computed; its other tensors and the final norm.* have no slot -- they are accepted and dropped, neither missing
 * nor an error.  pnpi_missing_weights, pnpi_mark_all_loaded and the UNet / VAE entry points do not look at "dino." slots.
 * Preprocessing is the reference's: uint8 image (* 0 / 1 mask) as float 0..255, NOT divided by 255; torchvision 0.13's Resize on a tensor =
 * two-tap bilinear, align_corners = False, no antialiasing; Normalize(ImageNet mean, std) on those 0..255 values.
 * Every entry point refuses, with a status and a message and before anything is launched: nothing attached (PNPI_ESTATE), a second
 * attach (PNPI_ESTATE), missing weights (PNPI_ESTATE, every name), n out of range (PNPI_EINVAL), an S outside 16 .. 8192
 * (PNPI_ESHAPE), a mask byte other than 0 / 1 (PNPI_EINVAL; the masks are read back to the host), a NULL output (PNPI_EINVAL). */
typedef struct {
  int struct_size;                 /* = sizeof(pnpi_dino_config), set by pnpi_dino_config_vitb8 / the caller; a mismatch is PNPI_EINVAL */
  int image_size;                  /* 224 */
  int patch;                       /* 8 */
  int width;                       /* 768 */
  int layers;                      /* 12 */
  int heads;                       /* 12 */
  int intermediate;                /* 3072 */
} pnpi_dino_config;
void pnpi_dino_config_vitb8(pnpi_dino_config* cfg);
/* up to max_pairs image pairs (2 * max_pairs images) per call */
int pnpi_dino_attach(pnpi_ctx* ctx, const pnpi_dino_config* cfg, int max_pairs);
/* the concatenated keys of the last block: img_hwc device uint8 [n][S][S][3], mask_hw nullable device uint8 [n][S][S];
 * keys_out device fp32 [n][T][width], T = (image_size / patch)^2 + 1; n <= 2 * max_pairs */
int pnpi_dino_keys(pnpi_ctx* ctx, const uint8_t* img_hwc, const uint8_t* mask_hw, int n, int S, float* keys_out);
/* calculate_structure_distance for n pairs, n <= max_pairs: one tower pass over the 2 n images, one fused distance launch set.
 * dist_out device fp32 [n]: mean over T^2 of (sim_pred - sim_gt)^2, sim[i][j] = k_i . k_j / max(|k_i| |k_j|, 1e-8). */
int pnpi_structure_distance(pnpi_ctx* ctx, const uint8_t* img_pred, const uint8_t* mask_pred, const uint8_t* img_gt, const uint8_t* mask_gt,
                            int n, int S, float* dist_out);
/* kernel-level: the preprocessing alone, to out_size (a multiple of the attached tower's patch).  resized_f32_out (nullable) device
 * fp32 [n][3][out][out], the resized 0..255 values; patches_f16_out (nullable) device fp16 [n][(out / patch)^2][3 * patch^2], the
 * normalised values as patch rows in the patch-embedding weight's (c, ky, kx) order.  Needs no weights. */
int pnpi_op_dino_preprocess(pnpi_ctx* ctx, const uint8_t* img_hwc, const uint8_t* mask_hw, int n, int S, int out_size,
                            float* resized_f32_out, void* patches_f16_out);
/* kernel-level: the fused self-similarity distance of n pairs of given key matrices, device fp16 [n][T][D], D % 32 == 0, 16-byte
 * aligned; needs no attached tower.  dist_out device fp32 [n]; sim_a_out (nullable) device fp32 [n][T][T]: the map of keys_a, written
 * by the debug variant of the same tile body.  The two maps of the distance never reach memory; the reduction order is fixed. */
int pnpi_op_keys_selfsim_mse(pnpi_ctx* ctx, const void* keys_a_f16, const void* keys_b_f16, int n, int T, int D, float* dist_out,
                             float* sim_a_out);
/* Host-only, no context: the taps of the resize for in_size -> out_size per output index, by PyTorch's fp32 arithmetic
 * (area_pixel_compute_source_index, align_corners = False): src = max(scale * (o + 0.5) - 0.5, 0), scale = in / out;
 * idx0 = min(floor(src), in - 1), idx1 = idx0 + (idx0 < in - 1), lambda = weight of idx1 = clamp(src - idx0, 0, 1); the weight of
 * idx0 is 1 - lambda in fp32.  in_size == out_size: idx0 = idx1 = o, lambda = 0.  Each output nullable, [out_size].
 * Returns 0, or PNPI_ESHAPE for sizes outside 1 .. 8192. */
int pnpi_dino_resize_taps(int in_size, int out_size, int* idx0_out, int* idx1_out, float* lambda_out);

/* ---- LPIPS, SqueezeNet backbone (evaluation/matrics_calculator.py:324-342 -> torchmetrics
 * LearnedPerceptualImagePatchSimilarity(net_type = "squeeze")) ------------------------------------------------------------------
 * torchvision's squeezenet1_1().features 0 .. 12 and the seven 1 x 1 `lin` layers attached to a context, which needs nothing else: no
 * text tower, no UNet rows, no VAE images.  Weights and workspaces are an allocation of their own, freed by pnpi_destroy; a context
 * that never attaches is unchanged.  Weights arrive through pnpi_load_weights under the prefix "lpips.": torchvision's keys
 * features.0.{weight, bias}, features.N.{squeeze, expand1x1, expand3x3}.{weight, bias} for N in 3, 4, 6, 7, 9, 10, 11, 12, and
 * lin0.weight .. lin6.weight ([1][C][1][1], no bias).  pnpi_missing_weights, pnpi_mark_all_loaded and the UNet / VAE entry points do
 * not look at "lpips." slots.
 * Computed per image: x = ((uint8 / 255) * mask) * 2 - 1 (a cleared pixel is -1), (x - shift) / scale with shift (-.030, -.088, -.188),
 * scale (.458, .448, .450), no resize; seven taps = the outputs of features 1, 4, 7, 9, 10, 11, 12 (64, 128, 256, 384, 384, 512, 512
 * channels; the max pools are ceil_mode).  Per pair and tap: a^ = a / sqrt(1e-8 + sum_c a_c^2) per pixel (torchmetrics >= 1.0's form:
 * the eps under the root), d = sum_c w_c (a^_c - b^_c)^2, the tap's term is the mean of d over the pixels; the score is the sum of the
 * seven terms.  Activations are fp16, sums fp32; reductions run in a fixed order (the same call twice gives the same bits) and every
 * convolution takes the tile of its max_pairs form (a pair's score does not depend on the batch it is in).
 * Every entry point refuses, with a status and a message and before anything is launched: nothing attached (PNPI_ESTATE), a second
 * attach (PNPI_ESTATE), missing weights (PNPI_ESTATE, every name), n out of range (PNPI_EINVAL), an S outside 17 .. 8192 (PNPI_ESHAPE;
 * below 17 the third max pool has no window), a mask byte other than 0 / 1 (PNPI_EINVAL; the masks are read back to the host), a NULL
 * output (PNPI_EINVAL).  The workspaces are sized for 512 x 512 images at attach and grow at the first call with a larger S. */
/* up to max_pairs image pairs (2 * max_pairs images) per call; a refused attach leaves nothing behind */
int pnpi_lpips_attach(pnpi_ctx* ctx, int max_pairs);
/* LPIPS of n pairs, n <= max_pairs: one pass of the network over the 2 n images, then the seven fused tap distances.  img_* device
 * uint8 [n][S][S][3], mask_* nullable device uint8 [n][S][S]; score_out device fp32 [n] */
int pnpi_lpips(pnpi_ctx* ctx, const uint8_t* img_pred, const uint8_t* mask_pred, const uint8_t* img_gt, const uint8_t* mask_gt, int n, int S,
               float* score_out);
/* one tap's feature map (tests): out_f32 device fp32 [n][H_tap][H_tap][C_tap] (NHWC), tap 0 .. 6; n <= 2 * max_pairs.
 * H_0 = (S - 3) / 2 + 1; each ceil-mode pool: H -> ceil((H - 3) / 2) + 1, one less if that window would start outside the map */
int pnpi_lpips_features(pnpi_ctx* ctx, const uint8_t* img_hwc, const uint8_t* mask_hw, int n, int S, int tap, float* out_f32);
/* kernel-level: one tap's distance for n pairs of given feature maps, device fp16 [n][HW][C], C % 8 == 0 (else PNPI_ESHAPE), 16-byte
 * aligned; w device fp32 [C], any sign; needs no attached network.  out device fp32 [n].  The normalised maps never reach memory. */
int pnpi_op_lpips_layer(pnpi_ctx* ctx, const void* a_f16, const void* b_f16, const float* w, int n, int HW, int C, float* out);
/* kernel-level: MaxPool2d(3, stride 2, ceil_mode = True) on device fp16 NHWC [n][H][H][C] -> [n][Ho][Ho][C], overhanging windows clipped
 * to the map; C % 8 == 0, H >= 2, 16-byte aligned; needs no attached network */
int pnpi_op_maxpool3s2_ceil(pnpi_ctx* ctx, const void* x_f16, int n, int H, int C, void* out_f16);

/* ---- level 2: loop boundary (whole phases device-resident, no host round trip per step) ------------------------- */
/* DirectInversion.ddim_loop (inversion.py:308-319): latents_out [nsteps+1][nimg][4][h][w]; timesteps_host = scheduler.timesteps */
int pnpi_ddim_invert(pnpi_ctx* ctx, const float* z0, int nimg, const float* ctx_cond /*[nimg][77][768]*/, int nsteps,
                     const int* timesteps_host, float* latents_out);
/* DirectInversion.offset_calculate (inversion.py:375-391): noise_loss_out [nsteps][nimg][2][4][h][w] */
int pnpi_offset_calculate(pnpi_ctx* ctx, const float* ddim_latents /*[nsteps+1][nimg][...]*/, int nimg,
                          const float* context4 /*[nimg][4][77][768]*/, int nsteps, const int* timesteps_host,
                          float guidance_scale, const float* offset_scale_host /*[nsteps], nullable = all 1*/,
                          float* noise_loss_out);
/* DirectInversion.ddim_with_guidance_scale_loop (inversion.py:334-347): DDIM inversion under classifier-free guidance
 * (the directinversion+p2p_guidance_<inv>_<fwd> methods); uncond / cond rows share one launch per step */
int pnpi_ddim_invert_cfg(pnpi_ctx* ctx, const float* z0, int nimg, const float* ctx_uncond /*[nimg][77][768]*/,
                         const float* ctx_cond, float guidance_scale, int nsteps, const int* timesteps_host,
                         float* latents_out);
/* direct_inversion_p2p_guidance_forward (p2p_guidance_forward.py:135-173) incl. controller + LocalBlend:
 * latents_out [nimg][2][4][h][w].  ctrl_host: nullable or [nimg].
 * prox 1 ('l0') / 2 ('l1'): the proximal-guidance step of proximal_guidance_forward.py:39-64 -- the CFG difference is
 * soft-thresholded at quantile `quantile` of its magnitude over the image's two rows (torch.quantile, linear); a
 * quantile <= 0 means the fixed threshold -quantile.  prox 0: plain CFG.  recon (nullable): reconstruction guidance. */
int pnpi_edit_loop(pnpi_ctx* ctx, const float* x_T /*[nimg][4][h][w]*/, int nimg, const float* context4,
                   const float* noise_loss /*[nsteps][nimg][2][...], nullable*/, int offset_rows,
                   const pnpi_ctrl_desc* ctrl_host, int nsteps, const int* timesteps_host, float guidance_scale,
                   int prox, float quantile, const pnpi_recon_desc* recon, float* latents_out);

/* The denoising half of P2PEditor.edit_image_directinversion (p2p_editor.py:99-160) as ONE loop: offset_calculate
 * (inversion.py:375-391) and npass direct_inversion_p2p_guidance_forward passes (p2p_guidance_forward.py:135-173; the
 * reference runs an AttentionStore reconstruction pass and the edit pass) advance in lock step, one UNet launch of
 * (1 + npass) * 4 * nimg rows per timestep.  ctrl_host: nullable or [npass][nimg] (kind 0 = no attention edit).
 * noise_loss_out [nsteps][nimg][2][4][h][w]; latents_out [npass][nimg][2][4][h][w].
 * Tuning "src_share" (pnpi_set_tuning): the source rows of the guidance passes repeat the offset pass's bit for bit and are launched
 * once -- (4 + 2 npass) * nimg rows per step; outputs, layouts and unet_sample_forwards are unchanged (see unet_shared_rows). */
int pnpi_direct_edit(pnpi_ctx* ctx, const float* ddim_latents /*[nsteps+1][nimg][...]*/, int nimg, const float* context4,
                     int npass, const pnpi_ctrl_desc* ctrl_host, int offset_rows, int nsteps, const int* timesteps_host,
                     float guidance_scale, const float* offset_scale_host /*[nsteps], nullable*/, float* noise_loss_out,
                     float* latents_out);

/* The pruned-equivalent schedule (SURVEY.md 8a Note D; an algebraic reformulation of the same edit, parity-tested against the
 * faithful loops): with the direct-inversion offset the source latent of every step IS x*_{t-1}, so it is assigned from the stored
 * inversion trajectory and only [uncond_tgt, cond_src, cond_tgt] are evaluated -- one 3-row UNet launch per step and image, 200
 * sample-forwards per image instead of 650.  latents_out [nimg][2][4][h][w] = (x*_0, edited latent). */
int pnpi_direct_edit_pruned(pnpi_ctx* ctx, const float* ddim_latents, int nimg, const float* context4,
                            const pnpi_ctrl_desc* ctrl_host /* nullable or [nimg] */, int nsteps, const int* timesteps_host,
                            float guidance_scale, float* latents_out);

/* ---- edit-friendly DDPM inversion (models/edit_friendly_ddm/inversion_utils.py, eta > 0) ------------------------------------------
 * Latents fp32 [.][4][h][w], E = 4*h*w.  The per-step scalars are the reference's 0-dim fp32 expressions in its order (get_variance
 * :91-98, :157-168, :190-206); every element-wise op is rounded separately as in eager PyTorch, so the level-1 kernels are bit-exact
 * against the reference's formulas given the same eps.
 * One deviation: at a step whose variance is exactly 0 (t = 0 when ab_prev == ab[t], i.e. set_alpha_to_one=False) the reference divides
 * by zero and its xts[0] is NaN; here z = 0 and xts[0] keeps x0.  Neither value is read by anything (zs[0] is zeroed at :173-174). */
/* the host scalars of one step, no context: out6 = [sqrt(ab_t), sqrt(1-ab_t), sqrt(ab_prev), sqrt(1-ab_prev-eta*var), eta*sqrt(var), var]
 * with ab_prev = alphas_cumprod[t - step_ratio] (final_alpha below 0) */
int pnpi_ef_step_scalars(const float* alphas_cumprod, int n, float final_alpha, int t, int step_ratio, float eta, float* out6);
/* sample_xts_from_x0 (:31-55): xts_out[1 + k] = x0 * sqrt(ab[t]) + noise[k] * sqrt(1 - ab[t]) for the k-th draw, t = timesteps_host[nsteps-1-k]
 * (the reference draws in reversed(timesteps) order).  noise [nsteps][nimg][E], xts_out [nsteps+1][nimg][E]; level 0 is not written. */
int pnpi_ef_sample_xts(pnpi_ctx* ctx, const float* x0, int nimg, const float* noise, size_t row_elems, int nsteps,
                       const int* timesteps_host, float* xts_out);
/* one step of inversion_forward_process (:151-171): eps [nimg][2][E] (uncond, cond; cfg != 0) or [nimg][1][E] (cfg == 0: prompt ""),
 * xt = xts[idx+1], xprev = xts[idx] (overwritten with the corrected mu + sigma z), z_out = zs[idx].  eta <= 0 is PNPI_EINVAL. */
int pnpi_ef_noise_map(pnpi_ctx* ctx, const float* eps, int cfg, float cfg_scale, const float* xt, float* xprev, float* z_out, int nimg,
                      size_t row_elems, int t, int step_ratio, float eta);
/* reverse_step (:179-208) after the per-row CFG of :254-258: eps [nimg][2P][E] (P uncond rows, then P cond rows), x / out [nimg][P][E]
 * (may alias), z [nimg][E] (one noise map per image, every prompt row), cfg_scales_host [P], P = nprompts in {1, 2}.  eta <= 0 adds no
 * noise (:203). */
int pnpi_ef_reverse_step(pnpi_ctx* ctx, const float* eps, const float* x, const float* z, int nimg, int nprompts, size_t row_elems,
                         const float* cfg_scales_host, int t, int step_ratio, float eta, float* out);
/* inversion_forward_process(model, x0, etas, prompt, cfg_scale) (:100-176), device-resident: xts_out [nsteps+1][nimg][E] (level 0 = x0),
 * zs_out [nsteps][nimg][E] (zs[0] = 0).  noise [nsteps][nimg][E] = the draws in the reference's order; etas_host [nsteps] indexed like
 * the reference's etas[idx] (all > 0).  One UNet launch of nimg x [uncond, cond] rows per step (uncond only when ctx_cond is NULL). */
int pnpi_ef_invert(pnpi_ctx* ctx, const float* x0, int nimg, const float* noise, const float* ctx_uncond /*[nimg][77][768]*/,
                   const float* ctx_cond /*[nimg][77][768], nullable: prompt ""*/, float cfg_scale, const float* etas_host, int nsteps,
                   const int* timesteps_host, float* xts_out, float* zs_out);
/* inversion_reverse_process(model, xT, etas, prompts, cfg_scales, zs, controller) (:210-262), device-resident, over the last nsteps_run of
 * the nsteps_total timesteps: step k uses zs[nsteps_run-1-k] and etas_host[nsteps_run-1-k] (etas_host [nsteps_total]).
 * xT [nimg][E] (every prompt row starts there), zs [nsteps_run][nimg][E], context [nimg][2*nprompts][77][768] (nprompts uncond rows, then
 * nprompts cond rows), cfg_scales_host [nprompts], ctrl_host nullable or [nimg] (needs nprompts == 2, no LocalBlend; step index from 0),
 * latents_out [nimg][nprompts][E].  One UNet launch of 2 * nprompts * nimg rows per step. */
int pnpi_ef_edit(pnpi_ctx* ctx, const float* xT, const float* zs, int nimg, int nprompts, const float* context,
                 const float* cfg_scales_host, const pnpi_ctrl_desc* ctrl_host, const float* etas_host, int nsteps_run, int nsteps_total,
                 const int* timesteps_host, float* latents_out);

/* ---- Blended Latent Diffusion (run_editing_blended_latent_diffusion.py: BlendedLatnetDiffusion) -------------------------------
 * Mask-guided editing with one prompt: after every CFG + DDIM step the latent outside the user's mask is replaced by the source latent
 * noised to the step's own level t (edit_image :127-139).  Latents fp32 (the reference keeps fp16); random draws are inputs.
 * pnpi_bld_mask: _read_mask (:164-173) for n full-resolution uint8 masks [n][H][W] -> fp32 0/1 [n][h][w], h = w = the context's latent size:
 * PIL NEAREST (source pixel floor((i + 0.5) * H / h)), then `< 0.5 -> 0, else 1` (non-zero -> 1). */
int pnpi_bld_mask(pnpi_ctx* ctx, const uint8_t* mask_u8, int n, int H, int W, float* mask_out);
/* one step (:127-139) for nimg images in one launch: eps [nimg][2][row_elems] (uncond, cond), x / src / noise / x_out [nimg][row_elems] (x_out
 * may be x), mask [nimg][map_elems] fp32 0/1 indexed by e % map_elems (row_elems % map_elems == 0).
 *   e = eu + g (ec - eu);  prev = DDIMScheduler.step(e, t, x) with prev_t = t - step_ratio (final_alpha_cumprod below 0);
 *   noised = sqrt(ab[t]) src + sqrt(1 - ab[t]) noise  (add_noise at t, not prev_t);  x_out = prev * mask + noised * (1 - mask). */
int pnpi_bld_step(pnpi_ctx* ctx, const float* eps, const float* x, const float* src, const float* noise, const float* mask, int nimg,
                  size_t row_elems, size_t map_elems, float guidance_scale, int t, int step_ratio, float* x_out);
/* the loop of edit_image (:110-139), device-resident, over the last nsteps_run of the nsteps_total timesteps (timesteps[int(n * blending_
 * percentage):]): x_start [nimg][E] the N(0,1) start latents (:102-106), src [nimg][E] = 0.18215 * posterior mean of the source images,
 * noise [nsteps_run][nimg][E] the blending draws in step order (:137), mask [nimg][h*w] (pnpi_bld_mask), ctx_uncond / ctx_cond
 * [nimg][77][768], latents_out [nimg][E].  One UNet launch of 2 * nimg rows per step, text K / V cached for the loop.  2 * nimg >
 * max_unet_rows, nsteps_run outside 1 .. nsteps_total (PNPI_EINVAL) and arena overflow are refused before anything is launched. */
int pnpi_bld_edit(pnpi_ctx* ctx, const float* x_start, int nimg, const float* src, const float* noise, const float* mask,
                  const float* ctx_uncond, const float* ctx_cond, float guidance_scale, int nsteps_total, int nsteps_run,
                  const int* timesteps_host, float* latents_out);

/* ---- Plug-and-Play (run_editing_pnp.py: PNP, register_conv_control_efficient, register_attention_control_efficient) -----------
 * Feature and self-attention injection from a source row.  Every UNet launch holds three rows per image, [source latent of this level, x,
 * x] on the contexts ["", negative prompt, target prompt]; classifier-free guidance runs over rows 1 and 2 and the source row is never
 * stepped.  Latents and the step arithmetic are fp32 (the reference runs an fp16 pipeline).
 * pnpi_pnp_desc: which steps and which sites inject.  conv_site: decoder ResNet in execution order (up block i, layer j ->
 * i * (layers_per_block + 1) + j), -1 = none: after conv2 and before the shortcut add, rows 1 and 2 take row 0's hidden states
 * (:276-281).  qk_block_mask: bit b = transformer block b in execution order (down 0 .., mid, up ..): rows 1 and 2 take row 0's q and k
 * in its self-attention and keep their own v (:190-201), at every token count.  conv_steps / qk_steps: the number of LEADING steps that
 * inject (init_pnp :371-375: scheduler.timesteps[:n]). */
typedef struct pnpi_pnp_desc {
  uint32_t struct_size;            /* = sizeof(pnpi_pnp_desc), set by the caller (as pnpi_recon_desc); a mismatch is PNPI_EINVAL */
  int conv_steps;
  int qk_steps;
  int conv_site;
  uint32_t qk_block_mask;
} pnpi_pnp_desc;
size_t pnpi_pnp_desc_sizeof(void);
/* The reference's sites and schedule, derived from the model's structure (host only, no context): conv_site = the second ResNet of the
 * first decoder level that has attention (up_blocks[1].resnets[1] at SD-1.x), qk_block_mask = every decoder transformer block but the
 * first of that level (res_dict :231; blocks 8 .. 15 at SD-1.x), conv_steps = int(nsteps * 0.8), qk_steps = int(nsteps * 0.5)
 * (run_pnp :386-387).  PNPI_ESHAPE when the decoder has no such level. */
int pnpi_pnp_desc_default(const pnpi_model_config* cfg, int nsteps, pnpi_pnp_desc* out);
/* level 1, denoise_step :363-368 for nimg images in one launch: eps [nimg][3][row_elems] (row 0 unread), x / x_out [nimg][row_elems] (x_out
 * may be x):  e = e1 + g (e2 - e1);  x_out = DDIMScheduler.step(e, t, x) with prev_t = t - step_ratio (final_alpha_cumprod below 0), eta 0.
 * Bit-exact against eager fp32 PyTorch. */
int pnpi_pnp_step(pnpi_ctx* ctx, const float* eps, const float* x, int nimg, size_t row_elems, float guidance_scale, int t, int step_ratio,
                  float* x_out);
/* level 1: ONE forward of 3 * nimg rows [img][source, x, x] with a given injection state (the hooked UNet of denoise_step :361):
 * latents / eps_out [nimg][3][E], context [nimg][3][77][768], conv_on / qk_on: does desc's conv site / do desc's blocks inject in this
 * forward.  With conv_on the injected ResNet's norm1 -> conv1 -> norm2 -> conv2 run on the nimg source rows only (the other rows' results
 * would be overwritten) and pnpi_counters.executed_gemm_flops is lower by exactly that work.  3 * nimg > max_unet_rows, a wrong
 * struct_size and a site outside the model are refused before anything is launched. */
int pnpi_unet_forward_pnp(pnpi_ctx* ctx, const float* latents, int nimg, int t, const float* context, const pnpi_pnp_desc* desc,
                          int conv_on, int qk_on, float* eps_out);
/* level 2, PNP.sample_loop :393-396, device-resident for nimg images: src_latents [nsteps][nimg][E] the source latent of every step IN
 * STEP ORDER (step i is the reference's noisy_latent[-1 - i]), x_start [nimg][E] (noisy_latent[-1]), context [nimg][3][77][768],
 * timesteps_host [nsteps] (with steps_offset: 981, 961, .., 1), latents_out [nimg][E].  Step i injects at the conv site while
 * i < desc->conv_steps and in the q/k blocks while i < desc->qk_steps.  One UNet launch of 3 * nimg rows and one pnpi_pnp_step launch
 * per step, no host round trip, text K / V projected once.  3 * nimg > max_unet_rows, nsteps <= 0, a wrong struct_size, a site outside the
 * model and arena overflow are refused before anything is launched. */
int pnpi_pnp_edit(pnpi_ctx* ctx, const float* src_latents, const float* x_start, int nimg, const float* context, const pnpi_pnp_desc* desc,
                  int nsteps, const int* timesteps_host, float guidance_scale, float* latents_out);

/* ---- InstructPix2Pix (run_editing_instructpix2pix.py: CFGDenoiser around k-diffusion's CompVisDenoiser, sample_euler_ancestral) ------
 * The same UNet graph with an 8-channel conv_in (pnpi_model_config.in_channels = 8, out_channels = 4): input [z * c_in | image latent],
 * rows [img][edit text + image, null text + image, null text + zero image], a FRACTIONAL timestep (k-diffusion's sigma_to_t).
 * Step scalars: 6 host floats per step [sigma, sigma_down - sigma, sigma_up, c_in, t, sigma_next > 0 ? 1 : 0], evaluated by the caller in
 * the reference's fp32 order (pnpinversion_amd/instructpix2pix.py: step_table).
 *
 * level 1: pnpi_unet_forward (no controller) at a float timestep 0 <= t <= n_train - 1.  The sinusoid row is evaluated as the context's
 * table is (fp64 -> fp32, cos half first; the reference multiplies in fp32), so an integer t reproduces pnpi_unet_forward bit for bit; the
 * per-timestep bias cache is neither read nor filled.  latents [rows][in_channels][h][w], eps_out [rows][out_channels][h][w]. */
int pnpi_unet_forward_t(pnpi_ctx* ctx, const float* latents, int rows, float t, const float* context, float* eps_out);
/* level 1, one launch for nimg images: eps [nimg][3][row_elems], z / noise / image / z_out [nimg][row_elems] (z_out may be z):
 *   den_k = z + eps_k * (-sigma);  den = den_2 + cfg_text * (den_0 - den_1) + cfg_image * (den_1 - den_2);
 *   d = (z - den) / sigma;  z_out = z + d * (sigma_down - sigma);  z_out += noise * sigma_up  (only when sc6_host[5] != 0: noise is not
 *   read otherwise and may be NULL).  in_next (nullable) [nimg][2][2 * row_elems]: the next launch's two distinct inputs per image,
 *   [z_out * c_in_next | image] and [z_out * c_in_next | 0].  Bit-exact against eager fp32 PyTorch. */
int pnpi_ip2p_step(pnpi_ctx* ctx, const float* eps, const float* z, const float* noise, const float* image, int nimg, size_t row_elems,
                   float cfg_text, float cfg_image, const float* sc6_host, float c_in_next, float* z_out, float* in_next);
/* level 2, edit_instruct_pix2pix's sampler (:125-134), device-resident for nimg images: z0 [nimg][E] = randn * sigmas[0], image [nimg][E]
 * the VAE encoder's posterior mean (NOT scaled by 0.18215), noise [nsteps][nimg][E] the draws in step order, context [nimg][3][77][768] =
 * [edit, null, null], scalars_host [nsteps][6], z_out [nimg][E], trajectory_out (nullable) [nsteps][nimg][E] z after every step;
 * E = 4 h w.  One UNet launch of 3 * nimg rows on 2 * nimg distinct inputs (tuning "cfg_dedup" runs the text-independent prefix once per
 * input) and one pnpi_ip2p_step launch per step, no host round trip, text K / V projected once.  3 * nimg > max_unet_rows, a context whose
 * in_channels != 8 or out_channels != 4, nsteps <= 0, a scalar out of range and arena overflow are refused before anything is launched. */
int pnpi_ip2p_edit(pnpi_ctx* ctx, const float* z0, const float* image, const float* noise, int nimg, const float* context, float cfg_text,
                   float cfg_image, int nsteps, const float* scalars_host, float* z_out, float* trajectory_out);

/* ---- InstructDiffusion (run_editing_instructdiffusion.py: the same UNet function, sampler and step scalars as InstructPix2Pix) --------
 * Rows [img][edit text + image, null text + image, edit text + zero image] (CFGDenoiser :37-48): the two distinct 8-channel inputs and the
 * input map are InstructPix2Pix's, the third row pairs the zero image with the EDIT text, and the combine is symmetric around the mean of
 * the two single-condition rows:
 *   den = 0.5 * (den_1 + den_2) + cfg_text * (den_0 - den_1) + cfg_image * (den_0 - den_2)      summed left to right
 * level 1, pnpi_ip2p_step with that combine: same arguments, same refusals, the same move after it, bit-exact against eager fp32 PyTorch. */
int pnpi_instdiff_step(pnpi_ctx* ctx, const float* eps, const float* z, const float* noise, const float* image, int nimg, size_t row_elems,
                       float cfg_text, float cfg_image, const float* sc6_host, float c_in_next, float* z_out, float* in_next);
/* level 2, instruct_diffusion_edit's sampler (:110-120), device-resident: pnpi_ip2p_edit's arguments with context [nimg][3][77][768] =
 * [edit, null, edit], the same launches per step (the compact prefix of "cfg_dedup" applies unchanged) and the same refusals. */
int pnpi_instdiff_edit(pnpi_ctx* ctx, const float* z0, const float* image, const float* noise, int nimg, const float* context, float cfg_text,
                       float cfg_image, int nsteps, const float* scalars_host, float* z_out, float* trajectory_out);

/* ---- kernel-level entry points (used by tests/ and bench.py to exercise single kernels) ------------------------- */
int pnpi_op_conv(pnpi_ctx* ctx, const void* x1_nhwc_f16, const void* x2_nhwc_f16, int C1, int C2, int B, int H, int W,
                 int ksize, int stride, int pad, int upsample, int Ho, int Wo, const void* w_f16 /*[N][k*k*(C1+C2)]*/,
                 const float* bias, const void* residual_f16, int N, void* out_nhwc_f16, int force_cfg, int force_split);
/* pnpi_op_conv + the per-(m-tile, channel) (sum, sum of squares) partials its epilogue produces for the consumer GroupNorm
 * (replaces the statistics pass of torch.nn.GroupNorm, my_diffusers/models/resnet.py:296): stats_out [ceil(M/tile_rows)][N][2]
 * fp32 over the stored fp16 values; *tile_rows_out = rows per m-tile, 0 if this launch configuration produced none. */
int pnpi_op_conv_stats(pnpi_ctx* ctx, const void* x1_nhwc_f16, const void* x2_nhwc_f16, int C1, int C2, int B, int H, int W,
                       int ksize, int stride, int pad, int upsample, int Ho, int Wo, const void* w_f16, const float* bias,
                       const void* residual_f16, int N, void* out_nhwc_f16, int force_cfg, int force_split, float* stats_out,
                       int* tile_rows_out);
/* process-wide kernel tuning knobs: variant A/B inside one process (tools/fwd_ab.py, tools/fwd_tune.py) and tests of non-default
 * variants.  One table holds them all -- key, built-in default, accepted range, the environment variable that seeds it, one-line
 * description: PNPI_TUNING_KNOBS in pnpinversion_amd/csrc/tuning.h -- and pnpi_tuning_info enumerates it.  The environment is read once,
 * when the library is loaded; a variable whose value the knob does not accept leaves the built-in default.
 * pnpi_set_tuning: PNPI_EINVAL for an unknown key or a value outside the knob's range (the knob keeps its value).
 * pnpi_get_tuning: the current value; PNPI_EINVAL for an unknown key.
 * pnpi_tuning_info: row `index` of the table (0, 1, ... until PNPI_EINVAL): its key, its value at load (`initial`: the built-in default,
 * or what the environment variable gave) and its current value; each pointer is nullable.
 * pnpi_reset_tuning: every knob back to its value at load.
 * All four are host-only and need no context.  The knobs are plain process globals read by every context's launches: set them while no
 * other thread is inside a pnpi_* call (the product never sets one; several contexts on several threads --
 * P2PEditor.edit_stream_in_flight -- only READ them).  A non-zero "igemm_vpp" / "igemm_sched" / "attn_pipe" and "igemm_v128" /
 * "igemm_v320" = 11, 12, 15 select ablation instances that exist only in a library built with
 * `python -m pnpinversion_amd.build --ablations` (-DPNPI_ABLATIONS=1 -> csrc/libpnpi_ablations.so, loaded with PNPI_LIBRARY=<path>); the
 * product library REJECTS those values with PNPI_EINVAL instead of silently timing the default kernel.
 * "ff_fold" (1): each transformer block's ff2 GEMM and 1x1 proj_out run as one launch over folded weights [Wp W2 | Wp] derived at load
 * (same FLOPs, no hs3 round trip; fp16-rounding-level difference); 0 = the two launches.  May be switched on a live context.
 * "cfg_dedup" (1): in the loops that feed one latent to several UNet rows (classifier-free guidance: its unconditional and its
 * conditional row), everything before the first cross-attention -- conv_in, the first ResNet, the first transformer block up to its
 * cross-attention query -- runs once per distinct latent and is expanded to the rows of the launch there (behind the ResNet at steps
 * where that block's self-attention redirects rows).  1 = the compact launches choose their own tiles (fp16-rounding-level difference
 * where the choice differs), 2 = they are pinned to the tile / split-K of the full-row launch (bit-identical to 0), 0 = off.  Other
 * values are rejected.  pnpi_unet_forward and one-row loops are not affected.  May be switched on a live context.
 * "src_share" (1): pnpi_direct_edit launches each step's three bit-identical copies of the unconditional and of the conditional source
 * row (offset, reconstruction and edit pass) once and expands the prediction to the logical rows behind the UNet.  1 = the compact
 * launch chooses its own tiles (fp16-rounding-level difference where the choice differs), 2 = every GEMM is configured as at the logical
 * row count (bit-identical to 0), 0 = off.  The call falls back to 0 by itself with offset_rows < 1, a controller kind other than
 * 0 / 1 / 2, under a host attention callback, or on a recording context (one that holds the activation tape of
 * pnpi_unet_context_grad / the null-text loops: such a context keeps the full launch for every later call) -- the counter
 * unet_shared_rows then stays put; under 1 the full launch of a recording context is configured as the compact launch would be, so the
 * context gives the same bits as one without a tape.  Other values are rejected.
 * May be switched on a live context.
 * Keys (tests/test_tuning_host.py holds this list against the table): "text_kv", "temb_cache", "ff_fold", "cfg_dedup", "src_share",
 * "attn_aug", "attn_vt_perm", "attn_bwd_flash", "op_attention_aug", "op_gemm_vt_perm16", "op_attention_vt_perm", "gn_nofuse";
 * "igemm_dma", "igemm_v128", "igemm_v64", "igemm_v256", "igemm_v320", "igemm_v256n", "igemm_wide", "v128_bk64_tiles", "tile_order",
 * "igemm_force_cfg", "igemm_force_split", "igemm_bias_init", "igemm_sched", "igemm_vpp", "igemm_tapin", "igemm_pp_only_n",
 * "igemm_pp_only_k", "igemm_pp_only_m", "igemm_deep_rings", "igemm_vt_lds", "igemm_res_late", "igemm_table", "igemm_table_near",
 * "pp_rowtile"; "gn_inline_rows", "gn_small_max", "gn_small_min", "gn_wide_below"; "attn_pipe", "attn_nodma", "attn_ksq4",
 * "attn_noaug", "abf_prefetch". */
int pnpi_set_tuning(const char* key, int value);
int pnpi_get_tuning(const char* key, int* value);
int pnpi_tuning_info(int index, const char** key, int* initial, int* current);
int pnpi_reset_tuning(void);
/* Host-only query of the measured tile table launch_igemm consults before its cost model (no device work; used by the CPU tests):
 * returns 1 for an exact {M, N, K, ksize} entry, 2 when the same layer (N, K, ksize) is listed at another row count and the entry
 * nearest in M (at most 4x away) is used, 0 for none; cfg / split / entry_m (each nullable) receive the entry. */
int pnpi_tile_table_lookup(int M, int N, int K, int ksize, int* cfg, int* split, int* entry_m);
/* Host-only: the row height launch_igemm gives a ping-pong launch (tuning "pp_rowtile" = 1).  cfg names the tile the table chose
 * (16 = 256 x 256, 17 = 192 x 320; 19 = 128 x 320 and 20 = 192 x 256 name the same two families), M the LAUNCHED row count, split the
 * split-K factor.  Returns the rows of the tile that runs (256, 192 or 128): the family's shorter tile when it needs no more rounds
 * of one workgroup per CU on 256 CUs than the taller one; 0 when cfg is no ping-pong tile. */
int pnpi_pp_rowtile_query(int cfg, int M, int N, int split);
/* Host-only: everything launch_igemm decides for one launch -- tile, split-K, ring / variant, epilogue, grid, statistics -- without
 * launching: selection is a pure function of this description and the tuning knobs (no context, no device).  The description is
 * of a GEMM of M rows (a convolution's B * Ho * Wo): ksize 1 or 3, K = ksize^2 (C1 + C2), leading dimensions in elements; bias /
 * residual / stats are presence flags (bias_aligned16: the bias pointer is 16-byte aligned); vt_col0 >= N: no transposed columns;
 * rows_per_batch >= 1, nbatch >= 1; ws_bytes: split-K workspace (0: none); force_cfg -1 / force_split 0 / sel_M 0: the launcher
 * chooses, at the launched M.  The plan: err is 0 or launch_igemm's rejection (-2 ... -10; id -1: rejected before a tile was chosen,
 * stats_tile_rows -1: before the statistics were decided); id / split: tile id and split-K; variant / sparse: the tile's tuning
 * variant (ring depth folded in for ids 0 / 1) and 2 / 1 / 0 for at most one / two / more blocks per CU; bm x bn tiles on a
 * gx x gy x gz grid; epi_lds / bias_init / res_late / k_order: the epilogue flags the kernel gets; stats: requested statistics are
 * produced, stats_tile_rows rows per partial; cls: the kernel class pnpi_profile_end counts the launch in; dma 0: register-staged
 * fallback kernel (fastk: its 64-channel fast path); instance: the kernel instance that runs, an index for
 * pnpi_igemm_instance_info (-1: err was set before one was chosen). */
typedef struct {
  int M, N, K, ksize, C1, C2, ldx1, ldx2, ldw, ldo, ldres;
  int bias, bias_aligned16, residual, geglu, stats;
  int vt_col0, vt_ld, vt_f32, rows_per_batch, vt_perm16;
  int nbatch;
  long long ws_bytes;
  int force_cfg, force_split, sel_M;
} pnpi_igemm_launch_desc;
typedef struct {
  int err, id, split, kchunks_per_split;
  int variant, sparse;
  int bm, bn, gx, gy, gz;
  int vt_col0;
  int epi_lds, bias_init, res_late, k_order;
  int stats, stats_tile_rows, cls;
  int dma, fastk;
  int instance;
} pnpi_igemm_plan;
int pnpi_igemm_plan_query(const pnpi_igemm_launch_desc* desc, pnpi_igemm_plan* plan);
/* Host-only: row `index` (0, 1, ...) of the table of kernel instances launch_igemm can run, which a plan's `instance` indexes.  name:
 * "dma<BM,BN,BKT,NST[,wgmW][,kgK]>" (LDS-DMA kernel: tile, K step, ring stages; wave groups per k-group if not 2; k-groups if not 1),
 * "pp<BM,BN>" (ping-pong kernel), "v1<BM,BN,fast|generic>" (register-staged kernel); ablation instances add ",ablA".  geom7: the
 * seven integers the profiling records carry for a launch of it (the LDS-DMA kernel's BM, BN, BKT, NST, WGM, ABL, WK; the ping-pong
 * kernel's BM, BN, MI0, NI0, ABL, 0, -1; all 0 for the register-staged kernel).  ablation_only: the row exists in a `build --ablations`
 * library only.  Each output is nullable.  Returns PNPI_EINVAL past the end of the table. */
int pnpi_igemm_instance_info(int index, const char** name, int* geom7, int* ablation_only);
/* Host-only: the row maps of pnpi_direct_edit's shared-row launch ("src_share") for nimg images and npass guidance passes.  Logical row
 * 4 (p nimg + im) + k is row k of [unc_src, unc_tgt, cond_src, cond_tgt] of pass p (0 = the offset pass) of image im, on the logical
 * latent 2 (p nimg + im) + k % 2.  Outputs (each nullable): lsel [compact latent] -> logical latent, cmap [compact row] -> compact latent,
 * cctx [compact row] -> context4 row, omap [logical row] -> compact row, and the two counts ((4 + 2 npass) nimg rows on (2 + npass) nimg
 * latents, per image O0 O1 O2 O3 then the two target rows of every guidance pass). */
int pnpi_src_share_maps(int nimg, int npass, int* lsel, int* cmap, int* cctx, int* omap, int* compact_rows, int* compact_latents);
int pnpi_op_gemm(pnpi_ctx* ctx, const void* a_f16, int lda, const void* w_f16, int ldw, int M, int N, int K, float alpha,
                 const float* bias, const void* residual_f16, void* out_f16, int ldo, int vt_col0, void* outT,
                 int vt_ld, int vt_f32, int rows_per_batch, int force_cfg, int force_split);
/* out[m][j] = x * gelu(gate) with the N = 2*I weight rows / bias packed as [x(32) | gate(32)] groups (fused GEGLU epilogue) */
int pnpi_op_gemm_geglu(pnpi_ctx* ctx, const void* a_f16, int lda, const void* w_f16, int ldw, int M, int N, int K,
                       const float* bias, void* out_f16, int ldo);
int pnpi_op_groupnorm(pnpi_ctx* ctx, const void* x1, const void* x2, int C1, int C2, int B, int HW, int groups, float eps,
                      const float* gamma, const float* beta, int silu, void* out);
/* The GroupNorm the UNet forward runs behind a convolution that handed over its statistics: no statistics pass, st1 / st2 are the
 * per-(m-tile, channel) partials pnpi_op_conv_stats wrote for x1 / x2 ([B * HW / rows][C][2] fp32, batch item b's tiles from
 * b * HW / rows on; rows1 / rows2 the producers' tile_rows_out; st2 / rows2 ignored without x2).  PNPI_ESHAPE, with `out`
 * untouched, where the forward would recompute the statistics instead: rows <= 0, HW % rows != 0 or more than 256 tiles per item.
 * Tensors small enough for the one-launch kernel of pnpi_op_groupnorm (groups of C / G % 4 == 0 channels and at most 24576 elements
 * per item) take it and ignore the partials, as in the forward. */
int pnpi_op_groupnorm_stats(pnpi_ctx* ctx, const void* x1, const void* x2, int C1, int C2, int B, int HW, int groups, float eps,
                            const float* gamma, const float* beta, int silu, void* out, const float* st1, int rows1,
                            const float* st2, int rows2);
int pnpi_op_layernorm(pnpi_ctx* ctx, const void* x, int M, int C, float eps, const float* gamma, const float* beta, void* out);
int pnpi_op_geglu(pnpi_ctx* ctx, const void* x, int M, int inner, void* out);
int pnpi_op_softmax_rows(pnpi_ctx* ctx, void* x, int M, int N, int ld);
/* kernel-level: launchers that no other entry point reaches on their own.  softmax_rows_f32: in place over [M][N] contiguous fp32 rows
 * (the materialised attention scores of the controller call-back and of the backward).  f32_rows_to_f16_padded: in [M][N] fp32 -> out
 * [M][ld] fp16, columns N .. ld zero (ld >= N).  gemv: out[n] = bias[n] + bias2[n] + sum_k act(x[k]) w[n][k] with x fp32 [K], w fp16
 * [N][K], act = SiLU where silu_in != 0, K % 8 == 0; bias and bias2 nullable (the time-embedding MLP).  M, N, K <= 0: PNPI_EINVAL, as in
 * pnpi_op_geglu and pnpi_op_softmax_rows. */
int pnpi_op_softmax_rows_f32(pnpi_ctx* ctx, float* x, int M, int N);
int pnpi_op_f32_rows_to_f16_padded(pnpi_ctx* ctx, const float* in, int M, int N, int ld, void* out_f16);
int pnpi_op_gemv(pnpi_ctx* ctx, const float* x, int K, const void* w_f16, int N, const float* bias, const float* bias2, int silu_in,
                 float* out);
/* Activation-gradient kernels of the null-text / null-latent path (NullInversion.null_optimization's loss.backward(), inversion.py:
 * 196-225) -- groundwork, kernel-level only (no method string reaches them yet).  fp16 tensors in the forward's layouts.
 *   layernorm_bwd: dx of torch.nn.LayerNorm from the saved input;  groupnorm_bwd: dx (dense [B][HW][C1+C2]) of GroupNorm(+SiLU) over the
 *   virtual concat (x1, x2);  geglu_bwd: d(projection) in the interleaved [x(32)|gate(32)] layout;  softmax_bwd_rows: dS = scale * P *
 *   (dP - rowsum(dP * P)) as fp16 rows padded to ld;  accumulate: dst += src;  sumpool2x2: nearest-2x upsample backward;  zero_stuff2 +
 *   repack_dgrad: stride-2 / stride-1 convolution dgrad through the forward kernel (wd[c][k*k-1-tap][n] = w[n][tap][c]);
 *   null_text_loss: mse(prev_step(cfg(eps_u, eps_c)), target) and its gradient w.r.t. eps_u (times grad_scale);  adam_step: torch.optim.Adam
 *   defaults, step k >= 1, gradient times inv_scale. */
int pnpi_op_layernorm_bwd(pnpi_ctx* ctx, const void* x, const void* dy, int M, int C, float eps, const float* gamma, void* dx);
int pnpi_op_groupnorm_bwd(pnpi_ctx* ctx, const void* x1, const void* x2, int C1, int C2, int B, int HW, int groups, float eps,
                          const float* gamma, const float* beta, int silu, const void* dy, void* dx);
/* kernel-level: the forms of these kernels that the reverse walk (tape_backward) launches.
 *   groupnorm_bwd_split: the three-phase chip-wide GroupNorm backward with the walk's two destinations: columns 0 .. C1 of the gradient go
 *   to dx1 (row stride ld1), columns C1 .. C1 + C2 to dx2 (row stride ld2); acc != 0 adds into what is there (fp32 sum, one rounding); a
 *   NULL destination is not written (the source that needs no gradient).  scratch NULL: the context's workspace; otherwise a device buffer
 *   of scratch_floats >= pnpi_op_groupnorm_bwd_scratch_floats(B, HW, groups) floats (smaller: PNPI_ESHAPE).  Needs C1 % 8 == 0,
 *   (C1 + C2) % 8 == 0, ld % 8 == 0, 256 % groups == 0.
 *   groupnorm_bwd_ref: pnpi_op_groupnorm_bwd's arguments, always the one-block-per-group kernel (the walk's fallback for C1 % 8 != 0).
 *   strided_add: dst[r][0 .. C) (+)= src[r * ld + off + 0 .. C), r < R; C, ld, off multiples of 8.
 *   pad_heads: [R][heads * dh] -> [R][heads * Dp], pad columns zero.   add_f16_to_f32: dst (fp32) += scale * src (fp16), n elements.
 *   transpose: nbatch matrices s_src / s_dst elements apart, dst[c][r] = src[r][c] for r < R, c < Cc, dst columns R .. ld_dst zero.
 *   repack_dgrad_pad: pnpi_op_repack_dgrad into wd[Cin][taps][Npad], columns N .. Npad zero (conv_out's gradient map has 8 channels). */
int pnpi_op_groupnorm_bwd_split(pnpi_ctx* ctx, const void* x1, const void* x2, int C1, int C2, int B, int HW, int groups, float eps,
                                const float* gamma, const float* beta, int silu, const void* dy, void* dx1, int ld1, int acc1, void* dx2,
                                int ld2, int acc2, float* scratch, size_t scratch_floats);
size_t pnpi_op_groupnorm_bwd_scratch_floats(int B, int HW, int groups);
int pnpi_op_groupnorm_bwd_ref(pnpi_ctx* ctx, const void* x1, const void* x2, int C1, int C2, int B, int HW, int groups, float eps,
                              const float* gamma, const float* beta, int silu, const void* dy, void* dx);
int pnpi_op_strided_add(pnpi_ctx* ctx, void* dst, const void* src, int ld, int off, size_t R, int C, int accumulate);
int pnpi_op_pad_heads(pnpi_ctx* ctx, const void* src, size_t R, int heads, int dh, int Dp, void* dst);
int pnpi_op_add_f16_to_f32(pnpi_ctx* ctx, float* dst, const void* src, size_t n, float scale);
int pnpi_op_transpose(pnpi_ctx* ctx, const void* src, int ld_src, int R, int Cc, void* dst, int ld_dst, int nbatch, long s_src, long s_dst);
int pnpi_op_repack_dgrad_pad(pnpi_ctx* ctx, const void* w, int N, int Npad, int taps, int Cin, void* wd);
int pnpi_op_geglu_bwd(pnpi_ctx* ctx, const void* h, const void* dy, int M, int inner, void* dh);
int pnpi_op_softmax_bwd_rows(pnpi_ctx* ctx, const float* P, const float* dP, int R, int N, int ld, float scale, void* dS);
int pnpi_op_accumulate(pnpi_ctx* ctx, void* dst, const void* src, size_t n);
int pnpi_op_sumpool2x2(pnpi_ctx* ctx, const void* dup, int B, int H, int W, int C, void* dx);
int pnpi_op_zero_stuff2(pnpi_ctx* ctx, const void* dy, int B, int Ho, int Wo, int C, void* out);
int pnpi_op_repack_dgrad(pnpi_ctx* ctx, const void* w, int N, int taps, int Cin, void* wd);
int pnpi_op_null_text_loss(pnpi_ctx* ctx, const float* eps_u, const float* eps_c, const float* x, const float* target, int n, float w,
                           float c_x, float c_e, float grad_scale, void* d_eps_u, float* loss);
int pnpi_op_adam_step(pnpi_ctx* ctx, float* p, float* m, float* v, const float* g, int n, int k, float lr, float inv_scale);
/* Attention backward (CrossAttention.forward of my_diffusers/models/attention.py:217-259 differentiated), materialised per (row, head):
 * q / k / v are [B*N][ld] fp16 views with head h at columns off + h * Dp (dh real columns, pad columns zero), d_o is [B*Nq][ldo] with
 * heads * dh columns; dq / dk / dv receive the gradients in the layout of q / k / v (pad columns untouched).  scratch: device memory
 * of at least pnpi_op_attention_bwd_scratch_bytes(Nq, Nk, dh) bytes. */
int pnpi_op_attention_bwd(pnpi_ctx* ctx, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* v, int ldv,
                          int v_off, const void* d_o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, int B, void* dq,
                          void* dk, void* dv, void* scratch, size_t scratch_bytes);
size_t pnpi_op_attention_bwd_scratch_bytes(int Nq, int Nk, int dh);
/* kernel-level: pnpi_op_attention_bwd handed what the recording forward left -- lse_fwd [B][heads][Nq] (fp32, log2 domain:
 * log2 sum_k 2^(scale * log2(e) * q.k)) and its output o_fwd [B*Nq][ld_ofwd].  With both (and the flash form, see "attn_bwd_flash") dQ
 * skips its first pass over the keys; either NULL: exactly pnpi_op_attention_bwd. */
int pnpi_op_attention_bwd_fwd(pnpi_ctx* ctx, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* v, int ldv,
                              int v_off, const void* d_o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, int B, void* dq,
                              void* dk, void* dv, void* scratch, size_t scratch_bytes, const float* lse_fwd, const void* o_fwd,
                              int ld_ofwd);
/* Host-only: everything pnpi_op_attention_bwd(_fwd) and the reverse walk decide for one attention site before they launch, without
 * launching -- a pure function of the shape, the scratch the caller has (scratch_bytes; < 0: as much as the form asks for, 0: none) and
 * the tuning knobs "attn_bwd_flash" / "abf_prefetch"; have_fwd: the forward's lse and O are handed over (ld_ofwd % 8 == 0).
 * flash: 1 the flash kernel attn_bwd_flash_kernel<Dp, lt, mode, pf>, 0 the materialised form (lt 0); nsplit: shares of the dK / dV walk
 * over the queries (> 1: fp32 partials and the reduce kernel), share_rows queries each (whole lt tiles), empty_shares of them beginning
 * at or past Nq; pf_dq / pf_dk / pf_dv: the register-prefetch instance per launch; one_pass: dQ from the forward's lse and O;
 * scratch_bytes: the workspace the flash form carves, or the materialised form's per head. */
typedef struct {
  int flash, lt, nsplit;
  int pf_dq, pf_dk, pf_dv;
  int one_pass, share_rows, empty_shares;
  long long scratch_bytes;
} pnpi_attn_bwd_plan;
int pnpi_attn_bwd_plan_query(int heads, int Nq, int Nk, int Dp, int dh, long long scratch_bytes, int have_fwd, pnpi_attn_bwd_plan* plan);

/* ---- differentiable UNet forward (null-text path; groundwork) ---------------------------------------------------------------
 * pnpi_unet_context_grad: eps = unet(latents [1][4][h][w], t, context [1][77][768]) with every activation recorded, then the reverse
 * walk: d_context_out [77][768] = (d eps / d context)^T d_eps for the given d loss / d eps (fp32 in the layout of eps; multiply it by
 * a power-of-two loss scale -- activation gradients travel in fp16 -- and divide d_context_out by it).  eps_out nullable.
 * pnpi_null_text_optimize: NullInversion.null_optimization (models/p2p/inversion.py:196-225) for one image: ddim_latents
 * [nsteps + 1][4*h*w] (x*_0 first), the "" and the source-prompt embeddings, the denoising timesteps; uncond_out [nsteps][77][768]
 * (the optimised embedding of every step), iters_out [nsteps] (nullable: Adam iterations run per step), losses_out_host
 * [nsteps][num_inner_steps] (nullable, host: the loss of every Adam iteration, -1 where the early stop skipped it).  Context needs
 * max_unet_rows large enough for one row's activations kept without reuse (12 is). */
/* pnpi_edit_loop with per-step unconditional embeddings uncond_steps [nsteps][nimg][77][768] (the output of pnpi_null_text_optimize):
 * p2p_guidance_forward's `uncond_embeddings[i].expand(...)` (p2p_guidance_forward.py:56-57), or with uncond_first_only the single-branch
 * variant (:92).  No direct-inversion offset, no reconstruction guidance (what the null-text method strings use). */
int pnpi_edit_loop_uncond_steps(pnpi_ctx* ctx, const float* x_T, int nimg, const float* context4, const pnpi_ctrl_desc* ctrl_host, int nsteps,
                                const int* timesteps_host, float guidance_scale, int prox, float quantile, const float* uncond_steps,
                                int uncond_first_only, float* latents_out);
/* pnpi_edit_loop_uncond_steps with the reconstruction guidance of pnpi_edit_loop (recon nullable): the edit pass of
 * P2PEditor.edit_image_null_text_inversion_proximal_guidanca(use_reconstruction_guidance=True), models/p2p_editor.py:607-627. */
int pnpi_edit_loop_uncond_steps_recon(pnpi_ctx* ctx, const float* x_T, int nimg, const float* context4, const pnpi_ctrl_desc* ctrl_host, int nsteps,
                                      const int* timesteps_host, float guidance_scale, int prox, float quantile, const float* uncond_steps,
                                      int uncond_first_only, const pnpi_recon_desc* recon, float* latents_out);
int pnpi_unet_context_grad(pnpi_ctx* ctx, const float* latents, int t, const float* context, const float* d_eps, float* eps_out,
                           float* d_context_out);
int pnpi_null_text_optimize(pnpi_ctx* ctx, const float* ddim_latents, const float* ctx_uncond, const float* ctx_cond, int nsteps,
                            const int* timesteps_host, float guidance_scale, int num_inner_steps, float epsilon, float* uncond_out,
                            int* iters_out_host, float* losses_out_host);
/* replaces DirectInversion.null_latent_calculate                               models/p2p/inversion.py:419-460
 * ("ablation_null-latent-inversion+p2p"): the null-text optimisation of the source row's unconditional embedding per step, turned into
 * per-step latent offsets noise_loss_out [nsteps][2][4*h*w] (device) for pnpi_edit_loop.  context4 = [unc_src, unc_tgt, cond_src,
 * cond_tgt]; iters_out_host [nsteps] and losses_out_host [nsteps][num_inner_steps] nullable (host; -1 = iteration not run). */
int pnpi_null_latent_calculate(pnpi_ctx* ctx, const float* ddim_latents, const float* context4, int nsteps, const int* timesteps_host,
                               float guidance_scale, int num_inner_steps, float epsilon, float* noise_loss_out, int* iters_out_host,
                               float* losses_out_host);
int pnpi_op_attention(pnpi_ctx* ctx, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* vt,
                      int ldv, void* o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale,
                      const int* rows_dev /*[nrows][4]*/, int nrows);
/* kernel-level: pnpi_op_attention with causal (non-zero: key j > query i is masked, the CLIP text encoder's launch) and lse_dev
 * (nullable; [rows][heads][Nq] fp32 indexed by the OUTPUT row of each rows_dev entry: the log2-domain log-sum-exp of the recording
 * forward).  NULL q / k / vt / o / rows_dev: PNPI_EINVAL.  pnpi_op_attention is this call with (0, NULL). */
int pnpi_op_attention_ex(pnpi_ctx* ctx, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* vt,
                         int ldv, void* o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale,
                         const int* rows_dev /*[nrows][4]*/, int nrows, int causal, float* lse_dev);
/* ---- mask-guided MasaCtrl (models/masactrl/masactrl.py:114-193, MutualSelfAttentionControlMask) --------------------------------
 * Attach nimg pairs of BINARY uint8 masks [nimg][h][w] (host pointers, values 0 / 1) to the context: from then on, at the steps and
 * blocks a kind-2 controller controls, each target row attends to its source row's K / V restricted by class -- query i sees the keys j
 * with mask_s[j] == mask_t[i], both masks resized to the block's map by F.interpolate nearest (source = floor(dst * in / out)).  That is
 * the reference's two masked passes + blend in one softmax (exact for 0 / 1 masks); a query whose class no key carries gets the mean
 * of V, as the reference's all-finfo.min softmax does.  Source rows are untouched.  The resized masks live in context-owned memory at
 * fixed addresses, rewritten by every call.  (NULL, NULL) clears the masks: plain MasaCtrl again.  Applies to pnpi_edit_loop,
 * pnpi_direct_edit (every pass) and pnpi_unet_forward.  Refused with PNPI_EINVAL and a pnpi_last_error message, before anything is
 * launched: a value other than 0 / 1, one mask without the other, nimg outside 1 .. max_unet_rows / 4 -- and, by the loop that finds
 * kind-2 controllers, masks held for another nimg than the loop's. */
int pnpi_masa_set_masks(pnpi_ctx* ctx, const uint8_t* mask_s_u8_host, const uint8_t* mask_t_u8_host, int nimg, int h, int w);
/* read back level `level`'s resized masks (side = sample_size >> level), [nimg][side][side] bytes each, to host memory (tests) */
int pnpi_masa_get_level_masks(pnpi_ctx* ctx, int level, uint8_t* mask_s_out_host, uint8_t* mask_t_out_host, int* side_out);
/* kernel-level: the nearest resize of n device masks [n][H][W] -> [n][h][w] class bytes */
int pnpi_op_masa_mask_level(pnpi_ctx* ctx, const uint8_t* in_dev, int n, int H, int W, int h, int w, uint8_t* out_dev);
/* kernel-level: pnpi_op_attention with class-restricted keys.  kcls_dev [nmask][Nk] / qcls_dev [nmask][Nq] class bytes (non-zero = 1),
 * mrow_dev [nrows]: the class row used by entry r of rows_dev.  Nk <= 16384. */
int pnpi_op_attention_masked(pnpi_ctx* ctx, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* vt,
                             int ldv, void* o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale,
                             const int* rows_dev /*[nrows][4]*/, int nrows, const uint8_t* kcls_dev, const uint8_t* qcls_dev,
                             const int* mrow_dev);
int pnpi_op_cross_edit(pnpi_ctx* ctx, const void* q, int ldq, int q_off, const void* k, int ldk, int k_off, const void* vt,
                       int ldv, void* o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale,
                       const int* pairs_dev, int npairs, const void* mmatT_f16, const float* c1, const float* c2,
                       const float* lb_alpha, float* lb_acc, int lb_slot0, int lb_nslots);
int pnpi_op_local_blend(pnpi_ctx* ctx, const float* lb_acc, int nslots, int map_hw, int lat_hw, int C, float th,
                        float* latents, int nimg);
/* The same with LocalBlend substruct_words: lb_acc holds 4 planes per slot (blend src / tgt, substruct src / tgt); the mask is
 * (blend maps pooled > th) & ~(substruct maps unpooled > th_sub)  (attention_control.py:97-118). */
int pnpi_op_local_blend_sub(pnpi_ctx* ctx, const float* lb_acc, int nslots, int map_hw, int lat_hw, int C, float th, float th_sub,
                            float* latents, int nimg);

#ifdef __cplusplus
}
#endif
#endif /* PNPI_H */
