// Host-side model description for libpnpi: weight slots, SD-1.x UNet / VAE graphs, workspace planning.
#pragma once
#include <atomic>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/pnpi.h"
#include "ops.h"

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int round_up_i(int x, int a) { return (x + a - 1) / a * a; }

// Bump allocator. With base == nullptr it only measures (dry run) and hands out fake, never-dereferenced addresses.
struct Bump {
  char* base = nullptr;
  size_t cap = 0, off = 0, peak = 0;
  bool overflow = false;
  void* alloc(size_t bytes) {
    off = align_up(off, 256);
    size_t at = off;
    off += bytes;
    if (off > peak) peak = off;
    if (base && off > cap) { overflow = true; return base; }
    return base ? (void*)(base + at) : (void*)(uintptr_t)(0x1000 + at);
  }
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
  void reset() { off = 0; }
};

struct Slot {
  int kind;      // 0 = matrix (fp16), 1 = vector (fp32)
  void* dst;
  int rows, cols, taps, dst_ld, cin_pad, row0, dh, Dp;
  int n;
  int ilv_half;  // > 0: GEGLU x/gate row interleave (groups of 32)
  bool loaded;
};

struct ConvW { half_t* w; float* b; int cin, cin_pad, cout, k; };
struct LinW { half_t* w; float* b; int in, out; };
struct NormW { float* g; float* b; int c; };

struct ResnetW {
  NormW n1, n2;
  ConvW c1, c2, sc;
  bool has_sc;
  int temb_off;   // >= 0: conv1 bias comes from the forward's bias row (UNetFlight::bias_eff) at this offset; -1: static conv1 bias
  int cin, cout;
};

struct TransformerW {
  int C, heads, dh, Dp;
  NormW gn, ln1, ln2, ln3;
  ConvW proj_in, proj_out;
  half_t* w_qkv;      // [3*heads*Dp][C]   (self-attention, heads zero-padded to Dp)
  float* b_qkv_aug;   // [3*heads*Dp] or nullptr: zeros, but 1.0 at column dh of every K head and every V head -- d = 40 heads padded to 64:
                      // the 64-wide flash kernel takes its max shift and row sum through the MFMAs with it (attn.hip, AUG)
  LinW o1;            // [C][C] + bias
  half_t* w_q2;       // [heads*Dp][C]
  half_t* w_kv2;      // [2*heads*Dp][cross_dim]
  LinW o2;
  LinW ff1;           // [8C][C]
  LinW ff2;           // [C][4C]
  ConvW fo;           // ff2 folded into proj_out (derived, C % 64 == 0 only; fo.w == nullptr otherwise): w [C][4C | C] = [Wp W2 | Wp] as a
                      // two-source 1 x 1 convolution over f2 | hs2, b [C] = Wp b2 + bp -- rebuilt whenever ff2 / proj_out are (re)loaded
  int place;          // 0 down, 1 mid, 2 up
  int lb_slot0;       // first LocalBlend slot of this layer's cross-attention, or -1
};

struct VaeAttnW {
  int C;
  NormW gn;
  half_t* w_qkv; float* b_qkv;   // [3C][C]
  LinW proj;
};

struct UNetW {
  ConvW conv_in, conv_out;
  NormW norm_out;
  LinW t1, t2;
  half_t* temb_w;     // [sumC][4*C0]
  float* temb_b;      // [sumC] time_emb_proj biases
  float* conv1_b;     // [sumC] conv1 biases
  int temb_total;
  std::vector<std::vector<ResnetW>> down_res;
  std::vector<std::vector<TransformerW>> down_attn;
  std::vector<ConvW> down_samp;     // size n_blocks-1
  ResnetW mid_res[2];
  TransformerW mid_attn;
  std::vector<std::vector<ResnetW>> up_res;
  std::vector<std::vector<TransformerW>> up_attn;
  std::vector<ConvW> up_samp;
  int lb_nslots, lb_tokens;         // LocalBlend slots (5 layers x heads) and their token count (256), 0 if unavailable
};

struct VaeW {
  // encoder
  ConvW e_conv_in, e_conv_out;
  std::vector<std::vector<ResnetW>> e_res;
  std::vector<ConvW> e_down;
  ResnetW e_mid[2];
  VaeAttnW e_attn;
  NormW e_norm_out;
  ConvW quant;       // 1x1, 2L -> 2L
  // decoder
  ConvW post_quant;  // 1x1, L -> L (stored as 8 -> 8, zero padded)
  ConvW d_conv_in, d_conv_out;
  ResnetW d_mid[2];
  VaeAttnW d_attn;
  std::vector<std::vector<ResnetW>> d_res;
  std::vector<ConvW> d_up;
  NormW d_norm_out;
};

struct ClipLayerW {
  NormW ln1{}, ln2{};
  half_t* w_qkv = nullptr; float* b_qkv = nullptr;   // [3H][H] fused q | k | v (+ biases)
  LinW out{}, fc1{}, fc2{};
};
struct ClipW {
  int H = 0, heads = 0, I = 0, vocab = 0, T = 0;
  half_t* tok = nullptr;         // [vocab][H]
  half_t* pos = nullptr;         // [T][H]
  std::vector<ClipLayerW> layers;
  NormW final_ln;
};

// What every network attached to a context owns (api_vit.inc: attach sequence, free, refusals): its allocations live outside the
// context's own arenas, so a context that never attaches one is unchanged.
struct TowerW {
  const char* name = "";                  // in messages: "CLIP image tower", "DINO ViT", "LPIPS SqueezeNet"
  const char* prefix = "";                // of its weight slots' names: "clipv.", "dino.", "lpips."
  int max_images = 0;
  Bump arena;                             // weights (own allocation)
  Bump persist, temp;                     // activation workspaces of the forward (swapped into the context while it runs)
  Bump bufs;                              // small persistent buffers
};
// What the vision transformers share on top of that: the geometry, the patch embedding, the encoder layers.
struct VitTowerW : TowerW {
  int G = 0, NP = 0, T = 0, K = 0, W = 0; // patch grid side, patches, tokens (NP + 1), patch-row length 3 * patch^2 rounded up to 64, width
  half_t* w_patch = nullptr;              // [W][K] patch embedding, (c, ky, kx) columns, pad columns zero
  float* b_patch = nullptr;               // [W], or nullptr: a bias-free patch embedding (CLIP)
  float* cls = nullptr;                   // [W]
  float* pos = nullptr;                   // [T][W]
  std::vector<ClipLayerW> layers;
  int* rows_ident = nullptr;              // [max_images][4], first in bufs
};

// CLIP image tower + the two projections (pnpi_clipv_attach; transformers CLIPModel: vision_model, visual_projection, text_projection).
struct ClipVisionW : VitTowerW {
  pnpi_clipv_config cfg;
  NormW pre_ln, post_ln;
  half_t* w_vproj = nullptr;              // [proj][W]
  half_t* w_tproj = nullptr;              // [proj][H_text]
  half_t *pool_img = nullptr, *ln_img = nullptr, *emb_img16 = nullptr, *pool_txt = nullptr, *emb_txt16 = nullptr;
  float *emb_img = nullptr, *emb_txt = nullptr;   // [max_images][proj]
  // PIL's bicubic coefficient tables per source size (built on the host at first use): bounds [out][2] = (first source index, count),
  // coef [out][ksize] 22-bit fixed point
  struct ResizeTab { int S, out, ksize; int* bounds; int* coef; };
  std::vector<ResizeTab> tabs;
  uint8_t* tmp_u8 = nullptr; size_t tmp_bytes = 0;   // the horizontal pass's output [n][S][out][3], grown on demand
};

// DINO ViT for the structure distance (pnpi_dino_attach; facebookresearch/dino vision_transformer.py).  Of the last block only ln1,
// w_qkv, b_qkv exist.
struct DinoW : VitTowerW {
  pnpi_dino_config cfg;
  int max_pairs = 0;                      // max_images = 2 * max_pairs
  half_t* keys16 = nullptr;               // [max_images][T][W]: the last block's keys
  // resize taps per source size (built on the host at first use): idx0 | idx1 [out] ints, lam [out] floats, one allocation each
  struct ResizeTab { int S, out; int* idx; float* lam; };
  std::vector<ResizeTab> tabs;
};

// SqueezeNet 1.1 features + the seven `lin` layers of LPIPS (pnpi_lpips_attach; torchvision squeezenet1_1, richzhang/PerceptualSimilarity).
struct FireW { ConvW squeeze, expand1, expand3; };
struct LpipsW : TowerW {
  int max_pairs = 0;                      // max_images = 2 * max_pairs
  half_t* w0 = nullptr; float* b0 = nullptr;   // features.0: [64][27] in (ky, kx, c) columns, [64]
  FireW fire[8];                          // features.3, 4, 6, 7, 9, 10, 11, 12
  float* lin[7] = {};                     // lin0 .. lin6 [C_k]
  int sized_S = 0;                        // the workspaces hold a forward of max_images images of this side (grown on demand)
};

struct Tensor4 { half_t* p; int B, H, W, C; };

struct CtrlDev {
  bool any_edit = false;
  int nimg = 0, n_alpha_rows = 0;
  int npairs = 0;                 // images with kind == 1
  int lb_any = 0;
  std::vector<int> lb_start;      // per pair
  std::vector<float> lb_th;
  std::vector<float> lb_th_sub;   // per pair; +inf when the pair has no substruct words
  int lb_planes = 2;              // 2, or 4 when any pair of the batch has substruct words
  std::vector<int> lb_enabled;
  std::vector<int> pair_img;      // pair -> image
  int self_lo = 0, self_hi = 0, self_max_tokens = 0;
  // device tables
  int* rows_id = nullptr;         // [rows][4] identity
  int* rows_rep = nullptr;        // [rows][4] self-attention replacement
  int* rows_plain = nullptr;      // rows that take the plain cross-attention path
  int* rows_masa = nullptr;       // [rows][4] MasaCtrl: target rows read K, V of the source row of their CFG half
  bool masa_any = false;
  int masa_start_step = 0, masa_start_layer = 0;
  unsigned masa_layer_mask = 0;                     // bit 31: a layer_idx list was given (bits 0..15 = its blocks); 0 = the start_layer window
  std::vector<unsigned char> masa_step_on;          // step_idx list as a per-step flag array; empty + !masa_step_list = the start_step window
  bool masa_step_list = false;
  // mask-guided MasaCtrl (pnpi_masa_set_masks): at the controlled sites the plain launch takes every row but the kind-2 target rows,
  // which run the class-restricted kernel on {tgt, tgt, src, src} with the class rows of their image
  bool masa_masked = false;
  int* rows_masa_plain = nullptr; int n_masa_plain = 0;
  int* rows_masa_tgt = nullptr; int n_masa_tgt = 0;     // [n_masa_tgt][4]
  int* masa_tgt_img = nullptr;                          // [n_masa_tgt] mask image of each target row
  int n_plain = 0;
  int* pairs = nullptr;           // [npairs][2]
  half_t* mmatT = nullptr;        // [npairs][96][96]
  float* coef = nullptr;          // [n_alpha_rows][2][npairs][96]  (c1 block, c2 block per step)
  float* lb_alpha = nullptr;      // [npairs][lb_planes][96]
  float* lb_acc = nullptr;        // [npairs][nslots][lb_planes][tokens]
};

// Text K / V cache: the cross-attention keys / values depend only on the text context, which is constant over a denoising loop
// (to_k / to_v of attention.py:230-234 applied to encoder_hidden_states): computed once per loop for the 16 transformer blocks.
struct TextKV {
  std::vector<half_t*> k, vt;     // per transformer block in execution order: [rows][T][hd], [rows][hd][ldv]
  char* base = nullptr; size_t cap = 0;
  int rows = 0;                   // rows the cache holds (0 = invalid); a forward reads it when its call says so (UNetCall::cached_kv)
};

// Mask-guided MasaCtrl: the source / target masks of pnpi_masa_set_masks resized to every self-attention level, one class byte per
// token.  The buffer is allocated once per context (fixed addresses) and rewritten by every pnpi_masa_set_masks.
struct MasaMasks {
  uint8_t* base = nullptr;        // per level l: mask_s [cap_img][side_l^2], then mask_t [cap_img][side_l^2]
  uint8_t* stage = nullptr; size_t stage_bytes = 0;    // the caller's full-size masks on the device
  int cap_img = 0, nimg = 0;      // nimg == 0: no masks set
  std::vector<int> side;          // level sides: sample_size >> i
  std::vector<size_t> off;        // byte offset of level l's mask_s block
  const uint8_t* s_at(int l) const { return base + off[l]; }
  const uint8_t* t_at(int l) const { return base + off[l] + (size_t)cap_img * side[l] * side[l]; }
};

// Plug-and-Play injection parameters of one forward, the caller's (pnpi_unet_forward_pnp, pnpi_pnp_edit): rows [img][source, negative, target].
// conv: the decoder ResNet `conv_site` (execution order) runs its main branch on the source rows only and every row adds its image's
// result to its own shortcut; qk: the transformer blocks of qk_mask take the row table `rows` ({r, src, src, r}) in their self-attention.
struct PnpState {
  bool on = false, conv = false, qk = false;
  int nimg = 0, conv_site = -1;
  unsigned qk_mask = 0;
  int* rows = nullptr;            // [3 nimg][4] device
  int* src_rows = nullptr;        // [nimg] device: launch row of image i's source (3 i)
  int* hrow = nullptr;            // [3 nimg] device: launch row -> its image (r / 3)
};

struct ProfRec { int cls; double flops, bytes; hipEvent_t a, b; int M, N, K, ksize; int cfg = -1, split = 0; int geom[7] = {0, 0, 0, 0, 0, 0, 0}; };

struct Tape; struct UNetFlight;   // api_graph.inc: activation tape of a differentiable forward (null-text path); what one UNet forward mutates while it runs

struct pnpi_ctx {
  pnpi_model_config cfg;
  int device;
  hipStream_t st;
  std::string err;
  int max_rows, max_vae;
  bool dry = false;             // sizing run: the graphs allocate and count, nothing is launched (DryScope)
  UNetFlight* fw = nullptr;     // the UNet forward in flight (set and cleared by unet_fwd; the DINO forward sets one for its GEMM pin alone); nullptr in every other graph
  Bump warena, persist, temp, ctrl_arena;
  struct AugBias { float* p; int heads, Dp, dh; };
  std::vector<AugBias> aug_biases;                  // the b_qkv_aug vectors of this build (filled after the arena exists)
  // derived weights of the arena (tuning "ff_fold"): one entry per transformer block whose ff2 + proj_out pair has a folded form
  struct FfFold { const half_t* wp; int ldp; const float* bp; const half_t* w2; const float* b2; int C; half_t* w_fo; float* b_fo; std::string src[4]; };
  std::vector<FfFold> ff_folds;
  bool warena_borrowed = false;                     // pnpi_create_shared: warena.base is the parent's (never written here)
  // ff_fold_ready: the folded weights in the arena match the ff2 / proj_out weights next to them (set by the owner after a load,
  // read by every context on the arena before a forward takes the folded path)
  struct ArenaRef { void* base; std::atomic<int> refs; bool ff_fold_ready = false; };
  ArenaRef* warena_ref = nullptr;                   // shared by the owner and every context that borrows the arena: the last pnpi_destroy frees it
  float* splitk_ws; size_t splitk_bytes;
  float* gn_partial; size_t gn_partial_floats = 0;
  float* temb_table;      // [n_train][C0] fp32 sinusoid table
  float* temb_row = nullptr;   // [C0] the caller's sinusoid row of pnpi_unet_forward_t
  float* temb_h;          // [4*C0]
  float* temb_emb;        // [4*C0]
  float* bias_scratch;    // [temb_total]
  float* bias_tab = nullptr;          // [n_train][temb_total]: conv1 bias + time embedding per TIMESTEP, filled on first use -- it depends
  std::vector<char> bias_valid;       // on t and the weights only, so every later forward at that timestep launches no GEMV
  TextKV tkv;
  // level-1 fallback for controllers without a descriptor: materialise-and-call-back (pnpi_set_attention_callback)
  pnpi_attn_callback attn_cb = nullptr;
  float* gn_bwd_ws = nullptr; size_t gn_bwd_ws_floats = 0;   // partial sums of the three-phase GroupNorm backward (grown on demand)
  void* attn_cb_user = nullptr;
  float* attn_buf = nullptr; size_t attn_buf_bytes = 0;   // caller-owned device buffer the probabilities are materialised in
  std::unordered_map<std::string, Slot> slots;
  UNetW unet;
  VaeW vae;
  ClipW clip;
  ClipVisionW* cv = nullptr;   // pnpi_clipv_attach; nullptr: no image tower
  DinoW* dino = nullptr;       // pnpi_dino_attach; nullptr: no DINO ViT
  float* ss_ws = nullptr; size_t ss_ws_floats = 0;   // norms and partial sums of the self-similarity distance (grown on demand)
  LpipsW* lpips = nullptr;     // pnpi_lpips_attach; nullptr: no LPIPS network
  float* lp_ws = nullptr; size_t lp_ws_floats = 0;   // per-workgroup partial sums of the LPIPS tap distance (grown on demand)
  int* rows_ident = nullptr;  // [max(max_rows, 8)][4] identity attention-row table (text encoder)
  int rows_ident_n = 0;
  std::vector<float> ac;
  float final_alpha;
  bool sched_set;
  pnpi_counters ctr;
  CtrlDev cd;
  MasaMasks mm;
  std::vector<char> host_stage;
  bool prof_on = false;
  std::vector<ProfRec> prof;
  Tape* tape = nullptr;          // non-null once a recording forward ran on this context (UNetCall::record)
};
