// api_structdist.inc -- part of api.hip (one translation unit: included there behind api_clipscore.inc; not compiled on its own).
// DINO structure distance (evaluation/matrics_calculator.py:385-405 -> :237-246 -> :154-171): the DINO ViT attached to a context,
// the reference's preprocessing, the keys of the last block and the fused self-similarity distance.  What it shares with the CLIP
// image tower (attach sequence, free, refusals, token assembly) is in api_vit.inc; a context that never calls pnpi_dino_attach is unchanged.
// ---------------------------------------------------------------------------------------------------- resize taps (host)
// PyTorch's compute_source_index_and_lambda for align_corners = False, opmath float (aten/src/ATen/native/UpSample.h)
static void dino_resize_taps(int in_size, int out_size, int* idx0, int* idx1, float* lam) {
  const float scale = (float)in_size / (float)out_size;
  for (int o = 0; o < out_size; ++o) {
    int i0 = o, i1 = o;
    float l1 = 0.f;
    if (in_size != out_size) {
      float src = scale * ((float)o + 0.5f) - 0.5f;
      if (src < 0.f) src = 0.f;
      i0 = (int)src;
      if (i0 > in_size - 1) i0 = in_size - 1;
      l1 = src - (float)i0;
      l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
      i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    }
    if (idx0) idx0[o] = i0;
    if (idx1) idx1[o] = i1;
    if (lam) lam[o] = l1;
  }
}

// ---------------------------------------------------------------------------------------------------- attach / free
static void dino_free(pnpi_ctx* c) {
  DinoW* v = c->dino;
  if (!v) return;
  tower_free(c, v);
  for (auto& t : v->tabs) { (void)hipFree(t.idx); (void)hipFree(t.lam); }
  delete v;
  c->dino = nullptr;
}

// the ViT's weight slots, through the context's own slot helpers (under TowerArena)
static void dino_build(pnpi_ctx* c) {
  DinoW* v = c->dino;
  const pnpi_dino_config& g = v->cfg;
  const int W = g.width;
  v->w_patch = walloc_h(c, (size_t)W * v->K);
  reg_mat(c, "dino.patch_embed.proj.weight", v->w_patch, W, v->K, 1, v->K, v->K);      // [W][3][p][p] flattened = (c, ky, kx) columns
  v->b_patch = walloc_f(c, W);
  reg_vec(c, "dino.patch_embed.proj.bias", v->b_patch, W);
  v->cls = walloc_f(c, W);
  reg_vec(c, "dino.cls_token", v->cls, W);
  v->pos = walloc_f(c, (size_t)v->T * W);
  reg_vec(c, "dino.pos_embed", v->pos, v->T * W);
  v->layers.clear();
  for (int l = 0; l < g.layers; ++l) {
    const std::string pre = "dino.blocks." + std::to_string(l);
    const bool last = l == g.layers - 1;      // the hooked block: norm1 and the K third of attn.qkv, nothing else
    ClipLayerW L;
    L.ln1 = make_norm(c, pre + ".norm1", W);
    if (last) {
      L.w_qkv = walloc_h(c, (size_t)3 * W * W);      // the whole matrix is kept (one checkpoint tensor, one slot); rows W .. 2 W - 1 are read
      L.b_qkv = walloc_f(c, 3 * W);
      reg_mat(c, pre + ".attn.qkv.weight", L.w_qkv, 3 * W, W, 1, W, W);
      reg_vec(c, pre + ".attn.qkv.bias", L.b_qkv, 3 * W);
    } else {
      L.ln2 = make_norm(c, pre + ".norm2", W);
      L.w_qkv = walloc_h(c, (size_t)3 * W * W);      // DINO's qkv Linear: output columns [3][heads][dh] = q | k | v, as the layer reads them
      L.b_qkv = walloc_f(c, 3 * W);
      reg_mat(c, pre + ".attn.qkv.weight", L.w_qkv, 3 * W, W, 1, W, W);
      reg_vec(c, pre + ".attn.qkv.bias", L.b_qkv, 3 * W);
      L.out = make_lin(c, pre + ".attn.proj", W, W);
      L.fc1 = make_lin(c, pre + ".mlp.fc1", W, g.intermediate);
      L.fc2 = make_lin(c, pre + ".mlp.fc2", g.intermediate, W);
    }
    v->layers.push_back(L);
  }
}
// the row table and the tower's own small buffer
static void dino_bufs(pnpi_ctx* c, Bump& b) {
  DinoW* v = c->dino;
  vit_bufs(v, b);
  v->keys16 = (half_t*)b.alloc((size_t)v->max_images * v->T * v->W * sizeof(half_t));
}

static int dino_preprocess(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, int out, float* resized, half_t* patches);

// VisionTransformer.forward up to the hook on blocks[-1].attn.qkv: keys16 [n][T][W] fp16 = the K third of that Linear's output.
// img2 (nullable): a second batch of n2 images behind the first (the gt images of pnpi_structure_distance) -- one tower pass over both.
static int dino_fwd(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, const uint8_t* img2, const uint8_t* mask2, int n2, int S,
                    half_t* keys16) {
  DinoW* v = c->dino;
  const pnpi_dino_config& g = v->cfg;
  const int W = g.width, T = v->T, NP = v->NP, nt = n + n2, M = nt * T;
  TowerWorkspace ws(c, v);
  // every GEMM (M = nt x tokens) takes the tile / split-K of its max_images form: an image's keys do not depend on the batch it is in
  UNetFlight pin{UNetShare()};
  pin.pin_from = nt; pin.pin_to = v->max_images;
  FlightScope fs(c, &pin);
  c->persist.reset(); c->temp.reset();
  half_t* patches = palloc(c, (size_t)nt * NP * v->K);
  if (!c->dry) {
    CKP(dino_preprocess(c, img, mask, n, S, g.image_size, nullptr, patches));
    if (n2) CKP(dino_preprocess(c, img2, mask2, n2, S, g.image_size, nullptr, patches + (size_t)n * NP * v->K));
  }
  half_t* x = palloc(c, (size_t)M * W);
  CKP(vit_tokens(c, v, patches, nt, -1.0, x));      // the convolution's bias joins in the assembly
  for (int l = 0; l + 1 < g.layers; ++l) CKP(clip_encoder_layer(c, v->layers[l], x, nt, T, W, g.heads, g.intermediate, 0, v->rows_ident, 1e-6f, 1));
  {
    const ClipLayerW& L = v->layers.back();
    const size_t mk = c->temp.mark();
    half_t* h1 = talloc(c, (size_t)M * W);
    if (!c->dry) PROF(PNPI_KC_LAYERNORM, 0.0, 2.0 * M * (double)W * 2.0, launch_layernorm(x, M, W, 1e-6f, L.ln1.g, L.ln1.b, h1, c->st));
    CK(op_gemm(c, h1, W, M, W, L.w_qkv + (size_t)W * W, W, W, L.b_qkv + W, nullptr, 0, keys16, W));
    c->temp.release(mk);
  }
  if (c->persist.overflow || c->temp.overflow) return fail(c, PNPI_ENOMEM, "workspace overflow (DINO ViT)");
  return 0;
}
static int dino_dry_fwd(pnpi_ctx* c) { return dino_fwd(c, nullptr, nullptr, c->dino->max_images, nullptr, nullptr, 0, c->dino->cfg.image_size, c->dino->keys16); }

// ---------------------------------------------------------------------------------------------------- refusals (all before a launch)
static int dino_check_attached(pnpi_ctx* c) {
  if (!c->dino) return fail(c, PNPI_ESTATE, "no DINO ViT attached to this context (pnpi_dino_attach)");
  return 0;
}
static int dino_check_images(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int nmax, int S, const char* what) {
  if (!img) { c->err = std::string(what) + " is NULL"; return PNPI_EINVAL; }
  if (n <= 0 || n > nmax) return fail(c, PNPI_EINVAL, "n out of range: 1 .. max_pairs pairs, 1 .. 2 * max_pairs images of pnpi_dino_attach");
  if (S < 16 || S > 8192) return fail(c, PNPI_ESHAPE, "unsupported image side: square S with 16 <= S <= 8192");
  if (mask) CKP(check_mask01(c, mask, (size_t)n * S * S));
  return 0;
}
// the device taps for S -> out; allocations and copies only, no launch
static int dino_resize_prepare(pnpi_ctx* c, int S, int out, const DinoW::ResizeTab** tab_out) {
  DinoW* v = c->dino;
  for (auto& t : v->tabs)
    if (t.S == S && t.out == out) { *tab_out = &t; return 0; }
  std::vector<int> idx((size_t)2 * out);
  std::vector<float> lam(out);
  dino_resize_taps(S, out, idx.data(), idx.data() + out, lam.data());
  DinoW::ResizeTab t; t.S = S; t.out = out; t.idx = nullptr; t.lam = nullptr;
  CKH(hipMalloc((void**)&t.idx, idx.size() * sizeof(int)));
  if (hipMalloc((void**)&t.lam, lam.size() * sizeof(float)) != hipSuccess) { (void)hipFree(t.idx); return fail(c, PNPI_ENOMEM, "resize taps: allocation failed"); }
  v->tabs.push_back(t);      // owned by the tower from here on (dino_free)
  CKH(hipMemcpy(t.idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
  CKH(hipMemcpy(t.lam, lam.data(), lam.size() * sizeof(float), hipMemcpyHostToDevice));
  *tab_out = &v->tabs.back();
  return 0;
}
static int dino_preprocess(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, int out, float* resized, half_t* patches) {
  const DinoW::ResizeTab* t = nullptr;
  CKP(dino_resize_prepare(c, S, out, &t));
  CK(launch_dino_preprocess(img, mask, n, S, out, t->idx, t->idx + out, t->lam, c->dino->cfg.patch, resized, patches, c->st));
  return 0;
}
// norms and per-workgroup partial sums of the distance, grown on demand (no launch)
static int selfsim_scratch(pnpi_ctx* c, int n, int T) {
  const size_t need = keys_selfsim_scratch_floats(n, T);
  if (need <= c->ss_ws_floats) return 0;
  CKH(hipStreamSynchronize(c->st));
  (void)hipFree(c->ss_ws); c->ss_ws = nullptr; c->ss_ws_floats = 0;
  CKH(hipMalloc((void**)&c->ss_ws, need * sizeof(float)));
  c->ss_ws_floats = need;
  return 0;
}

// ---------------------------------------------------------------------------------------------------- C ABI
extern "C" {

void pnpi_dino_config_vitb8(pnpi_dino_config* g) {      /* facebookresearch/dino: dino_vitb8 = vit_base(patch_size = 8) */
  memset(g, 0, sizeof(*g));
  g->struct_size = (int)sizeof(*g);
  g->image_size = 224; g->patch = 8; g->width = 768; g->layers = 12; g->heads = 12; g->intermediate = 3072;
}

int pnpi_dino_resize_taps(int in_size, int out_size, int* idx0_out, int* idx1_out, float* lambda_out) {
  if (in_size <= 0 || out_size <= 0 || in_size > 8192 || out_size > 8192) return PNPI_ESHAPE;
  dino_resize_taps(in_size, out_size, idx0_out, idx1_out, lambda_out);
  return 0;
}

int pnpi_dino_attach(pnpi_ctx* c, const pnpi_dino_config* g, int max_pairs) {
  if (!c || !g) return PNPI_EINVAL;
  if (g->struct_size != (int)sizeof(pnpi_dino_config)) return fail(c, PNPI_EINVAL, "pnpi_dino_config.struct_size is not sizeof(pnpi_dino_config) of this library");
  if (c->dino) return fail(c, PNPI_ESTATE, "pnpi_dino_attach: a DINO ViT is already attached");
  if (max_pairs <= 0 || max_pairs > 128) return fail(c, PNPI_EINVAL, "max_pairs must be 1 .. 128");
  if (g->image_size <= 0 || g->patch <= 0 || g->patch % 8 || g->image_size % g->patch || g->image_size > 1024)
    return fail(c, PNPI_ESHAPE, "patch must be a multiple of 8 and image_size a multiple of patch, at most 1024");
  if (g->width <= 0 || g->width % 32 || g->width > 2048 || g->heads <= 0 || g->width % g->heads)
    return fail(c, PNPI_ESHAPE, "width must be a multiple of 32 and of heads, at most 2048");
  const int dh = g->width / g->heads;
  if (dh % 32 || dh > 160) return fail(c, PNPI_ESHAPE, "DINO head dim must be a multiple of 32 and <= 160");
  if (g->layers <= 0 || g->layers > 48 || g->intermediate <= 0 || g->intermediate % 8)
    return fail(c, PNPI_ESHAPE, "layers must be 1 .. 48, intermediate a multiple of 8");
  DinoW* v = new DinoW();
  v->name = "DINO ViT"; v->prefix = "dino.";
  v->cfg = *g; v->max_pairs = max_pairs; v->max_images = 2 * max_pairs; v->W = g->width;
  c->dino = v;
  return vit_attach(c, v, "pnpi_dino_attach", g->image_size, g->patch, {dino_build, dino_bufs, dino_dry_fwd, dino_free});      // K = 3 patch^2: patch % 8 == 0
}

int pnpi_op_dino_preprocess(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, int out_size, float* resized_out,
                            void* patches_f16_out) {
  if (!c) return PNPI_EINVAL;
  CKP(dino_check_attached(c));
  if (!resized_out && !patches_f16_out) return fail(c, PNPI_EINVAL, "pnpi_op_dino_preprocess: no output given");
  if (out_size <= 0 || out_size % c->dino->cfg.patch || out_size > 1024) return fail(c, PNPI_ESHAPE, "out_size must be a multiple of the ViT's patch, at most 1024");
  CKP(dino_check_images(c, img, mask, n, c->dino->max_images, S, "img_hwc"));
  return dino_preprocess(c, img, mask, n, S, out_size, resized_out, (half_t*)patches_f16_out);
}

int pnpi_dino_keys(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, float* keys_out) {
  if (!c) return PNPI_EINVAL;
  CKP(dino_check_attached(c));
  CKP(tower_check_weights(c, c->dino));
  if (!keys_out) return fail(c, PNPI_EINVAL, "keys_out is NULL");
  DinoW* v = c->dino;
  CKP(dino_check_images(c, img, mask, n, v->max_images, S, "img_hwc"));
  CKP(dino_fwd(c, img, mask, n, nullptr, nullptr, 0, S, v->keys16));
  CK(launch_f16_to_f32(v->keys16, (size_t)n * v->T * v->cfg.width, keys_out, c->st));
  return 0;
}

int pnpi_structure_distance(pnpi_ctx* c, const uint8_t* img_pred, const uint8_t* mask_pred, const uint8_t* img_gt, const uint8_t* mask_gt,
                            int n, int S, float* dist_out) {
  if (!c) return PNPI_EINVAL;
  CKP(dino_check_attached(c));
  CKP(tower_check_weights(c, c->dino));
  if (!dist_out) return fail(c, PNPI_EINVAL, "dist_out is NULL");
  DinoW* v = c->dino;
  CKP(dino_check_images(c, img_pred, mask_pred, n, v->max_pairs, S, "img_pred"));
  CKP(dino_check_images(c, img_gt, mask_gt, n, v->max_pairs, S, "img_gt"));
  CKP(selfsim_scratch(c, n, v->T));
  CKP(dino_fwd(c, img_pred, mask_pred, n, img_gt, mask_gt, n, S, v->keys16));
  CK(launch_keys_selfsim_mse(v->keys16, v->keys16 + (size_t)n * v->T * v->cfg.width, n, v->T, v->cfg.width, c->ss_ws, dist_out, nullptr, c->st));
  return 0;
}

int pnpi_op_keys_selfsim_mse(pnpi_ctx* c, const void* keys_a, const void* keys_b, int n, int T, int D, float* dist_out, float* sim_a_out) {
  if (!c) return PNPI_EINVAL;
  if (!keys_a || !keys_b) return fail(c, PNPI_EINVAL, "keys_a_f16 / keys_b_f16 is NULL");
  if (!dist_out) return fail(c, PNPI_EINVAL, "dist_out is NULL");
  if (n <= 0 || n > 65535 || T <= 0 || T > (1 << 20)) return fail(c, PNPI_EINVAL, "n must be 1 .. 65535, T 1 .. 2^20");
  if (D <= 0 || D % 32) return fail(c, PNPI_ESHAPE, "D must be a positive multiple of 32");
  if (((uintptr_t)keys_a | (uintptr_t)keys_b) & 15) return fail(c, PNPI_EINVAL, "the key matrices must be 16-byte aligned");
  CKP(selfsim_scratch(c, n, T));
  CK(launch_keys_selfsim_mse((const half_t*)keys_a, (const half_t*)keys_b, n, T, D, c->ss_ws, dist_out, sim_a_out, c->st));
  return 0;
}

}  // extern "C"
