// api_clipscore.inc -- part of api.hip (one translation unit: included there behind api_vit.inc; not compiled on its own).
// CLIP similarity (evaluation/matrics_calculator.py:290-302): the image tower of transformers' CLIPModel attached to a context that has
// the text tower, the two projections, CLIPProcessor's preprocessing and the score.  What it shares with the DINO ViT (attach sequence, free, refusals,
// token assembly) is in api_vit.inc; a context that never calls pnpi_clipv_attach is unchanged.
// ---------------------------------------------------------------------------------------------------- PIL coefficient tables
// precompute_coeffs + normalize_coeffs_8bpc of Pillow's libImaging/Resample.c for the bicubic filter (a = -0.5, support 2), in double
// as there: the filter's support is stretched by the scale factor on a downscale (antialiasing), the weights of one output pixel
// are normalised to sum 1 and then rounded half away from zero to 22-bit fixed point.  in_size == out_size: PIL returns a copy.
static double pil_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
static int pil_bicubic_tables(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& coef) {
  if (in_size == out_size) {
    bounds.resize((size_t)out_size * 2); coef.assign(out_size, 1 << 22);
    for (int i = 0; i < out_size; ++i) { bounds[2 * i] = i; bounds[2 * i + 1] = 1; }
    return 1;
  }
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  bounds.assign((size_t)out_size * 2, 0); coef.assign((size_t)out_size * ksize, 0);
  std::vector<double> k(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale, ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) { k[x] = pil_bicubic((x + xmin - center + 0.5) * ss); ww += k[x]; }
    for (int x = 0; x < xmax; ++x) {
      const double v = ww != 0.0 ? k[x] / ww : k[x];
      coef[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
    }
    bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

// ---------------------------------------------------------------------------------------------------- attach / free
static void clipv_free(pnpi_ctx* c) {
  ClipVisionW* v = c->cv;
  if (!v) return;
  tower_free(c, v);
  for (auto& t : v->tabs) { (void)hipFree(t.bounds); (void)hipFree(t.coef); }
  (void)hipFree(v->tmp_u8);
  delete v;
  c->cv = nullptr;
}

// the tower's weight slots, through the context's own slot helpers (under TowerArena)
static void clipv_build(pnpi_ctx* c) {
  ClipVisionW* v = c->cv;
  const pnpi_clipv_config& g = v->cfg;
  const int W = g.width, P = g.proj_dim, Ht = c->clip.H, K = 3 * g.patch * g.patch;
  const std::string vm = "clipv.vision_model.";
  v->w_patch = walloc_h(c, (size_t)W * v->K);
  reg_mat(c, vm + "embeddings.patch_embedding.weight", v->w_patch, W, K, 1, v->K, K);      // [W][3][p][p] flattened = (c, ky, kx) columns
  v->cls = walloc_f(c, W);
  reg_vec(c, vm + "embeddings.class_embedding", v->cls, W);
  v->pos = walloc_f(c, (size_t)v->T * W);
  reg_vec(c, vm + "embeddings.position_embedding.weight", v->pos, v->T * W);
  v->pre_ln = make_norm(c, vm + "pre_layrnorm", W);
  v->layers.clear();
  for (int l = 0; l < g.layers; ++l) {
    const std::string pre = vm + "encoder.layers." + std::to_string(l);
    ClipLayerW L;
    L.ln1 = make_norm(c, pre + ".layer_norm1", W);
    L.ln2 = make_norm(c, pre + ".layer_norm2", W);
    L.w_qkv = walloc_h(c, (size_t)3 * W * W);
    L.b_qkv = walloc_f(c, 3 * W);
    reg_mat(c, pre + ".self_attn.q_proj.weight", L.w_qkv, W, W, 1, W, W, 0);
    reg_mat(c, pre + ".self_attn.k_proj.weight", L.w_qkv, W, W, 1, W, W, W);
    reg_mat(c, pre + ".self_attn.v_proj.weight", L.w_qkv, W, W, 1, W, W, 2 * W);
    reg_vec(c, pre + ".self_attn.q_proj.bias", L.b_qkv, W);
    reg_vec(c, pre + ".self_attn.k_proj.bias", L.b_qkv + W, W);
    reg_vec(c, pre + ".self_attn.v_proj.bias", L.b_qkv + 2 * W, W);
    L.out = make_lin(c, pre + ".self_attn.out_proj", W, W);
    L.fc1 = make_lin(c, pre + ".mlp.fc1", W, g.intermediate);
    L.fc2 = make_lin(c, pre + ".mlp.fc2", g.intermediate, W);
    v->layers.push_back(L);
  }
  v->post_ln = make_norm(c, vm + "post_layernorm", W);
  v->w_vproj = walloc_h(c, (size_t)P * W);
  reg_mat(c, "clipv.visual_projection.weight", v->w_vproj, P, W, 1, W, W);
  v->w_tproj = walloc_h(c, (size_t)P * Ht);
  reg_mat(c, "clipv.text_projection.weight", v->w_tproj, P, Ht, 1, Ht, Ht);
}
// the row table and the tower's own small buffers
static void clipv_bufs(pnpi_ctx* c, Bump& b) {
  ClipVisionW* v = c->cv;
  vit_bufs(v, b);
  const size_t N = v->max_images, W = v->W, P = v->cfg.proj_dim, Ht = c->clip.H;
  v->pool_img = (half_t*)b.alloc(N * W * sizeof(half_t));
  v->ln_img = (half_t*)b.alloc(N * W * sizeof(half_t));
  v->emb_img16 = (half_t*)b.alloc(N * P * sizeof(half_t));
  v->pool_txt = (half_t*)b.alloc(N * Ht * sizeof(half_t));
  v->emb_txt16 = (half_t*)b.alloc(N * P * sizeof(half_t));
  v->emb_img = (float*)b.alloc(N * P * sizeof(float));
  v->emb_txt = (float*)b.alloc(N * P * sizeof(float));
}

static int clipv_preprocess(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, int out, uint8_t* resized, half_t* patches);

// CLIPVisionTransformer.forward -> pooled_output -> visual_projection, n images: emb16 [n][proj] fp16
static int clipv_fwd(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, half_t* emb16) {
  ClipVisionW* v = c->cv;
  const pnpi_clipv_config& g = v->cfg;
  const int W = g.width, T = v->T, NP = v->NP, M = n * T;
  TowerWorkspace ws(c, v);
  c->persist.reset(); c->temp.reset();
  half_t* patches = palloc(c, (size_t)n * NP * v->K);
  if (!c->dry) CKP(clipv_preprocess(c, img, mask, n, S, g.image_size, nullptr, patches));
  half_t* x = palloc(c, (size_t)M * W);
  {
    const size_t mk = c->temp.mark();
    half_t* xa = talloc(c, (size_t)M * W);
    CKP(vit_tokens(c, v, patches, n, 2.0 * n * NP * (double)W * 3 * g.patch * g.patch, xa));      // the pad columns do no work
    if (!c->dry) PROF(PNPI_KC_LAYERNORM, 0.0, 2.0 * M * (double)W * 2.0, launch_layernorm(xa, M, W, 1e-5f, v->pre_ln.g, v->pre_ln.b, x, c->st));
    c->temp.release(mk);
  }
  for (const ClipLayerW& L : v->layers) CKP(clip_encoder_layer(c, L, x, n, T, W, g.heads, g.intermediate, 0, v->rows_ident));
  if (!c->dry) {
    CK(launch_clip_gather_rows(x, n, T, W, nullptr, v->pool_img, c->st));
    PROF(PNPI_KC_LAYERNORM, 0.0, 2.0 * n * (double)W * 2.0, launch_layernorm(v->pool_img, n, W, 1e-5f, v->post_ln.g, v->post_ln.b, v->ln_img, c->st));
  }
  CK(op_gemm(c, v->ln_img, W, n, W, v->w_vproj, W, g.proj_dim, nullptr, nullptr, 0, emb16, g.proj_dim));
  if (c->persist.overflow || c->temp.overflow) return fail(c, PNPI_ENOMEM, "workspace overflow (CLIP image tower)");
  return 0;
}

static int clipv_dry_fwd(pnpi_ctx* c) { return clipv_fwd(c, nullptr, nullptr, c->cv->max_images, c->cv->cfg.image_size, c->cv->emb_img16); }

// get_text_features: the text tower in chunks of what its row table holds, the EOS rows, text_projection: emb16 [n][proj] fp16
static int clipv_text_fwd(pnpi_ctx* c, const int32_t* ids, int n, half_t* emb16) {
  ClipVisionW* v = c->cv;
  const int H = c->clip.H, T = c->clip.T;
  for (int i0 = 0; i0 < n; i0 += c->rows_ident_n) {
    const int m = n - i0 < c->rows_ident_n ? n - i0 : c->rows_ident_n;
    half_t* y = nullptr;
    CKP(clip_fwd(c, (const int*)ids + (size_t)i0 * T, m, nullptr, &y));
    CK(launch_clip_gather_rows(y, m, T, H, (const int*)ids + (size_t)i0 * T, v->pool_txt + (size_t)i0 * H, c->st));
    if (c->persist.overflow || c->temp.overflow) return fail(c, PNPI_ENOMEM, "workspace overflow (CLIP text tower)");
  }
  CK(op_gemm(c, v->pool_txt, H, n, H, v->w_tproj, H, v->cfg.proj_dim, nullptr, nullptr, 0, emb16, v->cfg.proj_dim));
  return 0;
}

// ---------------------------------------------------------------------------------------------------- refusals (all before a launch)
static int clipv_check_attached(pnpi_ctx* c) {
  if (!c->cv) return fail(c, PNPI_ESTATE, "no CLIP image tower attached to this context (pnpi_clipv_attach)");
  return 0;
}
static int clipv_check_weights(pnpi_ctx* c, bool text_too) {
  CKP(tower_check_weights(c, c->cv));
  if (text_too) CKP(check_clip_ready(c));
  return 0;
}
static int clipv_check_images(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, int out) {
  ClipVisionW* v = c->cv;
  if (!img) return fail(c, PNPI_EINVAL, "img_hwc is NULL");
  if (n <= 0 || n > v->max_images) return fail(c, PNPI_EINVAL, "n must be 1 .. max_images of pnpi_clipv_attach");
  if (S < out || S > 8192) return fail(c, PNPI_ESHAPE, "unsupported image side: square S with image_size <= S <= 8192");
  if (mask) CKP(check_mask01(c, mask, (size_t)n * S * S));
  return 0;
}
// the device tables for S -> out and the horizontal pass's buffer; allocations and copies only, no launch
static int clipv_resize_prepare(pnpi_ctx* c, int n, int S, int out, const ClipVisionW::ResizeTab** tab_out) {
  ClipVisionW* v = c->cv;
  const ClipVisionW::ResizeTab* tab = nullptr;
  for (auto& t : v->tabs) if (t.S == S && t.out == out) tab = &t;
  if (!tab) {
    std::vector<int> bounds, coef;
    ClipVisionW::ResizeTab t; t.S = S; t.out = out; t.bounds = nullptr; t.coef = nullptr;
    t.ksize = pil_bicubic_tables(S, out, bounds, coef);
    CKH(hipMalloc((void**)&t.bounds, bounds.size() * sizeof(int)));
    if (hipMalloc((void**)&t.coef, coef.size() * sizeof(int)) != hipSuccess) { (void)hipFree(t.bounds); return fail(c, PNPI_ENOMEM, "resize tables: allocation failed"); }
    v->tabs.push_back(t);      // owned by the tower from here on (clipv_free)
    CKH(hipMemcpy(t.bounds, bounds.data(), bounds.size() * sizeof(int), hipMemcpyHostToDevice));
    CKH(hipMemcpy(t.coef, coef.data(), coef.size() * sizeof(int), hipMemcpyHostToDevice));
    tab = &v->tabs.back();
  }
  const size_t need = (size_t)n * S * out * 3;
  if (need > v->tmp_bytes) {
    CKH(hipStreamSynchronize(c->st));
    (void)hipFree(v->tmp_u8); v->tmp_u8 = nullptr; v->tmp_bytes = 0;
    CKH(hipMalloc((void**)&v->tmp_u8, need));
    v->tmp_bytes = need;
  }
  *tab_out = tab;
  return 0;
}
static int clipv_preprocess(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, int out, uint8_t* resized, half_t* patches) {
  ClipVisionW* v = c->cv;
  const ClipVisionW::ResizeTab* t = nullptr;
  CKP(clipv_resize_prepare(c, n, S, out, &t));
  CK(launch_clip_resize_h(img, mask, n, S, out, t->bounds, t->coef, t->ksize, v->tmp_u8, c->st));
  CK(launch_clip_resize_v(v->tmp_u8, n, S, out, t->bounds, t->coef, t->ksize, v->cfg.patch, v->K, resized, patches, c->st));
  return 0;
}

// ---------------------------------------------------------------------------------------------------- C ABI
extern "C" {

void pnpi_clipv_config_vitl14(pnpi_clipv_config* g) {      /* openai/clip-vit-large-patch14: config.json, vision_config + projection_dim */
  memset(g, 0, sizeof(*g));
  g->struct_size = (int)sizeof(*g);
  g->image_size = 224; g->patch = 14; g->width = 1024; g->layers = 24; g->heads = 16; g->intermediate = 4096; g->proj_dim = 768;
}

int pnpi_clip_resize_tables(int in_size, int out_size, int* bounds_out, int* coef_out) {
  if (in_size <= 0 || out_size <= 0 || out_size > in_size || in_size > 8192) return PNPI_ESHAPE;
  std::vector<int> bounds, coef;
  const int ksize = pil_bicubic_tables(in_size, out_size, bounds, coef);
  if (bounds_out) memcpy(bounds_out, bounds.data(), bounds.size() * sizeof(int));
  if (coef_out) memcpy(coef_out, coef.data(), coef.size() * sizeof(int));
  return ksize;
}

int pnpi_clipv_attach(pnpi_ctx* c, const pnpi_clipv_config* g, int max_images) {
  if (!c || !g) return PNPI_EINVAL;
  if (g->struct_size != (int)sizeof(pnpi_clipv_config)) return fail(c, PNPI_EINVAL, "pnpi_clipv_config.struct_size is not sizeof(pnpi_clipv_config) of this library");
  if (c->clip.layers.empty()) return fail(c, PNPI_ESTATE, "pnpi_clipv_attach: this context has no text tower (clip_layers = 0)");
  if (c->cv) return fail(c, PNPI_ESTATE, "pnpi_clipv_attach: an image tower is already attached");
  if (max_images <= 0 || max_images > 256) return fail(c, PNPI_EINVAL, "max_images must be 1 .. 256");
  if (g->image_size <= 0 || g->patch <= 0 || g->image_size % g->patch || g->image_size > 1024)
    return fail(c, PNPI_ESHAPE, "image_size must be a multiple of patch, at most 1024");
  if (g->width <= 0 || g->width % 8 || g->width > 2048 || g->heads <= 0 || g->width % g->heads)
    return fail(c, PNPI_ESHAPE, "width must be a multiple of 8 and of heads, at most 2048");
  const int dh = g->width / g->heads;
  if (dh % 32 || dh > 160) return fail(c, PNPI_ESHAPE, "image tower head dim must be a multiple of 32 and <= 160");
  if (g->layers <= 0 || g->layers > 48 || g->intermediate <= 0 || g->intermediate % 8 || g->proj_dim <= 0 || g->proj_dim % 8)
    return fail(c, PNPI_ESHAPE, "layers must be 1 .. 48, intermediate and proj_dim multiples of 8");
  ClipVisionW* v = new ClipVisionW();
  v->name = "CLIP image tower"; v->prefix = "clipv.";
  v->cfg = *g; v->max_images = max_images; v->W = g->width;
  c->cv = v;
  return vit_attach(c, v, "pnpi_clipv_attach", g->image_size, g->patch, {clipv_build, clipv_bufs, clipv_dry_fwd, clipv_free});
}

int pnpi_op_clip_preprocess(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, int out_size, uint8_t* resized_out,
                            void* patches_f16_out) {
  if (!c) return PNPI_EINVAL;
  CKP(clipv_check_attached(c));
  if (!resized_out && !patches_f16_out) return fail(c, PNPI_EINVAL, "pnpi_op_clip_preprocess: no output given");
  if (out_size <= 0 || out_size % c->cv->cfg.patch || out_size > 1024) return fail(c, PNPI_ESHAPE, "out_size must be a multiple of the tower's patch, at most 1024");
  CKP(clipv_check_images(c, img, mask, n, S, out_size));
  return clipv_preprocess(c, img, mask, n, S, out_size, resized_out, (half_t*)patches_f16_out);
}

int pnpi_clip_image_embed(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, float* embed_out) {
  if (!c) return PNPI_EINVAL;
  CKP(clipv_check_attached(c));
  CKP(clipv_check_weights(c, false));
  if (!embed_out) return fail(c, PNPI_EINVAL, "embed_out is NULL");
  CKP(clipv_check_images(c, img, mask, n, S, c->cv->cfg.image_size));
  CKP(clipv_fwd(c, img, mask, n, S, c->cv->emb_img16));
  CK(launch_f16_to_f32(c->cv->emb_img16, (size_t)n * c->cv->cfg.proj_dim, embed_out, c->st));
  return 0;
}

int pnpi_clip_text_embed(pnpi_ctx* c, const int32_t* input_ids, int n, float* embed_out) {
  if (!c) return PNPI_EINVAL;
  CKP(clipv_check_attached(c));
  CKP(clipv_check_weights(c, true));
  if (!input_ids || !embed_out) return fail(c, PNPI_EINVAL, "input_ids / embed_out is NULL");
  if (n <= 0 || n > c->cv->max_images) return fail(c, PNPI_EINVAL, "n must be 1 .. max_images of pnpi_clipv_attach");
  CKP(clipv_text_fwd(c, input_ids, n, c->cv->emb_txt16));
  CK(launch_f16_to_f32(c->cv->emb_txt16, (size_t)n * c->cv->cfg.proj_dim, embed_out, c->st));
  return 0;
}

int pnpi_clip_score(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, const int32_t* input_ids, int n, int S, float* score_out) {
  if (!c) return PNPI_EINVAL;
  CKP(clipv_check_attached(c));
  CKP(clipv_check_weights(c, true));
  if (!input_ids || !score_out) return fail(c, PNPI_EINVAL, "input_ids / score_out is NULL");
  ClipVisionW* v = c->cv;
  CKP(clipv_check_images(c, img, mask, n, S, v->cfg.image_size));
  const size_t ne = (size_t)n * v->cfg.proj_dim;
  CKP(clipv_fwd(c, img, mask, n, S, v->emb_img16));
  CKP(clipv_text_fwd(c, input_ids, n, v->emb_txt16));
  CK(launch_f16_to_f32(v->emb_img16, ne, v->emb_img, c->st));
  CK(launch_f16_to_f32(v->emb_txt16, ne, v->emb_txt, c->st));
  CK(launch_clip_cosine(v->emb_img, v->emb_txt, n, v->cfg.proj_dim, score_out, c->st));
  return 0;
}

}  // extern "C"
