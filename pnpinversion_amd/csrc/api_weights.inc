// api_weights.inc -- part of api.hip (one translation unit: included there, in this order; not compiled on its own).
// weight slots of the packed arena and the model builder (diffusers / transformers state-dict names -> repacked tensors)
// ---------------------------------------------------------------------------------------------------- weight slots
static void reg_mat(pnpi_ctx* c, const std::string& name, half_t* dst, int rows, int cols, int taps, int dst_ld, int cin_pad,
                    int row0 = 0, int dh = 0, int Dp = 0) {
  Slot s; s.kind = 0; s.dst = dst; s.rows = rows; s.cols = cols; s.taps = taps; s.dst_ld = dst_ld; s.cin_pad = cin_pad;
  s.row0 = row0; s.dh = dh; s.Dp = Dp; s.n = 0; s.ilv_half = 0; s.loaded = false;
  c->slots[name] = s;
}
static void reg_vec(pnpi_ctx* c, const std::string& name, float* dst, int n) {
  Slot s; s.kind = 1; s.dst = dst; s.rows = 0; s.cols = 0; s.taps = 0; s.dst_ld = 0; s.cin_pad = 0; s.row0 = 0; s.dh = 0; s.Dp = 0;
  s.n = n; s.ilv_half = 0; s.loaded = false;
  c->slots[name] = s;
}
static half_t* walloc_h(pnpi_ctx* c, size_t n) { return (half_t*)c->warena.alloc(n * sizeof(half_t)); }
static float* walloc_f(pnpi_ctx* c, size_t n) { return (float*)c->warena.alloc(n * sizeof(float)); }

static ConvW make_conv(pnpi_ctx* c, const std::string& pre, int cin, int cout, int k, int cout_alloc = 0, float* bias_dst = nullptr) {
  ConvW w; w.cin = cin; w.cin_pad = round_up_i(cin, 8); w.cout = cout; w.k = k;
  int ra = cout_alloc > cout ? cout_alloc : cout;
  w.w = walloc_h(c, (size_t)ra * k * k * w.cin_pad);
  w.b = bias_dst ? bias_dst : walloc_f(c, ra);
  reg_mat(c, pre + ".weight", w.w, cout, cin, k * k, k * k * w.cin_pad, w.cin_pad);
  reg_vec(c, pre + ".bias", w.b, cout);
  return w;
}
static LinW make_lin(pnpi_ctx* c, const std::string& pre, int in, int out) {
  LinW l; l.in = in; l.out = out;
  l.w = walloc_h(c, (size_t)out * in);
  l.b = walloc_f(c, out);
  reg_mat(c, pre + ".weight", l.w, out, in, 1, in, in);
  reg_vec(c, pre + ".bias", l.b, out);
  return l;
}
static NormW make_norm(pnpi_ctx* c, const std::string& pre, int ch) {
  NormW n; n.c = ch; n.g = walloc_f(c, ch); n.b = walloc_f(c, ch);
  reg_vec(c, pre + ".weight", n.g, ch);
  reg_vec(c, pre + ".bias", n.b, ch);
  return n;
}
static ResnetW make_resnet(pnpi_ctx* c, const std::string& pre, int cin, int cout, bool temb) {
  ResnetW r; r.cin = cin; r.cout = cout;
  r.n1 = make_norm(c, pre + ".norm1", cin);
  if (temb) {
    UNetW& u = c->unet;
    r.temb_off = u.temb_total;
    r.c1 = make_conv(c, pre + ".conv1", cin, cout, 3, 0, u.conv1_b + r.temb_off);
    int te = 4 * c->cfg.block_out_channels[0];
    reg_mat(c, pre + ".time_emb_proj.weight", u.temb_w, cout, te, 1, te, te, r.temb_off);
    reg_vec(c, pre + ".time_emb_proj.bias", u.temb_b + r.temb_off, cout);
    u.temb_total += cout;
  } else {
    r.temb_off = -1;
    r.c1 = make_conv(c, pre + ".conv1", cin, cout, 3);
  }
  r.n2 = make_norm(c, pre + ".norm2", cout);
  r.c2 = make_conv(c, pre + ".conv2", cout, cout, 3);
  r.has_sc = cin != cout;
  if (r.has_sc) r.sc = make_conv(c, pre + ".conv_shortcut", cin, cout, 1);
  return r;
}
static TransformerW make_transformer(pnpi_ctx* c, const std::string& pre, int C, int place) {
  TransformerW t; t.C = C; t.heads = c->cfg.heads; t.dh = C / t.heads; t.Dp = round_up_i(t.dh, 32); t.place = place; t.lb_slot0 = -1;
  const int hd = t.heads * t.Dp, X = c->cfg.cross_dim;
  t.gn = make_norm(c, pre + ".norm", C);
  t.proj_in = make_conv(c, pre + ".proj_in", C, C, 1);
  const std::string tb = pre + ".transformer_blocks.0";
  t.ln1 = make_norm(c, tb + ".norm1", C);
  t.ln2 = make_norm(c, tb + ".norm2", C);
  t.ln3 = make_norm(c, tb + ".norm3", C);
  t.w_qkv = walloc_h(c, (size_t)3 * hd * C);
  reg_mat(c, tb + ".attn1.to_q.weight", t.w_qkv, C, C, 1, C, C, 0, t.dh, t.Dp);
  reg_mat(c, tb + ".attn1.to_k.weight", t.w_qkv, C, C, 1, C, C, hd, t.dh, t.Dp);
  reg_mat(c, tb + ".attn1.to_v.weight", t.w_qkv, C, C, 1, C, C, 2 * hd, t.dh, t.Dp);
  t.b_qkv_aug = nullptr;
  if (t.Dp == 64 && t.dh == 40) {      // SD-1.x's 64 x 64 level: one padding column of K and V carries a constant 1 (see TransformerW)
    t.b_qkv_aug = walloc_f(c, (size_t)3 * hd);
    c->aug_biases.push_back({t.b_qkv_aug, t.heads, t.Dp, t.dh});
  }
  t.o1 = make_lin(c, tb + ".attn1.to_out.0", C, C);
  t.w_q2 = walloc_h(c, (size_t)hd * C);
  reg_mat(c, tb + ".attn2.to_q.weight", t.w_q2, C, C, 1, C, C, 0, t.dh, t.Dp);
  t.w_kv2 = walloc_h(c, (size_t)2 * hd * X);
  reg_mat(c, tb + ".attn2.to_k.weight", t.w_kv2, C, X, 1, X, X, 0, t.dh, t.Dp);
  reg_mat(c, tb + ".attn2.to_v.weight", t.w_kv2, C, X, 1, X, X, hd, t.dh, t.Dp);
  t.o2 = make_lin(c, tb + ".attn2.to_out.0", C, C);
  t.ff1 = make_lin(c, tb + ".ff.net.0.proj", C, 8 * C);
  // GEGLU fused into this GEMM's epilogue: x rows and gate rows are interleaved in groups of 32 (attention.py:331-333)
  c->slots[tb + ".ff.net.0.proj.weight"].ilv_half = 4 * C;
  c->slots[tb + ".ff.net.0.proj.bias"].ilv_half = 4 * C;
  t.ff2 = make_lin(c, tb + ".ff.net.2", 4 * C, C);
  t.proj_out = make_conv(c, pre + ".proj_out", C, C, 1);
  // ff2 folded into proj_out (transformer_fwd): derived from the four tensors above by build_ff_fold, inside the arena so that every
  // context sharing it sees the same pointers.  Narrow widths keep the two launches and spend no memory on it.
  t.fo = ConvW{nullptr, nullptr, 5 * C, 5 * C, C, 1};
  if (C % 64 == 0) {
    t.fo.w = walloc_h(c, (size_t)C * 5 * C);
    t.fo.b = walloc_f(c, C);
    c->ff_folds.push_back({t.proj_out.w, t.proj_out.cin_pad, t.proj_out.b, t.ff2.w, t.ff2.b, C, t.fo.w, t.fo.b,
                           {pre + ".proj_out.weight", pre + ".proj_out.bias", tb + ".ff.net.2.weight", tb + ".ff.net.2.bias"}});
  }
  return t;
}
static VaeAttnW make_vae_attn(pnpi_ctx* c, const std::string& pre, int C) {
  VaeAttnW a; a.C = C;
  a.gn = make_norm(c, pre + ".group_norm", C);
  a.w_qkv = walloc_h(c, (size_t)3 * C * C);
  a.b_qkv = walloc_f(c, 3 * C);
  reg_mat(c, pre + ".query.weight", a.w_qkv, C, C, 1, C, C, 0);
  reg_mat(c, pre + ".key.weight", a.w_qkv, C, C, 1, C, C, C);
  reg_mat(c, pre + ".value.weight", a.w_qkv, C, C, 1, C, C, 2 * C);
  reg_vec(c, pre + ".query.bias", a.b_qkv, C);
  reg_vec(c, pre + ".key.bias", a.b_qkv + C, C);
  reg_vec(c, pre + ".value.bias", a.b_qkv + 2 * C, C);
  a.proj = make_lin(c, pre + ".proj_attn", C, C);
  return a;
}

// The folded ff2 + proj_out weights of every transformer block, from the packed weights next to them -- derived state of the arena,
// like the caches invalidate_derived() drops: the owner of the arena rebuilds them after every load that touched a source
// (pnpi_load_weights) and after the arena was overwritten wholesale (pnpi_mark_all_loaded).  Until all four sources of every block
// are loaded the arena is marked not ready and every forward on it takes the two-launch path.
static bool ff_fold_source(const pnpi_ctx* c, const std::string& name) {
  for (const pnpi_ctx::FfFold& f : c->ff_folds)
    for (const std::string& s : f.src) if (s == name) return true;
  return false;
}
static int build_ff_fold(pnpi_ctx* c) {
  if (c->warena_borrowed || !c->warena_ref) return 0;
  c->warena_ref->ff_fold_ready = false;
  if (c->ff_folds.empty()) return 0;
  for (const pnpi_ctx::FfFold& f : c->ff_folds)
    for (const std::string& s : f.src) {
      auto it = c->slots.find(s);
      if (it == c->slots.end() || !it->second.loaded) return 0;
    }
  for (const pnpi_ctx::FfFold& f : c->ff_folds)
    if (int r = launch_ff_fold_weights(f.wp, f.ldp, f.bp, f.w2, f.b2, f.C, f.w_fo, f.b_fo, c->st)) return r;
  c->warena_ref->ff_fold_ready = true;
  return 0;
}

static int temb_total_channels(const pnpi_model_config& g) {
  int n = g.n_blocks, total = 0;
  for (int i = 0; i < n; ++i) total += g.layers_per_block * g.block_out_channels[i];
  total += 2 * g.block_out_channels[n - 1];
  for (int i = 0; i < n; ++i) total += (g.layers_per_block + 1) * g.block_out_channels[n - 1 - i];
  return total;
}

static void build_model(pnpi_ctx* c) {
  const pnpi_model_config& g = c->cfg;
  c->slots.clear();
  c->aug_biases.clear();
  c->ff_folds.clear();
  UNetW& u = c->unet;
  u = UNetW();
  const int n = g.n_blocks, C0 = g.block_out_channels[0], TE = 4 * C0;
  const int sumC = temb_total_channels(g);
  u.temb_w = walloc_h(c, (size_t)sumC * TE);
  u.temb_b = walloc_f(c, sumC);
  u.conv1_b = walloc_f(c, sumC);
  u.temb_total = 0;
  u.conv_in = make_conv(c, "unet.conv_in", g.in_channels, C0, 3);
  u.t1 = make_lin(c, "unet.time_embedding.linear_1", C0, TE);
  u.t2 = make_lin(c, "unet.time_embedding.linear_2", TE, TE);
  std::vector<TransformerW*> down_stored, up_stored;
  int out_ch = C0;
  u.down_res.resize(n); u.down_attn.resize(n);
  for (int i = 0; i < n; ++i) {
    int in_ch = out_ch; out_ch = g.block_out_channels[i];
    for (int j = 0; j < g.layers_per_block; ++j) {
      std::string pre = "unet.down_blocks." + std::to_string(i);
      u.down_res[i].push_back(make_resnet(c, pre + ".resnets." + std::to_string(j), j == 0 ? in_ch : out_ch, out_ch, true));
      if (g.block_has_attn[i]) u.down_attn[i].push_back(make_transformer(c, pre + ".attentions." + std::to_string(j), out_ch, 0));
    }
    if (i != n - 1) u.down_samp.push_back(make_conv(c, "unet.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", out_ch, out_ch, 3));
  }
  const int Cl = g.block_out_channels[n - 1];
  u.mid_res[0] = make_resnet(c, "unet.mid_block.resnets.0", Cl, Cl, true);
  u.mid_attn = make_transformer(c, "unet.mid_block.attentions.0", Cl, 1);
  u.mid_res[1] = make_resnet(c, "unet.mid_block.resnets.1", Cl, Cl, true);
  u.up_res.resize(n); u.up_attn.resize(n);
  out_ch = Cl;
  for (int i = 0; i < n; ++i) {
    int prev_out = out_ch; out_ch = g.block_out_channels[n - 1 - i];
    int in_ch = g.block_out_channels[n - 1 - (i + 1 < n ? i + 1 : n - 1)];
    for (int j = 0; j <= g.layers_per_block; ++j) {
      int skip_ch = (j == g.layers_per_block) ? in_ch : out_ch;
      int res_in = (j == 0) ? prev_out : out_ch;
      std::string pre = "unet.up_blocks." + std::to_string(i);
      u.up_res[i].push_back(make_resnet(c, pre + ".resnets." + std::to_string(j), res_in + skip_ch, out_ch, true));
      if (g.block_has_attn[n - 1 - i]) u.up_attn[i].push_back(make_transformer(c, pre + ".attentions." + std::to_string(j), out_ch, 2));
    }
    if (i != n - 1) u.up_samp.push_back(make_conv(c, "unet.up_blocks." + std::to_string(i) + ".upsamplers.0.conv", out_ch, out_ch, 3));
  }
  u.norm_out = make_norm(c, "unet.conv_norm_out", C0);
  u.conv_out = make_conv(c, "unet.conv_out", C0, g.out_channels, 3);

  // LocalBlend layers: attention_store["down_cross"][2:4] + ["up_cross"][:3] over the stored (<= 32^2 token) cross maps
  // (models/p2p/attention_control.py:112,223)
  std::vector<std::pair<TransformerW*, int>> dstored, ustored;
  for (int i = 0; i < n; ++i) {
    int tok = (g.sample_size >> i) * (g.sample_size >> i);
    for (auto& t : u.down_attn[i]) if (tok <= 1024) dstored.push_back({&t, tok});
  }
  for (int i = 0; i < n; ++i) {
    int s = g.sample_size >> (n - 1 - i);
    for (auto& t : u.up_attn[i]) if (s * s <= 1024) ustored.push_back({&t, s * s});
  }
  u.lb_nslots = 0; u.lb_tokens = 0;
  if (dstored.size() >= 4 && ustored.size() >= 3) {
    std::vector<std::pair<TransformerW*, int>> lb = {dstored[2], dstored[3], ustored[0], ustored[1], ustored[2]};
    bool same = true;
    for (auto& e : lb) same = same && e.second == lb[0].second;
    int side = (int)lroundf(sqrtf((float)lb[0].second));
    if (same && side * side == lb[0].second) {
      for (size_t k = 0; k < lb.size(); ++k) lb[k].first->lb_slot0 = (int)k * g.heads;
      u.lb_nslots = 5 * g.heads;
      u.lb_tokens = lb[0].second;
    }
  }

  // ---- VAE
  VaeW& v = c->vae;
  v = VaeW();
  const int vn = g.vae_n_blocks, L = g.vae_latent_channels;
  const int* vb = g.vae_block_out_channels;
  v.e_conv_in = make_conv(c, "vae.encoder.conv_in", g.vae_in_channels, vb[0], 3);
  v.e_res.resize(vn);
  int o = vb[0];
  for (int i = 0; i < vn; ++i) {
    int in_ch = o; o = vb[i];
    for (int j = 0; j < g.vae_layers_per_block; ++j)
      v.e_res[i].push_back(make_resnet(c, "vae.encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? in_ch : o, o, false));
    if (i != vn - 1) v.e_down.push_back(make_conv(c, "vae.encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", o, o, 3));
  }
  const int Vl = vb[vn - 1];
  v.e_mid[0] = make_resnet(c, "vae.encoder.mid_block.resnets.0", Vl, Vl, false);
  v.e_attn = make_vae_attn(c, "vae.encoder.mid_block.attentions.0", Vl);
  v.e_mid[1] = make_resnet(c, "vae.encoder.mid_block.resnets.1", Vl, Vl, false);
  v.e_norm_out = make_norm(c, "vae.encoder.conv_norm_out", Vl);
  v.e_conv_out = make_conv(c, "vae.encoder.conv_out", Vl, 2 * L, 3, 8);
  v.quant = make_conv(c, "vae.quant_conv", 2 * L, 2 * L, 1, 8);
  v.post_quant = make_conv(c, "vae.post_quant_conv", L, L, 1, 8);
  v.d_conv_in = make_conv(c, "vae.decoder.conv_in", L, Vl, 3);
  v.d_mid[0] = make_resnet(c, "vae.decoder.mid_block.resnets.0", Vl, Vl, false);
  v.d_attn = make_vae_attn(c, "vae.decoder.mid_block.attentions.0", Vl);
  v.d_mid[1] = make_resnet(c, "vae.decoder.mid_block.resnets.1", Vl, Vl, false);
  v.d_res.resize(vn);
  o = Vl;
  for (int i = 0; i < vn; ++i) {
    int prev = o; o = vb[vn - 1 - i];
    for (int j = 0; j <= g.vae_layers_per_block; ++j)
      v.d_res[i].push_back(make_resnet(c, "vae.decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? prev : o, o, false));
    if (i != vn - 1) v.d_up.push_back(make_conv(c, "vae.decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv", o, o, 3));
  }
  v.d_norm_out = make_norm(c, "vae.decoder.conv_norm_out", vb[0]);
  v.d_conv_out = make_conv(c, "vae.decoder.conv_out", vb[0], g.vae_in_channels, 3);

  // ---- CLIP text encoder (transformers CLIPTextModel; keys without the optional "text_model." prefix)
  ClipW& t = c->clip;
  t = ClipW();
  if (g.clip_layers > 0) {
    t.H = g.cross_dim; t.heads = g.clip_heads; t.I = g.clip_intermediate; t.vocab = g.clip_vocab; t.T = g.ctx_len;
    const int H = t.H;
    t.tok = walloc_h(c, (size_t)t.vocab * H);
    t.pos = walloc_h(c, (size_t)t.T * H);
    reg_mat(c, "clip.embeddings.token_embedding.weight", t.tok, t.vocab, H, 1, H, H);
    reg_mat(c, "clip.embeddings.position_embedding.weight", t.pos, t.T, H, 1, H, H);
    for (int l = 0; l < g.clip_layers; ++l) {
      const std::string pre = "clip.encoder.layers." + std::to_string(l);
      ClipLayerW L;
      L.ln1 = make_norm(c, pre + ".layer_norm1", H);
      L.ln2 = make_norm(c, pre + ".layer_norm2", H);
      L.w_qkv = walloc_h(c, (size_t)3 * H * H);
      L.b_qkv = walloc_f(c, 3 * H);
      reg_mat(c, pre + ".self_attn.q_proj.weight", L.w_qkv, H, H, 1, H, H, 0);
      reg_mat(c, pre + ".self_attn.k_proj.weight", L.w_qkv, H, H, 1, H, H, H);
      reg_mat(c, pre + ".self_attn.v_proj.weight", L.w_qkv, H, H, 1, H, H, 2 * H);
      reg_vec(c, pre + ".self_attn.q_proj.bias", L.b_qkv, H);
      reg_vec(c, pre + ".self_attn.k_proj.bias", L.b_qkv + H, H);
      reg_vec(c, pre + ".self_attn.v_proj.bias", L.b_qkv + 2 * H, H);
      L.out = make_lin(c, pre + ".self_attn.out_proj", H, H);
      L.fc1 = make_lin(c, pre + ".mlp.fc1", H, t.I);
      L.fc2 = make_lin(c, pre + ".mlp.fc2", t.I, H);
      t.layers.push_back(L);
    }
    t.final_ln = make_norm(c, "clip.final_layer_norm", H);
  }
}
