// api_ctrl.inc -- part of api.hip (one translation unit: included there, in this order; not compiled on its own).
// per-loop text K / V cache and the controller descriptor -> device tables (Prompt-to-Prompt, MasaCtrl, LocalBlend)
// ---------------------------------------------------------------------------------------------------- text K / V cache
static void for_each_transformer(pnpi_ctx* c, const std::function<void(const TransformerW&, int)>& fn) {
  UNetW& u = c->unet;
  int idx = 0;
  for (auto& blk : u.down_attn) for (auto& t : blk) fn(t, idx++);
  fn(u.mid_attn, idx++);
  for (auto& blk : u.up_attn) for (auto& t : blk) fn(t, idx++);
}
static size_t text_kv_bytes(pnpi_ctx* c, int rows) {
  const int T = c->cfg.ctx_len, ldv = round_up_i(T, 8);
  size_t total = 0;
  for_each_transformer(c, [&](const TransformerW& t, int) {
    const size_t hd = (size_t)t.heads * t.Dp;
    total += align_up((size_t)rows * T * hd * sizeof(half_t), 256) + align_up((size_t)rows * hd * ldv * sizeof(half_t), 256);
  });
  return total + 4096;
}
// K = context W_k^T, V^T = (context W_v^T)^T for the 16 cross-attention layers, `rows` context rows (fp32 [rows][T][X] on the device)
// share: of the forwards that will read the cache -- pinned, the projections of the compact context rows are configured as at the logical rows
static int text_kv_precompute(pnpi_ctx* c, const float* context, int rows, const UNetShare& share = UNetShare()) {
  const pnpi_model_config& g = c->cfg;
  TextKV& kv = c->tkv;
  kv.rows = 0;
  if (rows <= 0 || rows > c->max_rows) return fail(c, PNPI_EINVAL, "text K/V precompute: rows out of range (max_unet_rows)");
  if (text_kv_bytes(c, rows) > kv.cap) return fail(c, PNPI_ENOMEM, "text K/V cache arena too small");
  const int T = g.ctx_len, X = g.cross_dim, ldv = round_up_i(T, 8);
  UNetFlight fw(share); FlightScope pinned(c, &fw);
  c->persist.reset(); c->temp.reset();
  half_t* ctx16 = palloc(c, (size_t)rows * T * X);
  CK(launch_f32_to_f16(context, (size_t)rows * T * X, ctx16, c->st));
  kv.k.clear(); kv.vt.clear();
  size_t off = 0;
  int rc = 0;
  for_each_transformer(c, [&](const TransformerW& t, int) {
    if (rc) return;
    const int hd = t.heads * t.Dp;
    half_t* k2 = (half_t*)(kv.base + off); off += align_up((size_t)rows * T * hd * sizeof(half_t), 256);
    half_t* vt2 = (half_t*)(kv.base + off); off += align_up((size_t)rows * hd * ldv * sizeof(half_t), 256);
    kv.k.push_back(k2); kv.vt.push_back(vt2);
    // the V^T rows are padded to 8 keys and the blocks sit at row-count-dependent offsets: a pad column of this layout may hold another
    // row count's projection data (or anything), and the call-back path multiplies pad columns by zero probabilities -- 0 * inf = NaN.
    // Clear the block before the projection writes the real columns (as the in-forward talloc path does).
    if (ldv != T && hipMemsetAsync(vt2, 0, (size_t)rows * hd * ldv * sizeof(half_t), c->st) != hipSuccess) { rc = PNPI_EHIP; return; }
    VtOut v; v.outT = vt2; v.col0 = hd; v.ld = ldv; v.f32 = 0; v.rpb = T;
    rc = op_gemm(c, ctx16, X, rows * T, X, t.w_kv2, X, 2 * hd, nullptr, nullptr, 0, k2, hd, 1.f, &v, 2.0 * rows * T * 2.0 * t.C * X);
  });
  if (rc) return fail_launch(c, rc, "text K/V projection");
  kv.rows = rows;
  c->ctr.text_kv_rows += rows;
  return 0;
}

// ---------------------------------------------------------------------------------------------------- controller tables
static float* misc_f(pnpi_ctx* c, size_t n) { return (float*)c->ctrl_arena.alloc(n * sizeof(float)); }

static int upload(pnpi_ctx* c, void* dst, const void* src, size_t bytes) {
  CKH(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->st));
  // the host staging vectors are reused by the caller: make the copy complete before returning
  CKH(hipStreamSynchronize(c->st));
  return 0;
}

// The launch rows of one (pseudo-)image: its unconditional / conditional source and target row.  unc_src < 0: the launch has none
// (the pruned schedule).  Several pseudo-images may name the same source rows (pnpi_direct_edit with shared source rows).
struct CtrlRows { int unc_src, unc_tgt, cond_src, cond_tgt; };
// the classic layout: image i owns the rows [i * rpi, (i + 1) * rpi), cond_src / cond_tgt at src_off / tgt_off, and with four rows
// per image [unc_src, unc_tgt, cond_src, cond_tgt]
static std::vector<CtrlRows> ctrl_rows_layout(int nimg, int rpi, int src_off, int tgt_off) {
  std::vector<CtrlRows> rt(nimg > 0 ? nimg : 0);
  for (int i = 0; i < nimg; ++i)
    rt[i] = rpi == 4 ? CtrlRows{4 * i, 4 * i + 1, 4 * i + src_off, 4 * i + tgt_off} : CtrlRows{-1, -1, i * rpi + src_off, i * rpi + tgt_off};
  return rt;
}
// Build the device-side tables for `rows` UNet rows; rt [nimg] (with cds): the launch rows of every (pseudo-)image.
// mask_nimg: the images of the caller's loop when the launch holds several pseudo-images per image (pnpi_direct_edit's passes: pseudo-image
// q is image q % mask_nimg); 0 = nimg.  Only the masks of pnpi_masa_set_masks are indexed by it.
static int setup_ctrl_rows(pnpi_ctx* c, const pnpi_ctrl_desc* cds, int nimg, int rows, const CtrlRows* rt, int mask_nimg = 0) {
  CtrlDev& cd = c->cd;
  if (cds && c->mm.nimg > 0) {      // refused before anything is uploaded or launched
    bool any2 = false;
    for (int i = 0; i < nimg; ++i) any2 = any2 || cds[i].kind == 2;
    if (any2 && c->mm.nimg != (mask_nimg > 0 ? mask_nimg : nimg))
      return fail(c, PNPI_EINVAL, "pnpi_masa_set_masks holds masks for another number of images than this call's nimg");
  }
  if (cds) {
    if (!rt) return fail(c, PNPI_EINVAL, "controllers need the row table of their images");
    for (int i = 0; i < nimg; ++i) {
      const int r4[4] = {rt[i].unc_src, rt[i].unc_tgt, rt[i].cond_src, rt[i].cond_tgt};
      for (int k = 0; k < 4; ++k)
        if (r4[k] >= rows || (r4[k] < 0 && (k >= 2 || cds[i].kind == 2)))
          return fail(c, PNPI_EINVAL, cds[i].kind == 2 && r4[k] < 0 ? "MasaCtrl controllers need the 4-row layout" : "controller row outside the launch");
    }
  }
  c->ctrl_arena.reset();
  cd = CtrlDev();
  cd.nimg = nimg;
  std::vector<int> id(rows * 4), rep(rows * 4), plain, pairs;
  for (int r = 0; r < rows; ++r) { id[r * 4] = r; id[r * 4 + 1] = r; id[r * 4 + 2] = r; id[r * 4 + 3] = r; }
  rep = id;
  const int T = c->cfg.ctx_len;
  if (T > 96) return fail(c, PNPI_ESHAPE, "ctx_len > 96 unsupported by the cross-attention edit kernel");
  std::vector<int> edit_img;
  if (cds)
    for (int i = 0; i < nimg; ++i) if (cds[i].kind == 1) edit_img.push_back(i);
  if (cds) {   // MasaCtrl images (kind 2): rows [unc_src, unc_tgt, cond_src, cond_tgt]; each target row reads its half's source K, V
    std::vector<int> masa = id;
    for (int i = 0; i < nimg; ++i) {
      if (cds[i].kind != 2) continue;
      std::vector<unsigned char> step_on;
      const bool step_list = cds[i].masa_n_steps > 0 && cds[i].masa_step_on_host;
      if (step_list) step_on.assign(cds[i].masa_step_on_host, cds[i].masa_step_on_host + cds[i].masa_n_steps);
      if (cd.masa_any && (cd.masa_start_step != cds[i].masa_start_step || cd.masa_start_layer != cds[i].masa_start_layer ||
                          cd.masa_layer_mask != cds[i].masa_layer_mask || cd.masa_step_list != step_list || cd.masa_step_on != step_on))
        return fail(c, PNPI_EINVAL, "all MasaCtrl controllers of one batch must share their step / layer windows (or lists)");
      cd.masa_any = true; cd.masa_start_step = cds[i].masa_start_step; cd.masa_start_layer = cds[i].masa_start_layer;
      cd.masa_layer_mask = cds[i].masa_layer_mask; cd.masa_step_list = step_list; cd.masa_step_on = step_on;
      for (int half = 0; half < 2; ++half) {      // a shared source row serves every pseudo-image that names it
        const int src = half ? rt[i].cond_src : rt[i].unc_src, tgt = half ? rt[i].cond_tgt : rt[i].unc_tgt;
        masa[tgt * 4 + 2] = src; masa[tgt * 4 + 3] = src;
      }
    }
    if (cd.masa_any) {
      cd.rows_masa = (int*)c->ctrl_arena.alloc(masa.size() * sizeof(int));
      CKP(upload(c, cd.rows_masa, masa.data(), masa.size() * sizeof(int)));
    }
    if (cd.masa_any && c->mm.nimg > 0) {
      std::vector<int> mplain, mtgt, mimg, tgt_img(rows, -1);
      for (int i = 0; i < nimg; ++i)
        if (cds[i].kind == 2) tgt_img[rt[i].unc_tgt] = tgt_img[rt[i].cond_tgt] = i % c->mm.nimg;
      for (int r = 0; r < rows; ++r) {      // every other row of the launch takes the plain kernel, once
        if (tgt_img[r] >= 0) {
          mtgt.insert(mtgt.end(), masa.begin() + r * 4, masa.begin() + r * 4 + 4);
          mimg.push_back(tgt_img[r]);
        } else mplain.insert(mplain.end(), masa.begin() + r * 4, masa.begin() + r * 4 + 4);
      }
      cd.masa_masked = true;
      cd.n_masa_plain = (int)mplain.size() / 4; cd.n_masa_tgt = (int)mtgt.size() / 4;
      cd.rows_masa_plain = (int*)c->ctrl_arena.alloc(mplain.size() * sizeof(int));
      cd.rows_masa_tgt = (int*)c->ctrl_arena.alloc(mtgt.size() * sizeof(int));
      cd.masa_tgt_img = (int*)c->ctrl_arena.alloc(mimg.size() * sizeof(int));
      CKP(upload(c, cd.rows_masa_plain, mplain.data(), mplain.size() * sizeof(int)));
      CKP(upload(c, cd.rows_masa_tgt, mtgt.data(), mtgt.size() * sizeof(int)));
      CKP(upload(c, cd.masa_tgt_img, mimg.data(), mimg.size() * sizeof(int)));
    }
  }
  cd.any_edit = !edit_img.empty();
  cd.npairs = (int)edit_img.size();
  std::vector<bool> is_pair_row(rows, false);
  for (int i : edit_img) {
    int src = rt[i].cond_src, tgt = rt[i].cond_tgt;
    rep[tgt * 4 + 1] = src; rep[tgt * 4 + 2] = src;  // q and k of the target row come from the source row
    pairs.push_back(src); pairs.push_back(tgt);
    is_pair_row[tgt] = true;   // only the target row leaves the plain path; the source row stays bit-identical to it
    cd.pair_img.push_back(i);
  }
  for (int r = 0; r < rows; ++r) if (!is_pair_row[r]) { plain.push_back(r); plain.push_back(r); plain.push_back(r); plain.push_back(r); }
  cd.n_plain = (int)plain.size() / 4;
  cd.rows_id = (int*)c->ctrl_arena.alloc(id.size() * sizeof(int));
  cd.rows_rep = (int*)c->ctrl_arena.alloc(rep.size() * sizeof(int));
  CKP(upload(c, cd.rows_id, id.data(), id.size() * sizeof(int)));
  CKP(upload(c, cd.rows_rep, rep.data(), rep.size() * sizeof(int)));
  if (!plain.empty()) {
    cd.rows_plain = (int*)c->ctrl_arena.alloc(plain.size() * sizeof(int));
    CKP(upload(c, cd.rows_plain, plain.data(), plain.size() * sizeof(int)));
  }
  if (!cd.any_edit) return 0;
  cd.pairs = (int*)c->ctrl_arena.alloc(pairs.size() * sizeof(int));
  CKP(upload(c, cd.pairs, pairs.data(), pairs.size() * sizeof(int)));
  const pnpi_ctrl_desc& d0 = cds[edit_img[0]];
  cd.n_alpha_rows = d0.n_alpha_rows;
  cd.self_lo = d0.self_replace_lo; cd.self_hi = d0.self_replace_hi; cd.self_max_tokens = d0.self_replace_max_tokens;
  const int P = cd.npairs;
  std::vector<half_t> mm((size_t)P * 96 * 96, (half_t)0.f);
  // LocalBlend planes: {src, tgt} blend-word selectors, plus {src, tgt} substruct-word selectors when any controller of the batch has them
  int planes = 2;
  for (int pi = 0; pi < P; ++pi)
    if (cds[edit_img[pi]].lb_enabled && cds[edit_img[pi]].lb_sub_alpha_host) planes = 4;
  cd.lb_planes = planes;
  std::vector<float> coef((size_t)cd.n_alpha_rows * 2 * P * 96, 0.f), lba((size_t)P * planes * 96, 0.f);
  for (int pi = 0; pi < P; ++pi) {
    const pnpi_ctrl_desc& d = cds[edit_img[pi]];
    if (d.n_alpha_rows != cd.n_alpha_rows || d.self_replace_lo != cd.self_lo || d.self_replace_hi != cd.self_hi ||
        d.self_replace_max_tokens != cd.self_max_tokens)
      return fail(c, PNPI_EINVAL, "all controllers of one batch must share the step schedule");
    if (!d.cross_alpha_host || !d.mapper_host || !d.alphas_host || !d.equalizer_host)
      return fail(c, PNPI_EINVAL, "controller tables missing");
    for (int w = 0; w < T; ++w)
      for (int j = 0; j < T; ++j) mm[((size_t)pi * 96 + j) * 96 + w] = (half_t)d.mapper_host[w * T + j];
    for (int s = 0; s < cd.n_alpha_rows; ++s)
      for (int j = 0; j < T; ++j) {
        float a = d.cross_alpha_host[s * T + j], eq = d.equalizer_host[j], al = d.alphas_host[j];
        coef[(((size_t)s * 2 + 0) * P + pi) * 96 + j] = a * eq * al;
        coef[(((size_t)s * 2 + 1) * P + pi) * 96 + j] = a * eq * (1.f - al) + (1.f - a);
      }
    cd.lb_enabled.push_back(d.lb_enabled);
    cd.lb_start.push_back(d.lb_start);
    cd.lb_th.push_back(d.lb_threshold);
    // a pair without substruct words in a 4-plane batch: its substruct maps are all zero and never exceed an infinite threshold
    cd.lb_th_sub.push_back(d.lb_enabled && d.lb_sub_alpha_host ? d.lb_threshold_sub : INFINITY);
    if (d.lb_enabled) {
      if (!d.lb_alpha_host) return fail(c, PNPI_EINVAL, "lb_alpha missing");
      if (c->unet.lb_nslots == 0) return fail(c, PNPI_ESHAPE, "LocalBlend needs the five 16x16 cross-attention maps (latent 64x64 layout)");
      cd.lb_any = 1;
      for (int w = 0; w < 2; ++w)
        for (int j = 0; j < T; ++j) {
          lba[((size_t)pi * planes + w) * 96 + j] = d.lb_alpha_host[w * T + j];
          if (d.lb_sub_alpha_host) lba[((size_t)pi * planes + 2 + w) * 96 + j] = d.lb_sub_alpha_host[w * T + j];
        }
    }
  }
  cd.mmatT = (half_t*)c->ctrl_arena.alloc(mm.size() * sizeof(half_t));
  cd.coef = misc_f(c, coef.size());
  CKP(upload(c, cd.mmatT, mm.data(), mm.size() * sizeof(half_t)));
  CKP(upload(c, cd.coef, coef.data(), coef.size() * sizeof(float)));
  if (cd.lb_any) {
    cd.lb_alpha = misc_f(c, lba.size());
    CKP(upload(c, cd.lb_alpha, lba.data(), lba.size() * sizeof(float)));
    size_t nacc = (size_t)P * c->unet.lb_nslots * planes * c->unet.lb_tokens;
    cd.lb_acc = misc_f(c, nacc);
    CKH(hipMemsetAsync(cd.lb_acc, 0, nacc * sizeof(float), c->st));
  }
  if (c->ctrl_arena.overflow) return fail(c, PNPI_ENOMEM, "controller arena overflow");
  return 0;
}

// the classic layout (every caller but pnpi_direct_edit's shared-row launch)
static int setup_ctrl(pnpi_ctx* c, const pnpi_ctrl_desc* cds, int nimg, int rows, int rpi = 4, int src_off = 2, int tgt_off = 3, int mask_nimg = 0) {
  if (!cds) return setup_ctrl_rows(c, nullptr, nimg, rows, nullptr, mask_nimg);
  if (rows != nimg * rpi) return fail(c, PNPI_EINVAL, "controllers need rows == rows_per_image * nimg");
  const std::vector<CtrlRows> rt = ctrl_rows_layout(nimg, rpi, src_off, tgt_off);
  return setup_ctrl_rows(c, cds, nimg, rows, rt.data(), mask_nimg);
}

static int apply_local_blend(pnpi_ctx* c, float* latents /*[nimg][2][E]*/, int step_index) {
  CtrlDev& cd = c->cd;
  if (!cd.lb_any) return 0;
  const pnpi_model_config& g = c->cfg;
  const size_t E = (size_t)g.in_channels * g.sample_size * g.sample_size;
  const int mhw = (int)lroundf(sqrtf((float)c->unet.lb_tokens));
  for (int pi = 0; pi < cd.npairs; ++pi) {
    if (!cd.lb_enabled[pi]) continue;
    if (step_index + 1 <= cd.lb_start[pi]) continue;   // LocalBlend.counter > start_blend (attention_control.py:108-110)
    const float* acc = cd.lb_acc + (size_t)pi * c->unet.lb_nslots * cd.lb_planes * c->unet.lb_tokens;
    CK(launch_local_blend(acc, c->unet.lb_nslots, mhw, g.sample_size, g.in_channels, cd.lb_th[pi],
                          latents + (size_t)cd.pair_img[pi] * 2 * E, 1, c->st, cd.lb_planes, cd.lb_th_sub[pi]));
  }
  return 0;
}
