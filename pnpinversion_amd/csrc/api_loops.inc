// api_loops.inc -- part of api.hip (one translation unit: included there, last, inside its extern "C" block; not compiled on its own).
// the level-2 entry points: whole inversion / editing loops in one C call (DDIM, direct inversion, Prompt-to-Prompt edit loops,
// edit-friendly DDPM, Blended Latent Diffusion, null-text optimisation)
// ---------------------------------------------------------------------------------------------------- loop scaffold
// The loops' text context is constant over their steps: project K / V once, then every forward of the loop reads the cache.
struct LoopKV {
  pnpi_ctx* c;
  bool armed = false;      // the loop's forwards read the cache (loop_unet: UNetCall::cached_kv)
  explicit LoopKV(pnpi_ctx* c_) : c(c_) {}
  int begin(const float* context, int rows, const UNetShare& share = UNetShare()) {
    if (g_text_kv) { CKP(text_kv_precompute(c, context, rows, share)); armed = true; }
    return 0;
  }
  // a loop's projections belong to the loop's context: dropped at its end, so that a later pnpi_unet_forward(context = NULL) can
  // never silently read them (it fails and names pnpi_text_kv_precompute instead)
  ~LoopKV() { if (armed) c->tkv.rows = 0; }
};
// What every loop sets up before its first step.  Scratch lives at the top of the controller arena (after the controller tables):
//   loop_begin    entry checks, E / CE / ratio, the controller tables (setup_ctrl resets the arena)
//   misc_f ...    the loop's own scratch;  loop_map / loop_maps_cfg: its row maps, built on the host
//   loop_commit   the step buffers, ONE overflow test before anything is launched on that scratch, one upload of all the maps
//   loop_unet     a step's prologue: gather the rows of the launch, run the UNet on them
struct Loop {
  pnpi_ctx* c;
  size_t E = 0, CE = 0;                        // floats per latent (input) row / per context row
  size_t E_out = 0;                            // floats per prediction row: E unless the model's in_channels != out_channels
  int ratio = 0, rows = 0;                     // scheduler stride; UNet rows per launch
  float *in = nullptr, *eps = nullptr;         // [rows][E] gathered input (loops with row maps only) and [rows][E_out] prediction of a step
  const float* temb_rows = nullptr;            // [nsteps][C0] sinusoid rows of a loop at fractional timesteps (loop_unet: step's row) ...
  float* bias_row = nullptr;                   // ... and the loop-owned [temb_total] bias row its GEMVs write
  LoopKV kv;
  UNetShare share; PnpState pnp;               // what loop_unet puts into every call: row sharing, the step's Plug-and-Play injection
  std::vector<int> maps;                       // host copy of all row maps, back to back
  std::vector<std::pair<int**, size_t>> map_dst;
  explicit Loop(pnpi_ctx* c_) : c(c_), kv(c_) {}
};
// cds (nullable): controller descriptors of the nq (pseudo-)images of the launch, rows = rpi * nq (src_off, tgt_off, mask_nimg: setup_ctrl)
// split_io: the loop keeps input rows (E) and prediction rows (E_out) apart; every other loop steps a latent by its own prediction
struct LoopLayout { const pnpi_ctrl_desc* cds = nullptr; int nq = 0, rpi = 4, src_off = 2, tgt_off = 3, mask_nimg = 0; bool split_io = false; };
// the entry checks of loop_begin alone (a loop that builds its controller tables itself)
static int loop_entry(Loop& L, int nsteps, int rows, const char* too_many_rows, bool split_io = false) {
  pnpi_ctx* c = L.c;
  CKP(check_loop_ready(c));
  const pnpi_model_config& g = c->cfg;
  if (!split_io && g.in_channels != g.out_channels) return fail(c, PNPI_EINVAL, "this loop needs a model with in_channels == out_channels");
  L.E = (size_t)g.in_channels * g.sample_size * g.sample_size; L.CE = (size_t)g.ctx_len * g.cross_dim;
  L.E_out = (size_t)g.out_channels * g.sample_size * g.sample_size;
  L.ratio = g.n_train_timesteps / nsteps; L.rows = rows;
  if (rows > c->max_rows) return fail(c, PNPI_EINVAL, too_many_rows);
  return 0;
}
static int loop_begin(Loop& L, int nsteps, int rows, const char* too_many_rows, const LoopLayout& y = LoopLayout()) {
  pnpi_ctx* c = L.c;
  CKP(loop_entry(L, nsteps, rows, too_many_rows, y.split_io));
  return y.cds ? setup_ctrl(c, y.cds, y.nq, rows, y.rpi, y.src_off, y.tgt_off, y.mask_nimg) : setup_ctrl(c, nullptr, 0, c->max_rows);
}
static void loop_map(Loop& L, const std::vector<int>& m, int** dev) {      // *dev is valid after loop_commit
  L.map_dst.push_back({dev, L.maps.size()});
  L.maps.insert(L.maps.end(), m.begin(), m.end());
}
// nq (pseudo-)images of P latents and 2 P rows [uncond_0 .. uncond_{P-1}, cond_0 .. cond_{P-1}] each; pseudo-image q starts from image
// q % nimg:  expand: image -> its P latents,  inmap: latents -> rows.  P = 2 is the layout [unc_src, unc_tgt, cond_src, cond_tgt].
static void loop_maps_cfg(Loop& L, int nq, int nimg, int P, int** d_expand, int** d_inmap) {
  std::vector<int> expand(nq * P), inmap(nq * 2 * P);
  for (int q = 0; q < nq; ++q) {
    for (int p = 0; p < P; ++p) expand[P * q + p] = q % nimg;
    for (int k = 0; k < 2 * P; ++k) inmap[2 * P * q + k] = P * q + k % P;
  }
  loop_map(L, expand, d_expand);
  loop_map(L, inmap, d_inmap);
}
static int loop_commit(Loop& L, bool step_bufs = true) {
  pnpi_ctx* c = L.c;
  if (step_bufs) L.eps = misc_f(c, (size_t)L.rows * L.E_out);
  if (step_bufs && !L.maps.empty()) L.in = misc_f(c, (size_t)L.rows * L.E);
  int* d = (int*)c->ctrl_arena.alloc(L.maps.size() * sizeof(int));
  // Bump::alloc hands out the arena's base on overflow: nothing may be launched on (or uploaded to) such scratch
  if (c->ctrl_arena.overflow) return fail(c, PNPI_ENOMEM, "loop arena overflow");
  for (auto& m : L.map_dst) *m.first = d + m.second;
  return L.maps.empty() ? 0 : upload(c, d, L.maps.data(), L.maps.size() * sizeof(int));
}
// inmap == NULL: lat already holds the rows of the launch.  Otherwise lat holds the distinct latents of the step and inmap (one of the
// loop's committed maps) sends every row to its latent: unet_fwd gets both, and runs what depends on the latent alone once per latent
static int loop_unet(Loop& L, const float* lat, const int* inmap, int t, const float* ctx, bool use_ctrl, int step) {
  pnpi_ctx* c = L.c;
  UNetCall k; k.latents = lat; k.rows = L.rows; k.t = t; k.context = ctx; k.use_ctrl = use_ctrl; k.cur_step = step; k.eps_out = L.eps;
  k.cached_kv = L.kv.armed; k.share = L.share; k.pnp = L.pnp.on ? &L.pnp : nullptr;
  if (L.temb_rows) { k.temb_row = L.temb_rows + (size_t)step * c->cfg.block_out_channels[0]; k.bias_row = L.bias_row; }
  if (!inmap) return unet_fwd(c, k);
  CK(launch_gather_rows_f32(lat, inmap, L.rows, L.E, L.in, c->st));
  k.latents = L.in;
  UNetDedup ud{lat, 0, nullptr, inmap};
  for (auto& m : L.map_dst)
    if (*m.first == inmap && m.second + (size_t)L.rows <= L.maps.size()) ud.hmap = L.maps.data() + m.second;
  for (int r = 0; ud.hmap && r < L.rows; ++r) ud.U = ud.hmap[r] + 1 > ud.U ? ud.hmap[r] + 1 : ud.U;
  if (ud.hmap) k.dedup = &ud;
  return unet_fwd(c, k);
}
// dst rows [img][uncond, cond] (ctx_cond == NULL: [img][uncond])
static int interleave_ctx(pnpi_ctx* c, float* dst, const float* ctx_uncond, const float* ctx_cond, int nimg, size_t CE) {
  const size_t w = CE * sizeof(float), pitch = (ctx_cond ? 2 : 1) * w;
  CKH(hipMemcpy2DAsync(dst, pitch, ctx_uncond, w, w, nimg, hipMemcpyDeviceToDevice, c->st));
  if (ctx_cond) CKH(hipMemcpy2DAsync(dst + CE, pitch, ctx_cond, w, w, nimg, hipMemcpyDeviceToDevice, c->st));
  return 0;
}
// the plain CFG + DDIM step of a loop: P latents per image, rows [uncond x P, cond x P] of eps
static CfgStepP cfg_step(const Loop& L, const float* eps, const float* x, int nimg, int P, float gs, float a_from, float a_to, float* x_out) {
  CfgStepP s;
  s.eps = eps; s.x = x; s.nimg = nimg; s.rows_per_img = P; s.row_elems = L.E; s.gscale = gs; s.a_t = a_from; s.a_prev = a_to; s.x_out = x_out;
  return s;
}

// ---------------------------------------------------------------------------------------------------- DDIM / direct inversion
int pnpi_ddim_invert(pnpi_ctx* c, const float* z0, int nimg, const float* ctx_cond, int nsteps, const int* ts, float* all) {
  if (!c || !z0 || !ctx_cond || !ts || !all || nsteps <= 0) return PNPI_EINVAL;
  Loop L(c);
  CKP(loop_begin(L, nsteps, nimg, "nimg exceeds max_unet_rows"));
  CKP(loop_commit(L));
  const size_t E = L.E;
  CKH(hipMemcpyAsync(all, z0, (size_t)nimg * E * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  CKP(L.kv.begin(ctx_cond, nimg));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[nsteps - i - 1];
    const float* cur = all + (size_t)i * nimg * E;
    CKP(loop_unet(L, cur, nullptr, t, ctx_cond, false, 0));
    float af, at; CKP(alphas_for(c, t, L.ratio, true, &af, &at));
    CK(launch_ddim_move(cur, L.eps, af, at, (size_t)nimg * E, all + (size_t)(i + 1) * nimg * E, c->st));
  }
  return 0;
}

/* DirectInversion.ddim_with_guidance_scale_loop (inversion.py:334-347): inversion under classifier-free guidance.  The reference
 * makes two B=1 UNet calls per step (uncond, cond); here they are the two rows of one launch. */
int pnpi_ddim_invert_cfg(pnpi_ctx* c, const float* z0, int nimg, const float* ctx_uncond, const float* ctx_cond, float gs, int nsteps,
                         const int* ts, float* all) {
  if (!c || !z0 || !ctx_uncond || !ctx_cond || !ts || !all || nsteps <= 0) return PNPI_EINVAL;
  Loop L(c);
  CKP(loop_begin(L, nsteps, 2 * nimg, "nimg * 2 exceeds max_unet_rows"));
  const size_t E = L.E;
  float* ctx2 = misc_f(c, (size_t)L.rows * L.CE);
  std::vector<int> inmap(L.rows);
  for (int r = 0; r < L.rows; ++r) inmap[r] = r / 2;
  int* d_inmap;
  loop_map(L, inmap, &d_inmap);
  CKP(loop_commit(L));
  CKP(interleave_ctx(c, ctx2, ctx_uncond, ctx_cond, nimg, L.CE));
  CKH(hipMemcpyAsync(all, z0, (size_t)nimg * E * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  CKP(L.kv.begin(ctx2, L.rows));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[nsteps - i - 1];
    const float* cur = all + (size_t)i * nimg * E;
    CKP(loop_unet(L, cur, d_inmap, t, ctx2, false, 0));
    float af, at; CKP(alphas_for(c, t, L.ratio, true, &af, &at));
    // noise = eps_u + gs * (eps_c - eps_u); next_step (the same fused kernel as the denoising direction, other alphas)
    CK(launch_cfg_ddim_prev(cfg_step(L, L.eps, cur, nimg, 1, gs, af, at, all + (size_t)(i + 1) * nimg * E), c->st));
  }
  return 0;
}

int pnpi_offset_calculate(pnpi_ctx* c, const float* lat_all, int nimg, const float* context4, int nsteps, const int* ts, float gs,
                          const float* offset_scale_host, float* noise_loss_out) {
  if (!c || !lat_all || !context4 || !ts || !noise_loss_out || nsteps <= 0) return PNPI_EINVAL;
  Loop L(c);
  CKP(loop_begin(L, nsteps, 4 * nimg, "nimg * 4 exceeds max_unet_rows"));
  const size_t E = L.E;
  float* cur = misc_f(c, (size_t)nimg * 2 * E);
  int *d_expand, *d_inmap;
  loop_maps_cfg(L, nimg, nimg, 2, &d_expand, &d_inmap);
  CKP(loop_commit(L));
  CK(launch_gather_rows_f32(lat_all + (size_t)nsteps * nimg * E, d_expand, nimg * 2, E, cur, c->st));
  CKP(L.kv.begin(context4, L.rows));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[i];
    CKP(loop_unet(L, cur, d_inmap, t, context4, false, 0));
    float af, at; CKP(alphas_for(c, t, L.ratio, false, &af, &at));
    CfgStepP s = cfg_step(L, L.eps, cur, nimg, 2, gs, af, at, cur);
    s.target = lat_all + (size_t)(nsteps - i - 1) * nimg * E; s.offset_scale = offset_scale_host ? offset_scale_host[i] : 1.f;
    s.offset_out = noise_loss_out + (size_t)i * nimg * 2 * E;
    CK(launch_cfg_ddim_prev(s, c->st));
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------- edit loops
// uncond_steps (nullable): [nsteps][nimg][77][768] per-step unconditional embeddings (null-text inversion).  p2p_guidance_forward uses the
// step's embedding for every unconditional row of the image (p2p_guidance_forward.py:56-57); uncond_first_only = the single-branch variant
// (:92: the first row only).  The text K / V are then projected once per STEP instead of once per loop.
static int edit_loop_impl(pnpi_ctx* c, const float* x_T, int nimg, const float* context4, const float* noise_loss, int offset_rows,
                          const pnpi_ctrl_desc* ctrl_host, int nsteps, const int* ts, float gs, int prox, float quantile,
                          const pnpi_recon_desc* recon, float* latents_out, const float* uncond_steps, int uncond_first_only) {
  if (!c || !x_T || !context4 || !ts || !latents_out || nsteps <= 0) return PNPI_EINVAL;
  CKP(recon_check(c, recon));
  if (prox < 0 || prox > 2) return fail(c, PNPI_EINVAL, "prox must be 0 (none), 1 (l0) or 2 (l1)");
  Loop L(c);
  LoopLayout lay; lay.cds = ctrl_host; lay.nq = nimg;
  CKP(loop_begin(L, nsteps, 4 * nimg, "nimg * 4 exceeds max_unet_rows", lay));
  const size_t E = L.E, CE = L.CE; const int rows = L.rows, S = c->cfg.sample_size;
  const bool use_ctrl = ctrl_host != nullptr;
  float* lat = misc_f(c, (size_t)nimg * 2 * E);
  float* thr = misc_f(c, (size_t)nimg);
  float* ctx_step = uncond_steps ? misc_f(c, (size_t)rows * CE) : nullptr;
  int *d_expand, *d_inmap;
  loop_maps_cfg(L, nimg, nimg, 2, &d_expand, &d_inmap);
  CKP(loop_commit(L));
  CK(launch_gather_rows_f32(x_T, d_expand, nimg * 2, E, lat, c->st));
  if (prox && !(quantile > 0.f)) CK(launch_fill_f32(thr, nimg, -quantile, c->st));   // negative quantile = fixed threshold (:43-44)
  if (uncond_steps) CKH(hipMemcpyAsync(ctx_step, context4, (size_t)rows * CE * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  else CKP(L.kv.begin(context4, rows));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[i];
    const float* ctx_i = context4;
    if (uncond_steps) {
      for (int im = 0; im < nimg; ++im) {
        const float* u = uncond_steps + ((size_t)i * nimg + im) * CE;
        CKH(hipMemcpyAsync(ctx_step + (size_t)(4 * im) * CE, u, CE * sizeof(float), hipMemcpyDeviceToDevice, c->st));
        if (!uncond_first_only) CKH(hipMemcpyAsync(ctx_step + (size_t)(4 * im + 1) * CE, u, CE * sizeof(float), hipMemcpyDeviceToDevice, c->st));
      }
      ctx_i = ctx_step;
      CKP(L.kv.begin(ctx_i, rows));
    }
    CKP(loop_unet(L, lat, d_inmap, t, ctx_i, use_ctrl, i));
    float af, at; CKP(alphas_for(c, t, L.ratio, false, &af, &at));
    CfgStepP s = cfg_step(L, L.eps, lat, nimg, 2, gs, af, at, lat);
    if (noise_loss) { s.noise_loss = noise_loss + (size_t)i * nimg * 2 * E; s.offset_rows = offset_rows; }
    if (prox) {
      if (quantile > 0.f) CK(launch_quantile_abs_diff(L.eps, nimg, 2, E, quantile, thr, c->st));
      s.prox_thr = thr; s.prox_mode = prox;
      s.recon_ref = recon_ref_at(recon, t);
      // inversion guidance: x_stars[len(x_stars) - i - 2] (proximal_guidance_forward.py:75), one latent per image for both of its rows
      if (recon_inv_at(recon, t)) s.inv_ref = recon->inv_x_stars + (size_t)(nsteps - 1 - i) * nimg * E;
      if (s.recon_ref || s.inv_ref) { s.recon_lr = recon->recon_lr; s.dilate = recon->dilate_mask; s.lat_h = s.lat_w = S; }
    }
    CK(launch_cfg_ddim_prev(s, c->st));
    if (use_ctrl) CKP(apply_local_blend(c, lat, i));
  }
  CKH(hipMemcpyAsync(latents_out, lat, (size_t)nimg * 2 * E * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  return 0;
}
int pnpi_edit_loop(pnpi_ctx* c, const float* x_T, int nimg, const float* context4, const float* noise_loss, int offset_rows,
                   const pnpi_ctrl_desc* ctrl_host, int nsteps, const int* ts, float gs, int prox, float quantile,
                   const pnpi_recon_desc* recon, float* latents_out) {
  return edit_loop_impl(c, x_T, nimg, context4, noise_loss, offset_rows, ctrl_host, nsteps, ts, gs, prox, quantile, recon, latents_out, nullptr, 0);
}
int pnpi_edit_loop_uncond_steps(pnpi_ctx* c, const float* x_T, int nimg, const float* context4, const pnpi_ctrl_desc* ctrl_host, int nsteps,
                                const int* ts, float gs, int prox, float quantile, const float* uncond_steps, int uncond_first_only,
                                float* latents_out) {
  return pnpi_edit_loop_uncond_steps_recon(c, x_T, nimg, context4, ctrl_host, nsteps, ts, gs, prox, quantile, uncond_steps, uncond_first_only, nullptr, latents_out);
}
// the same with reconstruction guidance (null-text-inversion+proximal-guidance, use_reconstruction_guidance=True: p2p_editor.py:620-627)
int pnpi_edit_loop_uncond_steps_recon(pnpi_ctx* c, const float* x_T, int nimg, const float* context4, const pnpi_ctrl_desc* ctrl_host, int nsteps,
                                      const int* ts, float gs, int prox, float quantile, const float* uncond_steps, int uncond_first_only,
                                      const pnpi_recon_desc* recon, float* latents_out) {
  if (!uncond_steps) return PNPI_EINVAL;
  return edit_loop_impl(c, x_T, nimg, context4, nullptr, 1, ctrl_host, nsteps, ts, gs, prox, quantile, recon, latents_out, uncond_steps,
                        uncond_first_only);
}

/* The row maps of pnpi_direct_edit's shared-row launch (tuning "src_share"), host only.  Logical rows: pseudo-image q = p * nimg + im
 * (pass p = 0 the offset pass O, then the npass guidance passes) owns the rows 4 q .. 4 q + 3 = [unc_src, unc_tgt, cond_src, cond_tgt] on
 * the latents 2 q (source) and 2 q + 1 (target).  The source rows of every pass repeat those of the offset pass bit for bit, so the
 * launch holds, per image, O0 O1 O2 O3 and the two target rows of each guidance pass (4 + 2 npass rows on 2 + npass latents):
 *   lsel [compact latent] -> logical latent     cmap [compact row] -> compact latent     cctx [compact row] -> context4 row
 *   omap [logical row] -> compact row */
struct SrcShareMaps { std::vector<int> lsel, cmap, cctx, omap; int crows = 0, nlat = 0; };
static void src_share_maps(int nimg, int npass, SrcShareMaps& m) {
  const int rpi = 4 + 2 * npass, lpi = 2 + npass;
  m.crows = rpi * nimg; m.nlat = lpi * nimg;
  m.lsel.assign(m.nlat, 0); m.cmap.assign(m.crows, 0); m.cctx.assign(m.crows, 0); m.omap.assign((size_t)(1 + npass) * 4 * nimg, 0);
  for (int im = 0; im < nimg; ++im) {
    const int rb = im * rpi, lb = im * lpi;
    m.lsel[lb] = 2 * im; m.lsel[lb + 1] = 2 * im + 1;
    for (int k = 0; k < 4; ++k) { m.cmap[rb + k] = lb + k % 2; m.cctx[rb + k] = 4 * im + k; }
    for (int p = 1; p <= npass; ++p) {
      m.lsel[lb + 1 + p] = 2 * (p * nimg + im) + 1;
      for (int h = 0; h < 2; ++h) { m.cmap[rb + 2 + 2 * p + h] = lb + 1 + p; m.cctx[rb + 2 + 2 * p + h] = 4 * im + 2 * h + 1; }
    }
    for (int p = 0; p <= npass; ++p)
      for (int k = 0; k < 4; ++k) m.omap[4 * (p * nimg + im) + k] = (p == 0 || k % 2 == 0) ? rb + k : rb + 2 + 2 * p + k / 2;
  }
}
int pnpi_src_share_maps(int nimg, int npass, int* lsel, int* cmap, int* cctx, int* omap, int* compact_rows, int* compact_latents) {
  if (nimg <= 0 || npass <= 0 || (long)(1 + npass) * 4 * nimg > (1 << 20)) return PNPI_EINVAL;
  SrcShareMaps m;
  src_share_maps(nimg, npass, m);
  if (lsel) std::copy(m.lsel.begin(), m.lsel.end(), lsel);
  if (cmap) std::copy(m.cmap.begin(), m.cmap.end(), cmap);
  if (cctx) std::copy(m.cctx.begin(), m.cctx.end(), cctx);
  if (omap) std::copy(m.omap.begin(), m.omap.end(), omap);
  if (compact_rows) *compact_rows = m.crows;
  if (compact_latents) *compact_latents = m.nlat;
  return 0;
}

/* offset_calculate + npass guidance-forward passes of P2PEditor.edit_image_directinversion (p2p_editor.py:99-160) advanced in
 * lock step: every pass walks the same timesteps and pass p's step i needs only noise_loss[i], which the offset pass produces
 * at the same step -- so one UNet launch per step serves all (1 + npass) * 4 * nimg rows.
 * Tuning "src_share": the unconditional and conditional SOURCE rows of the guidance passes repeat the offset pass's (same x_T, same
 * context rows, no controller writes a source row, and with offset_rows >= 1 every pass advances its source latent by the same
 * __fadd_rn(prev, noise_loss[i])), so the launch holds them once (src_share_maps) and eps is expanded to the logical rows behind it;
 * every latent, offset and output below keeps its layout.  Falls back to the full launch where that identity is not given. */
int pnpi_direct_edit(pnpi_ctx* c, const float* lat_all, int nimg, const float* context4, int npass, const pnpi_ctrl_desc* ctrl_host,
                     int offset_rows, int nsteps, const int* ts, float gs, const float* offset_scale_host, float* noise_loss_out,
                     float* latents_out) {
  if (!c || !lat_all || !context4 || !ts || !noise_loss_out || !latents_out || nsteps <= 0 || npass <= 0 || nimg <= 0) return PNPI_EINVAL;
  const int NI = (1 + npass) * nimg, rows = 4 * NI;
  std::vector<pnpi_ctrl_desc> cds(NI);
  memset(cds.data(), 0, cds.size() * sizeof(pnpi_ctrl_desc));      // the offset pass (pseudo-images 0..nimg-1) runs no controller
  if (ctrl_host) for (int i = 0; i < npass * nimg; ++i) cds[nimg + i] = ctrl_host[i];
  // Not on a recording context, under a host attention callback or in a sizing run.  This loop never records itself, so "recording
  // context" can only mean one that holds an activation tape (pnpi_unet_context_grad or a null-text loop ran on it); nothing in the
  // compact launch depends on the tape -- the fallback is the specified behaviour, visible in unet_shared_rows, not a necessity.
  bool can_share = offset_rows >= 1 && !c->attn_cb && !c->dry;
  for (const pnpi_ctrl_desc& d : cds) if (d.kind < 0 || d.kind > 2) can_share = false;
  const int share = (can_share && !c->tape) ? g_src_share : 0;
  // Free tile choice (1) on a context that keeps the full launch for its tape only: the full launch is configured as the compact one
  // would be (the pin of 2, turned round), so a context gives the same bits with and without a tape -- as it does under 0 and 2
  const bool mirror = can_share && c->tape && g_src_share == 1;
  Loop L(c);
  SrcShareMaps sm;
  const char* too_many = "(1 + npass) * nimg * 4 exceeds max_unet_rows";
  if (share) {
    src_share_maps(nimg, npass, sm);
    std::vector<CtrlRows> rt(NI);
    for (int q = 0; q < NI; ++q) rt[q] = CtrlRows{sm.omap[4 * q], sm.omap[4 * q + 1], sm.omap[4 * q + 2], sm.omap[4 * q + 3]};
    CKP(loop_entry(L, nsteps, rows, too_many));      // the logical rows are what max_unet_rows admits, whatever the knob says
    L.rows = sm.crows;
    CKP(setup_ctrl_rows(c, cds.data(), NI, sm.crows, rt.data(), nimg));
    L.share = UNetShare{sm.crows, rows, 2 * NI, share == 2};
  } else {
    LoopLayout lay; lay.cds = cds.data(); lay.nq = NI; lay.mask_nimg = nimg;
    CKP(loop_begin(L, nsteps, rows, too_many, lay));
    if (mirror) { src_share_maps(nimg, npass, sm); L.share = UNetShare{rows, sm.crows, sm.nlat, true}; }
  }
  const size_t E = L.E, CE = L.CE;
  float* lat = misc_f(c, (size_t)NI * 2 * E);
  float* ctxrep = misc_f(c, (size_t)L.rows * CE);
  float* latc = share ? misc_f(c, (size_t)sm.nlat * E) : nullptr;      // the distinct latents of the step
  float* eps_all = share ? misc_f(c, (size_t)rows * E) : nullptr;      // eps at the logical rows
  int *d_expand, *d_inmap, *d_ctxmap, *d_lsel = nullptr, *d_omap = nullptr;
  if (share) {
    std::vector<int> expand(NI * 2);
    for (int k = 0; k < NI * 2; ++k) expand[k] = k / 2 % nimg;
    loop_map(L, expand, &d_expand);
    loop_map(L, sm.cmap, &d_inmap); loop_map(L, sm.cctx, &d_ctxmap); loop_map(L, sm.lsel, &d_lsel); loop_map(L, sm.omap, &d_omap);
  } else {
    std::vector<int> ctxmap(rows);
    for (int r = 0; r < rows; ++r) ctxmap[r] = 4 * (r / 4 % nimg) + r % 4;
    loop_maps_cfg(L, NI, nimg, 2, &d_expand, &d_inmap);
    loop_map(L, ctxmap, &d_ctxmap);
  }
  CKP(loop_commit(L));
  CK(launch_gather_rows_f32(lat_all + (size_t)nsteps * nimg * E, d_expand, NI * 2, E, lat, c->st));
  CK(launch_gather_rows_f32(context4, d_ctxmap, L.rows, CE, ctxrep, c->st));
  CKP(L.kv.begin(ctxrep, L.rows, L.share));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[i];
    const float* eps = L.eps;
    if (share) {
      CK(launch_gather_rows_f32(lat, d_lsel, sm.nlat, E, latc, c->st));
      CKP(loop_unet(L, latc, d_inmap, t, ctxrep, true, i));
      CK(launch_gather_rows_f32(L.eps, d_omap, rows, E, eps_all, c->st));
      eps = eps_all;
      // the counters keep counting the rows served; unet_shared_rows tells how many of them were not launched
      const uint64_t saved = (uint64_t)(rows - sm.crows);
      c->ctr.unet_sample_forwards += saved; c->ctr.unet_shared_rows += saved;
      if (L.kv.armed) c->ctr.unet_sample_forwards_cached_kv += saved;
    } else {
      CKP(loop_unet(L, lat, d_inmap, t, ctxrep, true, i));
    }
    float af, at; CKP(alphas_for(c, t, L.ratio, false, &af, &at));
    float* nl = noise_loss_out + (size_t)i * nimg * 2 * E;
    CfgStepP s = cfg_step(L, eps, lat, nimg, 2, gs, af, at, lat);
    s.target = lat_all + (size_t)(nsteps - i - 1) * nimg * E; s.offset_scale = offset_scale_host ? offset_scale_host[i] : 1.f; s.offset_out = nl;
    CK(launch_cfg_ddim_prev(s, c->st));
    for (int p = 1; p <= npass; ++p) {
      float* lp = lat + (size_t)p * nimg * 2 * E;
      s = cfg_step(L, eps + (size_t)p * nimg * 4 * E, lp, nimg, 2, gs, af, at, lp);
      s.noise_loss = nl; s.offset_rows = offset_rows;
      CK(launch_cfg_ddim_prev(s, c->st));
    }
    CKP(apply_local_blend(c, lat, i));
  }
  CKH(hipMemcpyAsync(latents_out, lat + (size_t)nimg * 2 * E, (size_t)npass * nimg * 2 * E * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  return 0;
}

/* The pruned-equivalent schedule of SURVEY.md Note D (algebra, not approximation): in direct-inversion mode the source latent after
 * every step is prev + (x*_{t-1} - prev) == x*_{t-1}, and no controller ever touches the unconditional rows or the conditional
 * source row's output.  So the offset pass and the reconstruction pass are redundant, the source latent can be ASSIGNED from the
 * stored trajectory, and the unconditional-source row is dead: one 3-row launch per step and image
 * [uncond_tgt, cond_src (attention maps only), cond_tgt] instead of 12.  200 sample-forwards per image instead of 650.
 * context4 rows as everywhere: [unc_src, unc_tgt, cond_src, cond_tgt] per image (row 0 is not used). */
int pnpi_direct_edit_pruned(pnpi_ctx* c, const float* lat_all, int nimg, const float* context4, const pnpi_ctrl_desc* ctrl_host,
                            int nsteps, const int* ts, float gs, float* latents_out) {
  if (!c || !lat_all || !context4 || !ts || !latents_out || nsteps <= 0 || nimg <= 0) return PNPI_EINVAL;
  std::vector<pnpi_ctrl_desc> none(nimg);
  memset(none.data(), 0, none.size() * sizeof(pnpi_ctrl_desc));
  Loop L(c);
  LoopLayout lay; lay.cds = ctrl_host ? ctrl_host : none.data(); lay.nq = nimg; lay.rpi = 3; lay.src_off = 1; lay.tgt_off = 2;
  CKP(loop_begin(L, nsteps, 3 * nimg, "3 * nimg exceeds max_unet_rows", lay));
  const size_t E = L.E, CE = L.CE; const int rows = L.rows;
  float* lat = misc_f(c, (size_t)nimg * 2 * E);      // [img][src, tgt]
  float* eps2 = misc_f(c, (size_t)nimg * 2 * E);     // [img][unc_tgt, cond_tgt]
  float* xt = misc_f(c, (size_t)nimg * E);
  float* ctx3 = misc_f(c, (size_t)rows * CE);
  std::vector<int> expand(nimg * 2), inmap(rows), ctxmap(rows), epsmap(nimg * 2), tgtmap(nimg);
  for (int i = 0; i < nimg; ++i) {
    expand[2 * i] = i; expand[2 * i + 1] = i;
    inmap[3 * i] = 2 * i + 1; inmap[3 * i + 1] = 2 * i; inmap[3 * i + 2] = 2 * i + 1;
    ctxmap[3 * i] = 4 * i + 1; ctxmap[3 * i + 1] = 4 * i + 2; ctxmap[3 * i + 2] = 4 * i + 3;
    epsmap[2 * i] = 3 * i; epsmap[2 * i + 1] = 3 * i + 2;
    tgtmap[i] = 2 * i + 1;
  }
  int *d_expand, *d_inmap, *d_ctxmap, *d_epsmap, *d_tgtmap;
  loop_map(L, expand, &d_expand); loop_map(L, inmap, &d_inmap); loop_map(L, ctxmap, &d_ctxmap);
  loop_map(L, epsmap, &d_epsmap); loop_map(L, tgtmap, &d_tgtmap);
  CKP(loop_commit(L));
  CK(launch_gather_rows_f32(lat_all + (size_t)nsteps * nimg * E, d_expand, nimg * 2, E, lat, c->st));      // both rows start from x*_T
  CK(launch_gather_rows_f32(context4, d_ctxmap, rows, CE, ctx3, c->st));
  CKP(L.kv.begin(ctx3, rows));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[i];
    CKP(loop_unet(L, lat, d_inmap, t, ctx3, true, i));
    float af, at; CKP(alphas_for(c, t, L.ratio, false, &af, &at));
    CK(launch_gather_rows_f32(L.eps, d_epsmap, nimg * 2, E, eps2, c->st));
    CK(launch_gather_rows_f32(lat, d_tgtmap, nimg, E, xt, c->st));
    CK(launch_cfg_ddim_prev(cfg_step(L, eps2, xt, nimg, 1, gs, af, at, xt), c->st));
    // source latent := x*_{t-1} (assigned, not reconstructed); target latent := the step's result
    const float* target = lat_all + (size_t)(nsteps - i - 1) * nimg * E;
    CKH(hipMemcpy2DAsync(lat, 2 * E * sizeof(float), target, E * sizeof(float), E * sizeof(float), nimg, hipMemcpyDeviceToDevice, c->st));
    CKH(hipMemcpy2DAsync(lat + E, 2 * E * sizeof(float), xt, E * sizeof(float), E * sizeof(float), nimg, hipMemcpyDeviceToDevice, c->st));
    CKP(apply_local_blend(c, lat, i));
  }
  CKH(hipMemcpyAsync(latents_out, lat, (size_t)nimg * 2 * E * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  return 0;
}

// ---------------------------------------------------------------------------------------------------- edit-friendly DDPM inversion
// models/edit_friendly_ddm/inversion_utils.py (eta > 0: the forward process stores one noise map per step, the reverse process replays
// them).  Scalars: ef_step_scalars (step.hip), the reference's 0-dim fp32 expressions in its order.
int pnpi_ef_step_scalars(const float* alphas_cumprod, int n, float final_alpha, int t, int step_ratio, float eta, float* out6) {
  if (!alphas_cumprod || !out6 || t < 0 || t >= n || step_ratio <= 0) return PNPI_EINVAL;
  const int tp = t - step_ratio;
  ef_step_scalars(alphas_cumprod[t], tp >= 0 ? alphas_cumprod[tp] : final_alpha, eta, out6);
  return 0;
}
static int ef_scalars(pnpi_ctx* c, int t, int ratio, float eta, float* sc) {
  if (!c->sched_set) return fail(c, PNPI_ESTATE, "pnpi_set_scheduler not called");
  if (t < 0 || t >= (int)c->ac.size() || ratio <= 0) return fail(c, PNPI_EINVAL, "timestep out of range");
  return pnpi_ef_step_scalars(c->ac.data(), (int)c->ac.size(), c->final_alpha, t, ratio, eta, sc);
}
// (sqrt(ab[t]), sqrt(1 - ab[t])) of level 1 + k, k in draw order (timestep ts[nsteps - 1 - k]), uploaded to the controller arena
static int ef_levels(pnpi_ctx* c, int nsteps, const int* ts, float** dst) {
  if (!c->sched_set) return fail(c, PNPI_ESTATE, "pnpi_set_scheduler not called");
  std::vector<float> lev(2 * (size_t)nsteps);
  for (int k = 0; k < nsteps; ++k) {
    const int t = ts[nsteps - 1 - k];
    if (t < 0 || t >= (int)c->ac.size()) return fail(c, PNPI_EINVAL, "timestep out of range");
    lev[2 * k] = sqrtf(c->ac[t]);
    lev[2 * k + 1] = sqrtf(1.0f - c->ac[t]);
  }
  *dst = misc_f(c, lev.size());
  if (c->ctrl_arena.overflow) return fail(c, PNPI_ENOMEM, "loop arena overflow");
  return upload(c, *dst, lev.data(), lev.size() * sizeof(float));
}

int pnpi_ef_sample_xts(pnpi_ctx* c, const float* x0, int nimg, const float* noise, size_t row_elems, int nsteps, const int* ts, float* xts_out) {
  if (!c || !x0 || !noise || !ts || !xts_out || nimg <= 0 || nsteps <= 0 || row_elems == 0) return PNPI_EINVAL;
  CKP(setup_ctrl(c, nullptr, 0, c->max_rows));
  float* lev;
  CKP(ef_levels(c, nsteps, ts, &lev));
  CK(launch_ef_sample_xts(x0, noise, lev, nsteps, (size_t)nimg * row_elems, xts_out, c->st));
  return 0;
}

int pnpi_ef_noise_map(pnpi_ctx* c, const float* eps, int cfg, float cfg_scale, const float* xt, float* xprev, float* z_out, int nimg,
                      size_t row_elems, int t, int step_ratio, float eta) {
  if (!c || !eps || !xt || !xprev || !z_out || nimg <= 0 || row_elems == 0) return PNPI_EINVAL;
  if (!(eta > 0.f)) return fail(c, PNPI_EINVAL, "edit-friendly inversion needs eta > 0 (eta = 0 stores no noise maps)");
  float sc[6]; CKP(ef_scalars(c, t, step_ratio, eta, sc));
  CK(launch_ef_noise_map(eps, cfg ? 1 : 0, cfg_scale, xt, xprev, z_out, nimg, row_elems, sc, c->st));
  return 0;
}

int pnpi_ef_reverse_step(pnpi_ctx* c, const float* eps, const float* x, const float* z, int nimg, int nprompts, size_t row_elems,
                         const float* cfg_scales_host, int t, int step_ratio, float eta, float* out) {
  if (!c || !eps || !x || !z || !cfg_scales_host || !out || nimg <= 0 || row_elems == 0) return PNPI_EINVAL;
  if (nprompts != 1 && nprompts != 2) return fail(c, PNPI_EINVAL, "nprompts must be 1 or 2");
  float sc[6]; CKP(ef_scalars(c, t, step_ratio, eta, sc));
  CK(launch_ef_reverse_step(eps, x, z, nimg, nprompts, row_elems, cfg_scales_host[0], cfg_scales_host[nprompts - 1], sc, eta > 0.f ? 1 : 0,
                            out, c->st));
  return 0;
}

/* inversion_forward_process (inversion_utils.py:100-176) for nimg images: xts from x0 and the caller's draws, then for t = ts[0] .. ts[nsteps-1]
 * (idx = nsteps-1 .. 0) one UNet launch of the rows [img][uncond, cond] (uncond only when ctx_cond is NULL: prompt "") on xts[idx+1], and the
 * noise map / corrected xts[idx] of that step.  zs[0] is zeroed at the end (:173-174). */
int pnpi_ef_invert(pnpi_ctx* c, const float* x0, int nimg, const float* noise, const float* ctx_uncond, const float* ctx_cond, float cfg_scale,
                   const float* etas_host, int nsteps, const int* ts, float* xts_out, float* zs_out) {
  if (!c || !x0 || !noise || !ctx_uncond || !etas_host || !ts || !xts_out || !zs_out || nimg <= 0 || nsteps <= 0) return PNPI_EINVAL;
  for (int k = 0; k < nsteps; ++k)
    if (!(etas_host[k] > 0.f)) return fail(c, PNPI_EINVAL, "edit-friendly inversion needs eta > 0 at every step");
  const int rpi = ctx_cond ? 2 : 1;
  Loop L(c);
  CKP(loop_begin(L, nsteps, rpi * nimg, "nimg * (1 + has_cond) exceeds max_unet_rows"));
  const size_t E = L.E, N = (size_t)nimg * E;
  float* ctx2 = misc_f(c, (size_t)L.rows * L.CE);
  std::vector<int> inmap(L.rows);
  for (int r = 0; r < L.rows; ++r) inmap[r] = r / rpi;
  int* d_inmap;
  loop_map(L, inmap, &d_inmap);
  float* lev;
  CKP(ef_levels(c, nsteps, ts, &lev));
  CKP(loop_commit(L));
  CKP(interleave_ctx(c, ctx2, ctx_uncond, ctx_cond, nimg, L.CE));
  CKH(hipMemcpyAsync(xts_out, x0, N * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  CK(launch_ef_sample_xts(x0, noise, lev, nsteps, N, xts_out, c->st));
  CKP(L.kv.begin(ctx2, L.rows));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[i], idx = nsteps - 1 - i;
    const float* xt = xts_out + (size_t)(idx + 1) * N;
    CKP(loop_unet(L, xt, d_inmap, t, ctx2, false, 0));
    float sc[6]; CKP(ef_scalars(c, t, L.ratio, etas_host[idx], sc));
    CK(launch_ef_noise_map(L.eps, ctx_cond ? 1 : 0, cfg_scale, xt, xts_out + (size_t)idx * N, zs_out + (size_t)idx * N, nimg, E, sc, c->st));
  }
  CKH(hipMemsetAsync(zs_out, 0, N * sizeof(float), c->st));
  return 0;
}

/* inversion_reverse_process (inversion_utils.py:210-262) with stored noise maps, nimg images x nprompts prompt rows: the last nsteps_run of the
 * nsteps_total timesteps, step k (0-based) at t = ts[nsteps_total - nsteps_run + k] replays zs[nsteps_run-1-k] with etas[nsteps_run-1-k].
 * One UNet launch of 2 * nprompts * nimg rows per step, per image [uncond_0 .. uncond_{P-1}, cond_0 .. cond_{P-1}] (the reference's uncond and
 * cond calls); with two prompts that is the controller layout [uncond_src, uncond_tgt, cond_src, cond_tgt], and the controller's step index
 * runs from 0 (the edit pass's own cur_step). */
int pnpi_ef_edit(pnpi_ctx* c, const float* xT, const float* zs, int nimg, int nprompts, const float* context, const float* cfg_scales_host,
                 const pnpi_ctrl_desc* ctrl_host, const float* etas_host, int nsteps_run, int nsteps_total, const int* ts, float* latents_out) {
  if (!c || !xT || !zs || !context || !cfg_scales_host || !etas_host || !ts || !latents_out || nimg <= 0) return PNPI_EINVAL;
  if (nprompts != 1 && nprompts != 2) return fail(c, PNPI_EINVAL, "nprompts must be 1 or 2");
  if (nsteps_run <= 0 || nsteps_run > nsteps_total) return fail(c, PNPI_EINVAL, "need 0 < nsteps_run <= nsteps_total");
  if (ctrl_host && nprompts != 2) return fail(c, PNPI_EINVAL, "an attention controller needs two prompts (source, target)");
  if (ctrl_host)
    for (int i = 0; i < nimg; ++i)
      if (ctrl_host[i].lb_enabled) return fail(c, PNPI_EINVAL, "LocalBlend is not supported by the edit-friendly edit");
  const int P = nprompts;
  Loop L(c);
  LoopLayout lay; lay.cds = ctrl_host; lay.nq = nimg;
  CKP(loop_begin(L, nsteps_total, 2 * P * nimg, "2 * nprompts * nimg exceeds max_unet_rows", lay));
  const size_t E = L.E;
  float* lat = misc_f(c, (size_t)nimg * P * E);
  int *d_expand, *d_inmap;
  loop_maps_cfg(L, nimg, nimg, P, &d_expand, &d_inmap);
  CKP(loop_commit(L));
  CK(launch_gather_rows_f32(xT, d_expand, nimg * P, E, lat, c->st));      // xT.expand(batch_size, ...) (:240)
  CKP(L.kv.begin(context, L.rows));
  for (int k = 0; k < nsteps_run; ++k) {
    const int t = ts[nsteps_total - nsteps_run + k], idx = nsteps_run - 1 - k;
    CKP(loop_unet(L, lat, d_inmap, t, context, ctrl_host != nullptr, k));
    const float eta = etas_host[idx];
    float sc[6]; CKP(ef_scalars(c, t, L.ratio, eta, sc));
    CK(launch_ef_reverse_step(L.eps, lat, zs + (size_t)idx * nimg * E, nimg, P, E, cfg_scales_host[0], cfg_scales_host[P - 1], sc,
                              eta > 0.f ? 1 : 0, lat, c->st));
  }
  CKH(hipMemcpyAsync(latents_out, lat, (size_t)nimg * P * E * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  return 0;
}

// ---------------------------------------------------------------------------------------------------- Blended Latent Diffusion
// run_editing_blended_latent_diffusion.py, BlendedLatnetDiffusion (one prompt, one user mask; the background is re-anchored to the noised
// source after every step).  _read_mask (:164-173) at the context's latent size.
int pnpi_bld_mask(pnpi_ctx* c, const uint8_t* mask_u8, int n, int H, int W, float* mask_out) {
  if (!c || !mask_u8 || !mask_out || n <= 0 || H <= 0 || W <= 0) return PNPI_EINVAL;
  const int S = c->cfg.sample_size;
  CK(launch_bld_mask(mask_u8, n, H, W, S, S, mask_out, c->st));
  return 0;
}
// one step of the loop of edit_image (:127-139): scheduler.step at t (prev_t = t - step_ratio, final_alpha_cumprod below 0), add_noise at t
int pnpi_bld_step(pnpi_ctx* c, const float* eps, const float* x, const float* src, const float* noise, const float* mask, int nimg,
                  size_t row_elems, size_t map_elems, float guidance_scale, int t, int step_ratio, float* x_out) {
  if (!c || !eps || !x || !src || !noise || !mask || !x_out || nimg <= 0 || row_elems == 0 || map_elems == 0) return PNPI_EINVAL;
  if (row_elems % map_elems) return fail(c, PNPI_EINVAL, "row_elems must be a multiple of map_elems (the mask is broadcast over the channels)");
  if (step_ratio <= 0) return fail(c, PNPI_EINVAL, "step_ratio must be positive");
  float af, at; CKP(alphas_for(c, t, step_ratio, false, &af, &at));
  CK(launch_bld_step(eps, x, src, noise, mask, nimg, row_elems, map_elems, guidance_scale, af, at, x_out, c->st));
  return 0;
}
/* BlendedLatnetDiffusion.edit_image's loop (:110-139) for nimg images, device-resident: the last nsteps_run of the nsteps_total timesteps
 * (`timesteps[int(n * blending_percentage):]`, :110-112).  The start latent is the caller's N(0,1) draw (:102-106), NOT the noised source.
 * One UNet launch of the rows [img][uncond, cond] per step (the reference's torch.cat([latents] * 2), :114), then one bld_step launch;
 * step k blends with the caller's draw noise[k] (the torch.randn_like of :137). */
int pnpi_bld_edit(pnpi_ctx* c, const float* x_start, int nimg, const float* src, const float* noise, const float* mask, const float* ctx_uncond,
                  const float* ctx_cond, float guidance_scale, int nsteps_total, int nsteps_run, const int* ts, float* latents_out) {
  if (!c || !x_start || !src || !noise || !mask || !ctx_uncond || !ctx_cond || !ts || !latents_out || nimg <= 0 || nsteps_total <= 0) return PNPI_EINVAL;
  if (nsteps_run < 1 || nsteps_run > nsteps_total) return fail(c, PNPI_EINVAL, "need 1 <= nsteps_run <= nsteps_total");
  Loop L(c);
  CKP(loop_begin(L, nsteps_total, 2 * nimg, "2 * nimg exceeds max_unet_rows (blended latent diffusion runs [uncond, cond] per image)"));
  const size_t E = L.E, N = (size_t)nimg * E, HW = (size_t)c->cfg.sample_size * c->cfg.sample_size;
  float* lat = misc_f(c, N);
  float* ctx2 = misc_f(c, (size_t)L.rows * L.CE);
  std::vector<int> inmap(L.rows);
  for (int r = 0; r < L.rows; ++r) inmap[r] = r / 2;
  int* d_inmap;
  loop_map(L, inmap, &d_inmap);
  CKP(loop_commit(L));
  CKP(interleave_ctx(c, ctx2, ctx_uncond, ctx_cond, nimg, L.CE));
  CKH(hipMemcpyAsync(lat, x_start, N * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  CKP(L.kv.begin(ctx2, L.rows));
  for (int k = 0; k < nsteps_run; ++k) {
    const int t = ts[nsteps_total - nsteps_run + k];
    CKP(loop_unet(L, lat, d_inmap, t, ctx2, false, 0));
    float af, at; CKP(alphas_for(c, t, L.ratio, false, &af, &at));
    CK(launch_bld_step(L.eps, lat, src, noise + (size_t)k * N, mask, nimg, E, HW, guidance_scale, af, at, lat, c->st));
  }
  CKH(hipMemcpyAsync(latents_out, lat, N * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  return 0;
}

// ---------------------------------------------------------------------------------------------------- Plug-and-Play
// run_editing_pnp.py: PNP.denoise_step / sample_loop with register_conv_control_efficient and register_attention_control_efficient.
// Rows [img][source latent of this level, x, x] on the contexts ["", negative prompt, target prompt]; the source row is read from the
// caller's list every step and never stepped.
size_t pnpi_pnp_desc_sizeof(void) { return sizeof(pnpi_pnp_desc); }
static int pnp_transformer_count(const pnpi_model_config& g) {
  int n = 1;
  for (int i = 0; i < g.n_blocks; ++i) if (g.block_has_attn[i]) n += g.layers_per_block + (g.layers_per_block + 1);
  return n;
}
int pnpi_pnp_desc_default(const pnpi_model_config* g, int nsteps, pnpi_pnp_desc* out) {
  if (!g || !out || nsteps <= 0 || g->n_blocks <= 0 || g->n_blocks > 4 || g->layers_per_block < 1) return PNPI_EINVAL;
  const int n = g->n_blocks, lpb = g->layers_per_block;
  int first = -1;      // the first decoder level with attention (up_blocks[1] at SD-1.x)
  for (int i = 0; i < n && first < 0; ++i) if (g->block_has_attn[n - 1 - i]) first = i;
  if (first < 0) return PNPI_ESHAPE;
  int tf = 1;          // transformer blocks in execution order: the encoder's, the middle one, then the decoder's
  for (int i = 0; i < n; ++i) if (g->block_has_attn[i]) tf += lpb;
  uint32_t mask = 0;
  for (int i = 0; i < n; ++i) {
    if (!g->block_has_attn[n - 1 - i]) continue;
    for (int j = 0; j <= lpb; ++j, ++tf)
      if (!(i == first && j == 0) && tf < 32) mask |= 1u << tf;
  }
  out->struct_size = (uint32_t)sizeof(pnpi_pnp_desc);
  out->conv_steps = (int)(nsteps * 0.8);      // int(n_timesteps * pnp_f_t), Python float arithmetic
  out->qk_steps = (int)(nsteps * 0.5);
  out->conv_site = first * (lpb + 1) + 1;
  out->qk_block_mask = mask;
  return 0;
}
static int pnp_check(pnpi_ctx* c, const pnpi_pnp_desc* d, int nimg) {
  if (d->struct_size != (uint32_t)sizeof(pnpi_pnp_desc)) return fail(c, PNPI_EINVAL, "pnpi_pnp_desc.struct_size is not sizeof(pnpi_pnp_desc) of this library");
  const pnpi_model_config& g = c->cfg;
  if (nimg > c->max_rows / 3) return fail(c, PNPI_EINVAL, "3 * nimg exceeds max_unet_rows (Plug-and-Play runs [source, negative, target] per image)");
  if (d->conv_site < -1 || d->conv_site >= g.n_blocks * (g.layers_per_block + 1)) return fail(c, PNPI_EINVAL, "pnpi_pnp_desc.conv_site is no decoder ResNet of this model");
  const int ntf = pnp_transformer_count(g);
  if (ntf < 32 && (d->qk_block_mask >> ntf)) return fail(c, PNPI_EINVAL, "pnpi_pnp_desc.qk_block_mask names a transformer block this model does not have");
  if (d->conv_steps < 0 || d->qk_steps < 0) return fail(c, PNPI_EINVAL, "pnpi_pnp_desc: negative step count");
  return 0;
}
// rows [3 nimg][4] = {r, source row of r's image, the same, r};  src_rows [nimg];  hrow [3 nimg]
static void pnp_maps(int nimg, std::vector<int>& rows, std::vector<int>& src_rows, std::vector<int>& hrow) {
  rows.resize((size_t)nimg * 12); src_rows.resize(nimg); hrow.resize((size_t)nimg * 3);
  for (int i = 0; i < nimg; ++i) {
    src_rows[i] = 3 * i;
    for (int k = 0; k < 3; ++k) {
      const int r = 3 * i + k;
      rows[4 * r] = r; rows[4 * r + 1] = 3 * i; rows[4 * r + 2] = 3 * i; rows[4 * r + 3] = r;
      hrow[r] = i;
    }
  }
}
// the injection parameters of one forward; s: the device tables of pnp_maps (rows, src_rows, hrow)
static PnpState pnp_arm(const pnpi_pnp_desc* d, int nimg, bool conv, bool qk, PnpState s) {
  s.on = true; s.nimg = nimg; s.conv_site = d->conv_site; s.qk_mask = d->qk_block_mask;
  s.conv = conv && d->conv_site >= 0; s.qk = qk && d->qk_block_mask != 0;
  return s;
}

int pnpi_pnp_step(pnpi_ctx* c, const float* eps, const float* x, int nimg, size_t row_elems, float guidance_scale, int t, int step_ratio,
                  float* x_out) {
  if (!c || !eps || !x || !x_out || nimg <= 0 || row_elems == 0) return PNPI_EINVAL;
  if (step_ratio <= 0) return fail(c, PNPI_EINVAL, "step_ratio must be positive");
  float af, at; CKP(alphas_for(c, t, step_ratio, false, &af, &at));
  CK(launch_pnp_step(eps, x, nullptr, nimg, row_elems, guidance_scale, af, at, x_out, nullptr, c->st));
  return 0;
}

int pnpi_unet_forward_pnp(pnpi_ctx* c, const float* latents, int nimg, int t, const float* context, const pnpi_pnp_desc* desc, int conv_on,
                          int qk_on, float* eps_out) {
  if (!c || !latents || !eps_out || !desc || nimg <= 0) return PNPI_EINVAL;
  CKP(check_ready(c));
  CKP(pnp_check(c, desc, nimg));
  const int rows = 3 * nimg;
  if (c->attn_cb) return fail(c, PNPI_ESTATE, "an attention callback is installed: the Plug-and-Play forward takes its descriptor only");
  UNetCall k; CKP(level1_call(c, latents, rows, context, eps_out, k));
  CKP(setup_ctrl(c, nullptr, 0, c->max_rows));
  std::vector<int> rt, sr, hr;
  pnp_maps(nimg, rt, sr, hr);
  int* d = (int*)c->ctrl_arena.alloc((rt.size() + sr.size() + hr.size()) * sizeof(int));
  if (c->ctrl_arena.overflow) return fail(c, PNPI_ENOMEM, "controller arena overflow");
  std::vector<int> all(rt);
  all.insert(all.end(), sr.begin(), sr.end()); all.insert(all.end(), hr.begin(), hr.end());
  CKP(upload(c, d, all.data(), all.size() * sizeof(int)));
  PnpState tables; tables.rows = d; tables.src_rows = d + rt.size(); tables.hrow = d + rt.size() + sr.size();
  const PnpState pnp = pnp_arm(desc, nimg, conv_on != 0, qk_on != 0, tables);
  k.t = t; k.pnp = &pnp;
  return unet_fwd(c, k);
}

int pnpi_pnp_edit(pnpi_ctx* c, const float* src_latents, const float* x_start, int nimg, const float* context, const pnpi_pnp_desc* desc,
                  int nsteps, const int* ts, float gs, float* latents_out) {
  if (!c || !src_latents || !x_start || !context || !desc || !ts || !latents_out || nimg <= 0) return PNPI_EINVAL;
  if (nsteps <= 0 || nsteps > c->cfg.n_train_timesteps) return fail(c, PNPI_EINVAL, "need 1 <= nsteps <= n_train_timesteps");
  CKP(pnp_check(c, desc, nimg));
  for (int i = 0; i < nsteps; ++i)
    if (ts[i] < 0 || ts[i] >= c->cfg.n_train_timesteps) return fail(c, PNPI_EINVAL, "timestep out of range");
  if (!c->sched_set) return fail(c, PNPI_ESTATE, "pnpi_set_scheduler not called");
  Loop L(c);
  CKP(loop_begin(L, nsteps, 3 * nimg, "3 * nimg exceeds max_unet_rows (Plug-and-Play runs [source, negative, target] per image)"));
  const size_t E = L.E, N = (size_t)nimg * E;
  float* x = misc_f(c, N);
  float* rows3 = misc_f(c, 3 * N);
  L.eps = misc_f(c, 3 * N);
  std::vector<int> rt, sr, hr;
  pnp_maps(nimg, rt, sr, hr);
  loop_map(L, rt, &L.pnp.rows); loop_map(L, sr, &L.pnp.src_rows); loop_map(L, hr, &L.pnp.hrow);
  CKP(loop_commit(L, false));      // the rows of a launch are written in place by pnp_step: no gathered input buffer
  const size_t w = E * sizeof(float);
  CKH(hipMemcpyAsync(x, x_start, N * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  CKH(hipMemcpy2DAsync(rows3, 3 * w, src_latents, w, w, nimg, hipMemcpyDeviceToDevice, c->st));
  CKH(hipMemcpy2DAsync(rows3 + E, 3 * w, x_start, w, w, nimg, hipMemcpyDeviceToDevice, c->st));
  CKH(hipMemcpy2DAsync(rows3 + 2 * E, 3 * w, x_start, w, w, nimg, hipMemcpyDeviceToDevice, c->st));
  CKP(L.kv.begin(context, L.rows));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[i];
    L.pnp = pnp_arm(desc, nimg, i < desc->conv_steps, i < desc->qk_steps, L.pnp);
    CKP(loop_unet(L, rows3, nullptr, t, context, false, i));
    float af, at; CKP(alphas_for(c, t, L.ratio, false, &af, &at));
    // CFG over rows 1 and 2, the DDIM step, and the next launch's rows [source latent of the next level, x, x]
    CK(launch_pnp_step(L.eps, x, i + 1 < nsteps ? src_latents + (size_t)(i + 1) * N : nullptr, nimg, E, gs, af, at, x, rows3, c->st));
  }
  CKH(hipMemcpyAsync(latents_out, x, N * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  return 0;
}

// ---------------------------------------------------------------------------------------------------- InstructPix2Pix
// run_editing_instructpix2pix.py: CFGDenoiser (:33-46) around k-diffusion's CompVisDenoiser, sampled by sample_euler_ancestral.  The UNet
// takes 8 channels [z * c_in | image latent] and a FRACTIONAL timestep (sigma_to_t); rows [img][edit text + image, null text + image,
// null text + zero image].  The per-step scalars are the caller's: 6 floats per step [sigma, sigma_down - sigma, sigma_up, c_in, t,
// sigma_next > 0], evaluated on the host in the reference's fp32 order (pnpinversion_amd/instructpix2pix.py: step_table).
// The sinusoid row at a float timestep, cos half first.  A fractional t as the reference evaluates it (ldm's timestep_embedding: fp32 freqs =
// exp(-log(10000) * i / half), fp32 t * freqs, fp32 cos / sin); an integer t as the context's table is built (fp64, rounded once), so that it
// reproduces pnpi_unet_forward bit for bit.
static void temb_row_host(const pnpi_model_config& g, float t, float* row) {
  const int C0 = g.block_out_channels[0], half = C0 / 2;
  const bool whole = t == floorf(t);
  const float nl = (float)(-log(10000.0));
  for (int i = 0; i < half; ++i) {
    if (whole) {
      double e = exp(-log(10000.0) * (double)i / (double)half);
      double a = (double)t * e;
      row[i] = (float)cos(a);
      row[half + i] = (float)sin(a);
    } else {
      const float f = expf(nl * (float)i / (float)half);
      const float a = t * f;
      row[i] = cosf(a);
      row[half + i] = sinf(a);
    }
  }
}
// The two instruction editors share everything but the third row's text and the combine (step.hip: ip2p_move)
struct Ip2pKind {
  int combine;
  const char* name;          // in refusals
  const char* rows_msg;      // the row-limit refusal names the kind's own row layout
};
static const Ip2pKind kIp2p = {IP2P_CHAIN, "InstructPix2Pix",
                               "3 * nimg exceeds max_unet_rows (InstructPix2Pix runs [edit + image, null + image, null + no image] per image)"};
static const Ip2pKind kInstDiff = {IP2P_SYMMETRIC, "InstructDiffusion",
                                   "3 * nimg exceeds max_unet_rows (InstructDiffusion runs [edit + image, null + image, edit + no image] per image)"};
static int ip2p_fail(pnpi_ctx* c, const Ip2pKind& k, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s %s", k.name, what);
  return fail(c, PNPI_EINVAL, msg);
}
static int ip2p_model_check(pnpi_ctx* c, const Ip2pKind& k) {
  if (c->cfg.in_channels != 8 || c->cfg.out_channels != 4)
    return ip2p_fail(c, k, "needs a model with in_channels == 8 and out_channels == 4 (4 latent + 4 image-latent channels in, 4 out)");
  return 0;
}
static int ip2p_scalars_check(pnpi_ctx* c, const Ip2pKind& k, const float* sc, int n) {
  for (int i = 0; i < n; ++i) {
    const float* s = sc + 6 * (size_t)i;
    if (!(s[0] > 0.f) || !(s[3] > 0.f)) return ip2p_fail(c, k, "step scalars: sigma and c_in must be positive");
    if (!(s[4] >= 0.f) || !(s[4] <= (float)(c->cfg.n_train_timesteps - 1))) return fail(c, PNPI_EINVAL, "timestep out of range");
  }
  return 0;
}
// pnpi_unet_forward at a float timestep (no controller): the sinusoid row is evaluated here, the per-timestep bias cache is not touched
int pnpi_unet_forward_t(pnpi_ctx* c, const float* latents, int rows, float t, const float* context, float* eps_out) {
  if (!c || !latents || !eps_out) return PNPI_EINVAL;
  CKP(check_ready(c));
  if (c->attn_cb) return fail(c, PNPI_ESTATE, "an attention callback is installed: pnpi_unet_forward_t runs no controller");
  if (!(t >= 0.f) || !(t <= (float)(c->cfg.n_train_timesteps - 1))) return fail(c, PNPI_EINVAL, "timestep out of range");
  if (rows <= 0 || rows > c->max_rows) return fail(c, PNPI_EINVAL, "unet rows out of range (max_unet_rows)");
  UNetCall k; CKP(level1_call(c, latents, rows, context, eps_out, k));
  if (c->cd.any_edit || c->cd.nimg != 0) CKP(setup_ctrl(c, nullptr, 0, c->max_rows));
  std::vector<float> row(c->cfg.block_out_channels[0]);
  temb_row_host(c->cfg, t, row.data());
  CKP(upload(c, c->temb_row, row.data(), row.size() * sizeof(float)));
  k.temb_row = c->temb_row;
  return unet_fwd(c, k);
}
// one step (level 1): eps [nimg][3][row_elems], z / noise / image / z_out [nimg][row_elems], sc6_host the step's scalars (c_in and t unread),
// in_next (nullable) [nimg][2][2 * row_elems] scaled by c_in_next.  noise is not read when sc6_host[5] == 0 (sigma_next == 0).
static int ip2p_step_impl(pnpi_ctx* c, const Ip2pKind& k, const float* eps, const float* z, const float* noise, const float* image, int nimg,
                          size_t row_elems, float cfg_text, float cfg_image, const float* sc6_host, float c_in_next, float* z_out, float* in_next) {
  if (!c || !eps || !z || !sc6_host || !z_out || nimg <= 0 || row_elems == 0) return PNPI_EINVAL;
  if (!(sc6_host[0] > 0.f)) return ip2p_fail(c, k, "step scalars: sigma and c_in must be positive");
  const int add_noise = sc6_host[5] != 0.f;
  if (add_noise && !noise) return fail(c, PNPI_EINVAL, "sigma_next > 0: the step needs its draw");
  if (in_next && !image) return fail(c, PNPI_EINVAL, "in_next needs the image latent");
  CK(launch_ip2p_step(k.combine, eps, z, noise, image, nimg, row_elems, cfg_text, cfg_image, sc6_host, add_noise, c_in_next, z_out, in_next, c->st));
  return 0;
}
int pnpi_ip2p_step(pnpi_ctx* c, const float* eps, const float* z, const float* noise, const float* image, int nimg, size_t row_elems,
                   float cfg_text, float cfg_image, const float* sc6_host, float c_in_next, float* z_out, float* in_next) {
  return ip2p_step_impl(c, kIp2p, eps, z, noise, image, nimg, row_elems, cfg_text, cfg_image, sc6_host, c_in_next, z_out, in_next);
}
int pnpi_instdiff_step(pnpi_ctx* c, const float* eps, const float* z, const float* noise, const float* image, int nimg, size_t row_elems,
                       float cfg_text, float cfg_image, const float* sc6_host, float c_in_next, float* z_out, float* in_next) {
  return ip2p_step_impl(c, kInstDiff, eps, z, noise, image, nimg, row_elems, cfg_text, cfg_image, sc6_host, c_in_next, z_out, in_next);
}
/* edit_instruct_pix2pix's sampler (:125-134) and instruct_diffusion_edit's (run_editing_instructdiffusion.py:110-120) for nimg images,
 * device-resident.  z0 [nimg][4 S^2] = randn * sigmas[0], image [nimg][4 S^2] the encoder's posterior mean (not scaled), noise
 * [nsteps][nimg][4 S^2] the draws in step order (the last is not read when its sigma_next is 0), context [nimg][3][77][D] = [edit, null, null]
 * (InstructPix2Pix) or [edit, null, edit] (InstructDiffusion): the caller's rows, the loop reads them as given.  Per step one UNet launch of
 * 3 * nimg rows on 2 * nimg distinct inputs (rows 0 and 1 share theirs: the input map "cfg_dedup" compacts; the map is the same for both kinds,
 * the third row's zero image half is what both pair with their third text) and one ip2p_step launch with the kind's combine.  trajectory_out
 * (nullable) [nsteps][nimg][4 S^2]: z after every step. */
static int ip2p_edit_impl(pnpi_ctx* c, const Ip2pKind& k, const float* z0, const float* image, const float* noise, int nimg, const float* context,
                          float cfg_text, float cfg_image, int nsteps, const float* scalars_host, float* z_out, float* trajectory_out) {
  if (!c) return PNPI_EINVAL;
  if (nsteps <= 0 || nsteps > c->cfg.n_train_timesteps) return fail(c, PNPI_EINVAL, "need 1 <= nsteps <= n_train_timesteps");
  if (!z0 || !image || !noise || !context || !scalars_host || !z_out || nimg <= 0) return PNPI_EINVAL;
  CKP(ip2p_model_check(c, k));
  CKP(ip2p_scalars_check(c, k, scalars_host, nsteps));
  Loop L(c);
  LoopLayout lay; lay.split_io = true;
  CKP(loop_begin(L, nsteps, 3 * nimg, k.rows_msg, lay));
  const size_t E4 = L.E_out, N = (size_t)nimg * E4;
  const int C0 = c->cfg.block_out_channels[0];
  float* z = misc_f(c, N);
  float* in2 = misc_f(c, 2 * (size_t)nimg * L.E);      // [img][with image, without] 8-channel inputs
  float* trows = misc_f(c, (size_t)nsteps * C0);
  L.bias_row = misc_f(c, (size_t)c->unet.temb_total);
  std::vector<int> inmap((size_t)L.rows);
  for (int r = 0; r < L.rows; ++r) inmap[r] = 2 * (r / 3) + (r % 3 == 2);
  int* d_inmap;
  loop_map(L, inmap, &d_inmap);
  CKP(loop_commit(L));
  std::vector<float> rows_h((size_t)nsteps * C0);
  for (int i = 0; i < nsteps; ++i) temb_row_host(c->cfg, scalars_host[6 * (size_t)i + 4], rows_h.data() + (size_t)i * C0);
  CKP(upload(c, trows, rows_h.data(), rows_h.size() * sizeof(float)));
  L.temb_rows = trows;
  CK(launch_ip2p_step(k.combine, nullptr, z0, nullptr, image, nimg, E4, cfg_text, cfg_image, nullptr, 0, scalars_host[3], z, in2, c->st));
  CKP(L.kv.begin(context, L.rows));
  for (int i = 0; i < nsteps; ++i) {
    const float* sc = scalars_host + 6 * (size_t)i;
    CKP(loop_unet(L, in2, d_inmap, 0, context, false, i));
    const bool last = i + 1 == nsteps;
    CK(launch_ip2p_step(k.combine, L.eps, z, noise + (size_t)i * N, image, nimg, E4, cfg_text, cfg_image, sc, sc[5] != 0.f,
                        last ? 0.f : sc[6 + 3], z, last ? nullptr : in2, c->st));
    if (trajectory_out) CKH(hipMemcpyAsync(trajectory_out + (size_t)i * N, z, N * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  }
  CKH(hipMemcpyAsync(z_out, z, N * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  return 0;
}
int pnpi_ip2p_edit(pnpi_ctx* c, const float* z0, const float* image, const float* noise, int nimg, const float* context, float cfg_text,
                   float cfg_image, int nsteps, const float* scalars_host, float* z_out, float* trajectory_out) {
  return ip2p_edit_impl(c, kIp2p, z0, image, noise, nimg, context, cfg_text, cfg_image, nsteps, scalars_host, z_out, trajectory_out);
}
int pnpi_instdiff_edit(pnpi_ctx* c, const float* z0, const float* image, const float* noise, int nimg, const float* context, float cfg_text,
                       float cfg_image, int nsteps, const float* scalars_host, float* z_out, float* trajectory_out) {
  return ip2p_edit_impl(c, kInstDiff, z0, image, noise, nimg, context, cfg_text, cfg_image, nsteps, scalars_host, z_out, trajectory_out);
}

// ---------------------------------------------------------------------------------------------------- null-text optimisation
// differentiable UNet forward: one recorded row, reverse walk in api_backward.inc
static int tape_ensure(pnpi_ctx* c) {
  if (c->tape) return 0;
  const pnpi_model_config& g = c->cfg;
  // The activation arenas were sized at create for max_unet_rows rows of the plain forward (block temporaries released in stack order).
  // A recording forward of ONE row keeps every temporary: measure it with a dry run and grow the arenas if that is more (set-up time
  // only -- nothing is allocated in the optimisation loop).  New buffers are allocated BEFORE the old ones are freed and the context's
  // state changes only after every allocation has succeeded: a failed hipMalloc leaves the context as it was (and without a tape).
  std::unique_ptr<Tape> T(new Tape());
  CKH(hipStreamSynchronize(c->st));
  size_t pp, tp;
  {
    const Bump sp = c->persist, stmp = c->temp;
    c->persist = Bump(); c->temp = Bump();
    c->tape = T.get();
    UNetCall k; k.rows = 1; k.record = true;
    const int r = [&]() { DryScope dry(c); return unet_fwd(c, k); }();
    pp = align_up(c->persist.peak + (1 << 20), 4096); tp = align_up(c->temp.peak + (1 << 20), 4096);
    c->persist = sp; c->temp = stmp; c->tape = nullptr;
    if (r) return r;
  }
  // gradients + dgrad scratch of one UNet row: about 2.8x the recorded activations at SD-1.x width (1.1 of 0.4 GB); 6x with a 64 MB floor
  const size_t gcap = align_up(std::max((size_t)64 << 20, 6 * (pp + tp)), 4096);
  char *gbase = nullptr, *nper = nullptr, *ntmp = nullptr;
  float* dctx = nullptr;
  auto undo = [&]() { if (gbase) (void)hipFree(gbase); if (nper) (void)hipFree(nper); if (ntmp) (void)hipFree(ntmp); if (dctx) (void)hipFree(dctx); };
  hipError_t e = hipMalloc((void**)&gbase, gcap);
  if (e == hipSuccess) e = hipMalloc((void**)&dctx, (size_t)g.ctx_len * g.cross_dim * sizeof(float));
  if (e == hipSuccess && pp > c->persist.cap) e = hipMalloc((void**)&nper, pp);
  if (e == hipSuccess && tp > c->temp.cap) e = hipMalloc((void**)&ntmp, tp);
  if (e != hipSuccess) { undo(); const std::string msg = std::string("null-text tape: ") + hipGetErrorString(e); return fail(c, PNPI_EHIP, msg.c_str()); }
  if (nper) { (void)hipFree(c->persist.base); c->persist.base = nper; c->persist.cap = pp; }
  if (ntmp) { (void)hipFree(c->temp.base); c->temp.base = ntmp; c->temp.cap = tp; }
  c->persist.reset(); c->temp.reset(); c->persist.overflow = false; c->temp.overflow = false;
  T->garena.base = gbase; T->garena.cap = gcap; T->d_ctx = dctx;
  c->tape = T.release();
  return 0;
}
// one row with its own context, no controller; record: onto the context's tape, cleared first (tape_backward walks it afterwards)
static int unet_fwd_one(pnpi_ctx* c, const float* lat, int t, const float* context, float* eps_out, bool record) {
  UNetCall k; k.latents = lat; k.rows = 1; k.t = t; k.context = context; k.eps_out = eps_out; k.record = record;
  if (record) { Tape& T = *c->tape; T.ops.clear(); T.grads.clear(); T.garena.reset(); T.garena.overflow = false; }
  return unet_fwd(c, k);
}
// eps = UNet(latents, t, context) for ONE row, and d_context = (d loss / d eps)^T (d eps / d context) for the given d loss / d eps
// (fp32, the layout of eps; pre-multiplied by the caller's power-of-two loss scale -- activations' gradients travel in fp16).
int pnpi_unet_context_grad(pnpi_ctx* c, const float* latents, int t, const float* context, const float* d_eps, float* eps_out, float* d_context_out) {
  if (!c || !latents || !context || !d_eps || !d_context_out) return PNPI_EINVAL;
  CKP(check_loop_ready(c));
  CKP(tape_ensure(c));
  Tape& T = *c->tape;
  const pnpi_model_config& g = c->cfg;
  const size_t E = (size_t)g.in_channels * g.sample_size * g.sample_size, CE = (size_t)g.ctx_len * g.cross_dim;
  CKP(setup_ctrl(c, nullptr, 0, c->max_rows));
  float* eps = eps_out ? eps_out : misc_f(c, E);
  CKP(unet_fwd_one(c, latents, t, context, eps, true));
  half_t* d_out = tape_galloc(c, (size_t)g.sample_size * g.sample_size * 8);
  if (!d_out) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
  CK(launch_nchw_f32_to_nhwc_f16(d_eps, 1, g.in_channels, g.sample_size * g.sample_size, 8, d_out, c->st));
  CKH(hipMemsetAsync(T.d_ctx, 0, CE * sizeof(float), c->st));
  CKP(tape_backward(c, d_out));
  CKH(hipMemcpyAsync(d_context_out, T.d_ctx, CE * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  return 0;
}

// The Adam loop both optimisations share (inversion.py:203-218 and :430-447): eps_c = UNet(lat, t, ctx_cond) once, then up to
// num_inner_steps x {recording forward with the current embedding `unc`, loss = mse(prev_step(CFG), target) and its gradient, reverse
// walk to the embedding, Adam (torch.optim.Adam defaults, state fresh per DDIM step)}; the loss is read back for the reference's
// early-stop test `loss < epsilon + i * 2e-5`.  eps2 = [eps_u | eps_c] (2E floats).  losses_host (nullable): [num_inner_steps].
struct NullOptBufs { float *eps2, *d_eps, *am, *av, *loss_d; };
static int null_inner_loop(pnpi_ctx* c, const NullOptBufs& b, const float* lat, int t, int i, float* unc, const float* ctx_cond,
                           const float* target, float guidance_scale, float a_t, float a_p, int num_inner_steps, float epsilon,
                           int* its_out, float* losses_host) {
  const pnpi_model_config& g = c->cfg;
  const size_t E = (size_t)g.in_channels * g.sample_size * g.sample_size, CE = (size_t)g.ctx_len * g.cross_dim;
  const float scale = 4096.f;                                   // loss scale of the fp16 activation gradients (removed before Adam)
  const double sa_t = sqrt((double)a_t), sb_t = sqrt(1.0 - a_t), sa_p = sqrt((double)a_p), sb_p = sqrt(1.0 - a_p);
  const float c_x = (float)(sa_p / sa_t), c_e = (float)(sb_p - sa_p * sb_t / sa_t);       // rec = c_x x + c_e eps
  const float lr = (float)(1e-2 * (1.0 - i / 100.0));
  int its = 0;
  CKP(unet_fwd_one(c, lat, t, ctx_cond, b.eps2 + E, false));
  CKH(hipMemsetAsync(b.am, 0, CE * sizeof(float), c->st));
  CKH(hipMemsetAsync(b.av, 0, CE * sizeof(float), c->st));
  for (int j = 0; j < num_inner_steps; ++j) {
    // forward with the tape recording; the loss head needs eps_u first, so forward and backward are two calls of the tape machinery
    Tape& T = *c->tape;
    CKP(unet_fwd_one(c, lat, t, unc, b.eps2, true));
    CK(launch_null_text_loss(b.eps2, b.eps2 + E, lat, target, (int)E, guidance_scale, c_x, c_e, scale, b.d_eps, b.loss_d, c->st));
    half_t* d_out = tape_galloc(c, (size_t)g.sample_size * g.sample_size * 8);
    if (!d_out) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
    CK(launch_nchw_f32_to_nhwc_f16(b.d_eps, 1, g.in_channels, g.sample_size * g.sample_size, 8, d_out, c->st));
    CKH(hipMemsetAsync(T.d_ctx, 0, CE * sizeof(float), c->st));
    CKP(tape_backward(c, d_out));
    CK(launch_adam_step(unc, b.am, b.av, T.d_ctx, (int)CE, j + 1, lr, 1.f / scale, c->st));
    float loss_h = 0.f;
    CKH(hipMemcpyAsync(&loss_h, b.loss_d, sizeof(float), hipMemcpyDeviceToHost, c->st));
    CKH(hipStreamSynchronize(c->st));
    if (losses_host) losses_host[j] = loss_h;
    its = j + 1;
    c->ctr.unet_backward_rows += 1;
    if (loss_h < epsilon + i * 2e-5f) break;
  }
  *its_out = its;
  return 0;
}
static NullOptBufs null_bufs(const Loop& L) {
  pnpi_ctx* c = L.c;
  return {misc_f(c, 2 * L.E), misc_f(c, L.E), misc_f(c, L.CE), misc_f(c, L.CE), misc_f(c, 1)};
}

// NullInversion.null_optimization (models/p2p/inversion.py:196-225) for one image, device resident.  ddim_latents [nsteps + 1][E] (the
// inversion trajectory, x*_0 first), ctx_uncond / ctx_cond [77][768]; uncond_out [nsteps][77][768] receives the optimised embedding of
// every step; then the CFG step with the optimised embedding moves the latent on.  losses_out (nullable, host): [nsteps][num_inner_steps]
// loss of every Adam iteration (-1 for iterations the early stop skipped).
int pnpi_null_text_optimize(pnpi_ctx* c, const float* ddim_latents, const float* ctx_uncond, const float* ctx_cond, int nsteps,
                            const int* ts, float guidance_scale, int num_inner_steps, float epsilon, float* uncond_out, int* iters_out,
                            float* losses_out) {
  if (!c || !ddim_latents || !ctx_uncond || !ctx_cond || !ts || !uncond_out || nsteps <= 0 || num_inner_steps < 0) return PNPI_EINVAL;
  Loop L(c);
  CKP(loop_begin(L, nsteps, 1, "null-text inversion needs max_unet_rows >= 1"));
  CKP(tape_ensure(c));
  const size_t E = L.E, CE = L.CE;
  const NullOptBufs b = null_bufs(L);
  float* lat = misc_f(c, E);
  float* unc = misc_f(c, CE);
  CKP(loop_commit(L, false));
  if (losses_out) for (int k = 0; k < nsteps * num_inner_steps; ++k) losses_out[k] = -1.f;
  CKH(hipMemcpyAsync(unc, ctx_uncond, CE * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  CKH(hipMemcpyAsync(lat, ddim_latents + (size_t)nsteps * E, E * sizeof(float), hipMemcpyDeviceToDevice, c->st));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[i];
    float a_t, a_p; CKP(alphas_for(c, t, L.ratio, false, &a_t, &a_p));
    const float* target = ddim_latents + (size_t)(nsteps - i - 1) * E;
    int its = 0;
    if (num_inner_steps > 0)
      CKP(null_inner_loop(c, b, lat, t, i, unc, ctx_cond, target, guidance_scale, a_t, a_p, num_inner_steps, epsilon, &its,
                          losses_out ? losses_out + (size_t)i * num_inner_steps : nullptr));
    if (iters_out) iters_out[i] = its;
    CKH(hipMemcpyAsync(uncond_out + (size_t)i * CE, unc, CE * sizeof(float), hipMemcpyDeviceToDevice, c->st));
    // latent_cur = prev_step(CFG(eps(unc), eps(cond)))   (get_noise_pred with the optimised embedding, inversion.py:221-224)
    CKP(unet_fwd_one(c, lat, t, unc, b.eps2, false));
    if (num_inner_steps == 0) CKP(unet_fwd_one(c, lat, t, ctx_cond, b.eps2 + E, false));
    CK(launch_cfg_ddim_prev(cfg_step(L, b.eps2, lat, 1, 1, guidance_scale, a_t, a_p, lat), c->st));
  }
  return 0;
}

// DirectInversion.null_latent_calculate (models/p2p/inversion.py:419-460, "ablation_null-latent-inversion+p2p") for one (source, target)
// prompt pair.  context4 rows = [unc_src, unc_tgt, cond_src, cond_tgt].  Per step: the unconditional embeddings are optimised as in
// null-text inversion -- the reference's loss reads the SOURCE row only (:441), so the target row's embedding has a zero gradient, Adam
// leaves it where it is, and only the source row needs the recording forward / reverse walk; its conditional prediction is constant over
// the iterations -- then the step's effect becomes a latent offset for both rows:
//   noise_loss[i] = prev_step(CFG with the optimised embeddings) - prev_step(CFG with the ORIGINAL ones),  latent_cur = plain + noise_loss[i]
// (:449-459).  The two 4-row forwards run with rows ordered [unc_src, cond_src, unc_tgt, cond_tgt] (row results do not depend on the
// order) so that the step kernel sees them as two one-row images.  noise_loss_out [nsteps][2][E].
int pnpi_null_latent_calculate(pnpi_ctx* c, const float* ddim_latents, const float* context4, int nsteps, const int* ts, float guidance_scale,
                               int num_inner_steps, float epsilon, float* noise_loss_out, int* iters_out, float* losses_out) {
  if (!c || !ddim_latents || !context4 || !ts || !noise_loss_out || nsteps <= 0 || num_inner_steps < 0) return PNPI_EINVAL;
  Loop L(c);
  CKP(loop_begin(L, nsteps, 4, "null-latent inversion needs max_unet_rows >= 4"));
  CKP(tape_ensure(c));
  const size_t E = L.E, CE = L.CE;
  const NullOptBufs b = null_bufs(L);
  float* cur = misc_f(c, 2 * E);          // latent_cur [src, tgt]
  float* in4 = misc_f(c, 4 * E);          // [src, src, tgt, tgt]
  float* eps4 = misc_f(c, 4 * E);
  float* opt = misc_f(c, 2 * E);
  float* unc = misc_f(c, 2 * CE);         // the embeddings being optimised [src, tgt] (warm-started from step to step)
  float* ctx4 = misc_f(c, 4 * CE);        // [unc_src, cond_src, unc_tgt, cond_tgt] of the forward at hand
  CKP(loop_commit(L, false));
  if (losses_out) for (int k = 0; k < nsteps * num_inner_steps; ++k) losses_out[k] = -1.f;
  const float* cond = context4 + 2 * CE;
  auto d2d = [&](float* d, const float* s, size_t n) { return hipMemcpyAsync(d, s, n * sizeof(float), hipMemcpyDeviceToDevice, c->st); };
  CKH(d2d(unc, context4, 2 * CE));
  CKH(d2d(cur, ddim_latents + (size_t)nsteps * E, E));
  CKH(d2d(cur + E, ddim_latents + (size_t)nsteps * E, E));
  CKH(d2d(ctx4 + CE, cond, CE));
  CKH(d2d(ctx4 + 3 * CE, cond + CE, CE));
  for (int i = 0; i < nsteps; ++i) {
    const int t = ts[i];
    float a_t, a_p; CKP(alphas_for(c, t, L.ratio, false, &a_t, &a_p));
    const float* target = ddim_latents + (size_t)(nsteps - i - 1) * E;
    int its = 0;
    if (num_inner_steps > 0)
      CKP(null_inner_loop(c, b, cur, t, i, unc, cond, target, guidance_scale, a_t, a_p, num_inner_steps, epsilon, &its,
                          losses_out ? losses_out + (size_t)i * num_inner_steps : nullptr));
    if (iters_out) iters_out[i] = its;
    CKH(d2d(in4, cur, E)); CKH(d2d(in4 + E, cur, E)); CKH(d2d(in4 + 2 * E, cur + E, E)); CKH(d2d(in4 + 3 * E, cur + E, E));
    UNetCall k4; k4.latents = in4; k4.rows = 4; k4.t = t; k4.context = ctx4; k4.eps_out = eps4;
    // with the optimised embeddings -> opt
    CKH(d2d(ctx4, unc, CE)); CKH(d2d(ctx4 + 2 * CE, unc + CE, CE));
    CKP(unet_fwd(c, k4));
    CK(launch_cfg_ddim_prev(cfg_step(L, eps4, cur, 2, 1, guidance_scale, a_t, a_p, opt), c->st));
    // with the original ones -> plain; loss = opt - plain; latent_cur = plain + loss
    CKH(d2d(ctx4, context4, CE)); CKH(d2d(ctx4 + 2 * CE, context4 + CE, CE));
    CKP(unet_fwd(c, k4));
    CfgStepP s = cfg_step(L, eps4, cur, 2, 1, guidance_scale, a_t, a_p, cur);
    s.target = opt; s.offset_out = noise_loss_out + (size_t)i * 2 * E;
    CK(launch_cfg_ddim_prev(s, c->st));
  }
  return 0;
}
