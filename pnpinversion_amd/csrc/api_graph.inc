// api_graph.inc -- part of api.hip (one translation unit: included there, in this order; not compiled on its own).
// per-launch profiling records, the activation tape, the op wrappers and the static UNet graph (ResNet / transformer blocks, unet_fwd)
// ---------------------------------------------------------------------------------------------------- profiling
static void prof_open(pnpi_ctx* c, ProfRec& r) {
  (void)hipEventCreate(&r.a); (void)hipEventCreate(&r.b);
  (void)hipEventRecord(r.a, c->st);
}
static void prof_close(pnpi_ctx* c, ProfRec& r, int cls, double flops, double bytes, int M = 0, int N = 0, int K = 0, int ks = 0) {
  (void)hipEventRecord(r.b, c->st);
  r.cls = cls; r.flops = flops; r.bytes = bytes; r.M = M; r.N = N; r.K = K; r.ksize = ks;
  c->prof.push_back(r);
}
// tuning "ff_fold" = 1: the transformer block's last two GEMMs (ff2, then the 1 x 1 proj_out) run as ONE launch over the folded weights
// [Wp W2 | Wp] (TransformerW::fo) -- nothing non-linear sits between them and hs3 has no other reader.  Same FLOPs, one launch, no
// hs3 round trip.  0: the two launches.  Results differ at fp16-rounding level only (hs3 is no longer rounded between the GEMMs;
// Wp W2 is rounded once at load).
// tuning "cfg_dedup": the rows of a classifier-free-guidance launch that share a latent (its unconditional and its conditional row) share
// everything the UNet computes before its first cross-attention.  1 / 2: that prefix runs once per distinct latent (unet_fwd, UNetDedup)
// and is expanded to the rows of the launch where the text comes in; 2 pins every prefix GEMM to the tile / split-K of its full-row
// form, which makes the forward bit-identical to 0 (per-element accumulation order does not depend on the tile's position).  0: off.
// Default 1: every prefix GEMM is planned on the rows it launches (igemm_plan at the launched M: the table's rows for the compact shapes,
// tile_table.inc); against 2 that moves fp32 summation order only (panel pixels by up to 2 / 255, profiles/rowfit_ab.json).
// PNPI_CFG_DEDUP: whole-benchmark A/B runs.
// the distinct latents of a launch: lat_u fp32 [U][C][S][S]; row r of the launch is latent hmap[r] (host) = dmap[r] (device)
struct UNetDedup { const float* lat_u; int U; const int* hmap; const int* dmap; };
// tuning "src_share": pnpi_direct_edit runs the source rows that its offset, reconstruction and edit passes repeat bit for bit once
// per step (a compact launch, expanded to the logical rows behind the UNet).  1: the compact launch chooses its own tiles; 2: every
// GEMM is configured as at the logical row count (sel_M, as "cfg_dedup" = 2 does for the prefix) -- bit-identical to 0; 0: off.
// Default 1: the source rows of the three passes are one launch row, so they see the same arithmetic whatever tile is chosen, and the
// 8-row launch takes the table's 8-row entries (text K/V projections included: they are planned at their launched M like every GEMM).
// A context that holds a tape keeps the full launch, configured as the compact one (pnpi_direct_edit), so it gives the same bits.
// U > 0: the launch of `from` rows serves `to` logical rows resting on U logical latents.  pin (= 2): every GEMM of the forward is
// configured as at `to` rows (the prefix of "cfg_dedup" as at to / U rows), so each launch makes the choices of the full-row loop
// (from > to: the full launch of a tape-holding context under "src_share" = 1, configured as the compact launch it replaces)
struct UNetShare { int from = 0, to = 0, U = 0; bool pin = false; };
// What a caller asks of ONE UNet forward (unet_fwd); nothing of it outlives the call.
struct UNetCall {
  const float* latents = nullptr;      // fp32 [rows][in_channels][S][S]
  int rows = 0, t = 0, cur_step = 0;
  const float* context = nullptr;      // fp32 [rows][ctx_len][cross_dim]; not read with cached_kv
  bool use_ctrl = false;               // the controller tables of setup_ctrl act, at step cur_step
  float* eps_out = nullptr;            // fp32 [rows][out_channels][S][S]
  const UNetDedup* dedup = nullptr;    // the distinct latents behind the rows (the CFG loops); NULL = every row on its own
  // temb_row (device [C0]): the sinusoid row of this forward, given by the caller (a fractional timestep); t is then not read, the three
  // GEMVs run into bias_row (device [temb_total], NULL: the context's scratch row) and the per-timestep cache is neither read nor filled
  const float* temb_row = nullptr; float* bias_row = nullptr;
  bool cached_kv = false;              // read the text K / V of text_kv_precompute instead of projecting the context
  bool record = false;                 // push every op on the context's tape and keep every activation (never with cached_kv)
  const PnpState* pnp = nullptr;       // Plug-and-Play injection; NULL = none
  UNetShare share;
};
// What the graph mutates while one forward runs: on unet_fwd's stack, reached by the op wrappers through pnpi_ctx::fw.  With fw == nullptr
// (VAE, CLIP towers) no GEMM is pinned and nothing is recorded.
struct UNetFlight {
  int tf_index = 0, up_res_index = 0;  // transformer block counter (MasaCtrl start_layer, the K / V cache), decoder ResNet counter (Plug-and-Play)
  // a GEMM over pin_from rows takes the tile / split-K its pin_to-row form gets: in the deduplicated prefix ("cfg_dedup" = 2), or throughout
  int pin_from = 0, pin_to = 0;
  const float* bias_eff = nullptr;     // [temb_total] conv1 bias + time embedding of this forward (points into bias_tab once cached)
  bool cached_kv = false, record = false;
  PnpState pnp;                        // off without UNetCall::pnp
  UNetShare share;
  explicit UNetFlight(const UNetShare& s) : share(s) { pin_base(); }
  // the GEMM pin outside the deduplicated prefix: none, or (pinned row sharing) compact rows -> logical rows
  void pin_base() { const bool on = share.pin && share.U > 0; pin_from = on ? share.from : 0; pin_to = on ? share.to : 0; }
};
struct FlightScope { pnpi_ctx* c; FlightScope(pnpi_ctx* c_, UNetFlight* f) : c(c_) { c->fw = f; } ~FlightScope() { c->fw = nullptr; } };
struct DryScope { pnpi_ctx* c; bool prev; explicit DryScope(pnpi_ctx* c_) : c(c_), prev(c_->dry) { c->dry = true; } ~DryScope() { c->dry = prev; } };      // a sizing run
struct TfDedup { int U; const int* dmap; };     // transformer_fwd: x holds U rows, the block's first half runs on them
#define PROF(cls, flops, bytes, expr) PROFD(cls, flops, bytes, 0, 0, 0, expr)
#define PROFD(cls, flops, bytes, d0, d1, d2, expr)            \
  do {                                                        \
    if (c->prof_on && !c->dry) {                              \
      ProfRec _pr; prof_open(c, _pr);                         \
      int _r = (expr);                                        \
      prof_close(c, _pr, (cls), (flops), (bytes), (d0), (d1), (d2)); \
      if (_r) return fail_launch(c, _r, #expr);               \
    } else {                                                  \
      int _r = (expr);                                        \
      if (_r) return fail_launch(c, _r, #expr);               \
    }                                                         \
  } while (0)

// ---------------------------------------------------------------------------------------------------- activation tape
// A differentiable forward (NullInversion.null_optimization: loss.backward() w.r.t. the unconditional embedding, inversion.py:196-225)
// records every op of the UNet forward below -- through the same wrappers the plain forward uses -- and keeps all activations (the
// arenas stop releasing temporaries; one UNet row is ~0.4 GB).  tape_backward() walks the records in reverse.  Only activation
// gradients exist (no weight gradients); the fused variants that would hide an intermediate are switched off while recording
// (GEGLU in the GEMM epilogue, V^T written by the projection GEMM, the text K/V cache).
enum { TK_CONV = 0, TK_GEMM = 1, TK_GN = 2, TK_LN = 3, TK_ATTN = 4, TK_GEGLU = 5, TK_TRANSPOSE_V = 6 };
struct TapeOp {
  int kind = 0;
  const half_t *x1 = nullptr, *x2 = nullptr, *res = nullptr;
  half_t* out = nullptr;
  int C1 = 0, C2 = 0, B = 0, H = 0, W = 0, Ho = 0, Wo = 0, stride = 1, pad = 0, ups = 0, N = 0;      // conv
  const ConvW* cw = nullptr;
  int lda = 0, M = 0, K = 0, ldw = 0, ldo = 0;                                                        // gemm
  const half_t* w = nullptr;
  float alpha = 1.f;
  const NormW* nw = nullptr;                                                                         // norms
  int G = 0, HW = 0, silu = 0;
  float eps = 0.f;
  const half_t *q = nullptr, *k = nullptr, *v = nullptr;                                             // attention (base tensors)
  const float* lse = nullptr;                                                                        // [B][heads][Nq] log-sum-exp left by the forward kernel
  int ldq = 0, q_off = 0, ldk = 0, k_off = 0, ldv = 0, v_off = 0, heads = 0, Nq = 0, Nk = 0, Dp = 0, dh = 0;
  float scale = 0.f;
};
struct Tape {
  std::vector<TapeOp> ops;
  const half_t* no_grad_input = nullptr;              // the network input: its consumers' dgrad is skipped
  const half_t* ctx16 = nullptr;                      // the text context of this forward: gradients into it are summed in fp32
  Bump garena;                                        // gradient buffers + scratch of one backward
  std::unordered_map<const void*, half_t*> grads;     // activation pointer -> gradient buffer (same shape)
  std::unordered_map<const void*, half_t*> wd;        // weight pointer -> dgrad repack (device, built once)
  float* d_ctx = nullptr;                             // [rows * ctx_len * cross_dim] fp32
  void* attn_scratch = nullptr; size_t attn_scratch_bytes = 0;
};
// a recording forward (or the dry run that sizes the arenas for one) keeps every activation and takes the plain-layout transformer block
static inline bool keep_acts(pnpi_ctx* c) { return c->fw && c->fw->record; }
static inline bool taping(pnpi_ctx* c) { return keep_acts(c) && !c->dry; }

// ---------------------------------------------------------------------------------------------------- op wrappers
// Per-channel GroupNorm partial sums attached to an activation by the GEMM that produced it ([tiles][C][2], `rows` per tile).
// op_conv fills one for its caller on request: rows = rows per tile actually produced (0 = none).
struct Stats { const float* p = nullptr; int rows = 0; };
// Can launch_groupnorm_fused consume partials of `rows` rows per m-tile for maps of HW pixels?  The partials are indexed by global
// m-tile, so a tile must not straddle two batch items (HW % rows); beyond 256 tiles per item the statistics are recomputed.
// One rule for op_gn (which falls back to launch_groupnorm) and pnpi_op_groupnorm_stats (which refuses).
static inline bool gn_stats_usable(int HW, int rows) { return rows > 0 && HW % rows == 0 && HW / rows <= 256; }

static half_t* talloc(pnpi_ctx* c, size_t n) { return (half_t*)c->temp.alloc(n * sizeof(half_t)); }
static half_t* palloc(pnpi_ctx* c, size_t n) { return (half_t*)c->persist.alloc(n * sizeof(half_t)); }

static int op_gn(pnpi_ctx* c, const half_t* x1, const half_t* x2, int C1, int C2, int B, int HW, const NormW& nw, int G, float eps,
                 int silu, half_t* out, Stats s1 = Stats(), Stats s2 = Stats()) {
  if (c->dry) return 0;
  if (taping(c)) {
    TapeOp o; o.kind = TK_GN; o.x1 = x1; o.x2 = x2; o.C1 = C1; o.C2 = C2; o.B = B; o.HW = HW; o.nw = &nw; o.G = G; o.eps = eps; o.silu = silu; o.out = out;
    c->tape->ops.push_back(o);
  }
  const bool ok1 = s1.p && gn_stats_usable(HW, s1.rows);
  const bool ok2 = !x2 || (s2.p && gn_stats_usable(HW, s2.rows));
  if (ok1 && ok2 && !g_gn_nofuse) {
    PROFD(PNPI_KC_GROUPNORM, 0.0, 2.0 * B * HW * (double)(C1 + C2) * 2.0, B * HW, C1 + C2, 1,
          launch_groupnorm_fused(x1, x2, C1, C2, B, HW, G, eps, nw.g, nw.b, silu, out, s1.p, HW / s1.rows, s2.p,
                                 x2 ? HW / s2.rows : 1, c->gn_partial, c->st));
    return 0;
  }
  PROFD(PNPI_KC_GROUPNORM, 0.0, 3.0 * B * HW * (double)(C1 + C2) * 2.0, B * HW, C1 + C2, 0,
       launch_groupnorm(x1, x2, C1, C2, B, HW, G, eps, nw.g, nw.b, silu, out, c->gn_partial, c->st));
  return 0;
}

struct VtOut { void* outT = nullptr; int col0 = 1 << 30; int ld = 0; int f32 = 0; int rpb = 1; int perm16 = 0; };


static int igemm_prof(pnpi_ctx* c, const GemmP& p, double alg_flops, Stats* so = nullptr) {
  int srows = 0, r;
  // inside the pinned deduplicated prefix: configured as the same layer over all rows of the launch
  // Invariant behind the bit-identity claims of "cfg_dedup" = 2 and "src_share" = 2: a pinned GEMM's M is proportional to the row
  // count (M = pin_from rows x tokens), so M / pin_from * pin_to is exactly the M of the same layer in the full-row launch.  A GEMM
  // whose M is no multiple of pin_from is not row-proportional (the one-row time-embedding products): it has the same M in the
  // full-row launch and stays unpinned (sel_M = 0), as there.
  const UNetFlight* f = c->fw;
  const int sel_M = (f && f->pin_to > 0 && p.M % f->pin_from == 0) ? (int)((long)p.M / f->pin_from * f->pin_to) : 0;
  if (c->prof_on) {
    ProfRec pr; prof_open(c, pr);
    int used = 0;
    r = launch_igemm(p, c->splitk_ws, c->splitk_bytes, c->st, -1, 0, &used, &srows, sel_M);
    // algorithmic HBM bytes: the input tensor(s) once, the weight once, the output once (+ the residual it adds)
    const double in_rows = (double)p.B * p.H * p.W;
    const double alg_bytes = 2.0 * (in_rows * (p.C1 + p.C2) + (double)p.N * p.K + (double)p.M * (p.geglu ? p.N / 2 : p.N) * (p.res ? 2.0 : 1.0));
    igemm_last_launch(&pr.cfg, &pr.split, pr.geom);
    prof_close(c, pr, used, alg_flops, alg_bytes, p.M, p.N, p.K, p.ksize);
  } else {
    r = launch_igemm(p, c->splitk_ws, c->splitk_bytes, c->st, -1, 0, nullptr, &srows, sel_M);
  }
  if (so) so->rows = srows;
  return r;
}
static float* stats_alloc(pnpi_ctx* c, int M, int N) {   // worst case: 64-row tiles
  return (float*)c->persist.alloc((size_t)((M + 63) / 64) * N * 2 * sizeof(float));
}

static int op_conv(pnpi_ctx* c, const half_t* x1, int C1, const half_t* x2, int C2, int B, int H, int W, const ConvW& w, int stride,
                   int pad, int ups, const float* bias, const half_t* res, half_t* out, int Ho, int Wo, int N = -1,
                   const VtOut* vt = nullptr, Stats* so = nullptr, int ldo = 0) {      // ldo > 0: out's row stride (a column block of a wider buffer)
  GemmP p; gemm_defaults(p);
  int C1p = C2 ? C1 : w.cin_pad;  // single-source inputs are stored with the padded channel count
  p.x1 = x1; p.x2 = x2; p.C1 = C1p; p.C2 = C2; p.ldx1 = C1p; p.ldx2 = C2;
  p.B = B; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.ksize = w.k; p.stride = stride; p.pad = pad; p.ups = ups;
  p.K = w.k * w.k * (C1p + C2); p.w = w.w; p.ldw = p.K;
  p.M = B * Ho * Wo; p.N = N > 0 ? N : w.cout;
  p.bias = bias; p.res = res; p.ldres = p.N; p.out = out; p.ldo = ldo > 0 ? ldo : p.N;
  if (vt) { p.outT = vt->outT; p.vt_col0 = vt->col0; p.vt_ld = vt->ld; p.vt_f32 = vt->f32; p.rows_per_batch = vt->rpb; }
  c->ctr.executed_gemm_flops += 2.0 * p.M * p.N * p.K;
  if (so) { p.stats = stats_alloc(c, p.M, p.N); so->p = p.stats; so->rows = 0; }
  if (c->dry) return 0;
  if (taping(c)) {
    TapeOp o; o.kind = TK_CONV; o.x1 = x1; o.x2 = x2; o.C1 = C1p; o.C2 = C2; o.B = B; o.H = H; o.W = W; o.Ho = Ho; o.Wo = Wo; o.stride = stride; o.pad = pad;
    o.ups = ups; o.N = p.N; o.cw = &w; o.res = res; o.out = out;
    c->tape->ops.push_back(o);
  }
  return igemm_prof(c, p, 2.0 * p.M * (double)w.cout * w.k * w.k * w.cin, so);
}

struct GemmBatch { int n = 1; long sa = 0, sw = 0, sout = 0, soutT = 0; };   // n problems: strides of a / w / out in elements, of vt->outT in bytes
static int op_gemm(pnpi_ctx* c, const half_t* a, int lda, int M, int K, const half_t* w, int ldw, int N, const float* bias,
                   const half_t* res, int ldres, half_t* out, int ldo, float alpha = 1.f, const VtOut* vt = nullptr,
                   double alg_flops = -1.0, int geglu = 0, const GemmBatch* gb = nullptr) {
  GemmP p; gemm_defaults(p);
  if (gb && gb->n > 1) { p.nbatch = gb->n; p.sx1 = gb->sa; p.sw = gb->sw; p.sout = gb->sout; p.soutT = gb->soutT; }
  p.x1 = a; p.C1 = K; p.ldx1 = lda; p.B = 1; p.H = 1; p.W = M; p.Ho = 1; p.Wo = M; p.ksize = 1;
  p.w = w; p.ldw = ldw; p.M = M; p.N = N; p.K = K; p.bias = bias; p.res = res; p.ldres = ldres; p.alpha = alpha;
  p.out = out; p.ldo = ldo; p.geglu = geglu;
  if (vt) { p.outT = vt->outT; p.vt_col0 = vt->col0; p.vt_ld = vt->ld; p.vt_f32 = vt->f32; p.rows_per_batch = vt->rpb; p.vt_perm16 = vt->perm16; }
  c->ctr.executed_gemm_flops += 2.0 * M * N * K * p.nbatch;
  if (c->dry) return 0;
  if (taping(c) && out) {        // plain row-major outputs only: the recording forward uses no transposed / fused-GEGLU epilogue
    TapeOp o; o.kind = TK_GEMM; o.x1 = a; o.lda = lda; o.M = M; o.K = K; o.w = w; o.ldw = ldw; o.N = N; o.res = res; o.out = out; o.ldo = ldo; o.alpha = alpha;
    c->tape->ops.push_back(o);
  }
  return igemm_prof(c, p, alg_flops >= 0 ? alg_flops : 2.0 * M * (double)N * K * p.nbatch);
}

// The main branch of a ResNet block up to conv2's input: norm1 -> conv1 (+ the time-embedding bias) -> norm2 over B rows of x1 | x2
static int resnet_main(pnpi_ctx* c, const ResnetW& r, const half_t* x1, int C1, const half_t* x2, int C2, int B, int H, int W, int G,
                       float eps, Stats s1, Stats s2, half_t** t3) {
  const int HW = H * W;
  const size_t M = (size_t)B * HW;
  half_t* t1 = talloc(c, M * r.cin);
  CK(op_gn(c, x1, x2, C1, C2, B, HW, r.n1, G, eps, 1, t1, s1, s2));
  half_t* t2 = talloc(c, M * r.cout);
  const float* b1 = r.temb_off >= 0 ? c->fw->bias_eff + r.temb_off : r.c1.b;
  Stats st2;
  CK(op_conv(c, t1, r.cin, nullptr, 0, B, H, W, r.c1, 1, 1, 0, b1, nullptr, t2, H, W, -1, nullptr, &st2));
  *t3 = talloc(c, M * r.cout);
  CK(op_gn(c, t2, nullptr, r.cout, 0, B, HW, r.n2, G, eps, 1, *t3, st2));
  return 0;
}
// ResnetBlock2D.forward (my_diffusers/models/resnet.py:331-365); x2 = skip tensor concatenated on the channel axis
static int resnet_fwd(pnpi_ctx* c, const ResnetW& r, const half_t* x1, int C1, const half_t* x2, int C2, int B, int H, int W, int G,
                      float eps, half_t* out, Stats s1 = Stats(), Stats s2 = Stats(), Stats* so = nullptr) {
  const size_t mk = c->temp.mark();
  half_t* t3;
  CKP(resnet_main(c, r, x1, C1, x2, C2, B, H, W, G, eps, s1, s2, &t3));
  Stats sto;
  const half_t* sc = x1;
  if (r.has_sc) {      // conv2 below adds it as its residual
    half_t* s = talloc(c, (size_t)B * H * W * r.cout);
    CK(op_conv(c, x1, C1, x2, C2, B, H, W, r.sc, 1, 0, 0, r.sc.b, nullptr, s, H, W));
    sc = s;
  }
  CK(op_conv(c, t3, r.cout, nullptr, 0, B, H, W, r.c2, 1, 1, 0, r.c2.b, sc, out, H, W, -1, nullptr, &sto));
  if (so) *so = sto;
  if (!keep_acts(c)) c->temp.release(mk);      // a recording forward keeps every activation for the backward pass
  return 0;
}

// The same block at a Plug-and-Play conv-injection step (run_editing_pnp.py:276-281: after conv2, before the shortcut add, rows 1 and 2
// of every image take row 0's hidden states).  Everything the main branch computes for rows 1 and 2 is overwritten unread, so
// norm1 -> conv1 (+temb) -> norm2 -> conv2 run on the nimg source rows only and out[r] = shortcut(x[r]) + h[image of r]: the shortcut
// convolution writes `out`, add_rows_bcast_f16 adds the broadcast main branch in place (two fp16 roundings where conv2's residual
// epilogue has one).  The block's output carries no GroupNorm partial sums: its consumer recomputes the statistics.
static int resnet_fwd_pnp(pnpi_ctx* c, const ResnetW& r, const half_t* x1, int C1, const half_t* x2, int C2, int B, int H, int W, int G,
                          float eps, half_t* out, Stats s1, Stats s2) {
  const PnpState& ps = c->fw->pnp;
  const int HW = H * W, n = ps.nimg;
  if (B != 3 * n || !x2) return fail(c, PNPI_ESTATE, "Plug-and-Play conv injection: a decoder ResNet of a [img][3]-row launch expected");
  if (((size_t)HW * C1) % 8 || ((size_t)HW * C2) % 8 || ((size_t)HW * r.cout) % 8)
    return fail(c, PNPI_ESHAPE, "Plug-and-Play conv injection: row size is no multiple of 8 halfs");
  const size_t mk = c->temp.mark();
  const size_t M = (size_t)n * HW;
  const half_t *xs1 = x1, *xs2 = x2;
  if (n > 1) {      // the source rows 3 i, gathered; their statistics are recomputed (the partial sums are indexed by the launch's tiles)
    half_t *g1 = talloc(c, M * C1), *g2 = talloc(c, M * C2);
    if (!c->dry) {
      CK(launch_gather_rows_f16(x1, ps.src_rows, n, (size_t)HW * C1, g1, c->st));
      CK(launch_gather_rows_f16(x2, ps.src_rows, n, (size_t)HW * C2, g2, c->st));
    }
    xs1 = g1; xs2 = g2; s1 = s2 = Stats();
  }
  half_t* t3;
  CKP(resnet_main(c, r, xs1, C1, xs2, C2, n, H, W, G, eps, s1, s2, &t3));
  half_t* hsrc = talloc(c, M * r.cout);
  CK(op_conv(c, t3, r.cout, nullptr, 0, n, H, W, r.c2, 1, 1, 0, r.c2.b, nullptr, hsrc, H, W));
  if (!r.has_sc) return fail(c, PNPI_ESHAPE, "Plug-and-Play conv injection: the site has no shortcut convolution");   // a decoder ResNet concatenates its skip: cin != cout
  CK(op_conv(c, x1, C1, x2, C2, B, H, W, r.sc, 1, 0, 0, r.sc.b, nullptr, out, H, W));
  if (!c->dry) CK(launch_add_rows_bcast_f16(out, hsrc, ps.hrow, B, (size_t)HW * r.cout, out, c->st));
  c->temp.release(mk);
  return 0;
}

// The hooked attention forward of models/p2p/attention_control.py:20-47, literally: sim = q k^T * scale -> softmax -> controller(attn,
// is_cross, place) -> attn v, with the probabilities materialised in fp32 for a host callback (level-1 fallback for controllers
// without a descriptor).  One GEMM pair per (row, head); rows are not redirected (the callback does the editing).
static int attn_materialized(pnpi_ctx* c, const AttnP& a, int B, int is_cross, int place, int layer) {
  const half_t *q = a.q, *k = a.k, *vt = a.vt;
  const int ldq = a.ldq, q_off = a.q_off, ldk = a.ldk, k_off = a.k_off, ldv = a.ldv, ldo = a.ldo, heads = a.heads, Nq = a.Nq, Nk = a.Nk, Dp = a.Dp, dh = a.dh;
  const int ldp = round_up_i(Nk, 8);
  const size_t need = align_up((size_t)B * heads * Nq * Nk * sizeof(float), 256);
  // the fp16 copy of one (row, head) probability block (the MFMA operand of P V) lives behind the fp32 tensor in the caller's buffer
  if (!c->attn_buf || need + (size_t)Nq * ldp * sizeof(half_t) > c->attn_buf_bytes)
    return fail(c, PNPI_ENOMEM, "attention callback buffer too small for this site (rows*heads*Nq*Nk floats + Nq*Nk halfs)");
  half_t* p16 = reinterpret_cast<half_t*>(reinterpret_cast<char*>(c->attn_buf) + need);
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < heads; ++h) {
      float* S = c->attn_buf + ((size_t)b * heads + h) * Nq * Nk;
      VtOut v; v.outT = S; v.col0 = 0; v.ld = Nk; v.f32 = 1; v.rpb = Nk;      // outT[q][key] = scale * sum_d K[key][d] Q[q][d]
      CK(op_gemm(c, k + (size_t)b * Nk * ldk + k_off + h * Dp, ldk, Nk, Dp, q + (size_t)b * Nq * ldq + q_off + h * Dp, ldq, Nq, nullptr,
                 nullptr, 0, nullptr, Nq, a.scale, &v));
    }
  CK(launch_softmax_rows_f32(c->attn_buf, (size_t)B * heads * Nq, Nk, c->st));
  CKH(hipStreamSynchronize(c->st));                 // the callback is host code: it sees finished probabilities
  if (c->attn_cb(c->attn_cb_user, c->attn_buf, B, heads, Nq, Nk, is_cross, place, layer)) return fail(c, PNPI_ESTATE, "attention callback failed");
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < heads; ++h) {
      const float* S = c->attn_buf + ((size_t)b * heads + h) * Nq * Nk;
      CK(launch_f32_rows_to_f16_padded(S, Nq, Nk, ldp, p16, c->st));
      CK(op_gemm(c, p16, ldp, Nq, ldp, vt + ((size_t)b * heads + h) * Dp * (size_t)ldv, ldv, dh, nullptr, nullptr, 0,
                 a.o + (size_t)b * Nq * ldo + h * dh, ldo));
    }
  return 0;
}
static int op_ln(pnpi_ctx* c, const half_t* x, int M, int C, const NormW& nw, half_t* out) {
  if (c->dry) return 0;
  if (taping(c)) { TapeOp o; o.kind = TK_LN; o.x1 = x; o.M = M; o.C1 = C; o.nw = &nw; o.eps = 1e-5f; o.out = out; c->tape->ops.push_back(o); }
  PROF(PNPI_KC_LAYERNORM, 0.0, 2.0 * M * (double)C * 2.0, launch_layernorm(x, M, C, 1e-5f, nw.g, nw.b, out, c->st));
  return 0;
}
// One attention site of a transformer block: the fields AttnP, CrossEditP and the tape's TK_ATTN record share, written once.  The caller
// adds the row table (and vt_perm / aug / lse where the site has them).
static AttnP attn_site(const TransformerW& t, const half_t* q, int ldq, const half_t* k, int ldk, int k_off, const half_t* vt, int ldv,
                       half_t* o, int Nq, int Nk, float scale) {
  AttnP a; a.q = q; a.ldq = ldq; a.q_off = 0; a.k = k; a.ldk = ldk; a.k_off = k_off; a.vt = vt; a.ldv = ldv; a.rows = nullptr; a.nrows = 0;
  a.o = o; a.ldo = t.C; a.heads = t.heads; a.Nq = Nq; a.Nk = Nk; a.Dp = t.Dp; a.dh = t.dh; a.scale = scale;
  return a;
}
static CrossEditP cross_edit_site(const AttnP& a) {
  CrossEditP e; e.q = a.q; e.ldq = a.ldq; e.q_off = a.q_off; e.k = a.k; e.ldk = a.ldk; e.k_off = a.k_off; e.vt = a.vt; e.ldv = a.ldv;
  e.o = a.o; e.ldo = a.ldo; e.heads = a.heads; e.Nq = a.Nq; e.Nk = a.Nk; e.Dp = a.Dp; e.dh = a.dh; e.scale = a.scale;
  return e;
}
// the TK_ATTN record of site `a` over B rows; v: the plain-layout tensor a.vt is the transposed copy of
static void tape_attn(pnpi_ctx* c, const AttnP& a, const half_t* v, int ldv, int v_off, int B) {
  TapeOp o; o.kind = TK_ATTN; o.q = a.q; o.ldq = a.ldq; o.q_off = a.q_off; o.k = a.k; o.ldk = a.ldk; o.k_off = a.k_off; o.v = v; o.ldv = ldv; o.v_off = v_off;
  o.out = a.o; o.ldo = a.ldo; o.heads = a.heads; o.Nq = a.Nq; o.Nk = a.Nk; o.Dp = a.Dp; o.dh = a.dh; o.scale = a.scale; o.B = B; o.lse = a.lse;
  c->tape->ops.push_back(o);
}
// What a transformer block's self-attention does at this step, decided ahead of its launch.  form: one flash launch over `rows`; that
// launch plus the class-restricted kernel over `rows_tgt` (mask-guided MasaCtrl: source rows and rows of other images take the plain
// launch unchanged, every target row runs over its source row's K / V with this level's resized masks, pnpi_masa_set_masks); or the
// materialised probabilities handed to the host callback.  table: which rows `rows` redirects.
enum { SA_FLASH = 0, SA_FLASH_MASKED = 1, SA_CALLBACK = 2 };
enum { ST_IDENTITY = 0, ST_REPLACE = 1, ST_MASA = 2, ST_MASA_MASKED = 3, ST_PNP = 4 };
struct SelfAttn {
  int form = SA_FLASH, table = ST_IDENTITY;
  const int* rows = nullptr; int nrows = 0;
  const int* rows_tgt = nullptr; int nrows_tgt = 0; AttnMaskP mask{};      // SA_FLASH_MASKED
  int err = 0; const char* msg = nullptr;                                  // the combination is refused: fail(c, err, msg)
};
// B: the rows in hand; dedup: they are the distinct latents of a "cfg_dedup" first half, which only the identity table can serve
static SelfAttn self_attn_resolve(pnpi_ctx* c, bool use_ctrl, int cur_step, int block_index, int H, int W, int B, bool dedup) {
  const CtrlDev& cd = c->cd;
  SelfAttn s; s.rows = cd.rows_id; s.nrows = B;
  if (keep_acts(c)) return s;      // a recording forward: one prompt row, no controller, no callback
  auto refuse = [&s](int err, const char* msg) { s.err = err; s.msg = msg; return s; };
  const bool masa_step = cd.masa_step_list ? (cur_step >= 0 && cur_step < (int)cd.masa_step_on.size() && cd.masa_step_on[cur_step]) : cur_step >= cd.masa_start_step;
  const bool masa_layer = cd.masa_layer_mask ? ((cd.masa_layer_mask >> block_index) & 1u) != 0 && block_index < 31 : block_index >= cd.masa_start_layer;
  if (use_ctrl && cd.any_edit && cur_step >= cd.self_lo && cur_step < cd.self_hi && H * W <= cd.self_max_tokens) { s.table = ST_REPLACE; s.rows = cd.rows_rep; }
  else if (use_ctrl && cd.masa_any && masa_step && masa_layer) { s.table = ST_MASA; s.rows = cd.rows_masa; }
  const bool redirects = s.table != ST_IDENTITY;
  if (dedup && (redirects || c->attn_cb)) return refuse(PNPI_ESTATE, "cfg_dedup: this block's self-attention redirects rows");
  // Plug-and-Play q/k injection (run_editing_pnp.py:190-201): {r, src, src, r} for the rows of every image, at every token count
  const PnpState& ps = c->fw->pnp;
  if (ps.on && ps.qk && block_index < 32 && ((ps.qk_mask >> block_index) & 1u)) {
    if (dedup || c->attn_cb || redirects || B != 3 * ps.nimg)
      return refuse(PNPI_ESTATE, "Plug-and-Play q/k injection does not combine with cfg_dedup, a host callback or a controller");
    s.table = ST_PNP; s.rows = ps.rows;
  }
  if (c->attn_cb) s.form = SA_CALLBACK;       // rows are not redirected there: the callback does the editing
  else if (s.table == ST_MASA && cd.masa_masked && !c->dry) {
    int lev = -1;
    for (size_t l = 0; l < c->mm.side.size(); ++l) if (c->mm.side[l] == H && H == W) lev = (int)l;
    if (lev < 0) return refuse(PNPI_ESTATE, "mask-guided MasaCtrl: no resized mask for this self-attention level");
    s.form = SA_FLASH_MASKED; s.table = ST_MASA_MASKED;
    s.rows = cd.rows_masa_plain; s.nrows = cd.n_masa_plain; s.rows_tgt = cd.rows_masa_tgt; s.nrows_tgt = cd.n_masa_tgt;
    s.mask.kcls = c->mm.s_at(lev); s.mask.qcls = c->mm.t_at(lev); s.mask.mrow = cd.masa_tgt_img;
  }
  return s;
}

// SpatialTransformer + BasicTransformerBlock (my_diffusers/models/attention.py:140-200) with the hooked attention of
// models/p2p/attention_control.py:20-47 and the controller semantics of :178-190, :269-282 fused into the kernels: four stages over
// one TfBlock.  A recording forward (null-text path: one prompt row, no controller) runs the same stages; where the backward needs a
// plain layout the stage branches on `rec`: q | k | v as one row-major projection output (V^T for the flash kernel is a transposed
// COPY) with the log-sum-exp kept, the text K / V projected inside the forward from the context, GEGLU unfused.
struct TfBlock {
  const TransformerW& t;
  int H, W, N, C, hd;      // the map, its tokens, channels, heads * Dp
  int block_index;         // transformer blocks in execution order (down 0.., mid, up ..15)
  float scale;
  int B, M, Bf, Mf;        // the rows in hand and their tokens (dd: of the text-independent first half, until tf_cross_attn expands them); of the launch
  const TfDedup* dd;
  bool rec, use_ctrl;      // rec = keep_acts: every temporary stays, TapeOp records are pushed while taping
  int cur_step;
};
// ---- GroupNorm + proj_in
static int tf_enter(pnpi_ctx* c, const TfBlock& s, const half_t* x, Stats sx, half_t** hs) {
  half_t* g0 = talloc(c, (size_t)s.M * s.C);
  CK(op_gn(c, x, nullptr, s.C, 0, s.B, s.N, s.t.gn, c->cfg.norm_groups, 1e-6f, 0, g0, sx));
  *hs = talloc(c, (size_t)s.M * s.C);
  CK(op_conv(c, g0, s.C, nullptr, 0, s.B, s.H, s.W, s.t.proj_in, 1, 0, 0, s.t.proj_in.b, nullptr, *hs, s.H, s.W));
  return 0;
}
// ---- self-attention: ln1, the q | k | v projection, the launch self_attn_resolve chose, o1 (+ hs)
static int tf_self_attn(pnpi_ctx* c, const TfBlock& s, const half_t* hs, half_t** hs1) {
  const TransformerW& t = s.t;
  const int B = s.B, M = s.M, N = s.N, C = s.C, hd = s.hd;
  half_t* n1 = talloc(c, (size_t)M * C);
  CK(op_ln(c, hs, M, C, t.ln1, n1));
  const int ldq = (s.rec ? 3 : 2) * hd;      // q | k, and recording | v
  half_t* qkv = talloc(c, (size_t)M * ldq);
  const int ldv = round_up_i(N, 8);
  half_t* vt = talloc(c, (size_t)B * hd * ldv);
  half_t* ao = talloc(c, (size_t)M * C);
  AttnP a = attn_site(t, qkv, ldq, qkv, ldq, hd, vt, ldv, ao, N, N, s.scale);
  if (s.rec) {
    a.lse = (float*)talloc(c, (size_t)B * t.heads * N * 2);       // per-query log-sum-exp for the backward kernel
    CK(op_gemm(c, n1, C, M, C, t.w_qkv, C, 3 * hd, nullptr, nullptr, 0, qkv, 3 * hd));
    for (int b = 0; b < B && !c->dry; ++b) CK(launch_transpose_f16(qkv + (size_t)b * N * 3 * hd + 2 * hd, 3 * hd, N, hd, vt + (size_t)b * hd * ldv, ldv, c->st));
  } else {
    // call-back path: P V runs over the padded key count, so the pad columns of V^T must be zeros -- cleared BEFORE the projection fills
    // the real columns (only the 2 x 2 level of the narrow test configurations has a token count that is not a multiple of 8)
    if (c->attn_cb && !c->dry && ldv != N) CKH(hipMemsetAsync(vt, 0, (size_t)B * hd * ldv * sizeof(half_t), c->st));
    // the 4096-token sites run the 64-wide LDS-DMA kernel, which reads V^T in the permuted key order (one ds_read_b128 per P V fragment):
    // the projection's epilogue writes it that way (not under a host callback: the materialised path reads plain V^T)
    a.vt_perm = (g_vt_perm && !c->attn_cb && N % 16 == 0 && attn_flash_uses_dma64(t.Dp, N, 0)) ? 1 : 0;
    a.aug = (t.b_qkv_aug && g_attn_aug) ? 1 : 0;      // K / V column dh hold 1.0 (the projection below adds b_qkv_aug)
    VtOut v; v.outT = vt; v.col0 = 2 * hd; v.ld = ldv; v.f32 = 0; v.rpb = N; v.perm16 = a.vt_perm;
    CK(op_gemm(c, n1, C, M, C, t.w_qkv, C, 3 * hd, t.b_qkv_aug, nullptr, 0, qkv, 2 * hd, 1.f, &v, 2.0 * M * 3.0 * C * C));
  }
  const SelfAttn sa = self_attn_resolve(c, s.use_ctrl, s.cur_step, s.block_index, s.H, s.W, B, s.dd != nullptr);
  if (sa.err) return fail(c, sa.err, sa.msg);
  a.rows = sa.rows; a.nrows = sa.nrows;
  if (!s.rec || !c->dry) c->ctr.executed_attn_flops += 4.0 * B * t.heads * (double)N * N * t.Dp;      // the recording forward's sizing run has never counted its attention
  if (!c->dry && sa.form == SA_CALLBACK) CKP(attn_materialized(c, a, B, 0, t.place, 2 * s.block_index));
  else if (!c->dry) {
    PROFD(PNPI_KC_ATTN_FLASH, 4.0 * a.nrows * t.heads * (double)N * N * t.dh, 0.0, N, N, t.Dp, launch_attn_flash(a, c->st));
    if (sa.form == SA_FLASH_MASKED) {
      AttnP am = a; am.rows = sa.rows_tgt; am.nrows = sa.nrows_tgt;
      PROFD(PNPI_KC_ATTN_FLASH, 4.0 * am.nrows * t.heads * (double)N * N * t.dh, 0.0, N, N, t.Dp, launch_attn_flash_masked(am, sa.mask, c->st));
    }
    if (taping(c)) tape_attn(c, a, qkv, 3 * hd, 2 * hd, B);
  }
  *hs1 = talloc(c, (size_t)M * C);
  CK(op_gemm(c, ao, C, M, C, t.o1.w, C, C, t.o1.b, hs, C, *hs1, C));
  return 0;
}
// ---- cross-attention: ln2, q2, the text K / V (cached, or projected here), the launch, the controller's cross edit, o2 (+ hs1).  A
// deduplicated block leaves its compact rows behind q2: *x, like s.B / s.M, goes out at the rows of the launch; the GEMM pin ends there.
static int tf_cross_attn(pnpi_ctx* c, TfBlock& s, const half_t* ctx16, const half_t** x, const half_t* hs1, half_t** hs2) {
  const TransformerW& t = s.t;
  const CtrlDev& cd = c->cd;
  const int N = s.N, C = s.C, hd = s.hd, X = c->cfg.cross_dim, T = c->cfg.ctx_len;
  const bool edit = s.use_ctrl && cd.any_edit && !s.rec;
  int B = s.B, M = s.M;
  half_t* n2 = talloc(c, (size_t)M * C);
  CK(op_ln(c, hs1, M, C, t.ln2, n2));
  half_t* q2 = talloc(c, (size_t)M * hd);
  CK(op_gemm(c, n2, C, M, C, t.w_q2, C, hd, nullptr, nullptr, 0, q2, hd, 1.f, nullptr, 2.0 * M * (double)C * C));
  if (const TfDedup* dd = s.dd) {      // from here on every row has its own text: the three tensors the second half reads, at the rows of the launch
    c->fw->pin_base();
    B = s.B = s.Bf; M = s.M = s.Mf;
    half_t *hs1f = talloc(c, (size_t)M * C), *q2f = talloc(c, (size_t)M * hd), *xf = talloc(c, (size_t)M * C);
    CK(launch_gather_rows_f16(hs1, dd->dmap, B, (size_t)N * C, hs1f, c->st));
    CK(launch_gather_rows_f16(q2, dd->dmap, B, (size_t)N * hd, q2f, c->st));
    CK(launch_gather_rows_f16(*x, dd->dmap, B, (size_t)N * C, xf, c->st));
    hs1 = hs1f; q2 = q2f; *x = xf;
  }
  const int ldv2 = round_up_i(T, 8);
  const int ldk2 = (s.rec ? 2 : 1) * hd;      // k, and recording | v
  half_t *k2, *vt2;
  if (c->fw->cached_kv) {     // projected once per loop by text_kv_precompute (never while recording)
    k2 = c->tkv.k[s.block_index]; vt2 = c->tkv.vt[s.block_index];
  } else {
    k2 = talloc(c, (size_t)B * T * ldk2);
    vt2 = talloc(c, (size_t)B * hd * ldv2);
    if (s.rec) {
      CK(op_gemm(c, ctx16, X, B * T, X, t.w_kv2, X, 2 * hd, nullptr, nullptr, 0, k2, 2 * hd));
      for (int b = 0; b < B && !c->dry; ++b) CK(launch_transpose_f16(k2 + (size_t)b * T * 2 * hd + hd, 2 * hd, T, hd, vt2 + (size_t)b * hd * ldv2, ldv2, c->st));
    } else {
      // call-back path: the P V product runs over the padded key count, so the pad columns of V^T must be zeros (not stale arena bytes)
      if (c->attn_cb && !c->dry && ldv2 != T) CKH(hipMemsetAsync(vt2, 0, (size_t)B * hd * ldv2 * sizeof(half_t), c->st));
      VtOut v; v.outT = vt2; v.col0 = hd; v.ld = ldv2; v.f32 = 0; v.rpb = T;
      CK(op_gemm(c, ctx16, X, B * T, X, t.w_kv2, X, 2 * hd, nullptr, nullptr, 0, k2, hd, 1.f, &v, 2.0 * B * T * 2.0 * C * X));
    }
  }
  half_t* ao2 = talloc(c, (size_t)M * C);
  AttnP a = attn_site(t, q2, hd, k2, ldk2, 0, vt2, ldv2, ao2, N, T, s.scale);
  if (s.rec) a.lse = (float*)talloc(c, (size_t)B * t.heads * N * 2);
  a.rows = edit ? cd.rows_plain : cd.rows_id; a.nrows = edit ? cd.n_plain : B;
  if (!s.rec || !c->dry) c->ctr.executed_attn_flops += 4.0 * B * t.heads * (double)N * 96 * t.Dp;
  if (!c->dry && c->attn_cb && !s.rec) CKP(attn_materialized(c, a, B, 1, t.place, 2 * s.block_index + 1));
  else if (!c->dry) {
    PROFD(PNPI_KC_ATTN_FLASH, 4.0 * a.nrows * t.heads * (double)N * T * t.dh, 0.0, N, T, t.Dp, launch_attn_flash(a, c->st));
    if (taping(c)) tape_attn(c, a, k2, 2 * hd, hd, B);
    if (edit) {
      CrossEditP e = cross_edit_site(a);
      e.pairs = cd.pairs; e.npairs = cd.npairs; e.mmatT = cd.mmatT;
      int srow = s.cur_step < cd.n_alpha_rows ? s.cur_step : cd.n_alpha_rows - 1;
      e.c1 = cd.coef + ((size_t)srow * 2 + 0) * cd.npairs * 96;
      e.c2 = cd.coef + ((size_t)srow * 2 + 1) * cd.npairs * 96;
      const bool lb = cd.lb_any && t.lb_slot0 >= 0 && N == c->unet.lb_tokens;
      e.lb_alpha = lb ? cd.lb_alpha : nullptr;
      e.lb_acc = lb ? cd.lb_acc : nullptr;
      e.lb_slot0 = t.lb_slot0; e.lb_nslots = c->unet.lb_nslots; e.lb_planes = cd.lb_planes; e.write_src = 0;
      PROF(PNPI_KC_ATTN_EDIT, 4.0 * 2 * cd.npairs * t.heads * (double)N * T * t.dh, 0.0, launch_attn_cross_edit(e, c->st));
    }
  }
  *hs2 = talloc(c, (size_t)M * C);
  CK(op_gemm(c, ao2, C, M, C, t.o2.w, C, C, t.o2.b, hs1, C, *hs2, C));
  return 0;
}
// ---- GEGLU feed-forward and the exit: ln3, ff1 with the GEGLU product, ff2 (+ hs2), proj_out (+ x) -- or those two as one launch
static int tf_ff_exit(pnpi_ctx* c, const TfBlock& s, const half_t* x, const half_t* hs2, half_t* out, Stats* so) {
  const TransformerW& t = s.t;
  const int B = s.B, M = s.M, C = s.C, H = s.H, W = s.W;
  half_t* n3 = talloc(c, (size_t)M * C);
  CK(op_ln(c, hs2, M, C, t.ln3, n3));
  half_t* f1 = s.rec ? talloc(c, (size_t)M * 8 * C) : nullptr;      // recorded ahead of f2
  half_t* f2 = talloc(c, (size_t)M * 4 * C);
  if (!s.rec && C % 64 == 0) {
    // ff1 GEMM with the GEGLU product in its epilogue: [M][8C] never exists in memory
    CK(op_gemm(c, n3, C, M, C, t.ff1.w, C, 8 * C, t.ff1.b, nullptr, 0, f2, 4 * C, 1.f, nullptr, -1.0, 1));
  } else {
    // recording (the backward needs the gate pre-activation) and narrow test configurations: materialised, combined by a small kernel
    if (!f1) f1 = talloc(c, (size_t)M * 8 * C);
    CK(op_gemm(c, n3, C, M, C, t.ff1.w, C, 8 * C, t.ff1.b, nullptr, 0, f1, 8 * C));
    if (!c->dry) PROF(PNPI_KC_GEGLU, 0.0, 12.0 * M * (double)C * 2.0, launch_geglu(f1, M, 4 * C, f2, c->st));
    if (taping(c)) { TapeOp o; o.kind = TK_GEGLU; o.x1 = f1; o.out = f2; o.M = M; o.N = 4 * C; c->tape->ops.push_back(o); }
  }
  // ff2 + proj_out as one two-source 1 x 1 convolution over f2 | hs2 (K = 4C + C: both parts are whole 64-wide k-chunks).  Only with
  // folded weights that match the loaded ones (ff_fold_ready); the sizing dry run takes the two-launch path, which needs more memory
  // (hs3), so the knob can be flipped on a live context; a recording forward keeps hs3
  const bool fold = g_ff_fold && !c->dry && C % 64 == 0 && t.fo.w && c->warena_ref && c->warena_ref->ff_fold_ready && !s.rec;
  if (fold) CK(op_conv(c, f2, 4 * C, hs2, C, B, H, W, t.fo, 1, 0, 0, t.fo.b, x, out, H, W, -1, nullptr, so));
  else {
    half_t* hs3 = talloc(c, (size_t)M * C);
    CK(op_gemm(c, f2, 4 * C, M, 4 * C, t.ff2.w, 4 * C, C, t.ff2.b, hs2, C, hs3, C));
    CK(op_conv(c, hs3, C, nullptr, 0, B, H, W, t.proj_out, 1, 0, 0, t.proj_out.b, x, out, H, W, -1, nullptr, so));
  }
  return 0;
}

// dd (tuning "cfg_dedup"): x and sx hold dd->U rows, one per distinct latent of the B-row launch.  Everything up to the cross-attention
// query reads no text, so it runs on those rows; hs1, q2 and x are then expanded to the B rows (row r = compact row dmap[r]) for the
// second half.  Only for a block whose self-attention takes the identity row table at this step.  so (nullable): the output's GroupNorm sums.
static int transformer_fwd(pnpi_ctx* c, const TransformerW& t, const half_t* x, int B, int H, int W, const half_t* ctx16,
                           bool use_ctrl, int cur_step, half_t* out, Stats sx, Stats* so, const TfDedup* dd = nullptr) {
  const size_t mk = c->temp.mark();
  const int N = H * W, hd = t.heads * t.Dp, U = dd ? dd->U : B;
  TfBlock s{t, H, W, N, t.C, hd, c->fw->tf_index++, 1.0f / sqrtf((float)t.dh), U, U * N, B, B * N, dd, keep_acts(c), use_ctrl, cur_step};
  if (dd && ((N * s.C) % 8 || (N * hd) % 8)) return fail(c, PNPI_ESHAPE, "cfg_dedup: row size is no multiple of 8 halfs");
  // the sizing dry run takes the plain path and adds the three expanded tensors of the deduplicated one on top of it
  if (c->dry && s.block_index == 0 && !s.rec) { (void)talloc(c, (size_t)s.M * s.C); (void)talloc(c, (size_t)s.M * s.C); (void)talloc(c, (size_t)s.M * hd); }
  half_t *hs, *hs1, *hs2;
  CKP(tf_enter(c, s, x, sx, &hs));
  CKP(tf_self_attn(c, s, hs, &hs1));
  CKP(tf_cross_attn(c, s, ctx16, &x, hs1, &hs2));      // behind it s and x are at the rows of the launch
  CKP(tf_ff_exit(c, s, x, hs2, out, so));
  if (!s.rec) c->temp.release(mk);      // a recording forward keeps every activation for the backward pass
  return 0;
}
// TimestepEmbedding + the 22 time_emb_proj linears as three GEMVs: sinusoid row `sin_row` (device [C0]) -> conv1 bias + time embedding
// of every ResNet, `row` (device [temb_total])
static int temb_bias_row(pnpi_ctx* c, const float* sin_row, float* row) {
  const UNetW& u = c->unet;
  const int C0 = c->cfg.block_out_channels[0], TE = 4 * C0;
  CK(launch_gemv(sin_row, C0, u.t1.w, TE, u.t1.b, nullptr, 0, c->temb_h, c->st));
  CK(launch_gemv(c->temb_h, TE, u.t2.w, TE, u.t2.b, nullptr, 1, c->temb_emb, c->st));
  CK(launch_gemv(c->temb_emb, TE, u.temb_w, u.temb_total, u.temb_b, u.conv1_b, 1, row, c->st));
  return 0;
}
// A transformer block of the UNet behind *h (B rows of C channels): *h becomes its output and *s, the GroupNorm partial sums that travel
// with *h, those of the output.  A recording forward neither consumes nor produces them.
static int unet_transformer(pnpi_ctx* c, const TransformerW& t, half_t** h, int B, int H, int C, const half_t* ctx16, bool use_ctrl,
                            int cur_step, Stats* s) {
  half_t* out = palloc(c, (size_t)B * H * H * C);
  const Stats sx = keep_acts(c) ? Stats() : *s;
  *s = Stats();
  CKP(transformer_fwd(c, t, *h, B, H, H, ctx16, use_ctrl, cur_step, out, sx, keep_acts(c) ? nullptr : s));
  *h = out;
  return 0;
}
// The text-independent prefix once per distinct latent (tuning "cfg_dedup"): conv_in, down_res[0][0] and, while block 0's self-attention
// takes the identity row table, the first half of down_attn[0][0] on the ud.U rows of ud.lat_u.  *h / *hs: down_attn[0][0]'s B-row output.
static int unet_dedup_prefix(pnpi_ctx* c, const UNetDedup& ud, int B, const half_t* ctx16, bool use_ctrl, int cur_step, half_t** h, Stats* hs) {
  const pnpi_model_config& g = c->cfg;
  const UNetW& u = c->unet;
  const int U = ud.U, H = g.sample_size, C0 = g.block_out_channels[0], oc = C0;
  half_t* x0c = palloc(c, (size_t)U * H * H * 8);
  CK(launch_nchw_f32_to_nhwc_f16(ud.lat_u, U, g.in_channels, H * H, 8, x0c, c->st));
  // pinned row sharing: the compact prefix makes the choices of the logical launch's prefix (all rows under cfg_dedup = 2, its
  // distinct latents under 1)
  UNetFlight& f = *c->fw;
  if (f.share.pin && f.share.U > 0) { f.pin_from = U; f.pin_to = g_cfg_dedup == 2 ? f.share.to : f.share.U; }
  else if (g_cfg_dedup == 2) { f.pin_from = U; f.pin_to = B; }
  half_t* hc = palloc(c, (size_t)U * H * H * C0);
  Stats hcs, rcs;
  CK(op_conv(c, x0c, 8, nullptr, 0, U, H, H, u.conv_in, 1, 1, 0, u.conv_in.b, nullptr, hc, H, H, -1, nullptr, &hcs));
  half_t* rc = palloc(c, (size_t)U * H * H * oc);
  CKP(resnet_fwd(c, u.down_res[0][0], hc, C0, nullptr, 0, U, H, H, g.norm_groups, 1e-5f, rc, hcs, Stats(), &rcs));
  half_t* o2 = palloc(c, (size_t)B * H * H * oc);
  if (self_attn_resolve(c, use_ctrl, cur_step, f.tf_index, H, H, U, false).table == ST_IDENTITY) {
    const TfDedup td{U, ud.dmap};
    CKP(transformer_fwd(c, u.down_attn[0][0], rc, B, H, H, ctx16, use_ctrl, cur_step, o2, rcs, hs, &td));   // unpins after its first half
  } else {
    // the self-attention redirects rows at this step: the prefix ends behind the ResNet, whose output and per-image GroupNorm
    // partial sums are expanded to the rows of the launch
    f.pin_base();
    if (((size_t)H * H * oc) % 8) return fail(c, PNPI_ESHAPE, "cfg_dedup: row size is no multiple of 8 halfs");
    half_t* o = palloc(c, (size_t)B * H * H * oc);
    CK(launch_gather_rows_f16(rc, ud.dmap, B, (size_t)H * H * oc, o, c->st));
    Stats os;
    if (rcs.p && rcs.rows > 0 && (H * H) % rcs.rows == 0) {
      float* sp = stats_alloc(c, B * H * H, oc);
      CK(launch_gather_rows_f32(rcs.p, ud.dmap, B, (size_t)(H * H / rcs.rows) * oc * 2, sp, c->st));
      os.p = sp; os.rows = rcs.rows;
    }
    CKP(transformer_fwd(c, u.down_attn[0][0], o, B, H, H, ctx16, use_ctrl, cur_step, o2, os, hs));
  }
  f.pin_base();
  c->ctr.unet_dedup_prefix_rows += f.share.U > U ? f.share.U : U;      // under row sharing: the logical latents served (a mirrored full launch runs them all)
  *h = o2;
  return 0;
}

// UNet2DConditionModel.forward (my_diffusers/models/unet_2d_condition.py:189-273): the one forward `k` describes
static int unet_fwd(pnpi_ctx* c, const UNetCall& k) {
  const pnpi_model_config& g = c->cfg;
  const UNetW& u = c->unet;
  const int rows = k.rows, t = k.t, cur_step = k.cur_step;
  const bool use_ctrl = k.use_ctrl; const UNetDedup* ud = k.dedup;
  if (rows <= 0 || rows > c->max_rows) return fail(c, PNPI_EINVAL, "unet rows out of range (max_unet_rows)");
  if (!k.temb_row && (t < 0 || t >= g.n_train_timesteps)) return fail(c, PNPI_EINVAL, "timestep out of range");
  if (k.record && (!c->tape || k.cached_kv)) return fail(c, PNPI_ESTATE, "a recording forward needs the context's tape and projects its own text K/V");
  UNetFlight fw(k.share);
  fw.cached_kv = k.cached_kv; fw.record = k.record; fw.bias_eff = c->bias_scratch;
  if (k.pnp) fw.pnp = *k.pnp;
  const PnpState& pnp = fw.pnp;
  FlightScope in_flight(c, &fw);      // the only place a forward's state is attached to the context, and where it ends
  c->persist.reset(); c->temp.reset();
  const int S = g.sample_size, n = g.n_blocks, C0 = g.block_out_channels[0], G = g.norm_groups;
  const int B = rows;
  const float eps = 1e-5f;
  half_t* x0 = palloc(c, (size_t)B * S * S * 8);
  half_t* ctx16 = nullptr;
  if (fw.cached_kv && !c->dry) {
    if (c->tkv.rows != B) return fail(c, PNPI_ESTATE, "text K/V cache holds a different row count than this forward");
  } else {
    ctx16 = palloc(c, (size_t)B * g.ctx_len * g.cross_dim);
  }
  if (taping(c)) { c->tape->no_grad_input = x0; c->tape->ctx16 = ctx16; }
  if (!c->dry) {
    CK(launch_nchw_f32_to_nhwc_f16(k.latents, B, g.in_channels, S * S, 8, x0, c->st));
    if (ctx16) {
      if (!k.context) return fail(c, PNPI_EINVAL, "context is NULL and no text K/V cache is active");
      CK(launch_f32_to_f16(k.context, (size_t)B * g.ctx_len * g.cross_dim, ctx16, c->st));
    }
    // conv1 bias + time embedding of every ResNet for this timestep: a function of t and the weights only -> computed on the first
    // forward at t, then read from the table (not for a caller's row)
    const bool cached = !k.temb_row && c->bias_tab && g_temb_cache;
    float* row = cached ? c->bias_tab + (size_t)t * u.temb_total : (k.temb_row && k.bias_row) ? k.bias_row : c->bias_scratch;
    if (!cached || !c->bias_valid[t]) CKP(temb_bias_row(c, k.temb_row ? k.temb_row : c->temb_table + (size_t)t * C0, row));
    if (cached) c->bias_valid[t] = 1;
    fw.bias_eff = row;
  }
  // unet_dedup_prefix: no recording forward (the tape walks full-row records), host callback or sizing dry run (which sizes for both paths)
  bool dedup = ud && g_cfg_dedup && !c->dry && ud->U > 0 && ud->U < rows && g.block_has_attn[0] && !fw.record && !c->attn_cb &&
               ud->lat_u && ud->hmap && ud->dmap && !pnp.on;      // the Plug-and-Play layout [source, x, x] redirects rows: never deduplicated
  if (pnp.on && (fw.share.U > 0 || fw.record || c->attn_cb || use_ctrl || rows != 3 * pnp.nimg))
    return fail(c, PNPI_ESTATE, "Plug-and-Play forward: three rows per image, no src_share, tape, host callback or controller");
  for (int r = 0; dedup && r < rows; ++r) dedup = ud->hmap[r] >= 0 && ud->hmap[r] < ud->U;
  struct Act { half_t* p; int C, H; Stats s; };
  std::vector<Act> skips;
  int H = S;
  half_t* h = palloc(c, (size_t)B * H * H * C0);
  Stats hs_;   // GroupNorm partial sums travelling with h
  CK(op_conv(c, x0, 8, nullptr, 0, B, H, H, u.conv_in, 1, 1, 0, u.conv_in.b, nullptr, h, H, H, -1, nullptr, &hs_));
  int ch = C0;
  skips.push_back({h, ch, H, hs_});      // the first skip tensor holds every row: conv_in (K = 72) runs on both row sets
  if (c->dry && g.block_has_attn[0]) {   // what the deduplicated prefix keeps next to the plain path's tensors, at its upper bound U = B
    const size_t px = (size_t)B * S * S;
    (void)palloc(c, px * 8); (void)palloc(c, px * C0); (void)palloc(c, px * g.block_out_channels[0]); (void)palloc(c, px * g.block_out_channels[0]);
    for (int k = 0; k < 5; ++k) (void)stats_alloc(c, (int)px, g.block_out_channels[0] > C0 ? g.block_out_channels[0] : C0);
  }
  for (int i = 0; i < n; ++i) {
    const int oc = g.block_out_channels[i];
    for (int j = 0; j < g.layers_per_block; ++j) {
      if (dedup && i == 0 && j == 0) {      // down_res[0][0] and down_attn[0][0], their text-independent part on the distinct latents
        CKP(unet_dedup_prefix(c, *ud, B, ctx16, use_ctrl, cur_step, &h, &hs_));
        ch = oc;
        skips.push_back({h, ch, H, hs_});
        continue;
      }
      half_t* o = palloc(c, (size_t)B * H * H * oc);
      CKP(resnet_fwd(c, u.down_res[i][j], h, ch, nullptr, 0, B, H, H, G, eps, o, hs_, Stats(), &hs_));
      h = o; ch = oc;
      if (g.block_has_attn[i]) CKP(unet_transformer(c, u.down_attn[i][j], &h, B, H, oc, ctx16, use_ctrl, cur_step, &hs_));
      skips.push_back({h, ch, H, hs_});
    }
    if (i != n - 1) {
      const int Ho = H / 2;
      half_t* o = palloc(c, (size_t)B * Ho * Ho * oc);
      CK(op_conv(c, h, ch, nullptr, 0, B, H, H, u.down_samp[i], 2, 1, 0, u.down_samp[i].b, nullptr, o, Ho, Ho, -1, nullptr, &hs_));
      h = o; H = Ho;
      skips.push_back({h, ch, H, hs_});
    }
  }
  {
    half_t* o = palloc(c, (size_t)B * H * H * ch);
    CKP(resnet_fwd(c, u.mid_res[0], h, ch, nullptr, 0, B, H, H, G, eps, o, hs_, Stats(), &hs_));
    CKP(unet_transformer(c, u.mid_attn, &o, B, H, ch, ctx16, use_ctrl, cur_step, &hs_));
    half_t* o3 = palloc(c, (size_t)B * H * H * ch);
    CKP(resnet_fwd(c, u.mid_res[1], o, ch, nullptr, 0, B, H, H, G, eps, o3, hs_, Stats(), &hs_));
    h = o3;
  }
  for (int i = 0; i < n; ++i) {
    const int oc = g.block_out_channels[n - 1 - i];
    for (int j = 0; j <= g.layers_per_block; ++j) {
      Act s = skips.back(); skips.pop_back();
      half_t* o = palloc(c, (size_t)B * H * H * oc);
      if (pnp.on && pnp.conv && fw.up_res_index == pnp.conv_site) {      // leaves no GroupNorm partial sums
        CKP(resnet_fwd_pnp(c, u.up_res[i][j], h, ch, s.p, s.C, B, H, H, G, eps, o, hs_, s.s));
        hs_ = Stats();
      } else CKP(resnet_fwd(c, u.up_res[i][j], h, ch, s.p, s.C, B, H, H, G, eps, o, hs_, s.s, &hs_));
      fw.up_res_index++;
      h = o; ch = oc;
      if (g.block_has_attn[n - 1 - i]) CKP(unet_transformer(c, u.up_attn[i][j], &h, B, H, oc, ctx16, use_ctrl, cur_step, &hs_));
    }
    if (i != n - 1) {
      const int Ho = H * 2;
      half_t* o = palloc(c, (size_t)B * Ho * Ho * oc);
      CK(op_conv(c, h, ch, nullptr, 0, B, H, H, u.up_samp[i], 1, 1, 1, u.up_samp[i].b, nullptr, o, Ho, Ho, -1, nullptr, &hs_));
      h = o; H = Ho;
    }
  }
  half_t* gno = palloc(c, (size_t)B * H * H * ch);
  CK(op_gn(c, h, nullptr, ch, 0, B, H * H, u.norm_out, G, eps, 1, gno, hs_));
  {
    VtOut v; v.outT = k.eps_out; v.col0 = 0; v.ld = H * H; v.f32 = 1; v.rpb = H * H;
    CK(op_conv(c, gno, ch, nullptr, 0, B, H, H, u.conv_out, 1, 1, 0, u.conv_out.b, nullptr, nullptr, H, H, -1, &v));
  }
  c->ctr.unet_calls += c->dry ? 0 : 1;
  c->ctr.unet_sample_forwards += c->dry ? 0 : rows;
  c->ctr.unet_sample_forwards_cached_kv += (c->dry || !fw.cached_kv) ? 0 : rows;
  if (c->persist.overflow || c->temp.overflow) return fail(c, PNPI_ENOMEM, "workspace overflow");
  return 0;
}
