// api_backward.inc -- part of api.hip (one translation unit: included there, in this order; not compiled on its own).
// attention backward of one site, and the reverse walk over the activation tape (null-text path): gradient w.r.t. the unconditional embedding
// ---------------------------------------------------------------------------------------------------- tape backward
// Attention backward, materialised per (row, head) like the call-back path's forward (first version: generic GEMM launches and
// transposes; a fused flash backward replaces it later).  q / k: [B*N][ld] views with the head's columns at off + h * Dp (pad columns
// dh .. Dp are zero, as the forward guarantees); v: plain [B*Nk][ldvp] with the same head layout; d_o: [B*Nq][ldo], heads * dh wide.
// Outputs dq / dk / dv in the layout of q / k / v (their pad columns are left untouched: clear the buffers first).
//   S = scale q k^T, P = softmax(S);  dV = P^T dO;  dP = dO V^T;  dS = scale P (dP - rowsum(dP P));  dQ = dS K;  dK = dS^T Q.
// scratch: Nq * Nk * 8 (S / P and dP, fp32) + 2 * Nq * ldp * 2 (P, dS as fp16) + 2 * Nk * ldq8 * 2 (their transposes) + dh * (ldp + 2 * ldq8) * 2
// bytes (K^T, Q^T, dO^T), reused for every (row, head).
static size_t attn_bwd_scratch_bytes(int Nq, int Nk, int dh) {
  const size_t ldp = round_up_i(Nk, 8), ldq8 = round_up_i(Nq, 8);
  return align_up((size_t)Nq * Nk * 4, 256) * 2 + align_up((size_t)Nq * ldp * 2, 256) * 2 + align_up((size_t)Nk * ldq8 * 2, 256) * 2 +
         align_up((size_t)dh * ldp * 2, 256) + align_up((size_t)dh * ldq8 * 2, 256) * 2;
}
static int attn_bwd_materialized(pnpi_ctx* c, const half_t* q, int ldq, int q_off, const half_t* k, int ldk, int k_off, const half_t* v, int ldvp,
                                 int v_off, const half_t* d_o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, int B,
                                 half_t* dq, half_t* dk, half_t* dv, void* scratch, size_t scratch_bytes) {
  const size_t per = attn_bwd_scratch_bytes(Nq, Nk, dh);
  if (!scratch || scratch_bytes < per) return fail(c, PNPI_ENOMEM, "attention backward scratch too small");
  if ((dh & 7) || (ldq & 7) || (ldk & 7) || (ldvp & 7) || (ldo & 7)) return fail(c, PNPI_ESHAPE, "attention backward: extents must be multiples of 8");
  const int ldp = round_up_i(Nk, 8), ldq8 = round_up_i(Nq, 8);
  // The heads of a row are independent problems of one shape: every step below is ONE launch over a group of `nb` heads (as many as
  // the scratch holds; all of them with the tape's own scratch) -- a batched GEMM (grid z = head) or a row-wise kernel over nb * Nq rows.
  // Head by head the same work was 13 launches of a few microseconds each per head: 3 300 launches per reverse walk.
  const int nb_max = (int)std::min<size_t>((size_t)heads, scratch_bytes / per);
  const size_t szS = align_up((size_t)Nq * Nk * 4, 256), szP = align_up((size_t)Nq * ldp * 2, 256), szT = align_up((size_t)Nk * ldq8 * 2, 256),
               szK = align_up((size_t)dh * ldp * 2, 256), szQ = align_up((size_t)dh * ldq8 * 2, 256);
  for (int b = 0; b < B; ++b)
    for (int h0 = 0; h0 < heads; h0 += nb_max) {
      const int nb = std::min(nb_max, heads - h0);
      char* sp = (char*)scratch;
      auto take = [&](size_t bytes_each) { char* r = sp; sp += bytes_each * nb; return r; };     // [nb] consecutive per-head buffers
      float* S = (float*)take(szS);
      float* dP = (float*)take(szS);
      half_t* P16 = (half_t*)take(szP);
      half_t* dS16 = (half_t*)take(szP);
      half_t* PT = (half_t*)take(szT);
      half_t* dST = (half_t*)take(szT);
      half_t* Kt = (half_t*)take(szK);
      half_t* Qt = (half_t*)take(szQ);
      half_t* dOt = (half_t*)take(szQ);
      const long eS = (long)(szS / 4), eP = (long)(szP / 2), eT = (long)(szT / 2), eK = (long)(szK / 2), eQ = (long)(szQ / 2);   // per-head strides in elements
      const half_t* qh = q + (size_t)b * Nq * ldq + q_off + h0 * Dp;
      const half_t* kh = k + (size_t)b * Nk * ldk + k_off + h0 * Dp;
      const half_t* vh = v + (size_t)b * Nk * ldvp + v_off + h0 * Dp;
      const half_t* doh = d_o + (size_t)b * Nq * ldo + h0 * dh;
      GemmBatch gb; gb.n = nb;
      VtOut vs; vs.outT = S; vs.col0 = 0; vs.ld = Nk; vs.f32 = 1; vs.rpb = Nk;            // S[q][key] = scale * sum_d k[key][d] q[q][d]
      gb.sa = Dp; gb.sw = Dp; gb.sout = 0; gb.soutT = (long)szS;
      CK(op_gemm(c, kh, ldk, Nk, dh, qh, ldq, Nq, nullptr, nullptr, 0, nullptr, Nq, scale, &vs, -1.0, 0, &gb));
      VtOut vp; vp.outT = dP; vp.col0 = 0; vp.ld = Nk; vp.f32 = 1; vp.rpb = Nk;          // dP[q][key] = sum_d v[key][d] dO[q][d]
      gb.sa = Dp; gb.sw = dh;
      CK(op_gemm(c, vh, ldvp, Nk, dh, doh, ldo, Nq, nullptr, nullptr, 0, nullptr, Nq, 1.f, &vp, -1.0, 0, &gb));
      if (szS == (size_t)Nq * Nk * 4 && szP == (size_t)Nq * ldp * 2) {
        // the per-head buffers are dense: the row-wise kernels take all nb * Nq rows at once
        CK(launch_softmax_rows_f32(S, (size_t)nb * Nq, Nk, c->st));
        CK(launch_f32_rows_to_f16_padded(S, (size_t)nb * Nq, Nk, ldp, P16, c->st));
        CK(launch_softmax_bwd_rows(S, dP, (size_t)nb * Nq, Nk, ldp, scale, dS16, c->st));
      } else {
        for (int i = 0; i < nb; ++i) {
          CK(launch_softmax_rows_f32(S + i * eS, (size_t)Nq, Nk, c->st));
          CK(launch_f32_rows_to_f16_padded(S + i * eS, (size_t)Nq, Nk, ldp, P16 + i * eP, c->st));
          CK(launch_softmax_bwd_rows(S + i * eS, dP + i * eS, (size_t)Nq, Nk, ldp, scale, dS16 + i * eP, c->st));
        }
      }
      CK(launch_transpose_f16(P16, ldp, Nq, Nk, PT, ldq8, c->st, nb, eP, eT));
      CK(launch_transpose_f16(dS16, ldp, Nq, Nk, dST, ldq8, c->st, nb, eP, eT));
      CK(launch_transpose_f16(kh, ldk, Nk, dh, Kt, ldp, c->st, nb, Dp, eK));
      CK(launch_transpose_f16(qh, ldq, Nq, dh, Qt, ldq8, c->st, nb, Dp, eQ));
      CK(launch_transpose_f16(doh, ldo, Nq, dh, dOt, ldq8, c->st, nb, dh, eQ));
      gb.soutT = 0; gb.sout = Dp;
      gb.sa = eP; gb.sw = eK;
      CK(op_gemm(c, dS16, ldp, Nq, ldp, Kt, ldp, dh, nullptr, nullptr, 0, dq + (size_t)b * Nq * ldq + q_off + h0 * Dp, ldq, 1.f, nullptr, -1.0, 0, &gb));     // dQ = dS K
      gb.sa = eT; gb.sw = eQ;
      CK(op_gemm(c, dST, ldq8, Nk, ldq8, Qt, ldq8, dh, nullptr, nullptr, 0, dk + (size_t)b * Nk * ldk + k_off + h0 * Dp, ldk, 1.f, nullptr, -1.0, 0, &gb));   // dK = dS^T Q
      CK(op_gemm(c, PT, ldq8, Nk, ldq8, dOt, ldq8, dh, nullptr, nullptr, 0, dv + (size_t)b * Nk * ldvp + v_off + h0 * Dp, ldvp, 1.f, nullptr, -1.0, 0, &gb)); // dV = P^T dO
    }
  return 0;
}
// Attention backward in flash form (attn.hip: attn_bwd_flash_kernel): one launch each for dQ (which also leaves D, and the per-query
// log-sum-exp unless the forward did), dK and dV.  Workspace per batch row: 2 * heads * N floats (+ the fp32 partial sums of a split
// cross-attention walk) -- at the 64 x 64 level 260 KB against the 8.6 GB-per-8-heads of the score matrices.
// cross-attention (77 keys): dK / dV have one 128-row key tile per head, so the query walk is split over workgroups (fp32 partial sums,
// added in a fixed order by a small reduce launch)
static int attn_bwd_flash_nsplit(int Nq, int Nk) {
  if (Nk > 128 || Nq < 256) return 1;
  const int n = Nq / 128;
  return n > 32 ? 32 : n;
}
// The one place that decides how an attention backward runs (ops.h AttnBwdPlan).  Pure: the shape, the scratch the caller has and the knobs
//   "attn_bwd_flash": 0 = the materialised form everywhere, 1 = flash form for self- and cross-attention (dQ with the forward's
//   log-sum-exp where the tape has it), 2 = the same with the two-pass dQ always, 3 = self-attention only;
//   "abf_prefetch": 0 = never the register-prefetch instances.
AttnBwdPlan attn_bwd_plan(int heads, int Nq, int Nk, int Dp, int dh, size_t scratch_bytes, bool have_fwd) {
  AttnBwdPlan pl{};
  pl.nsplit = 1; pl.share_rows = Nq;
  pl.scratch_bytes = (long long)attn_bwd_scratch_bytes(Nq, Nk, dh);
  const bool self = Nq == Nk, cross = !self && Nk <= 128 && Nk >= 8;
  const int lt = attn_bwd_flash_lt(Dp);
  if (!g_attn_bwd_flash || !(self || (cross && g_attn_bwd_flash != 3))) return pl;
  if (!(Nq >= 64 && Nq % 64 == 0 && lt && dh <= Dp && !(dh & 7))) return pl;
  const int ns = attn_bwd_flash_nsplit(Nq, Nk);
  const size_t need = (size_t)heads * 2 * align_up((size_t)Nq * 4, 256) + (ns > 1 ? align_up((size_t)ns * heads * Nk * dh * 4, 256) : 0);
  if (scratch_bytes < need) return pl;       // the caller's workspace does not hold lse, D and the partials: materialised (which needs its own)
  pl.flash = 1; pl.lt = lt; pl.nsplit = ns; pl.scratch_bytes = (long long)need;
  pl.one_pass = have_fwd && g_attn_bwd_flash != 2;
  pl.share_rows = attn_bwd_share_rows(Nq, ns, lt);
  for (int s = 0; s < ns; ++s) pl.empty_shares += s * pl.share_rows >= Nq;
  // PF: 64- / 96-wide heads, many loop tiles per workgroup and at most ~one workgroup per CU (T workgroups of 128 block rows)
  for (int mode = 0; mode < 3; ++mode) {
    const int nb = mode ? Nk : Nq, nl = mode ? Nq : Nk, T = ((nb + 127) >> 7) * heads * (mode ? ns : 1);
    pl.pf[mode] = (Dp == 64 || Dp == 96) && g_abf_prefetch && nl >= 8 * lt && T <= 512;
  }
  return pl;
}
static int attn_bwd_flash(pnpi_ctx* c, const half_t* q, int ldq, int q_off, const half_t* k, int ldk, int k_off, const half_t* v, int ldvp,
                          int v_off, const half_t* d_o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, int B,
                          half_t* dq, half_t* dk, half_t* dv, void* scratch, const AttnBwdPlan& pl, const float* lse_fwd, const half_t* o_fwd, int ld_ofwd) {
  if ((ldq & 7) || (ldk & 7) || (ldvp & 7) || (ldo & 7) || (q_off & 7) || (k_off & 7) || (v_off & 7))
    return fail(c, PNPI_ESHAPE, "attention backward: extents must be multiples of 8");
  const size_t szF = align_up((size_t)Nq * 4, 256);
  char* sp = (char*)scratch;
  float* lse = (float*)sp; sp += szF * heads;
  float* dsum = (float*)sp; sp += szF * heads;
  float* part = (float*)sp;
  const int nsplit = pl.nsplit;
  if (szF != (size_t)Nq * 4) return fail(c, PNPI_ESHAPE, "attention backward: Nq * 4 must be a multiple of 256");   // [heads][Nq] dense (Nq >= 64, % 64 == 0 in every caller)
  for (int b = 0; b < B; ++b) {
    const half_t* qh = q + (size_t)b * Nq * ldq + q_off;
    const half_t* kh = k + (size_t)b * Nk * ldk + k_off;
    const half_t* vh = v + (size_t)b * Nk * ldvp + v_off;
    const half_t* doh = d_o + (size_t)b * Nq * ldo;
    const BwdMat mq{qh, Dp, ldq, dh}, mk{kh, Dp, ldk, dh}, mv{vh, Dp, ldvp, dh}, mdo{doh, dh, ldo, dh};
    AttnBwdP a{};
    a.heads = heads; a.scale = scale; a.lse = lse; a.dsum = dsum; a.out_hs = Dp; a.out_w = dh;
    a.b1 = mq; a.b2 = mdo; a.l1 = mk; a.l2 = mv; a.nb = Nq; a.nl = Nk;
    a.out = dq + (size_t)b * Nq * ldq + q_off; a.out_ld = ldq;
    if (pl.one_pass) {     // the recording forward left the log-sum-exp and O: dQ without its first pass over the keys
      a.lse = const_cast<float*>(lse_fwd) + (size_t)b * heads * Nq;       // read-only in this form
      a.o = o_fwd + (size_t)b * Nq * ld_ofwd; a.o_hs = dh; a.o_ld = ld_ofwd;
    }
    CK(launch_attn_bwd_flash(a, 0, Dp, pl.pf[0], c->st));
    // tile products of the three launches (dQ: S, dP, dQ -- twice S and dP without the forward's log-sum-exp; dK: S, dP, dK; dV: S, dV)
    c->ctr.executed_attn_flops += 2.0 * heads * (double)Nq * Nk * Dp * ((pl.one_pass ? 3 : 5) + 3 + 2);
    a.o = nullptr;
    a.b1 = mk; a.b2 = mv; a.l1 = mq; a.l2 = mdo; a.nb = Nk; a.nl = Nq;
    a.nsplit = nsplit; a.part = nsplit > 1 ? part : nullptr;
    a.out = dk + (size_t)b * Nk * ldk + k_off; a.out_ld = ldk;
    CK(launch_attn_bwd_flash(a, 1, Dp, pl.pf[1], c->st));
    if (nsplit > 1) CK(launch_attn_bwd_reduce(a, c->st));
    a.out = dv + (size_t)b * Nk * ldvp + v_off; a.out_ld = ldvp;
    CK(launch_attn_bwd_flash(a, 2, Dp, pl.pf[2], c->st));
    if (nsplit > 1) CK(launch_attn_bwd_reduce(a, c->st));
  }
  return 0;
}
// dq / dk / dv of one attention site: the flash form for self-attention, the materialised form otherwise
static int attn_bwd(pnpi_ctx* c, const half_t* q, int ldq, int q_off, const half_t* k, int ldk, int k_off, const half_t* v, int ldvp, int v_off,
                    const half_t* d_o, int ldo, int heads, int Nq, int Nk, int Dp, int dh, float scale, int B, half_t* dq, half_t* dk, half_t* dv,
                    void* scratch, size_t scratch_bytes, const float* lse_fwd = nullptr, const half_t* o_fwd = nullptr, int ld_ofwd = 0) {
  const AttnBwdPlan pl = attn_bwd_plan(heads, Nq, Nk, Dp, dh, scratch ? scratch_bytes : 0, lse_fwd && o_fwd && !(ld_ofwd & 7));
  if (pl.flash)
    return attn_bwd_flash(c, q, ldq, q_off, k, ldk, k_off, v, ldvp, v_off, d_o, ldo, heads, Nq, Nk, Dp, dh, scale, B, dq, dk, dv, scratch, pl,
                          lse_fwd, o_fwd, ld_ofwd);
  return attn_bwd_materialized(c, q, ldq, q_off, k, ldk, k_off, v, ldvp, v_off, d_o, ldo, heads, Nq, Nk, Dp, dh, scale, B, dq, dk, dv, scratch, scratch_bytes);
}
static int gn_bwd_workspace(pnpi_ctx* c, int B, int HW, int G, float** out) {
  const size_t need = groupnorm_bwd2_scratch_floats(B, HW, G);
  if (need > c->gn_bwd_ws_floats) {
    CKH(hipStreamSynchronize(c->st));                      // a launch in flight may still read the old buffer
    if (c->gn_bwd_ws) CKH(hipFree(c->gn_bwd_ws));
    c->gn_bwd_ws = nullptr; c->gn_bwd_ws_floats = 0;
    CKH(hipMalloc((void**)&c->gn_bwd_ws, need * sizeof(float)));
    c->gn_bwd_ws_floats = need;
  }
  *out = c->gn_bwd_ws;
  return 0;
}
static half_t* tape_galloc(pnpi_ctx* c, size_t n_halfs) {
  Tape& T = *c->tape;
  half_t* p = (half_t*)T.garena.alloc(n_halfs * sizeof(half_t));
  return T.garena.overflow ? nullptr : p;
}
// dst = the gradient buffer of activation `key` (n halfs).  First contribution: allocated, `fresh` = true, the producer writes it
// directly.  Later contributions: a scratch buffer is returned and tape_commit() adds it to the existing gradient.
struct GradDst { half_t* p = nullptr; half_t* into = nullptr; bool fresh = false; };
static int tape_target(pnpi_ctx* c, const void* key, size_t n, GradDst& d) {
  Tape& T = *c->tape;
  auto it = T.grads.find(key);
  d.p = tape_galloc(c, n);
  if (!d.p) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
  if (it == T.grads.end()) { T.grads[key] = d.p; d.fresh = true; d.into = d.p; }
  else { d.fresh = false; d.into = it->second; }
  return 0;
}
static int tape_commit(pnpi_ctx* c, const GradDst& d, size_t n) {
  if (d.fresh) return 0;
  CK(launch_accumulate_f16(d.into, d.p, n, c->st));
  return 0;
}
// gradient of `key` += src[r * ld + off + 0 .. C) for r < R (dense destination [R][C])
static int tape_add_strided(pnpi_ctx* c, const void* key, const half_t* src, int ld, int off, size_t R, int C) {
  Tape& T = *c->tape;
  auto it = T.grads.find(key);
  if (it == T.grads.end()) {
    // First contribution from a dense buffer of this backward's own arena (a dgrad result, or the finished gradient of the op's output on
    // its way into a residual branch): the buffer BECOMES the gradient -- no copy.  Safe because the walk is in reverse order: the source
    // is either fresh or the gradient of an activation whose consumers have all been processed, and later contributions are stream-ordered
    // behind this op's own reads of it.
    const char* sb = (const char*)src;
    if (ld == C && off == 0 && !T.garena.overflow && sb >= T.garena.base && sb + R * C * sizeof(half_t) <= T.garena.base + T.garena.cap) {
      T.grads[key] = const_cast<half_t*>(src);
      return 0;
    }
    half_t* p = tape_galloc(c, R * C);
    if (!p) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
    T.grads[key] = p;
    CK(launch_strided_add_f16(p, src, ld, off, R, C, 0, c->st));
  } else {
    CK(launch_strided_add_f16(it->second, src, ld, off, R, C, 1, c->st));
  }
  return 0;
}
// dgrad weights of a forward weight matrix w[N][taps][Cin] (built once per weight, kept on the device): wd[Cin][taps][Npad]
static int tape_wd(pnpi_ctx* c, const half_t* w, int N, int Npad, int taps, int Cin, const half_t** out) {
  Tape& T = *c->tape;
  auto it = T.wd.find(w);
  if (it == T.wd.end()) {
    half_t* p = nullptr;
    CKH(hipMalloc((void**)&p, (size_t)Cin * taps * Npad * sizeof(half_t)));
    CK(launch_repack_dgrad(w, N, Npad, taps, Cin, p, c->st));
    it = T.wd.emplace(w, p).first;
  }
  *out = it->second;
  return 0;
}
static int raw_conv(pnpi_ctx* c, const half_t* x, int Cx, int B, int H, int W, int ks, int pad, const half_t* w, int Nout, half_t* out) {
  GemmP p; gemm_defaults(p);
  p.x1 = x; p.C1 = Cx; p.ldx1 = Cx; p.B = B; p.H = H; p.W = W; p.Ho = H; p.Wo = W; p.ksize = ks; p.stride = 1; p.pad = pad;
  p.K = ks * ks * Cx; p.w = w; p.ldw = p.K; p.M = B * H * W; p.N = Nout; p.out = out; p.ldo = Nout;
  return igemm_prof(c, p, 2.0 * p.M * (double)p.N * p.K);
}

// Reverse walk.  d_out: gradient of the network output as NHWC fp16 with 8 channels (channels 4 .. 7 zero), consumed by conv_out's record
// (the one conv whose forward output is not an fp16 tensor).  Returns with T.d_ctx = d loss / d context (fp32, scaled like d_out).
static int tape_backward(pnpi_ctx* c, const half_t* d_out) {
  Tape& T = *c->tape;
  const pnpi_model_config& g = c->cfg;
  for (size_t oi = T.ops.size(); oi-- > 0;) {
    const TapeOp& o = T.ops[oi];
    const half_t* dy = nullptr;
    if (o.out) {
      auto it = T.grads.find(o.out);
      if (it == T.grads.end()) continue;          // nothing downstream depends on this op's output
      dy = it->second;
    } else if (o.kind == TK_CONV) {
      dy = d_out;
    } else continue;
    switch (o.kind) {
      case TK_CONV: {
        const int taps = o.cw->k * o.cw->k, Cin = o.C1 + o.C2, Ng = o.out ? o.N : 8;
        const size_t Mo = (size_t)o.B * o.Ho * o.Wo;
        if (o.res) CKP(tape_add_strided(c, o.res, dy, Ng, 0, Mo, Ng));
        if (o.x1 == T.no_grad_input) break;
        const half_t* wd = nullptr;
        CKP(tape_wd(c, o.cw->w, o.N, Ng, taps, Cin, &wd));
        const half_t* src = dy;
        int Hs = o.Ho, Ws = o.Wo;
        if (o.stride == 2) {
          half_t* z = tape_galloc(c, (size_t)o.B * 2 * o.Ho * 2 * o.Wo * Ng);
          if (!z) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
          CK(launch_zero_stuff2(dy, o.B, o.Ho, o.Wo, Ng, z, c->st));
          src = z; Hs = 2 * o.Ho; Ws = 2 * o.Wo;
        }
        half_t* dx = tape_galloc(c, (size_t)o.B * Hs * Ws * Cin);          // dense [B][Hs][Ws][C1 + C2]
        if (!dx) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
        CK(raw_conv(c, src, Ng, o.B, Hs, Ws, o.cw->k, o.cw->k == 3 ? 1 : 0, wd, Cin, dx));
        size_t Min = (size_t)o.B * Hs * Ws;
        if (o.ups) {                                                         // the conv read the 2x-upsampled map
          half_t* dd = tape_galloc(c, (size_t)o.B * o.H * o.W * Cin);
          if (!dd) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
          CK(launch_sumpool2x2(dx, o.B, o.H, o.W, Cin, dd, c->st));
          dx = dd; Min = (size_t)o.B * o.H * o.W;
        }
        CKP(tape_add_strided(c, o.x1, dx, Cin, 0, Min, o.C1));
        if (o.C2) CKP(tape_add_strided(c, o.x2, dx, Cin, o.C1, Min, o.C2));
        break;
      }
      case TK_GEMM: {
        if (o.res) CKP(tape_add_strided(c, o.res, dy, o.ldo, 0, (size_t)o.M, o.N));
        if (o.x1 == T.no_grad_input) break;
        const half_t* wt = nullptr;
        CKP(tape_wd(c, o.w, o.N, o.N, 1, o.K, &wt));                         // W^T: [K][N]
        half_t* dx = tape_galloc(c, (size_t)o.M * o.K);
        if (!dx) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
        CK(op_gemm(c, dy, o.ldo, o.M, o.N, wt, o.N, o.K, nullptr, nullptr, 0, dx, o.K, o.alpha));
        if (o.x1 == T.ctx16) CK(launch_add_f16_to_f32(T.d_ctx, dx, (size_t)o.M * o.K, 1.f, c->st));
        else CKP(tape_add_strided(c, o.x1, dx, o.K, 0, (size_t)o.M, o.K));
        break;
      }
      case TK_GN: {
        const int C = o.C1 + o.C2;
        if (!(C & 7) && !(o.C1 & 7) && o.G <= 64 && !(o.C2 && o.x2 == o.x1)) {
          // three chip-wide phases, dx written (or added) straight into the gradient buffers of the concat sources
          const size_t R = (size_t)o.B * o.HW;
          auto dest = [&](const half_t* key, int Cw, GnbOut& out) -> int {
            if (key == T.no_grad_input) { out = GnbOut{nullptr, 0, 0}; return 0; }
            auto it = T.grads.find(key);
            if (it == T.grads.end()) {
              half_t* p = tape_galloc(c, R * Cw);
              if (!p) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
              T.grads[key] = p;
              out = GnbOut{p, Cw, 0};
            } else out = GnbOut{it->second, Cw, 1};
            return 0;
          };
          GnbOut o1{nullptr, 0, 0}, o2{nullptr, 0, 0};
          CKP(dest(o.x1, o.C1, o1));
          if (o.C2) CKP(dest(o.x2, o.C2, o2));
          float* ws = nullptr;
          CKP(gn_bwd_workspace(c, o.B, o.HW, o.G, &ws));
          CK(launch_groupnorm_bwd2(o.x1, o.x2, o.C1, o.C2, o.B, o.HW, o.G, o.eps, o.nw->g, o.nw->b, o.silu, dy, o1, o2, ws, c->st));
          break;
        }
        half_t* dx = tape_galloc(c, (size_t)o.B * o.HW * C);
        if (!dx) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
        CK(launch_groupnorm_bwd(o.x1, o.x2, o.C1, o.C2, o.B, o.HW, o.G, o.eps, o.nw->g, o.nw->b, o.silu, dy, dx, c->st));
        if (o.x1 != T.no_grad_input) CKP(tape_add_strided(c, o.x1, dx, C, 0, (size_t)o.B * o.HW, o.C1));
        if (o.C2) CKP(tape_add_strided(c, o.x2, dx, C, o.C1, (size_t)o.B * o.HW, o.C2));
        break;
      }
      case TK_LN: {
        GradDst d;
        CKP(tape_target(c, o.x1, (size_t)o.M * o.C1, d));
        CK(launch_layernorm_bwd(o.x1, dy, o.M, o.C1, o.eps, o.nw->g, d.p, c->st));
        CKP(tape_commit(c, d, (size_t)o.M * o.C1));
        break;
      }
      case TK_GEGLU: {
        GradDst d;
        CKP(tape_target(c, o.x1, (size_t)o.M * 2 * o.N, d));
        CK(launch_geglu_bwd(o.x1, dy, o.M, o.N, d.p, c->st));
        CKP(tape_commit(c, d, (size_t)o.M * 2 * o.N));
        break;
      }
      case TK_ATTN: {
        // head widths that are not a multiple of 8 (reduced test configurations only): the gradient of the attention output is
        // re-laid out with Dp-wide heads (zero pads) and the whole backward runs on the padded width -- q / k / v pads are zero
        const bool pad_dh = (o.dh & 7) != 0;
        const int dh_eff = pad_dh ? o.Dp : o.dh;
        int ldo_eff = o.ldo;
        if (pad_dh) {
          half_t* dyp = tape_galloc(c, (size_t)o.B * o.Nq * o.heads * o.Dp);
          if (!dyp) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
          CK(launch_pad_heads_f16(dy, (size_t)o.B * o.Nq, o.heads, o.dh, o.Dp, dyp, c->st));
          dy = dyp; ldo_eff = o.heads * o.Dp;
        }
        const AttnBwdPlan apl = attn_bwd_plan(o.heads, o.Nq, o.Nk, o.Dp, dh_eff, SIZE_MAX, false);      // what the form needs that the shape allows
        const size_t need = apl.flash ? (size_t)apl.scratch_bytes : (size_t)apl.scratch_bytes * (size_t)o.heads;      // materialised: every head of a row in one set of launches
        if (need > T.attn_scratch_bytes) {
          if (T.attn_scratch) CKH(hipFree(T.attn_scratch));
          T.attn_scratch = nullptr; T.attn_scratch_bytes = 0;
          CKH(hipMalloc(&T.attn_scratch, need));
          T.attn_scratch_bytes = need;
        }
        // q, k, v are column ranges of at most two projection outputs (self: one tensor; cross: q2 and kv2): their gradients are
        // assembled in buffers of the projections' shapes, zero-initialised (the head pad columns get no gradient)
        auto grad_of = [&](const half_t* base, size_t n, half_t** out) -> int {
          auto it = T.grads.find(base);
          if (it == T.grads.end()) {
            half_t* p = tape_galloc(c, n);
            if (!p) return fail(c, PNPI_ENOMEM, "gradient arena overflow");
            CKH(hipMemsetAsync(p, 0, n * sizeof(half_t), c->st));
            T.grads[base] = p; *out = p;
          } else *out = it->second;
          return 0;
        };
        half_t *gq = nullptr, *gk = nullptr, *gv = nullptr;
        CKP(grad_of(o.q, (size_t)o.B * o.Nq * o.ldq, &gq));
        CKP(grad_of(o.k, (size_t)o.B * o.Nk * o.ldk, &gk));
        CKP(grad_of(o.v, (size_t)o.B * o.Nk * o.ldv, &gv));
        // (the projection outputs have exactly one consumer each -- this attention -- so the kernels may overwrite, not accumulate)
        CKP(attn_bwd(c, o.q, o.ldq, o.q_off, o.k, o.ldk, o.k_off, o.v, o.ldv, o.v_off, dy, ldo_eff, o.heads, o.Nq, o.Nk, o.Dp, dh_eff,
                     o.scale, o.B, gq, gk, gv, T.attn_scratch, T.attn_scratch_bytes, pad_dh ? nullptr : o.lse, o.out, o.ldo));
        break;
      }
      default: break;
    }
  }
  (void)g;
  return T.garena.overflow ? fail(c, PNPI_ENOMEM, "gradient arena overflow") : 0;
}
