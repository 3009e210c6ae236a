// api_lpips.inc -- part of api.hip (one translation unit: included there behind api_structdist.inc; not compiled on its own).
// LPIPS with the SqueezeNet backbone (evaluation/matrics_calculator.py:324-342 -> torchmetrics >= 1.0
// LearnedPerceptualImagePatchSimilarity(net_type = "squeeze")): torchvision's squeezenet1_1().features 0 .. 12 attached to a context,
// the metric's preprocessing in the first convolution, the seven taps and the fused tap distance.  What it shares with the attached
// ViTs (attach sequence, free, refusals) is in api_vit.inc; a context that never calls pnpi_lpips_attach is unchanged.
// ---------------------------------------------------------------------------------------------------- the network's shape
static constexpr int LP_FIRES = 8, LP_TAPS = 7;
static const int kLpFeature[LP_FIRES] = {3, 4, 6, 7, 9, 10, 11, 12};      // index in squeezenet1_1().features
static const int kLpIn[LP_FIRES] = {64, 128, 128, 256, 256, 384, 384, 512};
static const int kLpSqueeze[LP_FIRES] = {16, 16, 32, 32, 48, 48, 64, 64};
static const int kLpExpand[LP_FIRES] = {64, 64, 128, 128, 192, 192, 256, 256};      // each of expand1x1 / expand3x3
static const int kLpTapFire[LP_TAPS] = {-1, 1, 3, 4, 5, 6, 7};             // tap 0 is features.1; tap k > 0 the output of this Fire block
static const int kLpTapC[LP_TAPS] = {64, 128, 256, 384, 384, 512, 512};
static bool lp_pool_before(int fire) { return fire == 0 || fire == 2 || fire == 4; }      // features.2, 5, 8
// map side of every tap at image side S; false: a pool has no valid window (S < 17)
static bool lpips_tap_sides(int S, int* side) {
  int H = lpips_conv1_out(S);
  side[0] = H;
  for (int f = 0, t = 1; f < LP_FIRES; ++f) {
    if (lp_pool_before(f)) H = maxpool3s2_ceil_out(H);
    if (H <= 0) return false;
    if (t < LP_TAPS && kLpTapFire[t] == f) side[t++] = H;
  }
  return side[0] > 0;
}

// ---------------------------------------------------------------------------------------------------- attach / free
static void lpips_free(pnpi_ctx* c) {
  LpipsW* v = c->lpips;
  if (!v) return;
  tower_free(c, v);
  delete v;
  c->lpips = nullptr;
}
// torchvision's keys under "lpips.": features.0.{weight,bias}, features.N.{squeeze,expand1x1,expand3x3}.{weight,bias}; lin{k}.weight
static void lpips_build(pnpi_ctx* c) {
  LpipsW* v = c->lpips;
  v->w0 = walloc_h(c, 64 * 27);
  reg_mat(c, "lpips.features.0.weight", v->w0, 64, 3, 9, 27, 3);      // [64][3][3][3] -> (ky, kx, c) columns, no channel padding
  v->b0 = walloc_f(c, 64);
  reg_vec(c, "lpips.features.0.bias", v->b0, 64);
  for (int f = 0; f < LP_FIRES; ++f) {
    const std::string pre = "lpips.features." + std::to_string(kLpFeature[f]);
    v->fire[f].squeeze = make_conv(c, pre + ".squeeze", kLpIn[f], kLpSqueeze[f], 1);
    v->fire[f].expand1 = make_conv(c, pre + ".expand1x1", kLpSqueeze[f], kLpExpand[f], 1);
    v->fire[f].expand3 = make_conv(c, pre + ".expand3x3", kLpSqueeze[f], kLpExpand[f], 3);
  }
  for (int k = 0; k < LP_TAPS; ++k) {
    v->lin[k] = walloc_f(c, kLpTapC[k]);
    reg_vec(c, "lpips.lin" + std::to_string(k) + ".weight", v->lin[k], kLpTapC[k]);      // [1][C][1][1]
  }
}
static void lpips_bufs(pnpi_ctx*, Bump&) {}      // none: the taps live in the forward's workspace

// features 0 .. 12 over n + n2 images (img2: the gt images of pnpi_lpips behind the pred images -- one pass over both); tap[k]: the
// fp16 NHWC map of tap k in the persistent workspace, [n + n2][side[k]^2][kLpTapC[k]], until the next forward resets it
static int lpips_fwd(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, const uint8_t* img2, const uint8_t* mask2, int n2, int S,
                     half_t** tap, const int* side) {
  LpipsW* v = c->lpips;
  const int nt = n + n2;
  TowerWorkspace ws(c, v);
  // every convolution (M = nt x pixels) takes the tile / split-K of its max_images form: an image's features do not depend on the batch it is in
  UNetFlight pin{UNetShare()};
  pin.pin_from = nt; pin.pin_to = v->max_images;
  FlightScope fs(c, &pin);
  c->persist.reset(); c->temp.reset();
  int H = side[0], t = 1;
  half_t* x = palloc(c, (size_t)nt * H * H * 64);
  tap[0] = x;
  if (!c->dry) {
    CK(launch_lpips_conv1(img, mask, n, S, v->w0, v->b0, x, c->st));
    if (n2) CK(launch_lpips_conv1(img2, mask2, n2, S, v->w0, v->b0, x + (size_t)n * H * H * 64, c->st));
  }
  for (int f = 0; f < LP_FIRES; ++f) {
    const FireW& F = v->fire[f];
    const int Cin = kLpIn[f], Cs = kLpSqueeze[f], E = kLpExpand[f];
    if (lp_pool_before(f)) {
      const int Ho = maxpool3s2_ceil_out(H);
      half_t* y = palloc(c, (size_t)nt * Ho * Ho * Cin);
      if (!c->dry) CK(launch_maxpool3s2_ceil(x, nt, H, Cin, y, c->st));
      x = y; H = Ho;
    }
    const size_t M = (size_t)nt * H * H, mk = c->temp.mark();
    half_t* s = talloc(c, M * Cs);
    CK(op_conv(c, x, Cin, nullptr, 0, nt, H, H, F.squeeze, 1, 0, 0, F.squeeze.b, nullptr, s, H, H));
    if (!c->dry) CK(launch_relu_f16(s, M * Cs, c->st));
    half_t* y = palloc(c, M * 2 * E);      // cat(expand1x1, expand3x3) on the channels: the two convolutions write its halves
    CK(op_conv(c, s, Cs, nullptr, 0, nt, H, H, F.expand1, 1, 0, 0, F.expand1.b, nullptr, y, H, H, -1, nullptr, nullptr, 2 * E));
    CK(op_conv(c, s, Cs, nullptr, 0, nt, H, H, F.expand3, 1, 1, 0, F.expand3.b, nullptr, y + E, H, H, -1, nullptr, nullptr, 2 * E));
    if (!c->dry) CK(launch_relu_f16(y, M * 2 * E, c->st));
    c->temp.release(mk);
    x = y;
    if (t < LP_TAPS && kLpTapFire[t] == f) tap[t++] = x;
  }
  if (c->persist.overflow || c->temp.overflow) return fail(c, PNPI_ENOMEM, "workspace overflow (LPIPS SqueezeNet)");
  return 0;
}
static int lpips_dry_fwd(pnpi_ctx* c) {
  half_t* tap[LP_TAPS];
  int side[LP_TAPS];
  lpips_tap_sides(c->lpips->sized_S, side);
  return lpips_fwd(c, nullptr, nullptr, c->lpips->max_images, nullptr, nullptr, 0, c->lpips->sized_S, tap, side);
}
// the network runs at the image's own side: the workspaces follow the largest side seen (allocations only, no launch)
static int lpips_reserve(pnpi_ctx* c, int S) {
  LpipsW* v = c->lpips;
  if (S <= v->sized_S) return 0;
  CKH(hipStreamSynchronize(c->st));
  v->sized_S = S;
  const int r = tower_size_workspaces(c, v, "pnpi_lpips: ", lpips_dry_fwd);
  if (r) {      // nothing usable is left: the next call sizes again
    (void)hipFree(v->persist.base); (void)hipFree(v->temp.base);
    v->persist = Bump(); v->temp = Bump();
    v->sized_S = 0;
  }
  return r;
}
// per-workgroup partial sums of the tap distance, grown on demand (no launch)
static int lpips_scratch(pnpi_ctx* c, int n, int HW) {
  const size_t need = lpips_layer_scratch_floats(n, HW);
  if (need <= c->lp_ws_floats) return 0;
  CKH(hipStreamSynchronize(c->st));
  (void)hipFree(c->lp_ws); c->lp_ws = nullptr; c->lp_ws_floats = 0;
  CKH(hipMalloc((void**)&c->lp_ws, need * sizeof(float)));
  c->lp_ws_floats = need;
  return 0;
}

// ---------------------------------------------------------------------------------------------------- refusals (all before a launch)
static int lpips_check_attached(pnpi_ctx* c) {
  if (!c->lpips) return fail(c, PNPI_ESTATE, "no LPIPS network attached to this context (pnpi_lpips_attach)");
  return 0;
}
static int lpips_check_images(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int nmax, int S, const char* what) {
  if (!img) { c->err = std::string(what) + " is NULL"; return PNPI_EINVAL; }
  if (n <= 0 || n > nmax) return fail(c, PNPI_EINVAL, "n out of range: 1 .. max_pairs pairs, 1 .. 2 * max_pairs images of pnpi_lpips_attach");
  if (S < 17 || S > 8192) return fail(c, PNPI_ESHAPE, "unsupported image side: square S with 17 <= S <= 8192 (below 17 the third max pool has no window)");
  if (mask) CKP(check_mask01(c, mask, (size_t)n * S * S));
  return 0;
}

// ---------------------------------------------------------------------------------------------------- C ABI
extern "C" {

int pnpi_lpips_attach(pnpi_ctx* c, int max_pairs) {
  if (!c) return PNPI_EINVAL;
  if (c->lpips) return fail(c, PNPI_ESTATE, "pnpi_lpips_attach: an LPIPS network is already attached");
  if (max_pairs <= 0 || max_pairs > 128) return fail(c, PNPI_EINVAL, "max_pairs must be 1 .. 128");
  LpipsW* v = new LpipsW();
  v->name = "LPIPS SqueezeNet"; v->prefix = "lpips.";
  v->max_pairs = max_pairs; v->max_images = 2 * max_pairs;
  v->sized_S = 512;      // PIE-Bench's side; a larger image grows the workspaces at its first call
  c->lpips = v;
  return tower_attach(c, v, "pnpi_lpips_attach", {lpips_build, lpips_bufs, lpips_dry_fwd, lpips_free});
}

int pnpi_lpips_features(pnpi_ctx* c, const uint8_t* img, const uint8_t* mask, int n, int S, int tap_index, float* out) {
  if (!c) return PNPI_EINVAL;
  CKP(lpips_check_attached(c));
  CKP(tower_check_weights(c, c->lpips));
  if (!out) return fail(c, PNPI_EINVAL, "out_f32 is NULL");
  if (tap_index < 0 || tap_index >= LP_TAPS) return fail(c, PNPI_EINVAL, "tap must be 0 .. 6");
  LpipsW* v = c->lpips;
  CKP(lpips_check_images(c, img, mask, n, v->max_images, S, "img_hwc"));
  half_t* tap[LP_TAPS];
  int side[LP_TAPS];
  lpips_tap_sides(S, side);
  CKP(lpips_reserve(c, S));
  CKP(lpips_fwd(c, img, mask, n, nullptr, nullptr, 0, S, tap, side));
  CK(launch_f16_to_f32(tap[tap_index], (size_t)n * side[tap_index] * side[tap_index] * kLpTapC[tap_index], out, c->st));
  return 0;
}

int pnpi_lpips(pnpi_ctx* c, const uint8_t* img_pred, const uint8_t* mask_pred, const uint8_t* img_gt, const uint8_t* mask_gt, int n, int S,
               float* score_out) {
  if (!c) return PNPI_EINVAL;
  CKP(lpips_check_attached(c));
  CKP(tower_check_weights(c, c->lpips));
  if (!score_out) return fail(c, PNPI_EINVAL, "score_out is NULL");
  CKP(lpips_check_images(c, img_pred, mask_pred, n, c->lpips->max_pairs, S, "img_pred"));
  CKP(lpips_check_images(c, img_gt, mask_gt, n, c->lpips->max_pairs, S, "img_gt"));
  LpipsW* v = c->lpips;
  half_t* tap[LP_TAPS];
  int side[LP_TAPS];
  lpips_tap_sides(S, side);
  CKP(lpips_reserve(c, S));
  CKP(lpips_scratch(c, n, side[0] * side[0]));
  CKP(lpips_fwd(c, img_pred, mask_pred, n, img_gt, mask_gt, n, S, tap, side));
  for (int k = 0; k < LP_TAPS; ++k) {
    const int HW = side[k] * side[k], C = kLpTapC[k];
    const half_t* a = tap[k];
    const half_t* b = tap[k] + (size_t)n * HW * C;
    CK(launch_lpips_layer(a, b, v->lin[k], n, HW, C, c->lp_ws, score_out, k > 0, c->st));      // tap 0 writes, the others add: one stream, one order
  }
  return 0;
}

int pnpi_op_lpips_layer(pnpi_ctx* c, const void* a, const void* b, const float* w, int n, int HW, int C, float* out) {
  if (!c) return PNPI_EINVAL;
  if (!a || !b || !w) return fail(c, PNPI_EINVAL, "a_f16 / b_f16 / w is NULL");
  if (!out) return fail(c, PNPI_EINVAL, "out is NULL");
  if (n <= 0 || n > 65535 || HW <= 0 || HW > (1 << 26)) return fail(c, PNPI_EINVAL, "n must be 1 .. 65535, HW 1 .. 2^26");
  if (C <= 0 || C % 8) return fail(c, PNPI_ESHAPE, "C must be a positive multiple of 8");
  if (((uintptr_t)a | (uintptr_t)b) & 15) return fail(c, PNPI_EINVAL, "the feature maps must be 16-byte aligned");
  CKP(lpips_scratch(c, n, HW));
  CK(launch_lpips_layer((const half_t*)a, (const half_t*)b, w, n, HW, C, c->lp_ws, out, 0, c->st));
  return 0;
}

int pnpi_op_maxpool3s2_ceil(pnpi_ctx* c, const void* x, int n, int H, int C, void* out) {
  if (!c) return PNPI_EINVAL;
  if (!x || !out) return fail(c, PNPI_EINVAL, "x_f16 / out_f16 is NULL");
  if (n <= 0 || H < 2 || H > 8192) return fail(c, PNPI_ESHAPE, "n must be positive, H 2 .. 8192 (a 3 x 3 ceil-mode window needs two rows)");
  if (C <= 0 || C % 8) return fail(c, PNPI_ESHAPE, "C must be a positive multiple of 8");
  if (((uintptr_t)x | (uintptr_t)out) & 15) return fail(c, PNPI_EINVAL, "the maps must be 16-byte aligned");
  CK(launch_maxpool3s2_ceil((const half_t*)x, n, H, C, (half_t*)out, c->st));
  return 0;
}

}  // extern "C"
