// api_vit.inc -- part of api.hip (one translation unit: included there ahead of api_clipscore.inc, api_structdist.inc and api_lpips.inc;
// not compiled on its own).  What the networks attached to a context share (TowerW, model.h): the scopes that lend the context's
// helpers the tower's arenas, free, the refusals and the attach sequence; and what the vision transformers share on top (VitTowerW):
// the geometry, the identity row table and the token assembly.  What is particular to a tower -- its slots, its preprocessing, its
// config rules, everything behind the last full block -- is in that tower's own file.
// ---------------------------------------------------------------------------------------------------- scopes
// the tower's weight arena takes the place of the context's: walloc_* / reg_* / make_* then place the tower's slots in it
struct TowerArena {
  pnpi_ctx* c; TowerW* t;
  TowerArena(pnpi_ctx* c_, TowerW* t_) : c(c_), t(t_) { std::swap(c->warena, t->arena); }
  ~TowerArena() { std::swap(c->warena, t->arena); }
};
// the tower's workspaces take the place of the context's for a forward (palloc / talloc / op_gemm work on c->persist / c->temp)
struct TowerWorkspace {
  pnpi_ctx* c; TowerW* t;
  TowerWorkspace(pnpi_ctx* c_, TowerW* t_) : c(c_), t(t_) { std::swap(c->persist, t->persist); std::swap(c->temp, t->temp); }
  ~TowerWorkspace() { std::swap(c->persist, t->persist); std::swap(c->temp, t->temp); }
};

// ---------------------------------------------------------------------------------------------------- free, refusals
// the four allocations and the slots; the tower's own free goes on with its tables and deletes it
static void tower_free(pnpi_ctx* c, TowerW* t) {
  void* bases[] = {t->arena.base, t->persist.base, t->temp.base, t->bufs.base};
  for (void* b : bases) (void)hipFree(b);
  const size_t np = strlen(t->prefix);
  for (auto it = c->slots.begin(); it != c->slots.end();) {
    if (it->first.compare(0, np, t->prefix) == 0) it = c->slots.erase(it); else ++it;
  }
}
static int tower_check_weights(pnpi_ctx* c, const TowerW* t) {
  const size_t np = strlen(t->prefix);
  std::vector<std::string> miss;
  for (auto& kv : c->slots)
    if (!kv.second.loaded && kv.first.compare(0, np, t->prefix) == 0) miss.push_back(kv.first);
  if (miss.empty()) return 0;
  std::sort(miss.begin(), miss.end());
  c->err = std::string(t->name) + " weights not loaded (" + std::to_string(miss.size()) + "):";
  for (const std::string& m : miss) {
    if (c->err.size() + m.size() > 3800) { c->err += " ..."; break; }
    c->err += " " + m;
  }
  return PNPI_ESTATE;
}
// img * mask is a keep / clear choice only for 0 / 1: read the masks back and look
static int check_mask01(pnpi_ctx* c, const uint8_t* mask, size_t nbytes) {
  c->host_stage.resize(nbytes);
  CKH(hipStreamSynchronize(c->st));
  CKH(hipMemcpy(c->host_stage.data(), mask, nbytes, hipMemcpyDefault));
  for (size_t i = 0; i < nbytes; ++i)
    if ((unsigned char)c->host_stage[i] > 1) return fail(c, PNPI_EINVAL, "mask_hw holds a value other than 0 / 1");
  return 0;
}

// ---------------------------------------------------------------------------------------------------- attach
// The tower's parts of the sequence below.  The context already points at the tower when they run.
struct TowerParts {
  void (*build)(pnpi_ctx*);            // allocate and register the weight slots (runs twice under TowerArena: measure, then place)
  void (*bufs)(pnpi_ctx*, Bump&);      // allocate the tower's small buffers (runs twice likewise)
  int (*dry_fwd)(pnpi_ctx*);           // the forward at max_images; it runs under DryScope and sizes the workspaces
  void (*free_tower)(pnpi_ctx*);       // the tower's own free: leaves the context without a tower
  int (*fill_bufs)(pnpi_ctx*, TowerW*) = nullptr;      // write the small buffers once they are placed (nullable); != 0: "copy failed"
};
// measure-then-allocate of the two activation workspaces by a dry run of the forward (no launch, counters untouched); what they held is
// freed first.  On failure the tower is left as it is: the caller frees it.
static int tower_size_workspaces(pnpi_ctx* c, TowerW* t, const std::string& at, int (*dry_fwd)(pnpi_ctx*)) {
  (void)hipFree(t->persist.base); (void)hipFree(t->temp.base);
  const pnpi_counters saved = c->ctr;
  t->persist = Bump(); t->temp = Bump();
  const int r = [&]() { DryScope dry(c); return dry_fwd(c); }();
  c->ctr = saved;
  if (r) return r;
  const size_t pb = align_up(t->persist.peak + (1 << 20), 4096), tb = align_up(t->temp.peak + (1 << 20), 4096);
  t->persist = Bump(); t->temp = Bump();
  if (hipMalloc((void**)&t->persist.base, pb) != hipSuccess) { c->err = at + "workspace allocation failed"; return PNPI_ENOMEM; }
  t->persist.cap = pb;
  if (hipMalloc((void**)&t->temp.base, tb) != hipSuccess) { c->err = at + "workspace allocation failed"; return PNPI_ENOMEM; }
  t->temp.cap = tb;
  return 0;
}
// t: a new tower the context points at, validated config, name / prefix / max_images set.  api: the entry point's name, for messages.
// Every failure goes through the tower's free.
static int tower_attach(pnpi_ctx* c, TowerW* t, const char* api, const TowerParts& parts) {
  auto bail = [&](int status, const std::string& what) { parts.free_tower(c); c->err = what; return status; };
  const std::string at = std::string(api) + ": ";
  // weights: pass 1 measures, pass 2 places
  { TowerArena a(c, t); parts.build(c); }
  const size_t wbytes = align_up(t->arena.peak + 4096, 4096);
  t->arena = Bump();
  if (hipMalloc((void**)&t->arena.base, wbytes) != hipSuccess) return bail(PNPI_ENOMEM, at + "weight allocation failed");
  t->arena.cap = wbytes;
  if (hipMemsetAsync(t->arena.base, 0, wbytes, c->st) != hipSuccess) return bail(PNPI_EHIP, at + "memset failed");      // the pad columns of the patch embedding
  { TowerArena a(c, t); parts.build(c); }
  // small persistent buffers, the same two passes
  for (int pass = 0; pass < 2; ++pass) {
    Bump& b = t->bufs;
    b.reset();
    parts.bufs(c, b);
    if (pass == 0) {
      const size_t nb = align_up(b.peak + 256, 4096);
      b = Bump();
      if (hipMalloc((void**)&b.base, nb) != hipSuccess) return bail(PNPI_ENOMEM, at + "buffer allocation failed");
      b.cap = nb;
    }
  }
  if (parts.fill_bufs && parts.fill_bufs(c, t)) return bail(PNPI_EHIP, at + "copy failed");
  // workspaces: a dry run of the forward at max_images sizes them
  if (const int r = tower_size_workspaces(c, t, at, parts.dry_fwd)) return bail(r, std::string(c->err));
  if (hipStreamSynchronize(c->st) != hipSuccess) return bail(PNPI_EHIP, at + "synchronize failed");
  return 0;
}

// ---------------------------------------------------------------------------------------------------- the ViTs' part
// first in a ViT's bufs: the identity row table [max_images][4] of clip_encoder_layer
static void vit_bufs(VitTowerW* t, Bump& b) { t->rows_ident = (int*)b.alloc((size_t)t->max_images * 4 * sizeof(int)); }
static int vit_fill_bufs(pnpi_ctx*, TowerW* tw) {
  VitTowerW* t = static_cast<VitTowerW*>(tw);
  std::vector<int> idt((size_t)t->max_images * 4);
  for (int r = 0; r < t->max_images; ++r) idt[4 * r] = idt[4 * r + 1] = idt[4 * r + 2] = idt[4 * r + 3] = r;
  return hipMemcpy(t->rows_ident, idt.data(), idt.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess;
}
// tower_attach for a ViT (W set too): the patch geometry in front, the row table filled behind the buffers
static int vit_attach(pnpi_ctx* c, VitTowerW* t, const char* api, int image_size, int patch, TowerParts parts) {
  t->G = image_size / patch; t->NP = t->G * t->G; t->T = t->NP + 1; t->K = round_up_i(3 * patch * patch, 64);
  parts.fill_bufs = vit_fill_bufs;
  return tower_attach(c, t, api, parts);
}

// ---------------------------------------------------------------------------------------------------- forward prologue
// patch rows [n * NP][K] -> tokens dst [n][T][W]: the stride-p convolution as a bias-free GEMM over the patch rows (pad columns zero in
// both operands) into temp, then cls | pe (+ b_patch) + pos.  patch_gemm_flops: what the profiler books for the GEMM, < 0 for op_gemm's own figure.
static int vit_tokens(pnpi_ctx* c, const VitTowerW* t, const half_t* patches, int n, double patch_gemm_flops, half_t* dst) {
  const size_t mk = c->temp.mark();
  half_t* pe = talloc(c, (size_t)n * t->NP * t->W);
  CK(op_gemm(c, patches, t->K, n * t->NP, t->K, t->w_patch, t->K, t->W, nullptr, nullptr, 0, pe, t->W, 1.f, nullptr, patch_gemm_flops));
  if (!c->dry) CK(launch_vit_assemble_tokens(pe, t->b_patch, t->cls, t->pos, n, t->NP, t->W, dst, c->st));
  c->temp.release(mk);
  return 0;
}
