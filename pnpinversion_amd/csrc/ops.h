// Host-side launch wrappers for the gfx950 kernels (internal C++ interface; the public boundary is include/pnpi.h).
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------
// Implicit-GEMM convolution / linear:  out[m][n] = alpha * sum_k A(m,k) * W[n][k] + bias[n] (+ res[m][n])
//   A(m,k): NHWC gather from up to two concatenated sources (x1: channels [0,C1), x2: [C1,C1+C2)); m=(b,yo,xo),
//   k=(tap,c) with tap=(r,s) for 3x3; optional nearest-2x upsample folded into the address map; zero padding.
//   W: [N][K] fp16, K = ksize*ksize*(C1+C2), tap-major (KRSC).
// Columns n >= vt_col0 are written transposed per batch item into outT (fp16 or fp32):
//   outT[(b*(N-vt_col0) + (n-vt_col0))*vt_ld + (m % rows_per_batch)]   -- used for V^T (attention) and NCHW fp32 outputs.
// ---------------------------------------------------------------------------------------------------------------
struct GemmP {
  const half_t* x1; const half_t* x2;
  int C1, C2, ldx1, ldx2;
  int B, H, W, Ho, Wo;
  int ksize, stride, pad, ups;
  const half_t* w; int ldw;
  int M, N, K;
  const float* bias;
  const half_t* res; int ldres;
  float alpha;
  half_t* out; int ldo;
  void* outT; int vt_col0, vt_ld, vt_f32, rows_per_batch;
  int vt_perm16;   // transposed columns: token t of each aligned 16-token group is stored at position vt_perm16_pos(t) (see below)
  float* slab; int splitk, kchunks_per_split;
  float* stats;   // optional: per (m-tile, channel) sum / sum-of-squares of the fp16 output, [gridDim.x][N][2] (GroupNorm fusion)
  int geglu;      // N columns are [x(32) | gate(32)] interleaved groups; output has N/2 columns: x * gelu(gate)
  int epi_lds;    // set by launch_igemm: coalesced LDS-staged epilogue is applicable
  int bias_init;  // set by launch_igemm: the LDS-DMA kernel starts its accumulators at the bias (alpha == 1, no split-K) and its epilogue adds none
  int res_late;   // set by launch_igemm: the LDS epilogue adds the residual in its store loop instead of staging it
  int k_order;    // set by launch_igemm for the ping-pong kernel: 1 = 3 x 3 convolutions walk k channel-slab-major (nine taps per 64-channel slab in a row)
  int gx, gy, gz, tile_order;   // set by the launcher: logical tile grid and XCD-aware traversal order (see igemm_dma_kernel)
  // nbatch > 1: the launch holds nbatch independent problems of the same shape (grid z = problem index; no split-K): problem z reads
  // x1 + z * sx1, w + z * sw and writes out + z * sout (elements) / outT + z * soutT (bytes).  The attention backward's per-head GEMMs.
  int nbatch;
  long sx1, sw, sout, soutT;
};
void gemm_defaults(GemmP& p);
// ws: fp32 scratch for split-K slabs (ws_bytes available). force_cfg: -1 auto, 0 = 128x128, 1 = 64x64, 2 = 64x64 split-K.
// stats_tile_rows (out): rows per m-tile of the p.stats partials actually produced, 0 if this launch produced none
// sel_M > 0: the configuration is chosen as for sel_M rows instead of p.M (bit-identical per element to the sel_M-row launch's rows)
int launch_igemm(GemmP p, float* ws, size_t ws_bytes, hipStream_t st, int force_cfg = -1, int force_split = 0,
                 int* cfg_used = nullptr, int* stats_tile_rows = nullptr, int sel_M = 0);
// What launch_igemm decides before it launches, as plain integers (igemm_plan: a pure host function of the launch description and the
// tuning knobs; pnpi_igemm_plan_query hands it to the CPU tests).  err: 0, or launch_igemm's -2 ... -10 (id -1: rejected before a tile
// was chosen; stats_tile_rows -1: rejected before the statistics were decided).
struct IgemmPlan {
  int err, id, split, kchunks_per_split;
  int variant, sparse;      // the tile's tuning variant (ids 0 / 1: ring depth folded in; ping-pong: igemm_vpp); 2 / 1 / 0: at most one / two / more blocks per CU
  int bm, bn, gx, gy, gz;
  int vt_col0;              // clamped to N
  int epi_lds, bias_init, res_late, k_order;   // the GemmP fields of the same names
  int stats, stats_tile_rows, cls;             // requested statistics survive; rows per partial (0: none); cfg_used class
  int dma, fastk;           // LDS-DMA kernel families (0: the register-staged v1 kernel, with FASTK = fastk)
  int instance;             // the kernel instance that runs: an index for igemm_instance_info (-1: err before one was chosen)
};
IgemmPlan igemm_plan(GemmP p, bool have_ws, size_t ws_bytes, int force_cfg, int force_split, int sel_M);
int igemm_init();  // sets dynamic-LDS attributes once
// row `index` of the kernel instance table: name ("dma<128,128,32,8>", "pp<192,320>", "v1<64,64,fast>"), the seven geometry integers
// igemm_last_launch reports for it, whether it exists in a `build --ablations` library only (each nullable); -1 past the end; host only
int igemm_instance_info(int index, const char** name, int* geom7, int* ablation_only);
// tile configuration id / split-K of the most recent launch_igemm and the geometry of its instance: igemm_dma_kernel's <BM, BN, BKT, NST,
// WGM, ABL, WK>; igemm_pp_kernel's <BM, BN, MI0, NI0, ABL>, 0, -1; all 0 for the v1 kernel (profiling)
void igemm_last_launch(int* cfg, int* split, int* geom7);
// measured tile table: 1 = exact {M, N, K, ksize} entry, 2 = the same layer at the nearest row count (<= 4x away in M), 0 = none (cost model)
int igemm_table_lookup(int M, int N, int K, int ksize, int* cfg, int* split, int* entry_m);
int igemm_pp_rowtile_query(int cfg, int M, int N, int split);   // rows of the ping-pong tile launched for (cfg 16 / 17, M, N, split); host only

// ---------------------------------------------------------------------------------------------------------------
// Normalisation / elementwise
// ---------------------------------------------------------------------------------------------------------------
// GroupNorm over NHWC (two-source concat allowed). partial: [B][nchunk][G][2] fp32 scratch.
int launch_groupnorm(const half_t* x1, const half_t* x2, int C1, int C2, int B, int HW, int G, float eps,
                     const float* gamma, const float* beta, int silu, half_t* out, float* partial, hipStream_t st);
// GroupNorm whose statistics were produced by the GEMM epilogues of the tensor's producer(s): st1/st2 are [tiles][C][2]
// per-channel partial sums with tpb1/tpb2 m-tiles per batch item.
int launch_groupnorm_fused(const half_t* x1, const half_t* x2, int C1, int C2, int B, int HW, int G, float eps,
                           const float* gamma, const float* beta, int silu, half_t* out, const float* st1, int tpb1,
                           const float* st2, int tpb2, float* scratch, hipStream_t st);
// fp32 elements of `partial` (fused = false) / `scratch` (fused = true) that launch writes at most
size_t groupnorm_scratch_floats(int C1, int C2, int B, int HW, int G, bool fused);
int launch_layernorm(const half_t* x, int M, int C, float eps, const float* gamma, const float* beta, half_t* out,
                     hipStream_t st);
int launch_geglu(const half_t* x, int M, int I, half_t* out, hipStream_t st);       // x [M][2I] -> out [M][I]
int launch_softmax_rows(half_t* x, int M, int N, int ld, hipStream_t st);            // in place, fp32 internally
int launch_softmax_rows_f32(float* x, size_t M, int N, hipStream_t st);                  // in place, [M][N] contiguous
int launch_f32_rows_to_f16_padded(const float* in, size_t M, int N, int ld, half_t* out, hipStream_t st);
int launch_gemv(const float* x, int K, const half_t* W, int N, const float* bias, const float* bias2, int silu_in,
                float* out, hipStream_t st);
// weight repack (PyTorch layouts -> fp16 KRSC / head-padded rows, fp32 vectors)
// ilv_half > 0: rows [0, ilv_half) and [ilv_half, 2*ilv_half) are interleaved in groups of 32 (GEGLU x / gate pairing)
int launch_repack_matrix(const void* src, int src_f16, int rows, int cols, int taps, half_t* dst, int dst_ld, int cin_pad,
                         int row0, int dh, int Dp, hipStream_t st, int ilv_half = 0);
int launch_repack_vec(const void* src, int src_f16, int n, float* dst, hipStream_t st, int ilv_half = 0);
// ff2 folded into proj_out: w_fo [C][5C] = [Wp W2 | Wp] (fp32 sums of the stored fp16 weights, rounded once), b_fo [C] = Wp b2 + bp.
// wp [C][ldp], w2 [C][4C]; C % 64 == 0
int launch_ff_fold_weights(const half_t* wp, int ldp, const float* bp, const half_t* w2, const float* b2, int C, half_t* w_fo, float* b_fo,
                           hipStream_t st);
int launch_nchw_f32_to_nhwc_f16(const float* in, int B, int C, int HW, int Cp, half_t* out, hipStream_t st);
int launch_f32_to_f16(const float* in, size_t n, half_t* out, hipStream_t st);
int launch_img_u8_to_nhwc(const uint8_t* img, int n, int HW, int Cp, half_t* out, hipStream_t st);
int launch_dec_to_u8(const float* nchw, int n, int HW, uint8_t* out_hwc, hipStream_t st);
int launch_scale_f32(const float* in, size_t n, float s, float* out, hipStream_t st);
int launch_gather_rows_f32(const float* in, const int* rows, int nrows, size_t row_elems, float* out, hipStream_t st);
// out row r = in row rows[r], fp16, 16-byte vectors: row_elems % 8 == 0, both pointers 16-byte aligned
int launch_gather_rows_f16(const half_t* in, const int* rows, int nrows, size_t row_elems, half_t* out, hipStream_t st);
int launch_add_rows_bcast_f16(const half_t* a, const half_t* h, const int* hrow, int nrows, size_t row_elems, half_t* out, hipStream_t st);
// CLIP text embeddings: out[m][:] = fp16(tok_emb[ids[m]] + pos_emb[m % T]); quick_gelu in place; fp16 -> fp32
int launch_embed_tokens(const int* ids, int M, int T, int H, int vocab, const half_t* tok_emb, const half_t* pos_emb, half_t* out,
                        hipStream_t st);
int launch_quick_gelu(half_t* x, size_t n, hipStream_t st);
int launch_f16_to_f32(const half_t* in, size_t n, float* out, hipStream_t st);

// ---------------------------------------------------------------------------------------------------------------
// CLIP similarity (clipscore.hip): preprocessing, token assembly, pooled-row gather, cosine score
// ---------------------------------------------------------------------------------------------------------------
// PIL Image.resize(BICUBIC) on uint8 RGB in its 22-bit fixed point: bounds [out][2] = (first source index, taps), coef [out][ksize].
// Horizontal pass: img [n][S][S][3] (* mask [n][S][S] 0 / 1, nullable) -> tmp [n][S][out][3]
int launch_clip_resize_h(const uint8_t* img, const uint8_t* mask, int n, int S, int out, const int* bounds, const int* coef, int ksize,
                         uint8_t* tmp, hipStream_t st);
// Vertical pass: tmp -> resized [n][out][out][3] (nullable) and / or the normalised pixels as fp16 patch rows patches
// [n][(out / patch)^2][Kp] in (c, ky, kx) order, columns 3 * patch^2 .. Kp zero (nullable)
int launch_clip_resize_v(const uint8_t* tmp, int n, int S, int out, const int* bounds, const int* coef, int ksize, int patch, int Kp,
                         uint8_t* resized, half_t* patches, hipStream_t st);
// x [n][NP + 1][W]: row 0 = cls + pos[0], row 1 + p = (pe[n][p] [+ bias]) + pos[1 + p] (fp32 sums, one rounding); bias nullable;
// W % 8 == 0, every row 16-byte aligned.  Both attached ViTs (api_vit.inc).
int launch_vit_assemble_tokens(const half_t* pe, const float* bias, const float* cls, const float* pos, int n, int NP, int W, half_t* x,
                               hipStream_t st);
// out [n][H] = x [n][T][H] at token 0 (ids == nullptr) or at the first position of each row's largest id (ids [n][T]); H % 8 == 0
int launch_clip_gather_rows(const half_t* x, int n, int T, int H, const int* ids, half_t* out, hipStream_t st);
// out[i] = max(100 * a_i . b_i / (|a_i| |b_i|), 0) in fp32, one wavefront per pair; a, b [n][D]
int launch_clip_cosine(const float* a, const float* b, int n, int D, float* out, hipStream_t st);

// ---------------------------------------------------------------------------------------------------------------
// DINO structure distance (structdist.hip): preprocessing, token assembly, exact GELU, the fused key self-similarity distance
// ---------------------------------------------------------------------------------------------------------------
// Two-tap bilinear resize (taps idx0 / idx1 / lam [out] from the host, PyTorch align_corners = False) of img [n][S][S][3] (* mask
// [n][S][S] 0 / 1, nullable) -> resized fp32 [n][3][out][out] in 0..255 (nullable) and / or (v - mean) / std as fp16 patch rows
// [n][(out / patch)^2][3 * patch^2] in (c, ky, kx) order (nullable); patch even
int launch_dino_preprocess(const uint8_t* img, const uint8_t* mask, int n, int S, int out, const int* idx0, const int* idx1, const float* lam,
                           int patch, float* resized, half_t* patches, hipStream_t st);
int launch_gelu_erf(half_t* x, size_t n, hipStream_t st);      // erf-form GELU in place (gelu_f); n % 8 == 0, x 16-byte aligned
// dist[p] = mean over T^2 of (sim(keys_a[p]) - sim(keys_b[p]))^2, sim[i][j] = x_i . x_j / max(|x_i| |x_j|, 1e-8); keys fp16 [n][T][D],
// D % 32 == 0, 16-byte aligned; scratch: keys_selfsim_scratch_floats(n, T) floats; dist (nullable) needs keys_b; sim_a (nullable):
// fp32 [n][T][T], the map of keys_a.  Fixed reduction order, no atomics.
size_t keys_selfsim_scratch_floats(int n, int T);
int launch_keys_selfsim_mse(const half_t* keys_a, const half_t* keys_b, int n, int T, int D, float* scratch, float* dist, float* sim_a,
                            hipStream_t st);

// ---------------------------------------------------------------------------------------------------------------
// LPIPS, SqueezeNet (lpips.hip): the first convolution with the metric's preprocessing, ceil-mode max pool, ReLU, the fused tap distance
// ---------------------------------------------------------------------------------------------------------------
// img u8 [n][S][S][3] (* mask [n][S][S] 0 / 1, nullable) -> ((u8 / 255) * mask) * 2 - 1 -> (x - shift) / scale -> 3 x 3 stride-2
// convolution (w fp16 [64][27], (ky, kx, c) columns; bias fp32 [64]; fp32 accumulation) -> ReLU -> out fp16 [n][Ho][Ho][64]
int lpips_conv1_out(int S);                 // Ho = (S - 3) / 2 + 1
int launch_lpips_conv1(const uint8_t* img, const uint8_t* mask, int n, int S, const half_t* w, const float* bias, half_t* out, hipStream_t st);
// MaxPool2d(3, stride 2, ceil_mode = True) on fp16 NHWC [n][H][H][C] -> [n][Ho][Ho][C]; C % 8 == 0, 16-byte aligned; H >= 2
int maxpool3s2_ceil_out(int H);             // 0: no valid window
int launch_maxpool3s2_ceil(const half_t* x, int n, int H, int C, half_t* out, hipStream_t st);
int launch_relu_f16(half_t* x, size_t n, hipStream_t st);      // in place; n % 8 == 0, x 16-byte aligned
// out[p] (+)= mean over HW of sum_c w_c (a_c / sqrt(1e-8 + |a|^2) - b_c / sqrt(1e-8 + |b|^2))^2; a, b fp16 [n][HW][C],
// C % 8 == 0, 16-byte aligned; w fp32 [C]; scratch: lpips_layer_scratch_floats(n, HW) floats.  Fixed reduction order, no atomics.
size_t lpips_layer_scratch_floats(int n, int HW);
int launch_lpips_layer(const half_t* a, const half_t* b, const float* w, int n, int HW, int C, float* scratch, float* out, int accumulate,
                       hipStream_t st);

// ---------------------------------------------------------------------------------------------------------------
// Attention
// ---------------------------------------------------------------------------------------------------------------
// Key order of a "permuted" V^T (GemmP::vt_perm16 / AttnP::vt_perm): inside every aligned group of 16 tokens the two middle quads are
// swapped -- stored order [0-3, 8-11, 4-7, 12-15] -- so that the 8 keys one lane feeds to the P V MFMA (accumulator rows 4h + {0..3, 8..11}
// of a 16-key step) are ONE aligned 16-byte chunk: a single conflict-free ds_read_b128 instead of two 2-way-conflicted ds_read_b64.
__host__ __device__ inline int vt_perm16_pos(int tok) { return tok ^ ((((tok >> 2) ^ (tok >> 3)) & 1) ? 12 : 0); }

struct AttnP {
  const half_t* q; int ldq, q_off;
  const half_t* k; int ldk, k_off;
  const half_t* vt; int ldv;      // Vt[((row*heads + head)*Dp + d)*ldv + tok]
  half_t* o; int ldo;             // o[(row*Nq + tok)*ldo + head*dh + d]
  int heads, Nq, Nk, Dp, dh;
  float scale;
  const int* rows;                // device [nrows][4] = {out_row, q_row, k_row, v_row}
  int nrows;
  int causal = 0;                 // 1: key j is masked for query i when j > i (CLIP text encoder)
  int vt_perm = 0;                // 1: vt is stored in the permuted key order (only the 64-wide LDS-DMA self-attention kernel reads it)
  int aug = 0;                    // 1: column d = dh of every K row and every V row (V^T row dh) holds 1.0 (the producer's bias wrote it):
                                  //    the 64-wide LDS-DMA kernel then takes the max shift and the row sum through the MFMAs (attn.hip, AUG)
  float* lse = nullptr;           // optional [out_row][heads][Nq]: log2-domain log-sum-exp of every query (recording forward of the null-text path)
};
int launch_attn_flash(const AttnP& p, hipStream_t st);
bool attn_flash_uses_dma64(int Dp, int Nk, int causal);
// Class-restricted self-attention (mask-guided MasaCtrl, models/masactrl/masactrl.py:138-193 for binary masks): query i attends only to the
// keys j with kcls[j] == qcls[i]; a query whose class no key carries attends to all keys uniformly (the reference's softmax over logits
// that all equal finfo.min).  One softmax per query; key tiles without a key of the workgroup's classes are neither loaded nor computed.
struct AttnMaskP {
  const uint8_t* kcls;            // device [nmask][Nk] 0 / 1 (non-zero reads as 1)
  const uint8_t* qcls;            // device [nmask][Nq]
  const int* mrow;                // device [nrows]: which of the nmask class rows entry r of AttnP::rows uses
};
static constexpr int ATTN_MASK_MAX_KEYS = 16384;   // the per-key class bits of one row sit in LDS
// p.vt_perm: the permuted key order is read too (the 4096-token sites' projection writes it); p.aug is harmless (column dh of Q is zero padding)
int launch_attn_flash_masked(const AttnP& p, const AttnMaskP& m, hipStream_t st);

// Flash-style attention backward (null-text path): dQ / dK / dV of softmax(scale Q K^T) V without the [N][N] matrices in memory.
struct BwdMat { const half_t* p; long hs; int ld; int w; };   // (head, row, col) -> p[head * hs + row * ld + col]; columns >= w read as zero (w % 8 == 0)
struct AttnBwdP {
  BwdMat b1, b2;                  // the workgroup's own ("block") rows, held in registers: DQ: Q, dO;  DK: K, V;  DV: K
  BwdMat l1, l2;                  // the rows it walks ("loop" side, staged in LDS):        DQ: K, V;   DK: Q, dO; DV: Q, dO
                                  // (the transposed operand of the accumulation -- K^T, Q^T, dO^T -- is made from these tiles in LDS)
  int nb, nl, heads;              // block rows, loop rows
  float scale;
  float* lse;                     // [heads][queries] log2-domain log-sum-exp: written by DQ, read by DK / DV
  float* dsum;                    // [heads][queries] sum_k P dP                   (same)
  half_t* out; long out_hs; int out_ld, out_w;   // out[head * out_hs + block_row * out_ld + d], d < out_w
  const half_t* o = nullptr; long o_hs = 0; int o_ld = 0;   // DQ only, optional: the forward's output O (head * o_hs + query * o_ld + d) -- with it
                                  // `lse` is an INPUT (the forward kernel's) and D = rowsum(dO o O): the kernel's first pass over the keys is skipped
  int nsplit = 1;                 // DK / DV with few keys (cross-attention): the loop rows are split over nsplit workgroups per (key tile, head), each
  float* part = nullptr;          // writing fp32 partial sums part[((split * heads + head) * nb + block_row) * out_w + d]; summed in order by
};                                // launch_attn_bwd_reduce
// Everything the backward of one attention site decides before it launches (api_backward.inc: attn_bwd_plan; a pure host function of the shape and
// the tuning knobs "attn_bwd_flash" / "abf_prefetch"; pnpi_attn_bwd_plan_query hands it to the CPU tests).  attn_bwd, attn_bwd_flash and
// launch_attn_bwd_flash run what it says.
struct AttnBwdPlan {
  int flash;                      // 1: attn_bwd_flash_kernel, 0: the materialised form
  int lt;                         // loop-tile rows of the flash instance (64, or 32 at Dp 160); 0: materialised
  int nsplit;                     // shares of the dK / dV query walk (> 1: fp32 partials + attn_bwd_reduce_kernel)
  int pf[3];                      // per mode (dQ, dK, dV): the PF = true instance is launched
  int one_pass;                   // dQ takes the forward's log-sum-exp and O: no first pass over the keys
  int share_rows;                 // loop rows per share of the dK / dV walk (whole tiles; Nq when it is not split)
  int empty_shares;               // shares that begin at or past Nq (their partials are zeros)
  long long scratch_bytes;        // flash: the workspace attn_bwd_flash carves; materialised: attn_bwd_scratch_bytes of one head
};
constexpr int attn_bwd_flash_lt(int Dp) { return (Dp == 32 || Dp == 64 || Dp == 96) ? 64 : Dp == 160 ? 32 : 0; }   // 0: head width not instantiated
// the loop rows of one share of a split walk: whole LT tiles (kernel and plan)
__host__ __device__ constexpr int attn_bwd_share_rows(int nl, int nsplit, int LT) { return ((nl + nsplit - 1) / nsplit + LT - 1) / LT * LT; }
// scratch_bytes: what the caller has (0: none); have_fwd: the forward's lse and O are there (O's leading dimension a multiple of 8)
AttnBwdPlan attn_bwd_plan(int heads, int Nq, int Nk, int Dp, int dh, size_t scratch_bytes, bool have_fwd);
int launch_attn_bwd_reduce(const AttnBwdP& p, hipStream_t st);
// pf: the plan's pf[mode]; -1: head width not instantiated
int launch_attn_bwd_flash(const AttnBwdP& p, int mode /*0 DQ, 1 DK, 2 DV*/, int Dp, bool pf, hipStream_t st);

// Cross-attention with the Prompt-to-Prompt edit fused in (one (src,tgt) row pair per grid.z entry).
struct CrossEditP {
  const half_t* q; int ldq, q_off;
  const half_t* k; int ldk, k_off;
  const half_t* vt; int ldv;
  half_t* o; int ldo;
  int heads, Nq, Nk, Dp, dh;
  float scale;
  const int* pairs;               // device [npairs][2] = {src_row, tgt_row}
  int npairs;
  const half_t* mmatT;            // device [npairs][96][96] fp16: mmatT[j][w] = Mmat[w][j] (zero padded)
  const float* c1; const float* c2;   // device [npairs][96] blend coefficients for the current step
  const float* lb_alpha;          // device [npairs][lb_planes][96] LocalBlend token selectors (nullable)
  float* lb_acc;                  // device [npairs][nslots][lb_planes][Nq] accumulators (nullable)
  int lb_planes = 2;              // 2: {src, tgt} blend-word selectors; 4: + {src, tgt} substruct-word selectors (LocalBlend substruct_words)
  int lb_slot0, lb_nslots;        // this layer's first slot (slot = lb_slot0 + head)
  int write_src;                  // also store the source row's output (tests); the executor leaves that to the flash kernel
};
int launch_attn_cross_edit(const CrossEditP& p, hipStream_t st);

// ---------------------------------------------------------------------------------------------------------------
// Scheduler / latent step kernels (fp32, NCHW, bit-exact w.r.t. the reference's elementwise order)
// ---------------------------------------------------------------------------------------------------------------
// x_next = sqrt(a_next) * ((x - sqrt(1-a_t) * eps) / sqrt(a_t)) + sqrt(1-a_next) * eps
int launch_ddim_move(const float* x, const float* eps, float a_from, float a_to, size_t n, float* out, hipStream_t st);
// Classifier-free guidance + DDIM denoise step (+ direct-inversion offset). See include/pnpi.h pnpi_cfg_ddim_prev.
int launch_ddim_prev_recon(const float* x, const float* eps, float a_from, float a_to, const float* ref, float lr, const float* mask, size_t n,
                           float* out, float* x0_out, hipStream_t st);
struct CfgStepP {
  const float* eps = nullptr;                                 // [nimg][2 * rows_per_img][row_elems]: per image the unconditional rows, then the conditional
  const float* x = nullptr; float* x_out = nullptr;           // [nimg][rows_per_img][row_elems] (x_out may be x)
  int nimg = 0, rows_per_img = 1; size_t row_elems = 0;
  float gscale = 1.f, a_t = 1.f, a_prev = 1.f;                // the step goes from alpha_cumprod a_t to a_prev
  const float* noise_loss = nullptr; int offset_rows = 0;     // like x: added to the first offset_rows rows of every image (ignored with a target)
  const float* target = nullptr; float offset_scale = 1.f; float* offset_out = nullptr;   // target [nimg][row_elems], offset_out like x (offset_calculate)
  const float* prox_thr = nullptr; int prox_mode = 0;         // [nimg] thresholds of the proximal step; mode 0 none, 1 l0, 2 l1
  const float *recon_ref = nullptr, *inv_ref = nullptr;       // [nimg][row_elems] reconstruction / inversion guidance: both need prox_mode and the
  float recon_lr = 0.f; int dilate = 0, lat_h = 0, lat_w = 0; // lat_h x lat_w planes of a row (dilation of the edit mask)
};
int launch_cfg_ddim_prev(const CfgStepP& p, hipStream_t st);
// threshold of the proximal-guidance step: quantile q of |eps_c - eps_u| over the rows of each image (torch.quantile, linear)
int launch_quantile_abs_diff(const float* eps, int nimg, int rows_per_img, size_t row_elems, float q, float* thr_out, hipStream_t st);
int launch_fill_f32(float* p, int n, float v, hipStream_t st);
int launch_local_blend(const float* lb_acc, int nslots, int map_hw, int lat_hw, int C, float th, float* latents,
                       int nimg, hipStream_t st, int planes = 2, float th_sub = 0.3f);   // planes 4: planes 2, 3 are the substruct maps (no pooling, th_sub)
// edit-friendly DDPM (eta > 0, stored noise maps).  sc: the 6 host scalars of ef_step_scalars [sa_t, sb_t, sa_p, dcoef, sigma, var]
void ef_step_scalars(float ab_t, float ab_p, float eta, float* out);
int launch_ef_sample_xts(const float* x0, const float* noise, const float* lev_dev, int nlev, size_t per_lev, float* xts, hipStream_t st);
int launch_ef_noise_map(const float* eps, int cfg, float g, const float* xt, float* xprev, float* z_out, int nimg, size_t E, const float* sc,
                        hipStream_t st);
int launch_ef_reverse_step(const float* eps, const float* x, const float* z, int nimg, int P, size_t E, float g0, float g1, const float* sc,
                           int add_noise, float* out, hipStream_t st);
// Blended Latent Diffusion: CFG + DDIM step + noised source + mask blend in one launch (x_out may be x); mask [nimg][HW] 0/1, E % HW == 0.
int launch_bld_step(const float* eps, const float* x, const float* src, const float* noise, const float* mask, int nimg, size_t E, size_t HW,
                    float g, float a_t, float a_prev, float* x_out, hipStream_t st);
// uint8 [n][H][W] -> fp32 0/1 [n][h][w]: PIL-nearest resize, non-zero -> 1
int launch_bld_mask(const uint8_t* in, int n, int H, int W, int h, int w, float* out, hipStream_t st);
int launch_pnp_step(const float* eps, const float* x, const float* src_next, int nimg, size_t E, float g, float a_t, float a_prev, float* x_out,
                    float* rows_next, hipStream_t st);
// InstructPix2Pix: the three denoised rows, the two-scale CFG combine and the Euler-ancestral move in one launch (z_out may be z), and the next
// launch's two distinct 8-channel inputs per image.  sc (host): [sigma, sigma_down - sigma, sigma_up]; eps == NULL: inputs only.
// combine: IP2P_CHAIN (InstructPix2Pix, third row null text + zero image) or IP2P_SYMMETRIC (InstructDiffusion, third row text + zero image)
enum { IP2P_CHAIN = 0, IP2P_SYMMETRIC = 1 };
int launch_ip2p_step(int combine, const float* eps, const float* z, const float* noise, const float* image, int nimg, size_t E, float g_text,
                     float g_image, const float* sc, int add_noise, float c_in_next, float* z_out, float* in_next, hipStream_t st);
// uint8 [n][H][W] -> uint8 0/1 [n][h][w]: F.interpolate(mode="nearest") indexing, source = min(floor(dst * (float)H / h), H - 1)
int launch_masa_mask_level(const uint8_t* in, int n, int H, int W, int h, int w, uint8_t* out, hipStream_t st);

// ---------------------------------------------------------------------------------------------------------------
// Activation-gradient kernels of the null-text path (bwd.hip)
// ---------------------------------------------------------------------------------------------------------------
int launch_layernorm_bwd(const half_t* x, const half_t* dy, int M, int C, float eps, const float* gamma, half_t* dx, hipStream_t st);
int launch_groupnorm_bwd(const half_t* x1, const half_t* x2, int C1, int C2, int B, int HW, int G, float eps, const float* gamma,
                         const float* beta, int silu, const half_t* dy, half_t* dx, hipStream_t st);
// Three chip-wide phases instead of one block per group; dx goes straight into the gradient buffers of the two concat sources
// (p == nullptr: that source needs no gradient; acc: add to what is there).  scratch: groupnorm_bwd2_scratch_floats() floats.
struct GnbOut { half_t* p; int ld; int acc; };
size_t groupnorm_bwd2_scratch_floats(int B, int HW, int G);
int launch_groupnorm_bwd2(const half_t* x1, const half_t* x2, int C1, int C2, int B, int HW, int G, float eps, const float* gamma, const float* beta,
                          int silu, const half_t* dy, GnbOut o1, GnbOut o2, float* scratch, hipStream_t st);
int launch_geglu_bwd(const half_t* h, const half_t* dy, int M, int I, half_t* dh, hipStream_t st);
int launch_softmax_bwd_rows(const float* P, const float* dP, size_t R, int N, int ld, float scale, half_t* dS, hipStream_t st);
int launch_accumulate_f16(half_t* dst, const half_t* src, size_t n, hipStream_t st);
int launch_sumpool2x2(const half_t* dup, int B, int H, int W, int C, half_t* dx, hipStream_t st);
int launch_zero_stuff2(const half_t* dy, int B, int Ho, int Wo, int C, half_t* out, hipStream_t st);
int launch_repack_dgrad(const half_t* w, int N, int Npad, int taps, int Cin, half_t* wd, hipStream_t st);
int launch_strided_add_f16(half_t* dst, const half_t* src, int ld, int off, size_t R, int C, int accumulate, hipStream_t st);
int launch_add_f16_to_f32(float* dst, const half_t* src, size_t n, float scale, hipStream_t st);
int launch_null_text_loss(const float* eps_u, const float* eps_c, const float* x, const float* target, int n, float w, float c_x, float c_e,
                          float grad_scale, float* d_eps_u, float* loss, hipStream_t st);
int launch_adam_step(float* p, float* m, float* v, const float* g, int n, int k, float lr, float inv_scale, hipStream_t st);
int launch_pad_heads_f16(const half_t* src, size_t R, int heads, int dh, int Dp, half_t* dst, hipStream_t st);
int launch_transpose_f16(const half_t* src, int ld_src, int R, int Cc, half_t* dst, int ld_dst, hipStream_t st, int nbatch = 1, long s_src = 0,
                         long s_dst = 0);   // nbatch matrices, s_src / s_dst elements apart
