// tuning.h -- every process-wide tuning knob of the library, one row each.  tuning.hip defines the storage, seeds it from the
// environment once at load, and implements pnpi_set_tuning / pnpi_get_tuning / pnpi_tuning_info / pnpi_reset_tuning over this table;
// the launch wrappers (host code) read the ints below at launch time.  No kernel reads a knob.
//
//   X(storage, key, default, lo, hi, flags, environment variable or nullptr, ablation-only values (expression in v), description)
//
// lo..hi    accepted range: pnpi_set_tuning answers a value outside it with PNPI_EINVAL, an environment value outside it is ignored
// KNOB_BOOL the value is stored as 0 / 1;  KNOB_ENVSET the variable switches the knob to 1 by being set, whatever it holds
// ablation-only values select kernel instances that exist only in a `build --ablations` library (-DPNPI_ABLATIONS): the product
// library rejects them like out-of-range ones instead of silently timing the default kernel
#pragma once
#include <limits.h>

enum { KNOB_BOOL = 1, KNOB_ENVSET = 2 };

#define PNPI_TUNING_KNOBS(X)                                                                                                                  \
  /* UNet graph (api.hip); "ff_fold", "cfg_dedup" and "src_share" are described where they are defined (api_graph.inc) and in pnpi.h */     \
  X(g_text_kv, "text_kv", 1, INT_MIN, INT_MAX,0, nullptr, false, "0: project the text context inside every forward, as the reference does (A/B)")  \
  X(g_temb_cache, "temb_cache", 1, INT_MIN, INT_MAX,0, nullptr, false, "0: three time-embedding GEMVs per forward instead of the per-loop cache")  \
  X(g_ff_fold, "ff_fold", 1, INT_MIN, INT_MAX,0, nullptr, false, "each transformer block's ff2 and proj_out as one launch over folded weights")   \
  X(g_cfg_dedup, "cfg_dedup", 1, 0, 2, 0, "PNPI_CFG_DEDUP", false, "the text-independent UNet prefix runs once per distinct latent (2: tiles pinned, 0: off)") \
  X(g_src_share, "src_share", 1, 0, 2, 0, "PNPI_SRC_SHARE", false, "pnpi_direct_edit launches each step's identical source rows once (2: tiles pinned, 0: off)") \
  X(g_attn_aug, "attn_aug", 1, INT_MIN, INT_MAX,0, nullptr, false, "0: the 64-wide flash kernel ignores the augmented column (A/B)")               \
  X(g_vt_perm, "attn_vt_perm", 1, INT_MIN, INT_MAX,0, nullptr, false, "V^T of the 4096-token self-attention sites in the permuted key order (A/B)") \
  X(g_attn_bwd_flash, "attn_bwd_flash", 1, INT_MIN, INT_MAX,0, nullptr, false, "self-attention backward without the [N][N] matrices in memory (0: materialised everywhere, 2: two-pass dQ always, 3: self-attention only)") \
  X(g_op_attention_aug, "op_attention_aug", 0, INT_MIN, INT_MAX,0, nullptr, false, "pnpi_op_attention is handed K / V^T with 1.0 in column / row dh (kernel tests)") \
  X(g_op_gemm_vt_perm16, "op_gemm_vt_perm16", 0, INT_MIN, INT_MAX,KNOB_BOOL, nullptr, false, "pnpi_op_gemm writes its transposed columns in the permuted key order (GemmP::vt_perm16; kernel tests)") \
  X(g_op_attention_vt_perm, "op_attention_vt_perm", 0, INT_MIN, INT_MAX,0, nullptr, false, "pnpi_op_attention is handed a permuted V^T (kernel tests)") \
  X(g_gn_nofuse, "gn_nofuse", 0, INT_MIN, INT_MAX,KNOB_ENVSET, "PNPI_GN_NOFUSE", false, "1: GroupNorm always recomputes its statistics (ablation)") \
  /* GEMM / convolution tile selection (gemm.hip) */                                                                                         \
  X(g_use_dma, "igemm_dma", 1, INT_MIN, INT_MAX,0, "PNPI_IGEMM_DMA", false, "0: the register-staged v1 kernel everywhere")                         \
  X(g_var128, "igemm_v128", 2, INT_MIN, INT_MAX,0, "PNPI_IGEMM_V128", v == 11 || v == 12 || v == 15, "variant of the 128 x 128 tile")              \
  X(g_var64, "igemm_v64", 0, INT_MIN, INT_MAX,0, "PNPI_IGEMM_V64", false, "variant of the 64 x 64 tile")                                           \
  X(g_var256, "igemm_v256", 0, INT_MIN, INT_MAX,0, "PNPI_IGEMM_V256", false, "variant of the 256 x 128 tile")                                      \
  X(g_var320, "igemm_v320", 1, INT_MIN, INT_MAX,0, "PNPI_IGEMM_V320", v == 11 || v == 12 || v == 15, "variant of the 128 x 320 tile")              \
  X(g_var256n, "igemm_v256n", 1, INT_MIN, INT_MAX,0, "PNPI_IGEMM_V256N", false, "variant of the 128 x 256 tile")                                   \
  X(g_wide, "igemm_wide", 1, INT_MIN, INT_MAX,0, "PNPI_IGEMM_WIDE", false, "0: never pick the 128 x 320 / 128 x 256 tiles (ablation)")             \
  X(g_v128_bk64_tiles, "v128_bk64_tiles", 0, INT_MIN, INT_MAX,0, "PNPI_V128_BK64_TILES", false, "> 0: tile count from which the 128 x 128 kernel switches to 128-byte rows") \
  X(g_tile_order, "tile_order", -1, INT_MIN, INT_MAX,0, "PNPI_TILE_ORDER", false, ">= 0: force the XCD traversal order 0 / 1 (ablation)")          \
  X(g_force_cfg, "igemm_force_cfg", -1, INT_MIN, INT_MAX,0, nullptr, false, ">= 0: every auto-configured launch uses this tile id (tests, whole-forward A/B)") \
  X(g_force_split, "igemm_force_split", 0, INT_MIN, INT_MAX,0, nullptr, false, "> 0 with igemm_force_cfg: split-K of every auto-configured launch (sweeps)") \
  X(g_bias_init, "igemm_bias_init", 1, INT_MIN, INT_MAX,0, nullptr, false, "0: bias added in the epilogue instead of as the accumulators' initial value (ablation)") \
  X(g_sched, "igemm_sched", 0, INT_MIN, INT_MAX,0, nullptr, v != 0, "1 / 2: the hand-scheduled main loop for the one-k-group tiles")               \
  X(g_varpp, "igemm_vpp", 0, INT_MIN, INT_MAX,0, nullptr, v != 0, "ablations of the ping-pong kernel (1 no MFMAs, 2 no DMA, 3 DMA only, 4 MFMAs only: garbage, timing only)") \
  X(g_tapin, "igemm_tapin", 0, INT_MIN, INT_MAX,0, nullptr, false, "1: the ping-pong kernel walks 3 x 3 convolutions channel-slab-major (GemmP::k_order)") \
  X(g_pp_only_n, "igemm_pp_only_n", 0, INT_MIN, INT_MAX,0, nullptr, false, "> 0: the table's ping-pong entries apply only to launches with this N (< 0: to none; bisection)") \
  X(g_pp_only_k, "igemm_pp_only_k", 0, INT_MIN, INT_MAX,0, nullptr, false, "> 0: ... only to launches with this K")                                \
  X(g_pp_only_m, "igemm_pp_only_m", 0, INT_MIN, INT_MAX,0, nullptr, false, "> 0: ... only to launches with this M")                                \
  X(g_deep_rings, "igemm_deep_rings", 1, INT_MIN, INT_MAX,0, nullptr, false, "0: shallow LDS rings whatever the occupancy (A/B)")                  \
  X(g_vt_lds, "igemm_vt_lds", 1, INT_MIN, INT_MAX,0, nullptr, false, "0: transposed columns through the scalar epilogue (A/B)")                    \
  X(g_res_late, "igemm_res_late", 0, INT_MIN, INT_MAX,0, nullptr, false, "1: residual added in the store loop (fp16(fp16(acc + bias) + res)) instead of staged") \
  X(g_use_table, "igemm_table", 1, INT_MIN, INT_MAX,0, nullptr, false, "0: cost model only (no measured per-shape table)")                         \
  X(g_table_near, "igemm_table_near", 1, INT_MIN, INT_MAX,0, nullptr, false, "0: exact {M, N, K, ksize} table matches only (no nearest-row-count entry)") \
  X(g_pp_rowtile, "pp_rowtile", 1, INT_MIN, INT_MAX,KNOB_BOOL, "PNPI_PP_ROWTILE", false, "the ping-pong tile's row height follows the launched M (pp_rowtile_pick); 0: the table's tile as it stands") \
  /* GroupNorm (norm.hip) */                                                                                                                 \
  X(g_gn_inline_rows, "gn_inline_rows", 0, INT_MIN, INT_MAX,0, nullptr, false, "statistics-fused GroupNorm: one launch (finalize inside apply) up to this many B * HW rows") \
  X(g_gn_small_max, "gn_small_max", 24576, INT_MIN, INT_MAX,0, "PNPI_GN_SMALL_MAX", false, "elements per (sample, group) slice the one-launch kernel takes (lowers GN_SMALL_ELEMS only)") \
  X(g_gn_small_min, "gn_small_min", 0, INT_MIN, INT_MAX,0, "PNPI_GN_SMALL_MIN", false, "the one-launch kernel needs at least this many (sample, group) blocks") \
  X(g_gn_wide_below, "gn_wide_below", 1 << 30, INT_MIN, INT_MAX,0, "PNPI_GN_WIDE_BELOW", false, "the one-launch kernel runs 1024-thread blocks below this many blocks, 256-thread ones from it") \
  /* attention (attn.hip) */                                                                                                                 \
  X(g_attn_pipe, "attn_pipe", 0, INT_MIN, INT_MAX,0, nullptr, v != 0, "1 / 2: the half-tile software-pipelined forms of the 64-wide LDS-DMA kernel (measured slower)") \
  X(g_attn_nodma, "attn_nodma", 0, INT_MIN, INT_MAX,KNOB_ENVSET, "PNPI_ATTN_NODMA", false, "1: no launch takes the 64-wide LDS-DMA flash kernel (A/B)") \
  X(g_attn_ksq4, "attn_ksq4", 0, INT_MIN, INT_MAX,KNOB_ENVSET, "PNPI_ATTN_KSQ4", false, "1: always four k-steps in the 64-wide flash kernel (A/B)") \
  X(g_attn_noaug, "attn_noaug", 0, INT_MIN, INT_MAX,KNOB_ENVSET, "PNPI_ATTN_NOAUG", false, "1: launch_attn_flash ignores AttnP::aug (A/B)")        \
  X(g_abf_prefetch, "abf_prefetch", 1, INT_MIN, INT_MAX,0, "PNPI_ABF_PREFETCH", false, "0: the attention backward never takes the register-prefetch variant (A/B)")

#define X(var, ...) extern int var __attribute__((visibility("hidden")));
PNPI_TUNING_KNOBS(X)
#undef X
