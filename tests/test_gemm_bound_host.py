"""Where the per-element bound of tests/test_gpu_gemm_instances.py comes from, which kernel instance each of its cases runs, and what
the bound catches that the kernel suite's relative L2 does not.

Instance map.  instance_name(lib, plan) is the row of the library's instance table (kInstances, csrc/gemm.hip, through
pnpi_igemm_instance_info) that the plan query names in its `instance` field: the row launch_igemm launches, not a copy of its rules.  The
register-staged igemm_kernel<BM, BN, FASTK> is "v1<128,128,fast>", "v1<64,64,generic>", ...; the ping-pong kernel "pp<BM,BN>"; the LDS-DMA
kernel "dma<BM,BN,BKT,NST>" with ",wgm4" for the 8-wave tiles and ",kg2" / ",kg4" for the k-group tiles.  PRODUCT_INSTANCES is every
instance a product build can launch (36), written out here: the table's rows outside its ablation block have to be exactly this set, so
an instance added later fails here until it has cases; geom_of(), which reads an instance's geometry from its name, is held to the
table's own integers for each of them.  tests/test_igemm_instances_host.py holds the rules that pick a row to a recording.

Cases.  With BM x BN the tile, BKT its K step and NST its ring depth: M = BM + 2 and N = BN + 8 (one whole tile and a ragged one each way:
the weight-row and output-row clamps are live), K = c BKT with c in {1, NST - 1, NST, NST + 1} (prologue only, exactly full, drain; the
ping-pong kernel: 1 ... 4 K-tiles over its two buffers; the register-staged kernels: 1 ... 3 chunks, generic K with a part-filled last
chunk: K = 8, 72, 136).  K must be a multiple of 64 on the LDS-DMA kernels, so the BKT = 32 instances see even chunk counts only.  The
epilogues are spread over the chunk counts: (A) alpha 1, aligned bias, residual: bias as initial accumulator; (B) alpha 0.5, bias, no
residual; (C) a bias that is 4-byte but not 16-byte aligned, residual; (D) no bias, no residual; then at the second-largest K: (E) ldo = N + 4: the scalar
epilogue; (F) N = BN + 6 (N % 8 != 0, N % 4 != 0), alpha 0.5; and on four instances (G) A under igemm_bias_init = 0.  The ping-pong kernel
has no scalar epilogue (C, E, F would run on tile 0 instead): A, B, D only.  Split-K: K = 320 over 3 slices (2 + 2 + 1 chunks of 64: a
short last slice) once per tile id that takes split-K and per register-staged kernel, N % 8 == 0 (splitk_reduce_vec_kernel); once with
N = 134 (splitk_reduce_kernel).  k-group tiles also at a chunk count the groups do not divide (ids 8, 10, 11: 5, 3, 3 chunks; id 9 walks
32-deep chunks of a K % 64 == 0 range: always even, no such count exists).  The 257 ... 512-tile ring (sparse 1) once by tile count:
64 x 64 tiles at (1088, 1024).  One case per ping-pong tile at M = 2^15 + 2 (a linear layer's row index is an image coordinate), N = 8,
K = 64.  Tile ids 13, 14, 15, 18 launch instances ids 0 / 5 also reach: one case each.

The plan query takes no alpha (it assumes 1): a case with alpha != 1 reports bias_init = 1 where the launch runs with 0; bias_init_of()
applies the launcher's alpha == 1 condition.

Emulation.  emulate() accumulates in fp32 chunk by chunk in the kernel's chunk order (per k-group from zero, then the groups in ascending
order into group 0; per split-K slice from zero, slices added in order), starts at the bias where bias_init is set and otherwise adds it
after alpha * acc, adds the residual in fp32 before the one fp16 rounding (after a first rounding under igemm_res_late), and does not
round the fp32-transposed output.  Each chunk's product is torch's CPU fp32 matmul, NOT the MFMA's internal summation order: the bound
keeps a factor of two for that.

Bound.  ref = alpha sum_k a_k w_k + bias + res in float64, S = |alpha| sum_k |a_k w_k| + |bias| + |res|:

    |out - ref| <= 2^-11 |ref| + 2^-24 + kappa 2^-24 S          fp16 outputs
    |out - ref| <= kappa_t 2^-24 S                               fp32 (transposed NCHW) outputs
    |out - u gelu(g)| <= 2^-11 |u gelu(g)| + 2^-24 + kappa_g 2^-24 (S_u |gelu(g)| + 1.13 |u| S_g)      the GEGLU epilogue

kappa is measured: the smallest power of two that keeps the emulation's worst |err| / bound at or below 0.5 over every case and five
seeds (test_kappa_* assert: the value holds 0.5, half of it does not).

    kappa   =  8192   worst emulated ratio 0.499   (0.665 at 4096)
    kappa_t =    16   worst emulated ratio 0.294   (0.588 at 8)
    kappa_g = 16384   worst emulated ratio 0.449   (0.762 at 8192)

kappa is set by the fp16 rounding, not by fp32 arithmetic: where every term has one sign S = |ref| and half an ulp is up to 2^-11 |ref|, so
the 0.5 rule asks kappa 2^-24 S >= 2^-11 |ref|: 2^13.  In effect the bound is 2^-11 |ref| + 2^-11 S; an fp32 output is held to 2^-20 S,
and the GEGLU epilogue, which rounds the projection to fp16 before the product, to 2^-10 of its two slack terms.  The fp16 bound thus
catches structural mistakes (the mutants below) and would let an accumulation error thousands of fp32 ulps wide pass; accumulation
precision is held only through the fp32 outputs.

Inputs.  a ~ N(0, 1), w ~ N(0, 1 / K) as fp16 values, bias, res ~ N(0, 1); row 5 of a and row N - 3 of w (an output column of the ragged
n-tile) hold +-64 with signs chosen so that their own product cancels pair by pair (S = 4096 K against ref = bias + res, every partial
sum an exact integer); row 6 of a is zero.

Mutants (emulate(..., mutant=i)), each one mistake such a kernel can make; each exceeds the bound on at least one element of one case:
    1 last K chunk dropped for the rows of the ragged m-tile     5 alpha applied to the bias too
    2 one k term (k = K - 1) dropped in row 0                    6 the short last split-K slice added twice
    3 row M - 1 computed from row M - 2                          7 the short last split-K slice left out
    4 the ragged n-tile's bias shifted by one column             8 the short k-group's sums left out when the groups do not divide
The old criterion -- relative L2 below 2e-3 against the fp32 product on test_gemm's construction at (1000, 640, 640), alpha 0.5, bias and
residual at std 1 -- lets mutant 2 through (relative L2 3.9e-4, the unmutated emulation's own figure to three digits: one lost k term in one row is
invisible to it; mutant 3, one wrong row of 1000, reaches 1.4e-2 and the others 9.7e-2 ... 4.1e-1).  test_old_criterion_is_blind
asserts the list."""
import collections
import ctypes as C
import functools
import math

import pytest
import torch

from pnpinversion_amd import _capi

KAPPA = 8192.0
KAPPA_T = 16.0
KAPPA_G = 16384.0
SEEDS = (0, 1, 2, 3, 4)
MiB = 1 << 20
WS_BYTES = 96 * MiB                 # pnpi_create's split-K workspace for up to 12 rows
NO_VT = 1 << 30
ROW_C, ROW_Z = 5, 6                 # the constructed (+-64) and the all-zero row of a; the constructed row of w is N - 3

# ------------------------------------------------------------------------------------------------ instance map
PRODUCT_INSTANCES = frozenset([
    "v1<128,128,fast>", "v1<128,128,generic>", "v1<64,64,fast>", "v1<64,64,generic>",
    "dma<128,128,64,2>", "dma<128,128,64,3>", "dma<128,128,32,2>", "dma<128,128,32,3>", "dma<128,128,32,4>", "dma<128,128,32,8>",
    "dma<64,64,64,2>", "dma<64,64,64,3>", "dma<64,64,64,4>", "dma<64,64,64,8>", "dma<64,64,32,4>",
    "dma<256,128,32,2>", "dma<256,128,32,3>",
    "dma<128,320,32,2>", "dma<128,320,32,3>", "dma<128,320,32,5>", "dma<128,320,64,2>",
    "dma<128,256,32,2>", "dma<128,256,32,3>", "dma<128,256,32,6>", "dma<128,256,64,2>",
    "dma<256,320,64,2,wgm4>", "dma<256,256,64,2,wgm4>",
    "dma<64,64,64,2,kg4>", "dma<128,128,32,3,kg2>", "dma<128,128,64,2,kg2>", "dma<64,64,64,2,kg2>",
    "dma<64,320,32,2>",
    "pp<256,256>", "pp<192,320>", "pp<128,320>", "pp<192,256>",
])


Instance = collections.namedtuple("Instance", "name geom7 ablation_only")


@functools.lru_cache(maxsize=None)
def instance_table(lib):
    """the library's kernel instance table (kInstances through pnpi_igemm_instance_info), in index order"""
    rows, name, geom, abl = [], C.c_char_p(), (C.c_int * 7)(), C.c_int()
    while lib.pnpi_igemm_instance_info(len(rows), name, geom, abl) == 0:
        rows.append(Instance(name.value.decode(), tuple(geom), bool(abl.value)))
    return tuple(rows)


def instance_name(lib, pl):
    """the kernel instance launch_igemm runs for a plan: the row pnpi_igemm_plan.instance names"""
    assert pl.err == 0 and 0 <= pl.instance < len(instance_table(lib)), (pl.err, pl.instance)
    return instance_table(lib)[pl.instance].name


Geom = collections.namedtuple("Geom", "bm bn bkt nst wk")


def geom_of(instance):
    """tile, K step, ring depth and k-groups of an instance name (the ping-pong and register-staged kernels: 64-deep chunks, two buffers)"""
    fam, args = instance.split("<")
    args = args.rstrip(">").split(",")
    bm, bn = int(args[0]), int(args[1])
    if fam != "dma":
        return Geom(bm, bn, 64, 2, 1)
    wk = int(args[4][2:]) if len(args) > 4 and args[4].startswith("kg") else 1
    return Geom(bm, bn, int(args[2]), int(args[3]), wk)


def name_agrees_with_geom7(row):
    """what geom_of() reads from a product row's name, and the name's wgm field, against the row's seven integers (LDS-DMA: BM, BN, BKT, NST,
    WGM, ABL, WK; ping-pong: BM, BN, two quadrant counts the name does not hold, ABL, 0, -1; register-staged: all 0)"""
    g, t = geom_of(row.name), row.geom7
    if row.name.startswith("v1"):
        return t == (0,) * 7
    if row.name.startswith("pp"):
        return (g.bm, g.bn) == t[:2] and t[4:] == (0, 0, -1)
    wgm = [int(a[3:]) for a in row.name.rstrip(">").split(",")[4:] if a.startswith("wgm")]
    return (g.bm, g.bn, g.bkt, g.nst, wgm[0] if wgm else 2, 0, g.wk) == t


# ------------------------------------------------------------------------------------------------ case table
Case = collections.namedtuple("Case", "name M N K cfg split tune instance alpha bias res ldo exp_epi_lds exp_bias_init note")


def _case(instance, cfg, tune, M, N, K, epi, split=0, note=""):
    """epi: A ... G of the module docstring.  The expectations follow launch_igemm's rules: the LDS epilogue needs N % 8 == 0, ldo % 8 == 0
    and no split-K; bias_init (as the alpha-less plan query reports it) an LDS-DMA 4-wave kernel, no split-K, a 16-byte aligned bias,
    N % 4 == 0 and tuning igemm_bias_init."""
    alpha, bias, res, scalar = {"A": (1.0, "a16", True, False), "B": (0.5, "a16", False, False), "C": (1.0, "a4", True, False),
                                "D": (1.0, None, False, False), "E": (1.0, "a16", True, True), "F": (0.5, "a16", True, True),
                                "G": (1.0, "a16", True, False)}[epi]
    tune = dict(tune)
    if epi == "G":
        tune["igemm_bias_init"] = 0
    ldo = N + 4 if scalar else (N + 7) // 8 * 8 + 8
    sp = max(split, 1)
    epi_lds = int(N % 8 == 0 and ldo % 8 == 0 and sp == 1)
    dma = not instance.startswith("v1")
    bias_init = int(dma and not instance.startswith("pp") and sp == 1 and bias == "a16" and N % 4 == 0 and tune.get("igemm_bias_init", 1) == 1)
    name = "%s-%dx%dx%d-%s%s" % (instance, M, N, K, epi, "-s%d" % split if split else "")
    if cfg in (13, 14, 15, 18):
        name += "-id%d" % cfg
    return Case(name, M, N, K, cfg, split, tuple(sorted(tune.items())), instance, alpha, bias, res, ldo, epi_lds, bias_init, note)


# instance -> (tile id to force, the tuning keys that select it).  ids 0 / 1 fold the ring depth into the variant (sparse launches: 8 stages)
_REACH = [
    ("dma<128,128,32,8>", 0, {}),                                   # the default on these few-tile shapes (sparse 2)
    ("dma<128,128,32,3>", 0, {"igemm_deep_rings": 0}),              # variant 2 with sparse 0: what a full forward's large launches run
    ("dma<128,128,32,4>", 0, {"igemm_v128": 3}),                    # the 257 ... 512-tile ring, selected directly
    ("dma<128,128,32,2>", 0, {"igemm_v128": 4}),
    ("dma<128,128,64,3>", 0, {"igemm_v128": 1}),
    ("dma<128,128,64,2>", 0, {"igemm_v128": 0}),
    ("dma<64,64,64,8>", 1, {}),
    ("dma<64,64,64,3>", 1, {"igemm_deep_rings": 0}),
    ("dma<64,64,64,2>", 1, {"igemm_v64": 1}),
    ("dma<64,64,64,4>", 1, {"igemm_v64": 2}),
    ("dma<64,64,32,4>", 1, {"igemm_v64": 3}),
    ("dma<256,128,32,3>", 3, {}),
    ("dma<256,128,32,2>", 3, {"igemm_v256": 1}),
    ("dma<128,320,32,5>", 4, {}),
    ("dma<128,320,32,2>", 4, {"igemm_deep_rings": 0}),
    ("dma<128,320,32,3>", 4, {"igemm_v320": 0}),
    ("dma<128,320,64,2>", 4, {"igemm_v320": 2}),
    ("dma<128,256,32,6>", 5, {}),
    ("dma<128,256,32,2>", 5, {"igemm_deep_rings": 0}),
    ("dma<128,256,32,3>", 5, {"igemm_v256n": 0}),
    ("dma<128,256,64,2>", 5, {"igemm_v256n": 2}),
    ("dma<256,320,64,2,wgm4>", 6, {}),
    ("dma<256,256,64,2,wgm4>", 7, {}),
    ("dma<64,64,64,2,kg4>", 8, {}),
    ("dma<128,128,32,3,kg2>", 9, {}),
    ("dma<128,128,64,2,kg2>", 10, {}),
    ("dma<64,64,64,2,kg2>", 11, {}),
    ("dma<64,320,32,2>", 12, {}),
    ("pp<256,256>", 16, {}),
    ("pp<192,320>", 17, {}),
    ("pp<128,320>", 19, {}),
    ("pp<192,256>", 20, {}),
    ("v1<128,128,fast>", 0, {"igemm_dma": 0}),
    ("v1<64,64,fast>", 1, {"igemm_dma": 0}),
    ("v1<128,128,generic>", 0, {}),                                 # K % 64 != 0
    ("v1<64,64,generic>", 1, {}),
]
_NO_SPLIT_IDS = (3,)                                               # kTileDesc: splits = false


def _build_cases():
    cases, split_done = [], set()
    for instance, cfg, tune in _REACH:
        g = geom_of(instance)
        M, N = g.bm + 2, g.bn + 8                                  # one whole tile and a ragged one each way
        pp, v1 = instance.startswith("pp"), instance.startswith("v1")
        if v1 and instance.endswith("generic>"):
            ks = [8, 72, 136]                                      # 1, 2, 3 chunks, the last part-filled
        elif v1 or pp:
            ks = [64 * c for c in ((1, 2, 3, 4) if pp else (1, 2, 3))]
        else:                                                      # prologue only, NST - 1, NST, NST + 1 chunks (K % 64 == 0)
            ks = sorted(set(max(64, -(-c * g.bkt // 64) * 64) for c in (1, g.nst - 1, g.nst, g.nst + 1)))
        epis = "ABDA" if pp else "ABCD"
        for i, K in enumerate(ks):
            cases.append(_case(instance, cfg, tune, M, N, K, epis[i % 4]))
        if len(ks) < 4 and not pp:                                 # every epilogue at least once per instance
            for e in epis[len(ks):]:
                cases.append(_case(instance, cfg, tune, M, N, ks[-1], e))
        if not pp:
            kfull = ks[-2] if len(ks) > 1 else ks[-1]
            cases.append(_case(instance, cfg, tune, M, N, kfull, "E"))                    # ldo % 8 != 0: the scalar epilogue
            cases.append(_case(instance, cfg, tune, M, g.bn + 6, kfull, "F"))             # N % 8 != 0 and N % 4 != 0
        if g.wk > 1 and g.bkt == 64:                               # a chunk count the k-groups do not divide
            cases.append(_case(instance, cfg, tune, M, N, 64 * (5 if g.wk == 4 else 3), "A", note="kgroups ragged"))
        key = instance if v1 else cfg
        if cfg not in _NO_SPLIT_IDS and key not in split_done:     # 5 chunks of 64 over 3 slices: 2 + 2 + 1
            split_done.add(key)
            cases.append(_case(instance, cfg, tune, M, N, 264 if instance.endswith("generic>") else 320, "B" if pp else "A", split=3))
    for instance, cfg in (("dma<128,128,32,2>", 13), ("dma<128,128,64,2>", 14), ("dma<128,256,64,2>", 15), ("dma<128,128,64,3>", 18)):
        g = geom_of(instance)                                      # the tile ids that launch an instance ids 0 / 5 also reach
        cases.append(_case(instance, cfg, {}, g.bm + 2, g.bn + 8, 64 * g.nst, "A"))
        cases.append(_case(instance, cfg, {}, g.bm + 2, g.bn + 8, 320, "B", split=3))
    cases.append(_case("dma<128,128,32,8>", 0, {}, 130, 134, 320, "F", split=3, note="splitk_reduce_kernel"))      # N % 4 != 0 under split-K
    for instance in ("dma<128,128,32,8>", "dma<64,64,64,8>", "dma<128,320,32,5>", "dma<64,64,64,2,kg4>"):
        cfg, tune = next((c, t) for i, c, t in _REACH if i == instance)
        g = geom_of(instance)
        cases.append(_case(instance, cfg, tune, g.bm + 2, g.bn + 8, 128, "G"))            # bias in the epilogue
    cases.append(_case("dma<64,64,64,4>", 1, {}, 1088, 1024, 320, "A", note="sparse 1 by tile count: 17 x 16 = 272 tiles"))
    for instance, cfg in (("pp<256,256>", 16), ("pp<192,320>", 17), ("pp<128,320>", 19), ("pp<192,256>", 20)):
        cases.append(_case(instance, cfg, {}, (1 << 15) + 2, 8, 64, "A", note="row index beyond 2^15"))
    return cases


CASES = _build_cases()


def query_plan(lib, M, N, K, *, cfg, split=0, lda=None, ldw=None, ldo=None, bias=None, res=False, geglu=0, vt_col0=NO_VT, vt_ld=0, vt_f32=0, rpb=1,
               vt_perm16=0, ksize=1, C1=None, C2=0):
    """pnpi_igemm_plan_query under the tuning in force (the caller sets and restores it)"""
    C1 = K // (ksize * ksize) - C2 if C1 is None else C1
    d = _capi.IgemmLaunchDesc(M=M, N=N, K=K, ksize=ksize, C1=C1, C2=C2, ldx1=C1 if lda is None else lda, ldx2=C2, ldw=K if ldw is None else ldw,
                              ldo=N if ldo is None else ldo, ldres=N, bias=int(bias is not None), bias_aligned16=int(bias == "a16"), residual=int(res),
                              geglu=geglu, stats=0, vt_col0=vt_col0, vt_ld=vt_ld, vt_f32=vt_f32, rows_per_batch=rpb, vt_perm16=vt_perm16, nbatch=1,
                              ws_bytes=WS_BYTES, force_cfg=cfg, force_split=split, sel_M=0)
    pl = _capi.IgemmPlan()
    assert lib.pnpi_igemm_plan_query(d, pl) == 0
    return pl


def case_plan(lib, case):
    """the plan of a case in the poisoned layout of the GPU test (lda = K + 24, ldw = K + 8), under the case's tuning"""
    with _capi.tuning(lib, **dict(case.tune)):
        return query_plan(lib, case.M, case.N, case.K, cfg=case.cfg, split=case.split, lda=case.K + 24, ldw=case.K + 8, ldo=case.ldo, bias=case.bias,
                          res=case.res)


def check_case_plan(lib, case, pl):
    assert pl.err == 0, (case.name, pl.err)
    assert instance_name(lib, pl) == case.instance, (case.name, instance_name(lib, pl), pl.id, pl.variant, pl.sparse)
    assert pl.id == case.cfg, (case.name, pl.id)       # a forced ping-pong tile the launch is not eligible for would come back as id 0
    assert (pl.split, pl.epi_lds, pl.bias_init) == (max(case.split, 1), case.exp_epi_lds, case.exp_bias_init), (case.name, pl.split, pl.epi_lds, pl.bias_init)
    if case.split:
        nch = -(-case.K // 64)
        assert pl.kchunks_per_split * (pl.split - 1) < nch < pl.kchunks_per_split * pl.split, case.name      # a short, non-empty last slice


EmuPlan = collections.namedtuple("EmuPlan", "name split kchunks_per_split bias_init res_late")


def bias_init_of(case, pl):
    """the launcher's bias_init: the plan query's, with the alpha == 1 condition the query cannot see"""
    return int(bool(pl.bias_init) and case.alpha == 1.0)


def emu_plan(case):
    """the plan fields emulate() needs, from the case's own expectations (test_cases_reach_their_instances holds them to the plan query)"""
    sp = max(case.split, 1)
    return EmuPlan(case.instance, sp, -(-(-(-case.K // 64)) // sp), int(bool(case.exp_bias_init) and case.alpha == 1.0), 0)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K, seed=0):
    """a [M, K], w [N, K] fp16, bias [N] fp32, res [M, N] fp16 on the CPU.  Shared between tests: do not modify."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * M + 17 * N + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).half()
    sgn = torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
    alt = torch.where(torch.arange(K) % 2 == 0, 1.0, -1.0)
    if M > ROW_Z:
        a[ROW_C] = 64.0 * sgn
        a[ROW_Z] = 0.0
    if N > 3:
        w[N - 3] = 64.0 * sgn * alt                    # against a's constructed row: +4096 -4096 +4096 ..., zero over every even chunk
    return a.half(), w.half(), bias.float(), res


def ref64(a, w, bias, res, alpha):
    """-> (ref, S) float64 on the operands' device"""
    ad, wd = a.double(), w.double()
    ref = alpha * (ad @ wd.t())
    S = abs(alpha) * (ad.abs() @ wd.abs().t())
    if bias is not None:
        ref = ref + bias.double()
        S = S + bias.double().abs()
    if res is not None:
        ref = ref + res.double()
        S = S + res.double().abs()
    return ref, S


def bound_f16(ref, S, kappa=KAPPA):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -24 + kappa * 2.0 ** -24 * S


def bound_f32(ref, S, kappa=KAPPA_T):
    return kappa * 2.0 ** -24 * S


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an element with a zero bound (fp32 output of an all-zero row without bias) must be exact"""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return r.max().item()


# ------------------------------------------------------------------------------------------------ emulation
def emulate(a, w, bias, res, alpha, plan, f32_out=False, mutant=None):
    """What the kernel instance of `plan` (EmuPlan) computes, in fp32 on the CPU, in its chunk order; see the module docstring.  Each
    chunk's product is torch's fp32 matmul, not the MFMA's internal order.  mutant: one of the mistakes 1 ... 8 of the docstring."""
    g = geom_of(plan.name)
    M, K = a.shape
    N = w.shape[0]
    af, wf = a.float(), w.float()
    b = bias.float().clone() if bias is not None else None
    if mutant == 2:
        af = af.clone()
        af[0, K - 1] = 0.0
    if mutant == 3 and M > 1:
        af = af.clone()
        af[M - 1] = af[M - 2]
    if mutant == 4 and b is not None and N > g.bn:
        n_last = (N - 1) // g.bn * g.bn                # the last n-tile: the ragged one of the cases
        b[n_last:] = bias.float()[n_last - 1:N - 1]
    nch64 = -(-K // 64)
    per64 = plan.kchunks_per_split if plan.split > 1 else nch64
    sub = 64 // g.bkt                                  # kernel chunks per 64-wide chunk
    nch = -(-K // g.bkt)

    def chunk(c):
        k0, k1 = c * g.bkt, min(K, (c + 1) * g.bkt)
        p = af[:, k0:k1] @ wf[:, k0:k1].t()
        if mutant == 1 and c == nch - 1 and M > g.bm:
            p[g.bm:] = 0.0
        return p

    total = None
    for z in range(plan.split):
        kc0, kc1 = z * per64 * sub, min(nch, (z + 1) * per64 * sub)
        iters = -(-(kc1 - kc0) // g.wk)
        accs = []
        for grp in range(g.wk):
            c0 = min(kc1, kc0 + grp * iters)
            c1 = min(kc1, c0 + iters)
            acc = torch.zeros(M, N)
            if plan.bias_init and grp == 0:
                acc = acc + b
            for c in range(c0, c1):
                acc = acc + chunk(c)
            accs.append((acc, c1 - c0))
        acc = accs[0][0]
        for grp in range(1, g.wk):
            if mutant == 8 and 0 < accs[grp][1] < iters:
                continue
            acc = acc + accs[grp][0]
        short = plan.split > 1 and z == plan.split - 1 and (kc1 - kc0) < per64 * sub
        if mutant == 7 and short:
            continue
        total = acc if total is None else total + acc
        if mutant == 6 and short:
            total = total + acc
    o = total * torch.tensor(alpha, dtype=torch.float32)
    if b is not None and not plan.bias_init:
        o = o + (b * torch.tensor(alpha, dtype=torch.float32) if mutant == 5 else b)
    if res is not None:
        o = (o.half().float() if plan.res_late else o) + res.float()
    return o if f32_out else o.half()


def case_operands(case, seed=0):
    a, w, bias, res = gemm_inputs(case.M, case.N, case.K, seed)
    return a, w, (bias if case.bias else None), (res if case.res else None)


GEGLU_TILES = (0, 1, 4, 5, 6, 8, 9, 12, 13, 14, 15, 16, 17)        # the tiles tests/test_gpu_kernels.py::test_gemm_fused_geglu forces
_TILE_BM_BN = {0: (128, 128), 1: (64, 64), 4: (128, 320), 5: (128, 256), 6: (256, 320), 8: (64, 64), 9: (128, 128), 12: (64, 320), 13: (128, 128),
               14: (128, 128), 15: (128, 256), 16: (256, 256), 17: (192, 320)}


def geglu_shape(cfg):
    """M = BM + 2, N = 2 (BN + 64): one whole n-tile and a ragged one of whole [x(32) | gate(32)] groups; K = 192"""
    bm, bn = _TILE_BM_BN[cfg]
    return bm + 2, 2 * (bn + 64), 192


def ilv32(x, g):
    """[.., I] x and gate -> [.., 2 I] as [x(32) | gate(32)] groups, the layout of the fused GEGLU epilogue"""
    I = x.shape[-1]
    return torch.stack([x.reshape(*x.shape[:-1], I // 32, 32), g.reshape(*g.shape[:-1], I // 32, 32)], dim=-2).reshape(*x.shape[:-1], 2 * I)


def deilv32(h):
    """the inverse of ilv32: [.., 2 I] -> (x [.., I], gate [.., I])"""
    I = h.shape[-1] // 2
    t = h.reshape(*h.shape[:-1], I // 32, 2, 32)
    return t[..., 0, :].reshape(*h.shape[:-1], I), t[..., 1, :].reshape(*h.shape[:-1], I)


def geglu_ref64(a, w, bias):
    """a [M, K], interleaved w [2 I, K] / bias [2 I] -> (ref = u gelu(g), bound slack S_u |gelu(g)| + 1.13 |u| S_g) in float64"""
    h, S = ref64(a, w, bias, None, 1.0)
    u, g = deilv32(h)
    Su, Sg = deilv32(S)
    gl = 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))
    return u * gl, Su * gl.abs() + 1.13 * u.abs() * Sg


def bound_geglu(ref, slack, kappa=KAPPA_G):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -24 + kappa * 2.0 ** -24 * slack


def emulate_geglu(a, w, bias, instance):
    """the GEGLU epilogue: the projection rounded to fp16 once, x gelu(gate) in fp32, rounded again"""
    h = emulate(a, w, bias, None, 1.0, EmuPlan(instance, 1, -(-a.shape[1] // 64), 1, 0))
    u, g = deilv32(h.float())
    return (u * torch.nn.functional.gelu(g)).half()


# ------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def is_product_library(lib):
    """a product library refuses the tuning values that select ablation instances; a `build --ablations` one takes them"""
    try:
        with _capi.tuning(lib, igemm_vpp=1):
            return False
    except ValueError:
        return True


def test_instance_table_is_the_product_instances(lib):
    """the rows a product build can launch are PRODUCT_INSTANCES (hand-written above: a new instance fails here until it has cases), each
    row's seven integers are what its name says, and a product library holds no other row"""
    rows = instance_table(lib)
    product = [r for r in rows if not r.ablation_only]
    assert len(product) == len(PRODUCT_INSTANCES) == 36
    assert set(r.name for r in product) == PRODUCT_INSTANCES, (sorted(set(r.name for r in product) - PRODUCT_INSTANCES),
                                                                sorted(PRODUCT_INSTANCES - set(r.name for r in product)))
    for r in product:
        assert name_agrees_with_geom7(r), r
    assert rows[:len(product)] == tuple(product)                   # product rows first
    if is_product_library(lib):
        assert len(rows) == len(product), [r.name for r in rows if r.ablation_only]
    assert lib.pnpi_igemm_instance_info(len(rows), None, None, None) == _capi.PNPI_EINVAL == lib.pnpi_igemm_instance_info(-1, None, None, None)


def _plan_fields(pl):
    return (pl.err, pl.id, pl.variant, pl.sparse, pl.dma, pl.fastk, pl.split, pl.kchunks_per_split, pl.epi_lds, pl.bias_init)


def test_cases_reach_their_instances(lib):
    defaults = [_plan_fields(query_plan(lib, M, N, K, cfg=-1, bias="a16")) for M, N, K in ((130, 136, 320), (1088, 1024, 320), (194, 328, 192))]
    reached = set()
    for case in CASES:
        pl = case_plan(lib, case)
        check_case_plan(lib, case, pl)
        ep = emu_plan(case)
        assert (ep.split, ep.kchunks_per_split, ep.bias_init) == (pl.split, pl.kchunks_per_split, bias_init_of(case, pl)), case.name
        assert pl.res_late == 0
        reached.add(instance_name(lib, pl))
    assert reached == PRODUCT_INSTANCES, sorted(PRODUCT_INSTANCES - reached)
    assert len(set(c.name for c in CASES)) == len(CASES)
    assert all(c.M <= 1200 and c.N <= 1100 and c.K <= 1024 for c in CASES if not c.note.startswith("row index"))
    # case_plan left the knobs as it found them: unforced launches plan as they did before the table's tunings were set
    assert [_plan_fields(query_plan(lib, M, N, K, cfg=-1, bias="a16")) for M, N, K in ((130, 136, 320), (1088, 1024, 320), (194, 328, 192))] == defaults


def test_ping_pong_without_row_stores_falls_back_to_tile_0(lib):
    """The ping-pong kernel has no scalar epilogue (epi_select: pp_ok needs 16-byte row stores): a forced ping-pong tile whose transposed
    columns go through the scalar path (igemm_vt_lds = 0) or to fp32 plans as tile 0.  The GPU file therefore runs those two forms on
    the other families only; the fp16 LDS form stays on the ping-pong tile."""
    bm, bn, K = 192, 320, 128
    for rpb in (bm, 40):
        M, N = 3 * rpb, bn + 40
        for form, tune, col0, f32, want in (("lds", {}, bn, 0, 17), ("scalar", {"igemm_vt_lds": 0}, bn, 0, 0), ("f32", {}, 0, 1, 0)):
            with _capi.tuning(lib, **tune):
                pl = query_plan(lib, M, N, K, cfg=17, lda=K + 24, ldw=K + 8, ldo=col0 + 8 if col0 else N, bias="a16", vt_col0=col0, vt_ld=rpb + 8, vt_f32=f32,
                                rpb=rpb)
            assert (pl.err, pl.id) == (0, want), (rpb, form, pl.err, pl.id)
            assert instance_name(lib, pl) == ("pp<192,320>" if want == 17 else "dma<128,128,32,8>"), (rpb, form, instance_name(lib, pl))


def test_geglu_tiles_take_the_launch(lib):
    for cfg in GEGLU_TILES:
        M, N, K = geglu_shape(cfg)
        pl = query_plan(lib, M, N, K, cfg=cfg, lda=K + 24, ldw=K + 8, ldo=N // 2 + 8, bias="a16", geglu=1)
        assert (pl.err, pl.id, pl.epi_lds) == (0, cfg, 1), (cfg, pl.err, pl.id)


@functools.lru_cache(maxsize=None)
def _emulated_ratios():
    """worst |err| / (bound at kappa = 1's slack term), split so that any kappa can be evaluated: per case and seed the arrays would be
    large; instead -> worst ratios at (kappa, kappa / 2) for the fp16 bound and the fp32 bound"""
    out = {}
    for name, kap, f32 in (("f16", KAPPA, False), ("f32", KAPPA_T, True)):
        worst = [0.0, 0.0]
        for case in CASES:
            for seed in SEEDS:
                a, w, bias, res = case_operands(case, seed)
                ref, S = ref64(a, w, bias, res, case.alpha)
                got = emulate(a, w, bias, res, case.alpha, emu_plan(case), f32_out=f32)
                for i, k in enumerate((kap, kap / 2)):
                    bnd = bound_f32(ref, S, k) if f32 else bound_f16(ref, S, k)
                    worst[i] = max(worst[i], worst_ratio(got, ref, bnd))
        out[name] = tuple(worst)
    return out


def test_kappa_is_the_smallest_power_of_two():
    r = _emulated_ratios()
    print("kappa %g: worst emulated ratio %.3f (%.3f at %g)" % (KAPPA, r["f16"][0], r["f16"][1], KAPPA / 2))
    assert r["f16"][0] <= 0.5 < r["f16"][1], r["f16"]
    assert math.log2(KAPPA) == int(math.log2(KAPPA))


def test_kappa_t_is_the_smallest_power_of_two():
    r = _emulated_ratios()
    print("kappa_t %g: worst emulated ratio %.3f (%.3f at %g)" % (KAPPA_T, r["f32"][0], r["f32"][1], KAPPA_T / 2))
    assert r["f32"][0] <= 0.5 < r["f32"][1], r["f32"]
    assert math.log2(KAPPA_T) == int(math.log2(KAPPA_T))


def test_kappa_g_is_the_smallest_power_of_two():
    worst = [0.0, 0.0]
    for cfg in GEGLU_TILES:
        M, N, K = geglu_shape(cfg)
        instance = "dma<%d,%d,64,2>" % _TILE_BM_BN[cfg]            # one k-group, 64-deep chunks: the chunk order of every tile at K = 192
        for seed in SEEDS:
            a, w, bias, _ = gemm_inputs(M, N, K, seed)
            ref, slack = geglu_ref64(a, w, bias)
            got = emulate_geglu(a, w, bias, instance)
            for i, k in enumerate((KAPPA_G, KAPPA_G / 2)):
                worst[i] = max(worst[i], worst_ratio(got, ref, bound_geglu(ref, slack, k)))
    print("kappa_g %g: worst emulated ratio %.3f (%.3f at %g)" % (KAPPA_G, worst[0], worst[1], KAPPA_G / 2))
    assert worst[0] <= 0.5 < worst[1], worst


MUTANTS = (1, 2, 3, 4, 5, 6, 7, 8)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_breaks_the_bound(mutant):
    worst, where = 0.0, None
    for case in CASES:
        if case.M > 4096:
            continue
        a, w, bias, res = case_operands(case)
        ref, S = ref64(a, w, bias, res, case.alpha)
        r = worst_ratio(emulate(a, w, bias, res, case.alpha, emu_plan(case), mutant=mutant), ref, bound_f16(ref, S))
        if r > worst:
            worst, where = r, case.name
    print("mutant %d: worst ratio %.1f at %s" % (mutant, worst, where))
    assert worst > 1.0, (mutant, worst)


def _old_criterion(mutant):
    """test_gemm's construction at (1000, 640, 640): alpha 0.5, bias and residual at std 1, relative L2 against the fp32 product.  The
    instance is a 128 x 128 tile with 64-deep chunks; mutants 6 / 7 run it with split-K 3 (4 + 4 + 2 chunks), mutant 8 with four k-groups
    (3 + 3 + 3 + 1)"""
    M, N, K = 1000, 640, 640
    gen = torch.Generator().manual_seed

    def h16(*shape, scale=1.0, seed=0):
        return (torch.randn(*shape, generator=gen(seed)) * scale).half()

    a, w, res = h16(M, K, seed=1), h16(N, K, scale=1.0 / math.sqrt(K), seed=2), h16(M, N, seed=3)
    bias = torch.randn(N, generator=gen(4))
    if mutant in (6, 7):
        plan = EmuPlan("dma<128,128,64,2>", 3, 4, 0, 0)
    elif mutant == 8:
        plan = EmuPlan("dma<128,128,64,2,kg4>", 1, 10, 0, 0)
    else:
        plan = EmuPlan("dma<128,128,64,2>", 1, 10, 0, 0)
    out = emulate(a, w, bias, res, 0.5, plan, mutant=mutant).float()
    ref = 0.5 * (a.float() @ w.float().t()) + bias + res.float()
    return ((out - ref).norm() / ref.norm()).item()


OLD_CRITERION_LETS_THROUGH = (2,)


def test_old_criterion_is_blind():
    errs = {m: _old_criterion(m) for m in MUTANTS}
    print("relative L2 of the mutants at (1000, 640, 640): " + ", ".join("%d: %.2e" % kv for kv in errs.items()))
    assert _old_criterion(None) < 2e-3
    passed = tuple(m for m in MUTANTS if errs[m] < 2e-3)
    assert 2 in passed, errs[2]
    assert passed == OLD_CRITERION_LETS_THROUGH, errs
