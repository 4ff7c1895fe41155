"""GPU: every linear-layer GEMM kernel at its tile and pipeline edges, against the float64 references of tests/gemm_ref.py.

exact family  integer operands whose products and partial sums are exact in fp32: a correct kernel returns the exact integer (fp32) or its
              round-to-nearest-even (bf16, e4m3) whatever its summation order -- no tolerance. One dropped or doubled K element, a stale pipeline
              stage, a wrong last row of a ragged tile, a partial tile added twice or a bf16 rounding before the residual all change the result.
gauss family  N(0, 1) operands with hot K positions and cancelling rows, alpha = 0.37, against a per-element bound derived in gemm_ref.py.

Every operand is a view of a taller and wider buffer of bf16 NaNs, every output a view of a sentinel-guarded buffer (bounds_util.Guarded).
Kernels whose variants are chosen once per process from the environment run in one child process per setting, all shapes in one child.

MEASURED on the MI355X, gauss family, the worst case of each kernel. fp32 outputs: max |err| / (tol + 4 fp32 steps). bf16 outputs: the largest
fraction of tol that an element needs once half a bf16 step at the output, its own rounding, is taken off ("of tol"); their |err| reaches the
bracket's half-width (1.000) wherever the reference lies half-way between two bf16 values. The bound is a worst case over K (or R) terms and
loose by construction; no floor is asserted on these figures, the exact family is what pins the fp32 path.
  gemm_nt_kernel (BN = 64 | 128, BK = 32 | 64)       fp32 0.048, bf16 0.012 of tol; regstage 0.002, per-lane epilogue 0.002 of tol
  gemm_tn_kernel<4>      one split (atomics)         fp32 0.072, dbias 0.036
                         2 .. 12 splits (SL = 1)     fp32 0.0006, dbias 0.0002;  SL = 4 and SL = 16: below 0.0001
  gemm_tn_kernel<2>                                  fp32 0.042, dbias 0.010
  gemm_tn2_kernel                                    fp32 0.044, dbias 0.013
  gemm_tn5_kernel<3> and <2>                         fp32 0.055, dbias 0.018
  gemm_skinny_kernel<.., 4> / <.., 8>                fp32 0.0020 / 0.0002, bf16 0.000 of tol
  dec_gemm_kernel K = 768 / 3072 / NC = 1, 4         fp32 0.0008 / 0.0001 / 0.0012, bf16 0.000 of tol
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import gemm_ref as G
from attention_ref import bf16_figures
from bounds_util import Guarded
from test_kernels_gpu import _gemm_route, _gemm_variants

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _load_ops()


def _load_ops():
    from cxrmate_amd import ops as _ops
    from cxrmate_amd._lib import LIB
    LIB.load()
    return _ops


def _up8(n):
    return (n + 7) // 8 * 8


def _f32(t):
    return t.float().cuda().contiguous()


def _seed(v=4321):
    return torch.full((1,), v, dtype=torch.int32, device="cuda")


def _figure(out, ref, tol, what, kernel):
    """the gauss comparer, and the case's MEASURED line"""
    G.assert_gauss(out, ref, tol, what)
    if out.dtype == BF:
        frac, used = bf16_figures(out, ref, tol)
        print(f"MEASURED {kernel} | {what}: bf16 {frac:.4f} of the bracket, {used:.4f} of tol")
    else:
        r = float(np.max(np.abs(out.detach().cpu().double().numpy() - ref) / (tol + 4.0 * G.ulp32(ref))))
        print(f"MEASURED {kernel} | {what}: fp32 |err| / tol {r:.4f}")


# ------------------------------------------------------------------------------------------------ NT launches
def _nt_operands(ops, c, res_ld=None):
    """-> (a, w, keyword arguments of ops.gemm_nt, dropout factors | None)"""
    M, N = c["M"], c["N"]
    a, w = G.embed(c["a"], "cuda"), G.embed(c["w"], "cuda")
    kw, fac = {}, None
    if c.get("bias") is not None:
        kw["bias"] = _f32(c["bias"])
    if c.get("residual") is not None:
        kw["residual"] = G.embed(c["residual"], "cuda", ld=res_ld)
    if c.get("alpha") is not None:
        kw["alpha"] = c["alpha"]
    if c.get("row_scale") is not None:
        f, rows, after = c["row_scale"]
        kw["row_scale"] = (_f32(f), rows, after)
    if c.get("drop") is not None:
        p, site, rows_per_b, t0 = c["drop"]
        seed = _seed()
        kw["drop"] = (p, seed, site, rows_per_b, t0)
        fac = ops.dropout_mask(M, N, p, seed, site, rows_per_b, t0, factor=True).cpu().double()
        assert set(fac.unique().tolist()) <= {0.0, 2.0}
    return a, w, kw, fac


def _run_nt(ops, c, route="tiled", out_ld=None):
    """One gemm_nt launch of a case on `route` into a guarded output -> (output view, dropout factors | None)"""
    M, N = c["M"], c["N"]
    a, w, kw, fac = _nt_operands(ops, c)
    go = Guarded.rows(M, N, F32 if c["out_f32"] else BF, ld=out_ld or _up8(N) + 8)
    if c.get("out0") is not None:
        go.view.copy_(c["out0"])
    with _gemm_route(route):
        ops.gemm_nt(a, w, out=go.view, out_f32=c["out_f32"], accumulate=c.get("out0") is not None, **kw)
    go.check(f"{route} {M}x{N}x{c['K']} {c['variant']}")
    return go.view, fac


def _exact_nt(ops, M, N, K, variant="plain", route="tiled", out_ld=None, seed=0):
    c = G.exact_nt(M, N, K, variant, seed)
    out, fac = _run_nt(ops, c, route, out_ld)
    G.assert_exact(out, G.nt_reference(c, fac)[0], f"{route} {M}x{N}x{K} {variant} ld={out_ld}")


def _gauss_nt(ops, M, N, K, variant, kernel, route="tiled", out_ld=None):
    c = G.gauss_nt(M, N, K, variant)
    out, fac = _run_nt(ops, c, route, out_ld)
    ref, tol = G.gauss_nt_tol(c, fac)
    _figure(out, ref, tol, f"{M}x{N}x{K} {variant}", kernel)


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


# ------------------------------------------------------------------------------------------------ 1. gemm_nt_kernel
@pytest.mark.parametrize("M,N,K", G.TILED_BN64 + G.TILED_BN128, ids=_ids(G.TILED_BN64 + G.TILED_BN128))
def test_tiled_kernel_exact(ops, M, N, K):
    """gemm_nt_kernel<32 | 64, true, 2, 64 | 128>: 1 .. 7 K-steps, ragged row and column tiles, the N % 8 == 4 tail, one-row last tile"""
    _exact_nt(ops, M, N, K)


@pytest.mark.parametrize("M,N,K", G.TILED_BN64 + G.TILED_BN128, ids=_ids(G.TILED_BN64 + G.TILED_BN128))
def test_tiled_kernel_gauss(ops, M, N, K):
    _gauss_nt(ops, M, N, K, "bias+residual", "gemm_nt_kernel")
    _gauss_nt(ops, M, N, K, "f32+accumulate", "gemm_nt_kernel")


def test_tiled_kernel_per_lane_epilogue(ops):
    """output rows 4 mod 8 elements apart: not 16-byte aligned -> the per-lane epilogue"""
    M, N, K = G.TILED_LD4
    for variant in ("plain", "bias+residual", "f32+accumulate", "dropout+residual", "droppath after"):
        _exact_nt(ops, M, N, K, variant, out_ld=N + 8)
    _gauss_nt(ops, M, N, K, "bias+residual", "gemm_nt_kernel per-lane epilogue", out_ld=N + 8)
    assert (N + 8) % 8 == 4


@pytest.mark.parametrize("M,N,K", G.TILED_REGSTAGE, ids=_ids(G.TILED_REGSTAGE))
def test_tiled_kernel_register_staging(ops, M, N, K):
    """gemm_nt_kernel<32 | 64, false, 2, 128> (cxr_gemm_set_regstage)"""
    from cxrmate_amd._lib import LIB
    LIB.call("cxr_gemm_set_regstage", 1)
    try:
        _exact_nt(ops, M, N, K)
        _exact_nt(ops, M, N, K, "bias+residual")
        _gauss_nt(ops, M, N, K, "bias+residual", "gemm_nt_kernel regstage")
    finally:
        LIB.call("cxr_gemm_set_regstage", 0)


def _variant_names():
    """the entries of test_kernels_gpu._gemm_variants without a GELU, and this file's further ones"""
    theirs = [k for k in _gemm_variants(8, 8, 0) if "gelu" not in k]
    assert set(theirs) <= set(G.NT_VARIANTS), theirs
    return [v for v in G.NT_VARIANTS if v != "residual"]


@pytest.mark.parametrize("variant", [v for v in G.NT_VARIANTS if v != "residual"])
@pytest.mark.parametrize("M,N,K", G.TILED_EPILOGUE, ids=_ids(G.TILED_EPILOGUE))
def test_tiled_kernel_epilogue_chain_exact(ops, M, N, K, variant):
    """every step of the epilogue is exact on the integer family: a rounding to bf16 before the residual, a residual added before the row scale
    that belongs after it, a dropout mask of the wrong row (77 rows per image) all change the value"""
    assert variant in _variant_names()
    _exact_nt(ops, M, N, K, variant)


# ---- variants read once per process from the environment: one child process per setting
def _child(kind, env):
    code = (f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_gemm_exact_gpu as T; T.child_main({kind!r})")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    assert f"CHILD {kind} DONE" in r.stdout


def child_main(kind):
    """runs in the child process: all shapes of one environment setting"""
    ops = _load_ops()
    n = 0
    if kind == "stages":
        for M, N, K in G.TILED_STAGES:
            _exact_nt(ops, M, N, K)
            _exact_nt(ops, M, N, K, "bias+residual")
            n += 2
    else:
        shapes = {"tn2": G.TN2, "tn5": G.TN5, "tn5s2": G.TN5, "tns2": G.TN_STAGES2}[kind]
        for R, I, J in shapes:
            for alpha in (1.0, 0.5):
                _exact_tn(ops, R, I, J, alpha)
            _gauss_tn(ops, R, I, J, {"tn2": "gemm_tn2_kernel", "tn5": "gemm_tn5_kernel<3>", "tn5s2": "gemm_tn5_kernel<2>", "tns2": "gemm_tn_kernel<2>"}[kind])
            n += 3
    print(f"CHILD {kind} DONE {n} cases")


@pytest.mark.parametrize("stages", [3, 4])
def test_tiled_kernel_deeper_pipelines(stages):
    """gemm_nt_kernel<32, true, 3 | 4, 128> (CXR_GEMM_STAGES): K = 32 and 64 make the pipeline shorter than its depth"""
    _child("stages", {"CXR_GEMM_STAGES": str(stages)})


# ------------------------------------------------------------------------------------------------ 2. grouped launch
@pytest.mark.parametrize("Ms,N,K", G.GROUPS, ids=["257+1+129x196x96", "129+130x64x64"])
def test_grouped_launch_exact(ops, Ms, N, K):
    """cxr_gemm_nt_group_bf16 (gemm_nt_group_kernel): members of different heights, bias on one member only"""
    import ctypes
    from cxrmate_amd._lib import LIB
    cases = [G.exact_nt(M, N, K, "bias" if i == 1 else "plain", seed=10 + i) for i, M in enumerate(Ms)]
    arr = (ops._GemmNtDesc * len(cases))()
    keep, outs = [], []
    for d, c in zip(arr, cases):
        a, w, kw, _ = _nt_operands(ops, c)
        go = Guarded.rows(c["M"], N, BF, ld=_up8(N) + 8)
        keep.append((a, w, kw))
        outs.append(go)
        if "bias" in kw:
            d.bias = kw["bias"].data_ptr()
        d.A, d.lda, d.W, d.ldw, d.C, d.ldc = a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), go.view.data_ptr(), go.view.stride(0)
        d.M, d.N, d.K, d.alpha, d.drop_rows_per_b, d.rs_rows = c["M"], N, K, 1.0, 1, 1
    with _gemm_route("tiled"):
        LIB.call("cxr_gemm_nt_group_bf16", ctypes.addressof(arr), len(cases), ops._s())
    for go, c in zip(outs, cases):
        go.check(f"group member {c['M']}")
        G.assert_exact(go.view, G.nt_reference(c)[0], f"group {Ms}x{N}x{K} member {c['M']}")


# ------------------------------------------------------------------------------------------------ 3. implicit-GEMM convolution
@pytest.mark.parametrize("Bn,Cin,N,H,W", G.CONVS, ids=_ids(G.CONVS))
def test_conv_exact(ops, Bn, Cin, N, H, W):
    """cxr_gemm_nt_conv_bf16 (gemm_nt_conv_kernel) against torch conv2d in float64; H = W = 1: zero padding feeds eight of the nine taps"""
    from cxrmate_amd._lib import LIB
    c = G.exact_conv(Bn, Cin, N, H, W)
    x = G.embed(c["x"].reshape(Bn * H * W, Cin), "cuda", rows=(1, 2)).unflatten(0, (Bn, H * W))
    w, bias = G.embed(c["w"], "cuda"), _f32(c["bias"])
    M = Bn * c["Ho"] * c["Wo"]
    go = Guarded.rows(M, N, BF, ld=_up8(N) + 8)
    LIB.call("cxr_gemm_nt_conv_bf16", x.data_ptr(), x.stride(0), x.stride(1), Bn, H, W, Cin, 3, 2, 1, w.data_ptr(), w.stride(0), go.view.data_ptr(),
             go.view.stride(0), bias.data_ptr(), N, ops._s())
    go.check("conv")
    G.assert_exact(go.view, c["ref"], f"conv {Bn}x{Cin}x{N}x{H}x{W}")


# ------------------------------------------------------------------------------------------------ 4. row-strip kernel
@pytest.mark.parametrize("mt,stages", G.STRIP384, ids=[f"mt{m}-stages{s}" for m, s in G.STRIP384])
def test_row_strip_kernel_exact(ops, mt, stages):
    """gemm_strip384_kernel<mt, stages>: one row, one row short of / past a strip, two strips and a ragged third"""
    for M, N, K in G.strip_shapes(mt):
        for variant in G.STRIP_VARIANTS:
            _exact_nt(ops, M, N, K, variant, route=("strip", mt, stages))


@pytest.mark.parametrize("mt", G.STRIP192)
def test_row_strip_kernel_n192_exact(ops, mt):
    for M, N, K in G.strip_shapes(mt, n192=True):
        for variant in G.STRIP_VARIANTS:
            _exact_nt(ops, M, N, K, variant, route=("strip", mt, 0))


# ------------------------------------------------------------------------------------------------ 5. W-stationary kernel
@pytest.mark.parametrize("variant", G.WS_VARIANTS)
@pytest.mark.parametrize("M,N,K", G.WS, ids=_ids(G.WS))
def test_w_stationary_kernel_exact(ops, M, N, K, variant):
    """gemm_ws384_kernel<false | true>"""
    _exact_nt(ops, M, N, K, variant, route="ws")


# ------------------------------------------------------------------------------------------------ 6. persistent kernel
def _pk_id(cfg, variant):
    back = {1: 0, 4: 3}.get(cfg) if variant == "bias+residual" else None
    return f"pk{cfg}-{variant}" + (f"-runs-as-pk{back}" if back is not None else "")


@pytest.mark.parametrize("cfg,variant", [(c, v) for c in range(7) for v in G.PK_VARIANTS], ids=[_pk_id(c, v) for c in range(7) for v in G.PK_VARIANTS])
def test_persistent_kernel_exact(ops, cfg, variant):
    """gemm_nt_pk_kernel<PkC0 .. PkC6>; with a second [M, N] operand configurations 1 and 4 run as 0 and 3 (gemm_pk_launch). Configuration 6 (the
    only one with two A fragments per wave and two K halves per step) read only two of its four W fragments of the second K half until this test
    reached it: columns 32 .. 63 of every wave's 64 were wrong."""
    for M, N, K in G.PK:
        _exact_nt(ops, M, N, K, variant, route=("pk", cfg))


# ------------------------------------------------------------------------------------------------ 7. weight gradient
def _run_tn(ops, c, extra=24):
    R, I, J = c["R"], c["I"], c["J"]
    p, q = G.embed(c["p"], "cuda"), G.embed(c["q"], "cuda")
    go = Guarded((I + 4, J + extra), F32, (slice(2, 2 + I), slice(8, 8 + J)))
    gd = Guarded.flat(I, F32)
    go.view.copy_(c["out0"])
    gd.view.copy_(c["db0"])
    ops.gemm_tn(p, q, go.view, dbias=gd.view, alpha=c["alpha"])
    go.check(f"gemm_tn {R}x{I}x{J}")
    gd.check(f"gemm_tn dbias {R}x{I}x{J}")
    return go.view, gd.view


def _exact_tn(ops, R, I, J, alpha, extra=24):
    c = G.exact_tn(R, I, J, alpha)
    out, db = _run_tn(ops, c, extra)
    ref, ref_b = G.tn_reference(c)
    G.assert_exact(out, ref, f"gemm_tn {R}x{I}x{J} alpha={alpha}")
    G.assert_exact(db, ref_b, f"gemm_tn dbias {R}x{I}x{J}")


def _gauss_tn(ops, R, I, J, kernel, extra=24):
    c = G.gauss_tn(R, I, J)
    out, db = _run_tn(ops, c, extra)
    ref, tol, ref_b, tol_b = G.gauss_tn_tol(c)
    _figure(out, ref, tol, f"{R}x{I}x{J}", kernel)
    _figure(db, ref_b, tol_b, f"{R}x{I}x{J} dbias", kernel + " dbias")


def _lib_splits(R, I, J):
    import ctypes
    from cxrmate_amd._lib import LIB
    s, need = ctypes.c_int(0), ctypes.c_long(0)
    LIB.call("cxr_gemm_tn_plan", R, I, J, ctypes.byref(s), ctypes.byref(need))
    return s.value


@pytest.mark.parametrize("R,I,J", G.TN4, ids=_ids(G.TN4))
def test_weight_gradient_kernel(ops, R, I, J):
    """gemm_tn_kernel<4> and the ordered reduce gemm_tn_reduce_kernel<1 | 4 | 16>, into a strided view of a wider guarded matrix"""
    assert _lib_splits(R, I, J) == G.tn_plan(R, I, J)[0]
    for alpha in (1.0, 0.5):
        _exact_tn(ops, R, I, J, alpha)
    _gauss_tn(ops, R, I, J, f"gemm_tn_kernel<4> {G.tn_split_class(G.tn_plan(R, I, J)[0])}")


def test_weight_gradient_split_classes_and_row_stride(ops):
    """the shapes above reach every class of the reduce; R = 8001 and 16001 leave the last split and the last 32-row tile ragged"""
    classes = {G.tn_split_class(_lib_splits(*s)) for s in G.TN4}
    assert classes == {"atomic", "SL1", "SL4", "SL16"}, classes
    for R in (8001, 16001):
        splits, per, nrt = G.tn_plan(R, 128, 128)
        assert R % 32 and nrt % per and splits == _lib_splits(R, 128, 128)
    R, I, J = G.TN_LD4
    assert (J + 28) % 8 == 4
    _exact_tn(ops, R, I, J, 0.5, extra=28)


@pytest.mark.parametrize("kind,env", [("tn2", {"CXR_TN2_MIN": "1"}), ("tn5", {"CXR_TN5_MIN": "1"}), ("tn5s2", {"CXR_TN5_MIN": "1", "CXR_TN5_STAGES": "2"}),
                                      ("tns2", {"CXR_TN_STAGES": "2"})], ids=["gemm_tn2_kernel", "gemm_tn5_kernel-3", "gemm_tn5_kernel-2", "gemm_tn_kernel-2"])
def test_weight_gradient_kernel_variants(kind, env):
    _child(kind, env)


# ------------------------------------------------------------------------------------------------ 8. skinny GEMMs
def _run_skinny(ops, c, ld=None):
    M, N = c["M"], c["N"]
    a, w, kw, _ = _nt_operands(ops, c)
    kw.pop("alpha", None)
    fac = None
    if "drop" in kw:
        p, seed, site, _, t0 = kw.pop("drop")
        kw["drop"] = (p, seed, site, t0)
        fac = ops.dropout_mask(M, N, p, seed, site, 1, t0, factor=True).cpu().double()
    go = Guarded.rows(M, N, F32 if c["out_f32"] else BF, ld=ld or N + 5)
    ops.gemm_skinny(a, w, out=go.view, out_f32=c["out_f32"], **kw)
    go.check(f"skinny {M}x{N}x{c['K']} {c['variant']}")
    return go.view, fac


_SKINNY_AS = {"plain": "plain", "bias+residual": "bias+residual", "f32": "f32", "dropout": "dropout+residual"}


@pytest.mark.parametrize("M,N,K", G.SKINNY, ids=_ids(G.SKINNY))
def test_skinny_gemm(ops, M, N, K):
    """gemm_skinny_kernel<1 .. 4, false, 4 | 8>: ragged 16-row and 16-column tiles, K >= 2048: the 8-wave form; N = 100: rows 4 mod 8 apart"""
    for variant in G.SKINNY_VARIANTS:
        c = G.exact_nt(M, N, K, _SKINNY_AS[variant], seed=5)
        out, fac = _run_skinny(ops, c, ld=N if N == 100 else None)
        G.assert_exact(out, G.nt_reference(c, fac)[0], f"skinny {M}x{N}x{K} {variant}")
    for variant in ("bias+residual", "f32", "dropout+residual"):
        c = G.gauss_nt(M, N, K, variant)
        c.pop("alpha")
        out, fac = _run_skinny(ops, c)
        ref, tol = G.gauss_nt_tol(c, fac)
        _figure(out, ref, tol, f"{M}x{N}x{K} {variant}", "gemm_skinny_kernel" + ("<.., 8>" if K >= 2048 else "<.., 4>"))


@pytest.mark.parametrize("M,N,K", G.SKINNY3, ids=_ids(G.SKINNY3))
def test_skinny3_exact(ops, M, N, K):
    """three projections into strided KV-cache-like rows, with the precomputed-LoRA term t B^T on problems 0 and 1"""
    cs = [G.exact_nt(M, N, K, "bias", seed=20 + i) for i in range(3)]
    g = torch.Generator().manual_seed(M + N)
    a = G.embed(cs[0]["a"], "cuda")
    ws = [G.embed(c["w"], "cuda") for c in cs]
    bs = [_f32(c["bias"]) for c in cs]
    ld = N + 6
    caches = [Guarded((M, 5, ld), BF, (slice(None), 3, slice(0, N))) for _ in range(3)]
    for lora in (False, True):
        ts = [torch.randint(-15, 16, (M, 8), generator=g).double() for _ in range(2)]
        Bs = [torch.randint(-15, 16, (N, 8), generator=g).double() for _ in range(2)]
        kw = dict(lora0=(_f32(ts[0]), Bs[0].to(BF).cuda().contiguous()), lora1=(_f32(ts[1]), Bs[1].to(BF).cuda().contiguous())) if lora else {}
        ops.gemm_skinny3(a, ws[0], bs[0], caches[0].view, ws[1], bs[1], caches[1].view, ws[2], bs[2], caches[2].view, **kw)
        for i in range(3):
            caches[i].check(f"skinny3 problem {i}")
            ref = cs[0]["a"] @ cs[i]["w"].t() + cs[i]["bias"][None, :]
            if lora and i < 2:
                ref = ref + ts[i] @ Bs[i].t()
            G.assert_exact(caches[i].view, ref, f"skinny3 {M}x{N}x{K} problem {i} lora={lora}")


# ------------------------------------------------------------------------------------------------ 9. decode-step GEMM
def _run_dec(ops, c, kind, mt_hint=0, nc_hint=0):
    """One cxr_dec_gemm_bf16 launch of a case -> ([output per problem as a row-major tensor], dropout factors | None)"""
    M, K, Ns = c["M"], c["K"], c["Ns"]
    x = G.embed(c["a"], "cuda")
    a_dal, _ = ops.dec_to_dal(x)
    assert torch.equal(ops.dec_from_dal(a_dal, M, K).view(torch.int16), x.contiguous().view(torch.int16)), "the layout round trip changed bits"
    probs, guards = [], []
    for i, (N, w) in enumerate(zip(Ns, c["w"])):
        wp, bc = ops.dec_pack_weight(G.embed(w, "cuda"), None, None, None if c["bias"][i] is None else _f32(c["bias"][i]))
        colsum = w.sum(1)
        if c["family"] == "exact":
            G.assert_exact(bc[:, 1], colsum, f"dec_pack_weight column sums N={N}")
            G.assert_exact(bc[:, 0], c["bias"][i] if c["bias"][i] is not None else torch.zeros(N, dtype=torch.float64), f"dec_pack_weight bias N={N}")
        pr = dict(wp=wp, bc=bc, N=N)
        if not (kind == "dal" and i == 0):
            ld = N + (4 if N % 8 == 0 else 6) if i == 0 else N + 10
            go = Guarded.rows(M, N, F32 if kind == "f32" else BF, ld=ld)
            pr["out"] = go.view
            guards.append(go)
        probs.append(pr)
    kw, fac = {}, None
    if c["residual"] is not None:
        kw["residual"] = ops.dec_to_dal(G.embed(c["residual"], "cuda"))[0]
    if c["drop"] is not None:
        p, site, t = c["drop"]
        seed = _seed(11)
        kw["drop"] = (p, seed, site, t)
        fac = ops.dropout_mask(M, max(Ns), p, seed, site, 1, t, factor=True).cpu().double()
    outs, _ = ops.dec_gemm(a_dal, M, K, probs, out_f32=kind == "f32", mt_hint=mt_hint, nc_hint=nc_hint, **kw)
    for go in guards:
        go.check(f"dec_gemm {M}x{Ns}x{K}")
    if kind == "dal":
        outs[0] = ops.dec_from_dal(outs[0], M, Ns[0])
    return outs, fac


@pytest.mark.parametrize("M,K,Ns,kind,variant,mt_hint", G.DEC, ids=[f"{m}x{'+'.join(map(str, ns))}x{k}-{kind}-{v}-mt{h}" for m, k, ns, kind, v, h in G.DEC])
def test_decode_gemm(ops, M, K, Ns, kind, variant, mt_hint):
    """dec_gemm_kernel<1 | 2 | 4, 8, 3, 1> and <.., 16, 6, 1>: one to three problems of different widths per launch, ragged row and column tiles,
    outputs in the decode activation layout, in strided row-major rows (4 mod 8 elements apart for problem 0) and in fp32"""
    for hint in sorted({mt_hint, 0}):
        c = G.dec_case(M, K, Ns, variant)
        outs, fac = _run_dec(ops, c, kind, hint)
        for i, (ref, _) in enumerate(G.dec_reference(c, fac)):
            G.assert_exact(outs[i], ref, f"dec_gemm {M}x{Ns}x{K} {variant} {kind} problem {i} mt_hint={hint}")
    c = G.dec_case(M, K, Ns, variant, "gauss")
    outs, fac = _run_dec(ops, c, kind, mt_hint)
    for i, (ref, tol) in enumerate(G.dec_reference(c, fac)):
        _figure(outs[i], ref, tol, f"{M}x{Ns}x{K} {variant} {kind} problem {i}", f"dec_gemm_kernel K={K}")


@pytest.mark.parametrize("nc_hint", [1, 4])
def test_decode_gemm_vocabulary_width(ops, nc_hint):
    """dec_gemm_kernel<.., 8, 3, 1 | 4>: N = 8192, 16 or 64 columns per workgroup"""
    M, K, N = G.DEC_VOCAB
    c = G.dec_case(M, K, (N,), "bias")
    outs, _ = _run_dec(ops, c, "f32", 0, nc_hint)
    G.assert_exact(outs[0], G.dec_reference(c)[0][0], f"dec_gemm vocabulary nc_hint={nc_hint}")
    c = G.dec_case(M, K, (N,), "bias", "gauss")
    outs, _ = _run_dec(ops, c, "f32", 0, nc_hint)
    ref, tol = G.dec_reference(c)[0]
    _figure(outs[0], ref, tol, f"{M}x{N}x{K} nc_hint={nc_hint}", f"dec_gemm_kernel NC={nc_hint}")


def test_decode_gemm_refuses_a_layout_output_narrower_than_its_blocks(ops):
    """the decode activation layout is made of 32-column blocks: an output (or a residual) in that layout with N % 32 != 0 would be addressed past
    its [rows, N] buffer, so the entry point refuses it"""
    from cxrmate_amd._lib import CxrError
    c = G.dec_case(33, 768, (48,), "bias")
    a_dal, _ = ops.dec_to_dal(G.embed(c["a"], "cuda"))
    wp, bc = ops.dec_pack_weight(G.embed(c["w"][0], "cuda"), None, None, _f32(c["bias"][0]))
    with pytest.raises(CxrError):
        ops.dec_gemm(a_dal, 33, 768, [dict(wp=wp, bc=bc, N=48)])
    res = torch.zeros(ops.dal_rows(33), 64, dtype=BF, device="cuda")
    with pytest.raises(CxrError):
        ops.dec_gemm(a_dal, 33, 768, [dict(wp=wp, bc=bc, N=48, out=torch.empty(33, 48, dtype=BF, device="cuda"))], residual=res)


# ------------------------------------------------------------------------------------------------ 10. e4m3 GEMM
def _run_fp8(ops, c, ldc=None):
    from cxrmate_amd._lib import LIB
    M, N, K = c["M"], c["N"], c["K"]
    a8, w8 = G.embed_e4m3(c["a"], "cuda"), G.embed_e4m3(c["w"], "cuda")
    bias = _f32(c["bias"]) if c.get("bias") is not None else None
    res = G.embed(c["residual"], "cuda") if c.get("residual") is not None else None
    rs = c.get("row_scale")
    rsf = _f32(rs[0]) if rs is not None else None
    gc, g8 = Guarded.rows(M, N, BF, ld=ldc or _up8(N) + 8), Guarded.rows(M, N, torch.uint8, ld=(ldc or _up8(N) + 8))
    LIB.call("cxr_gemm_nt_fp8", a8.data_ptr(), a8.stride(0), w8.data_ptr(), w8.stride(0), gc.view.data_ptr(), gc.view.stride(0), g8.view.data_ptr(),
             g8.view.stride(0), 1.0 / c["out_scale"], M, N, K, float(c["alpha"]), None if bias is None else bias.data_ptr(),
             None if res is None else res.data_ptr(), 0 if res is None else res.stride(0), 0,
             *((rsf.data_ptr(), int(rs[1]), int(bool(rs[2]))) if rs is not None else (None, 1, 0)), ops._s())
    gc.check("fp8 bf16 output")
    g8.check("fp8 e4m3 output")
    return gc.view, g8.view


@pytest.mark.parametrize("variant", G.FP8_VARIANTS)
@pytest.mark.parametrize("M,N,K", G.FP8, ids=_ids(G.FP8))
def test_fp8_gemm_exact(ops, M, N, K, variant):
    """gemm_fp8_kernel<64>: 1, 2 and 3 K-steps of 64; N % 8 != 0: the per-element epilogue. The bf16 output is the RNE of the exact value, the
    e4m3 output the round-to-nearest-even of value / out_scale over the finite e4m3 codes (out_scale keeps it below 448: no saturation here)."""
    c = G.exact_fp8(M, N, K, variant)
    ref = G.nt_reference(c)[0]
    for ldc in (None, N + 4) if (M, N, K) == (129, 64, 128) else (None,):
        out, out8 = _run_fp8(ops, c, ldc)
        G.assert_exact(out, ref, f"fp8 {M}x{N}x{K} {variant} ldc={ldc}")
        G.assert_exact_e4m3(out8, ref.numpy(), c["out_scale"], f"fp8 e4m3 {M}x{N}x{K} {variant} ldc={ldc}")
