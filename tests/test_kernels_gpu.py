"""GPU: each HIP kernel (called through the C ABI) against an fp32 torch reference of the same op on the same
bf16-rounded inputs. Tolerances are those of bf16 storage with fp32 accumulation; integer kernels are bit-exact."""
import math

import numpy as np
import pytest
import torch
from bounds_util import Guarded, all_bf16, assert_bf16_bracket, assert_f32_bound, gelu64

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import ops as _ops
    from cxrmate_amd._lib import LIB
    LIB.load()
    return _ops


def dev(t):
    return t.cuda()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + int(np.prod(shape)) % 9973)
    return (torch.randn(*shape, generator=g) * scale)


def close(a, b, rtol=2e-2, atol=2e-2, what=""):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    denom = b.abs().max().item() + 1e-12
    rel_rms = (err.pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-12)).item()
    assert torch.isfinite(a).all(), f"{what}: non-finite output"
    assert rel_rms < rtol and err.max().item() < atol * max(1.0, denom), \
        f"{what}: rel_rms {rel_rms:.3e} max_err {err.max().item():.3e} (ref absmax {denom:.3e})"


# ------------------------------------------------------------------------------------------------ GEMM
class _gemm_route:
    """Force the NT GEMM onto one kernel family for a block of calls: 'tiled' (gemm_nt_kernel), ('pk', config index) (csrc/gemm_pk.hip),
    'ws' (csrc/gemm_ws.hip, every K = 384 / N % 384 == 0 shape)."""

    def __init__(self, route):
        self.route = route

    def __enter__(self):
        from cxrmate_amd._lib import LIB
        r = self.route
        LIB.call("cxr_gemm_strip_config", 0, -1, -1, -1)
        if r == "tiled":
            LIB.call("cxr_gemm_set_exclusive", 0)
        elif isinstance(r, tuple) and r[0] == "strip":
            LIB.call("cxr_gemm_set_exclusive", 0)
            LIB.call("cxr_gemm_strip_config", 1, r[1], 1, r[2])
        elif r == "ws":
            LIB.call("cxr_gemm_set_exclusive", 1)
            LIB.call("cxr_gemm_ws_config", 1, 1, 1, -1, 0)
            LIB.call("cxr_gemm_pk_config", 0, -1, -1, -1)
        else:
            LIB.call("cxr_gemm_set_exclusive", 1)
            LIB.call("cxr_gemm_ws_config", 0, -1, -1, -1, -1)
            LIB.call("cxr_gemm_pk_config", 1, 1000 + r[1], 1, -1)
        return self

    def __exit__(self, *exc):
        from cxrmate_amd._lib import LIB
        LIB.call("cxr_gemm_set_exclusive", 1)
        LIB.call("cxr_gemm_ws_config", 1, 0, 2048, -1, 0)
        LIB.call("cxr_gemm_pk_config", 1, 0, 2048, 0)
        LIB.call("cxr_gemm_strip_config", 1, 0, -2, 0)
        return False


def _gemm_variants(M, N, seed):
    bias = dev(rnd(N, seed=seed + 1))
    res = dev(rnd(M, N, seed=seed + 2).to(BF))
    rs = dev(torch.rand(max(1, (M + 576) // 577)) * 2)
    dseed = torch.tensor([4321], dtype=torch.int32, device="cuda")
    return {"plain": dict(), "bias": dict(bias=bias), "bias+residual": dict(bias=bias, residual=res), "gelu+saved": dict(bias=bias, act=1, aux="new"),
            "gelu": dict(bias=bias, act=1), "gelu'": dict(act=2, aux=res), "droppath after": dict(bias=bias, residual=res, row_scale=(rs, 577, True)),
            "droppath before": dict(bias=bias, residual=res, row_scale=(rs, 577, False)), "alpha": dict(alpha=0.37, bias=bias),
            "f32": dict(bias=bias, out_f32=True), "dropout+residual": dict(bias=bias, residual=res, drop=(0.1, dseed, 7, 256, 3))}


def _run_variant(ops, a, w, kw):
    kw = dict(kw)
    aux = None
    if kw.get("aux") == "new":
        aux = kw["aux"] = torch.zeros(a.shape[0], w.shape[0], device="cuda", dtype=BF)
    return ops.gemm_nt(a, w, **kw), aux


@pytest.mark.parametrize("route", [("pk", 0), ("pk", 1), ("pk", 2), ("pk", 3), ("pk", 4), ("pk", 5)])
@pytest.mark.parametrize("M,N,K", [(36928, 384, 384), (4000, 392, 128), (2049, 64, 64), (5000, 1000, 192), (300, 384, 1536), (70, 136, 64), (3000, 30000, 128)])
def test_gemm_persistent_kernel_is_bit_identical_to_the_tiled_kernel(ops, route, M, N, K):
    """csrc/gemm_pk.hip (every built tile configuration; ragged row / column tails, row strides != K, every epilogue) against gemm_nt_kernel: same
    MFMA orientation and K order -> the same bits; and against fp32 torch on the plain product."""
    a = dev(rnd(M + 3, K + 8, seed=M).to(BF))[:M, :K]
    w = dev((rnd(N, K, seed=N) * 0.1).to(BF))
    for name, kw in _gemm_variants(M, N, M + N).items():
        with _gemm_route("tiled"):
            ref, ref_aux = _run_variant(ops, a, w, kw)
        with _gemm_route(route):
            out, out_aux = _run_variant(ops, a, w, kw)
        assert torch.equal(ref, out), f"{route} {M}x{N}x{K} {name}: {int((ref != out).sum())} elements differ"
        assert ref_aux is None or torch.equal(ref_aux, out_aux), f"{route} {M}x{N}x{K} {name}: saved pre-activation differs"
        if name == "plain":
            close(out, a.float() @ w.float().t(), rtol=1e-2, atol=1e-2, what=f"{route} {M}x{N}x{K}")


@pytest.mark.parametrize("M,N", [(36928, 384), (9280, 384), (36928, 1536), (1000, 384), (70, 768), (4999, 1536)])
def test_gemm_w_stationary_kernel_is_bit_identical_to_the_tiled_kernel(ops, M, N):
    """csrc/gemm_ws.hip (K = 384: weights resident in registers, A / second-operand blocks through the LDS ring, anti-phased wave groups) against
    gemm_nt_kernel on every epilogue it takes; other shapes / epilogues must fall through to the tiled kernels unchanged."""
    K = 384
    a = dev(rnd(M + 3, K + 8, seed=M).to(BF))[:M, :K]
    w = dev((rnd(N, K, seed=N) * 0.1).to(BF))
    for name, kw in _gemm_variants(M, N, M + N).items():
        with _gemm_route("tiled"):
            ref, ref_aux = _run_variant(ops, a, w, kw)
        with _gemm_route("ws"):
            out, out_aux = _run_variant(ops, a, w, kw)
        assert torch.equal(ref, out), f"ws {M}x{N} {name}: {int((ref != out).sum())} elements differ"
        assert ref_aux is None or torch.equal(ref_aux, out_aux), f"ws {M}x{N} {name}: saved pre-activation differs"
        if name == "plain":
            close(out, a.float() @ w.float().t(), rtol=1e-2, atol=1e-2, what=f"ws {M}x{N}")


@pytest.mark.parametrize("mt,stages", [(10, 0), (6, 0), (4, 0), (2, 0), (10, 2), (4, 2), (10, 3), (10, 4)])      # (stages 0 at mt 10 = two stages of 64-deep steps, the default)
@pytest.mark.parametrize("M,K", [(36928, 384), (9280, 384), (5003, 1536), (100, 64)])
def test_gemm_row_strip_kernel_is_bit_identical_to_the_tiled_kernel(ops, mt, stages, M, K):
    """csrc/gemm_strip.hip (M x 384 x K: a strip of 16 mt rows x all 384 columns per workgroup, every strip height and stage count; ragged row tails,
    row strides != K, every epilogue it takes) against gemm_nt_kernel: same MFMA orientation and K order -> the same bits; the epilogues it does not take
    (GELU, dropout, fp32 output) must fall through to the tiled kernel unchanged."""
    N = 384
    a = dev(rnd(M + 3, K + 8, seed=M).to(BF))[:M, :K]
    w = dev((rnd(N, K, seed=N) * 0.1).to(BF))
    for name, kw in _gemm_variants(M, N, M + N).items():
        with _gemm_route("tiled"):
            ref, ref_aux = _run_variant(ops, a, w, kw)
        with _gemm_route(("strip", mt, stages)):
            out, out_aux = _run_variant(ops, a, w, kw)
        assert torch.equal(ref, out), f"strip mt={mt} {M}x{N}x{K} {name}: {int((ref != out).sum())} elements differ"
        assert ref_aux is None or torch.equal(ref_aux, out_aux), f"strip {M}x{N}x{K} {name}: saved pre-activation differs"
        if name == "plain":
            close(out, a.float() @ w.float().t(), rtol=1e-2, atol=1e-2, what=f"strip {M}x{N}x{K}")


@pytest.mark.parametrize("mt", [8, 12, 16])
@pytest.mark.parametrize("M,K", [(36864, 192), (5003, 768), (100, 64)])
def test_gemm_row_strip_kernel_n192_is_bit_identical_to_the_tiled_kernel(ops, mt, M, K):
    """The N = 192 form of csrc/gemm_strip.hip (CvT stage 2: strips of 16 mt rows x all 192 columns, 3 MFMA tile columns per wave) against gemm_nt_kernel."""
    N = 192
    a = dev(rnd(M + 3, K + 8, seed=M).to(BF))[:M, :K]
    w = dev((rnd(N, K, seed=N) * 0.1).to(BF))
    for name, kw in _gemm_variants(M, N, M + N).items():
        with _gemm_route("tiled"):
            ref, ref_aux = _run_variant(ops, a, w, kw)
        with _gemm_route(("strip", mt, 0)):
            out, out_aux = _run_variant(ops, a, w, kw)
        assert torch.equal(ref, out), f"strip192 mt={mt} {M}x{N}x{K} {name}: {int((ref != out).sum())} elements differ"
        assert ref_aux is None or torch.equal(ref_aux, out_aux), f"strip192 {M}x{N}x{K} {name}: saved pre-activation differs"
        if name == "plain":
            close(out, a.float() @ w.float().t(), rtol=1e-2, atol=1e-2, what=f"strip192 {M}x{N}x{K}")


def test_gemm_persistent_asymmetric_identity(ops):
    # A = I with an asymmetric W through the W-row deal of the persistent kernels: a permuted column would show exactly
    n = 384
    a = dev(torch.eye(n).repeat(8, 1).to(BF))                     # [3072, 384]: every row block sees the identity
    w = dev((torch.arange(n * n).reshape(n, n) % 251 - 125).float().to(BF))
    for route in (("pk", 0), ("pk", 1), "ws"):
        with _gemm_route(route):
            out = ops.gemm_nt(a, w)
        assert torch.equal(out.float().cpu(), w.float().t().repeat(8, 1).cpu()), route


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 192, 192), (577, 384, 1536), (1000, 30000 // 8 * 4, 768), (64, 64, 32),
                                   (9216, 64, 192), (17, 768, 3072), (256, 128, 96)])
@pytest.mark.parametrize("regstage", [0, 1])
def test_gemm_plain(ops, M, N, K, regstage):
    from cxrmate_amd._lib import LIB
    LIB.call("cxr_gemm_set_regstage", regstage)
    try:
        a, w = dev(rnd(M, K).to(BF)), dev(rnd(N, K, seed=1).to(BF))
        out = ops.gemm_nt(a, w)
        ref = a.float() @ w.float().t()
        close(out, ref, rtol=1e-2, atol=1e-2, what=f"gemm {M}x{N}x{K} regstage={regstage}")
    finally:
        LIB.call("cxr_gemm_set_regstage", 0)


def test_gemm_asymmetric_identity(ops):
    # A = I with an asymmetric W catches transposed / permuted fragment layouts exactly (integers are exact in bf16)
    K = 128
    a = torch.eye(K).to(BF).cuda()
    w = (torch.arange(192 * K).reshape(192, K) % 251 - 125).float().to(BF).cuda()
    out = ops.gemm_nt(a, w, out_f32=True)
    assert torch.equal(out.cpu(), w.float().t().cpu())


def test_gemm_epilogues(ops):
    M, N, K = 333, 256, 192
    a, w = dev(rnd(M, K).to(BF)), dev(rnd(N, K, seed=1, scale=0.1).to(BF))
    bias, res = dev(rnd(N, seed=2)), dev(rnd(M, N, seed=3).to(BF))
    base = a.float() @ w.float().t() + bias
    close(ops.gemm_nt(a, w, bias=bias), base, what="bias")
    aux = torch.empty(M, N, dtype=BF, device="cuda")
    out = ops.gemm_nt(a, w, bias=bias, act=1, aux=aux, residual=res)
    close(aux, base, what="preact")
    close(out, torch.nn.functional.gelu(base) + res.float(), what="gelu+res")
    # act=2: multiply by GELU'(aux)
    x = aux.float().requires_grad_(True)
    torch.nn.functional.gelu(x).sum().backward()
    out2 = ops.gemm_nt(a, w, act=2, aux=aux)
    close(out2, (a.float() @ w.float().t()) * x.grad, what="gelu'")
    # fp32 out with accumulate and alpha, row-strided operands
    big = dev(rnd(M, 2 * K, seed=5).to(BF))
    av = big[:, K:]
    acc = dev(rnd(M, N, seed=6))
    ref = acc + 0.5 * (av.float() @ w.float().t())
    ops.gemm_nt(av, w, out=acc, out_f32=True, accumulate=True, alpha=0.5)
    close(acc, ref, what="accumulate")


def test_transpose_colsum_weightgrad(ops):
    x = dev(rnd(577, 384).to(BF))
    t = ops.transpose(x, 64)
    assert t.shape == (384, 640)
    assert torch.equal(t[:, :577].cpu(), x.t().cpu()) and bool((t[:, 577:] == 0).all())
    out = torch.zeros(384, device="cuda")
    ops.colsum_into(x, out)
    close(out, x.float().sum(0), rtol=1e-3, atol=1e-3, what="colsum")
    dy = dev(rnd(577, 192, seed=3).to(BF))
    dw = torch.zeros(192, 384, device="cuda")
    db = torch.zeros(192, device="cuda")
    ops.linear_bwd_weight(dy, x, dw, db)
    close(dw, dy.float().t() @ x.float(), what="dW")
    close(db, dy.float().sum(0), rtol=1e-3, atol=1e-3, what="db")


@pytest.mark.parametrize("R,I,J", [(577, 192, 384), (18464, 384, 1536), (100, 64, 64), (8192, 768, 768), (4100, 1000, 768), (31, 8, 768),
                                   (36928, 384, 384), (36928, 1536, 384), (36928, 384, 1536), (40000, 768, 200), (33000, 384, 136)])     # (384 x 128 blocks)
def test_gemm_tn_weight_grad(ops, R, I, J):
    big = dev(rnd(R, I + 64, seed=1).to(BF))
    p, q = big[:, :I], dev(rnd(R, J, seed=2).to(BF))
    out = dev(rnd(I, J, seed=3))
    db = dev(rnd(I, seed=4))
    ref = out + 0.5 * (p.float().t() @ q.float())
    ref_b = db + p.float().sum(0)
    ops.gemm_tn(p, q, out, dbias=db, alpha=0.5)
    close(out, ref, rtol=1e-2, atol=1e-2, what=f"gemm_tn {R}x{I}x{J}")
    close(db, ref_b, rtol=1e-2, atol=1e-2, what="gemm_tn dbias")


@pytest.mark.parametrize("R,I,J", [(96, 128, 256), (4128, 384, 384), (4128, 768, 264), (4128, 512, 384)])
def test_gemm_tn_exact_integers(ops, R, I, J, monkeypatch):
    # small integers are exact in bf16 and in fp32 accumulation: any row/column permutation of the transposed LDS reads shows up
    # (the larger shapes run the 256 x 256- and the 384 x 128-block kernels: CXR_TN2_MIN=1 sends every shape wider than 128 there)
    if R > 96:
        import subprocess, sys, os
        code = ("import torch; from cxrmate_amd import ops\n"
                f"R, I, J = {R}, {I}, {J}\n"
                "BF = torch.bfloat16\n"
                "p = ((torch.arange(R * I).reshape(R, I) * 7) % 5 - 2).float().to(BF).cuda()\n"
                "q = ((torch.arange(R * J).reshape(R, J) * 3) % 7 - 3).float().to(BF).cuda()\n"
                "out = torch.zeros(I, J, device='cuda'); db = torch.zeros(I, device='cuda')\n"
                "ops.gemm_tn(p, q, out, dbias=db)\n"
                "assert torch.equal(out.cpu(), (p.double().t() @ q.double()).float().cpu()), 'product'\n"
                "assert torch.equal(db.cpu(), p.double().sum(0).float().cpu()), 'bias'\n")
        env = dict(os.environ, CXR_TN2_MIN="1")            # (read once per process by the library: a child process)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert r.returncode == 0, r.stderr[-2000:]
        return
    p = ((torch.arange(R * I).reshape(R, I) * 7) % 5 - 2).float().to(BF).cuda()
    q = ((torch.arange(R * J).reshape(R, J) * 3) % 7 - 3).float().to(BF).cuda()
    out = torch.zeros(I, J, device="cuda")
    ops.gemm_tn(p, q, out)
    assert torch.equal(out.cpu(), (p.float().t() @ q.float()).cpu())


@pytest.mark.parametrize("R,I,J", [(8192, 768, 768), (5000, 384, 1536), (3001, 200, 72), (36928, 384, 384)])
def test_gemm_tn_is_deterministic(ops, R, I, J):
    """Weight-gradient GEMM: the token dimension is split over workgroups; partial tiles are reduced in split order (no float atomics), so two
    launches on the same operands give the same bits -- also into a strided view of a wider gradient matrix and with the bias gradient."""
    p, q = dev(rnd(R, I, seed=11).to(BF)), dev(rnd(R, J, seed=12).to(BF))
    wide = [torch.zeros(I, J + 24, device="cuda") for _ in range(2)]
    dbs = [torch.zeros(I, device="cuda") for _ in range(2)]
    for w, d in zip(wide, dbs):
        ops.gemm_tn(p, q, w[:, 8:8 + J], dbias=d)
        ops.gemm_tn(p, q, w[:, 8:8 + J], dbias=d, alpha=0.25)          # accumulates
    assert torch.equal(wide[0], wide[1]) and torch.equal(dbs[0], dbs[1])
    assert float(wide[0][:, :8].abs().max()) == 0.0 and float(wide[0][:, 8 + J:].abs().max()) == 0.0
    close(wide[0][:, 8:8 + J], 1.25 * (p.float().t() @ q.float()), rtol=1e-2, atol=1e-2, what="deterministic gemm_tn")
    close(dbs[0], 2.0 * p.float().sum(0), rtol=1e-2, atol=1e-2, what="deterministic gemm_tn dbias")


def test_deferred_weight_gradient_sums_equal_the_immediate_ones(ops):
    """Round 4: on the weight-gradient stream every split-K weight-gradient GEMM only leaves its partial tiles behind (scratch of its own) and ONE
    batched launch adds all pending sums (cxr_gemm_tn_partial_bf16 + cxr_gemm_tn_reduce_batch, wgrad.reduce). Same lanes, same split order as the
    per-GEMM reduce launches: the gradients -- 60 of them here (two batches), strided outputs, bias gradients, accumulation into non-zero buffers,
    the same output hit twice -- are bit-identical to the immediate path, and a second deferred round over the recycled scratch is too."""
    from cxrmate_amd import wgrad
    shapes = [(8192, 768, 768), (5000, 384, 1536), (3001, 200, 72), (9280, 384, 384), (4096, 64, 64), (6000, 192, 576), (2048, 3072, 768)]
    probs = []
    for n in range(60):
        R, I, J = shapes[n % len(shapes)]
        R = R - 32 * (n // len(shapes))
        probs.append((dev(rnd(R, I, seed=100 + n).to(BF)), dev(rnd(R, J, seed=200 + n).to(BF)), n % 3 != 0, 1.0 if n % 2 else 0.5))

    calls = {"partial": 0, "batch": 0, "single": 0}
    real_call = ops.LIB.call

    def counting(name, *a):
        key = {"cxr_gemm_tn_partial_bf16": "partial", "cxr_gemm_tn_reduce_batch": "batch", "cxr_gemm_tn_bf16": "single"}.get(name)
        if key:
            calls[key] += 1
        return real_call(name, *a)

    def run(deferred):
        outs = [torch.full((p.shape[1], q.shape[1] + 8), 0.25, device="cuda") for p, q, _, _ in probs]
        dbs = [torch.full((p.shape[1],), -1.0, device="cuda") if b else None for p, _, b, _ in probs]
        rounds = []
        for rnd_ in range(2):
            if deferred:
                with wgrad.overlap():
                    for (p, q, b, al), o, d in zip(probs, outs, dbs):
                        ops.linear_bwd_weight(p, q, o[:, 4:4 + q.shape[1]], d) if al == 1.0 else wgrad.defer(
                            lambda p=p, q=q, o=o, d=d, al=al: ops.gemm_tn(p, q, o[:, 4:4 + q.shape[1]], dbias=d, alpha=al), p, q, o, d)
                    wgrad.flush()
                    wgrad.join()
                    assert not wgrad.scheduler.tn_pending
            else:
                for (p, q, b, al), o, d in zip(probs, outs, dbs):
                    ops.gemm_tn(p, q, o[:, 4:4 + q.shape[1]], dbias=d, alpha=al)
            torch.cuda.synchronize()
            rounds.append(([o.clone() for o in outs], [None if d is None else d.clone() for d in dbs]))
        return rounds

    ops.LIB.call = counting
    try:
        now, later = run(False), run(True)
    finally:
        ops.LIB.call = real_call
    # the deferred rounds went through the partial-tile entry point and needed far fewer reduce launches than GEMMs (a reduce is issued whenever 40
    # sums or 64 MB of partial tiles are pending, so that the tiles are still cache-resident when they are read)
    assert calls["single"] == 120 and calls["partial"] == 120 and 2 <= calls["batch"] <= 40, calls
    for (o0, d0), (o1, d1) in zip(now, later):
        for a, b in zip(o0, o1):
            assert torch.equal(a, b)
        for a, b in zip(d0, d1):
            assert (a is None and b is None) or torch.equal(a, b)
    p, q, _, al = probs[0]
    close(now[1][0][0][:, 4:4 + q.shape[1]], 0.25 + 2 * al * (p.float().t() @ q.float()), rtol=1e-2, atol=1e-2, what="accumulated twice")
    assert float((now[0][0][0][:, :4] - 0.25).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ attention
def ref_attention(q, k, v, heads, scale, kpm=None, causal=False, shift=0, drop=None):
    B, Tq, D = q.shape
    Tk = k.shape[1]
    qh = q.float().view(B, Tq, heads, 64).transpose(1, 2)
    kh = k.float().view(B, Tk, heads, 64).transpose(1, 2)
    vh = v.float().view(B, Tk, heads, 64).transpose(1, 2)
    s = qh @ kh.transpose(2, 3) * scale
    neg = torch.finfo(torch.float32).min
    if kpm is not None:
        s = s.masked_fill(~kpm.bool().view(B, 1, 1, Tk), neg)
    if causal:
        i = torch.arange(Tq, device=q.device).view(Tq, 1)
        j = torch.arange(Tk, device=q.device).view(1, Tk)
        s = s.masked_fill((j > i + shift).view(1, 1, Tq, Tk), neg)
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    if drop is not None:
        p = p * drop                       # nn.functional.dropout on the probabilities, factor = keep/(1-p) given as data
    return (p @ vh).transpose(1, 2).reshape(B, Tq, D), lse


@pytest.mark.parametrize("B,H,Tq,Tk,causal,masked", [(2, 1, 200, 77, False, False), (1, 3, 577, 145, False, False),
                                                     (2, 12, 40, 40, True, True), (2, 12, 256, 256, True, False),
                                                     (3, 12, 33, 1152, False, True), (2, 1, 1000, 2304, False, False),
                                                     (2, 12, 1, 130, True, True)])
def test_attention_fwd(ops, B, H, Tq, Tk, causal, masked):
    D = H * 64
    q, k, v = dev(rnd(B, Tq, D).to(BF)), dev(rnd(B, Tk, D, seed=1).to(BF)), dev(rnd(B, Tk, D, seed=2).to(BF))
    kpm = None
    if masked:
        kpm = torch.ones(B, Tk, dtype=torch.uint8)
        kpm[0, Tk // 2:] = 0
        kpm[-1, 3:7] = 0
        kpm = kpm.cuda()
    scale = 0.125 if H > 1 else 64 ** -0.5
    out, lse = ops.attention(q, k, v, H, scale, kpm=kpm, causal=causal, need_lse=True)
    ref, ref_lse = ref_attention(q, k, v, H, scale, kpm, causal, Tk - Tq)
    close(out, ref, rtol=2e-2, atol=2e-2, what="attn out")
    close(lse, ref_lse, rtol=1e-3, atol=1e-3, what="lse")


@pytest.mark.parametrize("B,H,Tq,Tk,causal,masked", [(2, 1, 1300, 200, False, False), (1, 3, 577, 145, False, False), (2, 2, 300, 300, True, True),
                                                     (2, 12, 70, 1152, False, True), (1, 2, 100, 33, False, False), (2, 1, 2100, 64, False, False),
                                                     (2, 3, 600, 576, False, False), (1, 2, 256, 256, True, False), (1, 1, 1000, 2304, False, False),
                                                     (2, 2, 130, 700, True, True)])
def test_attention_kernel_generations_agree(ops, B, H, Tq, Tk, causal, masked):
    """cxr_attn_config: the round-3 kernels (64 query rows per wave, one barrier per tile, skipped masked tiles; dQ kernel for unmasked Tq > 1024)
    against the rounds 1-2 kernels on the same inputs: context within one bf16 step of each other (the online softmax advances in 32-key steps
    instead of 64), LSE to fp32 rounding, dQ of the unmasked long calls BIT-identical (same arithmetic, other tiling), everything equally close to
    the fp32 reference. A whole image's keys masked (second half of row 0) exercises the skipped tiles."""
    D = H * 64
    q, k, v = dev(rnd(B, Tq, D).to(BF)), dev(rnd(B, Tk, D, seed=1).to(BF)), dev(rnd(B, Tk, D, seed=2).to(BF))
    do = dev(rnd(B, Tq, D, seed=3).to(BF))
    kpm = None
    if masked:
        kpm = torch.ones(B, Tk, dtype=torch.uint8)
        kpm[0, Tk // 2:] = 0
        kpm[-1, 3:7] = 0
        kpm = kpm.cuda()
    res = {}
    try:
        for ver in (1, 2):
            ops.attention_config(ver, ver)
            out, lse = ops.attention(q, k, v, H, 0.125, kpm=kpm, causal=causal, need_lse=True)
            res[ver] = (out, lse) + tuple(ops.attention_bwd(q, k, v, res[1][0] if ver == 2 else out, do, res[1][1] if ver == 2 else lse, H, 0.125, kpm=kpm,
                                                            causal=causal))
    finally:
        ops.attention_config(2, 2)
    ref, ref_lse = ref_attention(q, k, v, H, 0.125, kpm, causal, Tk - Tq)
    for ver in (1, 2):
        close(res[ver][0], ref, rtol=2e-2, atol=2e-2, what=f"attn out v{ver}")
        close(res[ver][1], ref_lse, rtol=1e-3, atol=1e-3, what=f"lse v{ver}")
    close(res[2][0], res[1][0].float(), rtol=1e-2, atol=1e-2, what="context v2 vs v1")
    close(res[2][1], res[1][1], rtol=1e-5, atol=1e-5, what="lse v2 vs v1")
    for i, name in ((2, "dq"), (3, "dk"), (4, "dv")):
        assert torch.equal(res[2][i], res[1][i]), name          # same O / LSE in: the dK/dV kernel is shared, the dQ kernels do the same arithmetic


def test_attention_e4m3_context_equals_quantised_bf16_context(ops):
    """cxr_attn_fwd_q8_bf16 (frozen e4m3 encoder): the context written as e4m3 by the attention kernel == cxr_quantize_fp8 of its bf16 context."""
    B, H, Tq, Tk = 2, 3, 577, 145
    D = H * 64
    q, k, v = dev(rnd(B, Tq, D).to(BF)), dev(rnd(B, Tk, D, seed=1).to(BF)), dev(rnd(B, Tk, D, seed=2).to(BF))
    out, _ = ops.attention(q, k, v, H, 0.125)
    scale = float(out.float().abs().max()) / 300.0
    want = ops.quantize_fp8(out.view(-1, D), scale)
    got = ops.attention_q8(q, k, v, H, 0.125, scale).view(-1, D)
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


def test_attention_exact_integers(ops):
    # one-hot keys/queries: softmax is (almost) a hard selection, V integers -> catches any key/lane permutation in P.V
    B, H, T = 1, 1, 128
    q = torch.zeros(B, T, 64)
    k = torch.zeros(B, T, 64)
    for t in range(T):
        q[0, t, t % 64] = 30.0
        k[0, t, (t * 7) % 64] = 30.0 if t < 64 else 0.0      # key t<64 is selected by queries with t%64 == (7t)%64
    v = (torch.arange(T * 64).reshape(1, T, 64) % 127).float()
    q, k, v = q.to(BF).cuda(), k.to(BF).cuda(), v.to(BF).cuda()
    out, _ = ops.attention(q, k, v, 1, 1.0)
    ref, _ = ref_attention(q, k, v, 1, 1.0)
    close(out, ref, rtol=1e-2, atol=1e-2, what="attn onehot")


def test_attention_strided_views(ops):
    # q/k/v as column slices of one packed [B,T,3D] buffer and a class-token offset view
    B, T, H = 2, 145, 6
    D = H * 64
    packed = dev(rnd(B, T + 1, 3 * D).to(BF))
    q, k, v = packed[:, 1:, :D], packed[:, 1:, D:2 * D], packed[:, 1:, 2 * D:]
    out, _ = ops.attention(q, k, v, H, 384 ** -0.5)
    ref, _ = ref_attention(q, k, v, H, 384 ** -0.5)
    close(out, ref, what="attn strided")


@pytest.mark.parametrize("B,H,Tq,Tk,causal,masked", [(2, 1, 200, 77, False, False), (1, 3, 577, 145, False, False),
                                                     (2, 12, 40, 40, True, True), (2, 12, 256, 256, True, False),
                                                     (2, 12, 70, 1152, False, True),
                                                     # the CvT-21 @384 stage-1 / stage-2 shapes of the benchmark (1 head, 9216 queries x 2304 keys;
                                                     # 3 heads, 2304 x 576): they select attn_bwd_dq2_kernel<4,0> and the large-grid dK/dV kernels
                                                     (2, 1, 9216, 2304, False, False), (2, 3, 2304, 576, False, False)])
def test_attention_bwd(ops, B, H, Tq, Tk, causal, masked):
    D = H * 64
    q, k, v = dev(rnd(B, Tq, D).to(BF)), dev(rnd(B, Tk, D, seed=1).to(BF)), dev(rnd(B, Tk, D, seed=2).to(BF))
    do = dev(rnd(B, Tq, D, seed=3).to(BF))
    kpm = None
    if masked:
        kpm = torch.ones(B, Tk, dtype=torch.uint8)
        kpm[0, Tk // 2:] = 0
        kpm[-1, 3:7] = 0
        kpm = kpm.cuda()
    scale = 0.125 if H > 1 else 64 ** -0.5
    out, lse = ops.attention(q, k, v, H, scale, kpm=kpm, causal=causal, need_lse=True)
    dq, dk, dv = ops.attention_bwd(q, k, v, out, do, lse, H, scale, kpm=kpm, causal=causal)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    ref, _ = ref_attention(qr, kr, vr, H, scale, kpm, causal, Tk - Tq)
    ref.backward(do.float())
    close(dq, qr.grad, rtol=3e-2, atol=3e-2, what="dq")
    close(dk, kr.grad, rtol=3e-2, atol=3e-2, what="dk")
    close(dv, vr.grad, rtol=3e-2, atol=3e-2, what="dv")


@pytest.mark.parametrize("B,H,Tq,Tk,causal,masked", [(2, 12, 40, 40, True, True), (2, 12, 256, 256, True, False), (2, 12, 70, 1152, False, True),
                                                     (1, 3, 200, 77, False, False), (1, 1, 9216, 2304, False, False), (1, 3, 2304, 576, False, False)])
def test_attention_dropout_fwd_bwd(ops, B, H, Tq, Tk, causal, masked):
    """Train-mode dropout on the probabilities: forward and both backward kernels regenerate the SAME counter-based mask that
    cxr_dropout_mask materialises (rows = (b*H+h, query), cols = key), and match autograd of softmax -> mask/(1-p) -> .V"""
    D = H * 64
    q, k, v = dev(rnd(B, Tq, D).to(BF)), dev(rnd(B, Tk, D, seed=1).to(BF)), dev(rnd(B, Tk, D, seed=2).to(BF))
    do = dev(rnd(B, Tq, D, seed=3).to(BF))
    kpm = None
    if masked:
        kpm = torch.ones(B, Tk, dtype=torch.uint8)
        kpm[0, Tk // 2:] = 0
        kpm = kpm.cuda()
    seed = torch.full((1,), 123457, dtype=torch.int32, device="cuda")
    pdrop, site, t0 = 0.1, 18, 5
    drop = (pdrop, seed, site, t0)
    out, lse = ops.attention(q, k, v, H, 0.125, kpm=kpm, causal=causal, need_lse=True, drop=drop)
    fac = ops.dropout_mask(B * H * Tq, Tk, pdrop, seed, site, Tq, t0, factor=True).view(B, H, Tq, Tk)
    keep_rate = (fac > 0).float().mean().item()
    assert abs(keep_rate - 0.9) < 4 * math.sqrt(0.09 / fac.numel()) + 1e-4, keep_rate
    assert torch.all((fac == 0) | ((fac - 1 / 0.9).abs() < 1e-6))
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    ref, ref_lse = ref_attention(qr, kr, vr, H, 0.125, kpm, causal, Tk - Tq, drop=fac)
    close(out, ref, what="attn dropout out")
    close(lse, ref_lse, rtol=1e-3, atol=1e-3, what="lse is dropout-free")
    dq, dk, dv = ops.attention_bwd(q, k, v, out, do, lse, H, 0.125, kpm=kpm, causal=causal, drop=drop)
    ref.backward(do.float())
    close(dq, qr.grad, rtol=3e-2, atol=3e-2, what="dq (dropout)")
    close(dk, kr.grad, rtol=3e-2, atol=3e-2, what="dk (dropout)")
    close(dv, vr.grad, rtol=3e-2, atol=3e-2, what="dv (dropout)")
    # another seed / site / position offset gives another mask; p = 0 is the plain kernel
    other = ops.dropout_mask(B * H * Tq, Tk, pdrop, seed, site + 1, Tq, t0).view(-1)
    same = (other == (fac.view(-1) > 0).to(torch.uint8)).float().mean().item()
    assert abs(same - 0.82) < 0.02, same                  # independent masks agree on 0.9^2 + 0.1^2 of the elements
    plain, _ = ops.attention(q, k, v, H, 0.125, kpm=kpm, causal=causal)
    off, _ = ops.attention(q, k, v, H, 0.125, kpm=kpm, causal=causal, drop=(0.0, None, 0, 0))
    assert torch.equal(plain, off)


def test_gemm_epilogue_dropout_and_droppath(ops):
    M, N, K, T = 192, 768, 256, 24
    a, w = dev(rnd(M, K).to(BF)), dev(rnd(N, K, seed=1, scale=0.1).to(BF))
    bias, res = dev(rnd(N, seed=2)), dev(rnd(M, N, seed=3).to(BF))
    seed = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    base = a.float() @ w.float().t() + bias
    fac = ops.dropout_mask(M, N, 0.1, seed, 27, T, 2, factor=True)
    out = ops.gemm_nt(a, w, bias=bias, residual=res, drop=(0.1, seed, 27, T, 2))
    close(out, base * fac + res.float(), what="gemm epilogue dropout")
    scale = dev(rnd(M // T, seed=4).abs())
    rs = scale.repeat_interleave(T)[:, None]
    close(ops.gemm_nt(a, w, bias=bias, residual=res, row_scale=(scale, T, False)), base * rs + res.float(), what="DropPath on the branch")
    close(ops.gemm_nt(a, w, bias=bias, residual=res, row_scale=(scale, T, True)), (base + res.float()) * rs, what="DropPath on the layer output")


def test_dropout_add_and_droppath(ops):
    R, C, T = 96, 768, 24
    y, res = dev(rnd(R, C).to(BF)), dev(rnd(R, C, seed=1).to(BF))
    seed = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    fac = ops.dropout_mask(R, C, 0.1, seed, 33, T, factor=True)
    out = ops.dropout_add(y, res, 0.1, seed, 33, T)
    close(out, res.float() + fac * y.float(), rtol=1e-2, atol=2e-2, what="dropout_add")
    back = ops.dropout_add(y, None, 0.1, seed, 33, T)
    close(back, fac * y.float(), rtol=1e-2, atol=2e-2, what="dropout backward")
    assert abs((fac > 0).float().mean().item() - 0.9) < 0.01
    # the mask of position t of sequence b does not depend on how rows are batched: a [B,1] decode step at t0 = t sees row (b, t) of the [B,T] pass
    step = ops.dropout_mask(R // T, C, 0.1, seed, 33, 1, 7)
    full = ops.dropout_mask(R, C, 0.1, seed, 33, T).view(R // T, T, C)
    assert torch.equal(step, full[:, 7, :])
    # DropPath: per-image scale
    scale = torch.tensor([1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9], device="cuda")
    out = ops.dropout_add(y, res, 0.0, None, 0, T, row_scale=scale)
    close(out, res.float() + scale.repeat_interleave(T)[:, None] * y.float(), rtol=1e-2, atol=2e-2, what="droppath")
    inplace = y.clone()
    ops.dropout_add(inplace, None, 0.0, None, 0, T, row_scale=scale, out=inplace)
    close(inplace, scale.repeat_interleave(T)[:, None] * y.float(), rtol=1e-2, atol=2e-2, what="droppath in place")


@pytest.mark.parametrize("M,N,K", [(16, 768, 768), (1, 768, 768), (16, 3072, 768), (16, 768, 3072), (32, 30000, 768), (50, 768, 768), (64, 2304, 768)])
def test_gemm_skinny_decode(ops, M, N, K):
    a, w = dev(rnd(M, K).to(BF)), dev(rnd(N, K, seed=1, scale=0.05).to(BF))
    bias, res = dev(rnd(N, seed=2)), dev(rnd(M, N, seed=3).to(BF))
    base = a.float() @ w.float().t() + bias
    close(ops.gemm_skinny(a, w, bias=bias), base, rtol=1e-2, atol=1e-2, what="skinny bias")
    close(ops.gemm_skinny(a, w, bias=bias, act=1, residual=res), torch.nn.functional.gelu(base) + res.float(), what="skinny gelu+res")
    close(ops.gemm_skinny(a, w, out_f32=True), a.float() @ w.float().t(), rtol=1e-2, atol=1e-2, what="skinny f32")
    cache = torch.zeros(M, 7, N, dtype=BF, device="cuda")                       # write into a strided row (KV-cache append)
    ops.gemm_skinny(a, w, bias=bias, out=cache[:, 3, :])
    close(cache[:, 3, :], base, rtol=1e-2, atol=1e-2, what="skinny strided out")
    assert bool((cache[:, 2, :] == 0).all())


@pytest.mark.parametrize("R", [96, 528])          # <= 256 rows: one workgroup per row (decode); above: one wave per row (teacher forcing)
def test_lora_train_mode_kernels(ops, R):
    """peft Linear under train(): y = base(x) + s * B(A(dropout(x))) and its backward, from the three rank-8 kernels of csrc/lora.hip."""
    K, N, T, r, s_ = 768, 768, 24, 8, 4.0
    x, dy = dev(rnd(R, K).to(BF)), dev(rnd(R, N, seed=1).to(BF))
    A, Bm = dev(rnd(r, K, seed=2, scale=0.05).to(BF)), dev(rnd(N, r, seed=3, scale=0.05).to(BF))
    A2 = dev(rnd(r, K, seed=4, scale=0.05).to(BF))
    seed = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    f = ops.dropout_mask(R, K, 0.1, seed, 21, T, factor=True)
    f2 = ops.dropout_mask(R, K, 0.1, seed, 22, T, factor=True)
    t, t2 = ops.lora_down(x, A, drop0=(0.1, 21), W1=A2, drop1=(0.1, 22), rows_per_b=T, seed=seed, scale=s_)
    close(t, s_ * (x.float() * f) @ A.float().t(), rtol=1e-3, atol=1e-3, what="lora down")
    close(t2, s_ * (x.float() * f2) @ A2.float().t(), rtol=1e-3, atol=1e-3, what="lora down (second problem)")
    y0 = dev(rnd(R, N, seed=5).to(BF))
    y = ops.lora_up_add_(y0.clone(), t, Bm, True)
    close(y, y0.float() + t @ Bm.float().t(), what="lora up")
    # backward pieces
    dt = ops.lora_down(dy, Bm, w_is_b=True, scale=s_)
    close(dt, s_ * dy.float() @ Bm.float(), rtol=1e-3, atol=1e-3, what="dt = s dy B")
    dB = torch.zeros(N, r, device="cuda")
    ops.lora_outer_into(dy, t, dB, r, 1)
    close(dB, dy.float().t() @ t, rtol=1e-3, atol=1e-3, what="dB")
    dA = torch.zeros(r, K, device="cuda")
    ops.lora_outer_into(x, dt, dA, 1, K, drop=(0.1, 21), rows_per_b=T, seed=seed)
    close(dA, dt.t() @ (x.float() * f), rtol=1e-3, atol=1e-3, what="dA")
    dx0 = dev(rnd(R, K, seed=6).to(BF))
    dx = ops.lora_up_add_(dx0.clone(), dt, A, False, drop=(0.1, 21), rows_per_b=T, seed=seed)
    close(dx, dx0.float() + f * (dt @ A.float()), what="dx")
    # LayerNorm of the raw row inside the down projection (decode path) and the rank-8 term in the decode GEMM epilogue
    g_, b_ = dev(1 + 0.1 * rnd(K, seed=7)), dev(0.1 * rnd(K, seed=8))
    raw = dev((rnd(32, K, seed=9) * 2 + 0.3).to(BF))
    ln = torch.nn.functional.layer_norm(raw.float(), (K,), g_, b_, 1e-12).to(BF).float()
    fl = ops.dropout_mask(32, K, 0.1, seed, 21, 1, 7, factor=True)
    tl = ops.lora_down(raw, A, drop0=(0.1, 21), rows_per_b=1, tpos0=7, seed=seed, ln=(g_, b_, 1e-12), scale=s_)
    close(tl, s_ * (ln * fl) @ A.float().t(), rtol=2e-3, atol=2e-3, what="lora down with fused LayerNorm")
    w, bias = dev(rnd(N, K, seed=10, scale=0.05).to(BF)), dev(rnd(N, seed=11))
    q, k, v = (torch.empty(32, N, dtype=BF, device="cuda") for _ in range(3))
    ops.gemm_skinny3(raw, w, bias, q, w, bias, k, w, bias, v, ln_a=(g_, b_, 1e-12, None), lora0=(tl, Bm))
    base = ln @ w.float().t() + bias
    close(q, base + tl @ Bm.float().t(), what="skinny3 + rank-8 epilogue")
    close(k, base, what="skinny3 problem without LoRA")


@pytest.mark.parametrize("R,K", [(528, 768), (4080, 768), (1000, 64), (300, 1024)])
def test_lora_kernels_with_several_problems_per_launch(ops, R, K):
    """The teacher-forced forms of the three rank-8 contractions (two adapters per launch: down projection on the matrix cores, both rank-8 updates of dx
    in one read-modify-write, dB / dA of both adapters in one launch) against fp32 torch with the materialised dropout masks, and against the
    one-problem kernels."""
    N, T, r, s_ = K, 24, 8, 4.0
    x, dq, dk = dev(rnd(R, K).to(BF)), dev(rnd(R, N, seed=1).to(BF)), dev(rnd(R, N, seed=11).to(BF))
    A, A2 = dev(rnd(r, K, seed=2, scale=0.05).to(BF)), dev(rnd(r, K, seed=4, scale=0.05).to(BF))
    Bq, Bk = dev(rnd(N, r, seed=3, scale=0.05).to(BF)), dev(rnd(N, r, seed=13, scale=0.05).to(BF))
    seed = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    f = ops.dropout_mask(R, K, 0.1, seed, 21, T, factor=True)
    f2 = ops.dropout_mask(R, K, 0.1, seed, 22, T, factor=True)
    # forward: t = s * dropout(x) A^T for both adapters, then q += t Bq^T, k += t2 Bk^T (separate outputs; one of them a column view of a wider matrix)
    t, t2 = ops.lora_down_multi([dict(x=x, W=A, drop=(0.1, 21)), dict(x=x, W=A2, drop=(0.1, 22))], rows_per_b=T, seed=seed, scale=s_)
    close(t, s_ * (x.float() * f) @ A.float().t(), rtol=1e-3, atol=1e-3, what="down, first adapter")
    close(t2, s_ * (x.float() * f2) @ A2.float().t(), rtol=1e-3, atol=1e-3, what="down, second adapter")
    if K <= 1024 and R > 256:
        o, o2 = ops.lora_down(x, A, drop0=(0.1, 21), W1=A2, drop1=(0.1, 22), rows_per_b=T, seed=seed, scale=s_)
        close(t, o, rtol=1e-4, atol=1e-4, what="down vs the one-wave-per-row kernel")
    q0 = dev(rnd(R, N, seed=5).to(BF))
    wide = dev(rnd(R, 2 * N + 8, seed=6).to(BF))
    k0 = wide[:, N + 8:]
    qk = [q0.clone(), wide.clone()]
    ops.lora_up_add_multi_([dict(y=qk[0], t=t, W=Bq, w_is_b=True), dict(y=qk[1][:, N + 8:], t=t2, W=Bk, w_is_b=True)])
    close(qk[0], q0.float() + t @ Bq.float().t(), what="up, first output")
    close(qk[1][:, N + 8:], k0.float() + t2 @ Bk.float().t(), what="up, second output (a column view)")
    assert torch.equal(qk[1][:, :N + 8], wide[:, :N + 8])
    # backward: dt = s * dy B for both (different inputs), dB / dA of both in one launch, dx += mask * (dt A) of both in one pass
    dt, dt2 = ops.lora_down_multi([dict(x=dq, W=Bq, w_is_b=True), dict(x=dk, W=Bk, w_is_b=True)], scale=s_)
    close(dt, s_ * dq.float() @ Bq.float(), rtol=1e-3, atol=1e-3, what="dt, first adapter")
    close(dt2, s_ * dk.float() @ Bk.float(), rtol=1e-3, atol=1e-3, what="dt, second adapter")
    dB, dB2, dA, dA2 = torch.zeros(N, r, device="cuda"), torch.ones(N, r, device="cuda"), torch.zeros(r, K, device="cuda"), torch.zeros(r, K, device="cuda")
    ops.lora_outer_multi_into([dict(a=dq, t=t, G=dB, g_ks=r, g_rs=1), dict(a=x, t=dt, G=dA, g_ks=1, g_rs=K, drop=(0.1, 21)),
                               dict(a=dk, t=t2, G=dB2, g_ks=r, g_rs=1), dict(a=x, t=dt2, G=dA2, g_ks=1, g_rs=K, drop=(0.1, 22))], rows_per_b=T, seed=seed)
    tol = dict(rtol=2e-3, atol=2e-3 * (R / 500.0) ** 0.5)
    close(dB, dq.float().t() @ t, what="dB", **tol)
    close(dB2, 1.0 + dk.float().t() @ t2, what="dB of the second adapter accumulates", **tol)
    close(dA, dt.t() @ (x.float() * f), what="dA", **tol)
    close(dA2, dt2.t() @ (x.float() * f2), what="dA of the second adapter", **tol)
    dx0 = dev(rnd(R, K, seed=6).to(BF))
    dx = dx0.clone()
    ops.lora_up_add_multi_([dict(y=dx, t=dt, W=A, drop=(0.1, 21)), dict(y=dx, t=dt2, W=A2, drop=(0.1, 22))], rows_per_b=T, seed=seed)
    close(dx, dx0.float() + f * (dt @ A.float()) + f2 * (dt2 @ A2.float()), what="dx from both adapters")
    one = dx0.clone()
    ops.lora_up_add_multi_([dict(y=one, t=dt, W=A, drop=(0.1, 21))], rows_per_b=T, seed=seed)
    close(one, dx0.float() + f * (dt @ A.float()), what="dx from one adapter")


@pytest.mark.parametrize("M", [1, 16, 32, 50])
def test_gemm_skinny_fused_layernorm(ops, M):
    """LayerNorm folded into the decode GEMMs: `ln_a` normalises the raw A rows inside the kernel and publishes (mean, rstd);
    `ln_r` applies the same LayerNorm to the residual operand."""
    K, N = 768, 768
    raw = dev((rnd(M, K) * 2 + 0.3).to(BF))
    w, bias = dev(rnd(N, K, seed=1, scale=0.05).to(BF)), dev(rnd(N, seed=2))
    g, b = dev(1 + 0.1 * rnd(K, seed=3)), dev(0.1 * rnd(K, seed=4))
    ln = torch.nn.functional.layer_norm(raw.float(), (K,), g, b, 1e-12)
    stats = torch.zeros(M, 2, device="cuda")
    out = ops.gemm_skinny(raw, w, bias=bias, act=1, ln_a=(g, b, 1e-12, stats))
    ref = torch.nn.functional.gelu(ln.to(BF).float() @ w.float().t() + bias)
    close(out, ref, what="skinny ln_a")
    close(stats[:, 0], raw.float().mean(1), rtol=1e-4, atol=1e-4, what="published mean")
    close(stats[:, 1], (raw.float().var(1, unbiased=False) + 1e-12).rsqrt(), rtol=1e-4, atol=1e-4, what="published rstd")
    y, _ = ops.layernorm(raw, g, b, 1e-12)
    close(out, ops.gemm_skinny(y, w, bias=bias, act=1), rtol=5e-3, atol=5e-3, what="fused vs separate LayerNorm kernel")
    x2 = dev(rnd(M, K, seed=5).to(BF))
    out2 = ops.gemm_skinny(x2, w, bias=bias, residual=raw, ln_r=(stats, g, b))
    close(out2, x2.float() @ w.float().t() + bias + ln, what="skinny ln_r")
    q, k, v = (torch.empty(M, N, dtype=BF, device="cuda") for _ in range(3))
    ops.gemm_skinny3(raw, w, bias, q, w, None, k, w, bias, v, ln_a=(g, b, 1e-12, None))
    close(q, ln.to(BF).float() @ w.float().t() + bias, what="skinny3 ln_a")
    close(k, ln.to(BF).float() @ w.float().t(), what="skinny3 ln_a (no bias)")


@pytest.mark.parametrize("B,H,Tk,masked", [(16, 12, 1152, True), (3, 12, 7, False), (2, 12, 261, True), (64, 12, 100, False)])
def test_attention_decode_single_query(ops, B, H, Tk, masked):
    D = H * 64
    q, kv = dev(rnd(B, 1, D).to(BF)), dev(rnd(B, Tk + 5, 2 * D, seed=1).to(BF))
    k, v = kv[:, :Tk, :D], kv[:, :Tk, D:]
    kpm = None
    if masked:
        kpm = torch.ones(B, Tk, dtype=torch.uint8)
        kpm[0, Tk // 2:] = 0
        kpm[-1, 1:3] = 0
        kpm = kpm.cuda()
    out = ops.attention_decode(q, k, v, H, 0.125, kpm=kpm)
    ref, _ = ref_attention(q, k, v, H, 0.125, kpm)
    close(out, ref[:, 0], what="attn decode")
    full, _ = ops.attention(q, k, v, H, 0.125, kpm=kpm)
    close(out, full[:, 0], rtol=1e-2, atol=1e-2, what="attn decode vs tiled kernel")
    # two query rows per K/V row (sample + greedy halves of one SCST step share the cross-attention K/V): rows b and b + B read K/V row b
    q2 = torch.cat([q, dev(rnd(B, 1, D, seed=9).to(BF))], 0)
    both = ops.attention_decode(q2, k, v, H, 0.125, kpm=kpm)
    close(both[:B], out, rtol=2e-3, atol=2e-3, what="attn decode, first half of a shared launch")
    ref2, _ = ref_attention(q2[B:], k, v, H, 0.125, kpm)
    close(both[B:], ref2[:, 0], what="attn decode, shared K/V")
    seed = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    dr = ops.attention_decode(q2, k, v, H, 0.125, kpm=kpm, drop=(0.1, seed, 18, 33))
    fac = ops.dropout_mask(2 * B * H, Tk, 0.1, seed, 18, 1, 33, factor=True).view(2 * B, H, 1, Tk)
    kk, vv = torch.cat([k, k], 0), torch.cat([v, v], 0)
    refd, _ = ref_attention(q2, kk, vv, H, 0.125, None if kpm is None else torch.cat([kpm, kpm], 0), drop=fac)
    close(dr, refd[:, 0], what="attn decode dropout (same hash as the tiled kernel / cxr_dropout_mask)")


# ------------------------------------------------------------------------------------------------ decode-step linear layers (csrc/decode_gemm.hip)
def _dal(ops, x):
    return ops.dec_to_dal(x, want_stats=True)


@pytest.mark.parametrize("M", [1, 16, 32, 50, 64])
def test_dec_gemm_fold_residual_stats(ops, M):
    """cxr_dec_gemm_bf16: LayerNorm folded into packed weights (rstd * (x W'^T - mean * colsum) + b'), LayerNorm on the residual operand, published
    per-tile row statistics, decode-activation-layout input / output, grouped problems writing strided row-major rows (KV cache)."""
    K, N = 768, 768
    raw = dev((rnd(M, K) * 2 + 0.3).to(BF))
    w, bias = dev(rnd(N, K, seed=1, scale=0.05).to(BF)), dev(rnd(N, seed=2))
    g, b = dev(1 + 0.1 * rnd(K, seed=3)), dev(0.1 * rnd(K, seed=4))
    ln = torch.nn.functional.layer_norm(raw.float(), (K,), g, b, 1e-12)
    a_dal, st = _dal(ops, raw)
    assert torch.equal(ops.dec_from_dal(a_dal, M, K), raw)                                   # layout round trip is exact
    close(st[..., 0].sum(0), raw.float().sum(1), rtol=1e-5, atol=1e-3, what="tile sums")
    wf, bcf = ops.dec_pack_weight(w, g, b, bias)
    (out,), ost = ops.dec_gemm(a_dal, M, K, [dict(wp=wf, bc=bcf, N=N, fold=True)], act=1, stats=st, eps=1e-12, out_stats=True)
    ref = torch.nn.functional.gelu(ln @ w.float().t() + bias)
    got = ops.dec_from_dal(out, M, N)
    close(got, ref, rtol=1e-2, what="LN-folded GEMM + GELU")
    for mt_hint in (1, 2):                        # one 16-row tile per workgroup / all rows in one workgroup: the same numbers
        (o2,), ost2 = ops.dec_gemm(a_dal, M, K, [dict(wp=wf, bc=bcf, N=N, fold=True)], act=1, stats=st, eps=1e-12, out_stats=True, mt_hint=mt_hint)
        assert torch.equal(ops.dec_from_dal(o2, M, N), got) and torch.equal(ost2, ost)
    # the published statistics describe the rounded output: Chan-combined they give its mean / variance
    gf = got.float()
    mean = ost[..., 0].sum(0) / N
    m2 = (ost[..., 1] + 16.0 * (ost[..., 0] / 16.0 - mean) ** 2).sum(0)
    close(mean, gf.mean(1), rtol=1e-4, atol=1e-4, what="published mean")
    close(m2 / N, gf.var(1, unbiased=False), rtol=1e-3, atol=1e-4, what="published variance")
    # plain weights + LayerNorm(residual) + fp32 row-major output
    x2 = dev(rnd(M, K, seed=5).to(BF))
    x2d, _ = ops.dec_to_dal(x2)
    wp, bcp = ops.dec_pack_weight(w, None, None, bias)
    rgb = torch.stack([g, b], 1).contiguous()
    (o32,), _ = ops.dec_gemm(x2d, M, K, [dict(wp=wp, bc=bcp, N=N)], out_f32=True, stats=st, eps=1e-12, residual=a_dal, rgb=rgb)
    close(o32, x2.float() @ w.float().t() + bias + ln, rtol=5e-3, what="plain GEMM + LN(residual)")
    (o_raw,), _ = ops.dec_gemm(x2d, M, K, [dict(wp=wp, bc=bcp, N=N)], out_f32=True, residual=a_dal)
    close(o_raw, x2.float() @ w.float().t() + bias + raw.float(), rtol=5e-3, what="plain GEMM + raw residual")
    # three grouped problems, k / v landing in strided cache rows; output dropout with the shared hash
    cache = torch.zeros(M, 5, 2 * N, dtype=BF, device="cuda")
    q = torch.empty(M, N, dtype=BF, device="cuda")
    ops.dec_gemm(a_dal, M, K, [dict(wp=wf, bc=bcf, N=N, fold=True, out=q), dict(wp=wf, bc=bcf, N=N, fold=True, out=cache[:, 3, :N]),
                              dict(wp=wp, bc=bcp, N=N, out=cache[:, 3, N:])], stats=st, eps=1e-12)
    close(q, ln @ w.float().t() + bias, rtol=1e-2, what="grouped q")
    close(cache[:, 3, :N], q, rtol=1e-6, atol=1e-6, what="grouped k (strided rows)")
    close(cache[:, 3, N:], raw.float() @ w.float().t() + bias, rtol=1e-2, what="grouped v (unfolded problem in the same launch)")
    assert float(cache[:, 2].abs().sum()) == 0 and float(cache[:, 4].abs().sum()) == 0
    seed = torch.full((1,), 11, dtype=torch.int32, device="cuda")
    (od,), _ = ops.dec_gemm(x2d, M, K, [dict(wp=wp, bc=bcp, N=N)], out_f32=True, residual=a_dal, drop=(0.1, seed, 19, 7))
    f = ops.dropout_mask(M, N, 0.1, seed, 19, 1, 7, factor=True)
    close(od, (x2.float() @ w.float().t() + bias) * f + raw.float(), rtol=5e-3, what="output dropout (hash of cxr_dropout_mask)")


def test_dec_gemm_wide_and_vocab(ops):
    """K = 3072 (FFN output projection, 16 waves) and a vocabulary-sized N that is not a multiple of the 64-column workgroup tile."""
    M = 32
    x = dev(rnd(M, 3072, scale=0.5).to(BF))
    w, bias = dev(rnd(768, 3072, seed=1, scale=0.03).to(BF)), dev(rnd(768, seed=2))
    xd, _ = ops.dec_to_dal(x)
    wp, bc = ops.dec_pack_weight(w, None, None, bias)
    (o,), _ = ops.dec_gemm(xd, M, 3072, [dict(wp=wp, bc=bc, N=768)], out_f32=True)
    close(o, x.float() @ w.float().t() + bias, rtol=5e-3, what="K = 3072")
    for V in (30000, 1000):
        h = dev((rnd(M, 768, seed=3) + 0.2).to(BF))
        hd, st = ops.dec_to_dal(h, want_stats=True)
        g, b = dev(1 + 0.1 * rnd(768, seed=4)), dev(0.1 * rnd(768, seed=5))
        wv, bv = dev(rnd(V, 768, seed=6, scale=0.05).to(BF)), dev(rnd(V, seed=7))
        wf, bcf = ops.dec_pack_weight(wv, g, b, bv)
        ref = torch.nn.functional.layer_norm(h.float(), (768,), g, b, 1e-12) @ wv.float().t() + bv
        for nc in (1, 4):
            (lg,), _ = ops.dec_gemm(hd, M, 768, [dict(wp=wf, bc=bcf, N=V, fold=True)], out_f32=True, stats=st, eps=1e-12, nc_hint=nc)
            close(lg, ref, rtol=1e-2, what=f"LM head V={V} nc={nc}")


def test_dec_gemm_lora_train_mode(ops):
    """Train-mode LoRA inside the folded GEMM: C += s * dropout(LN(x)) A^T B^T with the branch's own input mask (hash of csrc/lora.hip)."""
    M, K, N, s_ = 32, 768, 768, 4.0
    raw = dev((rnd(M, K) * 2 + 0.3).to(BF))
    w, bias = dev(rnd(N, K, seed=1, scale=0.05).to(BF)), dev(rnd(N, seed=2))
    g, b = dev(1 + 0.1 * rnd(K, seed=3)), dev(0.1 * rnd(K, seed=4))
    A, Bm = dev(rnd(8, K, seed=5, scale=0.05).to(BF)), dev(rnd(N, 8, seed=6, scale=0.05).to(BF))
    ln = torch.nn.functional.layer_norm(raw.float(), (K,), g, b, 1e-12)
    seed = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    a_dal, st = _dal(ops, raw)
    wf, bcf = ops.dec_pack_weight(w, g, b, bias)
    Ap = ops.dec_pack_lora(A, g, b)
    for p_ in (0.0, 0.1):
        fl = ops.dropout_mask(M, K, p_, seed, 21, 1, 7, factor=True) if p_ else torch.ones(M, K, device="cuda")
        q = torch.empty(M, N, dtype=BF, device="cuda")
        v = torch.empty(M, N, dtype=BF, device="cuda")
        ops.dec_gemm(a_dal, M, K, [dict(wp=wf, bc=bcf, N=N, fold=True, out=q, lora=(Ap, Bm, 21)), dict(wp=wf, bc=bcf, N=N, fold=True, out=v)],
                     stats=st, eps=1e-12, lora=(p_, seed, s_, 7))
        base = ln @ w.float().t() + bias
        close(q, base + s_ * ((ln * fl) @ A.float().t()) @ Bm.float().t(), rtol=1e-2, what=f"folded LoRA branch p={p_}")
        close(v, base, rtol=1e-2, what="problem without LoRA in the same launch")
    # no LayerNorm in front (first decoder layer: the embedding output is already normalised)
    Ap0 = ops.dec_pack_lora(A)
    wp, bcp = ops.dec_pack_weight(w, None, None, bias)
    fl = ops.dropout_mask(M, K, 0.1, seed, 22, 1, 3, factor=True)
    q = torch.empty(M, N, dtype=BF, device="cuda")
    ops.dec_gemm(a_dal, M, K, [dict(wp=wp, bc=bcp, N=N, out=q, lora=(Ap0, Bm, 22))], lora=(0.1, seed, s_, 3))
    close(q, raw.float() @ w.float().t() + bias + s_ * ((raw.float() * fl) @ A.float().t()) @ Bm.float().t(), rtol=1e-2, what="LoRA without fold")


@pytest.mark.parametrize("B,H,Tk,wg", [(16, 12, 1152, -576), (16, 12, 1152, 576), (16, 12, 1152, 288), (16, 12, 1152, 256), (4, 12, 72, -576),
                                       (3, 12, 300, 256), (3, 12, 300, -256)])
def test_attention_decode_geometries_and_layout(ops, B, H, Tk, wg):
    """Every workgroup geometry of the single-query attention kernel (split + merge, looping) gives the same result, also when written in the
    decode activation layout."""
    D = H * 64
    q, kv = dev(rnd(2 * B, 1, D).to(BF)), dev(rnd(B, Tk, 2 * D, seed=1).to(BF))
    k, v = kv[:, :, :D], kv[:, :, D:]
    kpm = torch.ones(B, Tk, dtype=torch.uint8)
    kpm[0, Tk // 2:] = 0
    kpm[-1, 1:3] = 0
    kpm = kpm.cuda()
    ref, _ = ref_attention(q, torch.cat([k, k], 0), torch.cat([v, v], 0), H, 0.125, torch.cat([kpm, kpm], 0))
    out = ops.attention_decode(q, k, v, H, 0.125, kpm=kpm, wg_keys=wg)
    close(out, ref[:, 0], what=f"attn decode wg_keys={wg}")
    od = ops.attention_decode(q, k, v, H, 0.125, kpm=kpm, wg_keys=wg, out_dal=True)
    assert torch.equal(ops.dec_from_dal(od, 2 * B, D), out)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C", [64, 128, 192, 384, 768])
def test_layernorm_fwd_bwd(ops, C):
    rows = 1000 + C // 64
    x = dev((rnd(rows, C) * 2 + 0.5).to(BF))
    g, b = dev(1 + 0.1 * rnd(C, seed=1)), dev(0.1 * rnd(C, seed=2))
    y, stats = ops.layernorm(x, g, b, 1e-5, need_stats=True)
    xr = x.float().requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (C,), gr, br, 1e-5)
    close(y, ref, what=f"ln fwd C={C}")
    dy = dev(rnd(rows, C, seed=3).to(BF))
    add = dev(rnd(rows, C, seed=4).to(BF))
    ref.backward(dy.float())
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx = ops.layernorm_bwd(x, dy, g, stats, dg, db, add=add)
    close(dx, xr.grad + add.float(), what=f"ln dx C={C}")
    close(dg, gr.grad, rtol=1e-2, atol=1e-2, what="ln dgamma")
    close(db, br.grad, rtol=1e-2, atol=1e-2, what="ln dbeta")
    # second output: the forward dropout mask / DropPath factor of the branch fed by this LayerNorm's input, re-applied to dx
    seed = torch.full((1,), 31, dtype=torch.int32, device="cuda")
    T = 8
    r8 = (rows // T) * T
    dx1, dx2 = ops.layernorm_bwd(x[:r8], dy[:r8], g, stats[:r8], None, None, add=add[:r8], drop=(0.1, seed, 44, T, 3))
    assert torch.equal(dx1, dx[:r8])
    close(dx2, dx1.float() * ops.dropout_mask(r8, C, 0.1, seed, 44, T, 3, factor=True), rtol=1e-2, atol=2e-2, what="ln dx2 (dropout)")
    scale = dev(rnd(r8 // T, seed=9).abs())
    dx1, dx2 = ops.layernorm_bwd(x[:r8], dy[:r8], g, stats[:r8], None, None, row_scale=(scale, T))
    close(dx2, dx1.float() * scale.repeat_interleave(T)[:, None], rtol=1e-2, atol=2e-2, what="ln dx2 (DropPath)")


# ------------------------------------------------------------------------------------------------ conv pieces
def test_im2col_pixels_matches_conv(ops):
    px = dev(rnd(2, 3, 96, 96))
    w = dev(rnd(64, 3, 7, 7, seed=1, scale=0.1))
    col, Ho, Wo = ops.im2col_pixels(px, 7, 4, 2, 192)
    wp = torch.zeros(64, 192, device="cuda")
    wp[:, :147] = w.view(64, -1)
    out = ops.gemm_nt(col, wp.to(BF))
    ref = torch.nn.functional.conv2d(px, w.to(BF).float(), stride=4, padding=2)
    ref = ref.flatten(2).transpose(1, 2).reshape(-1, 64)
    close(out, ref, what="patch conv 7x7")
    # the col matrix itself, bit for bit (bf16 of the gathered pixel, zero padding): the row-staged kernel, odd widths (scalar staging), other
    # kernel sizes / strides, and a geometry too large for LDS staging (the gather kernel)
    for (Bn, Cin, H, W, ks, st, pad, kpad) in ((2, 3, 384, 384, 7, 4, 2, 192), (3, 3, 50, 37, 7, 4, 2, 152), (2, 4, 33, 64, 3, 2, 1, 40), (1, 2, 20, 24, 5, 1, 2, 56),
                                                (1, 16, 40, 1024, 7, 4, 2, 784)):
        px = dev(rnd(Bn, Cin, H, W, seed=H + W))
        col, Ho, Wo = ops.im2col_pixels(px, ks, st, pad, kpad)
        un = torch.nn.functional.unfold(px, ks, padding=pad, stride=st).transpose(1, 2).reshape(-1, Cin * ks * ks)      # k = c*KS*KS + ky*KS + kx
        assert (Ho, Wo) == ((H + 2 * pad - ks) // st + 1, (W + 2 * pad - ks) // st + 1)
        assert torch.equal(col[:, :Cin * ks * ks], un.to(BF)), (Bn, Cin, H, W, ks, st, pad)
        assert float(col[:, Cin * ks * ks:].float().abs().sum()) == 0


@pytest.mark.parametrize("Bn,H,W", [(2, 96, 96), (1, 384, 384), (3, 100, 52), (2, 8, 384)])
def test_patch_embedding_in_one_launch(ops, Bn, H, W):
    """cxr_patch_embed_s1_f32 (round 4): Conv2d(3, 64, 7, stride 4, padding 2) + bias + LayerNorm(64) of the CvT stage-1 embedding as a direct
    convolution on the matrix cores, against torch's conv2d / layer_norm on the same bf16-rounded pixels and weights (fp32 accumulation both sides;
    e is rounded to bf16 before the LayerNorm, as when a GEMM wrote it), and against the im2col + GEMM + LayerNorm path it replaces. Partial last
    pixel tile (W / 4 not a multiple of 16), partial last row band, the full 384-pixel row."""
    px = dev(rnd(Bn, 3, H, W, seed=5) * 1.5 + 0.2)
    w = dev(rnd(64, 3, 7, 7, seed=6, scale=0.1))
    bias, gamma, beta = dev(rnd(64, seed=7) * 0.3), dev(1.0 + 0.2 * rnd(64, seed=8)), dev(0.2 * rnd(64, seed=9))
    wpk = ops.patch_embed_pack(w)
    assert torch.equal(wpk.view(64, 24, 8)[:, :21, :7].reshape(64, 3, 7, 7), w.to(BF)) and float(wpk.view(64, 24, 8)[:, 21:].abs().max()) == 0.0
    assert float(wpk.view(64, 24, 8)[:, :, 7].abs().max()) == 0.0
    y, e, stats, Ho, Wo = ops.patch_embed_s1(px, wpk, bias, gamma, beta, 1e-5, need_e=True)
    assert (Ho, Wo) == (H // 4, W // 4)
    ref_e = torch.nn.functional.conv2d(px.to(BF).float(), w.to(BF).float(), bias, stride=4, padding=2).flatten(2).transpose(1, 2).reshape(-1, 64)
    close(e, ref_e, rtol=4e-3, atol=1e-2, what="patch embedding conv + bias")
    er = e.float()
    ref_y = torch.nn.functional.layer_norm(er, (64,), gamma, beta, 1e-5)
    close(y, ref_y, rtol=4e-3, atol=2e-2, what="LayerNorm of the embedding")
    close(stats[:, 0], er.mean(1), rtol=1e-4, atol=1e-4, what="mean")
    close(stats[:, 1], (er.var(1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-3, atol=1e-3, what="rstd")
    y2 = ops.patch_embed_s1(px, wpk, bias, gamma, beta, 1e-5, need_e=False)[0]           # inference form: nothing but y is written
    assert torch.equal(y2, y)
    # the path it replaces
    wp = torch.zeros((64, 192), dtype=BF, device="cuda")
    wp[:, :147] = w.reshape(64, 147).to(BF)
    col, _, _ = ops.im2col_pixels(px, 7, 4, 2, 192)
    e_old = ops.gemm_nt(col, wp, bias=bias)
    y_old, st_old = ops.layernorm(e_old, gamma, beta, 1e-5, need_stats=True)
    close(e, e_old.float(), rtol=4e-3, atol=1e-2, what="e vs im2col + GEMM")
    close(y, y_old.float(), rtol=6e-3, atol=3e-2, what="y vs im2col + GEMM + LayerNorm")


def test_im2col_tokens_and_col2im(ops):
    Bn, C, H, W = 2, 64, 24, 24
    x = dev(rnd(Bn, H * W, C).to(BF))
    w = dev(rnd(192, C, 3, 3, seed=1, scale=0.1))
    col, Ho, Wo = ops.im2col_tokens(x, H, W, 2, 1)
    wp = w.permute(0, 2, 3, 1).reshape(192, 9 * C).contiguous().to(BF)
    out = ops.gemm_nt(col, wp)
    xi = x.float().transpose(1, 2).reshape(Bn, C, H, W).requires_grad_(True)
    ref = torch.nn.functional.conv2d(xi, w.to(BF).float(), stride=2, padding=1)
    close(out, ref.flatten(2).transpose(1, 2).reshape(-1, 192), what="conv 3x3 s2")
    # col2im == conv input gradient
    dy = dev(rnd(Bn * Ho * Wo, 192, seed=2).to(BF))
    dcol = ops.gemm_nt(dy, ops.transpose(wp))
    dx = ops.col2im_tokens(dcol, Bn, C, H, W, 2, 1)
    ref.backward(dy.float().view(Bn, Ho * Wo, 192).transpose(1, 2).reshape(Bn, 192, Ho, Wo))
    close(dx, xi.grad.flatten(2).transpose(1, 2), what="col2im")


@pytest.mark.parametrize("Bn,Cin,N,H,W", [(2, 64, 192, 24, 24), (3, 192, 384, 12, 12), (2, 64, 192, 7, 5), (5, 128, 136, 9, 20), (64, 64, 192, 96, 96)])
def test_implicit_gemm_stage_embedding_is_the_im2col_gemm(ops, Bn, Cin, N, H, W):
    """cxr_gemm_nt_conv_bf16 (round 4): the 3 x 3 / stride 2 / padding 1 stage embeddings of CvT as an implicit GEMM -- the A operand is gathered from
    the token-major activation by the GEMM's own staging loop, zeros outside the image. Same tile kernel, same K order as im2col + gemm_nt: the
    results are BIT-identical, also on odd grids (ragged last output row / column), a strided (class-token-offset) input view and a ragged last tile;
    against torch's conv2d within the bf16 tolerance."""
    base = dev(rnd(Bn, 1 + H * W, Cin, seed=3).to(BF))
    x = base[:, 1:, :]                                           # batch / row strides of a view behind a class token
    w = dev(rnd(N, Cin, 3, 3, seed=1, scale=0.1))
    bias = dev(rnd(N, seed=2))
    wp = w.permute(0, 2, 3, 1).reshape(N, 9 * Cin).contiguous().to(BF)
    col, Ho, Wo = ops.im2col_tokens(x, H, W, 2, 1)
    with _gemm_route("tiled"):
        want = ops.gemm_nt(col, wp, bias=bias)
    got, Ho2, Wo2 = ops.gemm_nt_conv(x, H, W, 2, 1, wp, bias=bias)
    assert (Ho2, Wo2) == (Ho, Wo) and got.shape == want.shape
    assert torch.equal(got, want)
    if Bn * H * W <= 4096:
        xi = x.float().transpose(1, 2).reshape(Bn, Cin, H, W)
        ref = torch.nn.functional.conv2d(xi, w.to(BF).float(), bias, stride=2, padding=1)
        close(got, ref.flatten(2).transpose(1, 2).reshape(-1, N), what="implicit conv 3x3 s2")


@pytest.mark.parametrize("C,H,tok0", [(64, 24, 0), (192, 12, 0), (384, 6, 1)])
def test_dwconv_bn_fwd_bwd(ops, C, H, tok0):
    Bn, W = 3, H
    x = dev(rnd(Bn, tok0 + H * W, C).to(BF))
    par = {}
    for name, seed in (("q", 1), ("k", 2), ("v", 3)):
        par[name] = dict(w=dev(rnd(C, 1, 3, 3, seed=seed, scale=0.3)), g=dev(1 + 0.1 * rnd(C, seed=seed + 10)), b=dev(0.1 * rnd(C, seed=seed + 20)),
                         mean=dev(0.1 * rnd(C, seed=seed + 30)), var=dev(1 + 0.1 * rnd(C, seed=seed + 40).abs()))
    fold = {n: ops.bn_fold(p["w"], p["g"], p["b"], p["mean"], p["var"], 1e-5) for n, p in par.items()}
    yq, _ = ops.dwconv_bn(x, H, W, 1, tok0, fold["q"])
    yk, yv = ops.dwconv_bn(x, H, W, 2, tok0, fold["k"], fold["v"])
    xs = x[:, tok0:].float().transpose(1, 2).reshape(Bn, C, H, W).requires_grad_(True)
    leaves = {n: {k: v.clone().requires_grad_(k in ("w", "g", "b")) for k, v in p.items()} for n, p in par.items()}

    def ref(n, stride):
        p = leaves[n]
        y = torch.nn.functional.conv2d(xs, p["w"], None, stride=stride, padding=1, groups=C)
        y = torch.nn.functional.batch_norm(y, p["mean"], p["var"], p["g"], p["b"], False, 0.0, 1e-5)
        return y.flatten(2).transpose(1, 2)

    refs = {"q": ref("q", 1), "k": ref("k", 2), "v": ref("v", 2)}
    for n, y in (("q", yq), ("k", yk), ("v", yv)):
        close(y[:, tok0:], refs[n], what=f"dwconv {n}")
        if tok0:
            assert torch.equal(y[:, 0], x[:, 0])
    dys = {n: dev(rnd(*y.shape, seed=7 + i).to(BF)) for i, (n, y) in enumerate((("q", yq), ("k", yk), ("v", yv)))}
    sum(((refs[n] * dys[n][:, tok0:].float()).sum() for n in refs)).backward()
    dx = ops.dwconv_bn_bwd_dx([(dys["q"], fold["q"][0], 1), (dys["k"], fold["k"][0], 2), (dys["v"], fold["v"][0], 2)], Bn, C, H, W, tok0)
    close(dx[:, tok0:], xs.grad.flatten(2).transpose(1, 2), what="dwconv dx")
    if tok0:
        close(dx[:, 0], sum(d[:, 0].float() for d in dys.values()), what="dwconv dx cls")
    for n, stride in (("q", 1), ("k", 2), ("v", 2)):
        G, S = ops.dwconv_bn_bwd_w(x, dys[n], H, W, stride, tok0)
        p = par[n]
        dw, dg, db = torch.zeros(C, 9, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        ops.bn_fold_bwd(p["w"], p["g"], p["mean"], p["var"], 1e-5, G, S, dw, dg, db)
        close(dw.view(C, 1, 3, 3), leaves[n]["w"].grad, what=f"dwconv dW {n}")
        close(dg, leaves[n]["g"].grad, what=f"bn dgamma {n}")
        close(db, leaves[n]["b"].grad, what=f"bn dbeta {n}")


@pytest.mark.parametrize("C,H,tok0", [(64, 24, 0), (192, 12, 0), (384, 6, 1)])
def test_dwconv_batchnorm_train_mode(ops, C, H, tok0):
    """Batch-statistics BatchNorm (model.train()): statistics pass + finalize + folded conv == F.batch_norm(training=True), running
    statistics moved like nn.BatchNorm2d(momentum=0.1), and the backward goes through the batch statistics."""
    Bn, W = 3, H
    x = dev((rnd(Bn, tok0 + H * W, C) + 0.3).to(BF))
    for name, stride, seed in (("q", 1, 1), ("kv", 2, 2)):
        n = 1 if name == "q" else 2
        par = [dict(w=dev(rnd(C, 1, 3, 3, seed=seed + i, scale=0.3)), g=dev(1 + 0.1 * rnd(C, seed=seed + 10 + i)), b=dev(0.1 * rnd(C, seed=seed + 20 + i)),
                    rm=dev(0.1 * rnd(C, seed=seed + 30 + i)), rv=dev(1 + 0.1 * rnd(C, seed=seed + 40 + i).abs())) for i in range(n)]
        raws = [p["w"].view(C, 9).t().contiguous() for p in par]
        stats = ops.dwconv_stats(x, H, W, stride, tok0, raws[0], raws[1] if n == 2 else None)
        Ho = (H - 1) // stride + 1
        count = Bn * Ho * Ho
        xs = x[:, tok0:].float().transpose(1, 2).reshape(Bn, C, H, W).requires_grad_(True)
        folds, kept, refs, leaves = [], [], [], []
        rm_start, rv_start = [p["rm"].clone() for p in par], [p["rv"].clone() for p in par]
        for i, p in enumerate(par):
            rm0, rv0 = p["rm"].clone(), p["rv"].clone()
            fold, mean, rstd = ops.bn_train_finalize(stats[i], count, p["w"], p["g"], p["b"], 1e-5, 0.1, p["rm"], p["rv"])
            lv = {k: p[k].clone().requires_grad_(True) for k in ("w", "g", "b")}
            c = torch.nn.functional.conv2d(xs, lv["w"], None, stride=stride, padding=1, groups=C)
            ref = torch.nn.functional.batch_norm(c, rm0, rv0, lv["g"], lv["b"], True, 0.1, 1e-5)
            close(mean, c.detach().mean((0, 2, 3)), rtol=1e-3, atol=1e-3, what="batch mean")
            close(rstd, (c.detach().var((0, 2, 3), unbiased=False) + 1e-5).rsqrt(), rtol=1e-3, atol=1e-3, what="batch rstd")
            close(p["rm"], rm0, rtol=1e-4, atol=1e-4, what="running mean")           # F.batch_norm updated rm0/rv0 in place
            close(p["rv"], rv0, rtol=1e-4, atol=1e-4, what="running var")
            folds.append(fold); kept.append((mean, rstd)); refs.append(ref.flatten(2).transpose(1, 2)); leaves.append(lv)
        ys = ops.dwconv_bn(x, H, W, stride, tok0, *folds)
        for i in range(n):
            close(ys[i][:, tok0:], refs[i], what=f"train-mode bn fwd {name}{i}")
        # the one-call variant (statistics + row sum + finalize in two launches) gives the same folds / statistics / running-stat update
        fresh = [dict(wt=raws[i], w=par[i]["w"], g=par[i]["g"], b=par[i]["b"], run_mean=rm_start[i].clone(), run_var=rv_start[i].clone()) for i in range(n)]
        fused, cnt = ops.dwconv_bn_train_fwd_stats(x, H, W, stride, tok0, 1e-5, 0.1, fresh)
        assert cnt == count
        for i in range(n):
            close(fused[i][0][0], folds[i][0], rtol=1e-4, atol=1e-5, what="fused folded taps")
            close(fused[i][0][1], folds[i][1], rtol=1e-4, atol=1e-4, what="fused shift")
            close(fused[i][1], kept[i][0], rtol=1e-4, atol=1e-5, what="fused mean"); close(fused[i][2], kept[i][1], rtol=1e-4, atol=1e-4, what="fused rstd")
            close(fresh[i]["run_mean"], par[i]["rm"], rtol=1e-5, atol=1e-6, what="fused running mean")
            close(fresh[i]["run_var"], par[i]["rv"], rtol=1e-5, atol=1e-6, what="fused running var")
        dys = [dev(rnd(*ys[i].shape, seed=7 + i).to(BF)) for i in range(n)]
        sum((refs[i] * dys[i][:, tok0:].float()).sum() for i in range(n)).backward()
        fdg, fdb = [torch.zeros(C, device="cuda") for _ in range(n)], [torch.zeros(C, device="cuda") for _ in range(n)]
        fcoefs = ops.dwconv_bn_train_bwd_stats(x, H, W, stride, tok0, [dict(wt=raws[i], dy=dys[i], g=par[i]["g"], mean=kept[i][0], rstd=kept[i][1],
                                                                             dg=fdg[i], db=fdb[i]) for i in range(n)])
        projs = []
        for i, p in enumerate(par):
            dc = dys[i].clone()
            SD = ops.dwconv_stats(x, H, W, stride, tok0, raws[i], dy0=dc)[0]             # (sum dy, sum dy*c)
            if n == 2 and i == 1:                                                       # the paired launch (key + value) gives the same sums
                both = ops.dwconv_stats(x, H, W, stride, tok0, raws[0], raws[1], dy0=dys[0], dy1=dys[1])
                close(both[1], SD, rtol=1e-4, atol=1e-3, what="paired backward statistics")
            dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
            coef = ops.bn_train_bwd_coef(p["g"], kept[i][0], kept[i][1], SD, count, dg, db)
            close(fcoefs[i], coef, rtol=1e-4, atol=1e-5, what="fused backward coefficients")
            close(fdg[i], dg, rtol=1e-4, atol=1e-4, what="fused dgamma"); close(fdb[i], db, rtol=1e-4, atol=1e-4, what="fused dbeta")
            ops.dwconv_bn_train_dc_(x, raws[i], coef, dc, H, W, stride, tok0)
            if tok0:
                assert torch.equal(dc[:, 0], dys[i][:, 0])                            # class-token rows bypass conv + BN
            G2, _ = ops.dwconv_bn_bwd_w(x, dc, H, W, stride, tok0)
            dw = torch.zeros(C, 9, device="cuda")
            ops.tap_grad_accum(G2, dw)
            close(dw.view(C, 1, 3, 3), leaves[i]["w"].grad, rtol=3e-2, atol=3e-2, what=f"train-mode dW {name}{i}")
            close(dg, leaves[i]["g"].grad, what=f"train-mode dgamma {name}{i}")
            close(db, leaves[i]["b"].grad, what=f"train-mode dbeta {name}{i}")
            projs.append((dc, raws[i], stride))
        dx = ops.dwconv_bn_bwd_dx(projs, Bn, C, H, W, tok0)
        close(dx[:, tok0:], xs.grad.flatten(2).transpose(1, 2), rtol=3e-2, atol=3e-2, what=f"train-mode dx {name}")


@pytest.mark.parametrize("Ms,N,K", [((18464, 4640, 4640), 384, 384), ((300, 77), 192, 192), ((8192, 8192, 8192), 768, 768), ((130,), 64, 96),
                                    ((36928, 9280, 9280), 384, 384), ((36928, 9283), 384, 1536)])       # (the last two: the grouped row-strip launch)
def test_gemm_nt_group_equals_single_launches(ops, Ms, N, K):
    """Grouped launch (query / key / value projections in one kernel) == the same problems launched one by one, bit for bit; with a member of >= 24577
    rows at N = 384 the group goes out as ONE row-strip launch (csrc/gemm_strip.hip), compared here with the tiled kernel too."""
    probs = []
    for i, M in enumerate(Ms):
        probs.append((dev(rnd(M, K, seed=i).to(BF)), dev(rnd(N, K, seed=10 + i, scale=0.1).to(BF)), dev(rnd(N, seed=20 + i)) if i != 1 else None))
    outs = ops.gemm_nt_group(probs)
    for (a, w, b), o in zip(probs, outs):
        assert torch.equal(o, ops.gemm_nt(a, w, bias=b))
        with _gemm_route("tiled"):
            assert torch.equal(o, ops.gemm_nt(a, w, bias=b))
        close(o, a.float() @ w.float().t() + (b if b is not None else 0), what="grouped gemm")


def test_attention_bwd_strided_dkdv_outputs(ops):
    """dK / dV written as column slices of one wider matrix (the decoder's fused cross-attention gradient buffer) == the contiguous outputs."""
    B, Tq, Tk, H = 2, 70, 150, 3
    D = H * 64
    q, k, v = (dev(rnd(B, T, D, seed=i).to(BF)) for i, T in enumerate((Tq, Tk, Tk)))
    o, lse = ops.attention(q, k, v, H, 0.125, need_lse=True)
    do = dev(rnd(B, Tq, D, seed=5).to(BF))
    dq0, dk0, dv0 = ops.attention_bwd(q, k, v, o, do, lse, H, 0.125)
    wide = torch.zeros(B, Tk, 5 * D, device="cuda", dtype=BF)
    dq1, dk1, dv1 = ops.attention_bwd(q, k, v, o, do, lse, H, 0.125, dk_out=wide[:, :, D:2 * D], dv_out=wide[:, :, 3 * D:4 * D])
    assert torch.equal(dq0, dq1) and torch.equal(dk0, wide[:, :, D:2 * D]) and torch.equal(dv0, wide[:, :, 3 * D:4 * D])
    assert float(wide[:, :, :D].abs().max()) == 0 and float(wide[:, :, 2 * D:3 * D].abs().max()) == 0 and float(wide[:, :, 4 * D:].abs().max()) == 0


def test_batched_layout_and_mask_launches_equal_their_single_launch_forms(ops):
    """One-launch-per-step helpers: DropPath factors of consecutive sites, raw-tap re-layout of many projections, LayerNorm parameter-gradient
    row sum issued separately -- each equals the per-item / fused launch it replaces."""
    seed = torch.tensor([12345], dtype=torch.int32, device="cuda")
    f = ops.dropout_site_factors(6, 37, 0.2, seed, 1010)
    for s_ in range(6):
        assert torch.equal(f[s_], ops.dropout_mask(37, 1, 0.2, seed, 1010 + s_, 1, factor=True).view(37))
    ws = [dev(rnd(C, 9, seed=i)) for i, C in enumerate((64, 192, 384, 64))]
    tl = ops.TapsLayout(ws)
    for w, o in zip(ws, tl.run()):
        assert torch.equal(o, w.t().contiguous())
    ws[2].mul_(2.0)
    assert torch.equal(tl.run()[2], ws[2].t().contiguous())                     # persistent destinations, refreshed in place
    rows, C = 1000, 384
    x, dy = dev(rnd(rows, C).to(BF)), dev(rnd(rows, C, seed=1).to(BF))
    g = dev(1 + 0.1 * rnd(C, seed=2))
    _, st = ops.layernorm(x, g, g, 1e-5, need_stats=True)
    dg0, db0 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx0 = ops.layernorm_bwd(x, dy, g, st, dg0, db0)
    from cxrmate_amd import wgrad
    with wgrad.overlap():
        try:
            dg1, db1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
            dx1 = ops.layernorm_bwd(x, dy, g, st, dg1, db1)                      # partial rows on this stream, row sum on the side stream
        finally:
            wgrad.join()
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1)
    close(dg1, dg0, rtol=1e-5, atol=1e-4, what="dgamma via side-stream row sum"); close(db1, db0, rtol=1e-5, atol=1e-4, what="dbeta via side-stream row sum")


def test_top_p_without_top_k_matches_hf_warper_semantics(ops):
    """Nucleus filtering over the whole vocabulary (no top-k): the kept set is the minimal top set whose softmax mass reaches top_p
    (TF5 generation/logits_process.py TopPLogitsWarper), and sampling draws only from it."""
    R, V = 12, 30000
    for scale, top_p, temp in ((3.0, 0.9, 1.0), (0.5, 0.5, 1.0), (6.0, 0.95, 0.7), (0.1, 0.3, 1.0)):
        logits = dev(rnd(R, V, seed=int(scale * 10)) * scale)
        thr = ops.topk_threshold(logits, 0, top_p, temp)
        sc = (logits / temp).double()
        srt, idx = torch.sort(sc, dim=-1, descending=False)
        cum = srt.softmax(-1).cumsum(-1)
        remove = cum <= (1 - top_p)
        remove[:, -1:] = False
        ref_keep = torch.zeros_like(remove).scatter(1, idx, ~remove)
        keep = logits >= thr[:, None]
        # fp32 mass sums vs the float64 reference may move the boundary by a token or two when the cumulative mass sits within rounding of top_p
        diff = (keep != ref_keep).sum(1)
        assert int(diff.max()) <= 2, diff
        assert bool((keep.sum(1) >= 1).all())
        u = torch.rand(R, device="cuda")
        tok = ops.select_token(logits, mode=1, temperature=temp, top_k=0, u=u, top_p=top_p)
        tok = tok[0] if isinstance(tok, tuple) else tok
        assert bool(keep.gather(1, tok[:, None]).all())                          # every sample lies inside the nucleus
    # large top-k (> the 256-entry list path) + top-p takes the same route
    logits = dev(rnd(R, V, seed=3) * 2)
    thr = ops.topk_threshold(logits, 2000, 0.8, 1.0)
    kth = torch.topk(logits, 2000)[0][:, -1]
    assert bool((thr >= kth).all())
    sc = logits.double().masked_fill(logits < kth[:, None], float("-inf"))
    srt, idx = torch.sort(sc, dim=-1, descending=False)
    remove = srt.softmax(-1).cumsum(-1) <= 0.2
    remove[:, -1:] = False
    ref_keep = torch.zeros_like(remove).scatter(1, idx, ~remove) & (logits >= kth[:, None])
    assert int(((logits >= thr[:, None]) != ref_keep).sum(1).max()) <= 2


DWPROJ_SHAPES = [(3, 64, 24, 24, 0), (3, 192, 12, 12, 0), (3, 384, 6, 6, 1), (2, 64, 7, 5, 1), (2, 128, 9, 20, 0), (32, 384, 24, 24, 1), (8, 64, 96, 96, 0)]


def _dwproj_params(C, seeds=(1, 2, 3)):
    par = []
    for seed in seeds:
        par.append(dict(w=dev(rnd(C, 1, 3, 3, seed=seed, scale=0.3)), g=dev(1 + 0.1 * rnd(C, seed=seed + 10)), b=dev(0.1 * rnd(C, seed=seed + 20)),
                        rm=dev(0.1 * rnd(C, seed=seed + 30)), rv=dev(1 + 0.1 * rnd(C, seed=seed + 40).abs())))
    return par


@pytest.mark.parametrize("Bn,C,H,W,tok0", DWPROJ_SHAPES)
def test_dwproj_fused_eval(ops, Bn, C, H, W, tok0):
    """Fused q/k/v projections with the running statistics folded in (model.eval()): forward, input gradient, tap sums."""
    strides = (1, 2, 2)
    x = dev((rnd(Bn, tok0 + H * W, C) + 0.2).to(BF))
    par = _dwproj_params(C)
    folds = [ops.bn_fold(p["w"], p["g"], p["b"], p["rm"], p["rv"], 1e-5) for p in par]
    ys = ops.dwproj_apply(x, H, W, tok0, [dict(stride=st, taps=f[0], shift=f[1]) for st, f in zip(strides, folds)])
    xs = x[:, tok0:].float().transpose(1, 2).reshape(Bn, C, H, W).requires_grad_(True)
    leaves = [{k: p[k].clone().requires_grad_(True) for k in ("w", "g", "b")} for p in par]
    refs = []
    for st, p, lv in zip(strides, par, leaves):
        c = torch.nn.functional.conv2d(xs, lv["w"], None, stride=st, padding=1, groups=C)
        refs.append(torch.nn.functional.batch_norm(c, p["rm"], p["rv"], lv["g"], lv["b"], False, 0.0, 1e-5).flatten(2).transpose(1, 2))
    for i, (y, r) in enumerate(zip(ys, refs)):
        assert y.shape == (Bn, tok0 + r.shape[1], C)
        close(y[:, tok0:], r, what=f"dwproj eval fwd {i}")
        if tok0:
            assert torch.equal(y[:, :tok0], x[:, :tok0])
    dys = [dev(rnd(*y.shape, seed=7 + i).to(BF)) for i, y in enumerate(ys)]
    sum((r * d[:, tok0:].float()).sum() for r, d in zip(refs, dys)).backward()
    keep = [d.clone() for d in dys]
    GS = ops.dwproj_dc_taps_(x, H, W, tok0, [dict(stride=st, taps=f[0], y=d) for st, f, d in zip(strides, folds, dys)])
    for d, k in zip(dys, keep):
        assert torch.equal(d, k)                                                     # no coefficients: gradients are not rewritten
    for i, (p, lv) in enumerate(zip(par, leaves)):
        dw, dg, db = torch.zeros(C, 9, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        ops.bn_fold_bwd(p["w"], p["g"], p["rm"], p["rv"], 1e-5, GS[i, :9], GS[i, 9], dw, dg, db)
        close(dw.view(C, 1, 3, 3), lv["w"].grad, what=f"dwproj eval dW {i}")
        close(dg, lv["g"].grad, what=f"dwproj eval dgamma {i}")
        close(db, lv["b"].grad, what=f"dwproj eval dbeta {i}")
    dx = ops.dwproj_dx([dict(stride=st, taps=f[0], y=d) for st, f, d in zip(strides, folds, dys)], Bn, C, H, W, tok0)
    close(dx[:, tok0:], xs.grad.flatten(2).transpose(1, 2), what="dwproj eval dx")
    if tok0:
        close(dx[:, 0], sum(d[:, 0].float() for d in dys), what="dwproj dx cls")
    # the per-projection kernels of conv.hip compute the same thing
    yq, _ = ops.dwconv_bn(x, H, W, 1, tok0, folds[0])
    close(ys[0], yq, rtol=1e-3, atol=1e-2, what="dwproj vs dwconv q")


def _fp8_values(t8):
    """e4m3 bytes -> fp32 values (torch's own cast)"""
    return t8.float()


@pytest.mark.parametrize("Bn,C,H,W,tok0", [(2, 64, 12, 12, 0), (2, 384, 6, 6, 1)])
def test_dwproj_and_layernorm_e4m3_outputs(ops, Bn, C, H, W, tok0):
    """Producers of the frozen e4m3 encoder (BASELINE.json configs[4]): cxr_dwproj_apply_q8 and cxr_layernorm_q8_bf16 write e4m3(value / scale)
    directly. They quantise the fp32 value (the separate pass quantised the bf16-rounded one): equal to quantising the bf16 output up to one e4m3
    step, and the dequantised result stays as close to the fp32 reference as the e4m3 grid allows (relative step 2^-3 at worst, 2^-4 typical)."""
    strides = (1, 2, 2)
    x = dev((rnd(Bn, tok0 + H * W, C) + 0.2).to(BF))
    par = _dwproj_params(C)
    folds = [ops.bn_fold(p["w"], p["g"], p["b"], p["rm"], p["rv"], 1e-5) for p in par]
    projs = [dict(stride=st, taps=f[0], shift=f[1]) for st, f in zip(strides, folds)]
    ys = ops.dwproj_apply(x, H, W, tok0, projs)
    scales = [float(y.float().abs().max()) / 400.0 for y in ys]
    y8 = ops.dwproj_apply_q8(x, H, W, tok0, projs, scales)
    for y, q8, sc in zip(ys, y8, scales):
        assert q8.shape == y.shape and q8.dtype == ops.FP8
        want = ops.quantize_fp8(y.reshape(-1, C), sc).view(y.shape)
        a, b = _fp8_values(q8) * sc, _fp8_values(want) * sc
        assert float((a - b).abs().max()) <= 0.13 * float(y.float().abs().max())          # at most one e4m3 step apart (fp32 vs bf16 rounding at a tie)
        assert float(((a - b) != 0).float().mean()) < 0.05                                   # ... and almost never
        assert bool(((a - y.float()).abs() <= 0.0635 * y.float().abs() + sc * 2.0 ** -9).all())          # e4m3 rounding: 2^-4 relative, 2^-10 * scale near zero
    g, b_ = dev(rnd(C, seed=5) * 0.1 + 1.0), dev(rnd(C, seed=6) * 0.1)
    x2 = x.view(-1, C)
    y, _ = ops.layernorm(x2, g, b_, 1e-5)
    sc = float(y.float().abs().max()) / 400.0
    q8 = ops.layernorm_q8(x2, g, b_, 1e-5, sc)
    want = ops.quantize_fp8(y, sc)
    a, b = _fp8_values(q8) * sc, _fp8_values(want) * sc
    assert float(((a - b) != 0).float().mean()) < 0.05
    assert bool(((a - y.float()).abs() <= 0.0635 * y.float().abs() + sc * 2.0 ** -9).all())


@pytest.mark.parametrize("Bn,C,H,W,tok0", DWPROJ_SHAPES)
def test_dwproj_fused_train(ops, Bn, C, H, W, tok0):
    """Fused q/k/v projections under model.train(): batch statistics, running-stat update, forward, and the backward through the statistics
    (dgamma, dbeta, raw-tap gradient, dx) against autograd of conv2d + batch_norm(training=True)."""
    strides = (1, 2, 2)
    x = dev((rnd(Bn, tok0 + H * W, C) + 0.3).to(BF))
    par = _dwproj_params(C)
    raws = [p["w"].view(C, 9).t().contiguous() for p in par]
    rm0, rv0 = [p["rm"].clone() for p in par], [p["rv"].clone() for p in par]
    st = ops.dwproj_bn_train_stats(x, H, W, tok0, 1e-5, 0.1, [dict(stride=s_, taps=r, w=p["w"].view(C, 9), gamma=p["g"], beta=p["b"], run_mean=p["rm"], run_var=p["rv"])
                                                              for s_, r, p in zip(strides, raws, par)])
    xs = x[:, tok0:].float().transpose(1, 2).reshape(Bn, C, H, W).requires_grad_(True)
    leaves = [{k: p[k].clone().requires_grad_(True) for k in ("w", "g", "b")} for p in par]
    refs = []
    for i, (s_, lv) in enumerate(zip(strides, leaves)):
        c = torch.nn.functional.conv2d(xs, lv["w"], None, stride=s_, padding=1, groups=C)
        ref = torch.nn.functional.batch_norm(c, rm0[i], rv0[i], lv["g"], lv["b"], True, 0.1, 1e-5)      # moves rm0 / rv0 in place
        assert st[i]["count"] == c.numel() // C
        close(st[i]["mean"], c.detach().mean((0, 2, 3)), rtol=1e-3, atol=1e-3, what=f"batch mean {i}")
        close(st[i]["rstd"], (c.detach().var((0, 2, 3), unbiased=False) + 1e-5).rsqrt(), rtol=1e-3, atol=1e-3, what=f"batch rstd {i}")
        close(par[i]["rm"], rm0[i], rtol=1e-4, atol=1e-4, what=f"running mean {i}")
        close(par[i]["rv"], rv0[i], rtol=1e-4, atol=1e-4, what=f"running var {i}")
        refs.append(ref.flatten(2).transpose(1, 2))
    ys = ops.dwproj_apply(x, H, W, tok0, st)
    for i, (y, r) in enumerate(zip(ys, refs)):
        close(y[:, tok0:], r, what=f"dwproj train fwd {i}")
    dys = [dev(rnd(*y.shape, seed=7 + i).to(BF)) for i, y in enumerate(ys)]
    sum((r * d[:, tok0:].float()).sum() for r, d in zip(refs, dys)).backward()
    keep = [d.clone() for d in dys]
    dg = [torch.zeros(C, device="cuda") for _ in par]
    db = [torch.zeros(C, device="cuda") for _ in par]
    dw = [torch.zeros(C, 9, device="cuda") for _ in par]
    coefs = ops.dwproj_bn_train_bwd_stats(x, H, W, tok0, [dict(stride=s_, taps=r, y=d, gamma=p["g"], mean=t["mean"], rstd=t["rstd"], dgamma=a, dbeta=b)
                                                          for s_, r, d, p, t, a, b in zip(strides, raws, dys, par, st, dg, db)])
    # the same statistics from the projections' FORWARD outputs (yf + beta handed over: c recovered from the bf16 output instead of the recomputed
    # convolution); one projection gets a channel with gamma = 0, whose 64-channel slice must fall back to the convolution
    dg_y = [torch.zeros(C, device="cuda") for _ in par]
    db_y = [torch.zeros(C, device="cuda") for _ in par]
    coefs_y = ops.dwproj_bn_train_bwd_stats(x, H, W, tok0, [dict(stride=s_, taps=r, y=d, gamma=p["g"], beta=p["b"], mean=t["mean"], rstd=t["rstd"], dgamma=a, dbeta=b, yf=y)
                                                            for s_, r, d, p, t, a, b, y in zip(strides, raws, dys, par, st, dg_y, db_y, ys)])
    for i in range(len(par)):
        close(dg_y[i], dg[i], rtol=5e-3, atol=5e-3, what=f"dgamma from the forward output {i}")
        assert torch.equal(db_y[i], db[i]) or float((db_y[i] - db[i]).abs().max()) <= 1e-3 * float(db[i].abs().max())
        close(coefs_y[i], coefs[i], rtol=5e-3, atol=5e-3, what=f"dc coefficients from the forward output {i}")
    g0 = par[0]["g"].clone(); g0[5] = 0.0
    y0 = ops.dwproj_apply(x, H, W, tok0, [dict(stride=strides[0], taps=ops.bn_fold(par[0]["w"], g0, par[0]["b"], st[0]["mean"], 1.0 / st[0]["rstd"] ** 2 - 1e-5, 1e-5)[0],
                                               shift=ops.bn_fold(par[0]["w"], g0, par[0]["b"], st[0]["mean"], 1.0 / st[0]["rstd"] ** 2 - 1e-5, 1e-5)[1])])[0]
    dz, dz_y = [torch.zeros(C, device="cuda") for _ in range(2)], [torch.zeros(C, device="cuda") for _ in range(2)]
    base = dict(stride=strides[0], taps=raws[0], y=dys[0], gamma=g0, mean=st[0]["mean"], rstd=st[0]["rstd"])
    cz = ops.dwproj_bn_train_bwd_stats(x, H, W, tok0, [dict(base, dgamma=dz[0], dbeta=dz[1])])
    cz_y = ops.dwproj_bn_train_bwd_stats(x, H, W, tok0, [dict(base, beta=par[0]["b"], yf=y0, dgamma=dz_y[0], dbeta=dz_y[1])])
    close(dz_y[0], dz[0], rtol=5e-3, atol=5e-3, what="dgamma with a zero gamma channel")
    assert torch.equal(dz_y[0][:64], dz[0][:64]) and torch.equal(cz_y[0][:, :64], cz[0][:, :64])      # the slice with the zero gamma took the convolution path
    # pretrained-style parameters, |beta| >> |gamma| in one slice (beta 2.0, gamma 0.02: bf16 rounding of the stored output would put an error of
    # 2^-9 * 100 on the recovered normalised activation): that slice must take the convolution path (bit-identical to the run without yf), the others
    # may keep the streaming path
    if C >= 128:
        g1, b1 = par[1]["g"].clone(), par[1]["b"].clone()
        g1[64:128] = 0.02; b1[64:128] = 2.0
        var1 = 1.0 / st[1]["rstd"] ** 2 - 1e-5
        f1 = ops.bn_fold(par[1]["w"], g1, b1, st[1]["mean"], var1, 1e-5)
        y1 = ops.dwproj_apply(x, H, W, tok0, [dict(stride=strides[1], taps=f1[0], shift=f1[1])])[0]
        da, da_y = [torch.zeros(C, device="cuda") for _ in range(2)], [torch.zeros(C, device="cuda") for _ in range(2)]
        base1 = dict(stride=strides[1], taps=raws[1], y=dys[1], gamma=g1, mean=st[1]["mean"], rstd=st[1]["rstd"])
        ca = ops.dwproj_bn_train_bwd_stats(x, H, W, tok0, [dict(base1, dgamma=da[0], dbeta=da[1])])
        ca_y = ops.dwproj_bn_train_bwd_stats(x, H, W, tok0, [dict(base1, beta=b1, yf=y1, dgamma=da_y[0], dbeta=da_y[1])])
        assert torch.equal(da_y[0][64:128], da[0][64:128]) and torch.equal(ca_y[0][:, 64:128], ca[0][:, 64:128])
        close(da_y[0], da[0], rtol=5e-3, atol=5e-3, what="dgamma with a large-beta / small-gamma slice")
        close(ca_y[0], ca[0], rtol=5e-3, atol=5e-3, what="dc coefficients with a large-beta / small-gamma slice")
    GS = ops.dwproj_dc_taps_(x, H, W, tok0, [dict(stride=s_, taps=r, y=d, coef=cf, dw=w_) for s_, r, d, cf, w_ in zip(strides, raws, dys, coefs, dw)], need_GS=True)
    for i, lv in enumerate(leaves):
        if tok0:
            assert torch.equal(dys[i][:, :tok0], keep[i][:, :tok0])                   # class-token rows bypass conv + BN
        close(dg[i], lv["g"].grad, what=f"dwproj train dgamma {i}")
        close(db[i], lv["b"].grad, what=f"dwproj train dbeta {i}")
        close(dw[i].view(C, 1, 3, 3), lv["w"].grad, rtol=3e-2, atol=3e-2, what=f"dwproj train dW {i}")
        close(GS[i, :9].t(), dw[i], rtol=1e-5, atol=1e-5, what=f"dwproj GS rows {i}")
    dx = ops.dwproj_dx([dict(stride=s_, taps=r, y=d) for s_, r, d in zip(strides, raws, dys)], Bn, C, H, W, tok0)
    close(dx[:, tok0:], xs.grad.flatten(2).transpose(1, 2), rtol=3e-2, atol=3e-2, what="dwproj train dx")
    # second call accumulates into dgamma / dbeta / dw (gradient-buffer semantics)
    d2 = [k.clone() for k in keep]
    ops.dwproj_bn_train_bwd_stats(x, H, W, tok0, [dict(stride=s_, taps=r, y=d, gamma=p["g"], mean=t["mean"], rstd=t["rstd"], dgamma=a, dbeta=b)
                                                  for s_, r, d, p, t, a, b in zip(strides, raws, d2, par, st, dg, db)])
    close(dg[0], 2 * leaves[0]["g"].grad, what="dgamma accumulates")


# ------------------------------------------------------------------------------------------------ embeddings / integer ops
def test_bert_embed_fwd_bwd(ops):
    V, T, B, C = 500, 20, 3, 768
    word, typ, pos = dev(rnd(V, C).to(BF)), dev(rnd(2, C, seed=1).to(BF)), dev(rnd(64, C, seed=2).to(BF))
    g, b = dev(1 + 0.1 * rnd(C, seed=3)), dev(0.1 * rnd(C, seed=4))
    gen = torch.Generator().manual_seed(0)
    ids = torch.randint(0, V, (B, T), generator=gen).cuda()
    tt = torch.randint(0, 2, (B, T), generator=gen).cuda()
    pid = torch.randint(0, 64, (B, T), generator=gen).cuda()
    out, ssum, stats = ops.bert_embed(ids, tt, pid, word, typ, pos, g, b, 1e-12, T, need_sum=True)
    ref_sum = word.float()[ids] + typ.float()[tt] + pos.float()[pid]
    ref = torch.nn.functional.layer_norm(ref_sum, (C,), g, b, 1e-12).view(-1, C)
    close(out, ref, what="embed")
    out2, _, _ = ops.bert_embed(ids, None, None, word, typ, pos, g, b, 1e-12, T, pos_offset=3)
    ref2 = word.float()[ids] + typ.float()[0] + pos.float()[torch.arange(T).cuda() + 3]
    close(out2, torch.nn.functional.layer_norm(ref2, (C,), g, b, 1e-12).view(-1, C), what="embed default ids")
    dsum = dev(rnd(B * T, C, seed=5).to(BF))
    dw, dt, dp = torch.zeros(V, C, device="cuda"), torch.zeros(2, C, device="cuda"), torch.zeros(64, C, device="cuda")
    ops.bert_embed_bwd(dsum, ids, tt, pid, dw, dt, dp, T, 0, padding_idx=0)
    rw = torch.zeros(V, C, device="cuda").index_add_(0, ids.view(-1), dsum.float())
    rw[0] = 0
    close(dw, rw, rtol=1e-3, atol=1e-3, what="dword")
    close(dt, torch.zeros(2, C, device="cuda").index_add_(0, tt.view(-1), dsum.float()), rtol=1e-3, atol=1e-3, what="dtype")
    close(dp, torch.zeros(64, C, device="cuda").index_add_(0, pid.view(-1), dsum.float()), rtol=1e-3, atol=1e-3, what="dpos")


def test_token_ops_bit_exact(ops):
    import golden_util as gu
    from oracle import token_ops
    g = gu.load("token_ops.json")
    for case in g["random"] + g["documented"]:
        ids = torch.tensor(case["ids"], dtype=torch.int64).cuda()
        tt = ops.token_type_ids(ids, case["special"], case["sections"])
        ttp = ops.token_type_ids(ids, case["special"], case["sections"], past=True)
        assert tt.cpu().tolist() == case["token_type_ids"], case
        assert ttp.cpu().tolist() == case["token_type_ids_past"], case
    gen = torch.Generator().manual_seed(3)
    for T in (1, 5, 64, 65, 200, 512):
        ids = torch.randint(0, 6, (4, T), generator=gen)
        mask, pos = ops.mask_position_ids(ids.cuda(), 4)
        assert np.array_equal(mask.cpu().numpy(), (ids != 4).numpy().astype(np.uint8))
        assert np.array_equal(pos.cpu().numpy(), token_ops.position_ids_from_mask((ids != 4).numpy()))
    px = torch.randn(3, 2, 3, 8, 8)
    px[1, 1] = 0
    px[2, 0, 0, 0, 0] = 0
    m = ops.image_mask(px.cuda(), 36)
    assert torch.equal(m.cpu().bool(), (px[:, :, 0, 0, 0] != 0).repeat_interleave(36, dim=1))


# ------------------------------------------------------------------------------------------------ losses / selection
def test_topk_threshold_one_pass_form_is_exact(ops):
    """Round 5: the k-th largest of a row in ONE pass (row in registers, group maxima as a lower bound, candidates ranked by counting;
    csrc/loss.hip kth_largest_onepass) at the shape of the SCST re-scoring pass (4080 x 30000, k = 50) and at its edges: bit-equal to torch.topk on
    random rows, on rows with -inf entries (earlier warpers), with ties AT the threshold, with long runs of equal values around it (the candidate
    list overflows: the radix select takes over), for k = 1 / 128 (one pass) and k = 129 (radix), and on a strided view."""
    V, k = 30000, 50
    g = torch.Generator().manual_seed(5)
    big = (torch.randn(4080, V, generator=g) * 3).cuda()
    assert torch.equal(ops.topk_threshold(big, k), torch.topk(big, k)[0][:, -1])
    x = (torch.randn(16, V, generator=g) * 2).cuda()
    x[0, 1000:] = float("-inf")                                       # only 1000 finite entries
    x[1, :] = float("-inf"); x[1, 17] = 0.5; x[1, 29999] = -1.0      # fewer finite entries than k: the threshold is -inf
    x[2, 5000:5040] = 7.25; x[2, 77] = 9.0                            # 40 tied entries straddle rank 50? (1 above + 40 tied = 41 < 50: below the ties)
    x[3, 100:180] = 9.5                                               # 80 tied entries AT the threshold
    x[4, :] = 1.0                                                      # every entry equal: candidate list overflows -> radix select
    x[5, :] = torch.arange(V, device="cuda", dtype=torch.float32) * 1e-3          # sorted ascending
    x[6, :] = torch.arange(V, 0, -1, device="cuda", dtype=torch.float32) * 1e-3    # sorted descending: every group maximum sits in the first loads
    x[7, ::2] = -0.0; x[7, 1::2] = 0.0                                 # signed zeros: equal as floats, distinct as ordered keys (torch.topk compares values)
    for kk in (1, 2, 50, 128, 129, 300):
        got, want = ops.topk_threshold(x, kk), torch.topk(x, kk)[0][:, -1]
        assert torch.equal(got[:7], want[:7]), (kk, got[:7], want[:7])
        assert float(got[7]) == 0.0                                    # +0.0 or -0.0: the same float threshold
    for Vw in (1000, 1024, 1028, 4096, 30720, 30724):                  # both edges of the one-pass form's width range (1024 .. 30720, multiples of 4)
        y = (torch.randn(5, Vw, generator=g) * 2).cuda()
        for kk in (1, 50, 128):
            assert torch.equal(ops.topk_threshold(y, kk), torch.topk(y, kk)[0][:, -1]), (Vw, kk)
    wide = torch.zeros(8, V + 40, device="cuda")
    wide[:, 8:8 + V] = x[:8]
    assert torch.equal(ops.topk_threshold(wide[:, 8:8 + V], k)[:7], torch.topk(x[:8], k)[0][:7, -1])       # (row base 32-byte aligned, ld = V + 40)


def test_softmax_ce_and_reinforce(ops):
    R, V = 37, 30000
    logits = dev(rnd(R, V) * 2)
    labels = torch.randint(5, V, (R,), generator=torch.Generator().manual_seed(1))
    labels[::5] = 4
    labels = labels.cuda()
    w = ops.ce_weights(labels, 4)
    loss, row_loss, dl = ops.softmax_ce(logits, labels, 4, w)
    lr = logits.clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lr, labels, ignore_index=4)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-4
    close(dl, lr.grad, rtol=2e-2, atol=2e-2, what="dlogits")
    # bf16 logits (the training step's LM-head output): same loss / gradient as the fp32 kernel on the rounded values, ragged vocabulary too
    for Vb in (V, 1000, 29992):
        l16 = logits[:, :Vb].to(BF).contiguous()
        lab = labels.clamp(max=Vb - 1)
        wb = ops.ce_weights(lab, 4)
        a = ops.softmax_ce(l16, lab, 4, wb)
        b = ops.softmax_ce(l16.float(), lab, 4, wb)
        assert abs(a[0].item() - b[0].item()) < 1e-5 and torch.allclose(a[1], b[1], atol=1e-5) and torch.equal(a[2], b[2])
    # REINFORCE over top-k filtered scores: B=3, T=5
    B, T, k = 3, 5, 50
    logits = dev(rnd(B * T, V, seed=2) * 2)
    thr = ops.topk_threshold(logits, k)
    kth = torch.topk(logits, k)[0][:, -1]
    assert torch.equal(thr, kth)
    # the radix select keeps the keys that share the two leading digits in LDS (2048 entries) for its last two passes: rows whose values ALL share them
    # (every entry in [1, 1.0039): 30000 candidates) overflow the list and take the full scans; ragged widths take the 4-byte-load path; ties at the
    # k-th value; k = 1 and k = V - 1
    tight = dev(1.0 + rnd(4, V, seed=12).abs() * 1e-3)
    assert torch.equal(ops.topk_threshold(tight, k), torch.topk(tight, k)[0][:, -1])
    ragged = logits[:, :V - 3]
    assert torch.equal(ops.topk_threshold(ragged, k), torch.topk(ragged, k)[0][:, -1])
    ties = logits.clone(); ties[:, 100:180] = 9.5
    assert torch.equal(ops.topk_threshold(ties, k), torch.topk(ties, k)[0][:, -1])
    for kk in (1, 2048, 2049, V - 1):
        assert torch.equal(ops.topk_threshold(logits, kk), torch.topk(logits, kk)[0][:, -1]), kk
    sampled = torch.topk(logits, k)[1][:, 7].clone()
    sampled[4] = 4
    reward = torch.tensor([0.3, -0.2, 0.9]).cuda()
    w = ops.ce_weights(sampled, 4, mode=1, reward=reward, T=T)
    loss, _, dl = ops.softmax_ce(logits, sampled, 4, w, thr=thr)
    lr = logits.clone().requires_grad_(True)
    scores = lr.masked_fill(lr < kth[:, None], float("-inf")).view(B, T, V).permute(0, 2, 1)
    nll = torch.nn.functional.nll_loss(torch.log_softmax(scores, 1), sampled.view(B, T), ignore_index=4, reduction="none")
    ref = (nll.sum(-1) * reward).mean()
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-4, (loss.item(), ref.item())
    close(dl, lr.grad, rtol=2e-2, atol=2e-2, what="reinforce dlogits")
    # a drawn token whose re-scored logit sits BELOW the re-computed threshold (rank 51 / rank 300) takes the place of the k-th entry: kept =
    # { > thr } + the token, still k entries with a gradient; fp32 rows through the register kernel and the generic one (ld % 4 != 0), bf16 rows
    order = torch.topk(logits, 300)[1]
    below = sampled.clone()
    below[0], below[7], below[11] = order[0, 50], order[7, 299], order[11, 50]
    wb = ops.ce_weights(below, 4, mode=1, reward=reward, T=T)
    def restated(lg32, exact=True):
        lr2 = lg32.clone().requires_grad_(True)
        kth2 = torch.topk(lg32, k)[0][:, -1]
        at = lg32.gather(1, below.view(-1, 1))[:, 0]
        keep = torch.where((at < kth2)[:, None], lg32 > kth2[:, None], lg32 >= kth2[:, None]).scatter(1, below.view(-1, 1), True)
        assert not exact or (int(keep.sum(1).min()) == k and int(keep.sum(1).max()) == k)     # (bf16 rows: values tie at the threshold)
        sc2 = lr2.masked_fill(~keep, float("-inf")).view(B, T, V).permute(0, 2, 1)
        nll2 = torch.nn.functional.nll_loss(torch.log_softmax(sc2, 1), below.view(B, T), ignore_index=4, reduction="none")
        r2 = (nll2.sum(-1) * reward).mean()
        r2.backward()
        return r2, lr2.grad
    ref2, g2 = restated(logits)
    for lg in (logits, torch.cat([logits, logits[:, :1]], 1)[:, :V]):           # second form: row stride V + 1 -> the 256-thread kernel
        loss2, _, dl2 = ops.softmax_ce(lg, below, 4, wb, thr=thr)
        assert abs(loss2.item() - ref2.item()) < 1e-4, (loss2.item(), ref2.item())
        close(dl2, g2, rtol=2e-2, atol=2e-2, what="reinforce dlogits, drawn token below the threshold")
        live = (dl2[:, :V].float() != 0).sum(1)
        assert int(live[0]) == k and int(live[7]) == k and int(live[11]) == k and int(live[4]) == 0, live
    l16 = logits.to(torch.bfloat16)
    ref3, g3 = restated(l16.float(), exact=False)
    loss3, _, dl3 = ops.softmax_ce(l16, below, 4, wb, thr=ops.topk_threshold(l16.float(), k))
    assert abs(loss3.item() - ref3.item()) < 1e-4, (loss3.item(), ref3.item())
    close(dl3, g3, rtol=2e-2, atol=2e-2, what="reinforce dlogits bf16 rows, drawn token below the threshold")


def test_select_token(ops):
    R, V = 16, 30000
    logits = dev(rnd(R, V))
    logits[3, 100] = logits[3, 20000] = 50.0            # tie -> lowest index
    nxt, margin = ops.select_token(logits, need_margin=True)
    assert torch.equal(nxt, logits.argmax(-1)) and nxt[3].item() == 100
    t2 = torch.topk(logits, 2)[0]
    close(margin, t2[:, 0] - t2[:, 1], rtol=1e-5, atol=1e-5, what="margin")
    unf = torch.ones(R, dtype=torch.int32).cuda()
    unf[5] = 0
    eos = int(nxt[7])
    out, _ = ops.select_token(logits, unfinished=unf, eos=eos, pad=4)
    assert out[5].item() == 4 and out[7].item() == eos and unf[7].item() == 0 and unf[6].item() == 1
    # sampling: draws land inside the top-k set and follow the filtered distribution
    k = 50
    row = logits[:1].expand(4096, V).contiguous()
    u = torch.rand(4096, generator=torch.Generator().manual_seed(5)).cuda()
    draws, _ = ops.select_token(row, mode=1, temperature=0.7, top_k=k, u=u)
    topv, topi = torch.topk(logits[0], k)
    assert bool(torch.isin(draws, topi).all())
    p = torch.softmax(topv / 0.7, -1)
    freq = torch.stack([(draws == i).float().mean() for i in topi])
    assert (freq - p).abs().max().item() < 0.03
    # inverse-CDF order is the vocabulary order: u -> 0 picks the smallest kept index, u -> 1 the largest
    lo, _ = ops.select_token(row[:1], mode=1, temperature=1.0, top_k=k, u=torch.tensor([0.0]).cuda())
    hi, _ = ops.select_token(row[:1], mode=1, temperature=1.0, top_k=k, u=torch.tensor([0.999999]).cuda())
    assert lo.item() == topi.min().item() and hi.item() == topi.max().item()
    # sampled and greedy rows in ONE launch, written into a strided column of a wider id buffer (the cached decode of an SCST step)
    buf = torch.full((R, 7), -1, dtype=torch.int64, device="cuda")
    uu = torch.rand(R // 2, generator=torch.Generator().manual_seed(8)).cuda()
    ops.select_token(logits, mode=1, temperature=1.0, top_k=k, u=uu, out=buf[:, 3], n_sample=R // 2)
    assert torch.equal(buf[R // 2:, 3], logits[R // 2:].argmax(-1)) and bool((buf[:, 2] == -1).all()) and bool((buf[:, 4] == -1).all())
    alone, _ = ops.select_token(logits[: R // 2], mode=1, temperature=1.0, top_k=k, u=uu)
    assert torch.equal(buf[: R // 2, 3], alone)
    # ties at the k-th value are all kept (TopKLogitsWarper removes only scores < the k-th): a constant row keeps the whole vocabulary
    # (this also exercises the general radix path: more than 1024 elements reach the candidate filter's lower bound)
    flat = torch.zeros(1, V, device="cuda")
    a, _ = ops.select_token(flat, mode=1, temperature=1.0, top_k=k, u=torch.tensor([0.0]).cuda())
    b, _ = ops.select_token(flat, mode=1, temperature=1.0, top_k=k, u=torch.tensor([0.5]).cuda())
    assert a.item() == 0 and abs(b.item() - V // 2) <= 1
    # a tie exactly at the k-th value inside the candidate path: both tied entries stay in the support
    tied = logits[:1].clone()
    kth, kp1 = topi[k - 1].item(), torch.topk(logits[0], k + 1)[1][k].item()
    tied[0, kp1] = tied[0, kth]
    many = tied.expand(2048, V).contiguous()
    d2, _ = ops.select_token(many, mode=1, temperature=5.0, top_k=k, u=torch.rand(2048, generator=torch.Generator().manual_seed(6)).cuda())
    assert bool(torch.isin(d2, torch.cat([topi, torch.tensor([kp1], device="cuda")])).all()) and bool((d2 == kp1).any())


def test_adamw_matches_torch(ops):
    n = 4096 * 3
    p = dev(rnd(n))
    g = dev(rnd(n, seed=1))
    ref_p = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref_p], lr=1e-3)
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    p16 = torch.empty(n, dtype=BF, device="cuda")
    for step in range(1, 4):
        ref_p.grad = g.clone() * step
        opt.step()
        ops.adamw_step(p, g * step, m, v, p16, 1e-3, 0.9, 0.999, 1e-8, 0.01, step)

    close(p, ref_p.detach(), rtol=1e-5, atol=1e-5, what="adamw")
    assert torch.equal(p16, p.to(BF))
    # device-resident step counter (hipGraph replay path) gives the same trajectory
    p2, m2, v2 = dev(rnd(n)), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    t_dev = torch.zeros((), dtype=torch.int32, device="cuda")
    for step in range(1, 4):
        ops.increment_(t_dev)
        ops.adamw_step(p2, g * step, m2, v2, None, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0, step_dev=t_dev)
    close(p2, p, rtol=1e-6, atol=1e-6, what="adamw device step")


def test_pixels_normalize_pad_collate(ops):
    """ToTensor + Normalize + pad_sequence of the reference collate (single.py:248-262, multi.py:155-164) from uint8 HWC images."""
    from cxrmate_amd.pixels import collate_images, IMAGENET_MEAN, IMAGENET_STD
    g = torch.Generator().manual_seed(5)
    studies = [torch.randint(0, 256, (n, 96, 96, 3), generator=g, dtype=torch.uint8) for n in (2, 1, 3)]
    out = collate_images(studies, "cuda")
    mean, std = torch.tensor(IMAGENET_MEAN).view(3, 1, 1), torch.tensor(IMAGENET_STD).view(3, 1, 1)
    ref = torch.nn.utils.rnn.pad_sequence([(s.permute(0, 3, 1, 2).float() / 255.0 - mean) / std for s in studies], batch_first=True, padding_value=0.0)
    assert out.shape == ref.shape == (3, 3, 3, 96, 96)
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    assert bool((out[1, 1:] == 0).all()) and bool((out[0, 2] == 0).all())
    # the cross-attention mask rule of the reference (first pixel of the image != 0, quirk Q3) sees exactly the padded images
    assert (out[:, :, 0, 0, 0] != 0).cpu().tolist() == [[True, True, False], [True, False, False], [True, True, True]]


def test_top_p_threshold_and_sampling(ops):
    """TopKLogitsWarper(50) + TopPLogitsWarper(p): the threshold kernel marks exactly the oracle's surviving set, and sampling never leaves it."""
    from oracle import generate as ogen
    R, V, k = 8, 30000, 50
    logits = dev(rnd(R, V) * 2.0)
    for p, temp in ((0.9, 1.0), (0.5, 0.7), (0.05, 1.0), (1.0, 1.0)):
        thr = ops.topk_threshold(logits, k, p, temp)
        want = ogen.top_p_filter(ogen.top_k_filter(logits.cpu() / temp, k), p) if p < 1.0 else ogen.top_k_filter(logits.cpu() / temp, k)
        kept = (logits >= thr[:, None]).cpu()
        assert torch.equal(kept, torch.isfinite(want)), (p, temp, kept.sum(-1), torch.isfinite(want).sum(-1))
        row = logits[:1].expand(2048, V).contiguous()
        u = torch.rand(2048, generator=torch.Generator().manual_seed(3)).cuda()
        draws, _ = ops.select_token(row, mode=1, temperature=temp, top_k=k, top_p=p, u=u)
        support = torch.nonzero(torch.isfinite(want[0]))[:, 0].cuda()
        assert bool(torch.isin(draws, support).all())
        probs = torch.softmax(want[0][support.cpu()], -1)
        freq = torch.stack([(draws == i).float().mean() for i in support]).cpu()
        assert (freq - probs).abs().max().item() < 0.04


def _beam_step_host(logits, st, cur, prompt_len, max_length, eos, penalty):
    """One step of the library's beam search (TF5 generation/utils.py:3380-3520, do_sample=False, early_stopping=False) on study-major torch
    tensors: the checker of the device-side kernel. st: running / sequences [B,nb,L], run_scores / beam_scores [B,nb], finished [B,nb] bool,
    unsat [B,1] bool. Returns (new state, beam_idx [B,nb] parent beam, hits [B,2nb])."""
    B, nb, L = st["running"].shape
    V = logits.shape[-1]
    lp = torch.log_softmax(logits.float().view(B, nb, V), -1) + st["run_scores"][:, :, None]
    topk_lp, topk_idx = torch.topk(lp.view(B, nb * V), 2 * nb)
    beam_of, tok = topk_idx // V, topk_idx % V
    g = lambda t, i: torch.gather(t, 1, i.view(*i.shape, *([1] * (t.dim() - 2))).expand(-1, -1, *t.shape[2:]))
    topk_seq = g(st["running"], beam_of).clone()
    topk_seq[:, :, cur] = tok
    hits = (tok == eos) | (cur + 1 >= max_length)
    run_lp = topk_lp + hits.float() * -1.0e9
    nxt = torch.topk(run_lp, nb)[1]
    just = hits & (torch.arange(2 * nb, device=logits.device) < nb)[None]
    fin_lp = topk_lp / ((cur + 1 - prompt_len) ** penalty) + (~st["unsat"]).float() * -1.0e9 + (~just).float() * -1.0e9
    m_seq, m_sc, m_fin = torch.cat((st["sequences"], topk_seq), 1), torch.cat((st["beam_scores"], fin_lp), 1), torch.cat((st["finished"], just), 1)
    best = torch.topk(m_sc, nb)[1]
    new = dict(running=g(topk_seq, nxt), run_scores=g(run_lp, nxt), sequences=g(m_seq, best), beam_scores=g(m_sc, best), finished=g(m_fin, best))
    best_run = new["run_scores"][:, :1] / ((cur + 1 - prompt_len) ** penalty)
    worst = torch.where(new["finished"], new["beam_scores"].min(1, keepdim=True)[0], torch.full_like(new["beam_scores"], -1.0e9))
    new["unsat"] = st["unsat"] & torch.any(best_run > worst, -1, keepdim=True)
    return new, g(beam_of, nxt), hits


@pytest.mark.parametrize("nb,penalty,V", [(4, 2.0, 600), (2, 1.0, 9001), (3, 0.7, 600), (4, 2.0, 30000)])
def test_beam_step_kernel_follows_the_library_step(ops, nb, penalty, V):
    """Device-side beam search bookkeeping (cxr_beam_step) against the library's step restated with torch ops, over a whole search with EOS hits,
    the length limit, and the frozen state after the stop condition."""
    torch.manual_seed(5)
    B, L, P, eos, pad = 3, 14, 2, 7, 0
    dev = "cuda"
    run0 = torch.full((B, nb, L), pad, dtype=torch.int64, device=dev)
    run0[:, :, :P] = torch.randint(8, V, (B, 1, P), device=dev)
    st = dict(running=run0.clone(), sequences=run0.clone(), run_scores=torch.zeros((B, nb), device=dev), beam_scores=torch.full((B, nb), -1.0e9, device=dev),
              finished=torch.zeros((B, nb), dtype=torch.bool, device=dev), unsat=torch.ones((B, 1), dtype=torch.bool, device=dev))
    st["run_scores"][:, 1:] = -1.0e9
    d_run = run0.permute(1, 0, 2).contiguous(); d_seq = d_run.clone()
    d_rs, d_bs = st["run_scores"].clone(), st["beam_scores"].clone()
    d_fin = torch.zeros((B, nb), dtype=torch.uint8, device=dev)
    d_unsat = torch.ones((2, B), dtype=torch.int32, device=dev); d_hit = torch.zeros((2, B), dtype=torch.int32, device=dev)
    d_idx = torch.zeros(nb * B, dtype=torch.int64, device=dev)
    stopped = False
    for cur in range(P, L):
        logits = torch.randn((B, nb, V), device=dev) * 3.0
        logits[:, :, eos] += 4.0 + 0.5 * (cur - P) + math.log(V / 600.0) * 3.0     # EOS becomes likely after a few steps
        bm = logits.permute(1, 0, 2).reshape(nb * B, V).contiguous()      # beam-major rows
        before = (d_run.clone(), d_seq.clone(), d_rs.clone(), d_bs.clone(), d_fin.clone())
        ops.beam_step(bm, d_run, d_seq, d_rs, d_bs, d_fin, d_unsat, d_hit, d_idx, cur, L, eos, float(cur + 1 - P) ** penalty)
        if stopped:                                                        # frozen: nothing moves, identity reorder
            for a, b in zip(before, (d_run, d_seq, d_rs, d_bs, d_fin)):
                assert torch.equal(a, b)
            assert torch.equal(d_idx, torch.arange(nb * B, device=dev))
            continue
        st, parent, hits = _beam_step_host(logits, st, cur, P, L, eos, penalty)
        ok = hits.sum(1) <= nb            # more ended continuations than that: the running set is a tie at -1e9 (the search is over for the study)
        assert torch.equal(d_run.permute(1, 0, 2)[ok], st["running"][ok]), cur
        torch.testing.assert_close(d_rs, st["run_scores"], atol=2e-4, rtol=1e-6)
        assert torch.equal((d_idx.view(nb, B).t() // B)[ok], parent[ok]) and torch.equal(d_idx.view(nb, B).t() % B, torch.arange(B, device=dev)[:, None].expand(B, nb))
        st["running"] = d_run.permute(1, 0, 2).clone()                           # (carry the device's tie winners forward)
        assert torch.equal(d_fin.bool(), st["finished"]), cur
        fin = st["finished"]
        torch.testing.assert_close(d_bs[fin], st["beam_scores"][fin], atol=2e-4, rtol=1e-6)
        assert torch.equal(d_seq.permute(1, 0, 2)[fin], st["sequences"][fin]), cur         # (slots still at -1e9 hold arbitrary tie winners)
        assert torch.equal(d_unsat[cur & 1].bool(), st["unsat"][:, 0]), cur
        assert torch.equal(d_hit[cur & 1].bool(), hits.all(1)), cur
        stopped = not (bool(st["unsat"].any()) and not bool(hits.all()))
    assert stopped and bool(st["finished"][:, 0].all())


def _device_beam_state(B, nb, L, P, pad, first_token, dev="cuda"):
    run = torch.full((nb, B, L), pad, dtype=torch.int64, device=dev)
    run[:, :, :P] = first_token
    rs = torch.zeros((B, nb), device=dev); rs[:, 1:] = -1.0e9
    return dict(run=run, seq=run.clone(), rs=rs, bs=torch.full((B, nb), -1.0e9, device=dev), fin=torch.zeros((B, nb), dtype=torch.uint8, device=dev),
                unsat=torch.ones((2, B), dtype=torch.int32, device=dev), hit=torch.zeros((2, B), dtype=torch.int32, device=dev),
                idx=torch.zeros(nb * B, dtype=torch.int64, device=dev))


def _drive_device_beam_search(ops, logits_steps, lp, B, nb, L, eos, pad, bos, trace, fed=None):
    """cxr_beam_step + cxr_gather_batch_multi_bf16 driven with GIVEN fp32 logits (study-major rows [B*nb, V] per step, as the oracle / the reference
    order them): every step is compared with the oracle's trace of the same search -- running beams, parent beam, new token, finished set, finished
    hypotheses bit for bit -- and a stand-in KV cache (row r, position t holds the token beam r was fed at t) is reordered by the kernel's beam index:
    after every step each cache row must spell its beam's own history. -> final (sequences [B,nb,L], scores [B,nb])."""
    dev, P = "cuda", 1
    V = logits_steps[0].shape[-1]
    st = _device_beam_state(B, nb, L, P, pad, bos)
    R, C = nb * B, 8
    cache, cache2 = (torch.zeros((R, L, C), dtype=BF, device=dev) for _ in range(2))
    for t, lg in enumerate(logits_steps):
        cur = P + t
        tr = trace[t]
        dev_running = st["run"].permute(1, 0, 2)[:, :, :cur].cpu()                      # [B, nb, cur]
        assert torch.equal(dev_running, tr["running_in"]), (t, dev_running, tr["running_in"])
        if fed is not None:
            assert torch.equal(dev_running[:, :, -1].reshape(-1), fed[t]), t
        cache[:, cur - 1, :] = st["run"].view(R, L)[:, cur - 1].to(BF)[:, None]         # the "key/value" of the token fed at this step (ids < 256: exact in bf16)
        bm = lg.view(B, nb, V).permute(1, 0, 2).reshape(R, V).contiguous().cuda()
        ops.beam_step(bm, st["run"], st["seq"], st["rs"], st["bs"], st["fin"], st["unsat"], st["hit"], st["idx"], cur, L, eos, float(cur + 1 - P) ** lp)
        ops.gather_batch_multi([cache], st["idx"], cur, [cache2])
        cache, cache2 = cache2, cache
        parent = (st["idx"].view(nb, B).t() // B).cpu()
        assert torch.equal(st["idx"].view(nb, B).t() % B, torch.arange(B, device=dev)[:, None].expand(B, nb)), t      # a beam never leaves its study
        live = tr["running_scores"] > -1.0e8                                             # (slots at -1e9 are ties between ended continuations)
        assert torch.equal(parent[live], tr["parent"][live]) and torch.equal(st["run"].permute(1, 0, 2)[:, :, cur].cpu()[live], tr["token"][live]), t
        np.testing.assert_allclose(st["rs"].cpu().numpy()[live.numpy()], tr["running_scores"].numpy()[live.numpy()], rtol=2e-6, atol=2e-5)   # (fp32 log-sum-exp order)
        assert torch.equal(st["fin"].bool().cpu(), tr["finished"]), t
        fin = tr["finished"]
        assert torch.equal(st["seq"].permute(1, 0, 2).cpu()[fin], tr["sequences"][fin]), t
        np.testing.assert_allclose(st["bs"].cpu().numpy()[fin.numpy()], tr["beam_scores"].numpy()[fin.numpy()], rtol=2e-6, atol=2e-5)
        # the reordered cache rows spell their beams' histories (what the next step's attention would read)
        hist = st["run"].view(R, L)[:, :cur].to(BF)
        lv = live.t().reshape(-1).cuda()
        assert torch.equal(cache[:, :cur, 0][lv], hist[lv]) and torch.equal(cache[:, :cur, C - 1][lv], hist[lv]), t
    par = (P + len(logits_steps) - 1) & 1
    stopped = not (bool(st["unsat"][par].max() > 0) and bool(st["hit"][par].min() == 0))
    return st["seq"].permute(1, 0, 2).cpu(), st["bs"].cpu(), stopped


def test_device_beam_search_is_bit_equal_on_the_references_recorded_logits(ops):
    """The last link of the beam-search parity chain, as INDEX work (no model on the device, no bf16 noise): tests/golden/beam_index.npz holds the
    fp32 logits of every step of the reference's own beam-4 generate (early EOS, hypotheses of different length, length_penalty 0.5 / 1 / 2, searches
    that end before max_length). Fed to cxr_beam_step + the cache-reorder kernel they must give the reference's four final hypotheses per study bit
    for bit, and the oracle's beams at every step (oracle == reference on the same data: tests/test_oracle_golden.py)."""
    import golden_util as gu
    from oracle import generate as ogen
    steps, cases = gu.beam_index_cases()
    for name, lp, logits, fed, ref_all, ref_scores in cases:
        trace = []
        ogen.beam_search(gu.replay_logits_fn(logits), "multi", 3, 4, [gu.SEP], gu.BOS, gu.EOS, gu.PAD, steps + 1, length_penalty=lp, return_all=True, trace=trace)
        seqs, scores, stopped = _drive_device_beam_search(ops, list(logits), lp, 3, 4, steps + 1, gu.EOS, gu.PAD, gu.BOS, trace, fed=fed)
        assert stopped, name                                                             # the device's stop flags fall on the step the reference stopped on
        assert torch.equal(seqs[:, :, : ref_all.shape[-1]], ref_all), (name, seqs, ref_all)
        assert bool((seqs[:, :, ref_all.shape[-1]:] == gu.PAD).all()), name
        np.testing.assert_allclose(scores.numpy(), ref_scores.numpy(), rtol=2e-6, atol=2e-5, err_msg=name)


@pytest.mark.parametrize("nb,lp,V,seed", [(4, 0.5, 30000, 0), (4, 2.0, 30000, 1), (4, 1.0, 9001, 2), (2, 2.0, 30000, 3), (2, 0.5, 4096, 4)])
def test_device_beam_search_is_bit_equal_to_the_oracle_on_full_vocabulary_logits(ops, nb, lp, V, seed):
    """The same teacher-fed comparison at the real vocabulary size (several 4096-wide scan chunks per row) on seeded synthetic logits whose EOS
    column rises step by step, so that hypotheses end at different lengths and the length penalty ranks them: device == oracle.beam_search
    (pinned against the reference by beam_index.npz) at every step and at the end, bit for bit."""
    import golden_util as gu
    from oracle import generate as ogen
    B, L = 3, 18
    g = torch.Generator().manual_seed(100 + seed)
    logits = [torch.randn((B * nb, V), generator=g) * 3.0 for _ in range(L - 1)]
    base = 3.0 * math.sqrt(2 * math.log(V)) - 8.0                                      # EOS starts ~3 sigma below the row maximum and gains 0.45 per step
    for t, lg in enumerate(logits):
        lg[:, gu.EOS] += base + 0.45 * t + 2.0 * torch.rand((B * nb,), generator=g)
    trace = []
    ref_all, ref_scores = ogen.beam_search(gu.replay_logits_fn(logits), "multi", B, nb, [gu.SEP], gu.BOS, gu.EOS, gu.PAD, L, length_penalty=lp, return_all=True, trace=trace)
    assert min(t["min_gap"] for t in trace) > 1e-5
    seqs, scores, stopped = _drive_device_beam_search(ops, logits[: len(trace)], lp, B, nb, L, gu.EOS, gu.PAD, gu.BOS, trace)
    assert stopped
    assert torch.equal(seqs[:, :, : ref_all.shape[-1]], ref_all)
    np.testing.assert_allclose(scores.numpy(), ref_scores.numpy(), rtol=2e-6, atol=2e-5)
    e = ref_all == gu.EOS
    lens = torch.where(e.any(-1), e.int().argmax(-1) + 1, torch.full(e.shape[:-1], ref_all.shape[-1]))
    assert len(set(lens.reshape(-1).tolist())) >= 3                                      # hypotheses of different length were ranked


def test_gather_batch_multi_equals_single_gathers(ops):
    torch.manual_seed(6)
    B, T, C, rows = 12, 40, 768, 23
    srcs = [torch.randn((B, T, C), device="cuda").to(BF) for _ in range(12)]
    idx = torch.randint(0, B, (B,), device="cuda")
    outs = [torch.zeros_like(s) for s in srcs]
    ops.gather_batch_multi(srcs, idx, rows, outs)
    for s, o in zip(srcs, outs):
        assert torch.equal(o[:, :rows], s[idx][:, :rows]) and float(o[:, rows:].abs().max()) == 0.0


@pytest.mark.parametrize("M,N,K,act,res", [(1000, 384, 384, 0, True), (300, 64, 256, 0, False), (2304, 1536, 384, 1, False), (777, 192, 768, 0, True),
                                           (4096, 768, 384, 0, False)])
def test_gemm_nt_fp8_matches_dequantised_fp32_product(ops, M, N, K, act, res):
    """e4m3 (OCP) GEMM with per-tensor scales: EXACT operands (the e4m3 bytes, dequantised to fp32 on the host side) -> the only differences from
    an fp32 product are the accumulation order and the bf16 output rounding (rel 2^-8)."""
    torch.manual_seed(M + N)
    a = (torch.randn(M, K, device="cuda") * 1.7).to(BF)
    w = (torch.randn(N, K, device="cuda") * 0.05).to(BF)
    sa, sw = float(a.float().abs().max()) / 448.0, float(w.float().abs().max()) / 448.0
    a8, w8 = ops.quantize_fp8(a, sa), ops.quantize_fp8(w, sw)
    # the quantiser itself: round-to-nearest-even e4m3 of x / scale, as torch's conversion
    assert torch.equal(a8.view(torch.uint8), (a.float() / sa).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    bias = torch.randn(N, device="cuda")
    r = torch.randn(M, N, device="cuda").to(BF) if res else None
    ref = (a8.float() @ w8.float().t()) * (sa * sw) + bias
    if act == 1:
        ref = torch.nn.functional.gelu(ref)
    if res:
        ref = ref + r.float()
    so = float(ref.abs().max()) / 448.0
    c, c8 = ops.gemm_nt_fp8(a8, w8, sa * sw, bias=bias, residual=r, act=act, out_scale=so)
    close(c, ref, rtol=4e-3, atol=1e-2, what="fp8 gemm bf16 output")
    close(c8.float() * so, ref, rtol=4e-2, atol=7e-2, what="fp8 gemm e4m3 output")          # e4m3: 3 mantissa bits -> rel 2^-4 per element
    # and against the UNQUANTISED product: the stated fp8 tolerance of a single layer (two e4m3 operands, K-fold averaging)
    full = a.float() @ w.float().t() + bias
    if act == 1:
        full = torch.nn.functional.gelu(full)
    if res:
        full = full + r.float()
    rel = ((c.float() - full).pow(2).mean().sqrt() / full.pow(2).mean().sqrt()).item()
    assert rel < 0.05, rel


@pytest.mark.parametrize("Bkv,share,Tk,masked,drop", [(3, 2, 1152, True, 0.0), (2, 4, 576, False, 0.0), (5, 1, 1152, True, 0.1), (2, 2, 320, True, 0.1), (16, 2, 1152, True, 0.1),
                                                       (3, 2, 1728, True, 0.1), (2, 4, 2880, True, 0.0)])
def test_attention_cross_mfma_matches_the_valu_decode_kernel(ops, Bkv, share, Tk, masked, drop):
    """Cached cross-attention on the matrix cores (attn_cross_mfma_kernel, fragment-ordered K / V copies) against the VALU decode kernel and an fp32 reference:
    shared K/V rows, key-padding bit mask, the same train-mode dropout hash (probabilities enter P.V as bf16 here: tolerance of that rounding)."""
    torch.manual_seed(Bkv * 7 + Tk)
    H, D, B = 12, 768, Bkv * share
    q = (torch.randn(B, D, device="cuda") * 0.7).to(BF)
    k = (torch.randn(Bkv, Tk, D, device="cuda") * 0.7).to(BF)
    v = torch.randn(Bkv, Tk, D, device="cuda").to(BF)
    kpm = None
    if masked:
        kpm = torch.ones(Bkv, Tk, dtype=torch.uint8, device="cuda")
        kpm[0, Tk // 2:] = 0
        kpm[-1, 5:37] = 0
    bits = ops.pack_mask_bits(kpm) if masked else None
    seed = torch.tensor([1234], dtype=torch.int32, device="cuda")
    dr = (drop, seed, 21, 9) if drop > 0 else None
    wide = torch.randn(Bkv, Tk, 2 * D + 64, device="cuda").to(BF)                    # K / V as column blocks of a wider buffer (strided rows)
    wide[:, :, :D] = k; wide[:, :, D + 64:] = v
    pk = ops.pack_cross_kv(wide[:, :, :D], wide[:, :, D + 64:], H)
    ref = ops.attention_decode(q, k, v, H, 0.125, kpm=kpm, drop=dr)
    out = ops.attention_cross_mfma(q, pk, Bkv, Tk, H, 0.125, kpm_bits=bits, drop=dr)
    close(out, ref, rtol=1e-2, atol=2e-2, what="cross-attention mfma vs valu kernel")
    if drop == 0:
        kk, vv = k.float().repeat(share, 1, 1), v.float().repeat(share, 1, 1)                      # query row b + g*Bkv <-> K/V row b
        qh, kh, vh = q.float().view(B, H, 1, 64), kk.view(B, Tk, H, 64).transpose(1, 2), vv.view(B, Tk, H, 64).transpose(1, 2)
        s = (qh @ kh.transpose(2, 3)) * 0.125
        if masked:
            s = s.masked_fill(~kpm.bool().repeat(share, 1).view(B, 1, 1, Tk), torch.finfo(torch.float32).min)
        full = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, D)
        close(out, full, rtol=1e-2, atol=2e-2, what="cross-attention mfma vs fp32")
    # decode activation layout output == row-major output re-laid out
    dal = ops.attention_cross_mfma(q, pk, Bkv, Tk, H, 0.125, kpm_bits=bits, drop=dr, out_dal=True)
    assert torch.equal(ops.dec_from_dal(dal, B, D), out)


@pytest.mark.parametrize("Bkv,share,Tk,masked,drop", [(16, 2, 1152, False, 0.0), (16, 2, 1152, True, 0.1), (1, 1, 1152, False, 0.0), (3, 2, 320, True, 0.0), (5, 1, 576, True, 0.1),
                                                       (16, 2, 1728, True, 0.0), (2, 2, 1920, True, 0.1), (32, 2, 1152, True, 0.0), (8, 4, 1152, True, 0.0), (3, 3, 576, False, 0.1),
                                                       (5, 4, 1728, True, 0.1)])
def test_attention_cross_mfma_with_the_query_projection_inside(ops, Bkv, share, Tk, masked, drop):
    """cxr_attn_cross_mfma_q_bf16 (query Linear with the LayerNorm folded in computed per (study, head) inside the cross-attention kernel) against the two
    launches it replaces (cxr_dec_gemm_bf16 for q, then cxr_attn_cross_mfma_bf16) and against fp32 LayerNorm -> Linear -> attention."""
    torch.manual_seed(Bkv * 11 + Tk)
    H, D, B = 12, 768, Bkv * share
    raw = ((torch.randn(B, D, device="cuda") * 1.5 + 0.3)).to(BF)
    w, bias = (torch.randn(D, D, device="cuda") * 0.04).to(BF), torch.randn(D, device="cuda") * 0.1
    g, b = 1 + 0.1 * torch.randn(D, device="cuda"), 0.1 * torch.randn(D, device="cuda")
    k = (torch.randn(Bkv, Tk, D, device="cuda") * 0.7).to(BF)
    v = torch.randn(Bkv, Tk, D, device="cuda").to(BF)
    kpm = None
    if masked:
        kpm = torch.ones(Bkv, Tk, dtype=torch.uint8, device="cuda")
        kpm[0, Tk // 2:] = 0
        kpm[-1, 5:37] = 0
    bits = ops.pack_mask_bits(kpm) if masked else None
    seed = torch.tensor([4321], dtype=torch.int32, device="cuda")
    dr = (drop, seed, 23, 5) if drop > 0 else None
    pk = ops.pack_cross_kv(k, v, H)
    x_dal, st = _dal(ops, raw)
    wf, bcf = ops.dec_pack_weight(w, g, b, bias)
    q = torch.empty(B, D, dtype=BF, device="cuda")
    ops.dec_gemm(x_dal, B, D, [dict(wp=wf, bc=bcf, N=D, fold=True, out=q)], stats=st, eps=1e-12)
    two = ops.attention_cross_mfma(q, pk, Bkv, Tk, H, 0.125, kpm_bits=bits, drop=dr)
    for out_dal in (True, False):
        one = ops.attention_cross_mfma_q(x_dal, B, st, 1e-12, wf, bcf, pk, Bkv, Tk, H, 0.125, kpm_bits=bits, drop=dr, out_dal=out_dal)
        got = ops.dec_from_dal(one, B, D) if out_dal else one
        close(got, two, rtol=1e-2, atol=2e-2, what=f"fused query projection vs two launches (dal={out_dal})")
    if drop == 0:
        qf = torch.nn.functional.layer_norm(raw.float(), (D,), g, b, 1e-12) @ w.float().t() + bias
        kk, vv = k.float().repeat(share, 1, 1), v.float().repeat(share, 1, 1)
        qh, kh, vh = qf.view(B, H, 1, 64), kk.view(B, Tk, H, 64).transpose(1, 2), vv.view(B, Tk, H, 64).transpose(1, 2)
        s_ = (qh @ kh.transpose(2, 3)) * 0.125
        if masked:
            s_ = s_.masked_fill(~kpm.bool().repeat(share, 1).view(B, 1, 1, Tk), torch.finfo(torch.float32).min)
        full = (torch.softmax(s_, -1) @ vh).transpose(1, 2).reshape(B, D)
        close(got, full, rtol=2e-2, atol=3e-2, what="fused query projection vs fp32")
    # statistics split over several producer tiles (the layout a dec_gemm with out_stats publishes) give the same result
    (y,), yst = ops.dec_gemm(x_dal, B, D, [dict(wp=wf, bc=bcf, N=D, fold=True)], stats=st, eps=1e-12, out_stats=True)
    assert yst.shape[0] > 1
    q2 = torch.empty(B, D, dtype=BF, device="cuda")
    ops.dec_gemm(y, B, D, [dict(wp=wf, bc=bcf, N=D, fold=True, out=q2)], stats=yst, eps=1e-12)
    two2 = ops.attention_cross_mfma(q2, pk, Bkv, Tk, H, 0.125, kpm_bits=bits, drop=dr)
    one2 = ops.attention_cross_mfma_q(y, B, yst, 1e-12, wf, bcf, pk, Bkv, Tk, H, 0.125, kpm_bits=bits, drop=dr, out_dal=False)
    close(one2, two2, rtol=1e-2, atol=2e-2, what="fused query projection, multi-tile statistics")


# ------------------------------------------------------------------------------------------------ GELU epilogues, exhaustively over bf16
# Every epilogue evaluates csrc/common.h's minimax GELU. A selection weight W[n, k] = (k == n % K) makes A @ W^T exact in fp32, so with act = 1
# output column n is gelu(A[:, n % K]) and A holds every finite bf16 value; with act = 2, A = ones and aux holds every finite bf16 value, so the
# output is gelu'(aux). Bounds against the float64 erf GELU: fp32 outputs within 2.6e-5 (value) / 1.1e-4 (derivative) + 4 ulp_f32(ref); bf16
# outputs between the bf16 values just outside ref -+ the same tolerance.
GELU_TOL, GELU_D_TOL = 2.6e-5, 1.1e-4
_N_BF16 = 65024                                                     # finite bf16 values


def _all_bf16_filling(M, K):
    x = all_bf16()
    return x.repeat(-(-(M * K) // x.numel()))[:M * K].view(M, K)


def _selection_weight(N, K):
    w = torch.zeros(N, K)
    w[torch.arange(N), torch.arange(N) % K] = 1
    return w.to(BF)


def _check_gelu(out, x, deriv, what):
    v, d = gelu64(x.double())
    tol = GELU_D_TOL if deriv else GELU_TOL
    if out.dtype == torch.float32:
        err = assert_f32_bound(out, d if deriv else v, tol, 4, what)
        print(f"MEASURED {what}: max |err| {err:.4e}")
    else:
        err = assert_bf16_bracket(out, d if deriv else v, tol, what)
        print(f"MEASURED {what}: max |err| / bracket half-width {err:.3f}")


# name -> (route, K, N, row stride of the output / aux buffers, M); the tiled kernel's epilogue form each case reaches is in the comment
_GELU_FORMS = {
    "tiled": ("tiled", 128, 128, 128, None),          # LDS-staged row-contiguous epilogue, N % 8 == 0 (gemm.hip ~240)
    "tiled-n4": ("tiled", 128, 132, 136, None),       # LDS-staged, N % 8 == 4: the 4-column tail form (gemm.hip ~300); 16-byte aligned rows
    "tiled-bk32": ("tiled", 96, 96, 96, 257 * 128),   # K % 64 != 0 -> BK = 32; 257 row tiles and N % 128 = 96 -> BN = 128: the 64 x 64 fp32
                                                      # sub-tiles do not fit the BK = 32 staging LDS -> per-lane fallback form (gemm.hip ~385)
    "tiled-unaligned": ("tiled", 128, 128, 132, None),  # aux (and bf16 output) rows 4 mod 8 elements: not 16-byte aligned -> fallback form
    "pk": (("pk", 0), 384, 384, 384, None),           # csrc/gemm_pk.hip
    "ws": ("ws", 384, 384, 384, None),                # csrc/gemm_ws.hip (bf16 output only)
    "strip": (("strip", 10, 0), 384, 384, 384, None),  # csrc/gemm_strip.hip (derivative, bf16 output only)
}


def _gelu_gemm_case(ops, form, act, out_f32):
    route, K, N, ld, M = _GELU_FORMS[form]
    M = M or -(-_N_BF16 // K)
    w = _selection_weight(N, K).cuda()
    if act == 1:
        a = _all_bf16_filling(M, K)
        x = a.float()[:, torch.arange(N) % K]
        aux_src = None
    else:
        a = torch.ones(M, K, dtype=BF)
        x = _all_bf16_filling(M, N).float()
        aux_src = x.to(BF)
    go = Guarded((M, ld), torch.float32 if out_f32 else BF, (slice(None), slice(0, N)))
    ga = Guarded((M, ld), BF, (slice(None), slice(0, N)))
    if aux_src is not None:
        ga.view.copy_(aux_src.cuda())
    with _gemm_route(route):
        ops.gemm_nt(a.cuda(), w, act=act, aux=ga.view, out=go.view, out_f32=out_f32)
    go.check(f"{form} act={act} output")
    ga.check(f"{form} act={act} aux")
    if act == 1:                                                     # the saved pre-activation is the exact input
        assert torch.equal(ga.view.cpu(), x.to(BF)), f"{form}: saved pre-activation"
    return go.view, x


@pytest.mark.parametrize("form,out_f32", [("tiled", False), ("tiled", True), ("tiled-n4", False), ("tiled-n4", True), ("tiled-bk32", False),
                                          ("tiled-bk32", True), ("tiled-unaligned", False), ("tiled-unaligned", True), ("pk", False), ("pk", True),
                                          ("ws", False)])
def test_gemm_gelu_epilogue_over_every_bf16(ops, form, out_f32):
    out, x = _gelu_gemm_case(ops, form, 1, out_f32)
    _check_gelu(out, x, False, f"gelu {form} {'f32' if out_f32 else 'bf16'}")


@pytest.mark.parametrize("form,out_f32", [("tiled", False), ("tiled", True), ("tiled-n4", False), ("tiled-n4", True), ("tiled-bk32", False),
                                          ("tiled-bk32", True), ("tiled-unaligned", False), ("tiled-unaligned", True), ("pk", False), ("pk", True),
                                          ("ws", False), ("strip", False)])
def test_gemm_gelu_derivative_epilogue_over_every_bf16(ops, form, out_f32):
    out, x = _gelu_gemm_case(ops, form, 2, out_f32)
    _check_gelu(out, x, True, f"gelu' {form} {'f32' if out_f32 else 'bf16'}")


@pytest.mark.parametrize("out_f32", [False, True])
def test_skinny_and_decode_gemm_gelu_over_every_bf16(ops, out_f32):
    """gemm_skinny (K = 128, 64-row launches) and dec_gemm (K = 768, decode activation layout; 64 + 21 rows)"""
    K = 128
    a = _all_bf16_filling(-(-_N_BF16 // K), K)
    w = _selection_weight(K, K).cuda()
    for m0 in range(0, a.shape[0], 64):
        blk = a[m0:m0 + 64]
        go = Guarded((blk.shape[0], K + 8), torch.float32 if out_f32 else BF, (slice(None), slice(0, K)))
        ops.gemm_skinny(blk.cuda(), w, act=1, out=go.view, out_f32=out_f32)
        go.check(f"skinny rows {m0}")
        _check_gelu(go.view, blk.float(), False, f"gelu skinny rows {m0}.. {'f32' if out_f32 else 'bf16'}")
    K = 768
    a = _all_bf16_filling(-(-_N_BF16 // K), K)
    wp, bc = ops.dec_pack_weight(_selection_weight(K, K).cuda())
    for m0 in range(0, a.shape[0], 64):
        blk = a[m0:m0 + 64]
        M = blk.shape[0]
        xd, _ = ops.dec_to_dal(blk.cuda())
        (o,), _ = ops.dec_gemm(xd, M, K, [dict(wp=wp, bc=bc, N=K)], act=1, out_f32=out_f32)
        _check_gelu(o if out_f32 else ops.dec_from_dal(o, M, K), blk.float(), False, f"gelu dec_gemm rows {m0}.. {'f32' if out_f32 else 'bf16'}")


@pytest.mark.parametrize("N", [64, 68])                 # N % 8 == 0: vector epilogue; N = 68: per-element epilogue
def test_gemm_fp8_gelu_over_every_e4m3(ops, N):
    K = 64
    codes = torch.tensor([c for c in range(256) if c not in (0x7F, 0xFF)] + [0, 0], dtype=torch.uint8).view(4, K)   # every finite e4m3
    a8 = codes.view(ops.FP8).cuda()
    w8 = _selection_weight(N, K).float().to(ops.FP8).cuda()
    c, _ = ops.gemm_nt_fp8(a8, w8, 1.0, act=1)
    x = a8.float().cpu()[:, torch.arange(N) % K]
    _check_gelu(c, x, False, f"gelu fp8 N={N}")
