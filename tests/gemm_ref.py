"""Seeded input families, float64 references, comparers and case tables of the linear-layer GEMM tests (tests/test_gemm_exact_gpu.py runs them on
the HIP kernels, tests/test_gemm_ref.py checks this file itself without a GPU). CPU only (torch / numpy).

exact   Operands are random integers |v| <= 15 (8 bits of bf16 and 4 bits of e4m3 hold them). A bf16 x bf16 product is exact in fp32, and as long as
        every partial sum of every element stays below 2^24 in units of that element's power-of-two scale, fp32 addition is exact too: the result
        does not depend on the summation order and a correct kernel returns THE integer. Plain products scale every row of A and of W by a power of
        two 2^e, e in [-3, 3] (a swapped row or column then shows even where the integers coincide); epilogue cases keep unscaled integers and take
        alpha in {0.5, 2}, integer bias |b| <= 1024, integer bf16 residual |r| <= 255, row scales from {0, 0.5, 1, 2}, dropout p = 0.5 (factor 2) and an
        integer-valued fp32 output to accumulate onto, so that every epilogue step is exact in fp32 as well. The generator asserts the 2^24 cap and
        that at least a quarter of the reference elements need more than 8 significant bits (a bf16 rounding anywhere before the last step shows).
        Comparison: torch.equal with the float64 reference cast to fp32, or rounded to nearest even to bf16 -- values, not bit patterns (the sign of
        a zero sum is not specified).

gauss   N(0, 1) operands rounded to bf16; a tenth of the K (TN: token) positions is scaled by 64; the last row of A is minus the first (TN: column of
        P), and the second half of row 0 of A mirrors its first half against a W row 0 whose halves are equal, so that an output cancels to zero;
        alpha = 0.37, Gaussian bias, residual and accumulation target. Tolerance per element, derived:
            tol = |alpha| 2 K 2^-24 sum_k |a_k w_k|  +  4 fp32 steps of each epilogue intermediate
        K 2^-24 sum|a w| bounds any order of fp32 additions of the (exact) products; the factor 2 allows an accumulator that truncates where fp32
        rounds (how the MFMA rounds internally is not documented). bf16 outputs are checked with bounds_util.assert_bf16_bracket, fp32 outputs
        with assert_f32_bound(.., 4).

Epilogue order of every NT kernel (csrc/gemm.hip): v = alpha acc + bias; dropout; row scale (before); + residual; row scale (after); + old output.
"""
import functools

import numpy as np
import torch

BF = torch.bfloat16
F32 = torch.float32
NAN_BF16 = 0x7FA5                  # int16 pattern of a bf16 NaN
NAN_E4M3 = 0x7F                    # the e4m3 (OCP "fn") NaN
VMAX = 15
CAP = 2.0 ** 24
U = 2.0 ** -24
GAUSS_ALPHA = 0.37


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ------------------------------------------------------------------------------------------------ buffers
def embed(t, device="cpu", rows=(1, 2), col0=8, ld=None):
    """[R, C] (values exactly representable in bf16) -> a bf16 view [R, C] of a taller and wider buffer whose other elements are bf16 NaN patterns.
    The view starts col0 = 8 elements (16 bytes) into a row and the row stride is a multiple of 8 elements unless `ld` says otherwise."""
    R, C = t.shape
    ld = ld or ((C + col0 + 8 + 7) // 8) * 8
    assert ld >= C + col0
    buf = torch.full((R + rows[0] + rows[1], ld), NAN_BF16, dtype=torch.int16).view(BF)
    buf[rows[0]:rows[0] + R, col0:col0 + C] = t.to(BF)
    assert torch.equal(buf[rows[0]:rows[0] + R, col0:col0 + C].double(), t.double()), "operand is not exact in bf16"
    return buf.to(device)[rows[0]:rows[0] + R, col0:col0 + C]


def embed_e4m3(t, device="cpu", rows=(1, 2)):
    """[R, C] float64 (exact in e4m3) -> float8_e4m3fn view of a NaN-filled buffer; 16 bytes in, row stride a multiple of 16 bytes."""
    R, C = t.shape
    ld = ((C + 32 + 15) // 16) * 16
    codes = e4m3_encode(t.numpy())
    assert np.array_equal(E4M3_VALUES[codes], t.numpy()), "operand is not exact in e4m3"
    buf = torch.full((R + rows[0] + rows[1], ld), NAN_E4M3, dtype=torch.uint8)
    buf[rows[0]:rows[0] + R, 16:16 + C] = torch.from_numpy(codes)
    return buf.to(device).view(torch.float8_e4m3fn)[rows[0]:rows[0] + R, 16:16 + C]


# ------------------------------------------------------------------------------------------------ e4m3 table
def _e4m3_table():
    v = np.zeros(256, np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        mag = m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        v[c] = -mag if c & 0x80 else mag
    v[0x7F] = v[0xFF] = np.nan
    return v


E4M3_VALUES = _e4m3_table()                       # value of every e4m3 code (NaN for the two NaN codes)
_E4M3_POS = E4M3_VALUES[:0x7F]                    # codes 0 .. 0x7E: 0 .. 448, ascending


def e4m3_encode(x):
    """round-to-nearest-even over the table of finite e4m3 codes (ties go to the even code); |x| <= 448 -> uint8 codes"""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    assert np.all(a <= 448.0), "saturation is not part of this reference"
    hi = np.clip(np.searchsorted(_E4M3_POS, a, side="left"), 0, 0x7E)
    lo = np.clip(hi - 1, 0, 0x7E)
    dlo, dhi = a - _E4M3_POS[lo], _E4M3_POS[hi] - a
    code = np.where(dhi < dlo, hi, np.where(dlo < dhi, lo, np.where(hi % 2 == 0, hi, lo)))
    code = np.where(_E4M3_POS[hi] == a, hi, code)
    return (code | np.where(np.signbit(x) & (code != 0), 0x80, 0)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ exact family
def _ints(shape, g, vmax=VMAX):
    return torch.randint(-vmax, vmax + 1, shape, generator=g).double()


def _pow2(n, g):
    return 2.0 ** torch.randint(-3, 4, (n,), generator=g).double()


def needs_more_than_8_bits(ref):
    """share of the elements that a rounding to bf16 changes"""
    r = torch.as_tensor(ref, dtype=torch.float64)
    return float((r.float().to(BF).double() != r).double().mean())


NT_VARIANTS = ("plain", "bias", "bias+residual", "alpha", "alpha2", "f32", "f32+accumulate", "droppath before", "droppath after", "dropout+residual",
               "residual")
ROWS_PER_IMAGE = 77                              # rows_per_b / rs_rows of the epilogue cases: does not divide 128


def nt_reference(c, fac=None):
    """float64 [M, N] of a case dict (exact or gauss), in the kernels' epilogue order. fac: dropout factors [M, N] (from ops.dropout_mask) when
    the case drops. Also returns the epilogue intermediates (for the gauss tolerance)."""
    a, w = c["a"], c["w"]
    v = c.get("alpha", 1.0) * (a @ w.t())
    if c.get("bias") is not None:
        v = v + c["bias"][None, :]
    inter = [v]
    if c.get("drop") is not None:
        v = v * torch.as_tensor(fac, dtype=torch.float64)
    rs = c.get("row_scale")
    if rs is not None:
        rows = rs[0][torch.arange(a.shape[0]) // rs[1]][:, None]
        if not rs[2]:
            v = v * rows
    if c.get("residual") is not None:
        v = v + c["residual"]
        inter.append(v)
    if rs is not None and rs[2]:
        v = v * rows
    if c.get("out0") is not None:
        v = v + c["out0"]
        inter.append(v)
    return v, inter


def _nt_cap(c):
    """largest |intermediate| of any element, in units of the element's power-of-two scale (every factor of the chain at its largest)"""
    a, w = c["a"], c["w"]
    alpha = c.get("alpha", 1.0)
    unit = (c["sa"][:, None] * c["sw"][None, :]) * min(1.0, alpha)
    v = abs(alpha) * (a.abs() @ w.abs().t())
    if c.get("bias") is not None:
        v = v + c["bias"].abs()[None, :]
    if c.get("drop") is not None:
        v = v * 2.0
    rs = c.get("row_scale")
    if rs is not None:
        unit = unit * 0.5
        v = v * 2.0
    if c.get("residual") is not None:
        v = v + c["residual"].abs()
    if rs is not None:
        v = v * 2.0
    if c.get("out0") is not None:
        v = v + c["out0"].abs()
    return float((v / unit).max())


@functools.lru_cache(maxsize=None)
def exact_nt(M, N, K, variant="plain", seed=0, vmax=VMAX, share=True):
    """Exact-family case of out = epi(a [M, K] @ w [N, K]^T): dict of float64 CPU tensors a, w, sa, sw and the epilogue operands of `variant`
    (alpha, bias, residual, row_scale = (factors, rows, after), drop = (p, site, rows_per_b, t0), out0, out_f32)."""
    assert variant in NT_VARIANTS
    for attempt in range(32):
        g = _gen(M, N, K, NT_VARIANTS.index(variant), seed, attempt)
        c = dict(M=M, N=N, K=K, variant=variant, out_f32=variant.startswith("f32"))
        a, w = _ints((M, K), g, vmax), _ints((N, K), g, vmax)
        if variant == "plain":
            c["sa"], c["sw"] = _pow2(M, g), _pow2(N, g)
        else:
            c["sa"], c["sw"] = torch.ones(M, dtype=torch.float64), torch.ones(N, dtype=torch.float64)
        c["a"], c["w"] = a * c["sa"][:, None], w * c["sw"][:, None]
        if variant not in ("plain", "alpha2", "residual"):
            c["bias"] = _ints((N,), g, 1024)
        if variant in ("bias+residual", "droppath before", "droppath after", "dropout+residual", "residual"):
            c["residual"] = _ints((M, N), g, 255)
        if variant in ("alpha", "f32+accumulate"):
            c["alpha"] = 0.5
        if variant == "alpha2":
            c["alpha"] = 2.0
        if variant == "f32+accumulate":
            c["out0"] = _ints((M, N), g, 4096)
        if variant.startswith("droppath"):
            nimg = (M + ROWS_PER_IMAGE - 1) // ROWS_PER_IMAGE
            f = torch.tensor([0.0, 0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, (nimg,), generator=g)]
            if nimg >= 4:
                f[:4] = torch.tensor([2.0, 0.5, 0.0, 1.0], dtype=torch.float64)
            c["row_scale"] = (f, ROWS_PER_IMAGE, variant.endswith("after"))
        if variant == "dropout+residual":
            c["drop"] = (0.5, 7 + seed, ROWS_PER_IMAGE, 3)
        cap = _nt_cap(c)
        assert cap < CAP, f"exact family {M}x{N}x{K} {variant}: a partial sum may reach {cap:.3e} units, not below 2^24"
        c["cap"] = cap
        c["wide"] = needs_more_than_8_bits(nt_reference(c, None if "drop" not in c else torch.full((M, N), 2.0))[0])
        if not share or c["wide"] >= 0.25:
            return c
    raise AssertionError(f"exact family {M}x{N}x{K} {variant}: fewer than a quarter of the elements need more than 8 bits ({c['wide']:.2f})")


@functools.lru_cache(maxsize=None)
def exact_tn(R, I, J, alpha=1.0, seed=0, vmax=VMAX):
    """Exact-family case of out [I, J] += alpha p [R, I]^T q [R, J], db [I] += colsum(p): unscaled integers (the sum runs over the token rows, so
    a per-row scale would not factor out), integer-valued out0 / db0."""
    for attempt in range(32):
        g = _gen(R, I, J, int(alpha * 4), seed, attempt, 99)
        c = dict(R=R, I=I, J=J, alpha=alpha, p=_ints((R, I), g, vmax), q=_ints((R, J), g, vmax), out0=_ints((I, J), g, 1024), db0=_ints((I,), g, 1024))
        cap = float((abs(alpha) * (c["p"].abs().t() @ c["q"].abs()) + c["out0"].abs()).max()) / min(1.0, alpha)
        assert cap < CAP and R * vmax + 1024 < CAP, f"exact family TN {R}x{I}x{J}: a partial sum may reach {cap:.3e} units, not below 2^24"
        c["cap"] = cap
        c["wide"] = needs_more_than_8_bits(tn_reference(c)[0])
        if c["wide"] >= 0.25:
            return c
    raise AssertionError(f"exact family TN {R}x{I}x{J}: fewer than a quarter of the elements need more than 8 bits")


def tn_reference(c):
    """-> (out [I, J], db [I]) float64"""
    return c["out0"] + c["alpha"] * (c["p"].t() @ c["q"]), c["db0"] + c["p"].sum(0)


@functools.lru_cache(maxsize=None)
def exact_conv(Bn, Cin, N, H, W, seed=0):
    """Integer image x [Bn, H*W, Cin] (token-major) and 3 x 3 weights w [N, 9 Cin] in (ky, kx, c) order, each output channel scaled by a power of
    two, integer bias times that scale. Reference: torch conv2d (stride 2, padding 1) in float64 -> [Bn*Ho*Wo, N]."""
    g = _gen(Bn, Cin, N, H, W, seed, 3)
    x, w, sw = _ints((Bn, H * W, Cin), g), _ints((N, 9 * Cin), g), _pow2(N, g)
    bias = _ints((N,), g, 1024) * sw
    w = w * sw[:, None]
    cap = float(((x.abs().sum(-1).max() * VMAX * 9) + 1024))
    assert cap < CAP
    img = x.view(Bn, H, W, Cin).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(img, w.view(N, 3, 3, Cin).permute(0, 3, 1, 2), bias, stride=2, padding=1)
    Ho, Wo = ref.shape[2], ref.shape[3]
    ref = ref.permute(0, 2, 3, 1).reshape(Bn * Ho * Wo, N)
    return dict(x=x, w=w, bias=bias, ref=ref, Ho=Ho, Wo=Wo, wide=needs_more_than_8_bits(ref))


FP8_VARIANTS = ("bias", "residual", "rowscale before", "rowscale after")


@functools.lru_cache(maxsize=None)
def exact_fp8(M, N, K, variant, seed=0):
    """e4m3 integers, a power-of-two product scale (0.25) and the epilogue operands of `variant`; out_scale is the power of two that keeps the
    reference within 448."""
    assert variant in FP8_VARIANTS
    for attempt in range(32):
        g = _gen(M, N, K, FP8_VARIANTS.index(variant), seed, attempt, 8)
        c = dict(M=M, N=N, K=K, variant=variant, a=_ints((M, K), g), w=_ints((N, K), g), alpha=0.25, sa=torch.ones(M, dtype=torch.float64),
                 sw=torch.ones(N, dtype=torch.float64))
        if variant != "residual":
            c["bias"] = _ints((N,), g, 1024)
        if variant != "bias":
            c["residual"] = _ints((M, N), g, 255)
        if variant.startswith("rowscale"):
            nimg = (M + ROWS_PER_IMAGE - 1) // ROWS_PER_IMAGE
            f = torch.tensor([0.5, 2.0, 1.0, 0.0], dtype=torch.float64)[torch.arange(nimg) % 4]
            c["row_scale"] = (f, ROWS_PER_IMAGE, variant.endswith("after"))
        assert _nt_cap(c) < CAP
        ref = nt_reference(c)[0]
        c["wide"] = needs_more_than_8_bits(ref)
        c["out_scale"] = 2.0 ** int(np.ceil(np.log2(max(float(ref.abs().max()), 1.0) / 448.0)))
        assert float(ref.abs().max()) / c["out_scale"] <= 448.0
        if c["wide"] >= 0.25:
            return c
    raise AssertionError("fp8 exact family: too few wide elements")


# ------------------------------------------------------------------------------------------------ gauss family
def _bf(t):
    return t.to(BF).double()


def gauss_nt(M, N, K, variant="bias+residual", seed=0):
    """Gauss-family case; variant: plain | bias | bias+residual | f32 | f32+accumulate | dropout+residual (alpha = 0.37 in all but plain)."""
    g = _gen(M, N, K, seed, 1234)
    a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    hot = torch.randperm(K, generator=g)[: max(1, K // 10)]
    a[:, hot] *= 64.0
    a, w = _bf(a), _bf(w)
    h = K // 2
    w[0, h:] = w[0, :h]
    a[0, h:] = -a[0, :h]                                             # out[0, 0] cancels to zero exactly
    if M >= 2:
        a[M - 1] = -a[0]
    c = dict(M=M, N=N, K=K, variant=variant, a=a, w=w, out_f32=variant.startswith("f32"))
    if variant != "plain":
        c["alpha"] = GAUSS_ALPHA
        c["bias"] = torch.randn(N, generator=g).float().double()
    if variant in ("bias+residual", "dropout+residual"):
        c["residual"] = _bf(torch.randn(M, N, generator=g))
    if variant == "f32+accumulate":
        c["out0"] = torch.randn(M, N, generator=g).float().double() * 8.0
    if variant == "dropout+residual":
        c["drop"] = (0.5, 11 + seed, ROWS_PER_IMAGE, 3)
    return c


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def gauss_nt_tol(c, fac=None):
    """-> (ref, tol) float64 numpy [M, N] (module docstring)"""
    ref, inter = nt_reference(c, fac)
    tol = abs(c.get("alpha", 1.0)) * 2.0 * c["K"] * U * (c["a"].abs() @ c["w"].abs().t()).numpy() + 4.0 * ulp32(inter[0].numpy())
    if c.get("drop") is not None:
        tol = tol * np.asarray(torch.as_tensor(fac).cpu(), np.float64)      # the factor (0 or 2) is exact
    for v in inter[1:]:
        tol = tol + 4.0 * ulp32(v.numpy())
    return ref.numpy(), tol


def gauss_tn(R, I, J, alpha=GAUSS_ALPHA, seed=0):
    g = _gen(R, I, J, seed, 4321)
    p, q = torch.randn(R, I, generator=g), torch.randn(R, J, generator=g)
    hot = torch.randperm(R, generator=g)[: max(1, R // 10)]
    p[hot] *= 64.0
    p, q = _bf(p), _bf(q)
    if I >= 2:
        p[:, I - 1] = -p[:, 0]
    return dict(R=R, I=I, J=J, alpha=alpha, p=p, q=q, out0=torch.randn(I, J, generator=g).float().double() * 8.0,
                db0=torch.randn(I, generator=g).float().double())


def gauss_tn_tol(c):
    """-> (out, tol_out, db, tol_db): R in place of K; the intermediates are alpha acc and the sum with the old output"""
    out, db = tn_reference(c)
    prod = c["alpha"] * (c["p"].t() @ c["q"])
    tol = abs(c["alpha"]) * 2.0 * c["R"] * U * (c["p"].abs().t() @ c["q"].abs()).numpy() + 4.0 * ulp32(prod.numpy()) + 4.0 * ulp32(out.numpy())
    tol_db = 2.0 * c["R"] * U * c["p"].abs().sum(0).numpy() + 4.0 * ulp32(c["p"].sum(0).numpy()) + 4.0 * ulp32(db.numpy())
    return out.numpy(), tol, db.numpy(), tol_db


# ------------------------------------------------------------------------------------------------ comparers
def assert_exact(out, ref, what):
    """out: fp32 or bf16 tensor; ref: float64, exact. fp32 must equal ref, bf16 its round-to-nearest-even (values: -0 == +0, a NaN equals nothing)"""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    out = out.detach().cpu()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    exp = ref.float() if out.dtype == F32 else ref.float().to(BF)
    if out.dtype == F32:
        assert torch.equal(exp.double(), ref), f"{what}: the reference itself is not exact in fp32"
    if not torch.equal(out, exp):
        bad = (out != exp) | torch.isnan(out)
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact value, first at {i}: got {float(out[i])!r}, "
                             f"exact {float(ref[i])!r}")


def assert_exact_e4m3(codes, ref, out_scale, what):
    """codes: uint8 tensor of e4m3 codes; the values must equal RNE(ref / out_scale) over the finite e4m3 codes"""
    got = E4M3_VALUES[codes.detach().cpu().numpy()]
    exp = E4M3_VALUES[e4m3_encode(np.asarray(ref, np.float64) / out_scale)]
    bad = ~(got == exp)
    assert not bad.any(), f"{what}: {int(bad.sum())} e4m3 elements differ, first: got {got[bad][0]!r} for {np.asarray(ref)[bad][0] / out_scale!r}"


def assert_gauss(out, ref, tol, what):
    """-> largest |err| / tol-figure of the comparer used (bf16: fraction of the bracket's half-width; fp32: of tol + 4 fp32 steps)"""
    from bounds_util import assert_bf16_bracket, assert_f32_bound
    out = out.detach()
    ref, tol = np.asarray(ref, np.float64), np.asarray(tol, np.float64)
    assert np.isfinite(out.float().cpu().numpy()).all(), f"{what}: non-finite output"
    if out.dtype == BF:
        return assert_bf16_bracket(out, ref, tol, what)
    assert_f32_bound(out, ref, tol.ravel(), 4, what)
    return float(np.max(np.abs(out.cpu().double().numpy() - ref) / (tol + 4.0 * ulp32(ref))))


# ------------------------------------------------------------------------------------------------ weight-gradient launch plan
def tn_plan(R, I, J, target=176):
    """Token splits gemm_tn_kernel takes for a shape that stays on the 128 x 128-tile kernel (csrc/gemm.hip tn_plan with its shipped settings);
    the GPU test checks this against cxr_gemm_tn_plan."""
    tiles = -(-I // 128) * -(-J // 128)
    nrt = -(-R // 32)
    splits = max(1, min(-(-target // tiles), max(1, nrt // 8)))
    per = -(-nrt // splits)
    return -(-nrt // per), per, nrt


def tn_split_class(splits):
    return "atomic" if splits == 1 else ("SL1" if splits <= 12 else ("SL4" if splits <= 48 else "SL16"))


# ------------------------------------------------------------------------------------------------ case tables (M, N, K) / (R, I, J)
_K32, _K64 = (32, 96, 160, 224), (64, 128, 192, 320)
TILED_BN64 = [(257, 196, k) for k in _K32 + _K64] + [(1, 4, 32), (17, 60, 96), (127, 64, 160), (128, 68, 224), (129, 132, 64), (1, 196, 128),
                                                    (129, 4, 192), (128, 60, 320), (17, 68, 64), (127, 132, 128)]
TILED_BN128 = [(16513, 224, 96), (16513, 228, 64), (16513, 256, 192), (16513, 228, 96)]
TILED_REGSTAGE = [(129, 196, 96), (257, 132, 128)]
TILED_STAGES = [(257, 196, k) for k in (32, 64, 96, 160)]
TILED_EPILOGUE = [(257, 196, 96), (129, 68, 128)]
TILED_LD4 = (257, 196, 96)                                        # + an output row stride of 4 mod 8 elements: the per-lane epilogue
GROUPS = [((257, 1, 129), 196, 96), ((129, 130), 64, 64)]
CONVS = [(1, 64, 64, 3, 3), (2, 64, 196, 7, 5), (1, 128, 132, 9, 20), (1, 64, 64, 1, 1)]       # (Bn, Cin, N, H, W); the last: 8 of 9 taps are padding
STRIP384 = [(2, 0), (4, 0), (6, 0), (10, 0), (10, 2), (10, 3), (10, 4)]                       # (mt, stages)
STRIP192 = [8, 12, 16]
STRIP_VARIANTS = ("plain", "bias+residual", "droppath before", "droppath after")


def strip_shapes(mt, n192=False):
    ms = (1, 16 * mt - 1, 16 * mt + 1, 32 * mt + 17)
    ks = (64, 192) if n192 else _K64
    return [(m, 192 if n192 else 384, ks[(i + j) % len(ks)]) for i, m in enumerate(ms) for j in range(2)]


WS = [(1, 384, 384), (31, 768, 384), (32, 1152, 384), (33, 384, 384), (65, 768, 384), (1000, 1152, 384), (1000, 384, 384), (33, 768, 384)]
WS_VARIANTS = ("plain", "bias+residual")
PK = [(1, 8, 64), (63, 136, 128), (65, 264, 192), (255, 8, 128), (257, 136, 192), (513, 264, 64), (513, 8, 192), (257, 264, 128)]
PK_VARIANTS = ("plain", "bias+residual", "f32")
TN4 = [(1, 8, 8), (31, 72, 128), (32, 128, 136), (33, 136, 72), (255, 200, 264), (257, 264, 200), (1025, 72, 8), (3401, 128, 128), (3401, 264, 200),
       (3401, 8, 264), (8001, 128, 72), (16001, 128, 128)]
TN_LD4 = (257, 264, 200)
TN2 = [(r, i, j) for (i, j) in ((136, 136), (256, 264), (520, 136)) for r in (33, 257, 4129)]
TN5 = [(r, i, j) for (i, j) in ((384, 192), (384, 576), (768, 192)) for r in (33, 257, 4129)]
TN_STAGES2 = [(33, 136, 72), (257, 264, 200), (3401, 128, 128), (8001, 128, 72)]
SKINNY = [(1, 1, 128), (15, 15, 384), (16, 16, 768), (17, 17, 2048), (33, 100, 3072), (48, 1, 768), (49, 15, 2048), (64, 100, 384), (64, 17, 3072)]
SKINNY_VARIANTS = ("plain", "bias+residual", "f32", "dropout")
SKINNY3 = [(17, 100, 384), (49, 16, 768), (64, 136, 2048)]
FP8 = [(1, 64, 64), (127, 68, 128), (129, 132, 192), (129, 64, 128), (1, 132, 64), (127, 132, 192), (129, 68, 64)]

# ------------------------------------------------------------------------------------------------ decode-step GEMM (csrc/decode_gemm.hip)
# (M, K, the N of each problem of the launch, output kind: rows | f32 | dal, variant: plain | bias | bias+residual | dropout, mt_hint)
# dal: problem 0 writes the decode activation layout and takes a residual in that layout (N % 32 == 0: the layout's 32-column blocks)
DEC = [(1, 768, (16,), "rows", "bias", 0), (15, 768, (18, 48), "rows", "plain", 1), (16, 3072, (48,), "f32", "bias", 0),
       (17, 768, (770, 16, 18), "rows", "dropout", 0), (33, 3072, (770,), "f32", "dropout", 1), (47, 768, (96, 48), "dal", "bias+residual", 0),
       (64, 768, (96,), "dal", "bias+residual", 1), (64, 3072, (18, 770), "rows", "bias", 0), (16, 768, (16, 770), "f32", "plain", 1)]
DEC_VOCAB = (33, 768, 8192)                                      # with nc_hint 1 and 4


@functools.lru_cache(maxsize=None)
def dec_case(M, K, Ns, variant, family="exact", seed=0):
    """One activation matrix a [M, K] and a weight (and bias) per problem; residual [M, Ns[0]] for problem 0; drop = (p, site, t).
    exact: integers (plain: rows of a and of every w scaled by powers of two); gauss: as gauss_nt, without alpha."""
    g = _gen(M, K, sum(Ns), len(Ns), seed, 77, family == "exact")
    c = dict(M=M, K=K, Ns=Ns, variant=variant, family=family, bias=[None] * len(Ns), residual=None, drop=None)
    if family == "exact":
        sa = _pow2(M, g) if variant == "plain" else torch.ones(M, dtype=torch.float64)
        c["a"] = _ints((M, K), g) * sa[:, None]
        c["w"] = [_ints((N, K), g) * (_pow2(N, g) if variant == "plain" else torch.ones(N, dtype=torch.float64))[:, None] for N in Ns]
        if variant != "plain":
            c["bias"] = [_ints((N,), g, 1024) for N in Ns]
        if variant == "bias+residual":
            c["residual"] = _ints((M, Ns[0]), g, 255)
        assert VMAX * VMAX * K * 2 + 1024 * 2 + 255 < CAP
    else:
        a = torch.randn(M, K, generator=g)
        a[:, torch.randperm(K, generator=g)[: K // 10]] *= 64.0
        a = _bf(a)
        c["w"] = [_bf(torch.randn(N, K, generator=g)) for N in Ns]
        h = K // 2
        c["w"][0][0, h:] = c["w"][0][0, :h]
        a[0, h:] = -a[0, :h]
        if M >= 2:
            a[M - 1] = -a[0]
        c["a"] = a
        if variant != "plain":
            c["bias"] = [torch.randn(N, generator=g).float().double() for N in Ns]
        if variant == "bias+residual":
            c["residual"] = _bf(torch.randn(M, Ns[0], generator=g))
    if variant == "dropout":
        c["drop"] = (0.5, 19 + seed, 7)
    return c


def dec_reference(c, fac=None):
    """-> [(ref, tol)] float64 numpy per problem (tol: the gauss bound); fac: dropout factors [M, max N]. Order of the kernel's epilogue: sum of the
    waves' partial products + bias; dropout; + residual (problem 0)."""
    out = []
    for i, (N, w) in enumerate(zip(c["Ns"], c["w"])):
        v = c["a"] @ w.t()
        if c["bias"][i] is not None:
            v = v + c["bias"][i][None, :]
        tol = 2.0 * c["K"] * U * (c["a"].abs() @ w.abs().t()).numpy() + 4.0 * ulp32(v.numpy())
        if c["drop"] is not None:
            f = torch.as_tensor(fac, dtype=torch.float64)[:, :N]
            v, tol = v * f, tol * f.numpy()
        if i == 0 and c["residual"] is not None:
            v = v + c["residual"]
            tol = tol + 4.0 * ulp32(v.numpy())
        out.append((v.numpy(), tol))
    return out
