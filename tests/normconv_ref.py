"""Seeded input families, float64 references, per-element bounds, launch-plan mirrors and mutants of the depthwise-projection (csrc/dwproj.hip)
and LayerNorm (csrc/norm.hip) tests. tests/test_normconv_exact_gpu.py runs them on the HIP kernels, tests/test_normconv_ref.py checks this file
itself without a GPU. Everything here is torch float64 and device-agnostic: the GPU test evaluates the same functions on the device.

exact   Activations and gradients are random integers stored in bf16, taps / shifts / coefficients integers times a per-channel power of two in
        fp32; every product and every partial sum, in any order, stays below 2^24 units (asserted per case from sum |terms|), so a correct kernel
        returns THE integer (fp32) or its round-to-nearest-even (bf16, e4m3) whatever its summation order. Ranges per entry point:
          apply      x |v| <= 15, taps |v| <= 15, shift |v| <= 2048               (|y| <= 4073 units)
          apply_q8   x, taps in {-1, 0, 1}, shift |v| <= 7, scale 0.25 | 2        (|y| <= 16: y / scale is an e4m3 value, asserted)
          dx, taps   dc |v| <= 100, taps |v| <= 15, x |v| <= 15                   (dx: <= 17 terms; tap sums: count terms, asserted < 2^24)
          statistics x, taps |v| <= 3, dy |v| <= 7, mean in -2 .. 2, rstd in {0.5, 1, 2}: sum c, sum dy and sum dy c are integers below 2^24.
                     Observable exactly: the forward mean = fl32(S0 / count) (one correctly rounded fp32 division), dbeta = db0 + S and
                     dgamma = dg0 + rstd (D - mean S). The forward variance (a difference of fp32 quotients that the compiler may contract)
                     and the dc coefficients (quotients) are not; the gauss family bounds them.
        At least WIDE_SHARE = a quarter of the bf16 outputs of apply and dx need more than 8 significant bits (asserted in the generator).

gauss   N(0, 1) activations plus a per-channel offset in [-2, 2] (channel means well away from zero: E[c^2] - mean^2 cancels in fp32), a few
        pixels scaled by 16, BatchNorm parameters in the style of pretrained ones, one 64-channel slice with a |gamma rstd| < 1e-3 channel and
        one with |beta| > 8 |gamma| (the gates of the streaming backward statistics). Every bound is derived from the reference's own magnitudes;
        U = 2^-24 is the fp32 unit roundoff. The building block: a sum of n fp32 terms (products by fma count as terms) in ANY order is off by at
        most n U sum |terms|; no bound below knows the kernels' summation order. Derivations stand next to each bound. The fp32 outputs add a
        few fp32 steps of the result itself (assert_f32_bound's `ulps`), the bf16 outputs the bracket of bounds_util.assert_bf16_bracket.

        Looseness: the any-order bound grows with the number of terms, so at 10^4 .. 10^5 terms (batch statistics, dgamma of 131 k rows) it is
        several orders above what the kernels need. Mutants the gauss bounds do NOT reject although the exact family does: one partial row
        dropped from (or added twice to) a row reduction at large counts, and dead rows added to dbeta (tests/test_normconv_ref.py says
        which and checks that the exact family catches them). The bounds are not tightened past their derivation.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from gemm_ref import CAP, E4M3_VALUES, NAN_BF16, U, _gen, e4m3_encode, needs_more_than_8_bits

BF = torch.bfloat16
F64 = torch.float64
WIDE_SHARE = 0.25
EPS = float(np.float32(1e-5))                      # the kernels take eps and momentum as fp32
MOMENTUM = float(np.float32(0.1))


def f32r(t):
    """float64 -> the float64 value of its fp32 rounding (an fp32 operand of a kernel)"""
    return t.float().double()


def bfr(t):
    return t.to(BF).double()


def ulp32_t(t):
    """spacing of fp32 at |t| (float64 tensor)"""
    a = t.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


# ------------------------------------------------------------------------------------------------ launch-plan mirrors
# csrc/dwproj.hip: DW3_LDS_CAP, DW3_LDS_MAX, DW3_RED_SMALL, DW3_RED_TAPS, the wl[3][12][64] arrays, dw3_bytes_x, dw3_bytes_dx
DW3_LDS_CAP, DW3_LDS_MAX = 80 * 1024, 156 * 1024
DW3_STATIC = {"apply": 0, "stats": 512 * 4, "bwd_stats": 512 * 4, "dc": (2560 + 3 * 12 * 64) * 4, "dx": 3 * 12 * 64 * 4}
DW3_KERNELS = tuple(DW3_STATIC)


def dw3_bytes(kernel, band, W, strides):
    if kernel != "dx":
        return (band + 2) * (W + 2) * 128
    return sum((band + 2) * (W + 2) * 128 if s == 1 else (band // 2 + 1) * (W // 2 + 1) * 128 for s in strides)


def _dw3_pick_band(kernel, Bn, H, W, nslices, strides, cap, forced):
    """mirror of dw3_pick_band (csrc/dwproj.hip); forced = the CXR_DW3_BAND override (0: none). The library has no entry point that reports the band
    it launched (LayerNorm has cxr_layernorm_bwd_grid), so nothing compares this mirror with the picker at run time: whoever changes dw3_pick_band,
    dw3_plan, the LDS budgets or a kernel's static LDS changes this mirror and DW3_STATIC with it, or the cases quietly test another band."""
    static = DW3_STATIC[kernel]
    if forced >= 2 and not forced & 1 and dw3_bytes(kernel, forced, W, strides) + static <= cap:
        return forced
    best = fallback = best_cost = 0
    for band in range(2, ((H + 1) & ~1) + 1, 2):
        if dw3_bytes(kernel, band, W, strides) + static > cap:
            break
        nb = -(-H // band)
        fallback = fallback or band
        if Bn * nb * nslices < 384:
            continue
        cost = nb * (band + 2)
        if not best or cost <= best_cost:
            best, best_cost = band, cost
    return best or fallback


def dw3_plan(kernel, Bn, C, H, W, strides, forced=0):
    """mirror of dw3_plan's geometry: dict(band, nbands, last = rows in the last band, big = the one-workgroup-per-CU budget DW3_LDS_MAX is
    used, lds = dynamic + static bytes, G = partial rows of the row reductions)"""
    big = False
    band = _dw3_pick_band(kernel, Bn, H, W, C // 64, strides, DW3_LDS_CAP, forced)
    if band < 2:
        band, big = _dw3_pick_band(kernel, Bn, H, W, C // 64, strides, DW3_LDS_MAX, forced), True
    assert band >= 2, "W too large for this kernel family"
    nb = -(-H // band)
    return dict(band=band, nbands=nb, last=H - (nb - 1) * band, big=big, lds=dw3_bytes(kernel, band, W, strides) + DW3_STATIC[kernel], G=Bn * nb)


# csrc/norm.hip: rows per workgroup and iteration = 4 waves x LNCfg::RPW x U of the dispatch tables; grid caps of ln_grid / cxr_layernorm_bwd_grid
LN_BWD_RPB = {64: 64, 128: 32, 192: 32, 384: 8, 768: 4}
LN_FWD_RPB = {64: 128, 128: 64, 192: 64, 384: 32, 768: 16, 1024: 8}
LN_BWD_CAP, LN_FWD_CAP = 512, 4096
LN_BWD_KR = ((0, 1), (0, -1), (1, 0), (1, 3), (2, None), (3, 0), (3, 5), (4, 1))        # r = -1: rpb - 1; None: rpb + 1
LN_REDUCE_GRIDS = (1, 63, 64, 65, 512)


def ln_bwd_rows(C):
    """the row counts of the backward cases of width C: rows = 512 rpb k + r, then the reduce grids 63, 64 and 65"""
    rpb = LN_BWD_RPB[C]
    rows = [LN_BWD_CAP * rpb * k + (rpb - 1 if r == -1 else (rpb + 1 if r is None else r)) for k, r in LN_BWD_KR]
    return rows + [63 * rpb - 1, 64 * rpb, 64 * rpb + 1]


def ln_plan(rows, C, fwd=False):
    """dict(grid, it_min, it_max = loop iterations of the least / most loaded workgroup, dead = rows of the last row group past `rows`)"""
    rpb, cap = (LN_FWD_RPB[C], LN_FWD_CAP) if fwd else (LN_BWD_RPB[C], LN_BWD_CAP)
    blocks = -(-rows // rpb)
    grid = min(blocks, cap)
    return dict(grid=grid, it_min=blocks // grid, it_max=-(-blocks // grid), dead=blocks * rpb - rows, rpb=rpb)


# ------------------------------------------------------------------------------------------------ buffers
def embed3(t, device="cpu", front=1, ld=None, images=1):
    """[Bn, L, C] (exact in bf16) -> bf16 view of a NaN-filled [Bn + images, front + L + 2, ld] buffer: base[:Bn, front:front + L, :C]. front = 1 is a
    view behind a class token, ld > C a padded row stride; the batch stride is never the contiguous one."""
    Bn, L, C = t.shape
    ld = ld or C
    assert ld >= C and ld % 8 == 0
    buf = torch.full((Bn + images, front + L + 2, ld), NAN_BF16, dtype=torch.int16).view(BF)
    buf[:Bn, front:front + L, :C] = t.to(BF)
    assert torch.equal(buf[:Bn, front:front + L, :C].double(), t.double().cpu()), "operand is not exact in bf16"
    return buf.to(device)[:Bn, front:front + L, :C]


def out_hw(H, W, st):
    return (H - 1) // st + 1, (W - 1) // st + 1


def img(t, tok0, H, W):
    """[Bn, tok0 + H W, C] -> the spatial tokens as [Bn, H, W, C]"""
    return t[:, tok0:].reshape(t.shape[0], H, W, t.shape[2])


# ------------------------------------------------------------------------------------------------ depthwise 3 x 3 in float64 (pad 1, taps [9, C], t = 3 ky + kx)
def _win(p, ky, kx, st, Ho, Wo):
    return p[:, ky:ky + st * (Ho - 1) + 1:st, kx:kx + st * (Wo - 1) + 1:st]


def conv_taps(x, taps, st):
    """x [Bn, H, W, C] -> [Bn, Ho, Wo, C]: sum_t taps[t] x[oy st + ky - 1, ox st + kx - 1]"""
    Ho, Wo = out_hw(x.shape[1], x.shape[2], st)
    p = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros((x.shape[0], Ho, Wo, x.shape[3]), dtype=F64, device=x.device)
    for t in range(9):
        out += _win(p, t // 3, t % 3, st, Ho, Wo) * taps[t]
    return out


def tap_sums(x, dc, st):
    """-> [10, C]: G[t] = sum dc x_t over the launch (the raw-tap gradient), then S = sum dc"""
    Ho, Wo = dc.shape[1], dc.shape[2]
    p = F.pad(x, (0, 0, 1, 1, 1, 1))
    rows = [(_win(p, t // 3, t % 3, st, Ho, Wo) * dc).sum((0, 1, 2)) for t in range(9)]
    return torch.stack(rows + [dc.sum((0, 1, 2))])


def dx_taps(dcs, tapss, strides, H, W):
    """input gradient of sum_q conv_taps(x, taps_q, st_q) . dc_q -> [Bn, H, W, C]"""
    Bn, C = dcs[0].shape[0], dcs[0].shape[3]
    acc = torch.zeros((Bn, H + 2, W + 2, C), dtype=F64, device=dcs[0].device)
    for dc, taps, st in zip(dcs, tapss, strides):
        Ho, Wo = dc.shape[1], dc.shape[2]
        for t in range(9):
            _win(acc, t // 3, t % 3, st, Ho, Wo).add_(dc * taps[t])
    return acc[:, 1:H + 1, 1:W + 1]


def with_cls(cls_rows, body):
    """class-token rows [Bn, tok0, C] in front of a map [Bn, h, w, C] -> [Bn, tok0 + h w, C]"""
    return torch.cat([cls_rows, body.reshape(body.shape[0], -1, body.shape[3])], 1)


# ------------------------------------------------------------------------------------------------ exact family: depthwise projections
def _ints(shape, g, vmax):
    return torch.randint(-vmax, vmax + 1, shape, generator=g).double()


def _pow2(n, g, lo=-1, hi=1):
    return 2.0 ** torch.randint(lo, hi + 1, (n,), generator=g).double()


@functools.lru_cache(maxsize=None)
def dw_exact(Bn, C, H, W, tok0, strides, seed=0):
    """Exact-family case of all entry points on one geometry (module docstring); per projection a dict in c["p"]. References are attached:
    y, y8 (e4m3 values times scale), dx, GS, dw, mean, dgamma, dbeta."""
    g = _gen(Bn, C, H, W, tok0, sum(s * 3 ** i for i, s in enumerate(strides)), seed, 51)
    L = tok0 + H * W
    c = dict(Bn=Bn, C=C, H=H, W=W, tok0=tok0, strides=strides, x=_ints((Bn, L, C), g, 15), x8=_ints((Bn, L, C), g, 1), xs=_ints((Bn, L, C), g, 3), p=[])
    xi, x8i, xsi = img(c["x"], tok0, H, W), img(c["x8"], tok0, H, W), img(c["xs"], tok0, H, W)
    for q, st in enumerate(strides):
        Ho, Wo = out_hw(H, W, st)
        n = Bn * Ho * Wo
        sc = _pow2(C, g)
        p = dict(stride=st, Ho=Ho, Wo=Wo, count=n, taps=_ints((9, C), g, 15) * sc, shift=_ints((C,), g, 2048) * sc, taps8=_ints((9, C), g, 1),
                 shift8=_ints((C,), g, 7), scale8=(0.25, 2.0)[q % 2], dy=_ints((Bn, tok0 + Ho * Wo, C), g, 100), taps_s=_ints((9, C), g, 3),
                 dys=_ints((Bn, tok0 + Ho * Wo, C), g, 7), mean_in=_ints((C,), g, 2), rstd_in=_pow2(C, g), dg0=_ints((C,), g, 1024),
                 db0=_ints((C,), g, 1024), dw0=_ints((C, 9), g, 1024))
        # ---- apply
        p["y"] = with_cls(c["x"][:, :tok0], conv_taps(xi, p["taps"], st) + p["shift"])
        y8 = with_cls(c["x8"][:, :tok0], conv_taps(x8i, p["taps8"], st) + p["shift8"])
        v8 = (y8 / p["scale8"]).numpy()
        assert np.array_equal(E4M3_VALUES[e4m3_encode(v8)], v8), "exact family: an e4m3 output is not representable"
        p["y8"] = y8
        # ---- tap sums of dy (no coefficients): every partial sum of every column is bounded by sum |terms|
        dyi = img(p["dy"], tok0, Ho, Wo)
        cap = float(tap_sums(xi.abs(), dyi.abs(), st).max()) + 1024.0
        assert cap < CAP, f"exact family {Bn}x{C}x{H}x{W}: a tap sum may reach {cap:.3e}, not below 2^24"
        p["GS"] = tap_sums(xi, dyi, st)
        p["dw"] = p["dw0"] + p["GS"][:9].t()
        # ---- statistics: S0 = sum c, S = sum dy, D = sum dy c
        cs, cabs, dysi = conv_taps(xsi, p["taps_s"], st), conv_taps(xsi.abs(), p["taps_s"].abs(), st), img(p["dys"], tok0, Ho, Wo)
        # S0 <= sum |c|; D - mean S <= sum |dy c| + 2 sum |dy|, then + dg0 in units of rstd = 0.5 (x 2)
        cap = max(float(cabs.sum((0, 1, 2)).max()), 2.0 * (float((dysi.abs() * cabs).sum((0, 1, 2)).max()) + 2.0 * float(dysi.abs().sum((0, 1, 2)).max()) + 1024.0))
        assert cap < CAP, f"exact family {Bn}x{C}x{H}x{W}: a statistics sum may reach {cap:.3e} units, not below 2^24"
        p["mean"] = f32r(cs.sum((0, 1, 2)) / n)
        S, D = dysi.sum((0, 1, 2)), (dysi * cs).sum((0, 1, 2))
        p["dbeta"], p["dgamma"] = p["db0"] + S, p["dg0"] + p["rstd_in"] * (D - p["mean_in"] * S)
        c["p"].append(p)
    c["dx"] = with_cls(sum(p["dy"][:, :tok0] for p in c["p"]),
                       dx_taps([img(p["dy"], tok0, p["Ho"], p["Wo"]) for p in c["p"]], [p["taps"] for p in c["p"]], strides, H, W))
    c["wide"] = min([needs_more_than_8_bits(p["y"][:, tok0:]) for p in c["p"]] + [needs_more_than_8_bits(c["dx"][:, tok0:])])
    assert c["wide"] >= WIDE_SHARE, f"exact family {Bn}x{C}x{H}x{W} {strides}: only {c['wide']:.2f} of the bf16 outputs need more than 8 bits"
    return c


# ------------------------------------------------------------------------------------------------ gauss family: depthwise projections
@functools.lru_cache(maxsize=None)
def dw_gauss(Bn, C, H, W, tok0, strides, seed=0):
    """Gauss-family inputs (module docstring): x, and per projection w [C, 9], taps = w^T, gamma, beta, run_mean, run_var, dy, dg0, db0, dw0.
    Projection 1 has a channel with gamma = 1e-4 in its first slice, the last projection |beta| = 20 |gamma| in a channel of its last slice."""
    g = _gen(Bn, C, H, W, tok0, sum(s * 3 ** i for i, s in enumerate(strides)), seed, 52)
    L = tok0 + H * W
    x = torch.randn(Bn, L, C, generator=g).double() + (torch.rand(C, generator=g).double() * 4.0 - 2.0)
    hot = torch.randint(0, Bn * L * C, (4,), generator=g)
    x.view(-1)[hot] *= 16.0
    c = dict(Bn=Bn, C=C, H=H, W=W, tok0=tok0, strides=strides, x=bfr(x), p=[])
    for q, st in enumerate(strides):
        Ho, Wo = out_hw(H, W, st)
        r = lambda *s: torch.randn(*s, generator=g).double()
        p = dict(stride=st, Ho=Ho, Wo=Wo, count=Bn * Ho * Wo, w=f32r(0.3 * r(C, 9)), gamma=f32r((1.0 + 0.3 * r(C)).abs() + 0.05), beta=f32r(0.3 * r(C)),
                 run_mean=f32r(0.1 * r(C)), run_var=f32r(1.0 + 0.1 * r(C).abs()), dy=bfr(r(Bn, tok0 + Ho * Wo, C)), dg0=f32r(r(C)), db0=f32r(r(C)),
                 dw0=f32r(r(C, 9)))
        if q == 1:
            p["gamma"][5] = float(np.float32(1e-4))
        if q == len(strides) - 1:
            p["gamma"][C - 64 + 7], p["beta"][C - 64 + 7] = float(np.float32(0.05)), 1.0
        p["taps"] = p["w"].t().contiguous()
        c["p"].append(p)
    return c


def _rstd_bound(var, tol_var, eps):
    """rstd = (var + eps)^-1/2 and its bound for a variance within tol_var of var, clamped at 0 as the kernels clamp it: the function is monotone, so
    the bound is its value at the two ends; + U rstd for the rounding of var + eps (relative U on the argument is U / 2 on the result)"""
    rstd = (var + eps) ** -0.5
    lo, hi = (var - tol_var).clamp_min(0.0), var + tol_var
    return rstd, torch.maximum((lo + eps) ** -0.5 - rstd, rstd - (hi + eps) ** -0.5) + U * rstd


def dw_train_stats_ref(x, p, eps=EPS, momentum=MOMENTUM):
    """dwproj_bn_train_stats of one projection; x [Bn, H, W, C]. -> dict name -> (ref, tol, ulps) for mean, rstd, run_mean, run_var, taps [9, C], shift"""
    st, taps = p["stride"], p["taps"]
    c, A = conv_taps(x, taps, st), conv_taps(x.abs(), taps.abs(), st)
    N = float(p["count"])
    e = 9.0 * U * A                                               # |fl(c_i) - c_i|: 9 fma terms, sum |terms| = A_i
    # S0 = sum of N computed c_i in any order: N U sum |fl(c_i)| + sum e_i, with |fl(c_i)| <= A_i (1 + 9 U)
    tol_s0 = (N + 10.0) * U * A.sum((0, 1, 2))
    mean = c.sum((0, 1, 2)) / N
    tol_mean = tol_s0 / N + ulp32_t(mean)                         # + the rounding of the division
    # S1 = sum fl(c_i)^2: (|c_i| + e_i)^2 bounds each term, 2 |c_i| e_i + e_i^2 its distance from c_i^2
    tol_s1 = (N + 2.0) * U * ((c.abs() + e) ** 2).sum((0, 1, 2)) + (2.0 * c.abs() * e + e * e).sum((0, 1, 2))
    ex2 = (c * c).sum((0, 1, 2)) / N
    var = ((c - mean) ** 2).sum((0, 1, 2)) / N
    # var = fl(S1 / N) - fl(mean)^2: the two operands' errors, then the division, the square and the difference, each rounded at the operands' size
    tol_var = tol_s1 / N + (2.0 * mean.abs() + tol_mean) * tol_mean + 4.0 * U * (ex2 + mean * mean)
    rstd, tol_rstd = _rstd_bound(var, tol_var, eps)
    tr = tol_rstd + 4.0 * ulp32_t(rstd)                           # what a consumer of the stored rstd sees (rsqrtf: a few fp32 steps)
    tm = tol_mean
    out = dict(mean=(mean, tol_s0 / N, 1), rstd=(rstd, tol_rstd, 4))
    rm = (1.0 - momentum) * p["run_mean"] + momentum * mean
    out["run_mean"] = (rm, momentum * tm + 3.0 * U * ((1.0 - momentum) * p["run_mean"].abs() + momentum * mean.abs()), 2)
    unb = N / (N - 1.0) if N > 1 else 1.0
    out["run_var"] = ((1.0 - momentum) * p["run_var"] + momentum * var * unb,
                      momentum * unb * tol_var + 4.0 * U * ((1.0 - momentum) * p["run_var"].abs() + momentum * unb * (var + tol_var)), 2)
    sc = p["gamma"] * rstd
    tol_sc = p["gamma"].abs() * tr + U * sc.abs()
    out["taps"] = (p["w"].t() * sc, p["w"].t().abs() * tol_sc + U * (p["w"].t() * sc).abs(), 2)
    out["shift"] = (p["beta"] - mean * sc, sc.abs() * tm + (mean.abs() + tm) * tol_sc + 3.0 * U * (p["beta"].abs() + (mean * sc).abs()), 2)
    return out


def dw_apply_ref(x, taps, shift, st):
    """-> (y [Bn, Ho, Wo, C], tol): 9 fma terms and the shift in fp32: 10 U (sum |terms| + |shift|); the bf16 rounding is the comparer's bracket"""
    return conv_taps(x, taps, st) + shift, 10.0 * U * (conv_taps(x.abs(), taps.abs(), st) + shift.abs())


def stream_gate(p, mean_in, rstd_in):
    """per channel: True where the 64-channel slice takes c from the forward output (dw3_bwd_stats_kernel: |gamma rstd| >= 1e-3 and |beta| <= 8 |gamma|
    in all 64 channels; the products are fp32)"""
    ok = ((p["gamma"].float() * rstd_in.float()).abs() >= 1e-3) & (p["beta"].abs() <= 8.0 * p["gamma"].abs())
    return ok.view(-1, 64).all(1).repeat_interleave(64)


def dw_forward_output(x, p, mean_in, rstd_in):
    """yf64 = (c - mean) gamma rstd + beta (float64, before its bf16 rounding) [Bn, Ho, Wo, C]"""
    return (conv_taps(x, p["taps"], p["stride"]) - mean_in) * p["gamma"] * rstd_in + p["beta"]


def dw_bwd_stats_ref(x, p, mean_in, rstd_in, streaming=False):
    """dwproj_bn_train_bwd_stats of one projection against float64; dy = p["dy"] as a map [Bn, Ho, Wo, C]; mean_in / rstd_in are the fp32 operands.
    streaming: the slices stream_gate allows recover c from the bf16 forward output. -> dict name -> (ref, tol, ulps): dgamma, dbeta, coef [3, C]"""
    st, N, gam = p["stride"], float(p["count"]), p["gamma"]
    dy = p["dy_map"]
    c, A = conv_taps(x, p["taps"], st), conv_taps(x.abs(), p["taps"].abs(), st)
    e = 9.0 * U * A                                               # recomputed convolution: 9 fma terms
    if streaming:
        # c' = fl(yf k0 + k1), k0 = 1 / (gamma rstd), k1 = mean - beta k0, yf = bf16(yf64): bf16 holds 8 significant bits, so rounding to nearest moves
        # yf by at most half a step, 2^-8 |yf64| at the bottom of a binade, i.e. c' by 2^-8 |yf64 k0|; k0 (a product and a division), k1 and the fma
        # add 4 U of the magnitudes |yf k0|, |beta k0| and |mean|
        k0 = (1.0 / (gam * rstd_in)).abs()
        yf = dw_forward_output(x, p, mean_in, rstd_in).abs()
        es = 2.0 ** -8 * yf * k0 + 4.0 * U * ((1.0 + 2.0 ** -8) * yf * k0 + p["beta"].abs() * k0 + mean_in.abs())
        e = torch.where(stream_gate(p, mean_in, rstd_in).to(e.device), es, e)
    S, D = dy.sum((0, 1, 2)), (dy * c).sum((0, 1, 2))
    tol_S = N * U * dy.abs().sum((0, 1, 2))                       # N exact bf16 values, any order
    # D: each term dy_i fl(c_i) is off by |dy_i| e_i; N fma terms of size |dy_i| (|c_i| + e_i) in any order
    tol_D = (dy.abs() * e).sum((0, 1, 2)) + (N + 1.0) * U * (dy.abs() * (c.abs() + e)).sum((0, 1, 2))
    r, mu = rstd_in, mean_in
    dgam = r * (D - mu * S)
    tol_dgam = r.abs() * (tol_D + mu.abs() * tol_S) + 3.0 * U * r.abs() * (D.abs() + (mu * S).abs())        # product, difference, product
    out = dict(dgamma=(p["dg0"] + dgam, tol_dgam + U * dgam.abs(), 2), dbeta=(p["db0"] + S, tol_S + U * S.abs(), 2))
    a = gam * r
    m1, m2 = S / N, dgam / N
    kc = -a * m2 * r
    tol_kc = (a * r).abs() * tol_dgam / N + 4.0 * U * kc.abs()    # a, the division and two products
    kb = -a * m1 - kc * mu
    tol_kb = a.abs() * tol_S / N + mu.abs() * tol_kc + 4.0 * U * ((a * m1).abs() + (kc * mu).abs())
    out["coef"] = (torch.stack([a, kb, kc]), torch.stack([torch.zeros_like(a), tol_kb, tol_kc]), 2)
    return out


def dw_dc_ref(x, p, coef):
    """dc = a dy + kb + kc c of one projection; coef [3, C] = the fp32 operand. The convolution's 9 U A_i scaled by |kc|, then three fma roundings
    at the size of their terms: 4 U (|a dy| + |kb| + |kc| (|c| + e))"""
    c, A = conv_taps(x, p["taps"], p["stride"]), conv_taps(x.abs(), p["taps"].abs(), p["stride"])
    e = 9.0 * U * A
    a, kb, kc = coef[0], coef[1], coef[2]
    dy = p["dy_map"]
    return a * dy + kb + kc * c, kc.abs() * e + 4.0 * U * ((a * dy).abs() + kb.abs() + kc.abs() * (c.abs() + e))


def dw_taps_ref(x, dc, st, count, dw0=None):
    """GS [10, C] of the bf16 dc that the kernel wrote (the tap sums see the stored gradient) and dw = dw0 + G^T: `count` fma terms per column in any
    order: (count + 1) U sum |dc x_t|; dw adds one rounding at the size of the sum"""
    GS, GA = tap_sums(x, dc, st), tap_sums(x.abs(), dc.abs(), st)
    tol = (count + 1.0) * U * GA
    if dw0 is None:
        return GS, tol
    return GS, tol, dw0 + GS[:9].t(), tol[:9].t() + U * (dw0.abs() + GA[:9].t())


def dw_dx_ref(dcs, tapss, strides, H, W):
    """input gradient: at most 9 + 4 + 4 = 17 fma terms per pixel: 17 U sum |terms|"""
    return dx_taps(dcs, tapss, strides, H, W), 17.0 * U * dx_taps([d.abs() for d in dcs], [t.abs() for t in tapss], strides, H, W)


# ------------------------------------------------------------------------------------------------ banded models of the kernels, with mutants
def _stage(x, iy0, rows, ix0, cols, mut=None):
    """tile [Bn, rows, cols, C] of map rows iy0.. and columns ix0.., zeros outside the map (dw3_stage). Mutants:
    ragged: rows past the map read the clamped row instead of zero | padcol: the right zero-padding column reads the next row's first pixel"""
    Bn, H, W, C = x.shape
    tile = torch.zeros((Bn, rows, cols, C), dtype=F64)
    for r in range(rows):
        iy = iy0 + r
        if mut == "ragged" and iy >= H:
            iy = H - 1
        if not 0 <= iy < H:
            continue
        for cc in range(cols):
            ix = ix0 + cc
            if 0 <= ix < W:
                tile[:, r, cc] = x[:, iy, ix]
            elif mut == "padcol" and ix == W and iy + 1 < H:
                tile[:, r, cc] = x[:, iy + 1, 0]
    return tile


def banded_conv(x, taps, st, band, mut=None):
    """conv_taps as dw3_apply_kernel / dw3_stats_kernel compute it, band by band. mut: None | ragged | padcol | halo (the halo row above every band
    but the first is the row two above) | slices (neighbouring 64-channel slices swapped; C = 64: neighbouring 8-channel chunks)"""
    Bn, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, st)
    out = torch.zeros((Bn, Ho, Wo, C), dtype=F64)
    for bi in range(-(-H // band)):
        tile = _stage(x, bi * band - 1, band + 2, -1, W + 2, mut)
        if mut == "halo" and bi > 0:
            tile[:, 0] = _stage(x, bi * band - 2, 1, -1, W + 2)[:, 0]
        oy0 = bi * band // st
        for oyl in range(max(0, min(band // st, Ho - oy0))):
            for t in range(9):
                out[:, oy0 + oyl] += tile[:, oyl * st + t // 3, t % 3:t % 3 + st * (Wo - 1) + 1:st] * taps[t]
    if mut == "slices":
        k = 64 if C >= 128 else 8
        out = out.view(Bn, Ho, Wo, C // (2 * k), 2, k).flip(4).reshape(Bn, Ho, Wo, C)
    return out


def banded_dx(dcs, tapss, strides, H, W, band, mut=None):
    """dx_taps as dw3_dx_kernel computes it: per band, stride-1 gradient tiles [band + 2][W + 2], stride-2 tiles [band / 2 + 1][W / 2 + 1], pixels per
    parity class. mut: None | halo | ragged | plus1 (the stride-2 tile lacks its last row) | parity (class (0, 1) uses the taps of class (0, 0))"""
    Bn, C = dcs[0].shape[0], dcs[0].shape[3]
    dx = torch.zeros((Bn, H, W, C), dtype=F64)
    for bi in range(-(-H // band)):
        nrow = min(band, H - bi * band)
        for dc, taps, st in zip(dcs, tapss, strides):
            if st == 1:
                tile = _stage(dc, bi * band - 1, band + 2, -1, W + 2, "ragged" if mut == "ragged" else None)
                if mut == "halo" and bi > 0:
                    tile[:, 0] = _stage(dc, bi * band - 2, 1, -1, W + 2)[:, 0]
                for iyl in range(nrow):
                    for t in range(9):
                        dx[:, bi * band + iyl] += tile[:, iyl + 2 - t // 3, 2 - t % 3:2 - t % 3 + W] * taps[t]
            else:
                tile = _stage(dc, bi * band // 2, band // 2 + 1, 0, W // 2 + 1, "ragged" if mut == "ragged" else None)
                if mut == "plus1":
                    tile[:, band // 2] = 0.0
                for iyl in range(nrow):
                    py = iyl & 1
                    for ix in range(W):
                        px = ix & 1
                        kxs = range(0 if px else 1, 3, 2)
                        if mut == "parity" and (py, px) == (0, 1):
                            kxs = range(1, 3, 2)
                        for ky in range(0 if py else 1, 3, 2):
                            for kx in kxs:
                                dx[:, bi * band + iyl, ix] += tile[:, (iyl + 1 - ky) >> 1, (ix + 1 - kx) >> 1] * taps[ky * 3 + kx]
    return dx


def banded_tokens(cls_rows, body, nbands, cls_band=0, unwritten=float("nan")):
    """the token matrix [Bn, tok0 + h w, C] that a banded kernel leaves in a buffer of `unwritten`: every band writes its rows of the map `body`
    [Bn, h, w, C] (already assembled), and the workgroups of band `cls_band` alone write the class-token rows `cls_rows` [Bn, tok0, C] (the kernels:
    band 0). With cls_band >= nbands nobody writes them."""
    Bn, tok0, C = cls_rows.shape
    out = torch.full((Bn, tok0 + body.shape[1] * body.shape[2], C), unwritten, dtype=F64)
    out[:, tok0:] = body.reshape(Bn, -1, C)
    for bi in range(nbands):
        if bi == cls_band:
            out[:, :tok0] = cls_rows
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm
@functools.lru_cache(maxsize=8)
def ln_gauss(rows, C, seed=0):
    """x = 2 N(0, 1) + 0.5 with a few elements scaled by 16, dy and add N(0, 1), all bf16; gamma = 1 + 0.1 N, beta = 0.1 N; Gaussian dg0 / db0;
    row_scale per image of ROWS_PER_B rows. CPU tensors (float64 for the small ones, bf16 for the maps: the large cases stay cheap)."""
    g = _gen(rows, C, seed, 53)
    x = torch.randn(rows, C, generator=g) * 2.0 + 0.5
    x.view(-1)[torch.randint(0, rows * C, (4,), generator=g)] *= 16.0
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(rows=rows, C=C, x=x.to(BF), dy=r(rows, C).to(BF), add=r(rows, C).to(BF), gamma=f32r(1.0 + 0.1 * r(C).double()), beta=f32r(0.1 * r(C).double()),
                dg0=f32r(r(C).double()), db0=f32r(r(C).double()))


def ln_exact_dy(rows, C, seed=0):
    """integer dy |v| <= 15 and integer db0: dbeta = db0 + column sums is an integer below 2^24 in any order (asserted)"""
    g = _gen(rows, C, seed, 54)
    assert rows * 15 + 1024 < CAP
    return torch.randint(-15, 16, (rows, C), generator=g).to(BF), _ints((C,), g, 1024)


def ln_fwd_ref(x, gamma, beta, eps=EPS):
    """x [R, C] float64 -> dict name -> (ref, tol): y, mean, rstd (assert_f32_bound ulps: mean 1, rstd 4)"""
    C = x.shape[1]
    mean = x.mean(1)
    tol_mean = U * x.abs().sum(1)                                 # C exact terms in any order: C U sum |x|, divided by C
    tm = (tol_mean + 2.0 * ulp32_t(mean))[:, None]                # + the rounding of 1 / C and of the product with it
    d = x - mean[:, None]
    dl = tm + U * d.abs()                                         # fl(x - fl(mean)) against x - mean
    var = (d * d).mean(1)
    # sum of C squares of perturbed differences: each within 2 |d| dl + dl^2 of d^2, C + 2 roundings at (|d| + dl)^2; + the final product
    tol_var = ((2.0 * d.abs() * dl + dl * dl).sum(1) + (C + 2.0) * U * ((d.abs() + dl) ** 2).sum(1)) / C + U * var
    rstd, tol_rstd = _rstd_bound(var, tol_var, eps)
    tr = (tol_rstd + 4.0 * ulp32_t(rstd))[:, None]
    y = d * rstd[:, None] * gamma + beta
    # y = ((x - mean) rstd) gamma + beta: the difference's dl times the largest rstd, |d| times rstd's bound, 4 roundings at the terms' size
    tol_y = gamma.abs() * (dl * (rstd[:, None] + tr) + d.abs() * tr) + 4.0 * U * ((d * rstd[:, None] * gamma).abs() + beta.abs())
    return dict(y=(y, tol_y), mean=(mean, tol_mean), rstd=(rstd, tol_rstd))


def ln_stats64(x, eps=EPS):
    """[R, 2] float64 (mean, rstd)"""
    mean = x.mean(1)
    return torch.stack([mean, (((x - mean[:, None]) ** 2).mean(1) + eps) ** -0.5], 1)


def ln_bwd_ref(x, dy, gamma, stats, add=None):
    """LayerNorm backward with the fp32 statistics `stats` [R, 2] as operands (float64 values of the fp32 numbers the kernel reads).
    -> dict name -> (ref, tol): dx [R, C]; dgamma, dbeta [C] WITHOUT their starting values"""
    R, C = x.shape
    mean, rstd = stats[:, 0:1], stats[:, 1:2]
    xh = (x - mean) * rstd
    gg = dy * gamma
    s1, s2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    # xh: a difference of exact operands and a product: 2 U |xh|; g: one product: U |g|
    # s1: C terms in any order and the product with 1 / C: (C + 2) U mean |g|
    d1 = (C + 2.0) * U * gg.abs().mean(1, keepdim=True)
    # s2: C fma terms whose factors carry 3 U relative, and the product with 1 / C: (C + 5) U mean |g xh|
    d2 = (C + 5.0) * U * (gg * xh).abs().mean(1, keepdim=True)
    dx = rstd * (gg - s1 - xh * s2)
    # rstd (g - s1 - xh s2): the operands' errors U |g|, d1, |xh| d2 + 2 U |xh s2|, then a product, two differences and a product at the terms' size
    tol = rstd * (d1 + xh.abs() * d2 + 8.0 * U * (gg.abs() + s1.abs() + (xh * s2).abs()))
    if add is not None:
        dx = dx + add
        tol = tol + U * dx.abs()
    # dgamma = sum over R rows of dy xh (fma terms, xh with 2 U relative), dbeta = sum of R exact values, any order
    return dict(dx=(dx, tol), dgamma=((dy * xh).sum(0), (R + 3.0) * U * (dy * xh).abs().sum(0)), dbeta=(dy.sum(0), R * U * dy.abs().sum(0)))


def scaled(ref_tol, f):
    """dx2 = f dx: the bound scales with |f| (the factor is an exact fp32 operand) and one more product is rounded"""
    ref, tol = ref_tol
    return ref * f, tol * f.abs() + U * (ref * f).abs()


# ------------------------------------------------------------------------------------------------ comparers
def _bf16_floor_t(v):
    """largest bf16 <= v (float64 tensor) -> float64; the torch twin of bounds_util.bf16_floor"""
    f = v.float()
    f = torch.where(f.double() > v, torch.nextafter(f, torch.full_like(f, float("-inf"))), f)
    b = f.view(torch.int32)
    t = (b & -65536).view(torch.float32)
    t = torch.where(t > f, ((b & -65536) + 65536).view(torch.float32), t)          # negative and not representable: one bf16 step away from zero
    return t.double()


def assert_bf16_bracket_t(out, ref, tol, what):
    """bounds_util.assert_bf16_bracket on the tensors' own device (the large maps stay on the GPU): every element of `out` (bf16) lies between the
    bf16 value just below ref - tol and the one just above ref + tol. -> largest |out - ref| as a fraction of the bracket's half-width"""
    assert out.dtype == BF and out.shape == ref.shape, (what, out.dtype, out.shape, ref.shape)
    o, tol = out.double(), torch.broadcast_to(torch.as_tensor(tol, dtype=F64, device=ref.device), ref.shape)
    lo, hi = _bf16_floor_t(ref - tol), -_bf16_floor_t(-(ref + tol))
    bad = ~((o >= lo) & (o <= hi))
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bf16 bracket, first at {i}: got {float(o[i])!r}, ref {float(ref[i])!r}, "
                             f"tol {float(tol[i]):.3e}")
    half = torch.maximum(hi - ref, ref - lo)
    return float(torch.where(half > 0, (o - ref).abs() / half.clamp_min(1e-300), torch.zeros_like(half)).max())


def assert_f32_t(out, ref, tol, ulps, what):
    """fp32 output within tol + ulps fp32 steps of ref, every element. -> largest |err| / (tol + ulps steps)"""
    assert out.dtype == torch.float32 and out.shape == ref.shape, (what, out.dtype, out.shape, ref.shape)
    o = out.double()
    lim = torch.broadcast_to(torch.as_tensor(tol, dtype=F64, device=ref.device), ref.shape) + ulps * ulp32_t(ref)
    err = (o - ref).abs()
    bad = ~(err <= lim)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} beyond the bound, first at {i}: got {float(o[i])!r}, ref {float(ref[i])!r}, "
                             f"bound {float(lim[i]):.3e}")
    return float((err / lim.clamp_min(1e-300)).max())


def assert_exact_t(out, ref, what):
    """gemm_ref.assert_exact on the tensors' own device: fp32 equals the exact value, bf16 its round-to-nearest-even (values: -0 == +0)"""
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    exp = ref.float() if out.dtype == torch.float32 else ref.float().to(BF)
    if out.dtype == torch.float32:
        assert torch.equal(exp.double(), ref), f"{what}: the reference itself is not exact in fp32"
    bad = ~(out == exp)                                            # a NaN equals nothing
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact value, first at {i}: got {float(out[i])!r}, "
                             f"exact {float(ref[i])!r}")


_E4M3_SORTED = np.unique(E4M3_VALUES[np.isfinite(E4M3_VALUES)])                    # ascending; -0 and +0 are one value


def assert_e4m3_one_step(codes, ref_scaled, what):
    """codes: uint8 e4m3 codes; every value is the round-to-nearest-even of ref_scaled over the finite e4m3 values or one of its two neighbours
    (the kernels round the fp32 value, which may sit on the other side of a tie). -> share of the elements that are not the nearest value"""
    got = E4M3_VALUES[codes.detach().cpu().numpy()]
    r = np.asarray(ref_scaled, np.float64)
    assert got.shape == r.shape, (what, got.shape, r.shape)
    exp = E4M3_VALUES[e4m3_encode(r)]
    i = np.searchsorted(_E4M3_SORTED, exp)
    lo, hi = _E4M3_SORTED[np.maximum(i - 1, 0)], _E4M3_SORTED[np.minimum(i + 1, len(_E4M3_SORTED) - 1)]
    bad = ~((got >= lo) & (got <= hi))
    assert not bad.any(), f"{what}: {int(bad.sum())} e4m3 elements more than one step from the nearest value, first: got {got[bad][0]!r} for {r[bad][0]!r}"
    return float((got != exp).mean())


# ------------------------------------------------------------------------------------------------ case tables
STRIDES = (1, 2, 2)
# (Bn, C, H, W, tok0, band, bands, rows in the last band, what it reaches); the band holds for every kernel of the family at these widths
DW_GEOMETRIES = [
    (128, 64, 13, 3, 0, 6, 3, 1, "tall band, ragged by 1, odd H and W"),
    (64, 128, 11, 4, 1, 4, 3, 3, "ragged by 3, two slices"),
    (128, 64, 9, 3, 1, 4, 3, 1, "band 4 ragged by 1"),
    (400, 64, 9, 3, 0, 10, 1, 9, "band taller than H"),
    (64, 384, 7, 6, 1, 8, 1, 7, "six slices, one band, class token"),
    (2, 64, 7, 5, 0, 2, 4, 1, "fallback band"),
    (1, 64, 1, 1, 1, 2, 1, 1, "1 x 1 map: every tap but the centre is padding"),
    (1, 64, 2, 1, 0, 2, 1, 2, "2 x 1 map"),
    (1, 64, 3, 96, 0, 2, 2, 1, "dx on the DW3_LDS_MAX budget at the smallest size"),
]
DW_REDUCE_G = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)          # G = Bn nbands on a (Bn, 64, 2, 2) map: one band
DW_STRIDE_LISTS = [((1,), (128, 64, 13, 3, 0)), ((2,), (64, 128, 11, 4, 1)), ((2, 1), (128, 64, 9, 3, 1)), ((1, 1, 1), (2, 64, 7, 5, 0)),
                   ((2, 2, 1), (128, 64, 13, 3, 1))]
DW_FORCED = (2, 64, 9, 96, 0)                                     # stage-1 width under CXR_DW3_BAND = 4 | 6
# band each kernel runs under the override: 4 fits all but the dc / tap-sum pass (its static LDS), 6 fits only dx, at exactly DW3_LDS_MAX
DW_FORCED_BANDS = {4: dict(apply=4, stats=4, bwd_stats=4, dc=2, dx=4), 6: dict(apply=2, stats=2, bwd_stats=2, dc=2, dx=6)}
DW_FORCED_FITS = {4: ("apply", "stats", "bwd_stats", "dx"), 6: ("dx",)}
LN_FWD_EDGE_ROWS = (1, 3, 127, 129)
LN_FWD_CAP_CASES = ((4096 * 8 + 5, 1024), (4096 * 16 + 3, 768))
ROWS_PER_B = 7                                                    # rows per image of the dropout / DropPath cases: divides no block size
