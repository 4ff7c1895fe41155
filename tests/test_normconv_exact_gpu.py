"""GPU: the fused depthwise projections (csrc/dwproj.hip) and LayerNorm (csrc/norm.hip) at their band and loop edges, against the float64
references of tests/normconv_ref.py (evaluated in torch float64 on the device).

exact family  integer activations, gradients, taps and coefficients whose products and partial sums are exact in fp32: a correct kernel returns
              the exact integer (fp32) or its round-to-nearest-even (bf16, e4m3) whatever its summation order -- no tolerance. A wrong halo row, a
              band offset of one, a swapped column, a neighbouring channel slice, a dropped or doubled partial row all change the result.
gauss family  N(0, 1) activations with per-channel offsets and hot pixels, pretrained-style BatchNorm parameters, against per-element bounds derived
              in normconv_ref.py from the reference's own magnitudes. No element is excluded.

Every operand is a view of a larger buffer of bf16 NaNs with non-contiguous batch and row strides (behind a class token, padded rows), every
output a view of a sentinel-guarded buffer; accumulated vectors start from non-zero values. Each case asserts, through the launch-plan mirrors of
normconv_ref.py, the band height, the rows in the last band and the LDS budget (projections) or the grid and the loop iterations (LayerNorm) that
it claims to reach. CXR_DW3_BAND is read once per process: the forced bands run in one fresh child process per value.

Every gauss comparison prints a MEASURED line with the worst ratio of error to bound, and test_zz_report_measured_figures prints the worst
figure per kernel and output. fp32 outputs: max |err| / (tol + the allowed fp32 steps), a ratio (bounds_util.assert_f32_bound returns the absolute
error instead). bf16 outputs: |err| as a fraction of the bracket's half-width, 1.000 wherever the reference lies half-way between two bf16
values. No floor is asserted on these figures: the exact family is what pins the arithmetic.
MEASURED on the MI355X, worst case over all geometries (the forced-band children print theirs, none above these). Wall time of the file: 16.2 s
for 104 tests, the slowest (a forced-band child process) 2.9 s. Every bf16 output (dw3_apply y, dc, dw3_dx, LayerNorm y, dx, dx2) reaches 1.000 of its
bracket, as it does wherever a reference lies half-way between two bf16 values.
  dw3_stats + reduce_finalize        mean 0.141, rstd 0.225, run_mean 0.281, run_var 0.169, folded taps 0.225, shift 0.225
  dw3_bwd_stats + reduce_coef        recompute: dgamma 0.087, dbeta 0.232, coef 0.250; streaming: dgamma 0.824, dbeta 0.232, coef 0.824
  dw3_dc_taps + reduce_taps          GS 0.026, dw 0.199
  layernorm_fwd_kernel               mean 0.012 (C = 64) .. 0.0004 (1024), rstd 0.041 (64) .. 0.002 (1024); past the grid cap: mean 0.0014, rstd 0.0034
  layernorm_bwd_kernel + reduce      dgamma 0.234 (C = 64), 0.240 (128), 0.354 (192), 0.318 (384), 0.352 (768); dbeta 0.225 .. 0.240
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import gemm_ref as G
import normconv_ref as R
from bounds_util import Guarded

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


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


def _call(name, *args):
    from cxrmate_amd._lib import LIB
    LIB.call(name, *args)


def _measured(kernel, what, fig):
    key = kernel
    WORST[key] = max(WORST.get(key, 0.0), fig)
    print(f"MEASURED {kernel} | {what}: {fig:.4f}")


def _f(t):
    return t.float().cuda().contiguous()


def _d(t):
    return t.double().cuda()


def _g3(Bn, L, C, dtype=BF, front=1, pad=8, init=None):
    """guarded [Bn, L, C] inside [Bn + 1, front + L + 2, C + pad]"""
    g = Guarded((Bn + 1, front + L + 2, C + pad), dtype, (slice(0, Bn), slice(front, front + L), slice(0, C)))
    if init is not None:
        g.view.copy_(init)
    return g


def _gvec(shape, init=None):
    """guarded contiguous fp32 array of `shape`, optionally starting from `init`"""
    g = Guarded.flat(int(np.prod(shape)), F32)
    v = g.view.view(shape)
    if init is not None:
        v.copy_(init)
    return g, v


def _layout(i, C):
    """operand layout of case i: (front rows, row stride); every combination of a view behind a class token and a padded row stride occurs"""
    return (1, C + 8) if i % 3 == 0 else ((0, C + 8) if i % 3 == 1 else (1, C))


def _assert_plans(geo, strides, band, nbands, last, forced=0, bands=None, big_dx=None):
    Bn, C, H, W, _ = geo
    plans = {k: R.dw3_plan(k, Bn, C, H, W, strides, forced) for k in R.DW3_KERNELS}
    for k, p in plans.items():
        want = bands[k] if bands else band
        assert p["band"] == want, (geo, k, p, want)
        if not bands:
            assert (p["nbands"], p["last"]) == (nbands, last), (geo, k, p)
    if big_dx is not None:
        assert plans["dx"]["big"] == big_dx and not any(plans[k]["big"] for k in R.DW3_KERNELS if k != "dx"), plans
    return plans


# ------------------------------------------------------------------------------------------------ depthwise-projection launches
def _dw_geo_args(ops, x, geo):
    Bn, C, H, W, tok0 = geo
    assert x.shape == (Bn, tok0 + H * W, C)
    return [ops._p(x), x.stride(0), x.stride(1), Bn, C, H, W, tok0]


def _dw_apply(ops, x, geo, projs, scales=None):
    """projs: [{stride, taps, shift}] -> guarded outputs written by one launch (bf16, or e4m3 codes with `scales`)"""
    Bn, C, H, W, tok0 = geo
    outs = []
    for p in projs:
        Ho, Wo = R.out_hw(H, W, p["stride"])
        outs.append(_g3(Bn, tok0 + Ho * Wo, C, torch.uint8 if scales else BF))
    full = [dict(p, y=o.view.view(ops.FP8) if scales else o.view) for p, o in zip(projs, outs)]       # (alive across the launch: the array holds raw pointers)
    arr = ops._dwproj_array(full)
    if scales:
        inv = (ctypes.c_float * len(projs))(*[1.0 / s for s in scales])
        _call("cxr_dwproj_apply_q8", *_dw_geo_args(ops, x, geo), ctypes.addressof(arr), len(projs), inv, ops._s())
    else:
        _call("cxr_dwproj_apply_bf16", *_dw_geo_args(ops, x, geo), ctypes.addressof(arr), len(projs), ops._s())
    for o in outs:
        o.check(f"dwproj apply {geo}")
    return [o.view for o in outs]


def _dw_with_ws(ops, name, x, geo, projs, *lead):
    Bn, C, H, W, _ = geo
    arr = ops._dwproj_array(projs)
    _call(name, *_dw_geo_args(ops, x, geo), *lead, ctypes.addressof(arr), len(projs), ops._p(ops._dwproj_ws(Bn, C, H, W, x.device)), ops._s())


def _dw_train_stats(ops, x, geo, cps, eps, momentum):
    """cps: per projection dict of float64 taps, w, gamma, beta (and run_mean, run_var when momentum > 0) -> per projection dict of guarded outputs"""
    C = geo[1]
    res, projs, guards = [], [], []
    for p in cps:
        o = {}
        for k, shape in (("mean", (C,)), ("rstd", (C,)), ("taps_out", (9, C)), ("shift_out", (C,))):
            g, o[k] = _gvec(shape)
            guards.append(g)
        d = dict(stride=p["stride"], taps=_f(p["taps"]), w=_f(p["w"]), gamma=_f(p["gamma"]), beta=_f(p["beta"]), **o)
        if momentum > 0:
            for k in ("run_mean", "run_var"):
                g, o[k] = _gvec((C,), _f(p[k]))
                guards.append(g)
                d[k] = o[k]
        projs.append(d)
        res.append(o)
    _dw_with_ws(ops, "cxr_dwproj_bn_train_stats_bf16", x, geo, projs, float(eps), float(momentum))
    for g in guards:
        g.check(f"dwproj train stats {geo}")
    return res


def _dw_bwd_stats(ops, x, geo, cps, dys, means, rstds, yfs=None):
    """-> per projection dict(dgamma, dbeta, coef) of guarded outputs; dgamma / dbeta start from dg0 / db0"""
    C = geo[1]
    res, projs, guards = [], [], []
    for i, p in enumerate(cps):
        o = {}
        for k, shape, init in (("dgamma", (C,), _f(p["dg0"])), ("dbeta", (C,), _f(p["db0"])), ("coef", (3, C), None)):
            g, o[k] = _gvec(shape, init)
            guards.append(g)
        d = dict(stride=p["stride"], taps=_f(p["taps"]), y=dys[i], gamma=_f(p["gamma"]), mean=_f(means[i]), rstd=_f(rstds[i]), **o)
        if yfs is not None:
            d.update(yf=yfs[i], beta=_f(p["beta"]))
        projs.append(d)
        res.append(o)
    _dw_with_ws(ops, "cxr_dwproj_bn_train_bwd_stats_bf16", x, geo, projs)
    for g in guards:
        g.check(f"dwproj bwd stats {geo}")
    return res


def _dw_dc_taps(ops, x, geo, cps, dy_guards, coefs=None, want=None):
    """dy_guards: Guarded in / out gradients; want[q] = (GS?, dw?) -> per projection dict(GS, dw); dw starts from dw0"""
    C = geo[1]
    res, projs, guards = [], [], []
    for i, p in enumerate(cps):
        o = {}
        gs, dw = want[i] if want else (True, True)
        if gs:
            g, o["GS"] = _gvec((10, C))
            guards.append(g)
        if dw:
            g, o["dw"] = _gvec((C, 9), _f(p["dw0"]))
            guards.append(g)
        projs.append(dict(stride=p["stride"], taps=_f(p["taps"]), y=dy_guards[i].view, coef=None if coefs is None else _f(coefs[i]), **o))
        res.append(o)
    _dw_with_ws(ops, "cxr_dwproj_dc_taps_bf16", x, geo, projs)
    for g in guards + list(dy_guards):
        g.check(f"dwproj dc / taps {geo}")
    return res


def _dw_dx(ops, geo, cps, dcs):
    Bn, C, H, W, tok0 = geo
    out = _g3(Bn, tok0 + H * W, C)
    projs = [dict(stride=p["stride"], taps=_f(p["taps"]), y=d) for p, d in zip(cps, dcs)]     # (alive across the launch: the array holds raw pointers)
    arr = ops._dwproj_array(projs)
    _call("cxr_dwproj_dx_bf16", ops._p(out.view), out.view.stride(0), out.view.stride(1), Bn, C, H, W, tok0, ctypes.addressof(arr), len(cps), ops._s())
    out.check(f"dwproj dx {geo}")
    return out.view


# ------------------------------------------------------------------------------------------------ the two families on one geometry
def _run_dw_exact(ops, geo, strides, layout=0):
    Bn, C, H, W, tok0 = geo
    c = R.dw_exact(*geo, strides)
    front, ld = _layout(layout, C)
    what = f"exact {geo} {strides}"
    x = R.embed3(c["x"], "cuda", front, ld)
    ys = _dw_apply(ops, x, geo, [dict(stride=p["stride"], taps=_f(p["taps"]), shift=_f(p["shift"])) for p in c["p"]])
    for q, (y, p) in enumerate(zip(ys, c["p"])):
        R.assert_exact_t(y, _d(p["y"]), f"{what} apply {q}")
    x8 = R.embed3(c["x8"], "cuda", front, ld)
    scales = [p["scale8"] for p in c["p"]]
    y8 = _dw_apply(ops, x8, geo, [dict(stride=p["stride"], taps=_f(p["taps8"]), shift=_f(p["shift8"])) for p in c["p"]], scales)
    for q, (y, p) in enumerate(zip(y8, c["p"])):
        G.assert_exact_e4m3(y, p["y8"].numpy(), p["scale8"], f"{what} apply_q8 {q}")
    # tap sums and S of the unchanged gradient: GS and dw of projection 0, GS alone of 1, dw alone of 2
    dyg = [_g3(Bn, p["dy"].shape[1], C, init=p["dy"].cuda()) for p in c["p"]]
    res = _dw_dc_taps(ops, x, geo, c["p"], dyg, want=[(True, True), (True, False), (False, True)][:len(strides)])
    for q, (o, p, dg_) in enumerate(zip(res, c["p"], dyg)):
        if "GS" in o:
            R.assert_exact_t(o["GS"], _d(p["GS"]), f"{what} tap sums {q}")
        if "dw" in o:
            R.assert_exact_t(o["dw"], _d(p["dw"]), f"{what} dw {q}")
        assert torch.equal(dg_.view.double(), _d(p["dy"])), f"{what}: the gradient of projection {q} was rewritten without coefficients"
    dys = [R.embed3(p["dy"], "cuda", front, ld) for p in c["p"]]
    R.assert_exact_t(_dw_dx(ops, geo, c["p"], dys), _d(c["dx"]), f"{what} dx")
    # statistics: the forward mean = fl32(S0 / count); dbeta = db0 + S; dgamma = dg0 + rstd (D - mean S)
    xs = R.embed3(c["xs"], "cuda", front, ld)
    one, zero = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)
    sps = [dict(p, taps=p["taps_s"], w=p["taps_s"].t(), gamma=one, beta=zero) for p in c["p"]]
    st = _dw_train_stats(ops, xs, geo, sps, R.EPS, 0.0)
    for q, (o, p) in enumerate(zip(st, c["p"])):
        R.assert_exact_t(o["mean"], _d(p["mean"]), f"{what} batch mean {q}")
    dyss = [R.embed3(p["dys"], "cuda", front, ld) for p in c["p"]]
    bw = _dw_bwd_stats(ops, xs, geo, sps, dyss, [p["mean_in"] for p in c["p"]], [p["rstd_in"] for p in c["p"]])
    for q, (o, p) in enumerate(zip(bw, c["p"])):
        R.assert_exact_t(o["dbeta"], _d(p["dbeta"]), f"{what} dbeta {q}")
        R.assert_exact_t(o["dgamma"], _d(p["dgamma"]), f"{what} dgamma {q}")


def _cmp32(out, rt, what, kernel):
    ref, tol, ulps = rt
    _measured(kernel, what, R.assert_f32_t(out, ref, tol, ulps, what))


def _run_dw_gauss(ops, geo, strides, layout=0):
    Bn, C, H, W, tok0 = geo
    c = R.dw_gauss(*geo, strides)
    front, ld = _layout(layout, C)
    what = f"gauss {geo}"
    x = R.embed3(c["x"], "cuda", front, ld)
    xi = R.img(_d(c["x"]), tok0, H, W)
    cps = []
    for p in c["p"]:
        dp = {k: (_d(v) if torch.is_tensor(v) else v) for k, v in p.items()}
        dp["dy_map"] = R.img(dp["dy"], tok0, p["Ho"], p["Wo"])
        cps.append(dp)
    # ---- train-mode forward statistics, then apply with the folded taps the kernel produced
    st = _dw_train_stats(ops, x, geo, c["p"], R.EPS, R.MOMENTUM)
    refs = [R.dw_train_stats_ref(xi, dp) for dp in cps]
    for q, (o, r) in enumerate(zip(st, refs)):
        for k, ko in (("mean", "mean"), ("rstd", "rstd"), ("run_mean", "run_mean"), ("run_var", "run_var"), ("taps", "taps_out"), ("shift", "shift_out")):
            _cmp32(o[ko], r[k], f"{what} {k} {q}", f"dw3_stats + reduce_finalize {k}")
    ys = _dw_apply(ops, x, geo, [dict(stride=p["stride"], taps=o["taps_out"].clone(), shift=o["shift_out"].clone()) for p, o in zip(c["p"], st)])
    for q, (y, o, dp) in enumerate(zip(ys, st, cps)):
        ref, tol = R.dw_apply_ref(xi, o["taps_out"].double(), o["shift_out"].double(), dp["stride"])
        _measured("dw3_apply", f"{what} y {q}", R.assert_bf16_bracket_t(y[:, tok0:], ref.reshape(Bn, -1, C), tol.reshape(Bn, -1, C), f"{what} apply {q}"))
        assert torch.equal(y[:, :tok0].double(), _d(c["x"])[:, :tok0])
    # ---- backward statistics; their mean / rstd operands are the float64 statistics rounded to fp32 (independent of the forward kernel)
    means, rstds = [R.f32r(r["mean"][0]) for r in refs], [R.f32r(r["rstd"][0]) for r in refs]
    dys = [R.embed3(p["dy"], "cuda", front, ld) for p in c["p"]]
    bw = _dw_bwd_stats(ops, x, geo, c["p"], dys, means, rstds)
    brefs = [R.dw_bwd_stats_ref(xi, dp, m, r) for dp, m, r in zip(cps, means, rstds)]
    for q, (o, r) in enumerate(zip(bw, brefs)):
        for k in ("dgamma", "dbeta", "coef"):
            _cmp32(o[k], r[k], f"{what} {k} {q}", f"dw3_bwd_stats (recompute) + reduce_coef {k}")
    yfs, gates = [], []
    for dp, p, m, r in zip(cps, c["p"], means, rstds):
        yf = R.with_cls(torch.zeros((Bn, tok0, C), dtype=F64, device="cuda"), R.dw_forward_output(xi, dp, m, r))
        yfs.append(R.embed3(R.bfr(yf).cpu(), "cuda", 1 - front, C + 8))
        gates.append(R.stream_gate(dp, m, r).view(-1, 64)[:, 0].tolist())
    assert not any(gates[1]) or C > 64, gates
    assert not gates[1][0] and not gates[-1][-1] and all(gates[0]), f"{what}: the gates of the streaming path are not where the case puts them: {gates}"
    bws = _dw_bwd_stats(ops, x, geo, c["p"], dys, means, rstds, yfs)
    srefs = [R.dw_bwd_stats_ref(xi, dp, m, r, streaming=True) for dp, m, r in zip(cps, means, rstds)]
    for q, (o, r) in enumerate(zip(bws, srefs)):
        for k in ("dgamma", "dbeta", "coef"):
            _cmp32(o[k], r[k], f"{what} streaming {k} {q}", f"dw3_bwd_stats (streaming) + reduce_coef {k}")
    # ---- dc in place (coefficients: the float64 ones rounded to fp32), tap sums of the stored dc, dw
    coefs = [R.f32r(r["coef"][0]) for r in brefs]
    dyg = [_g3(Bn, p["dy"].shape[1], C, init=p["dy"].cuda()) for p in c["p"]]
    res = _dw_dc_taps(ops, x, geo, c["p"], dyg, coefs)
    dcs = []
    for q, (o, dp, cf, dg_) in enumerate(zip(res, cps, coefs, dyg)):
        ref, tol = R.dw_dc_ref(xi, dp, cf)
        dc = dg_.view
        _measured("dw3_dc_taps dc", f"{what} dc {q}", R.assert_bf16_bracket_t(dc[:, tok0:], ref.reshape(Bn, -1, C), tol.reshape(Bn, -1, C), f"{what} dc {q}"))
        assert torch.equal(dc[:, :tok0].double(), dp["dy"][:, :tok0]), f"{what}: class-token rows of projection {q} were rewritten"
        dcm = R.img(dc.double(), tok0, dp["Ho"], dp["Wo"])
        GS, tol, dw, tol_dw = R.dw_taps_ref(xi, dcm, dp["stride"], dp["count"], dp["dw0"])
        _cmp32(o["GS"], (GS, tol, 2), f"{what} GS {q}", "dw3_dc_taps + reduce_taps GS")
        _cmp32(o["dw"], (dw, tol_dw, 2), f"{what} dw {q}", "dw3_dc_taps + reduce_taps dw")
        dcs.append(dcm)
    # ---- dx of the rewritten dc
    dx = _dw_dx(ops, geo, c["p"], [g.view for g in dyg])
    ref, tol = R.dw_dx_ref(dcs, [dp["taps"] for dp in cps], strides, H, W)
    _measured("dw3_dx", f"{what} dx", R.assert_bf16_bracket_t(dx[:, tok0:], ref.reshape(Bn, -1, C), tol.reshape(Bn, -1, C), f"{what} dx"))
    if tok0:
        cls = sum(g.view[:, :tok0].double() for g in dyg)
        R.assert_bf16_bracket_t(dx[:, :tok0], cls, 3.0 * G.U * sum(g.view[:, :tok0].double().abs() for g in dyg), f"{what} dx class rows")


_GEO_IDS = ["x".join(str(v) for v in g[:5]) for g in R.DW_GEOMETRIES]


@pytest.mark.parametrize("i", range(len(R.DW_GEOMETRIES)), ids=_GEO_IDS)
def test_dwproj_band_edges_exact(ops, i):
    *geo, band, nbands, last, _ = R.DW_GEOMETRIES[i]
    _assert_plans(geo, R.STRIDES, band, nbands, last, big_dx=geo[3] == 96)
    _run_dw_exact(ops, tuple(geo), R.STRIDES, i)


@pytest.mark.parametrize("i", range(len(R.DW_GEOMETRIES)), ids=_GEO_IDS)
def test_dwproj_band_edges_gauss(ops, i):
    *geo, band, nbands, last, _ = R.DW_GEOMETRIES[i]
    _assert_plans(geo, R.STRIDES, band, nbands, last, big_dx=geo[3] == 96)
    _run_dw_gauss(ops, tuple(geo), R.STRIDES, i + 1)


@pytest.mark.parametrize("rows", R.DW_REDUCE_G)
def test_dwproj_row_reduction_thresholds_exact(ops, rows):
    """G = Bn nbands partial rows around the unrolled loops of dw3_rows_sum2 (r + 48 < G) and dw3_reduce_taps_kernel (r + 112 < G)"""
    geo = (rows, 64, 2, 2, rows % 2)
    plans = _assert_plans(geo, R.STRIDES, 2, 1, 2)
    assert all(p["G"] == rows for p in plans.values())
    _run_dw_exact(ops, geo, R.STRIDES, rows)


@pytest.mark.parametrize("strides,geo", R.DW_STRIDE_LISTS, ids=["".join(str(s) for s in st) for st, _ in R.DW_STRIDE_LISTS])
def test_dwproj_projection_lists_exact(ops, strides, geo):
    """1, 2 and 3 projections; a stride-2 projection first (dw3_dx_kernel without register taps), a stride-1 projection behind the first (taps from LDS)"""
    plans = {k: R.dw3_plan(k, *geo[:4], strides) for k in R.DW3_KERNELS}
    assert all(p["band"] > 2 or geo[0] == 2 for p in plans.values()) and all(p["last"] < p["band"] for p in plans.values()), plans
    _run_dw_exact(ops, geo, strides, len(strides))


# ---- CXR_DW3_BAND is read once per process: one fresh child process per value
def child_main(forced):
    """runs in the child process: both families at the stage-1 width under one forced band; stops at the first failure"""
    ops = _load_ops()
    geo = R.DW_FORCED
    plans = _assert_plans(geo, R.STRIDES, None, None, None, forced=forced, bands=R.DW_FORCED_BANDS[forced], big_dx=True)
    for k in R.DW_FORCED_FITS[forced]:
        budget = R.DW3_LDS_MAX if plans[k]["big"] else R.DW3_LDS_CAP
        assert plans[k]["band"] == forced and plans[k]["lds"] <= budget, (k, plans[k])
    if forced == 6:
        assert plans["dx"]["lds"] == R.DW3_LDS_MAX and plans["dx"]["last"] == 3
    else:
        assert plans["apply"]["last"] == 1
    _run_dw_exact(ops, geo, R.STRIDES, 0)
    _run_dw_gauss(ops, geo, R.STRIDES, 1)
    torch.cuda.synchronize()
    print(f"CHILD band {forced} DONE")


@pytest.mark.parametrize("forced", [4, 6])
def test_dwproj_stage1_width_forced_band(forced):
    """(2, 64, 9, 96): band 4 (apply, statistics, dx; ragged last band of 1) and band 6 (dx at the full DW3_LDS_MAX allocation, last band of 3)"""
    code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_normconv_exact_gpu as T; T.child_main({forced})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CXR_DW3_BAND=str(forced)), capture_output=True, text=True, cwd=ROOT, timeout=240)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    assert f"CHILD band {forced} DONE" in r.stdout


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_fwd(ops, x, gamma, beta, rows, C, ld_out=None, q8_inv=None):
    """-> (y guarded view, stats guarded view [rows, 2], e4m3 codes | None)"""
    gy = Guarded.rows(rows, C, BF, ld=ld_out or C + 8)
    gs, stats = _gvec((rows, 2))
    if q8_inv is None:
        _call("cxr_layernorm_fwd_bf16", ops._p(x), x.stride(0), ops._p(gamma), ops._p(beta), ops._p(gy.view), gy.view.stride(0), ops._p(stats), rows, C, R.EPS, ops._s())
        g8 = None
    else:
        g8 = Guarded.rows(rows, C, torch.uint8, ld=C + 16)
        _call("cxr_layernorm_q8_bf16", ops._p(x), x.stride(0), ops._p(gamma), ops._p(beta), ops._p(gy.view), gy.view.stride(0), ops._p(g8.view), g8.view.stride(0),
              float(q8_inv), ops._p(stats), rows, C, R.EPS, ops._s())
        g8.check("layernorm_q8 codes")
    gy.check("layernorm y")
    gs.check("layernorm stats")
    return gy.view, stats, None if g8 is None else g8.view


def _ln_bwd(ops, x, dy, gamma, stats, rows, C, dg=None, db=None, add=None, main=True, drop=None, row_scale=None, split=False):
    """one cxr_layernorm_bwd_bf16 launch into guarded outputs (split: the parameter gradients through cxr_layernorm_bwd_reduce) -> (dx, dx2)"""
    from cxrmate_amd._lib import LIB
    gdx = Guarded.rows(rows, C, BF, ld=C + 8) if main else None
    second = drop is not None or row_scale is not None
    gdx2 = Guarded.rows(rows, C, BF, ld=C + 16) if second else None
    nb = LIB.load().cxr_layernorm_bwd_grid(rows, C)
    gws, ws = _gvec((nb, 2, C))
    fused = dg is not None and not split
    _call("cxr_layernorm_bwd_bf16", ops._p(x), x.stride(0), ops._p(dy), dy.stride(0), ops._p(gamma), ops._p(stats), ops._p(add), add.stride(0) if add is not None else 0,
          ops._p(gdx.view) if main else None, gdx.view.stride(0) if main else C, ops._p(dg) if fused else None, ops._p(db) if fused else None, ops._p(ws), rows, C,
          ops._p(gdx2.view) if second else None, gdx2.view.stride(0) if second else 0, float(drop[0]) if drop else 0.0, ops._p(drop[1]) if drop else None,
          int(drop[2]) if drop else 0, int(drop[3]) if drop else (int(row_scale[1]) if row_scale else 1), int(drop[4]) if drop else 0,
          ops._p(row_scale[0]) if row_scale else None, ops._s())
    if dg is not None and split:
        _call("cxr_layernorm_bwd_reduce", ops._p(ws), rows, C, ops._p(dg), ops._p(db), ops._s())
    for g in (gdx, gdx2, gws):
        if g is not None:
            g.check(f"layernorm bwd {rows}x{C}")
    return (gdx.view if main else None), (gdx2.view if second else None)


def _ln_check_fwd(ops, rows, C, x, gamma, beta, xd, kernel, q8=False):
    ref = R.ln_fwd_ref(xd, _d(gamma), _d(beta))
    what = f"ln fwd {rows}x{C}"
    inv = None
    if q8:
        scale = float(ref["y"][0].abs().max()) / 400.0
        inv = float(np.float32(1.0 / scale))
    y, stats, y8 = _ln_fwd(ops, x, _f(gamma), _f(beta), rows, C, q8_inv=inv)
    _measured(f"{kernel} y", what, R.assert_bf16_bracket_t(y, *ref["y"], f"{what} y"))
    _measured(f"{kernel} mean", what, R.assert_f32_t(stats[:, 0], *ref["mean"], 2, f"{what} mean"))
    _measured(f"{kernel} rstd", what, R.assert_f32_t(stats[:, 1], *ref["rstd"], 4, f"{what} rstd"))
    if q8:
        R.assert_e4m3_one_step(y8, (ref["y"][0] * inv).cpu().numpy(), f"{what} e4m3")
    return stats


def _ln_bwd_cases(C):
    """(rows, grid, iterations of the least loaded workgroup, of the most loaded one) from (k, r) and the grid cap, without the mirror"""
    rpb = R.LN_BWD_RPB[C]
    out = []
    for rows in R.ln_bwd_rows(C):
        blocks = -(-rows // rpb)
        k, rem = divmod(blocks, R.LN_BWD_CAP)
        out.append((rows, min(blocks, 512), k if k else 1, k + (1 if rem else 0) if k else 1))
    return out


@pytest.mark.parametrize("C", [64, 128, 192, 384, 768])
def test_layernorm_case_table_reaches_every_edge(ops, C):
    from cxrmate_amd._lib import LIB
    cases = _ln_bwd_cases(C)
    assert {c[1] for c in cases} >= set(R.LN_REDUCE_GRIDS)
    assert {c[3] for c in cases} >= {1, 2, 3, 4, 5} and any(c[2] < c[3] for c in cases) and any(c[2] == c[3] > 1 for c in cases)
    assert any(R.ln_plan(c[0], C)["dead"] for c in cases) and any(c[0] == 1 for c in cases)
    for rows, grid, lo, hi in cases:
        p = R.ln_plan(rows, C)
        assert (p["grid"], p["it_min"], p["it_max"]) == (grid, lo, hi) and grid == LIB.load().cxr_layernorm_bwd_grid(rows, C), (rows, C, p)


_LN_BWD = [(C, i) for C in (64, 128, 192, 384, 768) for i in range(len(R.ln_bwd_rows(64)))]


@pytest.mark.parametrize("C,i", _LN_BWD, ids=[f"{C}-{R.ln_bwd_rows(C)[i]}" for C, i in _LN_BWD])
def test_layernorm_backward_loop_edges(ops, C, i):
    """rows = 512 rpb k + r: 1 .. 5 loop iterations per workgroup, both exits of the pipelined loop, a partly dead last row group; reduce grids 1,
    63, 64, 65 and 512. Variant by case: add with its own row stride | split reduce | DropPath dx2 | dropout dx2 without dx. The statistics operand is
    the forward kernel's output (checked here against its own bound); every third case uses the float64 statistics rounded to fp32 instead."""
    rows, grid, lo, hi = _ln_bwd_cases(C)[i]
    p = R.ln_plan(rows, C)
    assert (p["grid"], p["it_min"], p["it_max"]) == (grid, lo, hi), p
    c = R.ln_gauss(rows, C)
    kernel = f"layernorm_bwd_kernel<{C}>"
    x, dy = G.embed(c["x"], "cuda", ld=C + 16), G.embed(c["dy"], "cuda", ld=C + 8)
    xd, dyd, gam = c["x"].cuda().double(), c["dy"].cuda().double(), _d(c["gamma"])
    stats = _ln_check_fwd(ops, rows, C, x, c["gamma"], c["beta"], xd, f"layernorm_fwd_kernel<{C}>")
    if i % 3 == 2:
        stats = R.ln_stats64(xd).float().contiguous()
    gdg, dg = _gvec((C,), _f(c["dg0"]))
    gdb, db = _gvec((C,), _f(c["db0"]))
    variant = i % 4
    what = f"ln bwd {rows}x{C} variant {variant}"
    add = G.embed(c["add"], "cuda", ld=C + 24) if variant == 0 else None
    ref = R.ln_bwd_ref(xd, dyd, gam, stats.double(), c["add"].cuda().double() if variant == 0 else None)
    kw, f = {}, None
    if variant == 2:
        f = (torch.rand(-(-rows // R.ROWS_PER_B), generator=torch.Generator().manual_seed(rows)) * 2.0).float().cuda()
        f[0] = 0.0
        kw["row_scale"] = (f, R.ROWS_PER_B)
        f = f.double().repeat_interleave(R.ROWS_PER_B)[:rows, None]
    if variant == 3:
        seed = torch.full((1,), 4321, dtype=torch.int32, device="cuda")
        kw.update(drop=(0.25, seed, 17, R.ROWS_PER_B, 3), main=False)
        f = ops.dropout_mask(rows, C, 0.25, seed, 17, R.ROWS_PER_B, 3, factor=True).double()
        assert 0.6 < float((f != 0).double().mean()) < 0.9 or rows * C < 4096
    dx, dx2 = _ln_bwd(ops, x, dy, _f(c["gamma"]), stats, rows, C, dg, db, add=add, split=variant == 1, **kw)
    gdg.check(what), gdb.check(what)
    if dx is not None:
        _measured(f"{kernel} dx", what, R.assert_bf16_bracket_t(dx, *ref["dx"], f"{what} dx"))
    else:
        assert variant == 3
    if dx2 is not None:
        _measured(f"{kernel} dx2", what, R.assert_bf16_bracket_t(dx2, *R.scaled(ref["dx"], f), f"{what} dx2"))
    for k, out, start in (("dgamma", dg, c["dg0"]), ("dbeta", db, c["db0"])):
        r, tol = ref[k]
        _measured(f"{kernel} + reduce {k}", what, R.assert_f32_t(out, _d(start) + r, tol + G.U * r.abs(), 2, f"{what} {k}"))
    # exact family: integer dy, dbeta = db0 + column sums, whatever the order of the workgroups' partial rows and of the reduce kernel's atomics
    dyi, db0 = R.ln_exact_dy(rows, C)
    _, dbi = _gvec((C,), _f(db0))
    _, dgi = _gvec((C,))
    dgi.zero_()
    # (the call the gauss pass above did not take: every reduce grid, 63 included, runs the fused and the split call)
    _ln_bwd(ops, x, G.embed(dyi, "cuda", ld=C + 8), _f(c["gamma"]), stats, rows, C, dgi, dbi, split=variant != 1)
    R.assert_exact_t(dbi, _d(db0) + dyi.cuda().double().sum(0), f"ln bwd {rows}x{C} exact dbeta")


@pytest.mark.parametrize("C", [64, 128, 192, 384, 768, 1024])
def test_layernorm_forward_small_edges(ops, C):
    """rows below one wave's worth, one row less and one more than a workgroup's rows per iteration; the e4m3 output per element"""
    rpb = R.LN_FWD_RPB[C]
    for rows in R.LN_FWD_EDGE_ROWS + (rpb - 1, rpb + 1):
        c = R.ln_gauss(rows, C, 1)
        x = G.embed(c["x"], "cuda", ld=C + 16)
        p = R.ln_plan(rows, C, fwd=True)
        assert p["grid"] == -(-rows // rpb) and p["it_max"] == 1
        _ln_check_fwd(ops, rows, C, x, c["gamma"], c["beta"], c["x"].cuda().double(), f"layernorm_fwd_kernel<{C}>")
        if C != 1024:
            _ln_check_fwd(ops, rows, C, x, c["gamma"], c["beta"], c["x"].cuda().double(), f"layernorm_fwd_kernel<{C}, q8>", q8=True)


@pytest.mark.parametrize("rows,C", R.LN_FWD_CAP_CASES)
def test_layernorm_forward_past_the_grid_cap(ops, rows, C):
    p = R.ln_plan(rows, C, fwd=True)
    assert p["grid"] == R.LN_FWD_CAP and (p["it_min"], p["it_max"]) == (1, 2) and p["dead"] > 0, p
    c = R.ln_gauss(rows, C, 2)
    _ln_check_fwd(ops, rows, C, G.embed(c["x"], "cuda", ld=C + 16), c["gamma"], c["beta"], c["x"].cuda().double(), f"layernorm_fwd_kernel<{C}> past the cap")


def test_zz_report_measured_figures(ops):
    """prints the worst figure per kernel and output of this run (the MEASURED table of the module docstring)"""
    for k in sorted(WORST):
        print(f"MEASURED WORST {k}: {WORST[k]:.4f}")
