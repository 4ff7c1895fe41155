"""CPU: the generators, float64 references, bounds, launch-plan mirrors and comparers of tests/normconv_ref.py themselves.

The reference rounded to the output type passes every comparer; outputs that model a subtly wrong kernel (built from the same case by the banded
models of normconv_ref.py) are rejected, in the exact and in the gauss family. Where a gauss bound cannot reject a mutant that the exact family
rejects, the test says so:
  - a class-token row written by band 1 instead of band 0 differs only where there is a single band (the row then stays unwritten);
  - one partial row dropped from / added twice to a row reduction, and dead rows added to LayerNorm's dbeta, are rejected by the gauss bounds at
    the small counts used here; at 10^4 and more terms the any-order bound (count U sum |terms|) exceeds one partial row, and only the exact
    family catches them (checked below at the count where the bound gives way).
  - LayerNorm's exact family holds dbeta only: the stale-stage, skipped-stage and variance mutants apply to the gauss family alone.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
import gemm_ref as G
import normconv_ref as R
from bounds_util import _SENT, assert_bf16_bracket, bf16_floor

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GEO = (2, 128, 13, 5, 1)                       # CPU mutants: band 6 -> bands of 6, 6 and a ragged 1
BAND = 6


def _rejects(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


# ------------------------------------------------------------------------------------------------ mirrors and tables
def test_picker_mirror_reaches_the_geometries_of_the_table():
    for *geo, band, nbands, last, _ in R.DW_GEOMETRIES:
        for k in R.DW3_KERNELS:
            p = R.dw3_plan(k, *geo[:4], R.STRIDES)
            assert (p["band"], p["nbands"], p["last"]) == (band, nbands, last), (geo, k, p)
            assert p["big"] == (k == "dx" and geo[3] == 96)
    assert {g[4] for g in R.DW_GEOMETRIES} == {0, 1}
    # the stage-1 production geometry at batch 64: what the forced bands stand in for
    assert {k: R.dw3_plan(k, 64, 64, 96, 96, R.STRIDES)["band"] for k in R.DW3_KERNELS} == dict(apply=4, stats=4, bwd_stats=4, dc=2, dx=6)
    assert R.dw3_plan("dx", 64, 64, 96, 96, R.STRIDES)["lds"] == R.DW3_LDS_MAX == 150528 + 9216
    for forced, bands in R.DW_FORCED_BANDS.items():
        assert {k: R.dw3_plan(k, *R.DW_FORCED[:4], R.STRIDES, forced)["band"] for k in R.DW3_KERNELS} == bands
    assert all(R.dw3_plan(k, 8, 64, 96, 96, R.STRIDES)["band"] == 2 for k in R.DW3_KERNELS)          # the only 96-wide case of test_kernels_gpu.py
    for g_ in R.DW_REDUCE_G:
        assert all(R.dw3_plan(k, g_, 64, 2, 2, R.STRIDES)["G"] == g_ for k in R.DW3_KERNELS)
    assert {1, 15, 16, 17, 63, 64, 65, 127, 128, 129} == set(R.DW_REDUCE_G)                          # r + 48 < G and r + 112 < G, r < 16


@pytest.mark.parametrize("C", sorted(R.LN_BWD_RPB))
def test_layernorm_table_reaches_every_loop_edge(C):
    plans = [R.ln_plan(r, C) for r in R.ln_bwd_rows(C)]
    assert {p["it_max"] for p in plans} >= {1, 2, 3, 4, 5} and {p["grid"] for p in plans} >= set(R.LN_REDUCE_GRIDS)
    assert any(p["it_min"] < p["it_max"] for p in plans) and any(p["dead"] for p in plans) and 1 in R.ln_bwd_rows(C)
    assert max(R.ln_bwd_rows(64)) == 512 * 64 * 4 + 1
    for rows, c in R.LN_FWD_CAP_CASES:
        assert R.ln_plan(rows, c, fwd=True)["grid"] == 4096 and R.ln_plan(rows, c, fwd=True)["it_max"] == 2


# ------------------------------------------------------------------------------------------------ references against torch's own operators
def _rand_geo(seed=0, strides=R.STRIDES):
    g = torch.Generator().manual_seed(seed)
    Bn, C, H, W = 2, 64, 7, 5
    x = torch.randn(Bn, H, W, C, generator=g).double()
    tapss = [torch.randn(9, C, generator=g).double() for _ in strides]
    dcs = [torch.randn(Bn, *R.out_hw(H, W, s), C, generator=g).double() for s in strides]
    return x, tapss, dcs, H, W, C


def test_references_agree_with_conv2d_and_autograd():
    x, tapss, dcs, H, W, C = _rand_geo()
    xs = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    ws = [t.t().reshape(C, 1, 3, 3).clone().requires_grad_(True) for t in tapss]
    loss = 0
    for t, w, dc, st in zip(tapss, ws, dcs, R.STRIDES):
        y = F.conv2d(xs, w, None, stride=st, padding=1, groups=C)
        assert torch.allclose(R.conv_taps(x, t, st), y.permute(0, 2, 3, 1), rtol=0, atol=1e-12)
        loss = loss + (y * dc.permute(0, 3, 1, 2)).sum()
    loss.backward()
    assert torch.allclose(R.dx_taps(dcs, tapss, R.STRIDES, H, W), xs.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    for w, dc, st in zip(ws, dcs, R.STRIDES):
        GS = R.tap_sums(x, dc, st)
        assert torch.allclose(GS[:9].t(), w.grad.view(C, 9), rtol=0, atol=1e-11) and torch.allclose(GS[9], dc.sum((0, 1, 2)))


@pytest.mark.parametrize("band", [2, 4, 6, 8])
def test_banded_models_equal_the_references(band):
    x, tapss, dcs, H, W, C = _rand_geo(1)
    for t, st in zip(tapss, R.STRIDES):
        assert torch.allclose(R.banded_conv(x, t, st, band), R.conv_taps(x, t, st), rtol=0, atol=1e-12)
    for strides in (R.STRIDES, (2, 1), (1, 1, 1)):
        x, tapss, dcs, H, W, C = _rand_geo(2, strides)
        assert torch.allclose(R.banded_dx(dcs, tapss, strides, H, W, band), R.dx_taps(dcs, tapss, strides, H, W), rtol=0, atol=1e-12)


def test_batch_statistics_and_backward_agree_with_batch_norm_autograd():
    c = R.dw_gauss(2, 64, 7, 5, 1, R.STRIDES)
    xi = R.img(c["x"], 1, 7, 5)
    for p in c["p"]:
        p = dict(p, dy_map=R.img(p["dy"], 1, p["Ho"], p["Wo"]))
        xs = xi.permute(0, 3, 1, 2).clone().requires_grad_(True)
        gam, bet = p["gamma"].clone().requires_grad_(True), p["beta"].clone().requires_grad_(True)
        rm, rv = p["run_mean"].clone(), p["run_var"].clone()
        conv = F.conv2d(xs, p["w"].view(64, 1, 3, 3), None, stride=p["stride"], padding=1, groups=64)
        y = F.batch_norm(conv, rm, rv, gam, bet, True, R.MOMENTUM, R.EPS)
        ref = R.dw_train_stats_ref(xi, p)
        assert torch.allclose(ref["run_mean"][0], rm, rtol=0, atol=1e-12) and torch.allclose(ref["run_var"][0], rv, rtol=0, atol=1e-12)
        ya, _ = R.dw_apply_ref(xi, ref["taps"][0], ref["shift"][0], p["stride"])
        assert torch.allclose(ya, y.permute(0, 2, 3, 1), rtol=0, atol=1e-10)
        (y * p["dy_map"].permute(0, 3, 1, 2)).sum().backward()
        b = R.dw_bwd_stats_ref(xi, p, ref["mean"][0], ref["rstd"][0])
        assert torch.allclose(b["dgamma"][0] - p["dg0"], gam.grad, rtol=0, atol=1e-9) and torch.allclose(b["dbeta"][0] - p["db0"], bet.grad, rtol=0, atol=1e-9)
        dc, _ = R.dw_dc_ref(xi, p, b["coef"][0])
        gx = R.dx_taps([dc], [p["taps"]], [p["stride"]], 7, 5)
        assert torch.allclose(gx, xs.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-9)
        for r in (ref, b, R.dw_bwd_stats_ref(xi, p, ref["mean"][0], ref["rstd"][0], streaming=True)):
            assert all(bool((v[1] >= 0).all()) and bool(torch.isfinite(v[1]).all()) for v in r.values())


def test_layernorm_references_agree_with_autograd():
    c = R.ln_gauss(37, 192)
    x = c["x"].double().requires_grad_(True)
    gam, bet = c["gamma"].clone().requires_grad_(True), c["beta"].clone().requires_grad_(True)
    y = F.layer_norm(x, (192,), gam, bet, R.EPS)
    ref = R.ln_fwd_ref(c["x"].double(), c["gamma"], c["beta"])
    assert torch.allclose(ref["y"][0], y, rtol=0, atol=1e-12)
    y.backward(c["dy"].double())
    b = R.ln_bwd_ref(c["x"].double(), c["dy"].double(), c["gamma"], R.ln_stats64(c["x"].double()))
    assert torch.allclose(b["dx"][0], x.grad, rtol=0, atol=1e-11) and torch.allclose(b["dgamma"][0], gam.grad, rtol=0, atol=1e-10)
    assert torch.allclose(b["dbeta"][0], bet.grad, rtol=0, atol=1e-10)


# ------------------------------------------------------------------------------------------------ comparers
def test_device_comparers_are_the_twins_of_bounds_util():
    g = torch.Generator().manual_seed(3)
    v = torch.cat([torch.randn(4000, generator=g).double() * 10.0 ** torch.randint(-6, 6, (4000,), generator=g).double(), torch.tensor([0.0, 1.0, -1.0, 257.0, -257.0])])
    assert np.array_equal(R._bf16_floor_t(v).numpy(), bf16_floor(v.numpy()))
    tol = v.abs() * 1e-3
    out = (v + tol * (torch.rand(v.shape, generator=g).double() * 6.0 - 3.0)).to(BF)
    for i in range(0, len(v), 64):                 # the two comparers accept and reject the same chunks
        a = b = True
        try:
            R.assert_bf16_bracket_t(out[i:i + 64], v[i:i + 64], tol[i:i + 64], "t")
        except AssertionError:
            a = False
        try:
            assert_bf16_bracket(out[i:i + 64], v[i:i + 64].numpy(), tol[i:i + 64].numpy(), "n")
        except AssertionError:
            b = False
        assert a == b
    r = torch.tensor([1.0, 3.0, 1000.0], dtype=F64)
    R.assert_f32_t(r.float(), r, 0.0, 0, "f32")
    _rejects(R.assert_f32_t, torch.nextafter(r.float(), torch.tensor(2000.0)), r, 0.0, 0, "f32")
    R.assert_f32_t(torch.nextafter(r.float(), torch.tensor(2000.0)), r, 0.0, 1, "f32")
    _rejects(R.assert_exact_t, torch.tensor([float("nan")]), torch.tensor([0.0], dtype=F64), "nan")
    R.assert_exact_t(torch.tensor([-0.0]), torch.tensor([0.0], dtype=F64), "zero")
    R.assert_exact_t(torch.tensor([257.0, 259.0]).to(BF), torch.tensor([257.0, 259.0], dtype=F64), "rne")          # 256 and 260: ties to even
    _rejects(R.assert_exact_t, torch.tensor([258.0, 260.0]).to(BF), torch.tensor([257.0, 259.0], dtype=F64), "rne")
    codes = torch.from_numpy(G.e4m3_encode(np.array([1.0, 1.0625, 1.0625, 300.0])))
    assert R.assert_e4m3_one_step(codes, np.array([1.0, 1.0625, 1.05, 300.0]), "e4m3") == 0.0
    R.assert_e4m3_one_step(torch.from_numpy(G.e4m3_encode(np.array([1.125, -0.9375]))), np.array([1.0, -1.0]), "one step")
    _rejects(R.assert_e4m3_one_step, torch.from_numpy(G.e4m3_encode(np.array([1.25]))), np.array([1.0]), "two steps")
    _rejects(R.assert_e4m3_one_step, torch.tensor([0x7F], dtype=torch.uint8), np.array([1.0]), "nan")


# ------------------------------------------------------------------------------------------------ generators
def test_exact_generator_covers_every_table_and_states_its_share():
    geos = [tuple(g[:5]) + (R.STRIDES,) for g in R.DW_GEOMETRIES] + [(g_, 64, 2, 2, g_ % 2, R.STRIDES) for g_ in R.DW_REDUCE_G]
    geos += [tuple(geo) + (st,) for st, geo in R.DW_STRIDE_LISTS] + [R.DW_FORCED + (R.STRIDES,)]
    for geo in geos:
        c = R.dw_exact(*geo)                       # asserts the 2^24 caps, the e4m3 representability and the share itself
        assert c["wide"] >= R.WIDE_SHARE
        for p in c["p"]:
            for k in ("y", "dy", "GS", "dw", "mean", "dgamma", "dbeta"):
                assert torch.equal(p[k].float().double(), p[k]), k
            assert torch.equal(p["dy"].to(BF).double(), p["dy"])
    c = R.dw_exact(2, 64, 7, 5, 0, R.STRIDES)
    assert len({float(v) for v in c["x"].flatten()[:2000]}) > 20 and float(c["p"][0]["mean"].abs().max()) > 0


def test_gauss_generator_places_the_gates_and_the_offsets():
    for *geo, _, _, _, _ in R.DW_GEOMETRIES:
        c = R.dw_gauss(*geo, R.STRIDES)
        xi = R.img(c["x"], geo[4], geo[2], geo[3])
        gates = []
        for p in c["p"]:
            r = R.dw_train_stats_ref(xi, p)
            gates.append(R.stream_gate(p, R.f32r(r["mean"][0]), R.f32r(r["rstd"][0])).view(-1, 64)[:, 0].tolist())
        assert all(gates[0]) and not gates[1][0] and not gates[2][-1], (geo, gates)
        assert geo[1] == 64 or (all(gates[1][1:]) and all(gates[2][:-1])), (geo, gates)
    c = R.dw_gauss(128, 64, 13, 3, 0, R.STRIDES)
    assert float(c["x"].mean((0, 1)).abs().median()) > 0.5 and float(c["x"].abs().max()) > 16.0


# ------------------------------------------------------------------------------------------------ mutants: depthwise projections
def _sentinel_bf16():
    return float(torch.tensor([_SENT[BF][1]], dtype=torch.int16).view(BF))


def _families():
    """(name, x map, taps, gradient maps, accept(out64 -> bf16 out, ref, tol) raising on a mismatch)"""
    Bn, C, H, W, tok0 = GEO
    ce, cg = R.dw_exact(*GEO, R.STRIDES), R.dw_gauss(*GEO, R.STRIDES)
    ex = ("exact", R.img(ce["x"], tok0, H, W), [p["taps"] for p in ce["p"]], [R.img(p["dy"], tok0, p["Ho"], p["Wo"]) for p in ce["p"]],
          lambda out, ref, tol, what: R.assert_exact_t(out.float().to(BF), ref, what))
    ga = ("gauss", R.img(cg["x"], tok0, H, W), [p["taps"] for p in cg["p"]], [R.img(p["dy"], tok0, p["Ho"], p["Wo"]) for p in cg["p"]],
          lambda out, ref, tol, what: R.assert_bf16_bracket_t(out.to(BF), ref, tol, what))
    return ex, ga


@pytest.mark.parametrize("mut", ["halo", "ragged", "padcol", "slices"])
def test_apply_mutants_are_rejected(mut):
    for name, x, tapss, _, accept in _families():
        for taps, st in zip(tapss, R.STRIDES):
            ref, tol = R.dw_apply_ref(x, taps, torch.zeros(GEO[1], dtype=F64), st)
            accept(R.banded_conv(x, taps, st, BAND), ref, tol, f"{name} stride {st}")
            with pytest.raises(AssertionError):
                accept(R.banded_conv(x, taps, st, BAND, mut), ref, tol, f"{name} {mut} stride {st}")


@pytest.mark.parametrize("mut", ["halo", "ragged", "plus1", "parity"])
def test_dx_mutants_are_rejected(mut):
    H, W = GEO[2], GEO[3]
    for name, _, tapss, dcs, accept in _families():
        ref, tol = R.dw_dx_ref(dcs, tapss, R.STRIDES, H, W)
        accept(R.banded_dx(dcs, tapss, R.STRIDES, H, W, BAND), ref, tol, name)
        with pytest.raises(AssertionError):
            accept(R.banded_dx(dcs, tapss, R.STRIDES, H, W, BAND, mut), ref, tol, f"{name} {mut}")


def test_class_token_row_written_by_the_wrong_band_is_rejected_where_there_is_one_band():
    """apply and dx of a case assembled by the banded models, the class-token rows written by band 1 instead of band 0: with one band (band 8 on 7
    rows) nobody writes them and both families reject the output; with several bands the output is the same and passes."""
    Bn, C, H, W, tok0 = geo = (2, 64, 7, 5, 1)
    sent = _sentinel_bf16()
    for name, c in (("exact", R.dw_exact(*geo, R.STRIDES)), ("gauss", R.dw_gauss(*geo, R.STRIDES))):
        xi = R.img(c["x"], tok0, H, W)
        p = c["p"][1]
        taps, shift = p["taps"], p.get("shift", torch.zeros(C, dtype=F64))
        dcs, tapss = [R.img(q["dy"], tok0, q["Ho"], q["Wo"]) for q in c["p"]], [q["taps"] for q in c["p"]]
        yref, ytol = R.dw_apply_ref(xi, taps, shift, p["stride"])
        dref, dtol = R.dw_dx_ref(dcs, tapss, R.STRIDES, H, W)
        cls_dx = sum(q["dy"][:, :tok0] for q in c["p"])
        refs = (R.with_cls(c["x"][:, :tok0], yref), R.with_cls(torch.zeros_like(cls_dx), ytol)), \
               (R.with_cls(cls_dx, dref), R.with_cls(3.0 * G.U * sum(q["dy"][:, :tok0].abs() for q in c["p"]), dtol))
        for band, cls_band, ok in ((8, 0, True), (8, 1, False), (2, 0, True), (2, 1, True)):
            nb = -(-H // band)
            outs = (R.banded_tokens(c["x"][:, :tok0], R.banded_conv(xi, taps, p["stride"], band) + shift, nb, cls_band, sent),
                    R.banded_tokens(cls_dx, R.banded_dx(dcs, tapss, R.STRIDES, H, W, band), nb, cls_band, sent))
            for out, (ref, tol), what in zip(outs, refs, ("apply", "dx")):
                check = (lambda: R.assert_exact_t(out.float().to(BF), ref, what)) if name == "exact" else (lambda: R.assert_bf16_bracket_t(out.to(BF), ref, tol, what))
                if ok:
                    check()
                else:
                    with pytest.raises(AssertionError):
                        check()


@pytest.mark.parametrize("sign", [-1.0, 1.0], ids=["dropped", "twice"])
def test_row_reduction_mutants_are_rejected(sign):
    Bn, C, H, W, tok0 = GEO
    for name, x, _, dcs, _ in _families():
        for dc, st in zip(dcs, R.STRIDES):
            GS, tol = R.dw_taps_ref(x, dc, st, dc.shape[0] * dc.shape[1] * dc.shape[2])
            part = R.tap_sums(x[-1:], dc[-1:], st)                  # the partial rows of one image
            if name == "exact":
                R.assert_exact_t(GS.float(), GS, "GS")
                _rejects(R.assert_exact_t, (GS + sign * part).float(), GS, "GS mutant")
            else:
                R.assert_f32_t(GS.float(), GS, tol, 2, "GS")
                _rejects(R.assert_f32_t, (GS + sign * part).float(), GS, tol, 2, "GS mutant")


def test_gauss_bound_of_a_large_reduction_is_looser_than_one_partial_row_and_the_exact_family_is_not():
    """(400, 64, 9, 3): 10800 terms in 400 partial rows. The any-order bound 10801 U sum |terms| exceeds the partial row of one image in most columns,
    so the gauss family alone would let a dropped row pass there; the exact family's integers do not."""
    geo = (400, 64, 9, 3, 0)
    cg, ce = R.dw_gauss(*geo, R.STRIDES), R.dw_exact(*geo, R.STRIDES)
    x, dc = R.img(cg["x"], 0, 9, 3), R.img(cg["p"][0]["dy"], 0, 9, 3)
    GS, tol = R.dw_taps_ref(x, dc, 1, 10800)
    assert float((R.tap_sums(x[-1:], dc[-1:], 1).abs() < tol).double().mean()) > 0.5
    xe, de = R.img(ce["x"], 0, 9, 3), R.img(ce["p"][0]["dy"], 0, 9, 3)
    _rejects(R.assert_exact_t, (ce["p"][0]["GS"] - R.tap_sums(xe[-1:], de[-1:], 1)).float(), ce["p"][0]["GS"], "exact GS mutant")


# ------------------------------------------------------------------------------------------------ mutants: LayerNorm
LN_ROWS, LN_C = 512 * 4 * 2 + 3, 768             # 1025 row groups of 4 on 512 workgroups: up to 3 iterations, 1 dead row


def _ln_case():
    c = R.ln_gauss(LN_ROWS, LN_C)
    x, dy = c["x"].double(), c["dy"].double()
    return c, x, dy, R.ln_stats64(x)


def test_layernorm_reference_rounded_passes_every_comparer():
    c, x, dy, stats = _ln_case()
    f = R.ln_fwd_ref(x, c["gamma"], c["beta"])
    R.assert_bf16_bracket_t(f["y"][0].to(BF), *f["y"], "y")
    R.assert_f32_t(f["mean"][0].float(), *f["mean"], 2, "mean")
    R.assert_f32_t(f["rstd"][0].float(), *f["rstd"], 4, "rstd")
    b = R.ln_bwd_ref(x, dy, c["gamma"], R.f32r(stats), c["add"].double())
    R.assert_bf16_bracket_t(b["dx"][0].to(BF), *b["dx"], "dx")
    fac = torch.rand(LN_ROWS, 1, dtype=F64)
    R.assert_bf16_bracket_t((b["dx"][0] * fac).to(BF), *R.scaled(b["dx"], fac), "dx2")
    for k in ("dgamma", "dbeta"):
        R.assert_f32_t(b[k][0].float(), *b[k], 2, k)
    codes = torch.from_numpy(G.e4m3_encode((f["y"][0] / 0.25).clamp(-448, 448).numpy()))
    assert R.assert_e4m3_one_step(codes, (f["y"][0] / 0.25).clamp(-448, 448).numpy(), "q8") == 0.0


def test_layernorm_stale_stage_is_rejected():
    c, x, dy, stats = _ln_case()
    stale = torch.cat([stats[1:], stats[-1:]])                      # every row normalised with the next row's mean and rstd
    b = R.ln_bwd_ref(x, dy, c["gamma"], stats)
    _rejects(R.assert_bf16_bracket_t, R.ln_bwd_ref(x, dy, c["gamma"], stale)["dx"][0].to(BF), *b["dx"], "stale dx")
    f = R.ln_fwd_ref(x, c["gamma"], c["beta"])
    y = (x - stale[:, :1]) * stale[:, 1:] * c["gamma"] + c["beta"]
    _rejects(R.assert_bf16_bracket_t, y.to(BF), *f["y"], "stale y")


def test_layernorm_second_stage_missing_from_dgamma_is_rejected():
    c, x, dy, stats = _ln_case()
    b = R.ln_bwd_ref(x, dy, c["gamma"], stats)
    it = (torch.arange(LN_ROWS) // R.LN_BWD_RPB[LN_C]) // R.LN_BWD_CAP              # loop iteration that handles the row
    assert set(it.tolist()) == {0, 1, 2}
    keep = it != 1
    part = R.ln_bwd_ref(x[keep], dy[keep], c["gamma"], stats[keep])
    _rejects(R.assert_f32_t, part["dgamma"][0].float(), *b["dgamma"], 2, "dgamma without stage 1")


def test_layernorm_dead_rows_in_dbeta_are_rejected():
    c, x, dy, stats = _ln_case()
    dead = R.ln_plan(LN_ROWS, LN_C)["dead"]
    assert dead == 1
    dyi, db0 = R.ln_exact_dy(LN_ROWS, LN_C)
    ref = db0 + dyi.double().sum(0)
    R.assert_exact_t(ref.float(), ref, "dbeta")
    _rejects(R.assert_exact_t, (ref + dead * dyi[-1].double()).float(), ref, "dbeta with dead rows")
    # gauss: rejected at few rows (5 rows, 3 dead); at LN_ROWS the any-order bound rows U sum |dy| is above one row of dy in most columns
    c5 = R.ln_gauss(5, LN_C)
    b5 = R.ln_bwd_ref(c5["x"].double(), c5["dy"].double(), c5["gamma"], R.ln_stats64(c5["x"].double()))
    _rejects(R.assert_f32_t, (b5["dbeta"][0] + 3 * c5["dy"][-1].double()).float(), *b5["dbeta"], 2, "dbeta with dead rows")
    b = R.ln_bwd_ref(x, dy, c["gamma"], stats)
    assert float((dy[-1].abs() < b["dbeta"][1]).double().mean()) > 0.5


def test_layernorm_variance_without_the_mean_is_rejected():
    c, x, dy, stats = _ln_case()
    f = R.ln_fwd_ref(x, c["gamma"], c["beta"])
    rstd = ((x * x).mean(1) + R.EPS) ** -0.5
    _rejects(R.assert_f32_t, rstd.float(), *f["rstd"], 4, "rstd")
    y = (x - stats[:, :1]) * rstd[:, None] * c["gamma"] + c["beta"]
    _rejects(R.assert_bf16_bracket_t, y.to(BF), *f["y"], "y")


def test_projection_references_rounded_pass_every_comparer():
    Bn, C, H, W, tok0 = GEO
    c = R.dw_gauss(*GEO, R.STRIDES)
    xi = R.img(c["x"], tok0, H, W)
    dcs = []
    for p in c["p"]:
        p = dict(p, dy_map=R.img(p["dy"], tok0, p["Ho"], p["Wo"]))
        st = R.dw_train_stats_ref(xi, p)
        for k, (ref, tol, ulps) in st.items():
            R.assert_f32_t(ref.float(), ref, tol, ulps, k)
        y, tol = R.dw_apply_ref(xi, R.f32r(st["taps"][0]), R.f32r(st["shift"][0]), p["stride"])
        R.assert_bf16_bracket_t(y.to(BF), y, tol, "y")
        m, r = R.f32r(st["mean"][0]), R.f32r(st["rstd"][0])
        yf = R.bfr(R.dw_forward_output(xi, p, m, r))
        gate = R.stream_gate(p, m, r)
        cs = torch.where(gate, m + (yf - p["beta"]) / (p["gamma"] * r), R.conv_taps(xi, p["taps"], p["stride"]))      # what the streaming pass sums
        for streaming in (False, True):
            b = R.dw_bwd_stats_ref(xi, p, m, r, streaming)
            for k, (ref, tol, ulps) in b.items():
                R.assert_f32_t(ref.float(), ref, tol, ulps, k)
        D = (p["dy_map"] * cs).sum((0, 1, 2))
        S = p["dy_map"].sum((0, 1, 2))
        R.assert_f32_t((p["dg0"] + r * (D - m * S)).float(), *b["dgamma"][:2], 2, "dgamma from the rounded forward output")
        dc, tol = R.dw_dc_ref(xi, p, R.f32r(b["coef"][0]))
        R.assert_bf16_bracket_t(dc.to(BF), dc, tol, "dc")
        dcs.append(R.bfr(dc))
        GS, tol, dw, tol_dw = R.dw_taps_ref(xi, dcs[-1], p["stride"], p["count"], p["dw0"])
        R.assert_f32_t(GS.float(), GS, tol, 2, "GS"), R.assert_f32_t(dw.float(), dw, tol_dw, 2, "dw")
    dx, tol = R.dw_dx_ref(dcs, [p["taps"] for p in c["p"]], R.STRIDES, H, W)
    R.assert_bf16_bracket_t(dx.to(BF), dx, tol, "dx")
