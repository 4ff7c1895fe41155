"""CPU: the generators, references and comparers of tests/gemm_ref.py themselves. Mutation tests: outputs that model a subtly wrong kernel (one
K element dropped, one 32-deep K-step dropped from a 128-row tile, two rows swapped, a stale last row of a ragged tile, the accumulator rounded
to bf16 before the residual, one token split added twice) must be rejected; the reference rounded to the output type must pass."""
import numpy as np
import pytest
import torch
import gemm_ref as G

BF, F32 = torch.bfloat16, torch.float32
NT_SHAPE = (257, 196, 96)
TN_SHAPE = (1025, 72, 136)


def _to(ref, dtype):
    r = torch.as_tensor(ref, dtype=torch.float64).float()
    return r if dtype == F32 else r.to(BF)


def _pre_residual(c):
    """(alpha acc + bias, residual) of a case without dropout or row scale"""
    v = c.get("alpha", 1.0) * (c["a"] @ c["w"].t())
    if c.get("bias") is not None:
        v = v + c["bias"][None, :]
    return v, c["residual"]


def _nt_mutants(c):
    """name -> wrong float64 [M, N] of a bias+residual case"""
    M, N, K = c["M"], c["N"], c["K"]
    assert M > 256 and K >= 64
    al = c.get("alpha", 1.0)
    pre, res = _pre_residual(c)
    good = pre + res
    a, w = c["a"], c["w"]
    m = 130
    k = int((a[m] != 0).nonzero()[0])
    out = {}
    out["one K element dropped"] = good.clone()
    out["one K element dropped"][m] -= al * a[m, k] * w[:, k]
    out["one K-step dropped from a row tile"] = good.clone()
    out["one K-step dropped from a row tile"][128:256] -= al * (a[128:256, 32:64] @ w[:, 32:64].t())
    out["two rows swapped"] = good.clone()
    out["two rows swapped"][[m, m + 1]] = good[[m + 1, m]]
    out["stale last row"] = good.clone()
    out["stale last row"][M - 1] = good[M - 1 - 128]
    out["bf16 before the residual"] = pre.float().to(BF).double() + res
    return good, out


def _tn_mutant(c):
    out, _ = G.tn_reference(c)
    splits, per, _ = G.tn_plan(c["R"], c["I"], c["J"])
    assert splits > 1
    r0, r1 = 32 * per, min(c["R"], 64 * per)
    bad = out.clone()
    bad[:128, :128] += c["alpha"] * (c["p"][r0:r1, :128].t() @ c["q"][r0:r1, :128])
    return out, bad


# ------------------------------------------------------------------------------------------------ exact comparer
def test_exact_comparer_accepts_the_rounded_reference_and_rejects_every_mutant():
    c = G.exact_nt(*NT_SHAPE, "bias+residual")
    good, mutants = _nt_mutants(c)
    assert torch.equal(good, G.nt_reference(c)[0])
    for dtype in (BF, F32):
        G.assert_exact(_to(good, dtype), good, "reference")
        for name, bad in mutants.items():
            if dtype == F32 and name == "bf16 before the residual":
                assert not torch.equal(bad, good)
            with pytest.raises(AssertionError, match="differ from the exact value"):
                G.assert_exact(_to(bad, dtype), good, name)
    # a NaN and a wrong shape do not pass either; the sign of a zero does not matter
    z = torch.zeros(2, 2)
    G.assert_exact(-z, z.double(), "minus zero")
    with pytest.raises(AssertionError):
        G.assert_exact(torch.full((2, 2), float("nan")), z.double(), "nan")


def test_exact_comparer_sees_a_swapped_row_of_the_scaled_plain_family():
    c = G.exact_nt(*NT_SHAPE, "plain")
    assert len(set(c["sa"].tolist())) > 1 and len(set(c["sw"].tolist())) > 1
    good = G.nt_reference(c)[0]
    G.assert_exact(_to(good, BF), good, "reference")
    bad = good.clone()
    bad[:, [7, 8]] = good[:, [8, 7]]
    with pytest.raises(AssertionError):
        G.assert_exact(_to(bad, BF), good, "columns swapped")


def test_exact_comparer_rejects_a_split_added_twice():
    for alpha in (1.0, 0.5):
        c = G.exact_tn(*TN_SHAPE, alpha)
        good, bad = _tn_mutant(c)
        G.assert_exact(_to(good, F32), good, "reference")
        with pytest.raises(AssertionError, match="differ from the exact value"):
            G.assert_exact(_to(bad, F32), good, "split added twice")
        db = G.tn_reference(c)[1]
        G.assert_exact(_to(db, F32), db, "dbias")


# ------------------------------------------------------------------------------------------------ gauss comparer
def test_gauss_comparer_accepts_the_rounded_reference_and_rejects_the_large_mutants():
    for variant, dtype in (("bias+residual", BF), ("f32", F32)):
        c = G.gauss_nt(*NT_SHAPE, variant)
        if variant == "f32":
            c["residual"] = torch.zeros(c["M"], c["N"], dtype=torch.float64)
        good, mutants = _nt_mutants(c)
        if variant == "f32":
            c.pop("residual")
        ref, tol = G.gauss_nt_tol(c)
        assert np.array_equal(ref, good.numpy())
        prod = c["a"] @ c["w"].t()
        assert float(prod[0, 0]) == 0.0 and float((c["a"][0].abs() * c["w"][0].abs()).sum()) > 1.0            # an output that cancels to zero
        assert torch.equal(c["a"][c["M"] - 1], -c["a"][0])
        assert G.assert_gauss(_to(good, dtype), ref, tol, "reference") <= 1.0
        for name in ("one K-step dropped from a row tile", "two rows swapped", "stale last row"):
            bad = mutants[name]
            assert float(((bad - good).abs().numpy() > 2 * tol + (2.0 ** -7 * np.abs(ref) if dtype == BF else 0)).sum()) > 0, name
            with pytest.raises(AssertionError):
                G.assert_gauss(_to(bad, dtype), ref, tol, name)


def test_gauss_comparer_rejects_a_split_added_twice():
    c = G.gauss_tn(*TN_SHAPE)
    good, bad = _tn_mutant(c)
    ref, tol, db, tol_db = G.gauss_tn_tol(c)
    assert G.assert_gauss(_to(good, F32), ref, tol, "reference") <= 1.0
    assert G.assert_gauss(_to(db, F32), db, tol_db, "dbias") <= 1.0
    with pytest.raises(AssertionError):
        G.assert_gauss(_to(bad, F32), ref, tol, "split added twice")


def test_gauss_tolerance_is_the_derived_one():
    c = G.gauss_nt(17, 60, 96, "bias+residual")
    ref, tol = G.gauss_nt_tol(c)
    s = (c["a"].abs() @ c["w"].abs().t()).numpy()
    pre = G.GAUSS_ALPHA * (c["a"] @ c["w"].t()).numpy() + c["bias"].numpy()[None]
    want = G.GAUSS_ALPHA * 2 * 96 * 2.0 ** -24 * s + 4 * G.ulp32(pre) + 4 * G.ulp32(ref)
    assert np.allclose(tol, want, rtol=1e-12, atol=0)
    hot = (c["a"].abs().amax(0) > 30).sum()
    assert 1 <= int(hot) <= 96 // 10 + 2


# ------------------------------------------------------------------------------------------------ generators
def test_exact_family_keeps_every_partial_sum_below_2_24():
    for M, N, K in [(33, 100, 3072), (257, 196, 224), (129, 68, 128)]:
        for variant in G.NT_VARIANTS:
            c = G.exact_nt(M, N, K, variant)
            assert c["cap"] < G.CAP and c["wide"] >= 0.25, (M, N, K, variant)
            for key in ("a", "w", "residual"):
                if c.get(key) is not None:
                    assert torch.equal(c[key].to(BF).double(), c[key])
            assert float(c["a"].abs().max() / c["sa"].max()) <= G.VMAX
    assert 225 * 3072 * 8 < G.CAP and 225 * 45056 < G.CAP
    for R, I, J in [(16001, 128, 128), (4129, 520, 136)]:
        c = G.exact_tn(R, I, J, 0.5)
        assert c["cap"] < G.CAP and c["wide"] >= 0.25
    with pytest.raises(AssertionError, match=r"2\^24"):
        G.exact_nt(4, 8, 96, "plain", vmax=2000)
    for M, N, K in G.FP8[:3]:
        for variant in G.FP8_VARIANTS:
            c = G.exact_fp8(M, N, K, variant)
            assert c["wide"] >= 0.25 and float(G.nt_reference(c)[0].abs().max()) / c["out_scale"] <= 448.0
            assert np.log2(c["out_scale"]) == round(np.log2(c["out_scale"]))


def test_e4m3_rounding_is_nearest_even_over_the_finite_codes():
    v = G.E4M3_VALUES
    assert np.isnan(v[0x7F]) and np.isnan(v[0xFF]) and v[0x7E] == 448.0 and v[0x01] == 2.0 ** -9 and v[0x38] == 1.0
    fin = np.array([c for c in range(256) if c not in (0x7F, 0xFF)])
    assert np.array_equal(G.e4m3_encode(v[fin]) & 0x7F, fin & 0x7F)
    assert np.array_equal(v[G.e4m3_encode(v[fin])], v[fin])
    x = torch.linspace(-448, 448, 20001, dtype=torch.float64)
    x = torch.cat([x, torch.tensor([17.0, 19.0, 21.0, 23.0, 2.0 ** -10, 3 * 2.0 ** -10, 0.0])])      # ties: 17 -> 16, 19 -> 20, ...
    want = x.float().to(torch.float8_e4m3fn).float().double().numpy()
    assert np.array_equal(v[G.e4m3_encode(x.numpy())], want)
    assert v[G.e4m3_encode(np.array([17.0]))][0] == 16.0 and v[G.e4m3_encode(np.array([19.0]))][0] == 20.0


def test_embedded_operands_are_surrounded_by_nans_and_aligned():
    t = torch.arange(24, dtype=torch.float64).reshape(3, 8) - 12
    v = G.embed(t)
    assert torch.equal(v.double(), t) and v.stride(0) % 8 == 0 and v.storage_offset() % 8 == 0
    base = v._base if v._base is not None else v
    assert int(torch.isnan(base.float()).sum()) == base.numel() - 24
    v8 = G.embed_e4m3(t)
    assert torch.equal(v8.float().double(), t) and v8.stride(0) % 16 == 0 and v8.storage_offset() % 16 == 0
    assert G.embed(t, ld=20).stride(0) % 8 == 4
    with pytest.raises(AssertionError, match="not exact"):
        G.embed(t + 1000.5)


# ------------------------------------------------------------------------------------------------ case tables
def _col(cases, i):
    return {c[i] for c in cases}


def test_case_tables_hold_every_listed_size():
    t = G.TILED_BN64
    assert _col(t, 0) >= {1, 17, 127, 128, 129, 257} and _col(t, 1) >= {4, 60, 64, 68, 132, 196}
    assert _col(t, 2) >= {32, 96, 160, 224, 64, 128, 192, 320}
    assert {k for m, n, k in t if (m, n) == (257, 196)} >= {32, 96, 160, 224, 64, 128, 192, 320}
    for m, n, k in t:
        assert -(-m // 128) * -(-n // 128) <= 256                            # BN = 64
    t = G.TILED_BN128
    assert _col(t, 0) == {16513} and _col(t, 1) >= {224, 228, 256} and _col(t, 2) >= {64, 96, 192} and (16513, 224, 96) in t
    for m, n, k in t:
        assert -(-m // 128) * -(-n // 128) > 256 and (n % 128 == 0 or n % 128 > 64)
    assert set(G.TILED_REGSTAGE) == {(129, 196, 96), (257, 132, 128)}
    assert set(G.TILED_STAGES) == {(257, 196, k) for k in (32, 64, 96, 160)}
    assert set(G.TILED_EPILOGUE) == {(257, 196, 96), (129, 68, 128)} and G.ROWS_PER_IMAGE == 77 and 128 % G.ROWS_PER_IMAGE
    assert G.GROUPS == [((257, 1, 129), 196, 96), ((129, 130), 64, 64)]
    assert set(G.CONVS) >= {(1, 64, 64, 3, 3), (2, 64, 196, 7, 5), (1, 128, 132, 9, 20)} and any(h == w == 1 for *_, h, w in G.CONVS)
    assert set(G.STRIP384) == {(2, 0), (4, 0), (6, 0), (10, 0), (10, 2), (10, 3), (10, 4)} and G.STRIP192 == [8, 12, 16]
    for mt, _ in G.STRIP384:
        s = G.strip_shapes(mt)
        assert _col(s, 0) == {1, 16 * mt - 1, 16 * mt + 1, 32 * mt + 17} and _col(s, 1) == {384} and _col(s, 2) == {64, 128, 192, 320}
    for mt in G.STRIP192:
        s = G.strip_shapes(mt, True)
        assert _col(s, 0) == {1, 16 * mt - 1, 16 * mt + 1, 32 * mt + 17} and _col(s, 1) == {192} and _col(s, 2) == {64, 192}
    assert _col(G.WS, 0) == {1, 31, 32, 33, 65, 1000} and _col(G.WS, 1) == {384, 768, 1152} and _col(G.WS, 2) == {384}
    assert _col(G.PK, 0) == {1, 63, 65, 255, 257, 513} and _col(G.PK, 1) == {8, 136, 264} and _col(G.PK, 2) == {64, 128, 192}
    assert _col(G.TN4, 0) >= {1, 31, 32, 33, 255, 257, 3401}
    assert _col(G.TN4, 1) | _col(G.TN4, 2) == {8, 72, 128, 136, 200, 264} == _col(G.TN4, 1) == _col(G.TN4, 2)
    assert {G.tn_split_class(G.tn_plan(*s)[0]) for s in G.TN4} == {"atomic", "SL1", "SL4", "SL16"}
    assert set(G.TN2) == {(r, i, j) for (i, j) in ((136, 136), (256, 264), (520, 136)) for r in (33, 257, 4129)}
    assert set(G.TN5) == {(r, i, j) for (i, j) in ((384, 192), (384, 576), (768, 192)) for r in (33, 257, 4129)}
    assert _col(G.SKINNY, 0) == {1, 15, 16, 17, 33, 48, 49, 64} and _col(G.SKINNY, 1) == {1, 15, 16, 17, 100}
    assert _col(G.SKINNY, 2) == {128, 384, 768, 2048, 3072}
    assert {c[0] for c in G.DEC} == {1, 15, 16, 17, 33, 47, 64} and {c[1] for c in G.DEC} == {768, 3072}
    assert {n for c in G.DEC for n in c[2]} >= {16, 18, 48, 770} and {len(c[2]) for c in G.DEC} == {1, 2, 3}
    assert {c[3] for c in G.DEC} == {"rows", "f32", "dal"} and {c[5] for c in G.DEC} == {0, 1} and G.DEC_VOCAB == (33, 768, 8192)
    assert all(c[2][0] % 32 == 0 for c in G.DEC if c[3] == "dal")
    assert _col(G.FP8, 0) == {1, 127, 129} and _col(G.FP8, 1) == {64, 68, 132} and _col(G.FP8, 2) == {64, 128, 192}


def test_weight_gradient_plan_classes():
    assert G.tn_plan(3401, 128, 128)[0] == 12 and G.tn_plan(8001, 128, 72)[0] == 28 and G.tn_plan(16001, 128, 128)[0] == 56
    assert G.tn_plan(257, 264, 200)[0] == 1 and G.tn_plan(45056, 128, 128)[0] == 176
    for R in (8001, 16001):
        splits, per, nrt = G.tn_plan(R, 128, 128)
        assert R % 32 and nrt % per                                            # the last 32-row tile and the last split are ragged
