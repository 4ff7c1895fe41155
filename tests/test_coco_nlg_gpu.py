"""GPU: the COCO NLG metric (reference tools/metrics/coco.py) -- `cxr_coco_nlg_scores` against the fixture recorded from the reference class and
against the float64 restatement (tests/coco_nlg_ref.py) at the size of a test epoch, its bit-reproducibility, its length cap, workspace check and
degenerate inputs, the `ops` wrapper against the entry point, and `COCONLGMetricsMIMICCXR` end to end: dict, CSV, injected extra scorer.

Tolerances (coco_nlg_ref.assert_scores_close applies them; zeros must be exact zeros on both sides):
  ints          exact.
  BLEU, ROUGE   rtol 1e-12, atol 0. Each is a handful of float64 pow / exp / divide operations on exact integers; a few ulp (1e-15) apart at the
                most. Values near 1e-13 are legitimate (a record without a matching 4-gram), so no atol may hide them.
  CIDEr         rtol 32 * M * 2^-52 (2.1e-11 at M = 3000), atol 1e-14. The weight w = log M - log df cancels as df -> M. With a `log` within 1 ulp
                on each side, |dw| <= 2 ulp(log M) = 2^-48 for 8 <= log M < 16 (M = 3000: log M = 8.006), against a smallest nonzero weight
                log M - log(M - 1) ~ 1 / M: a relative error of w of up to M * 2^-48 = 16 M 2^-52. A score is at most quadratic in w, which
                doubles it: 32 M 2^-52. The sums' rounding (a few hundred non-negative terms, n * 2^-53 ~ 4e-14) is far inside that.
                Measured on the large case below (M = 3000, 700 labels) by moving the restatement's two logarithms one ulp up / down as a
                function of their argument (log M up and every log df down, the reverse, and alternating by df; a shift that depends on the
                argument alone keeps log M - log M = 0, as any real `log` does): the largest relative change of any record's CIDEr is
                7.09e-13, the largest absolute change 6.4e-14 -- a thirtieth of the bound, because n-grams whose df is near M (weights near
                1 / M) contribute next to nothing to a score. The derived bound is the one asserted, not the measurement.
"""
import glob
import os

import numpy as np
import pytest
import torch

import coco_nlg_ref as nref
from bounds_util import _SENT, F32, I64, Guarded

pytestmark = pytest.mark.gpu
F64 = torch.float64
CASES = list("abcdefgh")


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


class Guarded64:
    """A float64 output of `shape` inside a sentinel-guarded buffer (the 8-byte integer sentinel, viewed as float64)."""

    def __init__(self, *shape):
        self.g = Guarded.flat(int(np.prod(shape)), I64)
        self.t = self.g.view.view(F64).view(*shape)

    def check(self, what):
        self.g.check(what)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.g.view == _SENT[I64][1]).all())


class Guarded32:
    """An int32 output of `shape` inside a sentinel-guarded buffer (the 4-byte sentinel, viewed as int32)."""

    def __init__(self, *shape):
        self.g = Guarded.flat(int(np.prod(shape)), F32)
        self.t = self.g.view.view(torch.int32).view(*shape)

    def check(self, what):
        self.g.check(what)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.g.view.view(torch.int32) == _SENT[F32][1]).all())


NAMES = ("ids_a", "off_a", "ids_b", "off_b", "pairs", "ref_mult", "order", "study_off")


def _launch(c):
    """One call of the C entry point with every output and the workspace guarded -> (scores, ints, study, avg, workspace)."""
    from cxrmate_amd import ops
    from cxrmate_amd._lib import LIB
    d = {k: torch.as_tensor(np.ascontiguousarray(c[k], dtype=np.int32)).cuda() for k in NAMES}
    n_texts, n_rec, S = len(c["off_a"]) - 1, len(c["pairs"]), len(c["study_off"]) - 1
    need = ops.coco_nlg_workspace_bytes(len(c["ids_a"]), n_rec)
    outs = Guarded64(max(n_rec, 1), 6), Guarded32(max(n_rec, 1), 9), Guarded64(max(S, 1), 6), Guarded64(6), Guarded64(need // 8)
    try:
        LIB.call("cxr_coco_nlg_scores", d["ids_a"].data_ptr(), len(c["ids_a"]), d["off_a"].data_ptr(), d["ids_b"].data_ptr(), len(c["ids_b"]),
                 d["off_b"].data_ptr(), n_texts, d["pairs"].data_ptr(), d["ref_mult"].data_ptr(), n_rec, d["order"].data_ptr(),
                 d["study_off"].data_ptr(), S, outs[0].t.data_ptr(), outs[1].t.data_ptr(), outs[2].t.data_ptr(), outs[3].t.data_ptr(),
                 outs[4].t.data_ptr(), need, ops._s())
    finally:
        for o, name in zip(outs, ("scores", "ints", "study", "avg", "workspace")):
            o.check(f"coco_nlg_scores {name}")
    return outs


def _host(c, outs):
    M, S = len(c["pairs"]), len(c["study_off"]) - 1
    return outs[0].t.cpu().numpy()[:M], outs[1].t.cpu().numpy()[:M], outs[2].t.cpu().numpy()[:S], outs[3].t.cpu().numpy()


def _check_against_restatement(c, outs, what, want=None):
    scores, ints, study, avg = _host(c, outs)
    M = len(c["pairs"])
    want_scores, want_ints = want if want is not None else nref.scores_arrays(c["ids_a"], c["off_a"], c["ids_b"], c["off_b"], c["pairs"])
    assert np.array_equal(ints, want_ints), f"{what}: ints differ at {np.argwhere(ints != want_ints)[:5].tolist()}"
    nref.assert_scores_close(scores, want_scores, M, f"{what} scores")
    want_study, want_avg = nref.study_means(want_scores, c["order"], c["study_off"])
    nref.assert_scores_close(study, want_study, M, f"{what} study")
    nref.assert_scores_close(avg, want_avg, M, f"{what} avg")
    print(f"{what}: max rel err bleu/rouge {_rel(scores[:, :5], want_scores[:, :5]):.3e}, cider {_rel(scores[:, 5], want_scores[:, 5]):.3e}")
    return scores, ints, study, avg


def _rel(a, b):
    nz = b != 0
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


def _case_inputs(case):
    rec = nref.case_records(case)
    c = nref.stage(rec["prediction"], rec["label"])
    c.update(order=rec["order"], study_off=rec["study_off"])
    return c


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("name", CASES)
def test_kernel_vs_recorded_reference(cuda, name):
    """Every recorded case: the per-record scores equal the CSV the reference wrote, the averages equal the dict it returned (the columns the
    case asked for), and all six columns, the integers and the per-study means equal the restatement."""
    case = nref.load_fixture()["cases"][name]
    c = _case_inputs(case)
    outs = _launch(c)
    scores, _, _, avg = _check_against_restatement(c, outs, f"case {name}")
    want_scores, want_avg = nref.case_expected(case)
    asked = ~np.isnan(want_avg)
    assert asked.any()
    M = len(c["pairs"])
    nref.assert_scores_close(np.where(asked, scores, 0.0), np.where(asked, want_scores, 0.0), M, f"case {name} rows vs the recorded CSV")
    nref.assert_scores_close(np.where(asked, avg, 0.0), np.where(asked, want_avg, 0.0), M, f"case {name} means vs the recorded dict")


@pytest.fixture(scope="module")
def large():
    c = nref.large_case()
    return c, nref.scores_arrays(c["ids_a"], c["off_a"], c["ids_b"], c["off_b"], c["pairs"])


def test_kernel_vs_restatement_large_and_bitwise_repeatable(cuda, large):
    """M = 3000 records over 700 distinct labels (ref_mult up to 12), 682 079 tokens, word ids up to 79 998, lengths 0-400, 54 records with CIDEr
    exactly 0. Two launches give the same bits in every output although the table's slots differ between them."""
    c, want = large
    assert len(c["pairs"]) == 3000 and (c["ref_mult"] > 0).sum() == 700 and c["ref_mult"].max() > 1 and c["ids_a"].max() > 65535
    lens = np.diff(c["off_a"])
    assert lens.min() == 0 and 350 < lens.max() <= 400
    first = _launch(c)
    scores, ints, _, _ = _check_against_restatement(c, first, "large", want)
    assert (scores[:, 5] == 0).sum() > 0 and (scores[:, 5] > 0).sum() > 2900 and ints[:, 5].max() > 200
    again = _launch(c)
    for a, b, name in zip(first[:4], again[:4], ("scores", "ints", "study", "avg")):
        assert torch.equal(a.g.view, b.g.view), f"{name}: two launches differ"


def _long_case(n):
    """records over two texts of n tokens from 300 words (n-grams repeat inside a text; the second is a noisy copy of the first) and a short third
    text that is also its own reference, so that the long texts' shared n-grams have df < M and CIDEr is not trivially 0"""
    rng = np.random.default_rng(n)
    a = rng.integers(0, 300, size=n)
    b = a.copy()
    flip = rng.random(n) < 0.2
    b[flip] = rng.integers(0, 300, size=int(flip.sum()))
    short = rng.integers(0, 300, size=50)
    ids = np.concatenate([a, b, short]).astype(np.int32)
    off = np.array([0, n, 2 * n, 2 * n + 50], dtype=np.int32)
    return dict(ids_a=ids, off_a=off, ids_b=ids, off_b=off, pairs=np.array([[0, 1], [2, 1], [1, 0], [2, 2]], dtype=np.int32),
                ref_mult=np.array([1, 2, 1], dtype=np.int32), order=np.arange(4, dtype=np.int32), study_off=np.array([0, 2, 4], dtype=np.int32))


def test_length_cap(cuda):
    """A text of exactly 8192 tokens is scored; one of 8193 is refused by the entry point (invalid argument, nothing written) and by the wrapper
    with a ValueError that names the length."""
    from cxrmate_amd import ops
    from cxrmate_amd._lib import CxrError
    c = _long_case(8192)
    out = _check_against_restatement(c, _launch(c), "8192 tokens")
    scores, ints, _, _ = out
    assert ints[0, 0] == 8192 and ints[0, 1] == 8192 and ints[0, 6] > 6000 and scores[0, 5] > 0
    c = _long_case(8193)
    with pytest.raises(CxrError, match="cxr_coco_nlg_scores failed with code -1"):
        _launch(c)
    with pytest.raises(ValueError, match="8193"):
        ops.coco_nlg_scores(*(torch.as_tensor(c[k]).cuda() for k in NAMES))
    c = _long_case(100)                                          # only the split(" ") stream too long
    c["ids_b"] = np.concatenate([c["ids_b"], np.zeros(8193, dtype=np.int32)])
    c["off_b"] = np.array([0, 100, 200, 250 + 8193], dtype=np.int32)
    with pytest.raises(CxrError, match="cxr_coco_nlg_scores failed with code -1"):
        _launch(c)


def test_refusals_write_nothing_and_degenerate_inputs(cuda):
    from cxrmate_amd import ops
    from cxrmate_amd._lib import CxrError, LIB
    c = _case_inputs(nref.load_fixture()["cases"]["b"])
    need = ops.coco_nlg_workspace_bytes(len(c["ids_a"]), len(c["pairs"]))
    d = {k: torch.as_tensor(c[k]).cuda() for k in NAMES}
    M, S = len(c["pairs"]), len(c["study_off"]) - 1

    def call(outs, ws, ws_bytes, off_a=None):
        LIB.call("cxr_coco_nlg_scores", d["ids_a"].data_ptr(), len(c["ids_a"]), (d["off_a"] if off_a is None else off_a).data_ptr(),
                 d["ids_b"].data_ptr(), len(c["ids_b"]), d["off_b"].data_ptr(), len(c["off_a"]) - 1, d["pairs"].data_ptr(), d["ref_mult"].data_ptr(),
                 M, d["order"].data_ptr(), d["study_off"].data_ptr(), S, outs[0].t.data_ptr(), outs[1].t.data_ptr(), outs[2].t.data_ptr(),
                 outs[3].t.data_ptr(), ws.t.data_ptr(), ws_bytes, ops._s())

    bad_off = d["off_a"].clone()
    bad_off[3] = bad_off[2] - 1                                  # decreasing offsets
    past = d["off_a"].clone()
    past[-1] += 1                                                # the last text runs past the stream
    for kw in (dict(ws_bytes=need - 8), dict(ws_bytes=need, off_a=bad_off), dict(ws_bytes=need, off_a=past)):
        outs = Guarded64(M, 6), Guarded32(M, 9), Guarded64(S, 6), Guarded64(6)
        ws = Guarded64(need // 8)
        with pytest.raises(CxrError, match="cxr_coco_nlg_scores failed with code -1"):
            call(outs, ws, **kw)
        assert all(o.untouched() for o in outs) and ws.untouched(), kw
    # M == 0 with studies: every study mean and the averages are NaN (the mean of nothing); S == 0: the per-record scores are still written
    empty = dict(c, pairs=np.zeros((0, 2), dtype=np.int32), order=np.zeros(0, dtype=np.int32), study_off=np.array([0, 0, 0], dtype=np.int32))
    outs = _launch(empty)
    assert outs[0].untouched() and outs[1].untouched()
    assert torch.isnan(outs[2].t[:2]).all() and torch.isnan(outs[3].t).all()
    none = dict(c, order=np.zeros(0, dtype=np.int32), study_off=np.array([0], dtype=np.int32), pairs=np.zeros((0, 2), dtype=np.int32))
    outs = _launch(none)
    assert outs[0].untouched() and outs[2].untouched() and torch.isnan(outs[3].t).all()
    no_study = dict(c, study_off=np.array([0], dtype=np.int32))
    outs = _launch(no_study)
    want, _ = nref.scores_arrays(c["ids_a"], c["off_a"], c["ids_b"], c["off_b"], c["pairs"])
    nref.assert_scores_close(outs[0].t.cpu().numpy(), want, M, "S == 0 scores")
    assert outs[2].untouched() and torch.isnan(outs[3].t).all()
    # texts shorter than the order, an empty hypothesis, an empty reference; a text index outside the table gives NaN / -1 for that record only
    tiny = nref.stage(["a", "a b", "", "a b c", "x y"], ["a", "a b c d e", "a b", "", "x y"])
    tiny.update(order=np.arange(5, dtype=np.int32), study_off=np.array([0, 2, 5], dtype=np.int32))
    scores, ints, study, avg = _check_against_restatement(tiny, _launch(tiny), "tiny")
    assert np.array_equal(scores[2], np.zeros(6)) and ints[2, 0] == 0
    bad = dict(tiny, pairs=tiny["pairs"].copy())
    bad["pairs"][3, 0] = 99
    s2, i2, st2, _ = _host(bad, _launch(bad))
    assert np.isnan(s2[3]).all() and (i2[3] == -1).all() and np.isnan(st2[1]).all()
    assert np.array_equal(s2[:3, :5], scores[:3, :5]) and np.array_equal(i2[:3], ints[:3]) and np.array_equal(st2[0, :5], study[0, :5])


def test_wrapper_equals_the_entry_point(cuda):
    from cxrmate_amd import ops
    c = nref.large_case(seed=3, M=400, n_labels=90, max_len=120)
    direct = _launch(c)
    got = ops.coco_nlg_scores(*(torch.as_tensor(c[k]).cuda() for k in NAMES))
    S = len(c["study_off"]) - 1
    assert [tuple(t.shape) for t in got] == [(400, 6), (400, 9), (S, 6), (6,)]
    assert [t.dtype for t in got] == [F64, torch.int32, F64, F64]
    for a, b, name in zip(direct, got, ("scores", "ints", "study", "avg")):
        assert torch.equal(a.t.view(-1).view(I64 if a.t.dtype == F64 else torch.int32), b.view(-1).view(I64 if b.dtype == F64 else torch.int32)), name


# ------------------------------------------------------------------------------------------------ the class
def _run_metric(case, tmp_path, **kw):
    from cxrmate_amd.metrics import COCONLGMetricsMIMICCXR
    import pandas as pd
    exp = str(tmp_path / "exp")
    metric = COCONLGMetricsMIMICCXR("test", exp, case["accumulate_over_dicoms"], list(case["metrics"]), False, device="cuda", **kw)
    for c in case["calls"]:
        metric.update(c["predictions"], c["labels"], c["study_ids"], c.get("dicom_ids"))
    out = metric.compute(epoch=7)
    files = glob.glob(os.path.join(exp, "nlg_scores", "test_epoch-7_[0-9]*.csv"))
    assert len(files) == 1, files
    return out, pd.read_csv(files[0])


@pytest.mark.parametrize("name", CASES)
def test_metric_returns_the_recorded_dict_and_csv(cuda, tmp_path, name):
    case = nref.load_fixture()["cases"][name]
    out, df = _run_metric(case, tmp_path)
    res = case["result"]
    M = len(case["csv"]["rows"])
    assert list(out) == [k for k, _ in res]                                       # the reference's keys in the reference's order
    assert all(type(v) is float for v in out.values())
    n_ids = 2 if case["accumulate_over_dicoms"] else 1
    assert [out[k] for k, _ in res[:n_ids]] == [v for _, v in res[:n_ids]]
    cols = [k for k, _ in res[n_ids:]]

    def six(values_by_col):
        return np.array([[values_by_col.get(c, 0.0) for c in nref.COLUMNS]], dtype=np.float64)
    nref.assert_scores_close(six(out), six(dict(res)), M, f"{name} dict")
    assert list(df.columns) == case["csv"]["columns"] == (["dicom_id", "study_id"] if n_ids == 2 else ["study_id"]) + cols
    rows = case["csv"]["rows"]
    assert len(df) == M
    for j in range(n_ids):
        assert df.iloc[:, j].tolist() == [r[j] for r in rows]
    got = np.zeros((M, 6))
    want = np.zeros((M, 6))
    for c in cols:
        got[:, nref.COLUMNS.index(c)] = df[c].to_numpy()
        want[:, nref.COLUMNS.index(c)] = [r[case["csv"]["columns"].index(c)] for r in rows]
    nref.assert_scores_close(got, want, M, f"{name} csv")


def test_extra_scorer_column_sits_between_bleu_and_rouge(cuda, tmp_path):
    """An injected METEOR object: called with the reference's (gts, res) dicts of the scored records, its column follows bleu_4 in the dict and the
    CSV, and its per-record values go through the same DICOM -> study -> mean grouping as the device columns."""
    case = dict(nref.load_fixture()["cases"]["b"])
    rec = nref.case_records(case)
    seen = {}

    class Meteor:
        def compute_score(self, gts, res):
            seen["gts"], seen["res"] = gts, res
            per = [len(res[k][0].split()) / (1.0 + len(gts[k][0].split())) for k in gts]
            return float(np.mean(per)), per
    case["metrics"] = ["bleu", "cider", "meteor", "rouge"]
    out, df = _run_metric(case, tmp_path, extra_scorers={"meteor": Meteor()})
    assert list(out) == ["num_study_ids", "num_dicom_ids", "bleu_1", "bleu_2", "bleu_3", "bleu_4", "meteor", "rouge", "cider"]
    assert list(df.columns) == ["dicom_id", "study_id", "bleu_1", "bleu_2", "bleu_3", "bleu_4", "meteor", "rouge", "cider"]
    assert list(seen["gts"]) == rec["key"] == list(seen["res"])
    assert [v[0] for v in seen["res"].values()] == rec["prediction"] and [v[0] for v in seen["gts"].values()] == rec["label"]
    per = np.array([len(p.split()) / (1.0 + len(l.split())) for p, l in zip(rec["prediction"], rec["label"])])
    np.testing.assert_allclose(df["meteor"].to_numpy(), per, rtol=1e-15)
    want = np.mean([per[rec["order"][rec["study_off"][s]:rec["study_off"][s + 1]]].mean() for s in range(len(rec["studies"]))])
    assert out["meteor"] == pytest.approx(want, rel=1e-13)
    base = dict(nref.load_fixture()["cases"]["b"]["result"])
    for k in ("bleu_4", "rouge"):
        assert out[k] == pytest.approx(base[k], rel=1e-12)
