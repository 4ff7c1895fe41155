"""CPU: the COCO NLG metric's surface that needs no GPU -- the C ABI declaration, the wrapper refusing host tensors, the merge / de-duplication /
grouping step, the staging of texts as word ids, the metric's argument checks and the error paths of `tokenizer=` / `extra_scorers=` (reference
tools/metrics/coco.py), and the tests' own float64 restatement: against the fixture recorded from the reference class, and -- because that fixture
does not pin the scorers' numbers -- against closed forms derived by hand below."""
import ctypes
import math

import numpy as np
import pytest
import torch

import coco_nlg_ref as nref
from cxrmate_amd import metrics, ops
from cxrmate_amd._lib import CxrError, parse_header

CASES = list("abcdefgh")


def test_header_declares_the_entry_point():
    protos = parse_header()
    v, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    want = [("ids_a", v), ("n_ids_a", L), ("off_a", v), ("ids_b", v), ("n_ids_b", L), ("off_b", v), ("n_texts", I), ("pairs", v), ("ref_mult", v),
            ("M", I), ("order", v), ("study_off", v), ("S", I), ("scores", v), ("ints", v), ("study", v), ("avg", v), ("workspace", v),
            ("workspace_bytes", L), ("stream", v)]
    assert "cxr_coco_nlg_scores" in protos
    assert [(n, t) for t, n in protos["cxr_coco_nlg_scores"]] == want
    assert [n for n in protos if "coco" in n or "nlg" in n] == ["cxr_coco_nlg_scores"]            # exactly one entry point was added


def test_wrapper_refuses_host_tensors():
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    with pytest.raises(CxrError):
        ops.coco_nlg_scores(i32(0, 1), i32(0, 1, 2), i32(0, 1), i32(0, 1, 2), i32(0, 1).reshape(1, 2), i32(0, 1), i32(0), i32(0, 1))


def test_workspace_formula():
    assert ops.coco_nlg_workspace_bytes(0, 0) == 1024 * 12
    assert ops.coco_nlg_workspace_bytes(513, 3) == 2048 * 12 + 3 * 2056 + 96                       # 2 * 513 > 1024; 513 * 4 rounded up to 8
    assert ops.COCO_NLG_MAX_LEN == 8192


# ------------------------------------------------------------------------------------------------ merge, staging
def _parts():
    """Two hand-made rank parts. Rank 0: studies 30, 10, 30 (DICOMs a, b, c); rank 1: studies 20, 10, 30 (DICOMs d, b again, e). The repeated
    DICOM b carries other texts on rank 1: those are the ones scored, in b's first row."""
    p0 = {"prediction": ["p0", "p1", "p2"], "label": ["l0", "l1", "l0"], "study_id": [30, 10, 30], "dicom_id": ["a", "b", "c"]}
    p1 = {"prediction": ["p3", "p4", "p5"], "label": ["l2", "l3", "l2"], "study_id": [20, 10, 30], "dicom_id": ["d", "b", "e"]}
    return [p0, p1]


def test_merge_last_record_wins_at_the_first_position():
    m = metrics.merge_report_parts(_parts(), True)
    assert m["dicom_id"] == ["a", "b", "c", "d", "e"] and m["study_id"] == [30, 10, 30, 20, 30]
    assert m["prediction"] == ["p0", "p4", "p2", "p3", "p5"] and m["label"] == ["l0", "l3", "l0", "l2", "l2"]
    assert m["studies"] == [10, 20, 30]                                                        # pandas groupby: sorted by id
    assert m["order"].tolist() == [1, 3, 0, 2, 4]                                              # appearance order inside a study
    assert m["study_off"].tolist() == [0, 1, 2, 5] and m["study_off"].dtype == np.int32


def test_merge_one_row_per_study():
    parts = [{k: v for k, v in p.items() if k != "dicom_id"} for p in _parts()]
    m = metrics.merge_report_parts(parts, False)
    assert m["study_id"] == [30, 10, 20] and m["studies"] == [30, 10, 20] and m["dicom_id"] is None
    assert m["prediction"] == ["p5", "p4", "p3"] and m["label"] == ["l2", "l3", "l2"]         # the last record of studies 30 and 10
    assert m["order"].tolist() == [0, 1, 2] and m["study_off"].tolist() == [0, 1, 2, 3]
    ids = [torch.tensor(30), np.int64(10)]                                                    # tensor / numpy ids are unwrapped, as the reference
    one = metrics.merge_report_parts([{"prediction": ["x", "y"], "label": ["u", "v"], "study_id": ids}], False)
    assert one["studies"] == [30, 10] and all(type(s) is int for s in one["studies"])
    empty = metrics.merge_report_parts([{"prediction": [], "label": [], "study_id": []}], False)
    assert empty["prediction"] == [] and empty["study_off"].tolist() == [0] and len(empty["order"]) == 0


def test_staging_distinct_texts_and_both_token_streams():
    st = metrics.stage_texts(["a b ", "c\td", "a b "], ["x", "x", "a b"])
    # distinct texts in order of appearance: "a b " (0), "x" (1), "c\td" (2), "a b" (3)
    assert st["pairs"].tolist() == [[0, 1], [2, 1], [0, 3]] and st["ref_mult"].tolist() == [0, 2, 0, 1]
    assert st["off_a"].tolist() == [0, 2, 3, 5, 7] and st["off_b"].tolist() == [0, 3, 4, 5, 7]   # split(" "): "a b " has 3 tokens, the tab does not split
    a, b = st["ids_a"].tolist(), st["ids_b"].tolist()
    assert a[0:2] == a[5:7] and b[0:2] == b[5:7] == a[0:2]                                   # one dict over both streams: same word, same id
    assert b[2] not in a and b[4] not in a                                                    # the empty token and "c\td" exist for ROUGE only
    assert all(v.dtype == np.int32 for v in st.values())
    ref = nref.stage(["a b ", "c\td", "a b "], ["x", "x", "a b"])
    for k in ("off_a", "off_b", "pairs", "ref_mult"):
        assert np.array_equal(st[k], ref[k])


# ------------------------------------------------------------------------------------------------ the class without a GPU
def test_metric_argument_checks(tmp_path):
    m = metrics.COCONLGMetricsMIMICCXR("test", str(tmp_path / "exp"), True, use_tokenizer=False)
    assert (tmp_path / "exp" / "nlg_scores").is_dir() and m.metrics == ["bleu", "cider", "rouge"]
    assert m.columns() == ["bleu_1", "bleu_2", "bleu_3", "bleu_4", "rouge", "cider"]
    with pytest.raises(AssertionError, match='"predictions" must be a list of strings.'):
        m.update("not a list", [["a"]], [1], ["x"])
    with pytest.raises(AssertionError, match='Each element of "predictions" must be a string.'):
        m.update([1], [["a"]], [1], ["x"])
    with pytest.raises(AssertionError, match='"labels" must be a list of lists'):
        m.update(["a"], "not a list", [1], ["x"])
    with pytest.raises(AssertionError, match='Each element of "labels" must be a list of strings.'):
        m.update(["a"], ["not a list of lists"], [1], ["x"])
    with pytest.raises(AssertionError, match="each sub-list must have one or more strings."):
        m.update(["a"], [[3]], [1], ["x"])
    m.update(["a", "b"], [["c"], ["d"]], [1, 2], ["x", "y"])
    assert m.reports == [{"prediction": "a", "label": ["c"], "study_id": 1, "dicom_id": "x"},
                         {"prediction": "b", "label": ["d"], "study_id": 2, "dicom_id": "y"}]
    m.reset()
    assert m.reports == []
    m.update(["a"], [["c", "d"]], [1], ["x"])                                                 # two references: refused in compute, as the siblings do
    with pytest.raises(AssertionError):
        m.compute(0)
    m2 = metrics.COCONLGMetricsMIMICCXR("val", str(tmp_path / "exp"), False, ["ROUGE", "Cider"], False)      # the reference's positional order
    assert m2.metrics == ["rouge", "cider"] and m2.columns() == ["rouge", "cider"] and m2.use_tokenizer is False
    m2.update(["a"], [["c"]], [5])
    assert m2.reports == [{"prediction": "a", "label": ["c"], "study_id": 5}]


def test_tokenizer_and_extra_scorer_error_paths(tmp_path):
    exp = str(tmp_path / "exp")
    m = metrics.COCONLGMetricsMIMICCXR("test", exp, False)                                    # use_tokenizer defaults to True, as the reference
    m.update(["a"], [["a"]], [1])
    with pytest.raises(RuntimeError, match="needs tokenizer="):
        m.compute(0)
    for name in ("meteor", "spice"):
        with pytest.raises(ValueError, match=f"'{name}' is a Java scorer"):
            metrics.COCONLGMetricsMIMICCXR("test", exp, False, ["bleu", name], False)
        with pytest.raises(ValueError, match=f"'{name}' is a Java scorer"):
            metrics.COCONLGMetricsMIMICCXR("test", exp, False, ["bleu", name], False, extra_scorers={name: object()})
    with pytest.raises(ValueError, match="unknown COCO NLG metrics"):
        metrics.COCONLGMetricsMIMICCXR("test", exp, False, ["bleu", "wer"], False)

    class Stub:
        def compute_score(self, gts, res):
            return 0.0, [0.0] * len(gts)
    ok = metrics.COCONLGMetricsMIMICCXR("test", exp, False, ["Meteor", "bleu", "spice"], False, extra_scorers={"meteor": Stub(), "spice": Stub()})
    assert ok.columns() == ["bleu_1", "bleu_2", "bleu_3", "bleu_4", "meteor", "spice"]
    ok.update(["a"], [["a"]], [1])
    ok.device = torch.device("cpu")
    with pytest.raises(CxrError):                                                              # host tensors: refused, there is no fallback
        ok.compute(0)


# ------------------------------------------------------------------------------------------------ restatement against the recorded reference
@pytest.mark.parametrize("name", CASES)
def test_restatement_and_merge_reproduce_the_recorded_reference(name):
    """`merge_report_parts` + the restatement + plain means give the dict and the CSV the reference class returned and wrote (the scorers inside
    the reference run were the restatement's: this pins the de-duplication rule, the row order, the ids and both levels of means)."""
    case = nref.load_fixture()["cases"][name]
    acc = case["accumulate_over_dicoms"]
    part = {"prediction": [], "label": [], "study_id": [], "dicom_id": []}
    for c in case["calls"]:
        part["prediction"] += c["predictions"]
        part["label"] += [g[0] for g in c["labels"]]
        part["study_id"] += c["study_ids"]
        part["dicom_id"] += c.get("dicom_ids", [])
    half = len(part["prediction"]) // 2                                                       # as two ranks
    parts = [{k: v[:half] for k, v in part.items()}, {k: v[half:] for k, v in part.items()}]
    m = metrics.merge_report_parts(parts, acc)
    rec = nref.case_records(case)
    import re
    assert [re.sub(" +", " ", t) for t in m["prediction"]] == rec["prediction"] and [re.sub(" +", " ", t) for t in m["label"]] == rec["label"]
    assert m["study_id"] == rec["study_id"] and m["studies"] == rec["studies"]
    assert m["order"].tolist() == rec["order"].tolist() and m["study_off"].tolist() == rec["study_off"].tolist()
    cols, rows = case["csv"]["columns"], case["csv"]["rows"]
    assert cols[:2 if acc else 1] == (["dicom_id", "study_id"] if acc else ["study_id"])
    assert [r[cols.index("study_id")] for r in rows] == m["study_id"]
    if acc:
        assert [r[0] for r in rows] == m["dicom_id"]
    st = nref.stage(rec["prediction"], rec["label"])
    scores, _ = nref.scores_arrays(st["ids_a"], st["off_a"], st["ids_b"], st["off_b"], st["pairs"])
    _, avg = nref.study_means(scores, rec["order"], rec["study_off"])
    want_scores, want_avg = nref.case_expected(case)
    asked = ~np.isnan(want_avg)
    M = len(rows)
    nref.assert_scores_close(np.where(asked, scores, 0.0), np.where(asked, want_scores, 0.0), M, f"{name} rows")
    nref.assert_scores_close(np.where(asked, avg, 0.0), np.where(asked, want_avg, 0.0), M, f"{name} means")
    res = dict(case["result"])
    assert res["num_study_ids"] == float(len(m["studies"])) and (not acc or res["num_dicom_ids"] == float(len(set(m["dicom_id"]))))


# ------------------------------------------------------------------------------------------------ restatement against closed forms
def _one(hyp, ref, others=()):
    """scores of record 0 among the records [(hyp, ref), *others] -> (bleu [4], c [4], rouge, lcs, cider)"""
    pairs = [(hyp, ref), *others]
    bleu, c = nref.bleu_pair(hyp.split(), ref.split())
    rouge, length = nref.rouge_pair(hyp.split(" "), ref.split(" "))
    cider = nref.cider_scores([h.split() for h, _ in pairs], [r.split() for _, r in pairs])[0]
    return bleu, c, rouge, length, cider


def test_closed_form_identical_texts():
    """Five distinct words on both sides: c_k = g_k = 6 - k, so the running product is prod_{j<=k} (6 - j + 1e-15) / (6 - j + 1e-9). The lengths
    are equal, yet ratio = (5 + 1e-15) / (5 + 1e-9) is below 1 by 2e-10 (the two constants differ), so the library's brevity penalty
    exp(1 - 1 / ratio) applies as well: BLEU of identical texts is 1 - 2e-10, not 1. ROUGE: lcs = 5, p = r = 1, score (1 + b2) / (1 + b2) = 1.
    CIDEr with a second record that shares no word: M = 2, every n-gram of record 0 has df = 1, w = log 2, the two vectors are equal, every
    val_n = sum v^2 / (norm * norm) = 1 up to rounding, delta = 0: the score is 10."""
    t = "the heart is normal ."
    bleu, c, rouge, length, cider = _one(t, t, [("lungs are clear", "no effusion seen")])
    assert c == [5, 4, 3, 2] and length == 5
    bp = math.exp(1 - (5 + 1e-9) / (5 + 1e-15))
    prod = 1.0
    for k in range(1, 5):
        prod *= (6 - k + 1e-15) / (6 - k + 1e-9)
        assert bleu[k - 1] == pytest.approx(prod ** (1.0 / k) * bp, rel=1e-15, abs=0)
        assert 0 < 1 - bleu[k - 1] < 1e-9
    assert rouge == 1.0
    assert cider == pytest.approx(10.0, rel=1e-14, abs=0)


def test_closed_form_nothing_shared():
    """No common word: every c_k = 0, lcs = 0 -> ROUGE exactly 0.0; every min(v_hyp, v_ref) * v_ref has v_ref = 0 -> CIDEr exactly 0.0. BLEU is
    not exactly 0 in the library: the product carries (0 + 1e-15) / (g_k + 1e-9), about 2e-16 at k = 1, far below any score that matters."""
    bleu, c, rouge, length, cider = _one("a b c d e", "v w x y z", [("p q", "p q")])
    assert c == [0, 0, 0, 0] and length == 0 and rouge == 0.0 and cider == 0.0
    bp = math.exp(1 - (5 + 1e-9) / (5 + 1e-15))
    prod = 1.0
    for k in range(1, 5):
        prod *= 1e-15 / (6 - k + 1e-9)
        assert bleu[k - 1] == pytest.approx(prod ** (1.0 / k) * bp, rel=1e-15, abs=0) and bleu[k - 1] < 1e-15
    empty, c0 = nref.bleu_pair([], "v w x".split())                                            # an empty hypothesis: exp(1 - 3e15) underflows to 0
    assert empty == [0.0] * 4 and c0 == [0] * 4


def test_closed_form_strict_prefix():
    """Hypothesis = the first 3 of the reference's 6 distinct words: c = g = (3, 2, 1, 0); ratio = (3 + 1e-15) / (6 + 1e-9), so every order is
    multiplied by exp(1 - 1 / ratio) ~ exp(-1). lcs = 3: p = 1, r = 1/2, ROUGE = (1 + b2) / 2 / (1/2 + b2) with b2 = 1.44."""
    bleu, c, rouge, length, _ = _one("a b c", "a b c d e f")
    assert c == [3, 2, 1, 0] and length == 3
    ratio = (3 + 1e-15) / (6 + 1e-9)
    bp = math.exp(1 - 1 / ratio)
    assert bp == pytest.approx(math.exp(-1.0), rel=1e-9)
    prod = 1.0
    for k, (ck, gk) in enumerate(((3, 3), (2, 2), (1, 1), (0, 0)), 1):
        prod *= (ck + 1e-15) / (gk + 1e-9)
        assert bleu[k - 1] == pytest.approx(prod ** (1.0 / k) * bp, rel=1e-15, abs=0)
    assert bleu[0] == pytest.approx(math.exp(-1.0), rel=1e-9)
    assert rouge == pytest.approx(2.44 * 0.5 / (0.5 + 1.44), rel=1e-15)


def test_lcs_classic_pairs_and_tokenisation():
    assert nref.lcs(list("ABCBDAB"), list("BDCABA")) == 4
    assert nref.lcs(list("AGGTAB"), list("GXTXAYB")) == 4
    assert nref.lcs(list("abc"), []) == 0 and nref.lcs(list("abc"), list("xyz")) == 0
    # ROUGE splits on single blanks: a trailing blank is an empty token (precision 2/3), which BLEU's split() never sees
    r1, l1 = nref.rouge_pair("a b ".split(" "), "a b".split(" "))
    assert l1 == 2 and r1 == pytest.approx(2.44 * (2 / 3) / (1 + 1.44 * 2 / 3), rel=1e-15)
    assert nref.bleu_pair("a b ".split(), "a b".split()) == nref.bleu_pair("a b".split(), "a b".split())


def test_restatement_classes_have_the_library_signatures():
    gts, res = {1: ["a b c d"], 2: ["x y"]}, {1: ["a b c"], 2: ["x y"]}
    corpus, per = nref.Bleu(4).compute_score(gts, res)
    assert len(corpus) == 4 and [len(p) for p in per] == [2, 2, 2, 2]
    mean, per = nref.Rouge().compute_score(gts, res)
    assert per.shape == (2,) and per[1] == 1.0 and mean == pytest.approx(per.mean())
    mean, per = nref.Cider().compute_score(gts, res)
    assert per.shape == (2,) and per[1] == pytest.approx(5.0, rel=1e-14)                      # two words: orders 3 and 4 have no n-gram, val = 0
