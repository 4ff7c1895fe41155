"""CPU: the CheXbert classification metric's surface that needs no GPU -- the C ABI declaration, the wrapper refusing host tensors, the merge /
de-duplication / grouping step, the metric's argument checks (reference tools/metrics/chexbert.py), and the tests' own float64 restatement
against the numbers recorded from the reference."""
import ctypes

import numpy as np
import pytest
import torch

import chexbert_metric_ref as cref
from cxrmate_amd import metrics, ops
from cxrmate_amd._lib import CxrError, parse_header


def test_header_declares_the_entry_point():
    protos = parse_header()
    v, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    want = [("pred", v), ("n_pred", I), ("ref", v), ("n_ref", I), ("pred_row", v), ("ref_row", v), ("M", I), ("study_off", v), ("S", I),
            ("example", v), ("cls", v), ("avg", v), ("workspace", v), ("workspace_bytes", L), ("stream", v)]
    assert "cxr_chexbert_scores" in protos
    assert [(n, t) for t, n in protos["cxr_chexbert_scores"]] == want
    assert len([n for n in protos if "chexbert" in n]) == 1                      # one entry point


def test_wrapper_refuses_host_tensors():
    t = torch.zeros(2, 14, dtype=torch.int64)
    rows = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(CxrError):
        ops.chexbert_scores(t, t, rows, rows, torch.tensor([0, 1, 2], dtype=torch.int32))


def test_pathologies_in_head_order():
    assert metrics.PATHOLOGIES == ["enlarged_cardiomediastinum", "cardiomegaly", "lung_opacity", "lung_lesion", "edema", "consolidation", "pneumonia",
                                   "atelectasis", "pneumothorax", "pleural_effusion", "pleural_other", "fracture", "support_devices", "no_finding"]
    assert metrics.PATHOLOGIES == cref.load_fixture()["pathologies"]


def _parts():
    """Two hand-made rank parts. Rank 0: studies 30, 10, 30 (DICOMs a, b, c); rank 1: studies 20, 10, 30 (DICOMs d, b again, e). The repeated
    DICOM b carries other labels on rank 1, which must not count."""
    def rows(*first):
        return np.array([[f] + [0] * 13 for f in first], dtype=np.int64)
    p0 = {"pred": rows(1, 2, 3), "ref": rows(1, 0), "ref_row": [0, 1, 0], "study_id": [30, 10, 30], "dicom_id": ["a", "b", "c"]}
    p1 = {"pred": rows(0, 1, 1), "ref": rows(3, 1), "ref_row": [1, 0, 1], "study_id": [20, 10, 30], "dicom_id": ["d", "b", "e"]}
    return [p0, p1]


def test_merge_grouped_by_study_sorted():
    m = metrics.merge_label_parts(_parts(), True)
    assert m["pred"][:, 0].tolist() == [1, 2, 3, 0, 1, 1] and m["ref"][:, 0].tolist() == [1, 0, 3, 1]
    assert m["pred_row"].tolist() == [0, 1, 2, 3, 5] and m["pred_row"].dtype == np.int32       # record 4 repeats DICOM b: the first occurrence wins
    assert m["ref_row"].tolist() == [0, 1, 0, 3, 3] and m["ref_row"].dtype == np.int32         # rank 1's rows follow rank 0's two
    assert m["dicom_id"] == ["a", "b", "c", "d", "e"] and m["study_id"] == [30, 10, 30, 20, 30]
    assert m["studies"] == [10, 20, 30]                                                        # pandas groupby: sorted by id
    assert m["order"].tolist() == [1, 3, 0, 2, 4]                                              # appearance order inside a study
    assert m["study_off"].tolist() == [0, 1, 2, 5] and m["study_off"].dtype == np.int32


def test_merge_one_row_per_study_first_appearance():
    parts = [{k: v for k, v in p.items() if k != "dicom_id"} for p in _parts()]
    m = metrics.merge_label_parts(parts, False)
    assert m["pred_row"].tolist() == [0, 1, 3] and m["ref_row"].tolist() == [0, 1, 3]           # studies 30, 10, 20: their first records
    assert m["studies"] == [30, 10, 20] and m["study_id"] == [30, 10, 20] and m["dicom_id"] is None
    assert m["order"].tolist() == [0, 1, 2] and m["study_off"].tolist() == [0, 1, 2, 3]
    one = metrics.merge_label_parts(parts[:1], False)
    assert one["studies"] == [30, 10] and one["pred_row"].tolist() == [0, 1] and one["study_off"].tolist() == [0, 1, 2]


def test_metric_argument_checks(tmp_path):
    m = metrics.CheXbertClassificationMetrics("test", str(tmp_path), str(tmp_path), "chexbert.pth", 4, str(tmp_path / "exp"), True)
    assert (tmp_path / "exp" / "chexbert_outputs").is_dir()
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
    assert list(m.mini_batch([1, 2, 3], 2)) == [[1, 2], [3]]
    with pytest.raises(ValueError, match="The CheXbert checkpoint does not exist"):           # no labeller given: built from the checkpoint, as the reference
        m.compute(0)
    m.reset()
    assert m.reports == []
    m2 = metrics.CheXbertClassificationMetrics("val", None, None, None, 2, str(tmp_path / "exp"), False)
    m2.update(["a"], [["c"]], [5])
    assert m2.reports == [{"prediction": "a", "label": ["c"], "study_id": 5}]


@pytest.mark.parametrize("name", list("abcde"))
def test_restatement_matches_the_recorded_reference(name):
    """The float64 restatement the GPU tests compare the kernel with on large inputs reproduces what the reference returned and wrote."""
    fx = cref.load_fixture()
    case = fx["cases"][name]
    example, cls, avg = cref.scores(*cref.case_tables(case, fx["pathologies"]))
    res = case["result"]
    assert [k for k, _ in res[:12]] == [f"{r}_{a}" for a in ("example", "macro", "micro") for r in cref.RATIOS]
    cref.assert_close(avg, cref.nan_array([v for _, v in res[:12]]), f"{name} avg")
    assert [k for k, _ in res[12:68]] == [f"{r}_{p}" for r in cref.RATIOS for p in fx["pathologies"]]
    cref.assert_close(cls[:, 4:].T.reshape(-1), cref.nan_array([v for _, v in res[12:68]]), f"{name} cls")
    ex = case["csv"]["example_scores"]
    assert ex["columns"] == ["study_id", "tp", "tn", "fp", "fn", "accuracy", "precision", "recall", "f1"]
    cref.assert_close(example, np.array([cref.nan_array(r[1:]) for r in ex["rows"]]), f"{name} example")
    assert len(res) == (70 if case["accumulate_over_dicoms"] else 69) and res[68] == ["num_study_ids", float(len(ex["rows"]))]
