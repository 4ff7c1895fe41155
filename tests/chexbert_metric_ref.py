"""float64 numpy restatement of the CheXbert classification scores (reference tools/metrics/chexbert.py:191-336) for the metric tests, and the
table look-up labeller the fixture's cases are replayed through."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATIOS = ("accuracy", "precision", "recall", "f1")


def load_fixture():
    with open(os.path.join(GOLDEN, "chexbert_metric.json")) as f:
        return json.load(f)


def nan_array(values):
    return np.array([np.nan if v is None else v for v in values], dtype=np.float64)


def _fill0(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.asarray(num, dtype=np.float64) / np.asarray(den, dtype=np.float64)
    return np.where(np.isnan(q), 0.0, q)


def _ratios(tp, tn, fp, fn):
    return [_fill0(tp + tn, tp + tn + fp + fn), _fill0(tp, tp + fp), _fill0(tp, tp + fn), _fill0(tp, tp + 0.5 * (fp + fn))]


def scores(pred, ref, pred_row, ref_row, study_off):
    """-> example [S, 8], cls [14, 8], avg [12] in float64: positive = class 1, each error type of a study = mean over its records, zero-denominator
    ratios 0 in example / cls, the micro ratios plain divisions (NaN for 0 / 0)."""
    p = np.asarray(pred)[np.asarray(pred_row)] == 1
    y = np.asarray(ref)[np.asarray(ref_row)] == 1
    off = np.asarray(study_off, dtype=np.int64)
    S = len(off) - 1
    err = np.stack([p & y, ~p & ~y, p & ~y, ~p & y]).astype(np.float64)                  # [4, M, 14]
    per = np.stack([err[:, off[s]:off[s + 1]].mean(1) for s in range(S)], 1)                # [4, S, 14]
    et = per.sum(2)                                                                         # [4, S]
    example = np.stack(list(et) + _ratios(*et), 1)
    ct = per.sum(1)                                                                         # [4, 14]
    cls = np.stack(list(ct) + _ratios(*ct), 1)
    tp, tn, fp, fn = ct.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        micro = [np.float64(tp + tn) / (tp + tn + fp + fn), np.float64(tp) / (tp + fp), np.float64(tp) / (tp + fn),
                 np.float64(tp) / (tp + 0.5 * (fp + fn))]
    avg = np.concatenate([example[:, 4:].mean(0), cls[:, 4:].mean(0), micro])
    return example, cls, avg


def assert_close(got, want, what):
    """rtol 1e-12 / atol 1e-9 with the NaN positions coinciding exactly. Both sides are float64 sums of at most a few thousand terms no larger than
    14 in which only the order differs: the relative error of such a sum is bounded by n * 2^-53 ~ 1e-12 for n ~ 1e4."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    both = np.isnan(want)
    np.testing.assert_allclose(np.where(both, 0.0, got), np.where(both, 0.0, want), rtol=1e-12, atol=1e-9, err_msg=what)


class LookupLabeller:
    """report string -> its 14 class indices from a table, as a device tensor (the stand-in the fixture was recorded with)."""

    def __init__(self, table, device):
        import torch
        self.table, self.device, self.calls = table, torch.device(device), []

    def label_all(self, texts, mbatch_size):
        import torch
        self.calls.append(len(texts))
        return torch.tensor([self.table[t] for t in texts], dtype=torch.int64).reshape(-1, 14).to(self.device)


def case_tables(case, pathologies):
    """The kernel's inputs for a recorded case, built from the reference's own y_hat / y CSV rows and its example CSV's study order: one table row
    per kept record on the prediction side, one per distinct label row on the label side."""
    acc = case["accumulate_over_dicoms"]
    yh, y, ex = case["csv"]["y_hat"], case["csv"]["y"], case["csv"]["example_scores"]
    ns = 2 if acc else 1
    assert yh["columns"] == (["dicom_id", "study_id"] if acc else ["study_id"]) + pathologies and y["columns"] == yh["columns"]
    study_col = yh["columns"].index("study_id")
    pred = np.array([r[ns:] for r in yh["rows"]], dtype=np.int64)
    uniq, ref_row = {}, []
    for r in y["rows"]:
        ref_row.append(uniq.setdefault(tuple(r[ns:]), len(uniq)))
    ref = np.array(list(uniq), dtype=np.int64)
    studies = [r[0] for r in ex["rows"]]
    rank = {s: i for i, s in enumerate(studies)}
    group = np.array([rank[r[study_col]] for r in yh["rows"]])
    order = np.argsort(group, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=len(studies)))]).astype(np.int32)
    return pred, ref, order.astype(np.int32), np.asarray(ref_row, dtype=np.int32)[order], off
