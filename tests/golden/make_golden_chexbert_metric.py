#!/usr/bin/env python3
"""Generate tests/golden/chexbert_metric.json: what the reference's `CheXbertClassificationMetrics` (tools/metrics/chexbert.py) returns and writes
for given label tables (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chexbert_metric.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chexbert_metric.py --verify   # rebuild into a scratch directory, require identical bytes

The reference class is imported from /root/reference and run as it is (pandas does the arithmetic), with two stand-ins put into `sys.modules`
before the import:
  torchmetrics.Metric   `add_state` and `.device` only (torchmetrics is not installed here; the class uses nothing else of it)
  tools.chexbert        a table look-up `CheXbert`: report string -> 14 fixed class indices, `.to()` returns itself. The metric is arithmetic on
                        the labeller's output; the labeller itself is pinned elsewhere (tests/test_reward_scst_gpu.py).
Stored per case: the look-up table, the `update` calls, the returned dict as [key, value] pairs in the reference's key order (NaN as null) and the
four CSVs the reference wrote (header + rows, as pandas.read_csv returns them; NaN as null).

Cases:
  a  37 studies, no accumulation, study ids descending, 3 repeated records of the DDP kind (one of them with another prediction: the first stays)
  b  the same studies with accumulation: 1-3 DICOMs per study, repeated DICOMs, studies arriving unsorted
  c  no positive anywhere (classes 0, 2, 3 only): the three micro ratios are NaN
  d  pathologies without a positive on either side, classes 2 and 3 present
  e  a single study with a single record
"""
import glob
import json
import math
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FILE = "chexbert_metric.json"
N_PATH = 14


# ------------------------------------------------------------------------------------------------ stand-ins, then the reference class
class _Metric:
    def __init__(self, *args, **kwargs):
        self.device = "cpu"
        self._defaults = {}

    def add_state(self, name, default, **kwargs):
        self._defaults[name] = default
        setattr(self, name, list(default))


_TABLE = {}


class _LookupCheXbert:
    def __init__(self, **kwargs):
        pass

    def to(self, device):
        return self

    def __call__(self, reports):
        import torch
        return torch.tensor([_TABLE[r] for r in reports], dtype=torch.int64)


def reference_class():
    tm = types.ModuleType("torchmetrics")
    tm.Metric = _Metric
    cb = types.ModuleType("tools.chexbert")
    cb.CheXbert = _LookupCheXbert
    sys.modules["torchmetrics"] = tm
    sys.modules["tools.chexbert"] = cb
    sys.path.insert(0, "/root/reference")
    from tools.metrics.chexbert import PATHOLOGIES, CheXbertClassificationMetrics
    return CheXbertClassificationMetrics, PATHOLOGIES


# ------------------------------------------------------------------------------------------------ cases
def draw_table(rng, names, classes, p):
    """names -> 14 class indices drawn from `classes` with probabilities `p`; the last head (no finding) has two classes"""
    table = {}
    for n in names:
        row = rng.choice(classes, size=N_PATH, p=p).tolist()
        row[-1] = int(row[-1] == 1)
        table[n] = [int(v) for v in row]
    return table


def case_a(rng):
    studies = list(range(5037, 5000, -1))                              # 37 ids, descending
    preds = [f"prediction of study {s}" for s in studies]
    labels = [f"label text {i % 23}" for i in range(len(studies))]     # label texts shared between studies
    table = draw_table(rng, preds + sorted(set(labels)) + ["another prediction"], [0, 1, 2, 3], [0.4, 0.35, 0.15, 0.1])
    calls, lo = [], 0
    for n in (16, 16, 5):
        calls.append({"predictions": preds[lo:lo + n], "labels": [[t] for t in labels[lo:lo + n]], "study_ids": studies[lo:lo + n]})
        lo += n
    # the padding of the last DDP batch: records of studies already seen; the second carries another prediction, which must not count
    calls.append({"predictions": [preds[0], "another prediction", preds[2]], "labels": [[labels[0]], [labels[1]], [labels[2]]],
                  "study_ids": [studies[0], studies[1], studies[2]]})
    return {"accumulate_over_dicoms": False, "mbatch_size": 8, "table": table, "calls": calls}


def case_b(rng):
    studies = list(range(5037, 5000, -1))
    order = rng.permutation(len(studies)).tolist()                     # studies arrive unsorted: groupby sorts them
    preds, labels, sids, dids = [], [], [], []
    for k in order:
        for d in range(1 + k % 3):
            preds.append(f"prediction of study {studies[k]} image {d}")
            labels.append(f"label text {k % 23}")
            sids.append(studies[k])
            dids.append(f"dicom-{studies[k]}-{d}")
    table = draw_table(rng, preds + sorted(set(labels)) + ["another prediction"], [0, 1, 2, 3], [0.4, 0.35, 0.15, 0.1])
    calls = []
    for lo in range(0, len(preds), 16):
        calls.append({"predictions": preds[lo:lo + 16], "labels": [[t] for t in labels[lo:lo + 16]], "study_ids": sids[lo:lo + 16],
                      "dicom_ids": dids[lo:lo + 16]})
    calls.append({"predictions": [preds[5], "another prediction", preds[0]], "labels": [[labels[5]], [labels[9]], [labels[0]]],
                  "study_ids": [sids[5], sids[9], sids[0]], "dicom_ids": [dids[5], dids[9], dids[0]]})
    return {"accumulate_over_dicoms": True, "mbatch_size": 8, "table": table, "calls": calls}


def case_c(rng):
    studies = list(range(11, 20))
    preds = [f"negative prediction {s}" for s in studies]
    labels = [f"negative label {s % 4}" for s in studies]
    table = draw_table(rng, preds + sorted(set(labels)), [0, 2, 3], [0.5, 0.3, 0.2])
    return {"accumulate_over_dicoms": False, "mbatch_size": 4, "table": table,
            "calls": [{"predictions": preds, "labels": [[t] for t in labels], "study_ids": studies}]}


def case_d(rng):
    studies = [f"s{n:03d}" for n in range(21)]                         # string ids
    preds, labels, sids, dids = [], [], [], []
    for k, s in enumerate(studies):
        for d in range(1 + (k * 7) % 3):
            preds.append(f"sparse prediction {s} {d}")
            labels.append(f"sparse label {k % 9}")
            sids.append(s)
            dids.append(f"{s}_{d}")
    table = draw_table(rng, preds + sorted(set(labels)), [0, 1, 2, 3], [0.3, 0.3, 0.25, 0.15])
    for row in table.values():                                         # pathologies 3, 10, 11: never positive, on either side
        for j in (3, 10, 11):
            row[j] = 2 if row[j] == 1 else row[j]
    for n in preds:                                                    # pathology 6: positive in labels only (precision 0 / 0 -> 0)
        table[n][6] = 3 if table[n][6] == 1 else table[n][6]
    return {"accumulate_over_dicoms": True, "mbatch_size": 5, "table": table,
            "calls": [{"predictions": preds, "labels": [[t] for t in labels], "study_ids": sids, "dicom_ids": dids}]}


def case_e(rng):
    table = draw_table(rng, ["the only prediction", "the only label"], [0, 1, 2, 3], [0.25, 0.5, 0.15, 0.1])
    return {"accumulate_over_dicoms": False, "mbatch_size": 1, "table": table,
            "calls": [{"predictions": ["the only prediction"], "labels": [["the only label"]], "study_ids": [77]}]}


CASES = (("a", case_a, 11), ("b", case_b, 12), ("c", case_c, 13), ("d", case_d, 14), ("e", case_e, 15))


# ------------------------------------------------------------------------------------------------ run and record
def _clean(v):
    if isinstance(v, (float, np.floating)):
        return None if math.isnan(v) else float(v)
    if isinstance(v, (np.integer,)):
        return int(v)
    return v


def run_case(cls, case, work):
    import pandas as pd
    _TABLE.clear()
    _TABLE.update(case["table"])
    exp_dir = os.path.join(work, "exp")
    metric = cls("test", None, None, None, case["mbatch_size"], exp_dir, case["accumulate_over_dicoms"])
    for c in case["calls"]:
        metric.update(c["predictions"], c["labels"], c["study_ids"], c.get("dicom_ids"))
    out = metric.compute(epoch=7)
    csvs = {}
    for kind in ("y_hat", "y", "class_scores", "example_scores"):
        files = glob.glob(os.path.join(exp_dir, "chexbert_outputs", f"test_epoch-7_{kind}_[0-9]*.csv"))
        assert len(files) == 1, (kind, files)
        df = pd.read_csv(files[0])
        csvs[kind] = {"columns": list(df.columns), "rows": [[_clean(v) for v in row] for row in df.itertuples(index=False, name=None)]}
    shutil.rmtree(exp_dir)
    return {"result": [[k, _clean(v)] for k, v in out.items()], "csv": csvs}


def make(out_dir):
    cls, pathologies = reference_class()
    doc = {"pathologies": list(pathologies), "cases": {}}
    work = tempfile.mkdtemp(prefix="golden_chexbert_metric_")
    try:
        for name, build, seed in CASES:
            case = build(np.random.default_rng(seed))
            case.update(run_case(cls, case, work))
            doc["cases"][name] = case
            res = dict(case["result"])
            print(f"{name}: {len(case['result'])} keys, {int(res['num_study_ids'])} studies, f1 example / macro / micro = "
                  f"{res['f1_example']} / {res['f1_macro']} / {res['f1_micro']}")
    finally:
        shutil.rmtree(work)
    c = dict(doc["cases"]["c"]["result"])
    assert c["accuracy_example"] == 1.0 and c["accuracy_macro"] == 1.0 and c["f1_example"] == 0.0 and c["f1_macro"] == 0.0
    assert c["precision_micro"] is None and c["recall_micro"] is None and c["f1_micro"] is None
    assert [len(doc["cases"][k]["result"]) for k in "abcde"] == [69, 70, 69, 70, 69]
    path = os.path.join(out_dir, FILE)
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB")


def verify():
    tmp = tempfile.mkdtemp(prefix="golden_chexbert_metric_verify_")
    try:
        make(tmp)
        with open(os.path.join(tmp, FILE), "rb") as f, open(os.path.join(HERE, FILE), "rb") as g:
            assert f.read() == g.read(), "the regenerated fixture differs from the committed one"
        print("verify ok: identical bytes")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    if "--verify" in sys.argv[1:]:
        verify()
    else:
        make(HERE)
