#!/usr/bin/env python3
"""Generate tests/golden/coco_nlg.json: what the reference's `COCONLGMetricsMIMICCXR` (tools/metrics/coco.py) returns and writes for given reports
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_coco_nlg.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_coco_nlg.py --verify   # rebuild into a scratch directory, require identical bytes

The reference class is imported from /root/reference and run as it is, with `use_tokenizer=False` (pandas builds the table, drops the duplicate
rows, writes the CSV and takes the means), with stand-ins put into `sys.modules` before the import:
  torchmetrics.Metric                              `add_state` only (torchmetrics is not installed here; the class uses nothing else of it)
  pycocoevalcap.{bleu.bleu, rouge.rouge, cider.cider}   `Bleu`, `Rouge`, `Cider` of tests/coco_nlg_ref.py, the float64 restatement of the library
                                                   (pycocoevalcap is not installed here)
  pycocoevalcap.{meteor.meteor, spice.spice, tokenizer.ptbtokenizer}   classes that raise when constructed; no case constructs them

What the fixture pins FROM THE REFERENCE: which record's texts a repeated DICOM / study id keeps (the last) and where (the first's row, with the
first's ids), the order of the keys of the returned dict, the CSV's columns and row order, and the per-DICOM then per-study means.
What it does NOT pin: the scorers. The BLEU / ROUGE / CIDEr numbers in it are the restatement's own; tests/test_coco_nlg_abi.py checks the
restatement against closed forms derived by hand instead.

Stored per case: the constructor arguments, the `update` calls, the returned dict as [key, value] pairs in the reference's key order and the CSV the
reference wrote (header + rows, as pandas.read_csv returns them).

Cases:
  a  no accumulation: 23 studies with unsorted ids, label texts shared between studies, three repeated records of the DDP kind, one of them with
     a different prediction (the last one is scored, in the first one's row)
  b  accumulation: 1-3 DICOMs per study, studies arriving unsorted, a repeated DICOM with another prediction
  c  an empty prediction among ordinary ones
  d  texts with double blanks, a trailing blank, a leading blank and a tab
  e  predictions identical to their labels
  f  a single record (CIDEr 0: log 1 = 0)
  g  every label identical (every document frequency equals the number of records: all weights 0)
  h  bleu only, and cider + rouge given in another order and case: the columns follow the reference's order
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
FILE = "coco_nlg.json"
sys.path.insert(0, os.path.dirname(HERE))


# ------------------------------------------------------------------------------------------------ stand-ins, then the reference class
class _Metric:
    def __init__(self, *args, **kwargs):
        self._defaults = {}

    def add_state(self, name, default, **kwargs):
        self._defaults[name] = default
        setattr(self, name, list(default))


class _Never:
    def __init__(self, *args, **kwargs):
        raise RuntimeError("a Java component of pycocoevalcap: not available here, and no case uses it")


def reference_class():
    import coco_nlg_ref as nref
    tm = types.ModuleType("torchmetrics")
    tm.Metric = _Metric
    sys.modules["torchmetrics"] = tm
    for path, name, obj in (("bleu.bleu", "Bleu", nref.Bleu), ("rouge.rouge", "Rouge", nref.Rouge), ("cider.cider", "Cider", nref.Cider),
                            ("meteor.meteor", "Meteor", _Never), ("spice.spice", "Spice", _Never),
                            ("tokenizer.ptbtokenizer", "PTBTokenizer", _Never)):
        parts = ("pycocoevalcap." + path).split(".")
        for i in range(1, len(parts) + 1):
            sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
        setattr(sys.modules["pycocoevalcap." + path], name, obj)
    sys.path.insert(0, "/root/reference")
    from tools.metrics.coco import COCONLGMetricsMIMICCXR
    return COCONLGMetricsMIMICCXR


# ------------------------------------------------------------------------------------------------ cases
_FINDINGS = ("the heart is normal in size", "the lungs are clear", "there is no pleural effusion", "no pneumothorax is seen",
             "the mediastinal contours are unremarkable", "mild bibasilar atelectasis is present", "there is a small left pleural effusion",
             "the cardiac silhouette is mildly enlarged", "no acute osseous abnormality", "a right picc line ends in the lower svc",
             "there is no focal consolidation", "pulmonary vascular congestion has improved")


def _report(rng, lo=2, hi=6):
    return " . ".join(_FINDINGS[i] for i in rng.choice(len(_FINDINGS), size=int(rng.integers(lo, hi)), replace=False)) + " ."


def _noisy(rng, text):
    """a prediction near a label: some words dropped, some replaced"""
    extra = ("possible", "stable", "unchanged", "left", "right", "small", "moderate")
    out = []
    for w in text.split():
        u = rng.random()
        if u < 0.12:
            continue
        out.append(extra[int(rng.integers(len(extra)))] if u < 0.22 else w)
    return " ".join(out)


def case_a(rng):
    studies = [int(s) for s in rng.permutation(np.arange(50123, 50146))]         # 23 ids, unsorted
    labels = [_report(rng) for _ in range(9)]
    lab = [labels[i % 9] for i in range(len(studies))]
    preds = [_noisy(rng, t) for t in lab]
    calls, lo = [], 0
    for n in (8, 8, 7):
        calls.append({"predictions": preds[lo:lo + n], "labels": [[t] for t in lab[lo:lo + n]], "study_ids": studies[lo:lo + n]})
        lo += n
    calls.append({"predictions": [preds[0], "the lungs are clear . another prediction entirely .", preds[2]],
                  "labels": [[lab[0]], [lab[1]], [lab[2]]], "study_ids": [studies[0], studies[1], studies[2]]})
    return {"accumulate_over_dicoms": False, "metrics": ["bleu", "cider", "rouge"], "calls": calls}


def case_b(rng):
    studies = list(range(61017, 61000, -1))
    order = rng.permutation(len(studies)).tolist()
    labels = [_report(rng) for _ in range(7)]
    preds, lab, sids, dids = [], [], [], []
    for k in order:
        for d in range(1 + k % 3):
            lab.append(labels[k % 7])
            preds.append(_noisy(rng, lab[-1]))
            sids.append(studies[k])
            dids.append(f"dicom-{studies[k]}-{d}")
    calls = []
    for lo in range(0, len(preds), 8):
        calls.append({"predictions": preds[lo:lo + 8], "labels": [[t] for t in lab[lo:lo + 8]], "study_ids": sids[lo:lo + 8],
                      "dicom_ids": dids[lo:lo + 8]})
    calls.append({"predictions": [preds[5], "no pneumothorax is seen . the heart is large .", preds[0]], "labels": [[lab[5]], [lab[9]], [lab[0]]],
                  "study_ids": [sids[5], sids[9], sids[0]], "dicom_ids": [dids[5], dids[9], dids[0]]})
    return {"accumulate_over_dicoms": True, "metrics": ["bleu", "cider", "rouge"], "calls": calls}


def case_c(rng):
    lab = [_report(rng) for _ in range(6)]
    preds = [_noisy(rng, t) for t in lab]
    preds[2] = ""
    return {"accumulate_over_dicoms": False, "metrics": ["bleu", "cider", "rouge"],
            "calls": [{"predictions": preds, "labels": [[t] for t in lab], "study_ids": [f"s{n}" for n in range(6)]}]}


def case_d(rng):
    lab = ["the heart is  normal in size .  the lungs are clear . ", "no pneumothorax is seen .", " there is no pleural effusion .",
           "the lungs\tare clear . no effusion .", "mild atelectasis   is present ."]
    preds = ["the heart is normal in size . the lungs are clear .", "no pneumothorax is seen . ", "there is no pleural effusion .",
             "the lungs are clear . no\teffusion .", "mild  atelectasis is present  . "]
    sids = [7, 7, 8, 9, 9]
    dids = ["d0", "d1", "d2", "d3", "d4"]
    return {"accumulate_over_dicoms": True, "metrics": ["bleu", "cider", "rouge"],
            "calls": [{"predictions": preds, "labels": [[t] for t in lab], "study_ids": sids, "dicom_ids": dids}]}


def case_e(rng):
    lab = [_report(rng) for _ in range(5)]
    return {"accumulate_over_dicoms": False, "metrics": ["bleu", "cider", "rouge"],
            "calls": [{"predictions": list(lab), "labels": [[t] for t in lab], "study_ids": [5, 4, 3, 2, 1]}]}


def case_f(rng):
    lab = _report(rng)
    return {"accumulate_over_dicoms": False, "metrics": ["bleu", "cider", "rouge"],
            "calls": [{"predictions": [_noisy(rng, lab)], "labels": [[lab]], "study_ids": [77]}]}


def case_g(rng):
    lab = _report(rng, 4, 6)
    preds = [_noisy(rng, lab) for _ in range(7)]
    return {"accumulate_over_dicoms": True, "metrics": ["bleu", "cider", "rouge"],
            "calls": [{"predictions": preds, "labels": [[lab]] * 7, "study_ids": [1, 1, 2, 3, 3, 3, 4], "dicom_ids": list("abcdefg")}]}


def case_h(rng):
    case = case_a(rng)
    case["metrics"] = ["ROUGE", "Cider"]
    return case


CASES = (("a", case_a, 21), ("b", case_b, 22), ("c", case_c, 23), ("d", case_d, 24), ("e", case_e, 25), ("f", case_f, 26), ("g", case_g, 27),
         ("h", case_h, 28))


# ------------------------------------------------------------------------------------------------ run and record
def _clean(v):
    if isinstance(v, (float, np.floating)):
        return None if math.isnan(v) else float(v)
    if isinstance(v, np.integer):
        return int(v)
    return v


def run_case(cls, case, work):
    import pandas as pd
    exp_dir = os.path.join(work, "exp")
    metric = cls("test", exp_dir, case["accumulate_over_dicoms"], metrics=list(case["metrics"]), use_tokenizer=False)
    for c in case["calls"]:
        metric.update(c["predictions"], c["labels"], c["study_ids"], c.get("dicom_ids"))
    out = metric.compute(epoch=7)
    files = glob.glob(os.path.join(exp_dir, "nlg_scores", "test_epoch-7_[0-9]*.csv"))
    assert len(files) == 1, files
    df = pd.read_csv(files[0])
    shutil.rmtree(exp_dir)
    return {"result": [[k, _clean(v)] for k, v in out.items()],
            "csv": {"columns": list(df.columns), "rows": [[_clean(v) for v in row] for row in df.itertuples(index=False, name=None)]}}


def make(out_dir):
    cls = reference_class()
    doc = {"cases": {}}
    work = tempfile.mkdtemp(prefix="golden_coco_nlg_")
    try:
        for name, build, seed in CASES:
            case = build(np.random.default_rng(seed))
            case.update(run_case(cls, case, work))
            doc["cases"][name] = case
            print(f"{name}: {len(case['csv']['rows'])} rows, " + ", ".join(f"{k} {v:.6g}" for k, v in case["result"]))
    finally:
        shutil.rmtree(work)
    cases = doc["cases"]
    assert [k for k, _ in cases["a"]["result"]] == ["num_study_ids", "bleu_1", "bleu_2", "bleu_3", "bleu_4", "rouge", "cider"]
    assert [k for k, _ in cases["b"]["result"]] == ["num_study_ids", "num_dicom_ids", "bleu_1", "bleu_2", "bleu_3", "bleu_4", "rouge", "cider"]
    assert cases["b"]["csv"]["columns"] == ["dicom_id", "study_id", "bleu_1", "bleu_2", "bleu_3", "bleu_4", "rouge", "cider"]
    assert [k for k, _ in cases["h"]["result"]] == ["num_study_ids", "rouge", "cider"]
    assert dict(cases["f"]["result"])["cider"] == 0.0 and dict(cases["g"]["result"])["cider"] == 0.0
    assert dict(cases["e"]["result"])["rouge"] == 1.0
    assert cases["c"]["csv"]["rows"][2][1:] == [0.0] * 6                           # the empty prediction: exact zeros
    path = os.path.join(out_dir, FILE)
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB")


def verify():
    tmp = tempfile.mkdtemp(prefix="golden_coco_nlg_verify_")
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
