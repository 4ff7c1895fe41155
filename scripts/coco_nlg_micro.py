"""Epoch-end cost of the COCO NLG metric (cxrmate_amd.metrics.COCONLGMetricsMIMICCXR.compute) beside the float64 restatement on the CPU.

    python scripts/coco_nlg_micro.py [--studies 3000] [--reps 3] [--no-cpu]

Workload: `--studies` synthetic studies with 1-2 DICOMs each (a prediction per DICOM: its label with words dropped and replaced; one label text
per study, every tenth shared with another study), reports of 20-200 words drawn by a Zipf law from 5000 made-up words, `use_tokenizer=False`.
`compute` runs once to warm up, then `--reps` times; the score call (`ops.coco_nlg_scores`: 4 x (insert, count, pair) + lcs + record + the two mean
launches, and its one wait for the offsets check) is timed with device events, the rest of `compute` (merge, blank collapsing, interning the words,
upload, CSV) is the remainder. The CPU figure is tests/coco_nlg_ref.py (pure Python + numpy, the pycocoevalcap algorithms) scoring the same records
once: `Bleu`, `Rouge`, `Cider` through their `compute_score`. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic_epoch(n_studies, seed=0):
    rng = np.random.default_rng(seed)
    vocab = np.array([f"w{i}" for i in range(5000)])

    def report():
        return vocab[np.minimum(rng.zipf(1.3, size=int(rng.integers(20, 201))), len(vocab)) - 1]

    labels = [report() for _ in range(n_studies)]
    for s in range(10, n_studies, 10):
        labels[s] = labels[s - 1]
    preds, labs, studies, dicoms = [], [], [], []
    for s in range(n_studies):
        for d in range(int(rng.integers(1, 3))):
            u = rng.random(len(labels[s]))
            preds.append(" ".join(np.where(u < 0.15, report()[0], labels[s])[u > 0.1].tolist()))
            labs.append([" ".join(labels[s].tolist())])
            studies.append(50000000 + s)
            dicoms.append(f"{s}-{d}")
    return preds, labs, studies, dicoms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--studies", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from cxrmate_amd import ops
    from cxrmate_amd.metrics import COCONLGMetricsMIMICCXR
    preds, labs, studies, dicoms = synthetic_epoch(args.studies)
    t_score = []
    scores = ops.coco_nlg_scores

    def timed_scores(*a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = scores(*a)
        e1.record()
        e1.synchronize()
        t_score.append(e0.elapsed_time(e1))
        return out

    ops.coco_nlg_scores = timed_scores
    rows = []
    with tempfile.TemporaryDirectory() as exp_dir:
        metric = COCONLGMetricsMIMICCXR("test", exp_dir, True, use_tokenizer=False, device="cuda:0")
        metric.update(preds, labs, studies, dicoms)
        for rep in range(args.reps + 1):
            del t_score[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = metric.compute(epoch=rep)
            total = (time.perf_counter() - t0) * 1e3
            if rep:                                                   # the first run warms up (kernel load, allocator)
                rows.append((total, t_score[0]))
    total, score = (statistics.median(c) for c in zip(*rows))
    line = {"studies": int(out["num_study_ids"]), "dicoms": int(out["num_dicom_ids"]), "distinct_label_texts": len({g[0] for g in labs}),
            "words": sum(len(p.split()) for p in preds), "reps": args.reps, "compute_ms": total, "score_call_ms": score,
            "host_rest_ms": total - score, "bleu_4": out["bleu_4"], "rouge": out["rouge"], "cider": out["cider"]}
    if not args.no_cpu:
        import coco_nlg_ref as nref
        gts, res = {k: g for k, g in zip(dicoms, labs)}, {k: [p] for k, p in zip(dicoms, preds)}
        t0 = time.perf_counter()
        _, bleu = nref.Bleu(4).compute_score(gts, res)
        _, rouge = nref.Rouge().compute_score(gts, res)
        _, cider = nref.Cider().compute_score(gts, res)
        line["cpu_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        line["cpu_record_means"] = {"bleu_4": float(np.mean(bleu[3])), "rouge": float(np.mean(rouge)), "cider": float(np.mean(cider))}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
