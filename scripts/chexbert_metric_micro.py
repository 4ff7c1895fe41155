"""Epoch-end cost of the CheXbert classification metric (cxrmate_amd.metrics.CheXbertClassificationMetrics.compute), labelling split from scoring.

    python scripts/chexbert_metric_micro.py [--studies 3000] [--mbatch 64] [--reps 3]

Workload: `--studies` synthetic studies with 1-2 DICOMs each (a prediction per DICOM, one label text per study shared by its DICOMs, every tenth
label text shared with another study), reports of 4-45 words (about 80 tokens on average) drawn from the vocabulary of
tests/golden/tokenizer.json, the full-size labeller (BERT-base, 12 layers, seeded random weights: the cost does not depend on the values). `compute` runs once to warm up, then `--reps` times;
`label_all` is timed around its calls (host + device, synchronised), the score launch (`ops.chexbert_scores`: three kernels) with device events,
and the rest of `compute` (copying the two tables to the host, merge / de-duplication / grouping, upload, four CSVs) is the remainder.
Prints one JSON line."""
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


def synthetic_epoch(tok, n_studies, seed=0):
    rng = np.random.default_rng(seed)
    words = [w for w in tok.get_vocab() if w.isalpha() and len(w) > 2]
    words.sort()

    def report():
        return " ".join(rng.choice(words, size=int(rng.integers(4, 46))).tolist()) + "."

    labels = [report() for _ in range(n_studies)]
    for s in range(10, n_studies, 10):
        labels[s] = labels[s - 1]
    preds, labs, studies, dicoms = [], [], [], []
    for s in range(n_studies):
        for d in range(int(rng.integers(1, 3))):
            preds.append(report())
            labs.append([labels[s]])
            studies.append(50000000 + s)
            dicoms.append(f"{s}-{d}")
    return preds, labs, studies, dicoms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--studies", type=int, default=3000)
    ap.add_argument("--mbatch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import transformers
    from cxrmate_amd import ops
    from cxrmate_amd.chexbert import CheXbert
    from cxrmate_amd.metrics import CheXbertClassificationMetrics
    tok = transformers.PreTrainedTokenizerFast(tokenizer_file=os.path.join(ROOT, "tests", "golden", "tokenizer.json"), unk_token="[UNK]",
                                               pad_token="[PAD]", cls_token="[BOS]", sep_token="[SEP]", mask_token="[MASK]")
    dev = torch.device("cuda:0")
    cb = CheXbert(dev, tokenizer=tok)
    preds, labs, studies, dicoms = synthetic_epoch(tok, args.studies)
    t_label, t_score = [], []
    label_all, scores = cb.label_all, ops.chexbert_scores

    def timed_label_all(texts, mbatch_size):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = label_all(texts, mbatch_size)
        torch.cuda.synchronize()
        t_label.append((time.perf_counter() - t0) * 1e3)
        return out

    def timed_scores(*a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = scores(*a)
        e1.record()
        e1.synchronize()
        t_score.append(e0.elapsed_time(e1))
        return out

    cb.label_all, ops.chexbert_scores = timed_label_all, timed_scores
    rows = []
    with tempfile.TemporaryDirectory() as exp_dir:
        metric = CheXbertClassificationMetrics("test", None, None, None, args.mbatch, exp_dir, True, chexbert=cb)
        metric.update(preds, labs, studies, dicoms)
        for rep in range(args.reps + 1):
            del t_label[:], t_score[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = metric.compute(epoch=rep)
            total = (time.perf_counter() - t0) * 1e3
            if rep:                                                   # the first run warms up (kernel load, allocator)
                rows.append((total, sum(t_label), t_score[0]))
    total, label, score = (statistics.median(c) for c in zip(*rows))
    print(json.dumps({"studies": int(out["num_study_ids"]), "dicoms": int(out["num_dicom_ids"]), "distinct_label_texts": len({g[0] for g in labs}),
                      "mbatch_size": args.mbatch, "reps": args.reps, "compute_ms": total, "labelling_ms": label, "score_launch_ms": score,
                      "host_rest_ms": total - label - score, "labelling_share": label / total, "f1_macro": out["f1_macro"]}), flush=True)


if __name__ == "__main__":
    main()
