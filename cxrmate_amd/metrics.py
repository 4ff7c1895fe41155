"""Test-stage metrics on MI355X: `CXRBERT` (below) and `CheXbertClassificationMetrics` (its own docstring).

CXR-BERT similarity metric -- the evaluation-time consumer of the reward kernels (reference tools/metrics/cxr_bert.py:10-184).

Behaviour kept from the reference's torchmetrics `CXRBERT(split, ckpt_dir, mbatch_size, exp_dir, accumulate_over_dicoms)`:
  * `update(predictions, labels, study_ids, dicom_ids=None)` checks its arguments the way the reference does and collects the reports;
  * `compute(epoch)` scores every (prediction, label) pair by the cosine similarity of the projected CLS embeddings, merges the rows of all
    ranks, keeps one row per DICOM / study (DDP pads the last batch with repeats), writes
    `<exp_dir>/cxr_bert/<split>_epoch-<epoch>_scores_<time>.csv` on rank 0 and returns the mean similarity, averaged per study first when
    scores were accumulated per DICOM.

How it is computed is this build's own: the state is columnar (four parallel lists), all texts are tokenised in ONE call per side, the rows are
embedded longest-first in mini-batches of `mbatch_size` (so a batch pads to its own longest report, not to the epoch's), each distinct label text
is embedded once however many predictions share it, the cosine runs on the device over the whole epoch at once, and de-duplication /
per-study averaging are numpy index operations. The two BERT-base forwards run on the same HIP kernels as the SCST reward
(`reward.CXRBERTReward.embed_ids`). torchmetrics / pandas are not dependencies. The CXR-BERT weights and tokenizer are not available offline
(DESIGN.md section 2): pass `reward=CXRBERTReward(device, tokenizer=..., state_dict=...)`.
"""
from __future__ import annotations

import csv
import os
import time

import numpy as np
import torch


def _is_dist():
    return torch.distributed.is_available() and torch.distributed.is_initialized()


class CXRBERT:
    def __init__(self, split, ckpt_dir, mbatch_size, exp_dir, accumulate_over_dicoms, reward=None, device=None):
        self.split, self.ckpt_dir, self.mbatch_size, self.exp_dir = split, ckpt_dir, int(mbatch_size), exp_dir
        self.accumulate_over_dicoms = bool(accumulate_over_dicoms)
        self.reward = reward
        self.device = torch.device(device) if device is not None else (reward.device if reward is not None else None)
        self.save_dir = os.path.join(self.exp_dir, "cxr_bert")
        os.makedirs(self.save_dir, exist_ok=True)
        self.reset()

    # ------------------------------------------------------------------------------------------ state
    def reset(self):
        self._pred, self._label, self._study, self._dicom = [], [], [], []

    @property
    def reports(self):
        """The collected reports in the reference's record form (its torchmetrics state of the same name)."""
        keys = ("prediction", "label", "study_id") + (("dicom_id",) if self.accumulate_over_dicoms else ())
        cols = (self._pred, self._label, self._study) + ((self._dicom,) if self.accumulate_over_dicoms else ())
        return [dict(zip(keys, row)) for row in zip(*cols)]

    @staticmethod
    def mini_batch(iterable, mbatch_size=1):
        """Consecutive slices of at most `mbatch_size` items (kept for callers of the reference's helper of the same name)."""
        return (iterable[lo:lo + mbatch_size] for lo in range(0, len(iterable), mbatch_size))

    def update(self, predictions, labels, study_ids, dicom_ids=None):
        assert isinstance(predictions, list), '"predictions" must be a list of strings.'
        assert all(isinstance(p, str) for p in predictions), 'Each element of "predictions" must be a string.'
        assert isinstance(labels, list), '"labels" must be a list of lists, where each sub-list has a multiple strings.'
        assert all(isinstance(group, list) for group in labels), 'Each element of "labels" must be a list of strings.'
        assert all(isinstance(text, str) for group in labels for text in group), 'each sub-list must have one or more strings.'
        n = min(len(predictions), len(labels), len(study_ids)) if not self.accumulate_over_dicoms else \
            min(len(predictions), len(labels), len(study_ids), len(dicom_ids))
        self._pred += predictions[:n]
        self._label += labels[:n]
        self._study += list(study_ids[:n])
        if self.accumulate_over_dicoms:
            self._dicom += list(dicom_ids[:n])

    # ------------------------------------------------------------------------------------------ scoring
    def _embed_all(self, texts):
        """fp32 [len(texts), 128]: one tokenizer call, longest-first mini-batches (each pads to its own longest row), original order restored."""
        rw = self.reward
        kw = dict(add_special_tokens=True, padding=False, truncation=True, max_length=rw.config.max_position_embeddings)
        enc = rw.tokenizer(texts, **kw)["input_ids"]
        order = sorted(range(len(enc)), key=lambda i: -len(enc[i]))
        pad_id = getattr(rw.tokenizer, "pad_token_id", 0) or 0
        out = torch.empty((len(texts), rw.config.cls_projection_size), dtype=torch.float32, device=rw.device)
        for lo in range(0, len(order), self.mbatch_size):
            idx = order[lo:lo + self.mbatch_size]
            width = len(enc[idx[0]])
            ids = torch.full((len(idx), width), pad_id, dtype=torch.int64)
            mask = torch.zeros((len(idx), width), dtype=torch.int64)
            for r, i in enumerate(idx):
                ids[r, :len(enc[i])] = torch.tensor(enc[i], dtype=torch.int64)
                mask[r, :len(enc[i])] = 1
            out[torch.tensor(idx, device=rw.device)] = rw.embed_ids(ids.pin_memory().to(rw.device, non_blocking=True),
                                                                    mask.pin_memory().to(rw.device, non_blocking=True))
        return out

    def compute(self, epoch):
        from . import ops
        if self.reward is None or self.reward.tokenizer is None:
            raise RuntimeError("CXRBERT metric needs a CXRBERTReward with its tokenizer (CXR-BERT weights + tokenizer are not available offline): "
                               "pass reward=CXRBERTReward(device, tokenizer=..., state_dict=...)")
        for group in self._label:                              # following COCO the label of a report is a one-element list (cxr_bert.py:97-99)
            assert len(group) == 1
        label_texts = [group[0] for group in self._label]
        uniq = {}
        label_row = [uniq.setdefault(t, len(uniq)) for t in label_texts]        # every distinct label text is embedded once
        with torch.no_grad():
            pred_emb = self._embed_all(self._pred)
            lab_emb = self._embed_all(list(uniq))[torch.tensor(label_row, device=self.reward.device)]
            sim = ops.cosine_rows(pred_emb, lab_emb).float().cpu().numpy()
        table = {"study_id": np.asarray(self._study, dtype=object), "similarity": sim.astype(np.float64)}
        if self.accumulate_over_dicoms:
            table["dicom_id"] = np.asarray(self._dicom, dtype=object)
        if _is_dist():                                          # rows of all ranks, rank order (reference: all_gather_object of the row dicts)
            parts = [None] * torch.distributed.get_world_size()
            torch.distributed.all_gather_object(parts, table)
            table = {k: np.concatenate([p[k] for p in parts]) for k in table}
        key = "dicom_id" if self.accumulate_over_dicoms else "study_id"
        _, first = np.unique(table[key].astype(str), return_index=True)          # one row per DICOM / study: DDP pads the last batch with repeats
        keep = np.sort(first)
        table = {k: v[keep] for k, v in table.items()}
        if not _is_dist() or torch.distributed.get_rank() == 0:
            cols = (["dicom_id"] if self.accumulate_over_dicoms else []) + ["study_id", "similarity"]
            path = os.path.join(self.save_dir, f'{self.split}_epoch-{epoch}_scores_{time.strftime("%d-%m-%Y_%H-%M-%S")}.csv')
            with open(path, "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(cols)
                w.writerows(zip(*(table[c] for c in cols)))
        scores = table["similarity"]
        if self.accumulate_over_dicoms:                         # mean over the DICOMs of a study first
            _, inv = np.unique(table["study_id"].astype(str), return_inverse=True)
            scores = np.bincount(inv, weights=scores) / np.bincount(inv)
        return float(scores.mean())


# ================================================================================================ CheXbert classification metrics
PATHOLOGIES = [
    "enlarged_cardiomediastinum", "cardiomegaly", "lung_opacity", "lung_lesion", "edema", "consolidation", "pneumonia", "atelectasis",
    "pneumothorax", "pleural_effusion", "pleural_other", "fracture", "support_devices", "no_finding",
]
_ERRORS = ("tp", "tn", "fp", "fn")
_RATIOS = ("accuracy", "precision", "recall", "f1")


def _plain(v):
    return v.item() if hasattr(v, "item") else v


def merge_label_parts(parts, accumulate_over_dicoms):
    """The host step between labelling and scoring, as a pure function of the per-rank parts (rank order). A part is a dict: `pred` int64 [n, 14]
    (one row per record), `ref` int64 [u, 14] (one row per distinct label text of that rank), `ref_row` [n] (each record's row in `ref`),
    `study_id` [n] and, when accumulating, `dicom_id` [n].
    -> dict: `pred` / `ref` the concatenated tables; `pred_row`, `ref_row` int32 [M], `study_id`, `dicom_id` (lists): the kept records -- the
    first per DICOM, or per study when not accumulating -- in order of appearance; `order` int64 [M]: those records grouped by study, the
    studies sorted by id when accumulating (pandas groupby) and in order of first appearance otherwise; `studies`: the S ids in that order;
    `study_off` int32 [S + 1]: CSR offsets into `order`."""
    pred = np.concatenate([np.asarray(p["pred"], dtype=np.int64).reshape(-1, len(PATHOLOGIES)) for p in parts])
    ref = np.concatenate([np.asarray(p["ref"], dtype=np.int64).reshape(-1, len(PATHOLOGIES)) for p in parts])
    ref_base = np.cumsum([0] + [len(p["ref"]) for p in parts])
    ref_row = np.concatenate([np.asarray(p["ref_row"], dtype=np.int64) + b for p, b in zip(parts, ref_base)])
    study = [_plain(v) for p in parts for v in p["study_id"]]
    dicom = [_plain(v) for p in parts for v in p["dicom_id"]] if accumulate_over_dicoms else None
    seen, keep = set(), []
    for i, k in enumerate(dicom if accumulate_over_dicoms else study):     # one row per DICOM / study: DDP pads the last batch with repeats
        if k not in seen:
            seen.add(k)
            keep.append(i)
    kept_study = [study[i] for i in keep]
    first = {}
    for s in kept_study:
        first.setdefault(s, len(first))
    studies = sorted(first) if accumulate_over_dicoms else list(first)
    rank = {s: r for r, s in enumerate(studies)}
    group = np.array([rank[s] for s in kept_study], dtype=np.int64)
    order = np.argsort(group, kind="stable")
    study_off = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=len(studies)))]).astype(np.int32)
    return {"pred": pred, "ref": ref, "pred_row": np.asarray(keep, dtype=np.int32), "ref_row": ref_row[keep].astype(np.int32),
            "study_id": kept_study, "dicom_id": [dicom[i] for i in keep] if accumulate_over_dicoms else None, "order": order,
            "studies": studies, "study_off": study_off}


class CheXbertClassificationMetrics:
    """CheXbert classification metrics (reference tools/metrics/chexbert.py:34-336, the source of `val_report_chexbert_f1_macro`).

    Behaviour kept from the reference's torchmetrics `CheXbertClassificationMetrics(split, ckpt_dir, bert_path, checkpoint_path, mbatch_size, exp_dir,
    accumulate_over_dicoms)`: the update / compute / reset surface, the labeller built in `compute`, rows of all ranks merged in rank order, one row per
    DICOM / study, each error type averaged over the DICOMs of a study, the four CSVs under `<exp_dir>/chexbert_outputs` and the returned dict (12
    averaged scores, 56 per-pathology scores, `num_study_ids`, `num_dicom_ids`). How it is computed is this build's own: columnar state, every
    prediction and every DISTINCT label text labelled once over the whole epoch (`CheXbert.label_all`), only the two small class-index tables cross to
    the host, and everything pandas derives from them is one call of `cxr_chexbert_scores` (csrc/chexbert_metric.hip)."""

    def __init__(self, split, ckpt_dir, bert_path, checkpoint_path, mbatch_size, exp_dir, accumulate_over_dicoms, chexbert=None, device=None):
        self.split, self.ckpt_dir, self.bert_path, self.checkpoint_path = split, ckpt_dir, bert_path, checkpoint_path
        self.mbatch_size, self.exp_dir = int(mbatch_size), exp_dir
        self.accumulate_over_dicoms = bool(accumulate_over_dicoms)
        self.chexbert = chexbert
        self.device = torch.device(device) if device is not None else (chexbert.device if chexbert is not None else None)
        self.save_dir = os.path.join(self.exp_dir, "chexbert_outputs")
        os.makedirs(self.save_dir, exist_ok=True)
        self.reset()

    # ------------------------------------------------------------------------------------------ state (CXRBERT's: same columns, checks and messages)
    reset = CXRBERT.reset
    reports = CXRBERT.reports
    mini_batch = staticmethod(CXRBERT.mini_batch)
    update = CXRBERT.update

    # ------------------------------------------------------------------------------------------ scoring
    def _write(self, kind, epoch, header, rows):
        path = os.path.join(self.save_dir, f'{self.split}_epoch-{epoch}_{kind}_{time.strftime("%d-%m-%Y_%H-%M-%S")}.csv')
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(header)
            w.writerows(rows)

    def compute(self, epoch):
        from . import ops
        chexbert = self.chexbert
        if chexbert is None:                                    # as the reference: built here, from the checkpoint (tools/metrics/chexbert.py:108-113)
            from .chexbert import CheXbert
            chexbert = CheXbert(self.ckpt_dir, self.bert_path, self.checkpoint_path, self.device if self.device is not None else "cuda")
        for group in self._label:                               # following COCO the label of a report is a one-element list (:124-127)
            assert len(group) == 1
        uniq = {}
        label_row = [uniq.setdefault(group[0], len(uniq)) for group in self._label]      # every distinct label text is labelled once
        pred = chexbert.label_all(list(self._pred), self.mbatch_size)
        ref = chexbert.label_all(list(uniq), self.mbatch_size)
        part = {"pred": pred.cpu().numpy(), "ref": ref.cpu().numpy(), "ref_row": np.asarray(label_row, dtype=np.int64),
                "study_id": list(self._study)}
        if self.accumulate_over_dicoms:
            part["dicom_id"] = list(self._dicom)
        parts = [part]
        if _is_dist():                                          # parts of all ranks, rank order (reference: all_gather_object of the row dicts)
            parts = [None] * torch.distributed.get_world_size()
            torch.distributed.all_gather_object(parts, part)
        m = merge_label_parts(parts, self.accumulate_over_dicoms)
        dev = pred.device
        order = m["order"]
        example, cls, avg = ops.chexbert_scores(torch.from_numpy(m["pred"]).to(dev), torch.from_numpy(m["ref"]).to(dev),
                                                torch.from_numpy(m["pred_row"][order]).to(dev), torch.from_numpy(m["ref_row"][order]).to(dev),
                                                torch.from_numpy(m["study_off"]).to(dev))
        example, cls, avg = example.cpu().numpy(), cls.cpu().numpy(), avg.cpu().numpy()
        class_keys = [f"{r}_{p}" for r in _RATIOS for p in PATHOLOGIES]                      # the reference's melted column names
        class_vals = [float(cls[j, 4 + k]) for k in range(len(_RATIOS)) for j in range(len(PATHOLOGIES))]
        if not _is_dist() or torch.distributed.get_rank() == 0:
            ids = ["dicom_id", "study_id"] if self.accumulate_over_dicoms else ["study_id"]
            id_cols = ([m["dicom_id"]] if self.accumulate_over_dicoms else []) + [m["study_id"]]
            for kind, table, rows in (("y_hat", m["pred"], m["pred_row"]), ("y", m["ref"], m["ref_row"])):
                self._write(kind, epoch, ids + PATHOLOGIES, [list(i) + table[r].tolist() for *i, r in zip(*id_cols, rows)])
            self._write("class_scores", epoch, class_keys, [class_vals])
            self._write("example_scores", epoch, ["study_id", *_ERRORS, *_RATIOS], [[s] + example[i].tolist() for i, s in enumerate(m["studies"])])
        score = {f"{r}_{a}": float(avg[4 * j + k]) for j, a in enumerate(("example", "macro", "micro")) for k, r in enumerate(_RATIOS)}
        score.update(zip(class_keys, class_vals))
        score["num_study_ids"] = float(len(m["studies"]))
        if self.accumulate_over_dicoms:
            score["num_dicom_ids"] = float(len(set(m["dicom_id"])))
        return score
