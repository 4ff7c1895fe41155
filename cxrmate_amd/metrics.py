"""Test-stage metrics on MI355X: `CXRBERT` (below), `CheXbertClassificationMetrics` and `COCONLGMetricsMIMICCXR` (their own docstrings).

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
import re
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


# ================================================================================================ COCO NLG metrics
_NLG_DEVICE_COLUMNS = ("bleu_1", "bleu_2", "bleu_3", "bleu_4", "rouge", "cider")
_NLG_ORDER = ("bleu", "meteor", "rouge", "cider", "spice")                   # the reference's column order (tools/metrics/coco.py:155-172)
_NLG_HOST = ("meteor", "spice")                                             # Java scorers: only as injected objects


def merge_report_parts(parts, accumulate_over_dicoms):
    """The host step between gathering and scoring, as a pure function of the per-rank parts (rank order). A part is a dict of equally long lists:
    `prediction`, `label` (one string per record), `study_id` and, when accumulating, `dicom_id`.
    The reference fills dicts keyed by the DICOM id (by the study id when not accumulating) and drops duplicate rows from its table, so for a
    repeated key the texts of the LAST record are scored, at the position and with the ids of the FIRST (tools/metrics/coco.py:123-147).
    -> dict: `prediction`, `label`, `study_id`, `dicom_id` (lists, `dicom_id` None when not accumulating): the M scored records in order of first
    appearance; `order` int64 [M]: those records grouped by study, the studies sorted by id when accumulating (pandas groupby) and in order of
    first appearance otherwise; `studies`: the S ids in that order; `study_off` int32 [S + 1]: CSR offsets into `order`."""
    pred = [t for p in parts for t in p["prediction"]]
    label = [t for p in parts for t in p["label"]]
    study = [_plain(v) for p in parts for v in p["study_id"]]
    dicom = [_plain(v) for p in parts for v in p["dicom_id"]] if accumulate_over_dicoms else None
    first, last = {}, {}
    for i, k in enumerate(dicom if accumulate_over_dicoms else study):
        first.setdefault(k, i)
        last[k] = i
    kept_study = [study[i] for i in first.values()]
    rank = {}
    for s in kept_study:
        rank.setdefault(s, len(rank))
    studies = sorted(rank) if accumulate_over_dicoms else list(rank)
    rank = {s: r for r, s in enumerate(studies)}
    group = np.array([rank[s] for s in kept_study], dtype=np.int64)
    return {"prediction": [pred[last[k]] for k in first], "label": [label[last[k]] for k in first], "study_id": kept_study,
            "dicom_id": [dicom[i] for i in first.values()] if accumulate_over_dicoms else None, "order": np.argsort(group, kind="stable"),
            "studies": studies, "study_off": np.concatenate([[0], np.cumsum(np.bincount(group, minlength=len(studies)))]).astype(np.int32)}


def stage_texts(predictions, labels):
    """Scored texts -> the inputs of `ops.coco_nlg_scores` (int32 numpy arrays): every distinct text is staged once, words are interned into ids
    with one dict, `ids_a` / `off_a` hold the `str.split()` tokens (BLEU, CIDEr) and `ids_b` / `off_b` the `str.split(" ")` tokens (ROUGE-L, for
    which a leading or trailing blank is an empty token and a tab does not split); `pairs` [M, 2] names each record's two texts and `ref_mult`
    counts the records whose reference a text is."""
    texts, words = {}, {}
    pairs = np.array([(texts.setdefault(p, len(texts)), texts.setdefault(l, len(texts))) for p, l in zip(predictions, labels)],
                     dtype=np.int32).reshape(-1, 2)
    out = {"pairs": pairs, "ref_mult": np.bincount(pairs[:, 1], minlength=len(texts)).astype(np.int32)}
    for name, sep in (("a", None), ("b", " ")):
        ids, off = [], [0]
        for t in texts:
            ids.extend(words.setdefault(w, len(words)) for w in t.split(sep))
            off.append(len(ids))
        out["ids_" + name], out["off_" + name] = np.array(ids, dtype=np.int32), np.array(off, dtype=np.int32)
    return out


class COCONLGMetricsMIMICCXR:
    """COCO NLG metrics (reference tools/metrics/coco.py:18-196, the source of `val_<section>_nlg_*`): per-record BLEU-1..4, ROUGE-L and CIDEr-D,
    averaged over the DICOMs of a study first when accumulating, then over the studies.

    Behaviour kept from the reference's torchmetrics class: its arguments in its order, update / compute / reset, records of all ranks merged in rank
    order, one row per DICOM / study (see `merge_report_parts` for which record's texts a repeated key keeps), one CSV under `<exp_dir>/nlg_scores`
    written by rank 0, and the returned dict, key for key. How it is computed is this build's own: columnar state, every distinct text staged once
    as word ids, and everything the COCO caption scorers and pandas compute is ONE `cxr_coco_nlg_scores` call (csrc/coco_nlg.hip) in float64.

    `metrics=None` means ['bleu', 'cider', 'rouge'] (the reference's own default cannot be constructed). The PTB tokenizer, METEOR and SPICE are
    Java programs and are only accepted as injected objects: `tokenizer=` with `tokenize({id: [{'caption': str}]}) -> {id: [str]}` when
    `use_tokenizer=True`, and `extra_scorers={'meteor': obj}` with `obj.compute_score(gts, res) -> (score, per-record scores)`."""

    def __init__(self, split, exp_dir, accumulate_over_dicoms, metrics=None, use_tokenizer=True, dist_sync_on_step=False, tokenizer=None,
                 extra_scorers=None, device=None):
        self.split, self.exp_dir = split, exp_dir
        self.accumulate_over_dicoms = bool(accumulate_over_dicoms)
        self.metrics = [m.lower() for m in (["bleu", "cider", "rouge"] if metrics is None else metrics)]
        self.use_tokenizer, self.dist_sync_on_step, self.tokenizer = bool(use_tokenizer), dist_sync_on_step, tokenizer
        self.extra_scorers = dict(extra_scorers or {})
        unknown = [m for m in self.metrics if m not in _NLG_ORDER]
        if unknown:
            raise ValueError(f"unknown COCO NLG metrics {unknown}: choose from {list(_NLG_ORDER)}")
        for m in _NLG_HOST:
            if m in self.metrics and not hasattr(self.extra_scorers.get(m), "compute_score"):
                raise ValueError(f"'{m}' is a Java scorer that is not built here: pass extra_scorers={{'{m}': obj}} with obj.compute_score(gts, res)")
        self.device = torch.device(device) if device is not None else None
        self.save_dir = os.path.join(self.exp_dir, "nlg_scores")
        os.makedirs(self.save_dir, exist_ok=True)
        self.reset()

    # ------------------------------------------------------------------------------------------ state (CXRBERT's: same columns, checks and messages)
    reset = CXRBERT.reset
    reports = CXRBERT.reports
    update = CXRBERT.update

    # ------------------------------------------------------------------------------------------ scoring
    def columns(self):
        """The score columns in the reference's order, restricted to the metrics asked for."""
        cols = []
        for m in _NLG_ORDER:
            if m in self.metrics:
                cols += [f"bleu_{k}" for k in range(1, 5)] if m == "bleu" else [m]
        return cols

    def compute(self, epoch):
        from . import ops
        if self.use_tokenizer and self.tokenizer is None:
            raise RuntimeError("COCONLGMetricsMIMICCXR(use_tokenizer=True) needs tokenizer=: an object with the PTBTokenizer interface, "
                               "tokenize({id: [{'caption': str}]}) -> {id: [str]} (the Java tokenizer is not built here); or use_tokenizer=False")
        for group in self._label:                               # one reference per record, as the reference's callers pass it
            assert len(group) == 1
        part = {"prediction": list(self._pred), "label": [group[0] for group in self._label], "study_id": list(self._study)}
        if self.accumulate_over_dicoms:
            part["dicom_id"] = list(self._dicom)
        parts = [part]
        if _is_dist():                                          # parts of all ranks, rank order (reference: all_gather_object of the row dicts)
            parts = [None] * torch.distributed.get_world_size()
            torch.distributed.all_gather_object(parts, part)
        m = merge_report_parts(parts, self.accumulate_over_dicoms)
        keys = m["dicom_id"] if self.accumulate_over_dicoms else m["study_id"]
        preds = [re.sub(" +", " ", t) for t in m["prediction"]]
        labels = [re.sub(" +", " ", t) for t in m["label"]]
        if self.use_tokenizer:
            tok_p = self.tokenizer.tokenize({k: [{"caption": t}] for k, t in zip(keys, preds)})
            tok_l = self.tokenizer.tokenize({k: [{"caption": t}] for k, t in zip(keys, labels)})
            preds, labels = [tok_p[k][0] for k in keys], [tok_l[k][0] for k in keys]
        st = stage_texts(preds, labels)
        dev = self.device if self.device is not None else torch.device("cuda")
        up = {k: torch.from_numpy(v).to(dev) for k, v in st.items()}
        scores, _, _, avg = ops.coco_nlg_scores(up["ids_a"], up["off_a"], up["ids_b"], up["off_b"], up["pairs"], up["ref_mult"],
                                                torch.from_numpy(m["order"].astype(np.int32)).to(dev), torch.from_numpy(m["study_off"]).to(dev))
        scores, avg = scores.cpu().numpy(), avg.cpu().numpy()
        table, mean = {}, {}
        for c in self.columns():
            if c in _NLG_DEVICE_COLUMNS:
                j = _NLG_DEVICE_COLUMNS.index(c)
                table[c], mean[c] = scores[:, j], float(avg[j])
            else:                                               # an injected host scorer: its per-record values join the same study grouping
                gts, res = {k: [t] for k, t in zip(keys, labels)}, {k: [t] for k, t in zip(keys, preds)}
                _, per = self.extra_scorers[c].compute_score(gts, res)
                table[c] = np.asarray(per, dtype=np.float64).reshape(len(keys))
                per_study = np.add.reduceat(table[c][m["order"]], m["study_off"][:-1]) / np.diff(m["study_off"]) if len(keys) else np.zeros(0)
                mean[c] = float(per_study.mean()) if len(per_study) else float("nan")
        if not _is_dist() or torch.distributed.get_rank() == 0:
            id_cols = ([("dicom_id", m["dicom_id"])] if self.accumulate_over_dicoms else []) + [("study_id", m["study_id"])]
            path = os.path.join(self.save_dir, f'{self.split}_epoch-{epoch}_{time.strftime("%d-%m-%Y_%H-%M-%S")}.csv')
            with open(path, "w", newline="") as f:
                w = csv.writer(f)
                w.writerow([n for n, _ in id_cols] + list(table))
                w.writerows(zip(*(v for _, v in id_cols), *(v.tolist() for v in table.values())))
        out = {"num_study_ids": float(len(m["studies"]))}
        if self.accumulate_over_dicoms:
            out["num_dicom_ids"] = float(len(set(m["dicom_id"])))
        out.update(mean)
        return out
