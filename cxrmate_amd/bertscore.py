"""BERTScore with RoBERTa-large on MI355X (reference tools/metrics/bertscore.py `BERTScoreRoBERTaLarge`, the test stage's fourth metric family).

The reference builds `bert_score.BERTScorer(model_type='roberta-large', num_layers=17, idf=False, rescale_with_baseline=True)` and calls
`score(predictions, labels, batch_size=mbatch_size)`. What that computes, restated here:
  * every distinct sentence is tokenised once (bert_score's RoBERTa rule: strip, then `encode(add_special_tokens=True, add_prefix_space=True,
    truncation=True, max_length=model_max_length)`; an empty sentence is `<s></s>`) and embedded once by RoBERTa-large truncated to its first
    17 layers, the last hidden state of that truncated model being the token embedding;
  * each (candidate, reference) pair is matched greedily on cosine similarity, with weight 0 on `<s>` / `</s>` and 1 elsewhere (idf=False);
  * the raw (P, R, F) are rescaled with the baseline of layer 17: (x - b) / (1 - b).

Here the trunk is the bidirectional path of the decoder engine (`BertEngine`, 1024 wide, 16 heads) with the RoBERTa embedding kernel
(`cxr_roberta_embed_fwd`, positions computed on the device), the sentences are embedded longest first in mini-batches of `batch_size` with key
padding, and ONE launch of `cxr_bertscore_match` matches every pair straight from the bf16 hidden states (csrc/bertscore.hip). The reference pads
each chunk of `batch_size` consecutive pairs to the chunk's longest candidate and reference and multiplies the similarities by the mask, so the
padded zeros take part in the maxima: `floor_flags` reproduces that per pair.

The `roberta-large` weights and tokenizer and bert_score's baseline file are not available offline: pass `tokenizer=`, `state_dict=` and
`baseline=` (INTEGRATION.md says where they come from). Without weights the trunk is a seeded random initialisation (tests, benchmarks).
"""
from __future__ import annotations

import csv
import os
import time
from collections import OrderedDict

import numpy as np
import torch

from . import ops, weights
from .config import BertConfig
from .decoder import BertEngine
from .store import ParamStore

MAX_TOKENS = 512                       # RoBERTa's model_max_length; also the matching kernel's limit per side


def roberta_large_config(num_layers: int = 17) -> BertConfig:
    """RoBERTa-large (HF `roberta-large` config.json) truncated to `num_layers` layers, as bert_score truncates `model.encoder.layer`."""
    return BertConfig(vocab_size=50265, hidden_size=1024, num_hidden_layers=num_layers, num_attention_heads=16, intermediate_size=4096,
                      max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, is_decoder=False,
                      add_cross_attention=False, cls_projection_size=0)


def roberta_param_shapes(cfg: BertConfig):
    """Engine key names (`bert.embeddings.*`, `bert.encoder.layer.{l}.*`) of the trunk; no pooler, no LM head."""
    return OrderedDict((k, v) for k, v in weights.bert_param_shapes(cfg, prefix="").items() if not k.startswith("cls."))


def roberta_state_dict(state_dict, num_layers: int):
    """A RoBERTa state dict (`roberta.`-prefixed as in RobertaForMaskedLM, or unprefixed as in AutoModel / RobertaModel) -> the engine's names.
    `pooler.*`, `lm_head.*`, the position-id / token-type-id buffers and layers >= num_layers are dropped; other keys are kept under their
    own name, so that a strict load reports them."""
    out = OrderedDict()
    for k, v in state_dict.items():
        name = k[len("roberta."):] if k.startswith("roberta.") else k
        if name.startswith(("pooler.", "lm_head.")) or name in ("embeddings.position_ids", "embeddings.token_type_ids"):
            continue
        if name.startswith("encoder.layer."):
            if int(name.split(".")[2]) >= num_layers:
                continue
            out["bert." + name] = v
        elif name.startswith("embeddings."):
            out["bert." + name] = v
        else:
            out[k] = v
    return out


def load_baseline(baseline, num_layers: int):
    """(P, R, F) baseline as fp32 [3] from a 3-tuple, or from bert_score's `rescale_baseline/en/roberta-large.tsv`. bert_score reads that file
    with `pd.read_csv(path).iloc[num_layers].to_numpy()[1:]`: comma-separated despite its name, header `LAYER,P,R,F`, one row per layer from
    layer 0. That layout is restated from memory of bert_score and could not be checked against the file here; a tab-separated file is accepted
    too, and the row's LAYER value must equal num_layers."""
    if isinstance(baseline, (str, os.PathLike)):
        with open(baseline, newline="") as f:
            lines = [ln for ln in f.read().splitlines() if ln.strip()]
        delim = "," if "," in lines[0] else "\t"
        rows = list(csv.reader(lines, delimiter=delim))
        header, data = [c.strip() for c in rows[0]], rows[1:]
        if header[1:4] != ["P", "R", "F"]:
            raise ValueError(f"{baseline}: expected the columns LAYER,P,R,F, found {header}")
        if not 0 <= num_layers < len(data):
            raise ValueError(f"{baseline}: no row for layer {num_layers} ({len(data)} rows)")
        row = data[num_layers]
        if float(row[0]) != num_layers:
            raise ValueError(f"{baseline}: row {num_layers} is layer {row[0]}")
        vals = [float(x) for x in row[1:4]]
    else:
        vals = [float(x) for x in baseline]
        if len(vals) != 3:
            raise ValueError("baseline must be a path or a (P, R, F) 3-tuple")
    return torch.tensor(vals, dtype=torch.float32)


def floor_flags(hyp_lens, ref_lens, batch_size: int):
    """uint8 [pairs, 2]: (floor the precision row maxima at 0, floor the recall column maxima at 0) per pair. The reference matches chunks of
    `batch_size` consecutive pairs padded to the chunk's longest candidate / reference, with padded similarities exactly 0: a pair's row maxima
    see a padded 0 iff its reference is shorter than the chunk's longest reference, its column maxima iff its candidate is shorter than the
    chunk's longest candidate."""
    hl, rl = np.asarray(hyp_lens, dtype=np.int64), np.asarray(ref_lens, dtype=np.int64)
    assert hl.shape == rl.shape and batch_size >= 1
    out = np.zeros((len(hl), 2), dtype=np.uint8)
    for lo in range(0, len(hl), batch_size):
        h, r = hl[lo:lo + batch_size], rl[lo:lo + batch_size]
        out[lo:lo + batch_size, 0] = r < r.max()
        out[lo:lo + batch_size, 1] = h < h.max()
    return out


class RobertaScorer:
    """bert_score.score(cands, refs, model_type='roberta-large', num_layers=17, idf=False, rescale_with_baseline=True) on the HIP kernels."""

    def __init__(self, device, tokenizer=None, state_dict=None, num_layers: int = 17, baseline=None, config: BertConfig | None = None,
                 seed: int = 3):
        self.device = torch.device(device)
        self.num_layers = int(num_layers)
        self.config = config or roberta_large_config(self.num_layers)
        if self.config.num_hidden_layers != self.num_layers:
            raise ValueError(f"config has {self.config.num_hidden_layers} layers, num_layers is {self.num_layers}")
        self.tokenizer = tokenizer
        shapes = roberta_param_shapes(self.config)
        self.model = ParamStore(shapes, {}, self.device, trainable=lambda k: False)
        if state_dict is None:
            state_dict = weights.init_state_dict(shapes, seed=seed, std=self.config.initializer_range, perturb=0.05)
        else:
            state_dict = roberta_state_dict(state_dict, self.num_layers)
        self.model.load_state_dict(state_dict)
        self.engine = BertEngine(self.model, self.config, prefix="", roberta_embeddings=True)
        self.baseline = None if baseline is None else load_baseline(baseline, self.num_layers)
        mml = getattr(tokenizer, "model_max_length", MAX_TOKENS)
        self.max_length = min(int(mml) if mml else MAX_TOKENS, MAX_TOKENS, self.config.max_position_embeddings - self.config.pad_token_id - 1)
        self.cls_id = getattr(tokenizer, "cls_token_id", None)
        self.sep_id = getattr(tokenizer, "sep_token_id", None)
        self.cls_id = 0 if self.cls_id is None else int(self.cls_id)
        self.sep_id = 2 if self.sep_id is None else int(self.sep_id)

    @property
    def hash(self):
        """bert_score's hash string of this configuration (model, layer, idf, rescale)."""
        return f"roberta-large_L{self.num_layers}_no-idf_version=cxrmate_amd-rescaled"

    def tokenize(self, sentence: str):
        """bert_score's sent_encode for a RoBERTa tokenizer -> token ids (with <s> ... </s>)."""
        tok = self.tokenizer
        if tok is None:
            raise RuntimeError("RobertaScorer needs the roberta-large tokenizer (not available offline): pass tokenizer=...")
        s = sentence.strip()
        if s == "":
            return list(tok.build_inputs_with_special_tokens([]))
        return list(tok.encode(s, add_special_tokens=True, add_prefix_space=True, max_length=self.max_length, truncation=True))

    @torch.no_grad()
    def embed(self, toks, batch_size: int):
        """Token lists -> (hidden bf16 [rows, 1024], sentence table int32 [n, 2] = (first row, length), weights fp32 [rows]) on the device. Longest
        first in mini-batches of `batch_size`, each padded to its own longest row (key padding); the batches' outputs are the rows, so a sentence
        occupies `length` consecutive rows of its batch's padded block."""
        cfg, dev = self.config, self.device
        for t in toks:
            if not 1 <= len(t) <= MAX_TOKENS:
                raise ValueError(f"a tokenised sentence has {len(t)} tokens (1 .. {MAX_TOKENS})")
        order = sorted(range(len(toks)), key=lambda i: -len(toks[i]))
        table = np.zeros((len(toks), 2), dtype=np.int32)
        outs, wts, base = [], [], 0
        for lo in range(0, len(order), batch_size):
            idx = order[lo:lo + batch_size]
            width = len(toks[idx[0]])
            ids = np.full((len(idx), width), cfg.pad_token_id, dtype=np.int64)
            mask = np.zeros((len(idx), width), dtype=np.uint8)
            w = np.zeros((len(idx), width), dtype=np.float32)
            for r, i in enumerate(idx):
                t = np.asarray(toks[i], dtype=np.int64)
                ids[r, :len(t)] = t
                mask[r, :len(t)] = 1
                w[r, :len(t)] = (t != self.cls_id) & (t != self.sep_id)
                table[i] = (base + r * width, len(t))
            h, _ = self.engine.forward(torch.from_numpy(ids).to(dev), attn_mask=torch.from_numpy(mask).to(dev), causal=False, lm_head=False, train=False)
            outs.append(h.reshape(-1, cfg.hidden_size))
            wts.append(w.reshape(-1))
            base += len(idx) * width
        hidden = outs[0] if len(outs) == 1 else torch.cat(outs)
        return hidden, torch.from_numpy(table).to(dev), torch.from_numpy(np.concatenate(wts)).to(dev)

    @torch.no_grad()
    def score_raw(self, cands, refs, batch_size: int = 64, embed_batch_size: int | None = None):
        """Raw (P, R, F) fp32 CPU [len(cands)] in input order (bert_score before the baseline rescale). batch_size sets both the embedding
        mini-batches and the pair chunks (as in bert_score); embed_batch_size overrides the former alone."""
        assert len(cands) == len(refs), "cands and refs must have the same length"
        n = len(cands)
        if n == 0:
            e = torch.zeros((0,), dtype=torch.float32)
            return e, e.clone(), e.clone()
        uniq = {}
        for s in list(refs) + list(cands):                      # every distinct sentence is embedded once
            uniq.setdefault(s, len(uniq))
        toks = [self.tokenize(s) for s in uniq]
        hidden, table, wts = self.embed(toks, embed_batch_size or batch_size)
        hi = np.array([uniq[s] for s in cands], dtype=np.int32)
        ri = np.array([uniq[s] for s in refs], dtype=np.int32)
        lens = np.array([len(t) for t in toks])
        flags = floor_flags(lens[hi], lens[ri], batch_size)
        pairs = torch.from_numpy(np.stack([hi, ri], 1)).to(self.device)
        P, R, F = ops.bertscore_match(hidden, table, pairs, wts, torch.from_numpy(flags).to(self.device))
        out = torch.stack([P, R, F]).cpu()
        return out[0], out[1], out[2]

    def _need_baseline(self):
        if self.baseline is None:
            raise RuntimeError("rescale_with_baseline needs bert_score's baseline of roberta-large (rescale_baseline/en/roberta-large.tsv, not "
                               "available offline): pass baseline=<path to that file> or baseline=(P, R, F)")

    def rescale(self, P, R, F):
        self._need_baseline()
        b = self.baseline
        return tuple((x - b[k]) / (1 - b[k]) for k, x in enumerate((P, R, F)))

    def score(self, cands, refs, batch_size: int = 64):
        """bert_score.score(cands, refs, idf=False, rescale_with_baseline=True, batch_size=batch_size) -> (P, R, F) fp32 CPU, input order."""
        self._need_baseline()                                   # before any work is done
        return self.rescale(*self.score_raw(cands, refs, batch_size))


def _is_dist():
    return torch.distributed.is_available() and torch.distributed.is_initialized()


class BERTScoreRoBERTaLarge:
    """The reference's torchmetrics `BERTScoreRoBERTaLarge(split, ckpt_dir, mbatch_size, exp_dir, accumulate_over_dicoms, num_workers)`:
    `update(predictions, labels, study_ids, dicom_ids=None)` collects reports, `compute(epoch)` scores them, writes
    `<exp_dir>/bertscore/<split>_epoch-<epoch>_scores_<time>.csv` on rank 0 and returns {'f1', 'precision', 'recall'} (means over studies when
    reports were accumulated per DICOM). The scorer is `RobertaScorer(device, tokenizer=..., state_dict=..., baseline=...)`; `num_workers` is
    kept for the call surface (tokenisation runs in-process)."""

    def __init__(self, split, ckpt_dir, mbatch_size, exp_dir, accumulate_over_dicoms, num_workers, scorer=None, device=None):
        self.split, self.ckpt_dir, self.mbatch_size, self.exp_dir = split, ckpt_dir, int(mbatch_size), exp_dir
        self.accumulate_over_dicoms = bool(accumulate_over_dicoms)
        self.num_workers = num_workers
        self.scorer = scorer
        self.device = torch.device(device) if device is not None else (scorer.device if scorer is not None else None)
        self.save_dir = os.path.join(self.exp_dir, "bertscore")
        os.makedirs(self.save_dir, exist_ok=True)
        self.reset()

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

    def compute(self, epoch):
        if self.scorer is None:
            raise RuntimeError("BERTScoreRoBERTaLarge needs a RobertaScorer (the roberta-large weights, tokenizer and baseline are not available "
                               "offline): pass scorer=RobertaScorer(device, tokenizer=..., state_dict=..., baseline=...)")
        for group in self._label:                              # following COCO the label of a report is a one-element list
            assert len(group) == 1
        labels = [group[0] for group in self._label]
        P, R, F = self.scorer.score(list(self._pred), labels, batch_size=self.mbatch_size)
        print(self.scorer.hash)
        table = {"study_id": np.asarray(self._study, dtype=object), "f1": F.double().numpy(), "precision": P.double().numpy(),
                 "recall": R.double().numpy()}
        if self.accumulate_over_dicoms:
            table["dicom_id"] = np.asarray(self._dicom, dtype=object)
        if _is_dist():                                          # rows of all ranks, rank order
            parts = [None] * torch.distributed.get_world_size()
            torch.distributed.all_gather_object(parts, table)
            table = {k: np.concatenate([p[k] for p in parts]) for k in table}
        key = "dicom_id" if self.accumulate_over_dicoms else "study_id"
        _, first = np.unique(table[key].astype(str), return_index=True)          # DDP pads the last batch with repeats: keep the first row
        keep = np.sort(first)
        table = {k: v[keep] for k, v in table.items()}
        cols = (["dicom_id"] if self.accumulate_over_dicoms else []) + ["study_id", "f1", "precision", "recall"]
        if not _is_dist() or torch.distributed.get_rank() == 0:
            path = os.path.join(self.save_dir, f'{self.split}_epoch-{epoch}_scores_{time.strftime("%d-%m-%Y_%H-%M-%S")}.csv')
            with open(path, "w", newline="") as f:
                w = csv.writer(f)
                w.writerow(cols)
                w.writerows(zip(*(table[c] for c in cols)))
        out = {}
        for name in ("f1", "precision", "recall"):
            s = table[name]
            if self.accumulate_over_dicoms:                     # mean over the DICOMs of a study first
                _, inv = np.unique(table["study_id"].astype(str), return_inverse=True)
                s = np.bincount(inv, weights=s) / np.bincount(inv)
            out[name] = float(s.mean())
        return out
