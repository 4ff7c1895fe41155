"""GPU: BERTScore (reference tools/metrics/bertscore.py) -- the matching kernel, the RoBERTa embeddings and the 1024-wide LayerNorm against
float64, the RoBERTa trunk against transformers.RobertaModel, the scorer against a restatement of bert_score's pipeline on that oracle, and the
metric's update / compute flow."""

import numpy as np
import pytest
import torch

import bertscore_ref as bref
import golden_util as gu
from bounds_util import Guarded, assert_bf16_bracket

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ matching kernel
LENS = [1, 2, 3, 31, 33, 200, 512]


def _match_ref(H, sent, pairs, w, floors):
    """float64 restatement on the same bf16 rows: cosines from the exact bf16 values, max, weighted means, the floors, F, the empty rule."""
    H, w = H.double(), w.double()
    out = []
    for (hs, rs), (fp, fr) in zip(pairs.tolist(), floors.tolist()):
        (ho, lh), (ro, lr) = sent[hs].tolist(), sent[rs].tolist()
        h, r = H[ho:ho + lh], H[ro:ro + lr]
        sim = (h / h.norm(dim=1, keepdim=True)) @ (r / r.norm(dim=1, keepdim=True)).T
        pm, rm = sim.max(1).values, sim.max(0).values
        if fp:
            pm = pm.clamp(min=0)
        if fr:
            rm = rm.clamp(min=0)
        wh, wr = w[ho:ho + lh], w[ro:ro + lr]
        p, rr = float((wh * pm).sum() / wh.sum()) if wh.sum() > 0 else float("nan"), float((wr * rm).sum() / wr.sum()) if wr.sum() > 0 else float("nan")
        f = 2 * p * rr / (p + rr) if (p + rr) != 0 else float("nan")
        f = 0.0 if f != f else f
        if lh == 2 or lr == 2:
            p = rr = 0.0
        out.append((p, rr, f))
    return np.array(out)


def _match_case(D=1024):
    g = _gen(3)
    lens = LENS + LENS + [40, 40]                 # sentences 0-6 hyp side, 7-13 ref side, 14 / 15 the all-negative pair
    sent, rows = [], 0
    for L in lens:
        sent.append((rows, L))
        rows += L + 5                             # gaps between sentences: rows nobody should read as theirs
    H = torch.randn(rows, D, generator=g) * 0.5 + 0.3 * torch.randn(1, D, generator=g)      # a shared direction: most cosines positive
    v = torch.randn(D, generator=g)
    o14, o15 = sent[14][0], sent[15][0]
    H[o14:o14 + 40] = v + 0.3 * torch.randn(40, D, generator=g)
    H[o15:o15 + 40] = -v + 0.3 * torch.randn(40, D, generator=g)                            # every cosine of pair (14, 15) is negative
    H = H.to(BF)
    w = 0.5 + torch.rand(rows, generator=g)
    for o, L in sent:
        if L == 2:
            w[o:o + 2] = 0                        # <s></s>: an empty sentence
    pairs, floors = [], []
    for i in range(7):
        for j in range(7):
            for fp in (0, 1):
                for fr in (0, 1):
                    pairs.append((i, 7 + j)); floors.append((fp, fr))
    for fp in (0, 1):
        for fr in (0, 1):
            pairs.append((14, 15)); floors.append((fp, fr))
    for i in (0, 3, 5, 6):
        pairs.append((i, i)); floors.append((0, 0))                                       # identical hyp and ref
    return (H, torch.tensor(sent, dtype=torch.int32), torch.tensor(pairs, dtype=torch.int32), w.float(),
            torch.tensor(floors, dtype=torch.uint8))


@pytest.mark.parametrize("D", [768, 1024])
def test_match_kernel_vs_fp64(cuda, D):
    from cxrmate_amd import ops
    from cxrmate_amd._lib import LIB
    H, sent, pairs, w, floors = _match_case(D)
    m = pairs.shape[0]
    outs = [Guarded.flat(m, torch.float32) for _ in range(3)]
    Hd, sd, pd_, wd, fd = (t.cuda() for t in (H, sent, pairs, w, floors))
    LIB.call("cxr_bertscore_match", Hd.data_ptr(), H.shape[0], D, sd.data_ptr(), sent.shape[0], pd_.data_ptr(), wd.data_ptr(), fd.data_ptr(), m,
             *(o.view.data_ptr() for o in outs), ops._s())
    for o, name in zip(outs, "PRF"):
        o.check(f"bertscore_match {name}")
    got = torch.stack([o.view for o in outs], 1).cpu().double().numpy()
    want = _match_ref(H, sent, pairs, w, floors)
    both = np.isnan(want) & np.isnan(got)
    assert not (np.isnan(got) ^ np.isnan(want)).any()
    np.testing.assert_allclose(np.where(both, 0, got), np.where(both, 0, want), rtol=0, atol=1e-5)
    neg = slice(7 * 7 * 4, 7 * 7 * 4 + 4)                           # the all-negative pair: raw P / R < 0, floored to exactly 0
    assert (want[neg][0, :2] < -0.5).all() and got[neg][3, 0] == 0.0 and got[neg][3, 1] == 0.0
    assert got[neg][1, 0] < -0.5 and got[neg][1, 1] == 0.0 and got[neg][2, 0] == 0.0 and got[neg][2, 1] < -0.5
    np.testing.assert_allclose(got[-4:], 1.0, rtol=0, atol=1e-5)
    L = [n for _, n in sent.tolist()]
    empty = [k for k, (i, j) in enumerate(pairs.tolist()) if 2 in (L[i], L[j])]
    assert empty and (got[empty] == 0).all()
    P, R, F = ops.bertscore_match(Hd, sd, pd_, wd, fd)                 # the wrapper: same launch
    assert torch.equal(torch.stack([P, R, F], 1).cpu().double(), torch.from_numpy(got))
    bad = torch.tensor([[0, 10 ** 6]], dtype=torch.int32, device="cuda")    # a sentence past the buffer: NaN, nothing read
    assert torch.isnan(torch.stack(ops.bertscore_match(Hd, torch.cat([sd, bad]), torch.tensor([[0, sent.shape[0]]], dtype=torch.int32, device="cuda"),
                                                       wd, fd[:1]))).all()


# ------------------------------------------------------------------------------------------------ LayerNorm 1024 and RoBERTa embeddings
def test_layernorm_1024_vs_fp64(cuda):
    from cxrmate_amd import ops
    g = _gen(5)
    rows, C, ld = 1003, 1024, 1032
    x = (torch.randn(rows, ld, generator=g) * 2 + 0.5).to(BF)
    gam, bet = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    out = Guarded.rows(rows, C, BF, ld=ld)
    y, stats = ops.layernorm(x.cuda()[:, :C], gam.cuda(), bet.cuda(), 1e-5, need_stats=True, out=out.view)
    out.check("layernorm C=1024")
    xd = x[:, :C].double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    ref = (xd - mu) / torch.sqrt(var + 1e-5) * gam.double() + bet.double()
    assert_bf16_bracket(y, ref.numpy(), 2e-5 * (np.abs(ref.numpy()) + 1.0), "layernorm C=1024")
    np.testing.assert_allclose(stats[:, 0].cpu().double().numpy(), mu[:, 0].numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(stats[:, 1].cpu().double().numpy(), (1 / torch.sqrt(var + 1e-5))[:, 0].numpy(), rtol=2e-5)


@pytest.mark.parametrize("C", [768, 1024])
def test_roberta_embeddings_vs_fp64(cuda, C):
    from transformers.models.roberta.modeling_roberta import RobertaEmbeddings
    from cxrmate_amd import ops
    from cxrmate_amd._lib import CxrError
    g = _gen(7)
    V, NP, pad = 900, 514, 1
    word = (torch.randn(V, C, generator=g) * 0.5).to(BF)
    typ = (torch.randn(1, C, generator=g) * 0.5).to(BF)
    posw = (torch.randn(NP, C, generator=g) * 0.5).to(BF)
    gam, bet = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    B, T = 5, 512
    ids = torch.randint(3, V, (B, T), generator=g)
    for b, L in enumerate([512, 1, 2, 300, 65]):                    # right padding
        ids[b, L:] = pad
    ids[3, 7] = pad                                                 # a pad id inside a sentence keeps its padding position
    tabs = [t.cuda() for t in (word, typ, posw, gam, bet)]
    out, pos = ops.roberta_embed(ids.cuda(), *tabs[:3], tabs[3], tabs[4], 1e-5, pad, pos_out=True)
    want_pos = RobertaEmbeddings.create_position_ids_from_input_ids(ids, pad)
    assert torch.equal(pos.cpu(), want_pos)
    s = word.double()[ids] + typ.double()[0] + posw.double()[want_pos]
    mu = s.mean(-1, keepdim=True)
    var = ((s - mu) ** 2).mean(-1, keepdim=True)
    ref = ((s - mu) / torch.sqrt(var + 1e-5) * gam.double() + bet.double()).reshape(B * T, C).numpy()
    assert_bf16_bracket(out, ref, 2e-5 * (np.abs(ref) + 1.0), f"roberta embeddings C={C}")
    with pytest.raises(CxrError):                                   # positions would run past the table
        ops.roberta_embed(torch.full((1, 513), 5, dtype=torch.int64, device="cuda"), *tabs, 1e-5, pad)
    bad = ids[:1, :4].clone()
    bad[0, 2] = V                                                   # an id past the table: that row is NaN, the others are not
    o = ops.roberta_embed(bad.cuda(), *tabs, 1e-5, pad).float().cpu()
    assert torch.isnan(o[2]).all() and torch.isfinite(o[[0, 1, 3]]).all()


# ------------------------------------------------------------------------------------------------ trunk
def _small_cfg(layers, vocab=1000):
    from cxrmate_amd.bertscore import roberta_large_config
    cfg = roberta_large_config(layers)
    cfg.vocab_size = vocab
    return cfg


def _padded_batch(lens, vocab, seed):
    g = _gen(seed)
    ids = torch.full((len(lens), max(lens)), 1, dtype=torch.int64)
    mask = torch.zeros(len(lens), max(lens), dtype=torch.int64)
    for b, L in enumerate(lens):
        ids[b, :L] = torch.randint(3, vocab, (L,), generator=g)
        ids[b, 0], ids[b, L - 1] = 0, 2
        mask[b, :L] = 1
    return ids, mask


def _valid_rel(h, ref, mask):
    m = mask.bool()
    return gu.rel_rms(h.float().cpu()[m].numpy(), ref[m].numpy())


def test_roberta_trunk_vs_transformers(cuda):
    from cxrmate_amd import weights
    from cxrmate_amd.bertscore import RobertaScorer, roberta_param_shapes
    cfg = _small_cfg(3)
    sc = RobertaScorer(cuda, config=cfg, num_layers=3, seed=11)
    sd = {k: v.detach().float().cpu() for k, v in sc.model.state_dict().items()}
    hf = bref.hf_roberta(cfg, sd)
    ids, mask = _padded_batch([37, 5, 129, 64], cfg.vocab_size, 1)
    h, _ = sc.engine.forward(ids.cuda(), attn_mask=mask.to(torch.uint8).cuda(), causal=False, lm_head=False, train=False)
    with torch.no_grad():
        ref = hf(ids, attention_mask=mask).last_hidden_state
    rel = _valid_rel(h, ref, mask)
    assert rel < 2.5e-2, rel
    # a 4-layer RoBERTa checkpoint (HF names, `roberta.` prefix, pooler) loaded with num_layers=3 == the oracle's hidden_states[3]
    cfg4 = _small_cfg(4)
    sd4 = weights.init_state_dict(roberta_param_shapes(cfg4), seed=12, std=0.02, perturb=0.05)
    hf4 = bref.hf_roberta(cfg4, sd4)
    ck = {"roberta." + k: v for k, v in hf4.state_dict().items()}
    ck["roberta.pooler.dense.weight"] = torch.zeros(1024, 1024)
    sc3 = RobertaScorer(cuda, config=_small_cfg(3), num_layers=3, state_dict=ck)
    h3, _ = sc3.engine.forward(ids.cuda(), attn_mask=mask.to(torch.uint8).cuda(), causal=False, lm_head=False, train=False)
    with torch.no_grad():
        ref3 = hf4(ids, attention_mask=mask, output_hidden_states=True).hidden_states[3]
    rel3 = _valid_rel(h3, ref3, mask)
    print(f"trunk rel-RMS vs RobertaModel: {rel:.2e}; 4-layer checkpoint at 3 layers: {rel3:.2e}")
    assert rel3 < 2.5e-2, rel3


# ------------------------------------------------------------------------------------------------ scorer end to end
WORDS = "the lungs are clear no pleural effusion or pneumothorax heart size is normal mild cardiomegaly stable support devices".split()


def _sentences(seed):
    g = np.random.default_rng(seed)
    s = lambda n: " ".join(g.choice(WORDS, n))
    long_text = s(700)                                              # 700 words -> truncated to 512 tokens
    cands = [s(12), "", s(30), s(12), long_text, s(3), " " + s(8) + "  ", s(50), s(1)]
    refs = [s(10), s(9), s(30), s(20), s(40), long_text, s(8), s(2), s(1)]
    cands[3] = cands[0]                                             # a duplicated candidate
    refs[6] = cands[6].strip()                                      # a reference equal to a candidate once stripped (a different key)
    return cands, refs


def _restated_bertscore(sc, hf, cands, refs, batch_size):
    uniq = list(dict.fromkeys(list(refs) + list(cands)))
    toks = [sc.tokenize(s) for s in uniq]
    idf = lambda i: 0.0 if i in (0, 2) else 1.0
    stats = dict(zip(uniq, bref.trunk_stats(hf, toks, idf)))
    return bref.bert_cos_score(stats, refs, cands, batch_size), toks


@pytest.mark.parametrize("batch_size", [2, 4])
def test_scorer_vs_restated_bert_score(cuda, batch_size):
    from cxrmate_amd.bertscore import RobertaScorer
    cfg = _small_cfg(3)
    base = (0.83, 0.84, 0.835)
    sc = RobertaScorer(cuda, tokenizer=bref.WordTokenizer(cfg.vocab_size), config=cfg, num_layers=3, seed=21, baseline=base)
    hf = bref.hf_roberta(cfg, {k: v.detach().float().cpu() for k, v in sc.model.state_dict().items()})
    cands, refs = _sentences(batch_size)
    (P0, R0, F0), toks = _restated_bertscore(sc, hf, cands, refs, batch_size)
    assert max(len(t) for t in toks) == 512
    P, R, F = sc.score_raw(cands, refs, batch_size=batch_size)
    print(f"raw P/R/F max |err| vs the restated pipeline: {float((torch.stack([P, R, F]).double() - torch.stack([P0, R0, F0])).abs().max()):.2e}")
    # tolerance: the bf16 trunk's hidden states are within ~6.5e-3 rel-RMS of fp32 (the trunk test). The maxima of cosines of such vectors and
    # their weighted means moved by at most 4.4e-4 on an MI355X; 5e-3 on the raw values leaves 10x, and the rescale divides that by 1 - b ~ 0.16
    np.testing.assert_allclose(torch.stack([P, R, F]).numpy(), torch.stack([P0, R0, F0]).numpy(), rtol=0, atol=5e-3)
    assert P[1] == 0 and R[1] == 0 and F[1] == 0                    # the empty candidate
    Ps, Rs, Fs = sc.score(cands, refs, batch_size=batch_size)
    b = torch.tensor(base)
    for k, (x, x0) in enumerate(((Ps, P0), (Rs, R0), (Fs, F0))):
        np.testing.assert_allclose(x.numpy(), bref.rescale(x0.float(), b[k]).numpy(), rtol=0, atol=5e-3 / (1 - 0.84))
        np.testing.assert_allclose(x.numpy(), ((torch.stack([P, R, F])[k] - b[k]) / (1 - b[k])).numpy(), rtol=0, atol=1e-6)
    sc.baseline = None
    with pytest.raises(RuntimeError, match="roberta-large.tsv"):
        sc.score(cands, refs)


# ------------------------------------------------------------------------------------------------ metric flow
def test_bertscore_metric_matches_reference_flow(cuda, tmp_path):
    import glob
    import os
    import pandas as pd
    from cxrmate_amd.bertscore import BERTScoreRoBERTaLarge, RobertaScorer
    cfg = _small_cfg(2)
    sc = RobertaScorer(cuda, tokenizer=bref.WordTokenizer(cfg.vocab_size), config=cfg, num_layers=2, seed=31, baseline=(0.8, 0.8, 0.8))
    metric = BERTScoreRoBERTaLarge("test", None, 2, str(tmp_path), accumulate_over_dicoms=True, num_workers=4, scorer=sc)
    preds = ["the lungs are clear", "mild cardiomegaly is stable", "no pleural effusion", "the lungs are clear", "normal"]
    labels = [["the lungs are clear"], ["no acute process"], ["small left pleural effusion"], ["normal"], ["normal"]]
    metric.update(preds[:3], labels[:3], [10, 10, 11], ["a", "b", "c"])
    metric.update(preds[3:], labels[3:], [12, 12], ["d", "d"])                     # duplicated dicom (DDP padding) is dropped
    with pytest.raises(AssertionError):
        metric.update("not a list", labels, [1], ["x"])
    out = metric.compute(epoch=3)
    files = glob.glob(os.path.join(str(tmp_path), "bertscore", "test_epoch-3_scores_*.csv"))
    assert len(files) == 1
    df = pd.read_csv(files[0])
    assert list(df.columns) == ["dicom_id", "study_id", "f1", "precision", "recall"] and len(df) == 4
    assert list(df.dicom_id) == ["a", "b", "c", "d"]
    P, R, F = sc.score(preds, [l[0] for l in labels], batch_size=2)
    np.testing.assert_allclose(df.f1.to_numpy(), F[:4].double().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(df.precision.to_numpy(), P[:4].double().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(df.recall.to_numpy(), R[:4].double().numpy(), rtol=0, atol=1e-6)
    for name, col in (("f1", F), ("precision", P), ("recall", R)):
        v = col[:4].double().numpy()
        assert abs(out[name] - np.mean([np.mean(v[:2]), v[2], v[3]])) < 1e-6, name
    assert set(out) == {"f1", "precision", "recall"} and all(isinstance(v, float) for v in out.values())
    metric.reset()
    assert metric.reports == []
    m2 = BERTScoreRoBERTaLarge("val", None, 3, str(tmp_path), accumulate_over_dicoms=False, num_workers=0, scorer=sc)
    m2.update(preds, labels, [1, 2, 3, 4, 4])
    out2 = m2.compute(epoch=0)
    df2 = pd.read_csv(glob.glob(os.path.join(str(tmp_path), "bertscore", "val_epoch-0_scores_*.csv"))[0])
    assert list(df2.columns) == ["study_id", "f1", "precision", "recall"] and len(df2) == 4
    assert abs(out2["f1"] - df2.f1.mean()) < 1e-9


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_roberta_large_17_layers(cuda):
    from cxrmate_amd.bertscore import RobertaScorer
    sc = RobertaScorer(cuda, tokenizer=bref.WordTokenizer(50265), seed=41, baseline=(0.83, 0.84, 0.835))
    assert sc.config.num_hidden_layers == 17 and sc.config.hidden_size == 1024
    g = np.random.default_rng(0)
    n = [int(x) for x in g.integers(1, 700, 64)]
    n[0], n[1] = 700, 510                                           # two at the 512-token limit
    reps = [" ".join(g.choice(WORDS, k)) for k in n]
    cands, refs = reps[:32] * 2, reps[32:] + reps[:32]
    P, R, F = sc.score_raw(cands, refs, batch_size=16)
    assert all(torch.isfinite(x).all() for x in (P, R, F))
    P2, R2, F2 = sc.score_raw(cands, refs, batch_size=16, embed_batch_size=5)          # other embedding mini-batches, same pair chunks
    print(f"full size: F mean {float(F[:32].mean()):.4f}; max |change| with other embedding mini-batches "
          f"{float((torch.stack([P2, R2, F2]) - torch.stack([P, R, F])).abs().max()):.2e}")
    # a sentence's hidden states do not depend on its batch mates (key padding); only the GEMM / attention tiling of the bf16 kernels changes
    np.testing.assert_allclose(torch.stack([P2, R2, F2]).numpy(), torch.stack([P, R, F]).numpy(), rtol=0, atol=3e-3)
    np.testing.assert_allclose(F[32:].numpy(), 1.0, rtol=0, atol=1e-5)                 # the second half pairs every report with itself
