"""GPU: the per-step outputs of generate() -- `scores`, `logits`, `beam_indices` (output_scores / output_logits) -- and compute_transition_scores,
against tests/golden/gen_scores.npz (transformers 5.15.0 through the reference's models, tests/golden/make_golden_gen_scores.py).

  record kernel (csrc/gen_record.hip)   : copies bit-exact, log_softmax against torch, -inf entries, the beam-major -> study-major permutation
  cxr_beam_step_idx (csrc/decode.hip)    : the same search as cxr_beam_step(_lp) bit for bit, histories equal to a torch restatement of TF5
  model vs fixture                       : sequences and beam_indices exact (the fixture's decisions clear the bf16 error bound); scores, logits
                                           and transition scores within 3 x the bf16 logit error (1.2 % of a step's score spread)
"""
import math

import numpy as np
import pytest
import torch

import golden_util as gu
from cxrmate_amd.config import tiny_config

pytestmark = pytest.mark.gpu

ERR_REL = 0.012           # bf16 logit error relative to the spread of a step's scores (test_gen_controls_gpu.py)
SHARPEN_SUFFIXES = ("cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias")
FLAGS = dict(return_dict_in_generate=True, output_scores=True, output_logits=True)


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import modelling
    return modelling


@pytest.fixture(scope="module")
def G():
    return gu.load("gen_scores.npz")


# ------------------------------------------------------------------------------------------------ record kernel
@pytest.mark.parametrize("V,ld,nb", [(30000, 30000, 4), (30000, 30016, 1), (1000, 1000, 2), (997, 1001, 3)])
def test_record_kernel_matches_torch(M, V, ld, nb):
    from cxrmate_amd import ops
    g = torch.Generator().manual_seed(V + nb)
    R = 6 * nb
    base = torch.randn(R, ld, generator=g) * 4.0
    ban = torch.rand(R, ld, generator=g) < 0.05
    base = base.masked_fill(ban, float("-inf"))
    base[1, 1:] = float("-inf")                                          # one finite entry only
    x = base.cuda()[:, :V]                                               # row stride ld
    perm = torch.arange(R).view(nb, R // nb).t().reshape(-1)             # output row s * nb + b <- input row b * (R // nb) + s
    ref_x = x.cpu()[perm]
    lo, so = torch.full((R, V), 7.0, device="cuda"), torch.full((R, V), 7.0, device="cuda")
    ops.gen_record(x, lo, so, log_softmax=True, nb=nb)
    assert torch.equal(lo.cpu(), ref_x)
    want = torch.log_softmax(ref_x.double(), -1).float()
    got = so.cpu()
    assert torch.equal(torch.isinf(got), torch.isinf(want))
    fin = torch.isfinite(want)
    torch.testing.assert_close(got[fin], want[fin], rtol=1e-6, atol=2e-5)
    for log_softmax in (False, True):                                    # each output alone
        so2 = torch.zeros((R, V), device="cuda")
        ops.gen_record(x, None, so2, log_softmax=log_softmax, nb=nb)
        assert torch.equal(so2.cpu(), ref_x if not log_softmax else got)
    lo2 = torch.zeros((R, V), device="cuda")
    ops.gen_record(x, lo2, None, nb=nb)
    assert torch.equal(lo2.cpu(), ref_x)


# ------------------------------------------------------------------------------------------------ beam step with beam-index histories
def _restate_step(st, lp_rows, cur, P, L, eos, lp, nb):
    """TF5 _beam_search bookkeeping (generation/utils.py:3411-3470) in torch, study-major, on log-probs lp_rows [B * nb, V]."""
    B = st["run"].shape[0]
    V = lp_rows.shape[1]
    keep = 2 * nb

    def gather(t, idx):
        while idx.dim() < t.dim():
            idx = idx.unsqueeze(-1)
        return torch.gather(t, 1, idx.expand(-1, -1, *t.shape[2:]))
    acc = (lp_rows.view(B, nb, V) + st["rs"][:, :, None]).reshape(B, nb * V)
    topk_lp, topk_idx = torch.topk(acc, keep)
    beam_of = topk_idx // V
    off = (torch.arange(B, device=acc.device) * nb).view(B, 1)
    topk_seq = gather(st["run"], beam_of)
    topk_seq[:, :, cur] = topk_idx % V
    topk_bidx = gather(st["rb"], beam_of)
    topk_bidx[:, :, cur] = (beam_of + off).int()
    hits = (topk_seq[:, :, cur] == eos) | (cur + 1 >= L)
    run_lp = topk_lp + hits.float() * -1.0e9
    nxt = torch.topk(run_lp, k=nb)[1]
    st["run"], st["rs"], st["rb"] = gather(topk_seq, nxt), gather(run_lp, nxt), gather(topk_bidx, nxt)
    just = hits & (torch.arange(keep, device=acc.device) < nb)[None]
    fin_lp = topk_lp / ((cur + 1 - P) ** lp) + (~st["unsat"]).float() * -1.0e9 + (~just).float() * -1.0e9
    best = torch.topk(torch.cat((st["bs"], fin_lp), 1), k=nb)[1]
    st["seq"] = gather(torch.cat((st["seq"], topk_seq), 1), best)
    st["fb"] = gather(torch.cat((st["fb"], topk_bidx), 1), best)
    st["fin"] = gather(torch.cat((st["fin"], just), 1), best)
    st["bs"] = gather(torch.cat((st["bs"], fin_lp), 1), best)
    best_run = st["rs"][:, :1] / ((cur + 1 - P) ** lp)
    worst = torch.where(st["fin"], st["bs"].min(1, keepdim=True)[0], torch.full_like(st["bs"], -1.0e9))
    st["unsat"] = st["unsat"] & torch.any(best_run > worst, dim=-1, keepdim=True)
    return bool(st["unsat"].any()) and not bool(hits.all())


def _device_state(B, nb, L, P, pad, dev="cuda"):
    run = torch.full((nb, B, L), pad, dtype=torch.int64, device=dev)
    run[:, :, :P] = gu.BOS
    rs = torch.zeros((B, nb), device=dev)
    rs[:, 1:] = -1.0e9
    return dict(run=run, seq=run.clone(), rs=rs, bs=torch.full((B, nb), -1.0e9, device=dev), fin=torch.zeros((B, nb), dtype=torch.uint8, device=dev),
                unsat=torch.ones((2, B), dtype=torch.int32, device=dev), hit=torch.zeros((2, B), dtype=torch.int32, device=dev),
                idx=torch.zeros(nb * B, dtype=torch.int64, device=dev))


@pytest.mark.parametrize("nb,V,logprobs,lp", [(4, 30000, False, 1.0), (4, 5000, True, 2.0), (2, 9001, False, 0.5)])
def test_beam_step_idx_equals_beam_step_and_restatement(M, nb, V, logprobs, lp):
    from cxrmate_amd import ops
    B, L, P, eos = 3, 16, 1, gu.EOS
    g = torch.Generator().manual_seed(nb * 7 + V)
    plain, idx = _device_state(B, nb, L, P, gu.PAD), _device_state(B, nb, L, P, gu.PAD)
    rb = torch.full((nb, B, L), -1, dtype=torch.int32, device="cuda")
    fb = rb.clone()
    ref = dict(run=plain["run"].permute(1, 0, 2).clone(), seq=plain["seq"].permute(1, 0, 2).clone(), rs=plain["rs"].clone(), bs=plain["bs"].clone(),
               fin=torch.zeros((B, nb), dtype=torch.bool, device="cuda"), unsat=torch.ones((B, 1), dtype=torch.bool, device="cuda"),
               rb=rb.permute(1, 0, 2).clone(), fb=fb.permute(1, 0, 2).clone())
    going = True
    for cur in range(P, L):
        x = torch.randn((B * nb, V), generator=g) * 3.0
        x[:, eos] = 3.0 * math.sqrt(2 * math.log(V)) - 6.0 + 0.6 * (cur - P)     # EOS rises to the row maximum: hypotheses end at different steps
        xs = torch.log_softmax(x, -1) if logprobs else x                  # study-major rows
        bm = xs.view(B, nb, V).transpose(0, 1).reshape(B * nb, V).contiguous().cuda()
        div = float(cur + 1 - P) ** lp
        ops.beam_step(bm.clone(), plain["run"], plain["seq"], plain["rs"], plain["bs"], plain["fin"], plain["unsat"], plain["hit"], plain["idx"], cur, L,
                      eos, div, logprobs=logprobs)
        ops.beam_step(bm.clone(), idx["run"], idx["seq"], idx["rs"], idx["bs"], idx["fin"], idx["unsat"], idx["hit"], idx["idx"], cur, L, eos, div,
                      logprobs=logprobs, bidx=(rb, fb))
        for k in plain:
            assert torch.equal(plain[k], idx[k]), (cur, k)
        if going:
            going = _restate_step(ref, torch.log_softmax(xs.cuda(), -1), cur, P, L, eos, lp, nb)
            # running beams that can still continue, and finished hypotheses (slots at -1e9 are ties between ended continuations / empty slots)
            live, fin = ref["rs"] > -1.0e8, ref["fin"]
            assert torch.equal(ref["fin"], idx["fin"].bool()), cur
            assert torch.equal(ref["run"][live], idx["run"].permute(1, 0, 2)[live]), cur
            assert torch.equal(ref["rb"][live], rb.permute(1, 0, 2)[live]), (cur, ref["rb"], rb.permute(1, 0, 2))
            assert torch.equal(ref["seq"][fin], idx["seq"].permute(1, 0, 2)[fin]), cur
            assert torch.equal(ref["fb"][fin], fb.permute(1, 0, 2)[fin]), (cur, ref["fb"], fb.permute(1, 0, 2))
    assert bool((fb[:, :, :P] == -1).all())
    assert bool((fb >= 0).any()) and bool((fb[:, :, P:] < 0).any())           # some hypothesis ended before max_length


# ------------------------------------------------------------------------------------------------ models of the fixture
def _recipe(G, name):
    seed, pixel_seed, vocab, max_length = (int(v) for v in G[f"{name}_cfg"])
    sharpen, cross_gain, img_off, perturb, eos_bias = (float(v) for v in G[f"{name}_f"])
    return dict(seed=seed, pixel_seed=pixel_seed, vocab=vocab, max_length=max_length, sharpen=sharpen, cross_gain=cross_gain, img_off=img_off,
                perturb=perturb, eos_bias=eos_bias)


def model_case(M, G, name):
    c = _recipe(G, name)
    kw = dict(bos_token_id=gu.BOS, eos_token_id=gu.EOS, pad_token_id=gu.PAD, max_length=c["max_length"])
    if name[0] == "l":
        from cxrmate_amd import weights
        cfg = tiny_config(vocab_size=c["vocab"], decoder_layers=2, image_size=96, lora_r=8)
        sd = weights.init_encoder_decoder(cfg, seed=c["seed"], perturb=c["perturb"])
        for k in list(sd):
            if "crossattention.output.dense." in k:
                sd[k] = sd[k] * c["cross_gain"]
            if k.endswith(SHARPEN_SUFFIXES):
                sd[k] = sd[k] * c["sharpen"]
        m = M.LongitudinalPromptMultiCXREncoderDecoderModel(cfg, seed=None)
        m.load_state_dict(sd)
        gen = torch.Generator().manual_seed(c["pixel_seed"])
        x = torch.randn(2, 2, 3, 96, 96, generator=gen)
        x[0, 1] = 0.0
        with torch.no_grad():
            eo = m.encoder(x.cuda())
        pen, n = G["lg_opts"]
        return m, dict(kw, encoder_outputs=eo, decoder_input_ids=torch.from_numpy(G["lg_prompt"]).cuda(), special_token_ids=[gu.PMT_SEP, gu.BOS, gu.SEP],
                       mask_token_id=gu.PAD, repetition_penalty=float(pen), no_repeat_ngram_size=int(n)), 1 + G["lg_prompt"].shape[1]
    cfg = tiny_config(vocab_size=c["vocab"], decoder_layers=2, image_size=96)
    sd = gu.sharpened_state(cfg, c["seed"], c["perturb"], c["sharpen"], c["cross_gain"])
    if name[0] == "s":
        m = M.SingleCXREncoderDecoderModel(cfg, seed=None)
        x = torch.randn(3, 3, 96, 96, generator=torch.Generator().manual_seed(c["pixel_seed"]))
    else:
        m = M.MultiCXREncoderDecoderModel(cfg, seed=None)
        x = gu.distinct_study_pixels(c["pixel_seed"], c["img_off"])
    m.load_state_dict(sd)
    if c["eos_bias"]:
        with torch.no_grad():
            m.param("decoder.cls.predictions.bias")[gu.EOS] += c["eos_bias"]
    return m, dict(kw, pixel_values=x.cuda(), special_token_ids=[gu.SEP]), 1


def fixture_steps(G, name):
    """-> (scores, logits, keep) of the case as the reference returned them. Greedy: [steps, rows, V] each (scores = logits with the processed
    entries written in); keep None. Beam: [kept rows, V] each, scores = log_softmax(logits), and keep [steps, rows], the rows the returned
    hypotheses were chosen from (which slot holds a running beam that is not returned is not pinned by the fixture's robustness check: near-ties
    among such beams may sit in either slot)."""
    logits = torch.from_numpy(G[f"{name}_logits"])
    if f"{name}_keep" in G.files:
        return torch.log_softmax(logits, -1), logits, torch.from_numpy(G[f"{name}_keep"])
    scores = logits.clone()
    if f"{name}_changed_idx" in G.files:
        scores.view(-1)[torch.from_numpy(G[f"{name}_changed_idx"])] = torch.from_numpy(G[f"{name}_changed_val"])
    return scores, logits, None


def close_rows(got, ref, what, keep=None, factor=1.0):
    """-inf pattern equal, finite entries within factor x 3 x the bf16 logit error of the reference row's spread. got [steps, rows, V]; ref the
    same, or [kept rows, V] with keep [steps, rows]."""
    got, ref = got.double(), ref.double()
    if keep is not None:
        assert got.shape[:2] == keep.shape, (what, got.shape, keep.shape)
        got = got[keep]
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(fin, torch.isfinite(got)), what
    z = torch.where(fin, ref, torch.zeros_like(ref))
    mean = z.sum(-1, keepdim=True) / fin.sum(-1, keepdim=True)
    std = (torch.where(fin, (ref - mean) ** 2, torch.zeros_like(ref)).sum(-1, keepdim=True) / fin.sum(-1, keepdim=True)).sqrt()
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    worst = float((err / (factor * 3 * ERR_REL * std)).max())
    assert worst <= 1.0, (what, worst)


def check_against_fixture(m, G, name, out, n=None):
    """Per-step tuples of the case (a beam search's do not depend on num_return_sequences), sequences, beam indices and transition scores of
    the call (num_return_sequences n)."""
    k = name if n is None else f"{name}_n{n}"
    seq = out["sequences"].cpu()
    assert torch.equal(seq, torch.from_numpy(G[f"{k}_seq"])), (k, seq, G[f"{k}_seq"])
    ref_scores, ref_logits, keep = fixture_steps(G, name)
    steps = keep.shape[0] if keep is not None else ref_scores.shape[0]
    assert len(out["scores"]) == len(out["logits"]) == steps, (k, len(out["scores"]), len(out["logits"]), steps)
    beam = "beam_indices" in out
    # beam scores are log-probs: the error of an entry plus that of the row's log-sum-exp (about the error of its maximum)
    close_rows(torch.stack(out["scores"]).cpu(), ref_scores, (k, "scores"), keep, factor=2.0 if beam else 1.0)
    close_rows(torch.stack(out["logits"]).cpu(), ref_logits, (k, "logits"), keep)
    for t in out["logits"]:
        assert t.dtype == torch.float32 and not t.requires_grad
    fin = ref_scores[torch.isfinite(ref_scores)]
    std = float(fin.abs().std())
    if "beam_indices" in out:
        assert out["beam_indices"].dtype == torch.int32
        assert torch.equal(out["beam_indices"].cpu(), torch.from_numpy(G[f"{k}_bidx"])), (k, out["beam_indices"], G[f"{k}_bidx"])
        np.testing.assert_allclose(out["sequences_scores"].cpu().numpy(), G[f"{k}_seq_scores"], atol=3 * ERR_REL * std)
    ts = m.compute_transition_scores(out["sequences"], out["scores"], out.get("beam_indices"))
    np.testing.assert_allclose(ts.cpu().numpy(), G[f"{k}_ts"], atol=6 * ERR_REL * std)


def run(m, kw, **extra):
    return m.generate(**dict(kw, **extra))


@pytest.mark.parametrize("name", ["mg", "sg", "lg"])
def test_greedy_matches_fixture(M, G, name):
    m, kw, P = model_case(M, G, name)
    for graph in (True, False):
        m.graph_decode = graph
        out = run(m, kw, num_beams=1, **FLAGS)
        check_against_fixture(m, G, name, out)
        assert list(out.keys()) == ["sequences", "scores", "logits"]
    m.graph_decode = True
    if name == "lg":                                                       # processors: scores are not the raw logits
        assert not torch.equal(torch.stack(out["scores"]), torch.stack(out["logits"]))
    else:                                                                  # no processor: scores[t] == logits[t]
        assert all(torch.equal(s, l_) for s, l_ in zip(out["scores"], out["logits"]))


@pytest.mark.parametrize("name,ns", [("mb", (1, 2, 4)), ("sb", (1,))])
def test_beam_matches_fixture_device_host_and_eager(M, G, name, ns):
    m, kw, P = model_case(M, G, name)
    got = {}
    for dev, graph in ((True, True), (True, False), (False, True)):
        m.device_beam_search, m.graph_decode = dev, graph
        for n in ns:
            out = run(m, kw, num_beams=4, num_return_sequences=n, **FLAGS)
            assert list(out.keys()) == ["sequences", "sequences_scores", "scores", "logits", "beam_indices"]
            check_against_fixture(m, G, name, out, n)
            got[(dev, graph, n)] = out
    m.device_beam_search, m.graph_decode = True, True
    for n in ns:                                                           # device (graph / eager) and host loop: the same indices
        a = got[(True, True, n)]
        for other in ((True, False, n), (False, True, n)):
            assert torch.equal(a["beam_indices"], got[other]["beam_indices"]), (n, other)
            assert torch.equal(a["sequences"], got[other]["sequences"]), (n, other)
        assert torch.equal(torch.stack(a["scores"]), torch.stack(got[(True, False, n)]["scores"]))     # graph replay == eager launches


@pytest.mark.parametrize("name,lp", [("mb", 1.0), ("sb", 1.0), ("sb", 2.0), ("sb", 0.5)])
def test_transition_scores_reproduce_sequences_scores(M, G, name, lp):
    m, kw, P = model_case(M, G, name)
    for dev in (True, False):
        m.device_beam_search = dev
        out = run(m, dict(kw, max_length=14), num_beams=4, num_return_sequences=4, length_penalty=lp, **FLAGS)
        ts = m.compute_transition_scores(out["sequences"], out["scores"], out["beam_indices"])
        lens = (out["beam_indices"] >= 0).sum(1).double()
        torch.testing.assert_close(ts.double().sum(1) / lens ** lp, out["sequences_scores"].double(), rtol=1e-5, atol=1e-4)
        assert out["beam_indices"].shape == (out["sequences"].shape[0], out["sequences"].shape[1] - P)
    m.device_beam_search = True


def test_lengths_follow_eos_trimming(M, G):
    """The 8-step EOS polling overshoots by up to 16 steps: the tuples are trimmed to the returned steps, in greedy and in sampling."""
    m, kw, P = model_case(M, G, "mg")
    for extra in (dict(), dict(do_sample=True, top_k=5)):
        torch.manual_seed(3)
        out = m.generate(**dict(kw, max_length=60), num_beams=1, **FLAGS, **extra)
        steps = out["sequences"].shape[1] - P
        assert len(out["logits"]) == steps and len(out["scores"]) == steps
        if not extra:                                                   # greedy: every row of the case ends, the last on the last step
            gen = out["sequences"][:, P:]
            assert steps < 59 and bool((gen == gu.EOS).any(1).all()) and int((gen == gu.EOS).int().argmax(1).max()) == steps - 1


def test_flags_do_not_change_sequences(M, G):
    m, kw, P = model_case(M, G, "mb")
    kw = dict(kw, max_length=14)
    base = m.generate(**kw, num_beams=1)
    assert torch.equal(m.generate(**kw, num_beams=1, **FLAGS)["sequences"], base)
    for seed in (1, 2):
        torch.manual_seed(seed)
        s0 = m.generate(**kw, num_beams=1, do_sample=True, top_k=20, num_return_sequences=2)
        torch.manual_seed(seed)
        s1 = m.generate(**kw, num_beams=1, do_sample=True, top_k=20, num_return_sequences=2, return_dict_in_generate=True, output_logits=True)
        assert torch.equal(s0, s1["sequences"])
        assert len(s1["logits"]) == s1["sequences"].shape[1] - P and s1["logits"][0].shape == (6, int(G["mb_cfg"][2]))
    for dev in (True, False):
        m.device_beam_search = dev
        b0 = m.generate(**kw, num_beams=4, return_dict_in_generate=True, output_scores=False)
        b1 = m.generate(**kw, num_beams=4, **FLAGS)
        assert torch.equal(b0["sequences"], b1["sequences"])
        assert list(b0.keys()) == ["sequences", "sequences_scores"] and b0["sequences_scores"] is None
    m.device_beam_search = True
    g0 = m.generate(**kw, num_beams=1, return_dict_in_generate=True, output_scores=True)
    assert list(g0.keys()) == ["sequences", "scores"] and len(g0["scores"]) == g0["sequences"].shape[1] - P


def test_sampled_logits_are_raw_study_major_and_carry_no_gradient(M, G):
    """top_k = 1 sampling draws the argmax: every sample of a study repeats the greedy decode, so the study-major logits rows b * n + j are the
    greedy logits of study b; under generate.__wrapped__ the logits carry no gradient while the sampled scores still do."""
    m, kw, P = model_case(M, G, "mg")
    greedy = m.generate(**kw, num_beams=1, **FLAGS)
    n = 2
    out = m.generate.__wrapped__(m, **kw, num_beams=1, do_sample=True, top_k=1, num_return_sequences=n, **FLAGS)
    assert torch.equal(out["sequences"], greedy["sequences"].repeat_interleave(n, 0))
    assert len(out["logits"]) == len(greedy["logits"])
    for a, b in zip(out["logits"], greedy["logits"]):
        assert not a.requires_grad
        std = float(b.std())
        torch.testing.assert_close(a, b.repeat_interleave(n, 0), rtol=0, atol=3 * ERR_REL * std)


def test_flagged_greedy_is_not_served_by_the_speculative_baseline(M, G):
    """The SCST pair (sampling with scores, then greedy over the same inputs) is unchanged; a greedy call that asks for scores or logits decodes
    by itself and returns them."""
    m, kw, P = model_case(M, G, "lg")
    base = dict(kw)
    for k in ("repetition_penalty", "no_repeat_ngram_size"):
        base.pop(k)
    torch.manual_seed(0)
    m.generate(**base, num_beams=1, do_sample=True, output_scores=True, return_dict_in_generate=True, top_k=50)
    plain = m.generate(**base, num_beams=1)
    torch.manual_seed(0)
    m.generate(**base, num_beams=1, do_sample=True, output_scores=True, return_dict_in_generate=True, top_k=50)
    flagged = m.generate(**base, num_beams=1, **FLAGS)
    assert torch.equal(flagged["sequences"], plain)
    assert len(flagged["scores"]) == len(flagged["logits"]) == plain.shape[1] - P
