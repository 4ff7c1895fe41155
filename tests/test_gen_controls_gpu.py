"""GPU: the generation controls of generate() (repetition_penalty, no_repeat_ngram_size, min_length, min_new_tokens, num_return_sequences) against
tests/golden/gen_controls.npz (transformers 5.15.0 processors and the reference's own generate, tests/golden/make_golden_gen_controls.py).

  kernel (csrc/logits_proc.hip) : -inf pattern exact, penalised values bit-exact (the library divides, so does the kernel)
  greedy                        : identical up to the first step whose processed top-1/top-2 margin is below 3 x the bf16 logit error (1.2 % of
                                  the step's score spread, test_model_gpu.py rule for the sharpened fixtures)
  beam-4                        : the best hypothesis of every study and its score (a case robust under bf16-sized logit noise); the lower
                                  returned hypotheses are not robust: ranked below it, and where one equals the reference's, with its score
"""
import numpy as np
import pytest
import torch

import golden_util as gu
from cxrmate_amd.config import tiny_config

pytestmark = pytest.mark.gpu

ERR_REL = 0.012           # bf16 logit error relative to the spread of a step's scores
SHARPEN_SUFFIXES = ("cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import modelling
    return modelling


@pytest.fixture(scope="module")
def G():
    return gu.load("gen_controls.npz")


def restate(x, ids, cur, eos, penalty, n, min_length):
    """torch restatement of the three processors (TF5 order) on fp32 rows x [R, V], history ids[:, :cur]."""
    x = x.clone()
    h = ids[:, :cur]
    if penalty != 1.0 and cur > 0:
        s = torch.gather(x, 1, h)
        x.scatter_(1, h, torch.where(s < 0, s * penalty, s / penalty))
    if n > 0 and cur >= n:
        win = h.unfold(1, n, 1)                                          # [R, cur - n + 1, n]
        match = (win[..., :-1] == h[:, cur - n + 1:].unsqueeze(1)).all(-1)
        ban = torch.zeros((x.shape[0], x.shape[1] + 1), dtype=torch.bool, device=x.device)
        ban.scatter_(1, torch.where(match, win[..., -1], x.shape[1]), True)
        x = x.masked_fill(ban[:, :-1], float("-inf"))
    if cur < min_length and eos >= 0:
        x[:, eos] = float("-inf")
    return x


def test_kernel_matches_fixture(M, G):
    from cxrmate_amd import ops
    for i in range(int(G["n_kernel_cases"])):
        seed, R, V, cur, n, mlen, plen, mnew, lp = (int(v) for v in G[f"k{i}_params"])
        pen = float(G[f"k{i}_penalty"])
        x = torch.randn(R, V, generator=torch.Generator().manual_seed(seed)) * 3.0
        if lp:
            x = torch.log_softmax(x, dim=-1)
        want = x.clone().reshape(-1)
        want[torch.from_numpy(G[f"k{i}_changed_idx"])] = torch.from_numpy(G[f"k{i}_changed_val"])
        want = want.view(R, V)
        ids = torch.from_numpy(G[f"k{i}_ids"])
        min_abs = max(mlen, plen + mnew if mnew else 0)
        got = ops.logits_process_(x.cuda(), ids.cuda(), cur, gu.EOS, pen, n, min_abs).cpu()
        assert torch.equal(torch.isinf(got), torch.isinf(want)), i
        assert torch.equal(got, want), (i, int((got != want).sum()))


def test_kernel_matches_restatement_on_random_shapes(M):
    from cxrmate_amd import ops
    g = torch.Generator().manual_seed(3)
    for t in range(24):
        R = int(torch.randint(1, 65, (1,), generator=g))
        V = int(torch.randint(8, 5000, (1,), generator=g))
        cur = int(torch.randint(0, 513, (1,), generator=g))
        n = int(torch.randint(0, 5, (1,), generator=g))
        pen = [1.0, 1.3, 0.8, 2.5][t % 4]
        alpha = int(torch.randint(2, 9, (1,), generator=g))             # a tiny alphabet: heavy duplication and repeated n-grams
        ids = torch.randint(0, min(alpha, V), (R, cur + 3), generator=g)
        x = torch.randn(R, V, generator=g) * 2.0
        mlen = int(torch.randint(0, 600, (1,), generator=g))
        got = ops.logits_process_(x.cuda(), ids.cuda(), cur, 1, pen, n, mlen).cpu()
        want = restate(x, ids, cur, 1, pen, n, mlen)
        assert torch.equal(got, want), (t, R, V, cur, n, pen)


# ------------------------------------------------------------------------------------------------ model cases
def multi_model(M, G, kind, dropout=None):
    c = {k: G[f"multi_{kind}_{k}"].item() for k in ("seed", "pixel_seed", "vocab", "sharpen", "cross_gain", "img_off", "perturb")}
    cfg = tiny_config(vocab_size=int(c["vocab"]), decoder_layers=2, image_size=96)
    if dropout is not None:
        cfg.decoder.hidden_dropout_prob = cfg.decoder.attention_probs_dropout_prob = dropout
    sd = gu.sharpened_state(cfg, int(c["seed"]), float(c["perturb"]), float(c["sharpen"]), float(c["cross_gain"]))
    m = M.MultiCXREncoderDecoderModel(cfg, seed=None)
    m.load_state_dict(sd)
    x = gu.distinct_study_pixels(int(c["pixel_seed"]), float(c["img_off"]))
    return m, dict(pixel_values=x.cuda(), special_token_ids=[gu.SEP], bos_token_id=gu.BOS, eos_token_id=gu.EOS, pad_token_id=gu.PAD)


def longi_model(M, G):
    from cxrmate_amd import weights
    cfg = tiny_config(vocab_size=int(G["longi_vocab"]), decoder_layers=2, image_size=96, lora_r=8)
    sd = weights.init_encoder_decoder(cfg, seed=int(G["longi_seed"]), perturb=float(G["longi_perturb"]))
    for k in list(sd):
        if "crossattention.output.dense." in k:
            sd[k] = sd[k] * float(G["longi_cross_gain"])
        if k.endswith(SHARPEN_SUFFIXES):
            sd[k] = sd[k] * float(G["longi_sharpen"])
    m = M.LongitudinalPromptMultiCXREncoderDecoderModel(cfg, seed=None)
    m.load_state_dict(sd)
    gen = torch.Generator().manual_seed(int(G["longi_pixel_seed"]))
    x = torch.randn(2, 2, 3, 96, 96, generator=gen)
    x[0, 1] = 0.0
    with torch.no_grad():
        eo = m.encoder(x.cuda())
    prompt = torch.from_numpy(G["longi_prompt"])
    return m, dict(encoder_outputs=eo, decoder_input_ids=prompt.cuda(), special_token_ids=[gu.PMT_SEP, gu.BOS, gu.SEP], bos_token_id=gu.BOS,
                   eos_token_id=gu.EOS, pad_token_id=gu.PAD, mask_token_id=gu.PAD)


def opts(G, key):
    pen, n, mnew = G[key]
    return dict(repetition_penalty=float(pen), no_repeat_ngram_size=int(n), min_new_tokens=int(mnew))


def check_greedy(m, kw, G, name, o):
    ref = torch.from_numpy(G[f"{name}_greedy"])
    margin = G[f"{name}_greedy_margin"]
    safe = margin > 3 * ERR_REL * G[f"{name}_greedy_std"]
    L = int(G[f"{name}_max_length"])
    P = ref.shape[1] - margin.shape[1]                                   # columns before the first generated one (BOS + prompt)
    runs = []
    for graph in (True, False):
        m.graph_decode = graph
        runs.append(m.generate(**kw, **o, max_length=L, num_beams=1).cpu())
    m.graph_decode = True
    runs.append(m.generate(**kw, **o, max_length=L, num_beams=1).cpu())                       # a second replay of the captured steps
    eager = m.generate(**kw, **o, max_length=L, num_beams=1, return_margins=True, return_dict_in_generate=True)["sequences"].cpu()
    for r in runs[1:]:                                                   # graph replay and eager launches of the session: the same kernels
        assert torch.equal(r, runs[0])
    got = runs[0]
    for run in (got, eager):                                             # (the eager loop decodes with the teacher-forced kernels)
        pinned = 0
        for b in range(ref.shape[0]):
            unsafe = np.nonzero(~safe[b])[0]
            upto = P + (unsafe[0] if len(unsafe) else margin.shape[1])  # decisions up to (excluding) the first unsafe step are pinned
            w = min(upto, ref.shape[1], run.shape[1])
            assert torch.equal(run[b, :w], ref[b, :w]), (name, b, run[b], ref[b])
            pinned += w - P
        assert pinned >= 8, (name, pinned)
    plain = m.generate(**kw, max_length=L, num_beams=1).cpu()
    assert plain.shape != got.shape or not torch.equal(plain, got)      # the options act
    return got


def test_greedy_multi_matches_fixture(M, G):
    m, kw = multi_model(M, G, "greedy")
    check_greedy(m, kw, G, "multi", opts(G, "greedy_opts"))


def test_greedy_longitudinal_matches_fixture(M, G):
    m, kw = longi_model(M, G)
    got = check_greedy(m, kw, G, "longi", opts(G, "longi_opts"))
    assert bool((got[:, 0] == gu.BOS).all())


def test_beam_matches_fixture_with_return_sequences(M, G):
    m, kw = multi_model(M, G, "beam")
    o = opts(G, "beam_opts")
    ref, ref_sc, tol = G["multi_beam4_all"], G["multi_beam4_all_scores"], float(G["multi_beam4_tol"])
    assert int(G["multi_beam4_robust"]) == 1
    B, nb, T = ref.shape
    res = {}
    for dev in (True, False):
        m.device_beam_search = dev
        for n in (4, 2):
            out = m.generate(**kw, **o, max_length=T, num_beams=4, num_return_sequences=n, return_dict_in_generate=True, output_scores=True)
            seq, sc = out["sequences"].cpu(), out["sequences_scores"].cpu()
            assert seq.shape[0] == B * n and sc.shape == (B * n,)
            res[(dev, n)] = (seq, sc)
            seq, sc = seq.view(B, n, -1), sc.view(B, n)
            w = min(seq.shape[-1], T)
            for b in range(B):
                assert torch.equal(seq[b, 0, :w], torch.from_numpy(ref[b, 0, :w])), (dev, n, b, seq[b, 0], ref[b, 0])
                assert bool((sc[b, 1:] <= sc[b, :-1]).all()), sc[b]                      # best first
                for j in range(1, n):
                    if torch.equal(seq[b, j, :w], torch.from_numpy(ref[b, j, :w])):
                        assert abs(float(sc[b, j]) - float(ref_sc[b, j])) <= 3 * tol, (b, j, sc[b, j], ref_sc[b, j])
            np.testing.assert_allclose(sc[:, 0].numpy(), ref_sc[:, 0], atol=tol)
        if "multi_beam4_n2" in G.files:
            assert res[(dev, 2)][0].shape[1] == G["multi_beam4_n2"].shape[1]
    m.device_beam_search = True
    for n in (4, 2):
        assert torch.equal(res[(True, n)][0], res[(False, n)][0])
    one = m.generate(**kw, **o, max_length=T, num_beams=4, return_dict_in_generate=True, output_scores=True)
    assert torch.equal(one["sequences"].cpu(), res[(True, 4)][0].view(B, 4, -1)[:, 0, :one["sequences"].shape[1]])


def _has_repeat(row, n, eos):
    toks = row.tolist()
    if eos in toks:
        toks = toks[:toks.index(eos) + 1]
    grams = [tuple(toks[i:i + n]) for i in range(len(toks) - n + 1)]
    return len(grams) != len(set(grams))


def test_sampling_return_sequences_ban_and_min_new_tokens(M, G):
    m, kw = multi_model(M, G, "beam")                                   # vocabulary 200, sharpened head: repeats are frequent without the ban
    B, n, new, mnew = 3, 3, 256, 20
    kw = dict(kw, do_sample=True, top_k=8, max_new_tokens=new, num_beams=1, num_return_sequences=n)
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        runs.append(m.generate(**kw, no_repeat_ngram_size=3, min_new_tokens=mnew).cpu())
    seq = runs[0]
    assert torch.equal(runs[0], runs[1])
    assert seq.shape[0] == B * n and seq.shape[1] <= 1 + new
    assert len({tuple(r.tolist()) for r in seq}) > B                     # the n rows of a study are different samples
    for r in seq:
        assert not _has_repeat(r, 3, gu.EOS), r
        assert not bool((r[1:1 + mnew] == gu.EOS).any()), r
    torch.manual_seed(1234)
    plain = m.generate(**kw).cpu()
    assert plain.shape[0] == B * n
    assert any(_has_repeat(r, 3, gu.EOS) for r in plain)


@pytest.mark.parametrize("n", [2, 3])
def test_sampled_scores_with_return_sequences_reach_encoder_outputs(M, G, n):
    """n = 2: the decode shares one copy of the encoder rows; n = 3: repeated rows (the re-scoring pass may borrow the session's cross K / V)."""
    m, kw = multi_model(M, G, "beam")
    with torch.no_grad():
        eo = m.encoder(kw.pop("pixel_values"))
    enc = eo["last_hidden_state"].detach().clone().requires_grad_(True)
    eo2 = type(eo)(last_hidden_state=enc, attention_mask=eo["attention_mask"])
    torch.manual_seed(5)
    out = m.generate.__wrapped__(m, encoder_outputs=eo2, **kw, do_sample=True, output_scores=True, return_dict_in_generate=True, top_k=20,
                                 max_new_tokens=6, num_beams=1, num_return_sequences=n)
    seq, sc = out["sequences"], torch.stack(out["scores"], dim=-1)
    assert seq.shape[0] == 3 * n and sc.shape[0] == 3 * n and sc.shape[1] == int(G["multi_beam_vocab"])
    sampled = seq[:, 1:1 + sc.shape[2]]
    assert bool(torch.isfinite(torch.gather(sc, 1, sampled[:, None, :]))[sampled[:, None, :] != gu.PAD].all())
    sc.float().logsumexp(1).sum().backward()
    assert enc.grad is not None and bool(torch.isfinite(enc.grad).all()) and float(enc.grad.abs().sum()) > 0
    assert bool((enc.grad.abs().sum((1, 2)) > 0).all())                        # every study's rows receive gradient


def test_defaults_launch_nothing_new(M, G, monkeypatch):
    from cxrmate_amd import ops
    m, kw = multi_model(M, G, "beam")
    base_g = m.generate(**kw, max_length=11, num_beams=1).cpu()
    base_b = m.generate(**kw, max_length=11, num_beams=4, return_dict_in_generate=True, output_scores=True)

    def refuse(*a, **k):
        raise AssertionError("logits_process_ launched with every option at its default")
    monkeypatch.setattr(ops, "logits_process_", refuse)
    d = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0, num_return_sequences=1)
    g2 = m.generate(**kw, **d, max_length=11, num_beams=1).cpu()
    b2 = m.generate(**kw, **d, max_length=11, num_beams=4, return_dict_in_generate=True, output_scores=True)
    assert torch.equal(g2, base_g)
    assert torch.equal(b2["sequences"].cpu(), base_b["sequences"].cpu())
    assert torch.equal(b2["sequences_scores"].cpu(), base_b["sequences_scores"].cpu())
    m.device_beam_search = False
    b3 = m.generate(**kw, **d, max_length=11, num_beams=4)
    assert b3.shape[0] == 3


REPLAY_CASES = {"greedy": dict(num_beams=1), "sample": dict(num_beams=1, do_sample=True, top_k=5), "beam": dict(num_beams=4),
                "beam_early": dict(num_beams=4, early_stopping=True),
                "controls": dict(num_beams=1, repetition_penalty=1.3, suppress_tokens=[7]),
                "records": dict(num_beams=1, return_dict_in_generate=True, output_logits=True, output_scores=True)}


@pytest.fixture(scope="module")
def replay_model(M, G):
    return multi_model(M, G, "beam")


@pytest.mark.parametrize("case", list(REPLAY_CASES))
def test_a_repeated_call_replays_its_graphs(replay_model, case):
    """Equal options must find the step graphs of the call before (a plan compared by identity would capture every step again on every call and pass
    every other test); one changed option must not find them. max_length 11 over the one-token prompt: the eager prefill, one 7-step graph, one
    stop poll, one 2-step graph."""
    m, kw = replay_model
    o = REPLAY_CASES[case]

    def run(o):
        torch.manual_seed(77)
        out = m.generate(**{**kw, **o}, max_length=11)
        keys = [set(s_.graphs) for s_ in m._decode_sessions.values()]
        return (out if torch.is_tensor(out) else out["sequences"]).cpu(), set().union(*keys)
    m.__dict__.pop("_decode_sessions", None)                             # this case's graphs only
    first, keys = run(o)
    assert keys and {k[:2] for k in keys} == {(2, 7), (9, 2)}            # (column, steps) behind the eager prefill of column 1
    assert {k[3].kind for k in keys} == {"beam" if o["num_beams"] > 1 else "sample" if "do_sample" in o else "greedy"}
    second, keys2 = run(o)
    assert keys2 == keys                                                 # nothing was captured again
    assert torch.equal(second, first)
    if "top_k" in o:
        other = dict(o, top_k=6)
    elif "suppress_tokens" in o:
        other = dict(o, suppress_tokens=[8])
    elif "early_stopping" in o:
        other = dict(o, early_stopping=False)
    elif "output_logits" in o:
        other = dict(o, output_logits=False)
    elif case == "beam":
        other = dict(o, length_penalty=2.0)
    else:
        other = dict(o, pad_token_id=gu.PAD + 1)
    _, keys3 = run(other)
    added = keys3 - keys
    assert keys <= keys3 and added and {k[:3] for k in added} == {k[:3] for k in keys}      # the same steps, captured anew under another plan
    assert not {k[3] for k in added} & {k[3] for k in keys}


def test_invalid_options_raise(M, G):
    m, kw = multi_model(M, G, "beam")
    with pytest.raises(ValueError):
        m.generate(**kw, max_length=8, num_beams=1, num_return_sequences=2)
    with pytest.raises(ValueError):
        m.generate(**kw, max_length=8, num_beams=2, num_return_sequences=3)
    for bad in (0.0, -1.2):
        with pytest.raises(ValueError):
            m.generate(**kw, max_length=8, repetition_penalty=bad)
    with pytest.raises(NotImplementedError, match="output_scores"):
        m.generate.__wrapped__(m, **kw, max_length=8, do_sample=True, output_scores=True, no_repeat_ngram_size=2)
    with pytest.raises(NotImplementedError):
        m.generate(**kw, max_length=8, do_sample=True, output_scores=True, repetition_penalty=1.2)
    with pytest.raises(ValueError, match="max_length"):            # refused before any step is decoded (histories are at most 512 ids)
        m.generate(**kw, max_length=600, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="max_length"):
        m.generate(**kw, max_length=600, num_beams=4, repetition_penalty=1.2)


def test_ngram_sizes_the_library_ignores(M, G, monkeypatch):
    """TF5 adds NoRepeatNGramLogitsProcessor for sizes > 0 only; a size longer than any history can never complete an n-gram."""
    from cxrmate_amd import ops
    m, kw = multi_model(M, G, "beam")
    pen = m.generate(**kw, max_length=11, num_beams=1, repetition_penalty=1.3).cpu()
    for size in (-1, -3, 600):
        assert torch.equal(m.generate(**kw, max_length=11, num_beams=1, repetition_penalty=1.3, no_repeat_ngram_size=size).cpu(), pen)
    beam = m.generate(**kw, max_length=11, num_beams=4, repetition_penalty=1.3).cpu()
    assert torch.equal(m.generate(**kw, max_length=11, num_beams=4, repetition_penalty=1.3, no_repeat_ngram_size=-2).cpu(), beam)
    plain = m.generate(**kw, max_length=11, num_beams=1).cpu()

    def refuse(*a, **k):
        raise AssertionError("logits_process_ launched for an ignored n-gram size")
    monkeypatch.setattr(ops, "logits_process_", refuse)
    assert torch.equal(m.generate(**kw, max_length=11, num_beams=1, no_repeat_ngram_size=-1).cpu(), plain)


def test_train_mode_return_sequences_scores_belong_to_their_draws(M, G):
    """Under model.train() every decode row has its own dropout masks, keyed by row. Several samples per study are decoded as B * n rows; the
    differentiable scores must come from the forward that drew each token -- the re-scoring pass over the decode's own rows -- not from the masks
    of another sample of the same study. At temperature 0.01 over the whole vocabulary (sharpened head) a row draws the argmax of its own dropout
    forward, so the drawn token is the argmax of its re-scored row; a mask of another sample moves the argmax wherever the samples part."""
    m, kw = multi_model(M, G, "beam", dropout=0.4)                              # strong dropout: the samples of a study part early and often
    x = kw.pop("pixel_values")
    with torch.no_grad():
        eo = m.encoder(x)
    m.train()
    try:
        B, n, new = 3, 3, 16
        torch.manual_seed(21)
        out = m.generate.__wrapped__(m, encoder_outputs=eo, **dict(kw, eos_token_id=None), do_sample=True, output_scores=True,
                                     return_dict_in_generate=True, top_k=0, temperature=0.01, max_new_tokens=new, num_beams=1,
                                     num_return_sequences=n)
    finally:
        m.eval()
    seq, sc = out["sequences"], torch.stack(out["scores"], dim=-1)             # [B*n, L], [B*n, V, T]
    assert seq.shape == (B * n, 1 + new) and sc.shape[0] == B * n and sc.shape[2] == new
    drawn = seq[:, 1:]
    assert bool(torch.isfinite(torch.gather(sc, 1, drawn[:, None, :])).all())
    top = sc.detach().argmax(1)                                                 # [B*n, T]: the re-scored argmax of every step
    per_study = seq.view(B, n, -1)
    parted = sum(int((per_study[b, j] != per_study[b, 0]).sum()) for b in range(B) for j in range(1, n))
    agree = float((top == drawn).float().mean())
    print(f"train-mode re-scoring: drawn token is the re-scored argmax at {agree:.3f} of the steps; {parted} positions where samples part")
    assert parted >= 8, "dropout must make the samples of a study differ for this test to see anything"
    assert agree >= 0.95, (agree, parted, top, drawn)
