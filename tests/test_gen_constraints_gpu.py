"""GPU: the token constraints of generate() (sequence_bias, bad_words_ids, forced_bos_token_id, forced_eos_token_id, suppress_tokens,
begin_suppress_tokens), early_stopping and generation_config against tests/golden/gen_constraints.npz (transformers 5.15.0's own processor classes
and the reference's generate, tests/golden/make_golden_gen_constraints.py) and the CPU restatements of tests/gen_constraints_ref.py.

  kernel (csrc/logits_proc.hip logits_constrain_kernel) : -inf pattern exact and values bit-equal -- the only arithmetic is the bit-exact repetition
                                                          penalty and ONE IEEE add of an fp32 sum accumulated in the library's order
  greedy                                                : test_gen_controls_gpu.check_greedy (identical up to the first step whose processed margin
                                                          is below 3 x 1.2 % of the step's score spread)
  beam-4                                                : the best hypothesis of every study and its score, test_gen_controls_gpu's rule
  early stopping (csrc/decode.hip cxr_beam_step_es)     : the device search fed the reference's recorded logits, against the restated search at every
                                                          step; final hypotheses bit-equal, scores to 2e-6 relative (the bound of
                                                          test_kernels_gpu.test_device_beam_search_is_bit_equal_on_the_references_recorded_logits)
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gen_constraints_ref as ref
import golden_util as gu
from test_gen_controls_gpu import check_greedy, longi_model, multi_model

pytestmark = pytest.mark.gpu
NINF = float("-inf")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import modelling
    return modelling


@pytest.fixture(scope="module")
def G():
    return gu.load("gen_constraints.npz")


def unpack(tok, lens):
    out, at = [], 0
    for n in lens.tolist():
        out.append([int(t) for t in tok[at:at + n]])
        at += n
    return out


def kernel_case(G, i):
    """-> (scores, wanted scores, ids, positional arguments of the kernel, options as a caller passes them, prompt_len, max_length)."""
    k = f"k{i}_"
    seed, R, V, cur, n, mlen, plen, max_length, lp, fbos = (int(v) for v in G[k + "params"])
    x = torch.randn(R, V, generator=torch.Generator().manual_seed(seed)) * 3.0
    if lp:
        x = torch.log_softmax(x, dim=-1)
    want = x.clone().reshape(-1)
    want[torch.from_numpy(G[k + "changed_idx"])] = torch.from_numpy(G[k + "changed_val"])
    raw = {}
    if len(G[k + "bias_len"]):
        raw["sequence_bias"] = [[w, float(b)] for w, b in zip(unpack(G[k + "bias_tok"], G[k + "bias_len"]), G[k + "bias_val"])]
    if len(G[k + "bad_len"]):
        raw["bad_words_ids"] = unpack(G[k + "bad_tok"], G[k + "bad_len"])
    if fbos >= 0:
        raw["forced_bos_token_id"] = fbos
    for key, name in (("forced_eos", "forced_eos_token_id"), ("suppress", "suppress_tokens"), ("begin_suppress", "begin_suppress_tokens")):
        if len(G[k + key]):
            raw[name] = [int(t) for t in G[k + key]]
    return x, want.view(R, V), torch.from_numpy(G[k + "ids"]), (cur, gu.EOS, float(G[k + "penalty"]), n, mlen), raw, plen, max_length


def test_kernel_matches_fixture(M, G):
    from cxrmate_amd import generation as gen, ops
    assert int(G["n_kernel_cases"]) >= 12
    for i in range(int(G["n_kernel_cases"])):
        x, want, ids, args, raw, plen, max_length = kernel_case(G, i)
        cons = gen.token_constraints(x.shape[1], gu.EOS, plen, max_length, **raw)
        tables = gen.constraint_tables(cons, "cuda")
        got = ops.logits_constrain_(x.cuda(), ids.cuda(), *args, tables=tables).cpu()
        assert torch.equal(torch.isinf(got), torch.isinf(want)), i
        assert torch.equal(got, want), (i, int((got != want).sum()))
        again = ops.logits_constrain_(x.cuda(), ids.cuda(), *args, tables=tables).cpu()            # run to run
        assert torch.equal(again.view(torch.int32), got.view(torch.int32)), i


def random_case(g, t):
    R = int(torch.randint(1, 65, (1,), generator=g))
    V = int(torch.randint(8, 5001, (1,), generator=g))
    cur = 1 if t % 8 == 5 else int(torch.randint(1, 513, (1,), generator=g))
    alpha = min(int(torch.randint(2, 7, (1,), generator=g)), V)        # a tiny alphabet: prefixes match often, last tokens collide
    ids = torch.randint(0, alpha, (R, cur + 2), generator=g)
    x = torch.randn(R, V, generator=g) * 2.0
    n_entries = int(torch.randint(0, 41, (1,), generator=g))
    table = {}
    for _ in range(n_entries):
        k = int(torch.randint(1, 5, (1,), generator=g))
        key = tuple(torch.randint(0, alpha, (k,), generator=g).tolist())
        table[key] = NINF if int(torch.randint(0, 8, (1,), generator=g)) == 0 else round(float(torch.randn(1, generator=g)) * 1.7, 3)
    if t % 6 == 0 and cur >= 3:                                         # an entry as long as the history, one longer (skipped)
        table[tuple(ids[0, 1:cur].tolist()) + (1,)] = 0.77
        table[tuple(ids[0, :cur].tolist()) + (1,)] = -0.55
    entries = list(table.items())
    split = int(torch.randint(0, len(entries) + 1, (1,), generator=g))
    sup = torch.randint(0, V + 20, (int(torch.randint(0, 6, (1,), generator=g)),), generator=g).tolist()
    begin = torch.randint(0, V, (int(torch.randint(0, 4, (1,), generator=g)),), generator=g).tolist()
    kw = dict(sequence_bias=tuple(entries[:split]), bad_words=tuple(k for k, _ in entries[split:]),
              forced_bos=int(torch.randint(0, V, (1,), generator=g)) if t % 4 == 1 else None,
              forced_eos=tuple(torch.randint(0, V, (2,), generator=g).tolist()) if t % 3 == 0 else (),
              suppress=tuple(sup + sup[:1]), begin_suppress=tuple(begin), max_length=cur + 1 + (t % 2),
              begin_index=cur + (int(torch.randint(0, 2, (1,), generator=g))))
    ctl = dict(penalty=[1.0, 1.3, 0.8, 2.5][t % 4], n=int(torch.randint(0, 5, (1,), generator=g)), min_length=int(torch.randint(0, 600, (1,), generator=g)))
    return x, ids, cur, ctl, kw


def test_kernel_matches_restatement_on_random_shapes(M):
    from cxrmate_amd import ops
    g = torch.Generator().manual_seed(31)
    fired = dict(bias=0, bad=0, fbos=0, feos=0, begin=0)
    for t in range(24):
        x, ids, cur, ctl, kw = random_case(g, t)
        tables = ops.ConstraintTables("cuda", **kw)
        got = ops.logits_constrain_(x.cuda(), ids.cuda(), cur, 1, ctl["penalty"], ctl["n"], ctl["min_length"], tables=tables).cpu()
        want = ref.restate(x, ids, cur, 1, **ctl, **kw)
        assert torch.equal(got, want), (t, x.shape, cur, ctl, int((got != want).sum()))
        again = ops.logits_constrain_(x.cuda(), ids.cuda(), cur, 1, ctl["penalty"], ctl["n"], ctl["min_length"], tables=tables).cpu()
        assert torch.equal(again.view(torch.int32), got.view(torch.int32)), t
        fired["bias"] += bool(kw["sequence_bias"]); fired["bad"] += bool(kw["bad_words"])
        fired["fbos"] += kw["forced_bos"] is not None and cur == 1; fired["feos"] += bool(kw["forced_eos"]) and cur == kw["max_length"] - 1
        fired["begin"] += bool(kw["begin_suppress"]) and cur == kw["begin_index"]
    assert all(v > 0 for v in fired.values()), fired                     # every branch of the kernel was taken by some shape


def test_constraint_kernel_without_tables_equals_the_controls_kernel(M):
    """The three controls are the same device functions in both kernels: with empty tables the new entry point gives cxr_logits_process_f32's rows."""
    from cxrmate_amd import ops
    g = torch.Generator().manual_seed(32)
    for cur, V in ((17, 999), (512, 3000)):
        ids = torch.randint(0, 6, (5, cur), generator=g).cuda()
        x = (torch.randn(5, V, generator=g) * 2.0).cuda()
        a = ops.logits_process_(x.clone(), ids, cur, 1, 1.3, 2, 600)
        b = ops.logits_constrain_(x.clone(), ids, cur, 1, 1.3, 2, 600, tables=ops.ConstraintTables("cuda"))
        assert torch.equal(a, b) and not torch.equal(a, x)


def test_forced_row_through_select_token(M):
    """A forced row has ONE finite entry: every selection mode must return it."""
    from cxrmate_amd import ops
    g = torch.Generator().manual_seed(33)
    R, V, cur, tok = 6, 1000, 9, 417
    x = (torch.randn(R, V, generator=g) * 3.0).cuda()
    ids = torch.randint(0, 12, (R, cur), generator=g).cuda()
    tables = ops.ConstraintTables("cuda", forced_eos=[tok], max_length=cur + 1)
    ops.logits_constrain_(x, ids, cur, 2, tables=tables)
    assert int(torch.isfinite(x).sum()) == R and bool((x[:, tok] == 0).all())
    want = torch.full((R,), tok, dtype=torch.int64)
    u = torch.rand(R, generator=g).cuda()
    assert torch.equal(ops.select_token(x.clone())[0].cpu(), want)
    assert torch.equal(ops.select_token(x.clone(), mode=1, top_k=50, u=u)[0].cpu(), want)
    assert torch.equal(ops.select_token(x.clone(), mode=1, top_k=0, top_p=0.9, u=u)[0].cpu(), want)
    assert torch.equal(ops.select_token(x.clone(), mode=1, top_k=50, top_p=0.9, temperature=0.7, u=u[:3], n_sample=3)[0].cpu(), want)


# ------------------------------------------------------------------------------------------------ model cases
def options(G, name):
    return dict(bad_words_ids=unpack(G[f"{name}_bad_tok"], G[f"{name}_bad_len"]), begin_suppress_tokens=[int(t) for t in G[f"{name}_begin_suppress"]],
                forced_eos_token_id=int(G[f"{name}_forced_eos"]))


def check_scores(m, kw, o, L, P):
    """output_scores returns the scores AFTER the processors: -inf at the banned single token on every step, at the begin-suppressed token on
    the first step, and one finite entry (EOS, at 0) on the forced last step."""
    out = m.generate(**kw, **o, max_length=L, num_beams=1, return_dict_in_generate=True, output_scores=True)
    sc = [s.cpu() for s in out["scores"]]
    single = [w[0] for w in o["bad_words_ids"] if len(w) == 1]
    assert single and all(bool((s[:, single] == NINF).all()) for s in sc)
    assert bool((sc[0][:, o["begin_suppress_tokens"]] == NINF).all()) and bool(torch.isfinite(sc[1][:, o["begin_suppress_tokens"]]).any())
    if len(sc) == L - P:                                                # the decode reached the length limit
        assert int(torch.isfinite(sc[-1]).sum()) == sc[-1].shape[0] and bool((sc[-1][:, gu.EOS] == 0).all())
    return out["sequences"].cpu()


def test_greedy_multi_matches_fixture(M, G):
    m, kw = multi_model(M, G, "greedy")
    o = options(G, "multi_greedy")
    assert int(G["multi_greedy_opts_max_length"]) == int(G["multi_max_length"])
    got = check_greedy(m, kw, G, "multi", o)
    assert torch.equal(check_scores(m, kw, o, int(G["multi_max_length"]), 1), got)
    assert got.shape[1] == int(G["multi_max_length"]) and bool((got[:, -1] == gu.EOS).any())          # a row the forced EOS ended


def test_greedy_longitudinal_matches_fixture(M, G):
    m, kw = longi_model(M, G)
    o = options(G, "longi")
    got = check_greedy(m, kw, G, "longi", o)
    assert bool((got[:, 0] == gu.BOS).all())
    first = G["longi_greedy"].shape[1] - G["longi_greedy_margin"].shape[1]     # columns before the first generated one (BOS + prompt)
    assert torch.equal(check_scores(m, kw, o, int(G["longi_max_length"]), first), got)
    # the bigram ban starts in the prompt: the first generated token of row 1 is not the one the unconstrained decode takes
    bigram = [w for w in o["bad_words_ids"] if len(w) == 2][0]
    plain = torch.from_numpy(G["longi_greedy_plain"])
    assert int(plain[1, first - 1]) == bigram[0] and int(plain[1, first]) == bigram[1] and int(got[1, first]) != bigram[1]


def test_beam_matches_fixture_and_host_loop(M, G):
    m, kw = multi_model(M, G, "beam")
    o = options(G, "multi_beam")
    ref_seq, ref_sc, tol = G["multi_beam4_all"], G["multi_beam4_all_scores"], float(G["multi_beam4_tol"])
    assert int(G["multi_beam4_robust"]) == 1
    B, nb, T = ref_seq.shape
    assert T == int(G["multi_beam_opts_max_length"])
    res = {}
    for dev in (True, False):
        m.device_beam_search = dev
        out = m.generate(**kw, **o, max_length=T, num_beams=4, num_return_sequences=4, return_dict_in_generate=True, output_scores=True)
        seq, sc = out["sequences"].cpu().view(B, 4, -1), out["sequences_scores"].cpu().view(B, 4)
        res[dev] = (seq, sc)
        w = min(seq.shape[-1], T)
        print("beam best scores", dev, sc[:, 0].tolist(), ref_sc[:, 0].tolist(), "tol", tol)
        for b in range(B):
            assert torch.equal(seq[b, 0, :w], torch.from_numpy(ref_seq[b, 0, :w])), (dev, b, seq[b, 0], ref_seq[b, 0])
            assert bool((sc[b, 1:] <= sc[b, :-1]).all()), sc[b]
        np.testing.assert_allclose(sc[:, 0].numpy(), ref_sc[:, 0], atol=tol)
        # the recorded scores are the processed log-probs: the banned token is -inf on every step, in every beam row
        single = [w_[0] for w_ in o["bad_words_ids"] if len(w_) == 1]
        assert all(bool((s[:, single] == NINF).all()) for s in out["scores"])
    m.device_beam_search = True
    # device search == host loop: the same hypotheses. The two decode with different kernels (cached single-token steps over shared encoder rows
    # against the teacher-forced kernels over repeated rows), so their logits differ by bf16 rounding and their scores are not bit-equal: each best
    # score is within `tol` of the reference's (asserted above), hence within 2 x tol of the other. On identical logits the two searches are
    # compared bit for bit by the recorded-logits tests below.
    assert torch.equal(res[True][0], res[False][0])
    np.testing.assert_allclose(res[True][1][:, 0].numpy(), res[False][1][:, 0].numpy(), atol=2 * tol, rtol=0)
    plain = m.generate(**kw, max_length=T, num_beams=4).cpu()
    assert plain.shape[1] != res[True][0].shape[-1] or not torch.equal(plain, res[True][0][:, 0])


def test_three_ways_to_ban_a_token_are_one(M, G):
    m, kw = multi_model(M, G, "beam")
    plain = m.generate(**kw, max_length=11, num_beams=4).cpu()
    t = int(plain[0, 2])
    outs = []
    for o in (dict(suppress_tokens=[t]), dict(bad_words_ids=[[t]]), dict(sequence_bias={(t,): NINF})):
        out = m.generate(**kw, **o, max_length=11, num_beams=4, return_dict_in_generate=True, output_scores=True)
        outs.append((out["sequences"].cpu(), out["sequences_scores"].cpu()))
        g = m.generate(**kw, **o, max_length=11, num_beams=1).cpu()
        outs[-1] += (g,)
        assert not bool((out["sequences"] == t).any()) and not bool((g == t).any())
    for seq, sc, g in outs[1:]:
        assert torch.equal(seq, outs[0][0]) and torch.equal(sc.view(torch.int32), outs[0][1].view(torch.int32)) and torch.equal(g, outs[0][2])
    assert bool((plain == t).any())                                      # the unconstrained decode does use the token


def test_generation_config_object_equals_keywords(M, G):
    from transformers import GenerationConfig
    m, kw = multi_model(M, G, "beam")
    o = options(G, "multi_beam")
    T = int(G["multi_beam_opts_max_length"])
    want = m.generate(**kw, **o, max_length=T, num_beams=4, early_stopping=True).cpu()
    ids = {k: kw.pop(k) for k in ("bos_token_id", "eos_token_id", "pad_token_id")}
    for cfg in (GenerationConfig(**o, **ids, max_length=T, num_beams=4, early_stopping=True),
                SimpleNamespace(**o, **ids, max_length=T, num_beams=4, early_stopping=True, top_k=None)):
        assert torch.equal(m.generate(**kw, generation_config=cfg).cpu(), want)
    # a keyword wins over the object, even at its default value
    greedy = m.generate(**kw, **ids, **o, max_length=T, num_beams=1).cpu()
    assert torch.equal(m.generate(**kw, generation_config=cfg, num_beams=1).cpu(), greedy)
    with pytest.raises(NotImplementedError, match="penalty_alpha"):
        m.generate(**kw, generation_config=SimpleNamespace(**ids, max_length=T, penalty_alpha=0.6))


# ------------------------------------------------------------------------------------------------ early stopping
def device_beam_state(B, nb, L, pad, bos):
    run = torch.full((nb, B, L), pad, dtype=torch.int64, device="cuda")
    run[:, :, 0] = bos
    rs = torch.zeros((B, nb), device="cuda")
    rs[:, 1:] = -1.0e9
    return dict(run=run, seq=run.clone(), rs=rs, bs=torch.full((B, nb), -1.0e9, device="cuda"), fin=torch.zeros((B, nb), dtype=torch.uint8, device="cuda"),
                unsat=torch.ones((2, B), dtype=torch.int32, device="cuda"), hit=torch.zeros((2, B), dtype=torch.int32, device="cuda"),
                allfin=torch.zeros((2, B), dtype=torch.int32, device="cuda"), idx=torch.zeros(nb * B, dtype=torch.int64, device="cuda"))


def es_case(G, name):
    """-> the recorded logits and fed tokens of the steps the reference ran in this mode, plus ALL recorded steps (the longest run's: a search
    that goes on past the reference's stop would find logits to go on with), the reference's hypotheses and scores."""
    n = int(G[f"es_{name}_steps"])
    return (torch.from_numpy(G["es_logits"][:n]), torch.from_numpy(G["es_fed"][:n]), torch.from_numpy(G[f"es_{name}_all"]),
            torch.from_numpy(G[f"es_{name}_all_scores"]), torch.from_numpy(G["es_logits"]))


@pytest.mark.parametrize("name,mode", [("true", True), ("never", "never"), ("false", False)])
def test_device_early_stopping_on_the_references_recorded_logits(M, G, name, mode):
    from cxrmate_amd import generation as gen, ops
    B, nb, P = 3, 4, 1
    lp, L = float(G["es_length_penalty"]), int(G["es_steps"]) + 1
    logits, fed, want, want_sc, every = es_case(G, name)
    V = logits.shape[-1]
    _, _, trace = ref.beam_search(list(every), B, nb, gu.BOS, gu.EOS, gu.PAD, L, lp, mode, fed=fed)
    assert len(trace) == logits.shape[0] and trace[-1]["stop"]          # (the restatement against the reference: test_gen_constraints_abi.py)
    es = gen.early_stopping_mode(mode, lp)
    st = device_beam_state(B, nb, L, gu.PAD, gu.BOS)
    for t, tr in enumerate(trace):
        cur = P + t
        running = st["run"].permute(1, 0, 2)[:, :, :cur].cpu()
        assert torch.equal(running, tr["running_in"]) and torch.equal(running[:, :, -1].reshape(-1), fed[t]), (name, t)
        bm = logits[t].view(B, nb, V).permute(1, 0, 2).reshape(nb * B, V).contiguous().cuda()
        ops.beam_step(bm, st["run"], st["seq"], st["rs"], st["bs"], st["fin"], st["unsat"], st["hit"], st["idx"], cur, L, gu.EOS,
                      float(cur + 1 - P) ** lp, early=(es, float(L - P) ** lp if es == 2 else 0.0, st["allfin"]))
        live = tr["running_scores"] > -1.0e8
        parent = (st["idx"].view(nb, B).t() // B).cpu()
        assert torch.equal(parent[live], tr["parent"][live]) and torch.equal(st["run"].permute(1, 0, 2)[:, :, cur].cpu()[live], tr["token"][live]), (name, t)
        np.testing.assert_allclose(st["rs"].cpu().numpy()[live.numpy()], tr["running_scores"].numpy()[live.numpy()], rtol=2e-6, atol=2e-5)
        fin = tr["finished"]
        assert torch.equal(st["fin"].bool().cpu(), fin), (name, t)
        assert torch.equal(st["seq"].permute(1, 0, 2).cpu()[fin], tr["sequences"][fin]), (name, t)
        np.testing.assert_allclose(st["bs"].cpu().numpy()[fin.numpy()], tr["beam_scores"].numpy()[fin.numpy()], rtol=2e-6, atol=2e-5)
        par = cur & 1
        assert torch.equal(st["unsat"][par].bool().cpu(), tr["unsat"]), (name, t)
        if es == 1:
            assert torch.equal(st["allfin"][par].bool().cpu(), fin.all(dim=1)), (name, t)
        going = bool(st["unsat"][par].max() > 0) and bool(st["hit"][par].min() == 0) and not (es == 1 and bool(st["allfin"][par].min() > 0))
        assert going == (not tr["stop"]), (name, t)                      # the stop flags fall on the reference's step, not before
    # one more launch after the stop: the state is frozen, the reorder is the identity
    if P + len(trace) < L:
        before = [st[k].clone() for k in ("run", "seq", "rs", "bs", "fin")]
        ops.beam_step(every[len(trace)].view(B, nb, V).permute(1, 0, 2).reshape(nb * B, V).contiguous().cuda(), st["run"], st["seq"], st["rs"], st["bs"], st["fin"], st["unsat"], st["hit"], st["idx"],
                      P + len(trace), L, gu.EOS, 1.0, early=(es, 1.0, st["allfin"]))
        assert all(torch.equal(a, st[k]) for a, k in zip(before, ("run", "seq", "rs", "bs", "fin")))
        assert torch.equal(st["idx"], torch.arange(nb * B, device="cuda"))
    seqs, scores = st["seq"].permute(1, 0, 2).cpu(), st["bs"].cpu()
    assert torch.equal(seqs[:, :, :want.shape[-1]], want) and bool((seqs[:, :, want.shape[-1]:] == gu.PAD).all()), name
    np.testing.assert_allclose(scores.numpy(), want_sc.numpy(), rtol=2e-6, atol=2e-5, err_msg=name)


def test_the_three_modes_stop_on_three_different_steps(G):
    assert int(G["es_true_steps"]) < int(G["es_false_steps"]) < int(G["es_never_steps"]) <= int(G["es_steps"])


@pytest.mark.parametrize("name,mode", [("true", True), ("never", "never"), ("false", False)])
def test_host_loop_early_stopping_on_the_references_recorded_logits(M, G, name, mode, monkeypatch):
    """generate()'s host-loop beam search with the decoder's logits replaced by the recorded ones (study-major rows, as the loop orders them)."""
    from cxrmate_amd.config import tiny_config
    logits, fed, want, want_sc, every = es_case(G, name)
    cfg = tiny_config(vocab_size=int(G["es_vocab"]), decoder_layers=2, image_size=96)
    m = M.MultiCXREncoderDecoderModel(cfg, seed=3)
    m.device_beam_search = False
    step = {"t": 0}

    def replay(cache, new, *a, **k):
        t = step["t"]
        assert t < every.shape[0]
        assert torch.equal(new[:, -1].cpu(), torch.from_numpy(G["es_fed"][t])), t
        step["t"] = t + 1
        cache.len += new.shape[1]
        return every[t].cuda().clone()
    monkeypatch.setattr(m._dec, "decode", replay)
    x = gu.distinct_study_pixels(int(G["es_pixel_seed"]), float(G["es_img_off"])).cuda()
    out = m.generate(pixel_values=x, special_token_ids=[gu.SEP], bos_token_id=gu.BOS, eos_token_id=gu.EOS, pad_token_id=gu.PAD, num_beams=4,
                     num_return_sequences=4, max_length=int(G["es_steps"]) + 1, length_penalty=float(G["es_length_penalty"]), early_stopping=mode,
                     return_dict_in_generate=True, output_scores=True)
    assert step["t"] == logits.shape[0]                                  # stopped on the reference's step
    seq, sc = out["sequences"].cpu().view(3, 4, -1), out["sequences_scores"].cpu().view(3, 4)
    w = min(seq.shape[-1], want.shape[-1])
    assert torch.equal(seq[:, :, :w], want[:, :, :w]) and bool((want[:, :, w:] == gu.PAD).all()) and bool((seq[:, :, w:] == gu.PAD).all())
    np.testing.assert_allclose(sc.numpy(), want_sc.numpy(), rtol=2e-6, atol=2e-5)


@pytest.mark.parametrize("dev", [True, False])
def test_generate_early_stopping_orders_the_stop_steps(M, G, dev):
    """early_stopping through generate() (device search: graph replay, stop flags polled every 8 steps; host loop). The running beams of a search
    do not depend on early_stopping, so on one model and one set of kernels the three modes see the same logits step by step, and the stop steps
    are ordered exactly: True only ADDS a stop condition to False, and "never" (length_penalty 2) measures the running beams against a longer
    length than False, so it goes on at least as long. A second run of a mode repeats the first bit for bit. The LM head's EOS bias is raised
    (the recipe of the recorded-logits fixtures) so that hypotheses end early and the modes have something to disagree about."""
    m, kw = multi_model(M, G, "beam")
    sd = m.state_dict()
    keys = [k for k in sd if k.endswith(("cls.predictions.bias", "cls.predictions.decoder.bias"))]
    assert keys
    for k in keys:
        sd[k] = sd[k].clone()
        sd[k][gu.EOS] += 20.0
    m.load_state_dict(sd)
    m.device_beam_search = dev
    steps, first = {}, {}
    for mode in (True, False, "never", True):
        out = m.generate(**kw, max_length=14, num_beams=4, num_return_sequences=4, early_stopping=mode, length_penalty=2.0,
                         return_dict_in_generate=True, output_scores=True)
        got = (out["sequences"].cpu(), out["sequences_scores"].cpu(), len(out["scores"]))
        if mode in first:
            assert torch.equal(got[0], first[mode][0]) and torch.equal(got[1].view(torch.int32), first[mode][1].view(torch.int32)) and got[2] == first[mode][2]
        first[mode], steps[mode] = got, got[2]
    m.device_beam_search = True
    print("steps run", "device" if dev else "host", steps)
    assert steps[True] <= steps[False] <= steps["never"] <= 13
    # the steps every mode ran recorded the same scores: the beams are the same until a mode stops
    a = m.generate(**kw, max_length=14, num_beams=4, early_stopping=True, length_penalty=2.0, return_dict_in_generate=True, output_scores=True)
    assert len(a["scores"]) == steps[True]


# ------------------------------------------------------------------------------------------------ defaults and refusals
def test_defaults_call_no_new_entry_point(M, G, monkeypatch):
    from cxrmate_amd import ops
    m, kw = multi_model(M, G, "beam")
    m.graph_decode = False                                               # every step launches eagerly: each call is seen
    base_b = m.generate(**kw, max_length=11, num_beams=4, return_dict_in_generate=True, output_scores=True)
    base_g = m.generate(**kw, max_length=11, num_beams=1).cpu()
    calls = []
    real = ops.LIB.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(ops.LIB, "call", spy)
    d = dict(bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, sequence_bias=None, forced_bos_token_id=None,
             forced_eos_token_id=None, early_stopping=False, generation_config=None)
    g2 = m.generate(**kw, **d, max_length=11, num_beams=1).cpu()
    b2 = m.generate(**kw, **d, max_length=11, num_beams=4, return_dict_in_generate=True, output_scores=True)
    m.generate(**kw, **dict(d, early_stopping="never"), length_penalty=0.0, max_length=11, num_beams=4)      # "never" without a positive penalty is False
    m.generate(**kw, **d, max_length=11, num_beams=1, repetition_penalty=1.3)
    assert "cxr_logits_constrain_f32" not in calls and "cxr_beam_step_es" not in calls
    assert "cxr_logits_process_f32" in calls and "cxr_beam_step" in calls
    assert torch.equal(g2, base_g)
    assert torch.equal(b2["sequences"].cpu(), base_b["sequences"].cpu())
    assert torch.equal(b2["sequences_scores"].cpu().view(torch.int32), base_b["sequences_scores"].cpu().view(torch.int32))
    # with an option set: ONE launch of the new kernel per step, in place of the old one
    del calls[:]
    out = m.generate(**kw, max_length=11, num_beams=1, repetition_penalty=1.3, suppress_tokens=[int(base_g[0, 1])])
    assert calls.count("cxr_logits_constrain_f32") == calls.count("cxr_select_token") >= out.shape[1] - 1 and "cxr_logits_process_f32" not in calls
    del calls[:]
    m.generate(**kw, max_length=11, num_beams=4, early_stopping=True)
    assert "cxr_beam_step_es" in calls and "cxr_beam_step" not in calls


def test_refusals(M, G):
    m, kw = multi_model(M, G, "beam")
    with pytest.raises(NotImplementedError, match="output_scores"):
        m.generate.__wrapped__(m, **kw, max_length=8, do_sample=True, output_scores=True, bad_words_ids=[[7]])
    with pytest.raises(NotImplementedError, match="output_scores"):
        m.generate(**kw, max_length=8, do_sample=True, output_scores=True, suppress_tokens=[7])
    with pytest.raises(ValueError, match="max_length"):                 # histories are at most 512 ids: refused before decoding
        m.generate(**kw, max_length=514, suppress_tokens=[7])
    with pytest.raises(ValueError, match="max_length"):
        m.generate(**kw, max_length=600, num_beams=4, forced_eos_token_id=gu.EOS)
    with pytest.raises(ValueError, match="vocabulary size"):
        m.generate(**kw, max_length=8, bad_words_ids=[[5, 200]])
    with pytest.raises(ValueError, match="early_stopping"):
        m.generate(**kw, max_length=8, num_beams=4, early_stopping="sometimes")
