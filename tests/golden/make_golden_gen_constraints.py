#!/usr/bin/env python3
"""Generate tests/golden/gen_constraints.npz: the token constraints (sequence_bias, bad_words_ids, forced_bos_token_id, forced_eos_token_id,
suppress_tokens, begin_suppress_tokens) and early_stopping as transformers 5.15.0 and the reference apply them (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gen_constraints.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gen_constraints.py --verify   # rebuild into a scratch directory, require identical arrays

Three kinds of case:
  * kernel: random fp32 score rows [R, V] pushed through the library's OWN processor classes in the order of GenerationMixin._get_logits_processor
    (generation/utils.py:1123-1293): SequenceBias -> RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> MinLength -> ForcedBOS -> ForcedEOS ->
    SuppressTokens -> SuppressTokensAtBegin. The scores are NOT stored: the test redraws them from the recorded torch.Generator seed. Stored: the
    histories, the options as a caller would pass them, and every entry the processors changed (flat index and value).
  * model: greedy decodes of the reference's multi-image and longitudinal models and a beam-4 decode of the multi-image model, with options derived
    FROM the unconstrained decode so that they bite (make_golden_gen_controls.py recipe: margins for greedy, _robust_beam_case for beams).
  * early stopping: the reference's beam-4 generate with the fp32 logits of every step recorded (make_golden.fixture_beam_index recipe, a 48-word
    vocabulary to keep the file small) under early_stopping=True, "never" and False, all with length_penalty 2.0.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import make_golden_gen_controls as gc  # noqa: E402

from transformers.generation.logits_process import (  # noqa: E402
    ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor, LogitsProcessorList, MinLengthLogitsProcessor, NoBadWordsLogitsProcessor,
    NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor, SequenceBiasLogitsProcessor, SuppressTokensAtBeginLogitsProcessor,
    SuppressTokensLogitsProcessor)

from cxrmate_amd.config import tiny_config  # noqa: E402

FILE = "gen_constraints.npz"
BOS, EOS, SEP, PAD, PMT_SEP = mg.BOS, mg.EOS, mg.SEP, mg.PAD, mg.PMT_SEP


def processors(o, V):
    """The library's processors for the options `o`, in the order of _get_logits_processor."""
    p = LogitsProcessorList()
    if o.get("sequence_bias") is not None:
        p.append(SequenceBiasLogitsProcessor(sequence_bias=o["sequence_bias"]))
    if o.get("penalty", 1.0) != 1.0:
        p.append(RepetitionPenaltyLogitsProcessor(penalty=o["penalty"]))
    if o.get("ngram", 0) > 0:
        p.append(NoRepeatNGramLogitsProcessor(o["ngram"]))
    if o.get("bad_words_ids") is not None:
        p.append(NoBadWordsLogitsProcessor(o["bad_words_ids"], EOS))
    if o.get("min_length", 0) > 0:
        p.append(MinLengthLogitsProcessor(o["min_length"], EOS))
    if o.get("forced_bos_token_id") is not None:
        p.append(ForcedBOSTokenLogitsProcessor(o["forced_bos_token_id"]))
    if o.get("forced_eos_token_id") is not None:
        p.append(ForcedEOSTokenLogitsProcessor(o["max_length"], o["forced_eos_token_id"]))
    if o.get("suppress_tokens") is not None:
        p.append(SuppressTokensLogitsProcessor(o["suppress_tokens"]))
    if o.get("begin_suppress_tokens") is not None:
        n = o["prompt_len"]                                            # utils.py:1278-1283
        begin = n if (n > 1 or o.get("forced_bos_token_id") is None) else n + 1
        p.append(SuppressTokensAtBeginLogitsProcessor(o["begin_suppress_tokens"], begin))
    return p


def pack_lists(lists):
    """list of id lists -> (flat int64, lengths int64)."""
    return (np.array([t for w in lists for t in w], dtype=np.int64), np.array([len(w) for w in lists], dtype=np.int64))


def kernel_case(d, i, seed, R, V, cur, ids, logprobs=False, **o):
    x = gc.kernel_scores(seed, R, V, logprobs)
    o.setdefault("prompt_len", 1)
    o.setdefault("max_length", 0)
    y = processors(o, V)(ids[:, :cur], x.clone())
    same = (y == x) | (torch.isnan(y) & torch.isnan(x))
    changed = torch.nonzero((~same).reshape(-1)).reshape(-1)
    assert changed.numel() > 0, f"kernel case {i} changes nothing"
    k = f"k{i}_"
    d[k + "params"] = np.array([seed, R, V, cur, o.get("ngram", 0), o.get("min_length", 0), o["prompt_len"], o["max_length"], int(logprobs),
                                -1 if o.get("forced_bos_token_id") is None else o["forced_bos_token_id"]], dtype=np.int64)
    d[k + "penalty"] = np.array(o.get("penalty", 1.0), dtype=np.float32)
    d[k + "ids"] = ids.numpy()
    sb = o.get("sequence_bias") or []
    d[k + "bias_tok"], d[k + "bias_len"] = pack_lists([e[0] for e in sb])
    d[k + "bias_val"] = np.array([e[1] for e in sb], dtype=np.float64)
    d[k + "bad_tok"], d[k + "bad_len"] = pack_lists(o.get("bad_words_ids") or [])
    feos = o.get("forced_eos_token_id")
    d[k + "forced_eos"] = np.array([] if feos is None else ([feos] if isinstance(feos, int) else feos), dtype=np.int64)
    d[k + "suppress"] = np.array(o.get("suppress_tokens") or [], dtype=np.int64)
    d[k + "begin_suppress"] = np.array(o.get("begin_suppress_tokens") or [], dtype=np.int64)
    d[k + "changed_idx"] = changed.numpy()
    d[k + "changed_val"] = y.reshape(-1)[changed].numpy()
    print(f"kernel case {i}: R={R} V={V} cur={cur}: {changed.numel()} entries changed, {int(torch.isinf(y).sum())} at -inf")
    return i + 1


def kernel_cases(d):
    i = 0
    # (a) sequence_bias, V = 30000, cur = 40: four entries hit token 6 where the history ends in 3 5 7 9 (its single entry and three multi-token
    # ones), a 5-token entry ends in EOS, one entry never matches, one is longer than the history
    g = torch.Generator().manual_seed(721)
    ids = gc.history(g, 6, 40, 30000)
    ids[:4, -4:] = torch.tensor([3, 5, 7, 9])
    ids[4, -2:] = torch.tensor([7, 9])
    sb = [[[5], 0.1], [[7], -0.7], [[29999], 2.3], [[7, 9, 6], 1.5], [[6], 0.1], [[9, 6], -0.25], [[5, 7, 9, 6], 0.3], [[3, 5, 7, 9, 2], 2.3],
          [[1, 2, 3], 0.9], [[9, 11], -1.1], [list(range(1, 42)), 5.0]]
    i = kernel_case(d, i, 21, 6, 30000, 40, ids, sequence_bias=sb)
    # (b) bad words, cur = 5: an [EOS] single (dropped), a word ending in EOS (kept), a word as long as the history (its prefix is the history
    # without its first id), a word whose prefix is the ENTIRE history (one longer than the history: the library skips it), a longer one, a
    # single, a bigram
    g = torch.Generator().manual_seed(722)
    ids = gc.history(g, 6, 5, 1000)
    ids[:3, -2:] = torch.tensor([7, 9])
    h0 = ids[0].tolist()
    bad = [[EOS], [7, 9, EOS], h0[1:] + [50], h0 + [51], h0 + [52, 53], [13], [9, 20]]
    i = kernel_case(d, i, 22, 6, 1000, 5, ids, bad_words_ids=bad)
    # (c) forced_bos at cur = 1 and, same tables, cur = 2 (no-op: only the ban and the suppression act)
    g = torch.Generator().manual_seed(723)
    ids = torch.randint(0, 12, (4, 2), generator=g)
    for cur in (1, 2):
        i = kernel_case(d, i, 23, 4, 300, cur, ids, forced_bos_token_id=5, bad_words_ids=[[5], [6]], suppress_tokens=[7])
    # (d) forced_eos with a 2-id list at cur = max_length - 1 (suppression overrides the forced 0 of id 17) and at max_length - 2 (no-op)
    g = torch.Generator().manual_seed(724)
    ids = gc.history(g, 4, 19, 300)
    for cur in (19, 18):
        i = kernel_case(d, i, 24, 4, 300, cur, ids, forced_eos_token_id=[EOS, 17], max_length=20, suppress_tokens=[17, 30])
    # (e) suppress with duplicates, id 0, id V - 1 and an id >= V; begin_suppress at begin_index and one step later; the +1 shift of begin_index
    # (prompt of length 1 with forced_bos set): cur = 2 fires begin_suppress, cur = 1 the forced row only
    g = torch.Generator().manual_seed(725)
    ids = gc.history(g, 5, 8, 300)
    sup = [0, 0, 299, 5, 5, 303]
    for cur, plen, fbos in ((6, 6, None), (7, 6, None), (2, 1, 4), (1, 1, 4)):
        i = kernel_case(d, i, 25, 5, 300, cur, ids, suppress_tokens=sup, begin_suppress_tokens=[3, 8, 3], prompt_len=plen,
                        forced_bos_token_id=fbos)
    # (f) everything with penalty / n-gram / min-length on log-probs, V = 999 (no multiple of 256), the longest history
    g = torch.Generator().manual_seed(726)
    ids = gc.history(g, 8, 512, 999)
    ids[:5, -3:] = torch.tensor([4, 6, 8])
    sb = [[[6], 0.37], [[8], -1.9], [[6, 8, 10], 0.8], [[10], 0.21], [[4, 6, 8, 10], -0.45], [[8, 3], 1.7], [[998], -0.6]]
    bad = [[EOS], [6, 8, 5], [8, 7], [9], [6, 8, EOS]]
    i = kernel_case(d, i, 26, 8, 999, 512, ids, logprobs=True, sequence_bias=sb, bad_words_ids=bad, penalty=1.3, ngram=3, min_length=600,
                    suppress_tokens=[0, 998, 998, 2000], begin_suppress_tokens=[11, 12], prompt_len=512, forced_eos_token_id=[EOS], max_length=600)
    # ... and the same with forced_eos firing on the longest history (two rows: every entry of a forced row is a changed entry)
    i = kernel_case(d, i, 26, 2, 999, 512, ids[:2], logprobs=True, sequence_bias=sb, bad_words_ids=bad, penalty=1.3, ngram=3, min_length=600,
                    suppress_tokens=[0, 998, 998, 2000], begin_suppress_tokens=[11, 12], prompt_len=512, forced_eos_token_id=[EOS, 6], max_length=513)
    d["n_kernel_cases"] = np.array(i)


# ------------------------------------------------------------------------------------------------ model cases
def plain_tokens(model, kw, max_length, num_beams=1):
    """-> (the unconstrained decode, the number of columns before its first generated one)."""
    with torch.no_grad():
        o = model.generate(**kw, num_beams=num_beams, max_length=max_length, output_scores=True)
    # (a beam search runs more steps than its longest returned hypothesis has tokens; the beam case decodes from BOS alone)
    return o["sequences"], (o["sequences"].shape[1] - len(o["scores"]) if num_beams == 1 else 1)


def ordinary(t):
    return int(t) not in (BOS, EOS, SEP, PAD, PMT_SEP)


def derive_options(plain, P, first_prefix=None):
    """Options that bite, from the unconstrained decode `plain` (P columns before the first generated one): ban row 0's 3rd generated token and a
    bigram of row 1 (with `first_prefix`: the bigram (last prompt id of row 1, its first generated token), so the ban is decided by the prompt),
    begin_suppress the first generated token of the last row, force EOS at a length the decode runs through."""
    g = plain[:, P:]
    assert ordinary(g[0, 2]) and ordinary(g[1, 3]) and ordinary(g[1, 4]) and ordinary(g[-1, 0])
    bigram = [int(first_prefix), int(g[1, 0])] if first_prefix is not None else [int(g[1, 3]), int(g[1, 4])]
    lens = [(row.tolist().index(EOS) + 1 if EOS in row.tolist() else len(row)) for row in g]
    forced_len = P + max(lens) - 2                                     # the longest row is still running there
    assert max(lens) >= 8
    return dict(bad_words_ids=[[int(g[0, 2])], bigram], begin_suppress_tokens=[int(g[-1, 0])], forced_eos_token_id=EOS), forced_len


def store_options(d, name, opts, max_length):
    d[f"{name}_bad_tok"], d[f"{name}_bad_len"] = pack_lists(opts["bad_words_ids"])
    d[f"{name}_begin_suppress"] = np.array(opts["begin_suppress_tokens"], dtype=np.int64)
    d[f"{name}_forced_eos"] = np.array(opts["forced_eos_token_id"], dtype=np.int64)
    d[f"{name}_opts_max_length"] = np.array(max_length)


# the beam model: a seed (searched over 300..419) at which the constrained beam-4 decode is robust under bf16-sized logit noise
# (make_golden._robust_beam_case) and the three studies' best hypotheses are pairwise different
MULTI_BEAM = dict(gc.MULTI, seed=387, pixel_seed=2387)


def model_cases(d):
    model, kw = gc.multi_model(gc.MULTI_GREEDY)
    opts, L = derive_options(*plain_tokens(model, kw, 41))
    gc.greedy_case(d, "multi", model, kw, opts, L)
    store_options(d, "multi_greedy", opts, L)
    assert bool((torch.from_numpy(d["multi_greedy"])[:, -1] == EOS).any())          # the forced EOS ends a row at the length limit

    model, kw = gc.multi_model(MULTI_BEAM)
    opts, L = derive_options(*plain_tokens(model, kw, 11, num_beams=4))
    gc.beam_case(d, "multi", model, kw, opts, L)
    assert int(d["multi_beam4_robust"]) == 1, "the beam case is not robust under logit noise: pick other options"
    store_options(d, "multi_beam", opts, L)

    model, prompt, kw = gc.longi_model()
    plain, P = plain_tokens(model, kw, prompt.shape[1] + 1 + 24)
    opts, L = derive_options(plain, P, first_prefix=plain[1, P - 1])
    gc.greedy_case(d, "longi", model, kw, opts, L)
    store_options(d, "longi", opts, L)
    d["longi_prompt"] = prompt.numpy()
    for k, v in list(gc.MULTI_GREEDY.items()):
        d[f"multi_greedy_{k}"] = np.array(v)
    for k, v in list(MULTI_BEAM.items()):
        d[f"multi_beam_{k}"] = np.array(v)
    for k, v in list(gc.LONGI.items()):
        d[f"longi_{k}"] = np.array(v)


# ------------------------------------------------------------------------------------------------ early stopping
ES = dict(vocab=48, steps=10, seed=52, perturb=0.05, sharpen=16.0, cross_gain=8.0, img_off=1.0, pixel_seed=2052, length_penalty=2.0)
ES_MODES = (("true", True), ("never", "never"), ("false", False))


def es_run(bias, early_stopping):
    cfg = tiny_config(vocab_size=ES["vocab"], decoder_layers=2, depth=(1, 2, 3), image_size=96)
    model, _ = mg.build(mg.MultiCXREncoderDecoderModel, cfg, seed=ES["seed"], perturb=ES["perturb"], sharpen=ES["sharpen"], cross_gain=ES["cross_gain"])
    model.decoder.cls.predictions.bias.data[EOS] += bias
    x = mg.distinct_study_pixels(ES["pixel_seed"], ES["img_off"])
    logits, fed = [], []
    h1 = model.decoder.cls.register_forward_hook(lambda mod, inp, out: logits.append(out[:, -1].detach().float().clone()))
    h2 = model.decoder.bert.embeddings.register_forward_pre_hook(lambda mod, args, kwargs: fed.append(kwargs["input_ids"][:, -1].clone()), with_kwargs=True)
    try:
        with torch.no_grad():
            o = model.generate(pixel_values=x, special_token_ids=[SEP], max_length=ES["steps"] + 1, bos_token_id=BOS, eos_token_id=EOS, pad_token_id=PAD,
                               num_beams=4, num_return_sequences=4, return_dict_in_generate=True, use_cache=True, do_sample=False, output_scores=True,
                               length_penalty=ES["length_penalty"], early_stopping=early_stopping)
    finally:
        h1.remove(); h2.remove()
    return torch.stack(logits), torch.stack(fed), o["sequences"].view(3, 4, -1), o["sequences_scores"].view(3, 4)


def early_stopping_cases(d):
    """The running beams of a search do not depend on early_stopping (it decides what the finished set takes and when the loop ends), so the three
    runs see the same logits as far as each goes: ONE array is stored, that of the longest run, and each mode's number of steps."""
    for bias in (18.0, 20.0, 22.0):
        runs = {name: es_run(bias, mode) for name, mode in ES_MODES}
        n_true, n_false, n_never = (runs[k][0].shape[0] for k in ("true", "false", "never"))
        print(f"early stopping, EOS bias {bias}: steps run True {n_true}, False {n_false}, never {n_never}")
        if n_true < n_false < n_never:
            break
    else:
        raise AssertionError("no EOS bias makes the three modes end on three different steps")
    # True stops because every study's finished set is full: on an earlier step than False, and before the length limit; "never" measures the
    # running beams against the length limit and goes on after False has stopped
    assert n_true < n_false < n_never <= ES["steps"]
    logits, fed = runs["never"][0], runs["never"][1]
    assert logits.shape[1:] == (12, ES["vocab"]) and fed.shape == logits.shape[:2]
    for name, (lg, fd, seqs, sc) in runs.items():
        assert torch.equal(lg, logits[:lg.shape[0]]) and torch.equal(fd, fed[:fd.shape[0]]), name
        d[f"es_{name}_steps"] = np.array(lg.shape[0])
        d[f"es_{name}_all"], d[f"es_{name}_all_scores"] = seqs.numpy(), sc.numpy()
    d["es_logits"], d["es_fed"] = logits.numpy(), fed.numpy()
    d["es_eos_bias"] = np.array(bias)
    for k, v in ES.items():
        d[f"es_{k}"] = np.array(v)


def make(out_dir):
    torch.manual_seed(0)
    d = {}
    kernel_cases(d)
    model_cases(d)
    early_stopping_cases(d)
    np.savez_compressed(os.path.join(out_dir, FILE), **d)


def verify():
    tmp = tempfile.mkdtemp(prefix="golden_gen_constraints_verify_")
    try:
        make(tmp)
        new, old = np.load(os.path.join(tmp, FILE)), np.load(os.path.join(mg.COMMITTED, FILE))
        assert sorted(new.files) == sorted(old.files), set(new.files) ^ set(old.files)
        bad = [k for k in old.files if not np.array_equal(new[k], old[k], equal_nan=True)]
        assert not bad, f"arrays differ: {bad}"
        print(f"verify ok: {len(old.files)} arrays identical")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    if "--verify" in sys.argv[1:]:
        verify()
    else:
        make(mg.OUT)
