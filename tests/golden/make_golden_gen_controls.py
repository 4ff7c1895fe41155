#!/usr/bin/env python3
"""Generate tests/golden/gen_controls.npz: the generation controls (repetition_penalty, no_repeat_ngram_size, min_length, min_new_tokens,
num_return_sequences) as transformers 5.15.0 and the reference apply them (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gen_controls.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gen_controls.py --verify   # rebuild into a scratch directory, require identical arrays

Two kinds of case:
  * kernel: random fp32 score rows [R, V] (V up to 30000; raw logits, or log-probs as the beam path feeds them) with histories full of duplicates
    and repeated n-grams, pushed through TF5's RepetitionPenalty -> NoRepeatNGram -> MinLength -> MinNewTokensLength (generation/utils.py order).
    The scores are NOT stored: the test redraws them from the recorded torch.Generator seed. Stored: the histories, the parameters, and every
    entry the processors changed (flat index and value).
  * model: greedy decodes of the reference's multi-image and longitudinal models and beam-4 decodes of the multi-image model (the library's
    beam search cannot start from a given decoder prompt: it fails expanding the longitudinal prompt to the beams). make_golden.py recipe:
    seeded random-init weights, sharpened LM head and cross-attention gain so that decisions clear the bf16 error bound. Greedy cases keep
    per-step top-1/top-2 margins of the processed scores; beam cases a robustness check under logit noise (make_golden._robust_beam_case) and
    every returned hypothesis and its score (num_return_sequences 4 and 2).
Every processed decode is asserted to differ from the same decode without the options.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

from transformers.generation.logits_process import (  # noqa: E402
    LogitsProcessorList, MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
    RepetitionPenaltyLogitsProcessor)

from cxrmate_amd.config import tiny_config  # noqa: E402

FILE = "gen_controls.npz"
BOS, EOS, SEP, PAD, PMT_SEP = mg.BOS, mg.EOS, mg.SEP, mg.PAD, mg.PMT_SEP

# (seed, R, V, cur, penalty, ngram, min_length, prompt_len, min_new_tokens, logprobs)
KERNEL_CASES = [
    (11, 6, 30000, 40, 1.3, 3, 0, 0, 0, False),
    (12, 6, 30000, 120, 1.2, 2, 130, 0, 0, False),
    (13, 4, 1000, 2, 1.5, 3, 0, 0, 0, False),          # cur < n: no ban
    (14, 4, 1000, 3, 1.5, 4, 0, 0, 0, False),          # cur = n - 1: no complete window
    (15, 8, 1000, 64, 0.7, 1, 0, 40, 30, False),       # penalty < 1, unigram ban, min_new_tokens
    (16, 8, 200, 200, 1.3, 2, 0, 10, 4, True),         # log-probs (beam path)
    (17, 5, 30000, 512, 2.0, 4, 600, 0, 0, True),      # longest history
    (18, 3, 999, 17, 1.0, 3, 20, 8, 0, False),         # ban + min length only
]


def history(g, R, cur, V):
    """Ids from a small alphabet (duplicates), with a repeated phrase planted in each row (repeated n-grams), EOS in some rows."""
    ids = torch.randint(0, min(V, 12), (R, cur), generator=g)
    for r in range(R):
        if cur >= 8:
            L = int(torch.randint(2, 5, (1,), generator=g))
            a = int(torch.randint(0, cur - L, (1,), generator=g))
            b = int(torch.randint(0, cur - L, (1,), generator=g))
            ids[r, b:b + L] = ids[r, a:a + L].clone()
            ids[r, cur - L:] = ids[r, a:a + L].clone()         # the history ends in a phrase seen before: its successor is banned
        if r % 2 and cur > 3:
            ids[r, cur // 3] = EOS
    return ids


def kernel_scores(seed, R, V, logprobs):
    x = torch.randn(R, V, generator=torch.Generator().manual_seed(seed)) * 3.0
    return torch.log_softmax(x, dim=-1) if logprobs else x


def processors(penalty, ngram, min_length, prompt_len, min_new, eos):
    p = LogitsProcessorList()
    if penalty != 1.0:
        p.append(RepetitionPenaltyLogitsProcessor(penalty=penalty))
    if ngram > 0:
        p.append(NoRepeatNGramLogitsProcessor(ngram))
    if min_length > 0:
        p.append(MinLengthLogitsProcessor(min_length, eos))
    if min_new > 0:
        p.append(MinNewTokensLengthLogitsProcessor(prompt_len, min_new, eos))
    return p


def kernel_cases(d):
    for i, (seed, R, V, cur, pen, n, mlen, plen, mnew, lp) in enumerate(KERNEL_CASES):
        g = torch.Generator().manual_seed(seed + 500)
        ids = history(g, R, cur, V)
        x = kernel_scores(seed, R, V, lp)
        y = processors(pen, n, mlen, plen, mnew, EOS)(ids, x.clone())
        changed = torch.nonzero((y != x).reshape(-1)).reshape(-1)
        assert changed.numel() > 0
        k = f"k{i}_"
        d[k + "params"] = np.array([seed, R, V, cur, n, mlen, plen, mnew, int(lp)], dtype=np.int64)
        d[k + "penalty"] = np.array(pen, dtype=np.float32)
        d[k + "ids"] = ids.numpy()
        d[k + "changed_idx"] = changed.numpy()
        d[k + "changed_val"] = y.reshape(-1)[changed].numpy()
        print(f"kernel case {i}: R={R} V={V} cur={cur} n={n} penalty={pen}: {changed.numel()} entries changed, "
              f"{int(torch.isinf(y).sum())} banned")
    d["n_kernel_cases"] = np.array(len(KERNEL_CASES))


# ------------------------------------------------------------------------------------------------ model cases
SHARPEN_SUFFIXES = ("cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias")
MULTI_GREEDY = dict(seed=14, pixel_seed=104, vocab=1000, sharpen=16.0, cross_gain=8.0, img_off=1.0, perturb=0.05)
MULTI = dict(seed=369, pixel_seed=2369, vocab=200, sharpen=16.0, cross_gain=8.0, img_off=1.0, perturb=0.05)
GREEDY_OPTS = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=5)
BEAM_OPTS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3)
LONGI = dict(seed=15, pixel_seed=105, vocab=1000, sharpen=16.0, cross_gain=8.0, perturb=0.05)
LONGI_OPTS = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=4)


def multi_model(c):
    cfg = tiny_config(vocab_size=c["vocab"], decoder_layers=2, depth=(1, 2, 3), image_size=96)
    model, _ = mg.build(mg.MultiCXREncoderDecoderModel, cfg, seed=c["seed"], perturb=c["perturb"], sharpen=c["sharpen"], cross_gain=c["cross_gain"])
    x = mg.distinct_study_pixels(c["pixel_seed"], c["img_off"])
    return model, dict(pixel_values=x, special_token_ids=[SEP], bos_token_id=BOS, eos_token_id=EOS, pad_token_id=PAD, use_cache=True,
                       return_dict_in_generate=True, do_sample=False)


def longi_model():
    cfg = tiny_config(vocab_size=LONGI["vocab"], decoder_layers=2, depth=(1, 2, 3), image_size=96, lora_r=8)
    model, _ = mg.build(mg.LongitudinalPromptMultiCXREncoderDecoderModel, cfg, seed=LONGI["seed"], perturb=LONGI["perturb"], longitudinal=True,
                        cross_gain=LONGI["cross_gain"])
    for name, prm in model.named_parameters():                       # the LM head sits under the LoRA wrapper: sharpen it by name
        if name.endswith(SHARPEN_SUFFIXES):
            prm.data.mul_(LONGI["sharpen"])
    g = torch.Generator().manual_seed(LONGI["pixel_seed"])
    x = torch.randn(2, 2, 3, 96, 96, generator=g)
    x[0, 1] = 0.0
    prompt = mg.make_prompt(g, 2, LONGI["vocab"], [8, 5])
    prompt[0, 3] = PAD                                               # an interior PAD inside the prompt (masked, still part of the history)
    with torch.no_grad():
        eo = model.encoder(x)
    return model, prompt, dict(encoder_outputs=eo, decoder_input_ids=prompt, special_token_ids=[PMT_SEP, BOS, SEP], bos_token_id=BOS,
                               eos_token_id=EOS, pad_token_id=PAD, mask_token_id=PAD, use_cache=True, return_dict_in_generate=True, do_sample=False)


def greedy_case(d, name, model, kw, opts, max_length):
    with torch.no_grad():
        out = model.generate(**kw, **opts, num_beams=1, max_length=max_length, output_scores=True)
        plain = model.generate(**kw, num_beams=1, max_length=max_length)["sequences"]
    seq = out["sequences"]
    sc = torch.stack(out["scores"], 1)                               # processed scores [B, steps, V]
    t2 = torch.topk(sc, 2, dim=-1)[0]
    margin = (t2[..., 0] - t2[..., 1]).numpy()
    fin = torch.isfinite(sc)
    z = torch.where(fin, sc, torch.zeros_like(sc))
    mean = z.sum(-1) / fin.sum(-1)
    spread = (torch.where(fin, (sc - mean[..., None]) ** 2, torch.zeros_like(sc)).sum(-1) / fin.sum(-1)).sqrt().numpy()   # std of the finite scores
    assert plain.shape != seq.shape or not torch.equal(plain, seq), f"{name}: the options change nothing"
    d[f"{name}_greedy"] = seq.numpy()
    d[f"{name}_greedy_margin"] = margin
    d[f"{name}_greedy_std"] = spread
    d[f"{name}_greedy_plain"] = plain.numpy()
    d[f"{name}_max_length"] = np.array(max_length)
    print(f"{name} greedy {tuple(seq.shape)}: min margin {margin.min():.3f}; rows {seq[:, -8:].tolist()}")


def beam_case(d, name, model, kw, opts, max_length):
    bkw = dict(kw, **opts, num_beams=4, num_return_sequences=4, max_length=max_length, output_scores=True)
    # (the library cannot expand a given decoder prompt to beams x num_return_sequences rows: prompted cases keep the best hypothesis only)
    prompted = "decoder_input_ids" in kw
    res = None if prompted else mg._robust_beam_case(model, bkw, trials=4, min_rel_gap=0.05)
    robust = res is not None
    if not robust:                                                   # kept as a reference run; the test then checks the well-formedness only
        with torch.no_grad():
            o = model.generate(**dict(bkw, num_return_sequences=1 if prompted else 4))
        sc = o["sequences_scores"].view(o["sequences_scores"].shape[0] // (1 if prompted else 4), -1)
        seqs, tol = o["sequences"].view(sc.shape[0], sc.shape[1], -1), 0.0
    else:
        seqs, sc, tol = res
    B = sc.shape[0]
    with torch.no_grad():
        plain = model.generate(**dict(kw, num_beams=4, max_length=max_length))["sequences"]
        if not prompted:
            two = model.generate(**dict(bkw, num_return_sequences=2))
            assert torch.equal(two["sequences"].view(B, 2, -1), seqs[:, :2, :two["sequences"].shape[-1]])
            d[f"{name}_beam4_n2"] = two["sequences"].numpy()
            d[f"{name}_beam4_n2_scores"] = two["sequences_scores"].numpy()
    assert plain.shape[-1] != seqs.shape[-1] or not torch.equal(plain, seqs[:, 0]), f"{name}: the options change nothing"
    d[f"{name}_beam4_all"] = seqs.numpy()
    d[f"{name}_beam4_all_scores"] = sc.numpy()
    d[f"{name}_beam4_tol"] = np.array(tol)
    d[f"{name}_beam4_robust"] = np.array(int(robust))
    d[f"{name}_beam4_plain"] = plain.numpy()
    print(f"{name} beam4 {tuple(seqs.shape)}: robust {robust} tol {tol:.4f}; best {seqs[:, 0].tolist()}")


def make(out_dir):
    torch.manual_seed(0)
    d = {}
    kernel_cases(d)
    model, kw = multi_model(MULTI_GREEDY)
    greedy_case(d, "multi", model, kw, GREEDY_OPTS, 41)
    model, kw = multi_model(MULTI)
    beam_case(d, "multi", model, kw, BEAM_OPTS, 11)
    model, prompt, kw = longi_model()
    greedy_case(d, "longi", model, kw, LONGI_OPTS, prompt.shape[1] + 1 + 24)
    d["longi_prompt"] = prompt.numpy()
    for k, v in list(MULTI_GREEDY.items()):
        d[f"multi_greedy_{k}"] = np.array(v)
    for k, v in list(MULTI.items()):
        d[f"multi_beam_{k}"] = np.array(v)
    for k, v in list(LONGI.items()):
        d[f"longi_{k}"] = np.array(v)
    for pre, opts in (("greedy_opts", GREEDY_OPTS), ("beam_opts", BEAM_OPTS), ("longi_opts", LONGI_OPTS)):
        d[pre] = np.array([opts["repetition_penalty"], opts["no_repeat_ngram_size"], opts["min_new_tokens"]], dtype=np.float64)
    np.savez_compressed(os.path.join(out_dir, FILE), **d)


def verify():
    tmp = tempfile.mkdtemp(prefix="golden_gen_controls_verify_")
    try:
        make(tmp)
        new, old = np.load(os.path.join(tmp, FILE)), np.load(os.path.join(mg.COMMITTED, FILE))
        assert sorted(new.files) == sorted(old.files), set(new.files) ^ set(old.files)
        bad = [k for k in old.files if not np.array_equal(new[k], old[k])]
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
