#!/usr/bin/env python3
"""Generate tests/golden/gen_scores.npz: the per-step outputs of generate() -- `scores`, `logits`, `beam_indices` -- and
compute_transition_scores, as transformers 5.15.0 returns them through the reference's models (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gen_scores.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gen_scores.py --verify   # rebuild into a scratch directory, require identical arrays

Cases (make_golden.py recipe: seeded random-init weights, sharpened LM head and cross-attention gain, so that decisions clear the bf16 error bound):
  mg  multi-image greedy, study 1 with a zeroed image, an EOS bias that makes the rows end at different steps (ragged EOS)
  mb  multi-image beam-4 with num_return_sequences 1, 2 and 4 and an early EOS (make_golden.BEAM_SAFE recipe, EOS bias 8)
  sg  single-image greedy; sb  single-image beam-4
  lg  longitudinal prompted greedy with repetition_penalty + no_repeat_ngram_size (processed scores != raw logits)
Every greedy decision is asserted to clear 3 x the bf16 logit error (1.2 % of the step's score spread); every beam case is asserted to return the
same hypotheses AND beam indices under bf16-sized logit noise. Stored per case: the recipe, sequences, sequences_scores, beam_indices,
compute_transition_scores, and the raw logits of every step. The scores are stored only where they cannot be derived from the logits (asserted here):
  greedy without processors (mg, sg)  scores == logits: nothing more
  greedy with processors (lg)         the processed entries (flat index, value), as in gen_controls.npz
  beam (mb, sb)                       scores == log_softmax(logits); only the rows [steps, rows] `<case>_keep` the returned hypotheses were chosen
                                      from are stored (`<case>_logits` [kept rows, V]): those rows are what the robustness check pins
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

from cxrmate_amd.config import tiny_config  # noqa: E402

FILE = "gen_scores.npz"
BOS, EOS, SEP, PAD, PMT_SEP = mg.BOS, mg.EOS, mg.SEP, mg.PAD, mg.PMT_SEP
ERR_REL = 0.012                        # bf16 logit error relative to the spread of a step's scores (tests/test_gen_controls_gpu.py)
SHARPEN_SUFFIXES = ("cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias")

# recipe fields: seed, pixel_seed, vocab, max_length | sharpen, cross_gain, img_off, perturb, eos_bias
MG = dict(seed=14, pixel_seed=104, vocab=1000, max_length=13, sharpen=16.0, cross_gain=8.0, img_off=1.0, perturb=0.05)
MB = dict(seed=307, pixel_seed=2307, vocab=200, max_length=11, sharpen=16.0, cross_gain=8.0, img_off=1.0, perturb=0.05, eos_bias=8.0)
SG = dict(seed=41, pixel_seed=1041, vocab=1000, max_length=9, sharpen=16.0, cross_gain=1.0, img_off=0.0, perturb=0.05, eos_bias=0.0)
LG = dict(seed=27, pixel_seed=117, vocab=1000, max_length=0, sharpen=16.0, cross_gain=8.0, img_off=0.0, perturb=0.05, eos_bias=0.0)
LG_OPTS = dict(repetition_penalty=1.2, no_repeat_ngram_size=2)


def recipe(d, name, c):
    d[f"{name}_cfg"] = np.array([c["seed"], c["pixel_seed"], c["vocab"], c["max_length"]], dtype=np.int64)
    d[f"{name}_f"] = np.array([c["sharpen"], c["cross_gain"], c["img_off"], c["perturb"], c["eos_bias"]], dtype=np.float64)


def multi_model(c):
    cfg = tiny_config(vocab_size=c["vocab"], decoder_layers=2, depth=(1, 2, 3), image_size=96)
    model, _ = mg.build(mg.MultiCXREncoderDecoderModel, cfg, seed=c["seed"], perturb=c["perturb"], sharpen=c["sharpen"], cross_gain=c["cross_gain"])
    model.decoder.cls.predictions.bias.data[EOS] += c["eos_bias"]
    x = mg.distinct_study_pixels(c["pixel_seed"], c["img_off"])
    return model, dict(pixel_values=x, special_token_ids=[SEP], bos_token_id=BOS, eos_token_id=EOS, pad_token_id=PAD, use_cache=True,
                       return_dict_in_generate=True, do_sample=False, output_scores=True, output_logits=True, max_length=c["max_length"])


def single_model(c):
    cfg = tiny_config(vocab_size=c["vocab"], decoder_layers=2, depth=(1, 2, 3), image_size=96)
    model, _ = mg.build(mg.SingleCXREncoderDecoderModel, cfg, seed=c["seed"], perturb=c["perturb"], sharpen=c["sharpen"])
    x = torch.randn(3, 3, 96, 96, generator=torch.Generator().manual_seed(c["pixel_seed"]))
    return model, dict(pixel_values=x, special_token_ids=[SEP], bos_token_id=BOS, eos_token_id=EOS, pad_token_id=PAD, use_cache=True,
                       return_dict_in_generate=True, do_sample=False, output_scores=True, output_logits=True, max_length=c["max_length"])


def longi_model(c):
    cfg = tiny_config(vocab_size=c["vocab"], decoder_layers=2, depth=(1, 2, 3), image_size=96, lora_r=8)
    model, _ = mg.build(mg.LongitudinalPromptMultiCXREncoderDecoderModel, cfg, seed=c["seed"], perturb=c["perturb"], longitudinal=True,
                        cross_gain=c["cross_gain"])
    for name, prm in model.named_parameters():                       # the LM head sits under the LoRA wrapper: sharpen it by name
        if name.endswith(SHARPEN_SUFFIXES):
            prm.data.mul_(c["sharpen"])
    g = torch.Generator().manual_seed(c["pixel_seed"])
    x = torch.randn(2, 2, 3, 96, 96, generator=g)
    x[0, 1] = 0.0
    prompt = mg.make_prompt(g, 2, c["vocab"], [8, 5])
    prompt[0, 3] = PAD
    with torch.no_grad():
        eo = model.encoder(x)
    return model, prompt, dict(encoder_outputs=eo, decoder_input_ids=prompt, special_token_ids=[PMT_SEP, BOS, SEP], bos_token_id=BOS,
                               eos_token_id=EOS, pad_token_id=PAD, mask_token_id=PAD, use_cache=True, return_dict_in_generate=True,
                               do_sample=False, output_scores=True, output_logits=True)


def unsafe_steps(out, prompt_len):
    """-> bool [steps]: a step where some still-running row's processed top-1 / top-2 margin is within 3 x the bf16 logit error."""
    sc = torch.stack(out["scores"], 0)                                # [T, R, V]
    fin = torch.isfinite(sc)
    z = torch.where(fin, sc, torch.zeros_like(sc))
    mean = z.sum(-1) / fin.sum(-1)
    std = (torch.where(fin, (sc - mean[..., None]) ** 2, torch.zeros_like(sc)).sum(-1) / fin.sum(-1)).sqrt()
    t2 = torch.topk(sc, 2, dim=-1)[0]
    gen = out["sequences"][:, prompt_len:]
    ended = torch.cumsum((gen == EOS).int(), 1) - (gen == EOS).int() > 0        # rows that finished BEFORE step t (they only emit PAD)
    bad = ((t2[..., 0] - t2[..., 1]) <= 3 * ERR_REL * std) & ~ended.t()[: sc.shape[0]]
    return bad.any(1)


def store(d, name, model, out, n=None, steps_too=True):
    k = name if n is None else f"{name}_n{n}"
    d[f"{k}_seq"] = out["sequences"].numpy()
    beam = "beam_indices" in out and out["beam_indices"] is not None
    ts = model.compute_transition_scores(out["sequences"], out["scores"], out["beam_indices"] if beam else None)
    d[f"{k}_ts"] = ts.numpy()
    if beam:
        d[f"{k}_bidx"] = out["beam_indices"].numpy()
        d[f"{k}_seq_scores"] = out["sequences_scores"].numpy()
        lens = (out["beam_indices"] >= 0).sum(1).float()
        assert torch.allclose(ts.sum(1) / lens, out["sequences_scores"], atol=1e-5), name      # length_penalty 1
    if steps_too:
        sc, lg = torch.stack(out["scores"], 0), torch.stack(out["logits"], 0)          # [steps, rows, V]
        if beam:
            assert torch.equal(sc, torch.log_softmax(lg, -1)), name                  # no processor on the beam cases
            keep = torch.zeros(sc.shape[:2], dtype=torch.bool)
            bidx = out["beam_indices"]
            for t in range(bidx.shape[1]):
                keep[t, bidx[:, t][bidx[:, t] >= 0].long()] = True
            d[f"{name}_keep"] = keep.numpy()
            d[f"{name}_logits"] = lg[keep].numpy()
        else:
            d[f"{name}_logits"] = lg.numpy()
            changed = torch.nonzero((sc != lg).reshape(-1)).reshape(-1)
            if changed.numel():
                d[f"{name}_changed_idx"] = changed.numpy()
                d[f"{name}_changed_val"] = sc.reshape(-1)[changed].numpy()


def robust_beam(model, kw, trials=4, rel=0.02):
    """The hypotheses and beam indices of the search survive bf16-sized logit noise (2 x the measured error)."""
    with torch.no_grad():
        clean = model.generate(**kw)
    for t in range(trials):
        noise = mg._LogitNoise(model, rel, 1000 + t)
        try:
            with torch.no_grad():
                o = model.generate(**kw)
        finally:
            noise.remove()
        if not (torch.equal(o["sequences"], clean["sequences"]) and torch.equal(o["beam_indices"], clean["beam_indices"])):
            return None
    return clean


def greedy_case(d, name, model, kw, c, prompt_len, opts=None):
    with torch.no_grad():
        out = model.generate(**kw, **(opts or {}), num_beams=1)
    bad = unsafe_steps(out, prompt_len)
    assert not bool(bad.any()), (name, torch.nonzero(bad).reshape(-1).tolist())
    recipe(d, name, c)
    store(d, name, model, out)
    gen = out["sequences"][:, prompt_len:]
    print(f"{name}: greedy {tuple(out['sequences'].shape)}, {len(out['scores'])} steps, EOS rows {(gen == EOS).any(1).tolist()}")
    return out


def beam_case(d, name, model, kw, c, ns=(1, 2, 4)):
    full = robust_beam(model, dict(kw, num_beams=4, num_return_sequences=max(ns)))
    assert full is not None, f"{name}: beam indices are not robust under logit noise"
    recipe(d, name, c)
    for n in ns:
        with torch.no_grad():
            out = model.generate(**kw, num_beams=4, num_return_sequences=n)
        store(d, name, model, out, n, steps_too=n == max(ns))
    d[f"{name}_steps"] = np.array(len(full["scores"]))
    ended = bool((full["beam_indices"] < 0).any())
    print(f"{name}: beam-4 {tuple(full['sequences'].shape)}, {len(full['scores'])} steps, a hypothesis ended early: {ended}")
    return full


def make(out_dir):
    torch.manual_seed(0)
    d = {}
    # ---- multi greedy: the smallest EOS bias (steps of 0.5) for which rows end at different steps and every decision is safe
    c = dict(MG)
    for k in range(0, 41):
        c["eos_bias"] = 0.5 * k
        model, kw = multi_model(c)
        with torch.no_grad():
            out = model.generate(**kw, num_beams=1)
        gen = out["sequences"][:, 1:]
        e = gen == EOS
        first = torch.where(e.any(1), e.int().argmax(1), torch.full((gen.shape[0],), 99))
        if bool(e.any()) and len(set(first.tolist())) == gen.shape[0] and not bool(unsafe_steps(out, 1).any()):
            break
    else:
        raise AssertionError("no ragged-EOS bias with safe margins")
    greedy_case(d, "mg", model, kw, c, 1)
    # ---- multi beam-4, early EOS, num_return_sequences 1, 2, 4
    model, kw = multi_model(MB)
    full = beam_case(d, "mb", model, kw, MB)
    assert bool((full["beam_indices"] < 0).any()), "mb: no hypothesis ends early"
    # ---- single greedy and beam-4
    model, kw = single_model(SG)
    greedy_case(d, "sg", model, kw, SG, 1)
    beam_case(d, "sb", model, kw, SG, ns=(1,))
    # ---- longitudinal prompted greedy with processors: the longest safe decode (at least 8 steps)
    model, prompt, kw = longi_model(LG)
    P = prompt.shape[1] + 1
    with torch.no_grad():
        out = model.generate(**kw, **LG_OPTS, num_beams=1, max_length=P + 24)
    bad = torch.nonzero(unsafe_steps(out, P)).reshape(-1).tolist()
    steps = bad[0] if bad else len(out["scores"])
    assert steps >= 8, ("lg", bad)
    c = dict(LG, max_length=P + steps)
    out = greedy_case(d, "lg", model, dict(kw, max_length=c["max_length"]), c, P, LG_OPTS)
    assert not torch.equal(torch.stack(out["scores"]), torch.stack(out["logits"])), "lg: the processors change nothing"
    d["lg_prompt"] = prompt.numpy()
    d["lg_opts"] = np.array([LG_OPTS["repetition_penalty"], LG_OPTS["no_repeat_ngram_size"]], dtype=np.float64)
    np.savez_compressed(os.path.join(out_dir, FILE), **d)
    print(f"wrote {os.path.join(out_dir, FILE)}: {len(d)} arrays, {os.path.getsize(os.path.join(out_dir, FILE)) / 1e6:.2f} MB")


def verify():
    tmp = tempfile.mkdtemp(prefix="golden_gen_scores_verify_")
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
