#!/usr/bin/env python3
"""Generate tests/golden/tf_attentions.npz: the reference models' output_attentions / output_hidden_states (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attn.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attn.py --verify   # rebuild into a scratch directory, require identical arrays

Same recipe as make_golden.py (imported as a module: its model builder, report / prompt ids and study pixels): the reference's own
model classes with seeded random-init weights, eval(), fp32, CPU, eager attention. Three cases, each with its inputs:
  * multi:        3 studies x 2 images, study 1 with a zero-padded image, study 2 all zero (every cross key masked: uniform rows),
                  right-padded reports of different lengths;
  * single:       one image per report, no encoder mask;
  * longitudinal: LoRA decoder, a right-padded prompt in front of the report (masked tokens inside the sequence), explicit position ids.
Pixels are not stored: each case records the torch.Generator seed of its torch.randn draw (and which images it zeroes).
The attention maps are stored whole (<name>_self{l}, <name>_cross{l}); the hidden states as a strided sample and stats, like the other fixtures.
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

FILE = "tf_attentions.npz"


def _store(d, name, out, inputs):
    for k, v in inputs.items():
        d[f"{name}_{k}"] = v.numpy() if torch.is_tensor(v) else np.array(v)
    hs, sa, ca = out.decoder_hidden_states, out.decoder_attentions, out.cross_attentions
    d[f"{name}_n_hidden"], d[f"{name}_n_self"], d[f"{name}_n_cross"] = np.array(len(hs)), np.array(len(sa)), np.array(len(ca))
    for i, h in enumerate(hs):
        d[f"{name}_hidden{i}_sample"] = mg.sample(h, 2048)
        d[f"{name}_hidden{i}_stats"] = mg.stats(h)
        d[f"{name}_hidden{i}_shape"] = np.array(h.shape)
    for i, a in enumerate(sa):
        d[f"{name}_self{i}"] = a.detach().float().numpy()
    for i, a in enumerate(ca):
        d[f"{name}_cross{i}"] = a.detach().float().numpy()
    print(name, "hidden", len(hs), "self", tuple(sa[0].shape), "cross", tuple(ca[0].shape))


def case_multi(d):
    cfg = tiny_config(vocab_size=1000, decoder_layers=2, depth=(1, 2, 3), image_size=96)
    model, _ = mg.build(mg.MultiCXREncoderDecoderModel, cfg, seed=14, perturb=0.05)
    x = mg.distinct_study_pixels(104, 0.5)
    x[2] = 0.0                                                       # a study whose images are all zero: no cross key visible
    g = torch.Generator().manual_seed(104)
    ids = mg.rand_report_ids(g, 3, 13, 1000, [4, 6, 3], [13, 9, 6])
    am = (ids != mg.PAD).long()
    tt = model.token_ids_to_token_type_ids(ids, [mg.SEP])
    with torch.no_grad():
        out = model(pixel_values=x, decoder_input_ids=ids, decoder_attention_mask=am, decoder_token_type_ids=tt,
                    output_attentions=True, output_hidden_states=True, return_dict=True)
    _store(d, "multi", out, dict(seed=14, perturb=0.05, pixel_seed=104, img_off=0.5, zero_study=2, ids=ids, attention_mask=am, token_type_ids=tt))


def case_single(d):
    cfg = tiny_config(vocab_size=1000, decoder_layers=2, depth=(1, 2, 3), image_size=96)
    model, _ = mg.build(mg.SingleCXREncoderDecoderModel, cfg, seed=15, perturb=0.05)
    x = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(105))
    g = torch.Generator().manual_seed(205)
    ids = mg.rand_report_ids(g, 2, 11, 1000, [5, 3], [11, 7])
    am = (ids != mg.PAD).long()
    tt = model.token_ids_to_token_type_ids(ids, [mg.SEP])
    with torch.no_grad():
        out = model(pixel_values=x, decoder_input_ids=ids, decoder_attention_mask=am, decoder_token_type_ids=tt,
                    output_attentions=True, output_hidden_states=True, return_dict=True)
    _store(d, "single", out, dict(seed=15, perturb=0.05, pixel_seed=105, ids=ids, attention_mask=am, token_type_ids=tt))


def case_longitudinal(d):
    cfg = tiny_config(vocab_size=1000, decoder_layers=2, depth=(1, 2, 3), image_size=96, lora_r=8)
    model, _ = mg.build(mg.LongitudinalPromptMultiCXREncoderDecoderModel, cfg, seed=16, perturb=0.05, longitudinal=True)
    x = torch.randn(2, 2, 3, 96, 96, generator=torch.Generator().manual_seed(106))
    x[0, 1] = 0.0
    g = torch.Generator().manual_seed(206)
    prompt = mg.make_prompt(g, 2, 1000, [9, 5])
    full = mg.rand_report_ids(g, 2, 12, 1000, [4, 6], [12, 9])
    inp = torch.cat([prompt, full[:, :-1]], dim=1)
    am = torch.cat([(prompt != mg.PAD).long(), (full != mg.PAD).long()[:, 1:]], dim=1)     # row 1: padded prompt -> masked tokens inside
    pos = torch.nn.functional.relu(torch.cumsum(am, dim=1) - 1)
    tt = model.token_ids_to_token_type_ids(inp, [mg.PMT_SEP, mg.BOS, mg.SEP], [0, 1, 0, 1])
    with torch.no_grad():
        out = model(pixel_values=x, decoder_input_ids=inp, decoder_attention_mask=am, decoder_token_type_ids=tt, decoder_position_ids=pos,
                    output_attentions=True, output_hidden_states=True, return_dict=True)
    _store(d, "longitudinal", out, dict(seed=16, perturb=0.05, pixel_seed=106, zero_image=(0, 1), ids=inp, attention_mask=am, token_type_ids=tt, position_ids=pos))


def make(out_dir):
    import transformers
    d = {"transformers": np.array(transformers.__version__), "torch": np.array(torch.__version__)}
    case_multi(d)
    case_single(d)
    case_longitudinal(d)
    np.savez_compressed(os.path.join(out_dir, FILE), **d)


def verify():
    tmp = tempfile.mkdtemp(prefix="golden_attn_verify_")
    try:
        make(tmp)
        new, old = np.load(os.path.join(tmp, FILE)), np.load(os.path.join(mg.COMMITTED, FILE))
        assert sorted(new.files) == sorted(old.files), set(new.files) ^ set(old.files)
        bad = [k for k in old.files if not np.array_equal(new[k], old[k])]
        assert not bad, f"{FILE}: arrays differ after rebuild: {bad}"
        print(f"{FILE}: rebuilt identically ({len(old.files)} arrays)")
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    if "--verify" in sys.argv[1:]:
        verify()
    else:
        make(mg.OUT)
