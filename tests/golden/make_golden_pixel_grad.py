#!/usr/bin/env python3
"""Generate tests/golden/pixel_grad.npz: `pixel_values.grad` of the REFERENCE's MultiCXREncoderDecoderModel (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pixel_grad.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pixel_grad.py --verify   # rebuild into a scratch directory, require identical arrays

Recipe (make_golden.py: seeded random-init weights): tiny_config(image_size=96), eval mode, pixel_values [2, 2, 3, 96, 96] with one zero-padded
image, seeded report ids, teacher-forced cross-entropy (ignore_index = PAD) -> backward to the pixels. Stored: the recipe, the ids, the loss, the
per-image L2 norms of the gradient [2, 2] and its values at 4096 seeded flat indices (the gradient is dense: 110592 elements).
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

FILE = "pixel_grad.npz"
SEED, PERTURB, PIXEL_SEED, INDEX_SEED, N_INDEX = 61, 0.05, 161, 261, 4096


def make(out_dir):
    torch.manual_seed(0)
    cfg = tiny_config(vocab_size=1000, decoder_layers=2, depth=(1, 2, 3), image_size=96)
    model, _ = mg.build(mg.MultiCXREncoderDecoderModel, cfg, seed=SEED, perturb=PERTURB)
    g = torch.Generator().manual_seed(PIXEL_SEED)
    x = torch.randn(2, 2, 3, 96, 96, generator=g)
    x[1, 1] = 0.0                                                     # zero-padded image of a ragged study
    full = mg.rand_report_ids(g, 2, 17, 1000, [6, 9], [17, 12])
    attn = (full != mg.PAD).long()
    inp, lab, am = full[:, :-1], full[:, 1:].clone(), attn[:, 1:]
    tt = model.token_ids_to_token_type_ids(inp, [mg.SEP])
    x.requires_grad_(True)
    out = model(pixel_values=x, decoder_input_ids=inp, decoder_attention_mask=am, decoder_token_type_ids=tt, return_dict=True)
    loss = torch.nn.functional.cross_entropy(out.logits.permute(0, 2, 1), lab, ignore_index=mg.PAD)
    loss.backward()
    gr = x.grad.detach()
    idx = torch.randperm(gr.numel(), generator=torch.Generator().manual_seed(INDEX_SEED))[:N_INDEX].sort()[0]
    d = {"seed": np.array(SEED), "perturb": np.array(PERTURB), "pixel_seed": np.array(PIXEL_SEED), "index_seed": np.array(INDEX_SEED),
         "depth": np.array(cfg.encoder.depth), "full_ids": full.numpy(), "token_type_ids": tt.numpy(), "loss": np.array(loss.item()),
         "grad_shape": np.array(gr.shape), "grad_image_norms": gr.double().flatten(2).norm(dim=2).numpy(),
         "grad_index": idx.numpy(), "grad_values": gr.reshape(-1)[idx].numpy()}
    # eval mode: nothing couples the images of a batch and the tokens of the zero-padded image are masked out of the cross-attention
    norms = d["grad_image_norms"]
    assert norms[1, 1] == 0.0 and bool((np.delete(norms.ravel(), 3) > 0).all()), norms
    path = os.path.join(out_dir, FILE)
    np.savez_compressed(path, **d)
    print(f"wrote {path}: loss {loss.item():.5f}, image norms {d['grad_image_norms'].ravel()}, {os.path.getsize(path) / 1e3:.1f} KB")


def verify():
    tmp = tempfile.mkdtemp(prefix="golden_pixel_grad_verify_")
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
