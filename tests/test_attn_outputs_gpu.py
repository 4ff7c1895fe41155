"""GPU: output_attentions / output_hidden_states of the teacher-forced forward.

  * ops.attention_probs (csrc/attn_probs.hip) against fp32 torch on the same bf16 q / k, with the LSE of ops.attention: masked entries exactly 0,
    rows summing to 1 within 1e-3, values within |d| <= 2e-5 + 2e-3 |ref| (the same bf16 products, fp32 accumulation; only the exp and the
    LSE's own rounding differ);
  * train-mode maps: einsum(P, V) reproduces the context of ops.attention with the same dropout tuple (rel-rms <= 1e-2, bf16 rounding of P.V);
  * the three models against tests/golden/tf_attentions.npz (the reference, eval, fp32): counts, shapes and dtypes exact, masked entries
    exactly 0, values at the model tolerances of test_model_gpu.py (rel-rms <= 2.5e-2, cosine >= 0.9995);
  * asking for the maps changes nothing else: logits, loss and gradients bit-identical, default outputs as before.
"""
import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

ACT_RMS, ACT_COS = 2.5e-2, 0.9995
H, D = 12, 768


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import modelling
    return modelling


def _ref_probs(q, k, heads, scale, kpm, causal, causal_shift):
    """fp32 torch softmax of the same bf16 q / k; a row without a visible key is uniform over all keys (finfo.min in the reference)"""
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    qf = q.float().view(B, Tq, heads, 64)
    kf = k.float().view(B, Tk, heads, 64)
    s = torch.einsum("bihd,bjhd->bhij", qf, kf) * scale
    vis = torch.ones((B, 1, Tq, Tk), dtype=torch.bool, device=q.device)
    if kpm is not None:
        vis = vis & (kpm != 0).view(B, 1, 1, Tk)
    if causal:
        i = torch.arange(Tq, device=q.device).view(Tq, 1)
        j = torch.arange(Tk, device=q.device).view(1, Tk)
        vis = vis & (j <= i + causal_shift).view(1, 1, Tq, Tk)
    vis = vis.expand(B, heads, Tq, Tk)
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1)
    dead = ~vis.any(-1, keepdim=True)
    p = torch.where(dead, torch.full_like(p, 1.0 / Tk), p)
    return p, vis | dead


# (Tq, Tk, causal, kpm, fused): fused = q / k are column blocks of one [B, T, 3D] (self) or k a slice of a [B, S, 4D] buffer (cross)
CASES = [
    (1, 1, False, False, False),
    (13, 72, True, True, True),       # causal with causal_shift = 59 > 0, strided views
    (72, 72, True, True, True),
    (256, 256, True, True, True),
    (72, 13, False, True, False),
    (13, 1152, False, True, True),
    (256, 1728, False, True, True),
    (1152, 72, False, False, True),
    (1728, 1, False, True, False),
]


def _inputs(Tq, Tk, kpm_on, fused, B=2, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if fused and Tq == Tk:
        qkv = torch.randn((B, Tq, 3 * D), generator=g, device="cuda").to(torch.bfloat16)
        q, k, v = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    elif fused:
        q = torch.randn((B, Tq, D), generator=g, device="cuda").to(torch.bfloat16)
        kv = torch.randn((B, Tk, 4 * D), generator=g, device="cuda").to(torch.bfloat16)      # two layers' K / V blocks side by side
        k, v = kv[:, :, 2 * D:3 * D], kv[:, :, 3 * D:]
    else:
        q = torch.randn((B, Tq, D), generator=g, device="cuda").to(torch.bfloat16)
        k = torch.randn((B, Tk, D), generator=g, device="cuda").to(torch.bfloat16)
        v = torch.randn((B, Tk, D), generator=g, device="cuda").to(torch.bfloat16)
    kpm = None
    if kpm_on:
        kpm = torch.ones((B, Tk), dtype=torch.uint8, device="cuda")
        kpm[0, max(1, (2 * Tk) // 3):] = 0                       # right padding
        kpm[0, Tk // 3] = 0 if Tk > 3 else 1                     # an interior masked key
        kpm[B - 1, :] = 0                                        # every key masked: uniform rows
    return q, k, v, kpm


@pytest.mark.parametrize("Tq,Tk,causal,kpm_on,fused", CASES)
def test_attention_probs_match_fp32_torch(M, Tq, Tk, causal, kpm_on, fused):
    from cxrmate_amd import ops
    q, k, v, kpm = _inputs(Tq, Tk, kpm_on, fused)
    scale = 64 ** -0.5
    ctx, lse = ops.attention(q, k, v, H, scale, kpm=kpm, causal=causal, need_lse=True)
    p = ops.attention_probs(q, k, lse, H, scale, kpm=kpm, causal=causal)
    assert p.dtype == torch.float32 and p.shape == (2, H, Tq, Tk) and p.is_contiguous()
    ref, vis = _ref_probs(q, k, H, scale, kpm, causal, Tk - Tq)
    assert torch.isfinite(p).all()
    assert bool((p[~vis] == 0).all()), "masked entries must be exactly 0"
    assert float((p.sum(-1) - 1).abs().max()) <= 1e-3
    err = (p - ref).abs() - (2e-5 + 2e-3 * ref.abs())
    assert float(err.max()) <= 0, f"max |P - ref| {float((p - ref).abs().max()):.3e}"
    # the key-padded uniform rows (every key masked) are the reference's 1 / Tk
    if kpm_on and not causal:
        assert torch.allclose(p[1], torch.full_like(p[1], 1.0 / Tk), rtol=1e-6, atol=0)


def test_attention_probs_into_a_strided_out(M):
    """out= a slice of a wider buffer: the rows land where the strides say, nothing else is written"""
    from cxrmate_amd import ops
    q, k, v, kpm = _inputs(13, 72, True, False)
    scale = 64 ** -0.5
    _, lse = ops.attention(q, k, v, H, scale, kpm=kpm, need_lse=True)
    big = torch.full((2, H, 13, 80), -7.0, device="cuda")
    out = big[:, :, :, 4:76]
    ops.attention_probs(q, k, lse, H, scale, kpm=kpm, out=out)
    ref = ops.attention_probs(q, k, lse, H, scale, kpm=kpm)
    assert torch.equal(out, ref)
    assert bool((big[..., :4] == -7).all()) and bool((big[..., 76:] == -7).all())


@pytest.mark.parametrize("Tq,Tk,causal", [(72, 72, True), (256, 256, True), (13, 1152, False), (256, 1728, False)])
def test_dropout_maps_reproduce_the_forward_context(M, Tq, Tk, causal):
    from cxrmate_amd import ops
    q, k, v, kpm = _inputs(Tq, Tk, True, True, seed=1)
    scale = 64 ** -0.5
    seed = torch.tensor([123457], dtype=torch.int32, device="cuda")
    drop = (0.1, seed, 18, 3)
    ctx, lse = ops.attention(q, k, v, H, scale, kpm=kpm, causal=causal, need_lse=True, drop=drop)
    p = ops.attention_probs(q, k, lse, H, scale, kpm=kpm, causal=causal, drop=drop)
    B = q.shape[0]
    got = torch.einsum("bhij,bjhd->bihd", p, v.float().view(B, Tk, H, 64)).reshape(B, Tq, D)
    # rows compared: all of them, except under the causal rule the rows of the study whose keys are ALL padded. There the forward's context
    # averages the keys of the 64-key tiles it visits, while the maps follow the reference (uniform over all Tk keys); in the model such a
    # row needs a padded first token, which the reports never have.
    rows = slice(None) if not causal else slice(0, 1)
    r = gu.rel_rms(got[rows].cpu().numpy(), ctx[rows].float().cpu().numpy())
    assert r <= 1e-2, f"P.V vs forward context: rel-rms {r:.4f}"
    # about p of the visible entries are dropped, and the kept ones carry 1 / (1 - p)
    p0 = ops.attention_probs(q, k, lse, H, scale, kpm=kpm, causal=causal)
    nz = p0 > 0
    frac = float((p[nz] == 0).float().mean())
    assert 0.07 < frac < 0.13, frac
    kept = nz & (p > 0)
    assert torch.allclose(p[kept], p0[kept] / 0.9, rtol=1e-6, atol=0)
    # a different seed is a different mask: the context no longer matches
    p2 = ops.attention_probs(q, k, lse, H, scale, kpm=kpm, causal=causal, drop=(0.1, seed + 1, 18, 3))
    got2 = torch.einsum("bhij,bjhd->bihd", p2, v.float().view(B, Tk, H, 64)).reshape(B, Tq, D)
    assert gu.rel_rms(got2[rows].cpu().numpy(), ctx[rows].float().cpu().numpy()) > 3e-2


# ------------------------------------------------------------------------------------------------ models against the reference
def _study_pixels(pixel_seed, img_off, size=96):
    x = torch.randn(3, 2, 3, size, size, generator=torch.Generator().manual_seed(pixel_seed))
    for b in range(3):
        x[b] = x[b] * (1.0 + img_off * b) + img_off * b
    x[1, 1] = 0.0
    return x


def _case(M, name):
    from cxrmate_amd import weights
    from cxrmate_amd.config import tiny_config
    g = gu.load("tf_attentions.npz")
    pre = name + "_"
    lora = 8 if name == "longitudinal" else 0
    cfg = tiny_config(vocab_size=1000, decoder_layers=2, depth=(1, 2, 3), image_size=96, lora_r=lora)
    sd = weights.init_encoder_decoder(cfg, seed=int(g[pre + "seed"]), perturb=float(g[pre + "perturb"]))
    cls = {"multi": M.MultiCXREncoderDecoderModel, "single": M.SingleCXREncoderDecoderModel,
           "longitudinal": M.LongitudinalPromptMultiCXREncoderDecoderModel}[name]
    m = cls(cfg, seed=None)
    m.load_state_dict(sd)
    if name == "multi":
        x = _study_pixels(int(g[pre + "pixel_seed"]), float(g[pre + "img_off"]))
        x[int(g[pre + "zero_study"])] = 0.0
    elif name == "single":
        x = torch.randn(2, 3, 96, 96, generator=torch.Generator().manual_seed(int(g[pre + "pixel_seed"])))
    else:
        x = torch.randn(2, 2, 3, 96, 96, generator=torch.Generator().manual_seed(int(g[pre + "pixel_seed"])))
        zi = g[pre + "zero_image"]
        x[int(zi[0]), int(zi[1])] = 0.0
    kw = dict(decoder_input_ids=torch.from_numpy(g[pre + "ids"]).cuda(), decoder_attention_mask=torch.from_numpy(g[pre + "attention_mask"]).cuda(),
              decoder_token_type_ids=torch.from_numpy(g[pre + "token_type_ids"]).cuda())
    if pre + "position_ids" in g.files:
        kw["decoder_position_ids"] = torch.from_numpy(g[pre + "position_ids"]).cuda()
    return g, pre, m, x.cuda(), kw


@pytest.mark.parametrize("name", ["multi", "single", "longitudinal"])
def test_model_maps_and_states_match_the_reference(M, name):
    g, pre, m, x, kw = _case(M, name)
    with torch.no_grad():
        out = m(pixel_values=x, output_attentions=True, output_hidden_states=True, return_dict=True, **kw)
    assert list(out.keys()) == ["loss", "logits", "past_key_values", "decoder_hidden_states", "decoder_attentions", "cross_attentions",
                                "encoder_last_hidden_state"]
    hs, sa, ca = out.decoder_hidden_states, out.decoder_attentions, out.cross_attentions
    assert isinstance(hs, tuple) and isinstance(sa, tuple) and isinstance(ca, tuple)
    assert (len(hs), len(sa), len(ca)) == (int(g[pre + "n_hidden"]), int(g[pre + "n_self"]), int(g[pre + "n_cross"]))
    for i, h in enumerate(hs):
        assert h.dtype == torch.float32 and tuple(h.shape) == tuple(int(s) for s in g[pre + f"hidden{i}_shape"])
        assert not h.requires_grad
        check = gu.sample(h, 2048)
        r, c = gu.rel_rms(check, g[pre + f"hidden{i}_sample"]), gu.cosine(check, g[pre + f"hidden{i}_sample"])
        assert r <= ACT_RMS and c >= ACT_COS, f"{name} hidden {i}: rel_rms {r:.4f} cosine {c:.6f}"
    for kind, maps in (("self", sa), ("cross", ca)):
        for i, a in enumerate(maps):
            ref = g[pre + f"{kind}{i}"]
            assert a.dtype == torch.float32 and tuple(a.shape) == ref.shape, (kind, i, tuple(a.shape), ref.shape)
            a = a.cpu().numpy()
            assert np.isfinite(a).all()
            assert (a[ref == 0] == 0).all(), f"{name} {kind} {i}: entries the reference masks must be exactly 0"
            assert np.abs(a.sum(-1) - 1).max() <= 1e-3
            r, c = gu.rel_rms(a, ref), gu.cosine(a, ref)
            assert r <= ACT_RMS and c >= ACT_COS, f"{name} {kind} {i}: rel_rms {r:.4f} cosine {c:.6f}"


def test_model_inputs_embeds_path_returns_the_same_maps(M):
    g, pre, m, x, kw = _case(M, "multi")
    ids = kw.pop("decoder_input_ids")
    word = m.state_dict()["decoder.bert.embeddings.word_embeddings.weight"].cuda()
    with torch.no_grad():
        a = m(pixel_values=x, decoder_input_ids=ids, output_attentions=True, output_hidden_states=True, **kw)
        b = m(pixel_values=x, decoder_inputs_embeds=word[ids], output_attentions=True, output_hidden_states=True, **kw)
    for f in ("decoder_hidden_states", "decoder_attentions", "cross_attentions"):
        assert len(a[f]) == len(b[f])
        for s, t in zip(a[f], b[f]):
            assert s.shape == t.shape and torch.allclose(s, t, rtol=1e-3, atol=1e-5), f


# ------------------------------------------------------------------------------------------------ nothing else changes
def test_default_outputs_are_unchanged(M):
    g, pre, m, x, kw = _case(M, "multi")
    with torch.no_grad():
        plain = m(pixel_values=x, return_dict=True, **kw)
        flags = m(pixel_values=x, output_attentions=True, output_hidden_states=True, return_dict=True, **kw)
        off = m(pixel_values=x, output_attentions=False, output_hidden_states=False, return_dict=True, **kw)
        tup = m(pixel_values=x, return_dict=False, **kw)
        tup_flags = m(pixel_values=x, output_attentions=True, return_dict=False, **kw)
    assert list(plain.keys()) == ["loss", "logits", "past_key_values", "encoder_last_hidden_state"]
    assert list(off.keys()) == list(plain.keys()) and len(off.to_tuple()) == len(plain.to_tuple()) == len(tup)
    assert plain.decoder_attentions is None and plain.cross_attentions is None and plain.decoder_hidden_states is None
    assert torch.equal(plain.logits, flags.logits) and torch.equal(plain.logits, off.logits) and torch.equal(plain.logits, tup[0])
    assert torch.equal(plain[0], flags[0])
    # HF field order in the tuple form: logits, decoder_attentions, cross_attentions, encoder_last_hidden_state
    assert len(tup_flags) == 4 and torch.equal(tup_flags[0], plain.logits)
    assert len(tup_flags[1]) == 2 and tup_flags[1][0].shape == (3, H, 13, 13) and tup_flags[2][0].shape == (3, H, 13, 72)


def test_only_attentions_or_only_hidden_states(M):
    g, pre, m, x, kw = _case(M, "single")
    with torch.no_grad():
        a = m(pixel_values=x, output_attentions=True, **kw)
        h = m(pixel_values=x, output_hidden_states=True, **kw)
    assert "decoder_hidden_states" not in a and len(a.decoder_attentions) == 2 and len(a.cross_attentions) == 2
    assert "decoder_attentions" not in h and "cross_attentions" not in h and len(h.decoder_hidden_states) == 3


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_flags_leave_train_mode_logits_loss_and_gradients_bit_identical(M):
    g, pre, m, x, kw = _case(M, "multi")
    m.train()
    for p in m.parameters():
        p.requires_grad_(True)
    lab = torch.roll(kw["decoder_input_ids"], -1, 1)

    def run(flags):
        for p in m.parameters():
            p.grad = None
        torch.manual_seed(77)                                   # the same dropout seeds for both passes
        out = m(pixel_values=x, labels=lab, output_attentions=flags, output_hidden_states=flags, return_dict=True, **kw)
        out.loss.backward()
        torch.cuda.synchronize()
        return out, _grads(m)

    a, ga = run(False)
    b, gb = run(True)
    c, gc = run(False)                                          # control: what two identical calls agree on
    assert torch.equal(a.logits, c.logits) and torch.equal(a.loss, c.loss)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.loss, b.loss)
    assert ga.keys() == gb.keys() == gc.keys() and len(ga) > 0
    # the word / position / token-type table gradients are fp32 atomic scatter-adds (csrc/misc.hip): their summation order, and so their last
    # bits, differ between any two calls; every other gradient is bit-exact
    scatter = {n for n in ga if n.endswith("_embeddings.weight")}
    assert {n for n in ga if not torch.equal(ga[n], gc[n])} <= scatter
    differ = [n for n in ga if n not in scatter and not torch.equal(ga[n], gb[n])]
    assert not differ, differ
    for n in scatter:
        assert torch.allclose(ga[n], gb[n], rtol=1e-5, atol=1e-7), n
    maps = (*b.decoder_hidden_states, *b.decoder_attentions, *b.cross_attentions)
    assert len(maps) == 3 + 2 + 2 and not any(t.requires_grad for t in maps)
    # train-mode maps are post-dropout: some visible entries are exactly 0, the kept ones are scaled by 1 / (1 - p)
    with torch.no_grad():
        m.eval()
        e = m(pixel_values=x, output_attentions=True, **kw)
    sa = b.decoder_attentions[0]
    assert bool(((sa == 0) & (e.decoder_attentions[0] > 0)).any())
    rows = sa.sum(-1)
    assert float(rows.mean()) == pytest.approx(1.0, abs=0.05)


def test_flags_leave_eval_logits_bit_identical_for_every_model(M):
    for name in ("multi", "single", "longitudinal"):
        g, pre, m, x, kw = _case(M, name)
        with torch.no_grad():
            a = m(pixel_values=x, **kw).logits
            b = m(pixel_values=x, output_attentions=True, output_hidden_states=True, **kw).logits
        assert torch.equal(a, b), name
