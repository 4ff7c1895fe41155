"""GPU: pixel gradients -- pixel_values.grad through the CvT encoder backward.

  kernel  cxr_patch_embed_dgrad_f32 (csrc/conv.hip) against float64 on the bf16-rounded operands it multiplies. Per element
          |got - ref| <= (n + 1) * 2^-24 * sum |de * w| + 1/2 ulp32(ref)   (pixel_grad_ref.dgrad_bound: derived, not measured),
          exact 0.0 where no output position covers a pixel, guard sentinels intact, the same bits on a second call and over a NaN-filled output.
  model   against the CPU oracle's pixel gradient (pinned on the reference's by test_pixel_grad_oracle.py) and against the reference's
          pixel_values.grad itself (tests/golden/pixel_grad.npz): rel-rms < GRAD_RMS = 6e-2, the bound of tests/test_model_gpu.py for the stage-1
          patch-embedding weight gradient, which is contracted from the very same `de`; cosine > ACT_COS.
"""
import numpy as np
import pytest
import torch

import golden_util as gu
import pixel_grad_ref as pr
from bounds_util import BF, F32, Guarded, assert_f32_bound, bits
from test_gen_controls_gpu import longi_model, multi_model
from test_model_gpu import ACT_COS, GRAD_RMS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import modelling
    return modelling


@pytest.fixture(scope="module")
def G():
    return gu.load("gen_controls.npz")


# ------------------------------------------------------------------------------------------------ kernel
def _operands(Bn, H, W, Co, seed, zero_image=None):
    Ho, Wo = pr.out_hw(H, W)
    g = torch.Generator().manual_seed(seed)
    de = torch.randn(Bn * Ho * Wo, Co, generator=g)
    if zero_image is not None:
        de.view(Bn, Ho * Wo, Co)[zero_image] = 0.0
    w = torch.zeros(Co, 192)
    w[:, :147] = torch.randn(Co, 147, generator=g) * 0.1
    return de.to(BF).cuda(), w.to(BF).cuda()


def _check_kernel(Bn, H, W, Co=64, seed=0, zero_image=None):
    from cxrmate_amd import ops
    de, w = _operands(Bn, H, W, Co, seed, zero_image)
    ref, mag, n = pr.dgrad64(de, w, Bn, H, W)
    assert n.max() <= 4 * Co
    out = Guarded.flat(Bn * 3 * H * W, F32)                           # (the sentinel is a NaN: the first call writes over NaNs)
    dpx = out.view.view(Bn, 3, H, W)
    got = ops.patch_embed_dgrad(de, w, Bn, H, W, pr.KS, pr.STRIDE, pr.PAD, out=dpx)
    out.check(f"dgrad {(Bn, H, W, Co)}")
    first = bits(got)
    worst = assert_f32_bound(got, ref, pr.dgrad_bound(ref, mag, n).ravel(), 0.5, f"dgrad {(Bn, H, W, Co)}")
    print(f"dgrad {(Bn, H, W, Co)}: worst |err| {worst:.3e}, max |ref| {np.abs(ref).max():.3f}")
    ops.patch_embed_dgrad(de, w, Bn, H, W, pr.KS, pr.STRIDE, pr.PAD, out=dpx)      # over its own result: an accumulating kernel would double it
    out.check("second call")
    assert torch.equal(bits(dpx), first)
    fresh = ops.patch_embed_dgrad(de, w, Bn, H, W, pr.KS, pr.STRIDE, pr.PAD)       # allocated by the wrapper
    assert fresh.shape == (Bn, 3, H, W) and fresh.dtype == F32 and torch.equal(bits(fresh), first)
    return got, ref, n


@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 96, 96), (3, 64, 128), (2, 98, 102), (1, 8, 384)])
def test_kernel_against_fp64(M, shape):
    got, ref, n = _check_kernel(*shape, seed=sum(shape))
    Bn, H, W = shape
    if shape == (2, 98, 102):
        # Ho = 24, Wo = 25: pixel row 97 and pixel column 101 are covered by no output position
        assert n[:, :, 97, :].max() == 0 and n[:, :, :, 101].max() == 0 and n[:, :, :97, :101].min() > 0
        assert int(bits(got[:, :, 97, :]).abs().max()) == 0 and int(bits(got[:, :, :, 101]).abs().max()) == 0


def test_kernel_with_32_output_channels(M):
    _check_kernel(2, 98, 102, Co=32, seed=5)


def test_kernel_zero_rows_give_exact_zeros(M):
    got, ref, _ = _check_kernel(2, 96, 96, seed=6, zero_image=1)
    assert int(bits(got[1]).abs().max()) == 0 and float(got[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ model
def _state(m):
    return {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items()}


def _cmp(got, ref, what):
    got, ref = got.detach().float().cpu().numpy(), ref.detach().float().cpu().numpy()
    r, c = gu.rel_rms(got, ref), gu.cosine(got, ref)
    print(f"{what}: rel_rms {r:.4f} cos {c:.6f}")
    assert np.isfinite(got).all() and r < GRAD_RMS and c > ACT_COS, f"{what}: rel_rms {r:.4f} cos {c:.6f}"
    return r


def _fixture_model(M, drop_path=None):
    g, cfg, sd, x, inp, lab, am, tt = pr.fixture_case()
    if drop_path is not None:
        cfg.encoder.drop_path_rate = tuple(drop_path for _ in cfg.encoder.drop_path_rate)
    m = M.MultiCXREncoderDecoderModel(cfg, seed=None)
    m.load_state_dict(sd)
    return m, g, cfg, sd, x, inp, lab, am, tt


def _tf_loss(m, px, inp, lab, am, tt):
    out = m(pixel_values=px, decoder_input_ids=inp.cuda(), decoder_attention_mask=am.cuda(), decoder_token_type_ids=tt.cuda(), return_dict=True)
    return torch.nn.functional.cross_entropy(out.logits.permute(0, 2, 1), lab.cuda(), ignore_index=gu.PAD), out


def test_encoder_alone_matches_oracle(M, G):
    m, kw = multi_model(M, G, "beam")
    x = kw["pixel_values"].cpu()                                       # [3, 2, 3, 96, 96], study 1 with a zero-padded image
    px = x.cuda().requires_grad_(True)
    feats = m.encoder(px).last_hidden_state
    wt = torch.randn(feats.shape, generator=torch.Generator().manual_seed(3))
    (feats.float() * wt.cuda()).sum().backward()
    assert px.grad is not None and px.grad.shape == px.shape and px.grad.dtype == F32
    ref, _ = pr.oracle_encoder_pixel_grad(x, _state(m), m.config.encoder, wt)
    _cmp(px.grad, ref, "encoder pixel gradient")
    assert float(px.grad[1, 1].abs().sum()) > 0                        # the zero-padded image's tokens carry weight here: its gradient is not zero


def test_end_to_end_matches_reference_fixture(M):
    m, g, cfg, sd, x, inp, lab, am, tt = _fixture_model(M)
    px = x.cuda().requires_grad_(True)
    loss, _ = _tf_loss(m, px, inp, lab, am, tt)
    assert abs(loss.item() - float(g["loss"])) < 2e-2
    loss.backward()
    assert px.grad.shape == (2, 2, 3, 96, 96) and px.grad.dtype == F32
    got, ref = pr.at_index(px.grad, g), g["grad_values"]
    r, c = gu.rel_rms(got, ref), gu.cosine(got, ref)
    norms = pr.image_norms(px.grad)
    print(f"end to end: rel_rms {r:.4f} cos {c:.6f} image norms {norms.ravel()} reference {g['grad_image_norms'].ravel()}")
    assert r < GRAD_RMS and c > ACT_COS
    assert norms[1, 1] == 0.0                                           # eval mode, masked zero-padded image
    np.testing.assert_allclose(np.delete(norms.ravel(), 3), np.delete(g["grad_image_norms"].ravel(), 3), rtol=GRAD_RMS)
    # a GradScaler-scaled loss: the same gradient times the (power of two) scale
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 12)
    ps = x.cuda().requires_grad_(True)
    scaler.scale(_tf_loss(m, ps, inp, lab, am, tt)[0]).backward()
    assert gu.rel_rms((ps.grad / 2.0 ** 12).cpu().numpy(), px.grad.cpu().numpy()) < 1e-3
    # a bf16 input gets a bf16 gradient of its own shape
    p16 = x.to(BF).cuda().requires_grad_(True)
    _tf_loss(m, p16, inp, lab, am, tt)[0].backward()
    assert p16.grad.dtype == BF and p16.grad.shape == (2, 2, 3, 96, 96)
    oracle16, _ = pr.oracle_tf_pixel_grad(x.to(BF).float(), sd, cfg, inp, lab, am, tt, gu.PAD)
    assert gu.rel_rms(p16.grad.float().cpu().numpy(), oracle16.numpy()) < GRAD_RMS


def test_train_mode_batch_statistics_couple_the_images(M):
    m, g, cfg, sd, x, inp, lab, am, tt = _fixture_model(M, drop_path=0.0)      # DropPath off; BatchNorm on batch statistics
    m.train()
    state = _state(m)
    px = x.cuda().requires_grad_(True)                                 # image (1, 1) = image 3 of the 4-image launch is all zeros
    feats = m.encoder(px).last_hidden_state                            # [2, 2 * tokens, C]
    tokens = feats.shape[1] // 2
    wt = torch.randn(feats.shape, generator=torch.Generator().manual_seed(4))
    wt[1, tokens:] = 0.0                                               # no weight on image 3's tokens
    (feats.float() * wt.cuda()).sum().backward()
    ref, _ = pr.oracle_encoder_pixel_grad(x, state, cfg.encoder, wt, bn_train=True)
    rms = lambda t: float(t.detach().float().pow(2).mean().sqrt())
    print(f"train mode: rms of image 3's gradient {rms(px.grad[1, 1]):.4f} (oracle {rms(ref[1, 1]):.4f}), others {rms(px.grad[0]):.4f} (oracle {rms(ref[0]):.4f})")
    assert rms(ref[1, 1]) > 0.05 * rms(ref[0])                         # BatchNorm couples the batch: the "masked" image still has a gradient
    _cmp(px.grad, ref, "train-mode pixel gradient")
    _cmp(px.grad[1, 1], ref[1, 1], "train-mode pixel gradient of the zero image")
    # the same pass with the encoder frozen (dX chain only, BatchNorm by-products to scratch): the same bits, and no encoder gradient moves
    enc = _enc_params(m, False)
    held = [None if p.grad is None else p.grad.clone() for p in enc]
    p2 = x.cuda().requires_grad_(True)
    (m.encoder(p2).last_hidden_state.float() * wt.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(bits(p2.grad), bits(px.grad))
    assert all((h is None and p.grad is None) or torch.equal(h, p.grad) for h, p in zip(held, enc))
    m.eval()


def _enc_params(m, on):
    ps = [p for n, p in m.named_parameters() if n.startswith("encoder.")]
    for p in ps:
        p.requires_grad_(on)
    return ps


def _clear_grads(m):
    for p in m.parameters():
        p.grad = None


def test_frozen_encoder_runs_the_dx_chain_only(M, G, monkeypatch):
    from cxrmate_amd import ops
    m, kw = longi_model(M, G)
    x = torch.randn(2, 2, 3, 96, 96, generator=torch.Generator().manual_seed(int(G["longi_pixel_seed"])))
    x[0, 1] = 0.0
    ids = kw["decoder_input_ids"]
    lab = torch.randint(12, int(G["longi_vocab"]), ids.shape, generator=torch.Generator().manual_seed(9)).cuda()
    tt = m.token_ids_to_token_type_ids(ids, [gu.PMT_SEP, gu.BOS, gu.SEP], [0, 1, 0, 1])
    lora = [(n, p) for n, p in m.named_parameters() if n.startswith("decoder.") and p.requires_grad]
    assert lora

    def run(px):
        _clear_grads(m)
        out = m(pixel_values=px, decoder_input_ids=ids, decoder_token_type_ids=tt, return_dict=True)
        torch.nn.functional.cross_entropy(out.logits.permute(0, 2, 1), lab).backward()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in lora}

    enc = _enc_params(m, False)
    base = run(x.cuda())                                               # no pixel gradient asked for: the encoder is outside autograd
    lo = min(m._offsets[k] for k in m._offsets if k.startswith("encoder.") and m._offsets[k] < m._param_total)
    hi = max(m._offsets[k] + m._numel(k) for k in m._offsets if k.startswith("encoder.") and m._offsets[k] < m._param_total)
    m.gflat[lo:hi].fill_(1.25)                                         # whatever the range holds must still be there afterwards
    before = m.gflat[lo:hi].clone()
    px = x.cuda().requires_grad_(True)
    frozen = run(px)
    g_frozen = px.grad.clone()
    assert bool(torch.isfinite(g_frozen).all()) and float(g_frozen.abs().sum()) > 0
    assert all(p.grad is None for p in enc)
    assert torch.equal(m.gflat[lo:hi], before)
    for n in base:
        assert torch.equal(bits(frozen[n]), bits(base[n])), n          # the LoRA gradients do not depend on the pixels' request
    # the encoder backward alone launches no weight-gradient GEMM
    calls = []
    real_lbw, real_tn = ops.linear_bwd_weight, ops.gemm_tn
    monkeypatch.setattr(ops, "linear_bwd_weight", lambda *a, **k: (calls.append("linear_bwd_weight"), real_lbw(*a, **k))[1])
    monkeypatch.setattr(ops, "gemm_tn", lambda *a, **k: (calls.append("gemm_tn"), real_tn(*a, **k))[1])
    p2 = x.cuda().requires_grad_(True)
    feats = m.encoder(p2).last_hidden_state
    wt = torch.randn(feats.shape, generator=torch.Generator().manual_seed(8)).cuda()
    (feats.float() * wt).sum().backward()
    torch.cuda.synchronize()
    assert calls == [] and torch.equal(m.gflat[lo:hi], before) and all(p.grad is None for p in enc)
    g2_frozen = p2.grad.clone()
    monkeypatch.undo()
    # unfrozen: the same pixel gradient, bit for bit
    _enc_params(m, True)
    p3 = x.cuda().requires_grad_(True)
    (m.encoder(p3).last_hidden_state.float() * wt).sum().backward()
    assert torch.equal(bits(p3.grad), bits(g2_frozen))
    assert all(p.grad is not None for p in enc)
    p4 = x.cuda().requires_grad_(True)
    run(p4)
    assert torch.equal(bits(p4.grad), bits(g_frozen))


TIED = "decoder.bert.embeddings.word_embeddings.weight"


def test_unused_means_unchanged(M, monkeypatch):
    from cxrmate_amd._lib import LIB
    m, g, cfg, sd, x, inp, lab, am, tt = _fixture_model(M)
    names = []
    real = LIB.call

    def recording(name, *a):
        names.append(name)
        return real(name, *a)

    def run(want):
        _clear_grads(m)
        px = x.cuda().requires_grad_(want)
        del names[:]
        loss, out = _tf_loss(m, px, inp, lab, am, tt)
        loss.backward()
        torch.cuda.synchronize()
        logits = out.logits.detach().float().cpu()
        return list(names), logits, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}, px.grad

    run(False)                                                         # warm-up: weight re-layouts and scratch buffers of a first pass exist
    monkeypatch.setattr(LIB, "call", recording)
    n0, l0, g0, pg0 = run(False)
    n1, l1, g1, pg1 = run(True)
    assert pg0 is None and pg1 is not None
    assert torch.equal(l0, l1)
    assert sorted(g0) == sorted(g1) and len(g0) > 100
    for n in g0:
        if n == TIED:
            continue
        assert torch.equal(bits(g0[n]), bits(g1[n])), n
    # The tied word-embedding / LM-head weight is the one gradient that is not reproducible between two IDENTICAL plain passes: three addends per
    # element (the LM head's weight-gradient GEMM on the weight-gradient stream, the embedding scatter's float atomics on the main stream) meet in
    # an order the two streams decide. Measured before this feature existed in the pass: 4 plain passes gave 3 different bit patterns of it and
    # equal bits for every other gradient; passes with and without a pixel gradient gave equal bits of it as often as two plain ones. No code
    # of the pixel gradient touches it, and bit equality is undefined for it: it is held to the reordering of fp32 additions instead.
    assert gu.rel_rms(g1[TIED].cpu().numpy(), g0[TIED].cpu().numpy()) < 1e-5
    extra = list(n1)
    for n in n0:
        extra.remove(n)                                                # (raises if a launch of the plain run is missing)
    assert extra == ["cxr_patch_embed_dgrad_f32"], extra
    assert "cxr_patch_embed_dgrad_f32" not in n0
    with torch.no_grad():                                              # no_grad: the forward-only path, whatever the pixels ask for
        del names[:]
        a = m(pixel_values=x.cuda().requires_grad_(True), decoder_input_ids=inp.cuda(), decoder_attention_mask=am.cuda(),
              decoder_token_type_ids=tt.cuda()).logits.float().cpu()
        na = list(names)
        del names[:]
        b = m(pixel_values=x.cuda(), decoder_input_ids=inp.cuda(), decoder_attention_mask=am.cuda(), decoder_token_type_ids=tt.cuda()).logits.float().cpu()
        assert na == list(names) and torch.equal(a, b)


def test_in_place_edit_of_the_pixels_is_caught(M):
    m, g, cfg, sd, x, inp, lab, am, tt = _fixture_model(M)
    px = x.cuda().requires_grad_(True)
    feats = m.encoder(px).last_hidden_state
    with torch.no_grad():
        px.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        feats.float().sum().backward()
    m._settle_owed_join()


def test_scores_of_generate_reach_the_pixels(M, G):
    m, kw = multi_model(M, G, "beam")
    px = kw.pop("pixel_values").clone().requires_grad_(True)
    eo = m.encoder(px)
    torch.manual_seed(5)
    out = m.generate.__wrapped__(m, encoder_outputs=eo, **kw, do_sample=True, output_scores=True, return_dict_in_generate=True, top_k=20,
                                 max_new_tokens=6, num_beams=1)
    sc = torch.stack(out["scores"], dim=-1)                            # [rows, V, steps]; top-k leaves -inf outside the kept entries
    sc.float().logsumexp(1).sum().backward()
    assert px.grad is not None and px.grad.shape == px.shape
    assert bool(torch.isfinite(px.grad).all()) and float(px.grad.abs().sum()) > 0
