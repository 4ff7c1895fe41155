"""References of the pixel-gradient tests: the data gradient of the stage-1 patch-embedding convolution in float64, and the CPU oracle's
gradient with respect to its pixels."""
import numpy as np
import torch
import torch.nn.functional as F

KS, STRIDE, PAD = 7, 4, 2


def out_hw(H, W, ks=KS, stride=STRIDE, pad=PAD):
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def _conv_input_grad(de_nchw, w4, H, W, stride, pad):
    x = torch.zeros((de_nchw.shape[0], w4.shape[1], H, W), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w4, stride=stride, padding=pad)
    (g,) = torch.autograd.grad(y, x, grad_outputs=de_nchw)
    return g


def dgrad64(de, w, Bn, H, W, ks=KS, stride=STRIDE, pad=PAD):
    """de [Bn*Ho*Wo, Co] bf16, w [Co, kpad] bf16 (K order (c, ky, kx), zero padded) -> float64 numpy arrays [Bn, 3, H, W]:
      ref  the autograd of F.conv2d in float64 on exactly these (bf16-rounded) operands
      mag  the same sum over |de| * |w|: the magnitude the rounding errors of an fp32 accumulation scale with
      n    the number of products of each pixel (<= ceil(ks / stride)^2 * Co)"""
    Ho, Wo = out_hw(H, W, ks, stride, pad)
    Co = w.shape[0]
    d = de.detach().double().cpu().view(Bn, Ho, Wo, Co).permute(0, 3, 1, 2).contiguous()
    w4 = w.detach().double().cpu()[:, :3 * ks * ks].reshape(Co, 3, ks, ks)
    ref = _conv_input_grad(d, w4, H, W, stride, pad)
    mag = _conv_input_grad(d.abs(), w4.abs(), H, W, stride, pad)
    n = _conv_input_grad(torch.ones_like(d), torch.ones_like(w4), H, W, stride, pad)
    return ref.numpy(), mag.numpy(), n.numpy()


def dgrad_bound(ref, mag, n):
    """|got - ref| <= (n + 1) * 2^-24 * sum |de * w| + 1/2 ulp32(ref): products of two bf16 values are exact in fp32, every one of the n - 1 additions
    of an fp32 accumulation (in any order) rounds by at most 2^-24 of a partial sum that is bounded by sum |de * w|; the last term is the rounding of
    the exact sum to the fp32 result. -> the absolute part (the half ulp is the `ulps` argument of bounds_util.assert_f32_bound)."""
    return (n + 1.0) * 2.0 ** -24 * mag


def oracle_encoder_pixel_grad(x, sd, cfg_encoder, weight, bn_train=False):
    """d sum(feats * weight) / d pixels through oracle.cvt.encoder_forward (fp32, CPU). x [B, N, 3, H, W] or [B, 3, H, W]; weight like feats."""
    from oracle import cvt as ocvt
    x = x.detach().clone().float().requires_grad_(True)
    sd = {k: v.detach().clone() for k, v in sd.items()}
    h = ocvt.encoder_forward(x, sd, cfg_encoder, bn_train=bn_train)[0]
    (h * weight).sum().backward()
    return x.grad.detach(), h.detach()


def oracle_tf_pixel_grad(x, sd, cfg, inp, lab, am, tt, pad_id):
    """pixel gradient of the teacher-forced cross-entropy through the oracle's encoder and decoder (eval mode) -> (grad, loss)"""
    from oracle import bert as obert, cvt as ocvt, generate as ogen
    x = x.detach().clone().float().requires_grad_(True)
    h, emask = ocvt.encoder_forward(x, sd, cfg.encoder)
    logits = obert.decoder_forward(inp, sd, cfg.decoder, h, emask, am, tt, None)
    loss = ogen.tf_cross_entropy(logits, lab, pad_id)
    loss.backward()
    return x.grad.detach(), float(loss.item())


def fixture_case():
    """tests/golden/pixel_grad.npz (make_golden_pixel_grad.py) -> g, cfg, sd, x, inp, lab, am, tt"""
    import golden_util as gu
    from cxrmate_amd import weights
    from cxrmate_amd.config import tiny_config
    g = gu.load("pixel_grad.npz")
    cfg = tiny_config(vocab_size=1000, decoder_layers=2, depth=tuple(int(i) for i in g["depth"]), image_size=96)
    sd = weights.init_encoder_decoder(cfg, seed=int(g["seed"]), perturb=float(g["perturb"]))
    x = torch.randn(2, 2, 3, 96, 96, generator=torch.Generator().manual_seed(int(g["pixel_seed"])))
    x[1, 1] = 0.0
    full = torch.from_numpy(g["full_ids"])
    attn = (full != gu.PAD).long()
    return g, cfg, sd, x, full[:, :-1], full[:, 1:].clone(), attn[:, 1:], torch.from_numpy(g["token_type_ids"])


def image_norms(grad):
    return grad.detach().double().cpu().flatten(2).norm(dim=2).numpy()


def at_index(grad, g):
    return grad.detach().float().cpu().reshape(-1)[torch.from_numpy(g["grad_index"])].numpy()
