"""Micro-benchmark of output_attentions: the attention-probability kernel (ops.attention_probs, csrc/attn_probs.hip) at the decoder shapes of
the C3 forward (8 studies x 2 images, T = 256, S = 1152, 12 heads) and the whole C3 forward (eval, no_grad) with and without
output_attentions / output_hidden_states.

The kernel is bound by its fp32 output: B*H*Tq*Tk*4 bytes, 25.2 MB per self-attention layer and 113 MB per cross-attention layer, 0.83 GB
over the 6 layers; at 6.29 TB/s of achievable HBM bandwidth that is a floor of ~0.13 ms per forward. The script reports the achieved write
bandwidth of each call against that rate (device events around `--reps` back-to-back calls, after warm-up).

    python scripts/attn_probs_micro.py [--reps 50] [--fwd-reps 10] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cxrmate_amd import ops  # noqa: E402

HBM_TBS = 6.29          # achievable HBM bandwidth, TB/s (MI355X_MICROARCH.md)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps            # ms per call


def kernel_rows(reps):
    B, H, T, S, D = 8, 12, 256, 1152, 768
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn((B, T, 3 * D), generator=g, device="cuda").to(torch.bfloat16)
    q, k, v = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    am = torch.ones((B, T), dtype=torch.uint8, device="cuda")
    am[:, 200:] = 0
    q2 = torch.randn((B, T, D), generator=g, device="cuda").to(torch.bfloat16)
    kv = torch.randn((B, S, 12 * D), generator=g, device="cuda").to(torch.bfloat16)          # all-layer K / V buffer: row stride 2 L D
    k2, v2 = kv[:, :, :D], kv[:, :, D:2 * D]
    em = torch.ones((B, S), dtype=torch.uint8, device="cuda")
    em[1, 576:] = 0
    scale = 64 ** -0.5
    _, lse = ops.attention(q, k, v, H, scale, kpm=am, causal=True, need_lse=True)
    _, lse2 = ops.attention(q2, k2, v2, H, scale, kpm=em, need_lse=True)
    p = torch.empty((B, H, T, T), device="cuda")
    p2 = torch.empty((B, H, T, S), device="cuda")
    rows = []
    for name, fn, nbytes in (("self  [8,12,256,256]", lambda: ops.attention_probs(q, k, lse, H, scale, kpm=am, causal=True, out=p), p.numel() * 4),
                             ("cross [8,12,256,1152]", lambda: ops.attention_probs(q2, k2, lse2, H, scale, kpm=em, out=p2), p2.numel() * 4)):
        ms = timed(fn, reps)
        rows.append(dict(call=name, ms=ms, MB=nbytes / 1e6, TBs=nbytes / ms / 1e9, floor_ms=nbytes / (HBM_TBS * 1e9)))
    return rows


def forward_rows(reps):
    from cxrmate_amd import modelling
    from cxrmate_amd.config import EncoderDecoderConfig
    cfg = EncoderDecoderConfig()
    m = modelling.MultiCXREncoderDecoderModel(cfg, device="cuda", seed=0)
    B, N, T = 8, 2, 256
    g = torch.Generator().manual_seed(1)
    px = torch.randn(B, N, 3, cfg.encoder.image_size, cfg.encoder.image_size, generator=g).cuda()
    ids = torch.randint(12, cfg.decoder.vocab_size, (B, T), generator=g).cuda()
    am = torch.ones_like(ids)
    out = {}
    with torch.no_grad():
        for flags in (False, True, False, True):                # alternated; the second of each pair is reported
            out[flags] = timed(lambda: m(pixel_values=px, decoder_input_ids=ids, decoder_attention_mask=am, output_attentions=flags,
                                         output_hidden_states=flags), reps)
    return dict(forward_ms=out[False], forward_with_maps_ms=out[True], delta_ms=out[True] - out[False])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--fwd-reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU (no number is measured without it)"
    rows = kernel_rows(a.reps)
    for r in rows:
        print(f"{r['call']}: {r['ms'] * 1e3:8.1f} us  {r['MB']:7.1f} MB written  {r['TBs']:5.2f} TB/s  ({r['TBs'] / HBM_TBS:.0%} of {HBM_TBS} TB/s; "
              f"floor {r['floor_ms'] * 1e3:.1f} us)")
    per_fwd = 6 * sum(r["ms"] for r in rows)
    print(f"6 layers (self + cross): {per_fwd:.3f} ms of kernel time against a write floor of "
          f"{6 * sum(r['floor_ms'] for r in rows):.3f} ms")
    fw = forward_rows(a.fwd_reps)
    print(f"C3 forward (eval, no_grad): {fw['forward_ms']:.2f} ms; with output_attentions + output_hidden_states {fw['forward_with_maps_ms']:.2f} ms "
          f"(+{fw['delta_ms']:.2f} ms)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(kernel=rows, six_layers_ms=per_fwd, **fw), f, indent=1)


if __name__ == "__main__":
    main()
