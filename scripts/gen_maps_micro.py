"""Cost of the attention maps / hidden states of generate(): cached decode per token-step without the flags, with output_attentions, with
output_hidden_states and with both (return_dict_in_generate=True every time). On: per layer two csrc/attn_decode_probs.hip launches (self and
cross maps; where the query projection runs inside the cross-attention kernel one extra dec_gemm for the record's q2) resp. one hidden-state
launch per layer + 1, and one copy of the recorded slots at the end of the call.

    python scripts/gen_maps_micro.py [--reps 5]

Workloads (EOS disabled, every step runs): the decode shape of BASELINE.json configs[3], 16 rows x 2 images, 256 tokens, greedy; beam-4 over
8 studies x 2 images (32 beam rows), 256 tokens. The encoder runs once outside the timed region (encoder_outputs are passed in). The four modes
alternate in one process after warm-up (graph capture); device events time each run. Prints one JSON line per workload."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {"off": {}, "attentions": dict(output_attentions=True), "hidden_states": dict(output_hidden_states=True),
         "both": dict(output_attentions=True, output_hidden_states=True)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(name, model, kw, steps, reps):
    runs = {mode: (lambda o=opts: model.generate(**kw, **o)) for mode, opts in MODES.items()}      # outputs are dropped after each run
    for _ in range(2):                                 # captures the step graphs of every mode
        for f in runs.values():
            f()
    ms = {mode: [] for mode in runs}
    for _ in range(reps):
        for mode, f in runs.items():
            ms[mode].append(timed(f))
    med = {mode: statistics.median(v) for mode, v in ms.items()}
    out = {"workload": name, "steps": steps, "ms": ms}
    for mode in runs:
        out[f"us_per_step_{mode}"] = med[mode] * 1e3 / steps
        if mode != "off":
            out[f"delta_us_per_step_{mode}"] = (med[mode] - med["off"]) * 1e3 / steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from cxrmate_amd.config import EncoderDecoderConfig
    from cxrmate_amd.modelling import MultiCXREncoderDecoderModel
    dev = torch.device("cuda:0")
    model = MultiCXREncoderDecoderModel(EncoderDecoderConfig(), device=dev, seed=0)
    model.eval()
    L = 256
    g = torch.Generator().manual_seed(3000)
    for name, B, nb in (("configs[3] decode shape: greedy, 16 rows x 2 images", 16, 1), ("beam-4, 8 studies x 2 images (32 beam rows)", 8, 4)):
        images = torch.randn(B, 2, 3, 384, 384, generator=g).to(dev)
        with torch.no_grad():
            eo = model.encoder(images)
        kw = dict(encoder_outputs=eo, special_token_ids=[3], max_length=L, bos_token_id=1, eos_token_id=None, pad_token_id=4, num_beams=nb,
                  return_dict_in_generate=True)
        print(json.dumps(measure(name, model, kw, L - 1, args.reps)), flush=True)
        model.__dict__.pop("_decode_sessions", None)   # the next workload's slots are allocated afresh (GBs at these shapes)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
