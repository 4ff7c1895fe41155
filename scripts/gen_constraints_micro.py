"""Cost of the token constraints on the decode hot path: cached decode per token-step with no option set and with ONE bad word (csrc/logits_proc.hip
logits_constrain_kernel, one launch per greedy step; log_softmax + the kernel in front of the log-prob beam step, two launches per beam step), and
of early_stopping=True (cxr_beam_step_es in place of cxr_beam_step).

    python scripts/gen_constraints_micro.py [--reps 5]

Workloads (EOS disabled, every step runs): BASELINE.json configs[2] beam-4, 8 studies x 2 images, 256 tokens; greedy over 32 rows (32 studies x
2 images), 256 tokens. The encoder runs once outside the timed region (encoder_outputs are passed in). On and off runs alternate in one process
after warm-up (graph capture); device events time each run. Prints one JSON line per workload and option set."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPTION_SETS = {"one bad word": dict(bad_words_ids=[[1017, 2040]]), "early_stopping=True": dict(early_stopping=True)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(name, model, kw, opts, steps, reps):
    on = lambda: model.generate(**kw, **opts)          # noqa: E731
    off = lambda: model.generate(**kw)                 # noqa: E731
    for f in (on, off, on, off):                       # captures the step graphs of both modes
        f()
    t_on, t_off = [], []
    for _ in range(reps):
        t_off.append(timed(off))
        t_on.append(timed(on))
    m_on, m_off = statistics.median(t_on), statistics.median(t_off)
    return {"workload": name, "steps": steps, "us_per_step_off": m_off * 1e3 / steps, "us_per_step_on": m_on * 1e3 / steps,
            "delta_us_per_step": (m_on - m_off) * 1e3 / steps, "delta_pct": 100.0 * (m_on - m_off) / m_off,
            "ms_off": t_off, "ms_on": t_on, "options": {k: str(v) for k, v in opts.items()}}


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
    for name, B, nb in (("configs[2] beam-4, 8 studies x 2 images", 8, 4), ("greedy, 32 rows (32 studies x 2 images)", 32, 1)):
        images = torch.randn(B, 2, 3, 384, 384, generator=g).to(dev)
        with torch.no_grad():
            eo = model.encoder(images)
        kw = dict(encoder_outputs=eo, special_token_ids=[3], max_length=L, bos_token_id=1, eos_token_id=None, pad_token_id=4, num_beams=nb)
        for label, opts in OPTION_SETS.items():
            if nb == 1 and "early_stopping" in opts:
                continue
            print(json.dumps(measure(f"{name}; {label}", model, kw, opts, L - 1, args.reps)), flush=True)


if __name__ == "__main__":
    main()
