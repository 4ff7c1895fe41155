"""Cost of the device image transforms (cxrmate_amd.pixels.StudyImageTransform) for one training batch, beside Pillow on one host thread.

    python scripts/image_transform_micro.py [--studies 32] [--per-study 2] [--height 3056] [--width 2544] [--reps 5] [--train] [--no-cpu]

Workload: `--studies` x `--per-study` grey images of `--height` x `--width` (the MIMIC-CXR size), built from tests/image_transform_ref.py
`source()`; size 384, test-mode transforms unless --train (fixed crops and angles then). One warm-up call, then `--reps` repetitions, medians:
  entry_ms      the entry point alone (cxr_image_transform: both launches), device events around a call whose inputs are on the device already
  transform_ms  `transform` end to end: host packing into the pinned buffer, the copy, the launches; host clock, ends in a device synchronise
  pillow_ms     the reference's Pillow calls for the same batch on one thread (resize BILINEAR, crop, [rotate NEAREST]) + ToTensor/Normalize in numpy
Bytes: source = sum H * pitch; intermediate = sum H * ow (written once, read once by the vertical pass where the crop needs it); output = B * N *
3 * S * S * 4. `hbm_gbs` = (source + 2 * intermediate + output) / entry time. The two kernels' own times (and with them the horizontal pass's bytes per
second, (source + intermediate) / its time) come from `rocprofv3 --kernel-trace --stats -- python scripts/image_transform_micro.py --no-cpu`,
a run of its own: the kernels are image_resize_h_kernel and image_finish_kernel. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--studies", type=int, default=32)
    ap.add_argument("--per-study", type=int, default=2)
    ap.add_argument("--height", type=int, default=3056)
    ap.add_argument("--width", type=int, default=2544)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import image_transform_ref as ref
    from cxrmate_amd import ops, pixels
    if not torch.cuda.is_available():
        raise SystemExit("image_transform_micro needs a GPU: there is nothing to measure without one")
    S, n = args.size, args.studies * args.per_study
    base = ref.source(args.height, args.width, 1, 0)
    images = [np.ascontiguousarray(np.roll(base, 37 * i, axis=1)) for i in range(n)]          # distinct contents, one size
    studies = [images[b * args.per_study:(b + 1) * args.per_study] for b in range(args.studies)]
    t = pixels.StudyImageTransform(S, train=args.train)
    oh, ow = pixels.resized_hw(args.height, args.width, S)
    kw = {}
    if args.train:
        kw = dict(crops=[((oh - S) * (i % 3) // 2, (ow - S) * (i % 3) // 2) for i in range(n)], angles=[(i % 11) - 5.0 for i in range(n)])
    plan = t.plan([(args.height, args.width, 1)] * n, counts=[args.per_study] * args.studies, **kw)

    # ---- the entry point alone
    host = torch.empty((plan.src_bytes,), dtype=torch.uint8)
    for img, off, pitch in zip(images, plan.offsets, plan.pitches):
        host[off:off + args.height * pitch].view(args.height, pitch)[:, :args.width].copy_(torch.from_numpy(img))
    src = host.cuda()
    meta = torch.from_numpy(np.concatenate([plan.desc, plan.tables])).cuda()
    desc, tables = meta[:plan.desc.size], meta[plan.desc.size:]
    entry = []
    for rep in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, _ = ops.image_transform(src, desc, tables, n, plan.n_bands, plan.B, plan.Nmax, S, t.mean, t.std, plan.inter_bytes)
        e1.record()
        e1.synchronize()
        if rep:
            entry.append(e0.elapsed_time(e1))
    # ---- end to end
    total = []
    for rep in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out2 = t.transform(studies, "cuda", **kw)
        torch.cuda.synchronize()
        if rep:
            total.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(out, out2)
    entry_ms, total_ms = statistics.median(entry), statistics.median(total)
    src_bytes, inter_bytes, out_bytes = plan.src_bytes, plan.inter_bytes, out.numel() * 4
    line = {"images": n, "source_hw": [args.height, args.width], "size": S, "train": args.train, "reps": args.reps, "n_bands": plan.n_bands,
            "source_bytes": src_bytes, "intermediate_bytes": inter_bytes, "output_bytes": out_bytes,
            "entry_ms": entry_ms, "entry_ms_all": entry, "transform_ms": total_ms, "transform_ms_all": total,
            "hbm_gbs": (src_bytes + 2 * inter_bytes + out_bytes) / entry_ms / 1e6,
            "copy_overlapped": False}
    if not args.no_cpu:
        from PIL import Image
        torch.set_num_threads(1)
        mean, std = np.asarray(t.mean, np.float32).reshape(3, 1, 1), np.asarray(t.std, np.float32).reshape(3, 1, 1)
        t0 = time.perf_counter()
        outs = []
        for i, img in enumerate(images):
            im = Image.fromarray(img).convert("RGB")                                         # the reference's Image.open(...).convert('RGB')
            im = im.resize((ow, oh), Image.BILINEAR)
            top, left = kw["crops"][i] if args.train else pixels.center_crop_offsets(oh, ow, S)
            im = im.crop((left, top, left + S, top + S))
            if args.train:
                im = im.rotate(kw["angles"][i], Image.NEAREST, expand=False, center=None, fillcolor=0)
            outs.append((np.asarray(im).transpose(2, 0, 1).astype(np.float32) / 255.0 - mean) / std)
        line["pillow_ms"] = (time.perf_counter() - t0) * 1e3
        import PIL
        line["pillow"] = PIL.__version__
        got = out.view(n, 3, S, S).cpu().numpy()
        line["max_abs_diff_vs_pillow"] = float(np.abs(got - np.stack(outs)).max())
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
