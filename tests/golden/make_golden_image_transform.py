#!/usr/bin/env python
"""Generate tests/golden/image_transform.npz: what Pillow returns for the reference's image transforms
(modules/lightning_modules/single.py:229-262), called the way torchvision's PIL backend calls it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_transform.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_transform.py --verify   # rebuild in memory, require identical arrays

Pillow is the only library that touches the pixels here:
    Resize(S)           img.resize((ow, oh), Image.BILINEAR) unless the image has that size already; (oh, ow) by torchvision's rule (short edge
                        S, long edge int(S * long / short))
    CenterCrop(S)       img.crop((left, top, left + S, top + S)), top = int(round((oh - S) / 2.0)), left likewise
    RandomCrop(S)       img.crop(...) at the recorded (top, left)
    RandomRotation(d)   img.rotate(angle, Image.NEAREST, expand=False, center=None, fillcolor=0) at the recorded angle
The sources are NOT stored: tests/image_transform_ref.py `source()` builds them from a closed integer formula. The case list (shapes, modes,
crops, angles) also lives there (`cases()`); this file records the expected uint8 outputs -- one channel for a grey source, whose three output
channels are equal -- and, as metadata, the parameters of every image and the Pillow version.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
FILE = os.path.join(HERE, "image_transform.npz")


def pillow_transform(src, p):
    from PIL import Image
    import image_transform_ref as ref
    img = Image.fromarray(src)                                                       # mode L or RGB
    H, W, S = p["H"], p["W"], p["S"]
    oh, ow = ref.resized_hw(H, W, S)
    if (ow, oh) != img.size:
        img = img.resize((ow, oh), Image.BILINEAR)
    if p["train"]:
        top, left = p["crop"]
    else:
        top, left = int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0))
    img = img.crop((left, top, left + S, top + S))
    if p["train"]:
        img = img.rotate(p["angle"], Image.NEAREST, expand=False, center=None, fillcolor=0)
    return np.asarray(img)


def build():
    import PIL
    import image_transform_ref as ref
    arrays, params = {}, {}
    for name, case in ref.cases().items():
        outs = [pillow_transform(s, p) for s, p in zip(ref.case_sources(case), case["images"])]
        if all(o.ndim == 2 for o in outs):
            arrays["out_" + name] = np.stack(outs)                                   # grey: [n, S, S]
        else:
            arrays["out_" + name] = np.stack([o if o.ndim == 3 else np.repeat(o[:, :, None], 3, axis=2) for o in outs])
        params[name] = dict(counts=case["counts"], images=case["images"])
    meta = dict(pillow=PIL.__version__, cases=params)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def main():
    arrays = build()
    if "--verify" in sys.argv:
        with np.load(FILE) as z:
            assert sorted(z.files) == sorted(arrays), (sorted(z.files), sorted(arrays))
            for k in arrays:
                assert np.array_equal(z[k], arrays[k]), k
        print("identical")
        return
    np.savez_compressed(FILE, **arrays)
    print(FILE, os.path.getsize(FILE), "bytes")


if __name__ == "__main__":
    main()
