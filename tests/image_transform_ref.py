"""numpy restatement of the reference's image transforms (modules/lightning_modules/single.py:229-262) as Pillow executes them through
torchvision's PIL backend: Resize (antialiased bilinear, two 8-bit passes with 22-bit integer weights), CenterCrop / RandomCrop, RandomRotation
(nearest neighbour, 16.16 fixed point), ToTensor + Normalize and the pad_sequence of collate_fn. Everything up to the normalise is integer
arithmetic on values derived in IEEE double in a fixed operation order, so the restatement equals Pillow byte for byte
(tests/test_image_transform_abi.py checks that against the recorded fixture and against the installed Pillow).

The tables are built here with scalar Python loops on purpose: cxrmate_amd/pixels.py builds the same tables vectorised, and the tests compare the
two.

`source(H, W, C, case_id)` builds the test images from a closed integer formula (no RNG, no floats): identical on every machine, so the fixture
holds expected outputs only."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "image_transform.npz")
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 22


# ------------------------------------------------------------------------------------------------ test images
def source(H, W, C, case_id=0):
    """uint8 [H, W] (C == 1) or [H, W, 3]: fine texture (7x + 13y), coarse texture ((x*y) >> 6), a 16-pixel XOR pattern and a channel / case offset"""
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    chans = [((7 * x + 13 * y + ((x * y) >> 6) + 5 * ((x ^ y) & 15) + 31 * c + 17 * case_id) & 255).astype(np.uint8) for c in range(C)]
    return chans[0] if C == 1 else np.stack(chans, axis=-1)


# ------------------------------------------------------------------------------------------------ sizes and crops
def resized_hw(H, W, S):
    """torchvision Resize(int): the short edge becomes S, the long edge int(S * long / short); an image of that size already is left alone"""
    short, long_ = (W, H) if W <= H else (H, W)
    new_short, new_long = S, int(S * long_ / short)
    return (new_long, new_short) if W <= H else (new_short, new_long)               # (oh, ow)


def center_crop_offsets(oh, ow, S):
    return int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0))                      # Python's round: half to even


# ------------------------------------------------------------------------------------------------ resample tables
def coefficients(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter -> (ksize, xmin [out], n [out], k [out][ksize] int)"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmins, ns, ks = [], [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)                                            # C cast: truncation toward zero
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        n = xmax - xmin
        w = []
        ww = 0.0
        for x in range(n):
            t = ((x + xmin) - center + 0.5) * ss
            v = max(0.0, 1.0 - abs(t))
            w.append(v)
            ww += v                                                                   # tap order
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * 4194304.0 + 0.5) for v in w] + [0] * (ksize - n)
        xmins.append(xmin), ns.append(n), ks.append(k)
    return ksize, np.array(xmins, np.int64), np.array(ns, np.int64), np.array(ks, np.int64).reshape(out_size, ksize)


def resample_axis0(img, out_size):
    """one 8-bit pass along axis 0 of img [in, ...] -> uint8 [out, ...]"""
    in_size = img.shape[0]
    ksize, xmin, n, k = coefficients(in_size, out_size)
    acc = np.full((out_size,) + img.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    src = img.astype(np.int64)
    extra = (1,) * (img.ndim - 1)
    for t in range(ksize):
        idx = np.minimum(xmin + t, in_size - 1)                                       # taps beyond n carry weight 0
        acc += src[idx] * k[:, t].reshape((out_size,) + extra)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, S):
    """Resize(S): horizontal pass, then vertical pass; a pass whose sizes are equal is skipped"""
    H, W = img.shape[:2]
    oh, ow = resized_hw(H, W, S)
    if ow != W:
        img = np.swapaxes(resample_axis0(np.swapaxes(img, 0, 1), ow), 0, 1)
    if oh != H:
        img = resample_axis0(img, oh)
    return np.ascontiguousarray(img)


# ------------------------------------------------------------------------------------------------ rotation
def rotation_integers(angle, S):
    """Image.rotate(angle, NEAREST, expand=False, center=None) on an S x S image -> the six 16.16 integers a0..a5 of Pillow's affine_fixed"""
    ang = angle % 360.0
    r = -math.radians(ang)
    cx = cy = S / 2.0
    m0, m1, m3, m4 = round(math.cos(r), 15), round(math.sin(r), 15), round(-math.sin(r), 15), round(math.cos(r), 15)
    m2 = m0 * (-cx) + m1 * (-cy) + cx
    m5 = m3 * (-cx) + m4 * (-cy) + cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return [fix(m0), fix(m1), fix(m2 + m0 * 0.5 + m1 * 0.5), fix(m3), fix(m4), fix(m5 + m3 * 0.5 + m4 * 0.5)]


IDENTITY = [65536, 0, 32768, 0, 65536, 32768]


def rotate(img, angle):
    S = img.shape[0]
    assert img.shape[1] == S
    if not abs(angle) < 90:
        raise ValueError("only |angle| < 90")
    a0, a1, a2, a3, a4, a5 = rotation_integers(angle, S)
    y, x = np.meshgrid(np.arange(S, dtype=np.int64), np.arange(S, dtype=np.int64), indexing="ij")
    xin = (a2 + a1 * y + a0 * x) >> 16
    yin = (a5 + a4 * y + a3 * x) >> 16
    ok = (xin >= 0) & (xin < S) & (yin >= 0) & (yin < S)
    out = img[np.clip(yin, 0, S - 1), np.clip(xin, 0, S - 1)]
    out[~ok] = 0
    return out


# ------------------------------------------------------------------------------------------------ the whole transform
def transform_u8(img, S, train=False, crop=None, angle=0.0):
    """one image [H, W] or [H, W, 3] -> uint8 [S, S, 3]"""
    r = resize(img, S)
    oh, ow = r.shape[:2]
    if train:
        top, left = crop
        assert 0 <= top <= oh - S and 0 <= left <= ow - S
    else:
        top, left = center_crop_offsets(oh, ow, S)
    c = r[top:top + S, left:left + S]
    if train:
        c = rotate(c, angle)
    if c.ndim == 2:
        c = np.repeat(c[:, :, None], 3, axis=2)
    return np.ascontiguousarray(c)


def normalise(u8, mean=MEAN, std=STD):
    """uint8 [..., S, S, 3] -> float64 [..., 3, S, S] = (u / 255 - mean) / std"""
    x = (u8.astype(np.float64) / 255.0 - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return np.moveaxis(x, -1, -3)


def collate(u8, counts, mean=MEAN, std=STD):
    """uint8 [sum counts, S, S, 3] -> float64 [B, max counts, 3, S, S], absent images 0.0"""
    S = u8.shape[1]
    out = np.zeros((len(counts), max(counts), 3, S, S), np.float64)
    i = 0
    for b, n in enumerate(counts):
        out[b, :n] = normalise(u8[i:i + n], mean, std)
        i += n
    return out


# ------------------------------------------------------------------------------------------------ the cases of the fixture
# name -> list of images; an image = dict(H, W, C, id, S, train, crop, angle). crop None in train mode is filled in by `cases()`.
def _img(H, W, C=1, cid=0, S=48, train=False, crop=None, angle=0.0):
    return dict(H=H, W=W, C=C, id=cid, S=S, train=train, crop=crop, angle=angle)


ANGLES = [5.0, -5.0, 0.37, -1e-4, 0.0]


def cases():
    """name -> dict(S, train, images=[...], counts=[...]); one study per image unless `counts` says otherwise"""
    out = {}

    def add(name, images, counts=None):
        S, train = images[0]["S"], images[0]["train"]
        assert all(i["S"] == S and i["train"] == train for i in images)
        out[name] = dict(S=S, train=train, images=images, counts=counts or [1] * len(images))

    add("a", [_img(131, 107, cid=1)])
    add("b", [_img(107, 131, cid=2)])
    add("c", [_img(400, 333, cid=3)])
    add("d", [_img(40, 30, cid=4)])
    add("e", [_img(48, 77, cid=5), _img(77, 48, cid=6)])
    add("f", [_img(48, 48, cid=7)])
    add("g", [_img(131, 107, 3, cid=8)])
    h = []
    for H, W, cid in ((131, 107, 1), (107, 131, 2)):
        oh, ow = resized_hw(H, W, 48)
        crops = [(0, 0), (oh - 48, ow - 48), ((oh - 48) // 3, (ow - 48) // 3)]
        for i, ang in enumerate(ANGLES):
            h.append(_img(H, W, cid=cid, train=True, crop=crops[i % 3], angle=ang))
        h.append(_img(H, W, cid=cid, train=True, crop=crops[2], angle=5.0))
        h.append(_img(H, W, cid=cid, train=True, crop=crops[0], angle=-5.0))
    add("h", h)
    add("i_test", [_img(500, 417, cid=9, S=384)])
    add("i_train", [_img(500, 417, cid=9, S=384, train=True, crop=(31, 0), angle=3.3)])
    add("j", [_img(3056, 2544, cid=10, S=384)])
    add("k", [_img(131, 107, cid=1), _img(107, 131, 3, cid=11), _img(40, 30, cid=4), _img(400, 333, cid=3), _img(48, 48, 3, cid=12),
              _img(77, 48, cid=6)], counts=[2, 1, 3])
    # crop differences of 11 (5.5 -> 6, the even neighbour ABOVE; c and j have 9 -> 4 and 77 -> 38, the one below): 123 x 100 resamples to 59 x 48,
    # 48 x 59 has the target size already
    add("l", [_img(123, 100, cid=13), _img(48, 59, cid=14)])
    return out


def case_sources(case):
    return [source(i["H"], i["W"], i["C"], i["id"]) for i in case["images"]]


def case_expected(case):
    """the restatement's uint8 output [n, S, S, 3] of a case"""
    return np.stack([transform_u8(s, i["S"], i["train"], i["crop"], i["angle"]) for s, i in zip(case_sources(case), case["images"])])


def load_fixture():
    """-> {case name: uint8 [n, S, S, 3]} of the cases the fixture holds, and its metadata dict"""
    import json
    with np.load(FIXTURE) as z:
        meta = json.loads(bytes(z["meta"]).decode())
        outs = {k[4:]: z[k] for k in z.files if k.startswith("out_")}
    # a case of grey sources is stored with one channel: its three output channels are equal
    return {k: (np.repeat(v[..., None], 3, axis=-1) if v.ndim == 3 else v) for k, v in outs.items()}, meta
