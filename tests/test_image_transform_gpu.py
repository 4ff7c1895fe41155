"""GPU: the device image transforms (`cxr_image_transform`, `pixels.StudyImageTransform`) against the fixture recorded from Pillow
(tests/golden/image_transform.npz; the numpy restatement tests/image_transform_ref.py stands in for a case the fixture lacks).

Tolerances: none on the image content -- resize, crop and rotation are integer arithmetic and must equal Pillow byte for byte. The fp32 output is
u * (1 / (255 std)) - mean / std in fp32 against (u / 255 - mean) / std in float64: rtol 1e-5 / atol 1e-5, the bound
tests/test_kernels_gpu.py::test_pixels_normalize_pad_collate sets for the same expression. Padding slots are exactly 0.0."""
import numpy as np
import pytest
import torch

import image_transform_ref as ref
from bounds_util import F32, Guarded

pytestmark = pytest.mark.gpu

CASES = sorted(ref.cases())
U8 = torch.uint8


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import pixels
    return pixels


@pytest.fixture(scope="module")
def expected():
    """case -> uint8 [n, S, S, 3]: the Pillow fixture, or the restatement where the fixture has no entry; computed once, read-only"""
    fixture, _ = ref.load_fixture()
    out = {}
    for name, case in ref.cases().items():
        e = fixture[name] if name in fixture else ref.case_expected(case)
        e.setflags(write=False)
        out[name] = e
    return out


def _transform(P, case):
    return P.StudyImageTransform(case["S"], train=case["train"])


def _plan(P, case, sources=None):
    sources = ref.case_sources(case) if sources is None else sources
    t = _transform(P, case)
    kw = dict(crops=[i["crop"] for i in case["images"]], angles=[i["angle"] for i in case["images"]]) if case["train"] else {}
    shapes = [s.shape if s.ndim == 3 else s.shape + (1,) for s in sources]
    return t, t.plan(shapes, counts=case["counts"], **kw), sources


def _pack(plan, sources):
    """the packed source buffer, built here independently of pixels.py; the pitch padding is 0xFF so that a tap which strays into it shows"""
    buf = np.full(plan.src_bytes, 255, np.uint8)
    for s, (H, W, C), off, pitch in zip(sources, plan.shapes, plan.offsets, plan.pitches):
        buf[off:off + H * pitch].reshape(H, pitch)[:, :W * C] = s.reshape(H, W * C)
    return torch.from_numpy(buf).cuda()


def _call(t, plan, src, guards=None, **kw):
    """one guarded cxr_image_transform call -> (fp32 [B, Nmax, 3, S, S] | None, uint8 [n, S, S, 3] | None, the guarded buffers); `kw` overrides
    arguments. `guards`: a list that receives the guarded buffers before the call (for calls that are expected to fail)."""
    from cxrmate_amd import ops
    from cxrmate_amd._lib import LIB
    S, B, Nmax, n = plan.size, plan.B, plan.Nmax, plan.n_images
    want_f32, want_u8 = kw.pop("want_f32", True), kw.pop("want_u8", True)
    a = dict(n_images=n, n_bands=plan.n_bands, B=B, Nmax=Nmax, S=S, mean=t.mean, std=t.std, ws_bytes=plan.inter_bytes, inter_bytes=plan.inter_bytes,
             both_null=False)
    a.update(kw)
    desc, tables = torch.from_numpy(plan.desc).cuda(), torch.from_numpy(plan.tables).cuda()
    of = Guarded.flat(B * Nmax * 3 * S * S, F32)
    ou = Guarded.flat(n * S * S * 3, U8)
    ws = Guarded.flat(plan.inter_bytes + 8, U8)                                      # PAD = 8 guard bytes in front: + 8 more = 16-byte aligned
    ws.mask[8:16] = True                                                             # the alignment bytes are guard bytes as well
    if guards is not None:
        guards += [of, ou, ws]
    try:
        LIB.call("cxr_image_transform", src.data_ptr(), src.numel(), desc.data_ptr(), a["n_images"], a["n_bands"], tables.data_ptr(),
                 tables.numel(), a["B"], a["Nmax"], a["S"], *a["mean"], *a["std"], of.view.data_ptr() if want_f32 and not a["both_null"] else None,
                 ou.view.data_ptr() if want_u8 and not a["both_null"] else None, ws.view.data_ptr() + 8, a["ws_bytes"], a["inter_bytes"], ops._s())
    finally:
        for g, what in zip((of, ou, ws), ("fp32 output", "uint8 output", "workspace")):
            g.check(what)
    return (of.view.view(B, Nmax, 3, S, S) if want_f32 else None), (ou.view.view(n, S, S, 3) if want_u8 else None), (of, ou, ws)


def _untouched(g):
    it, v = {F32: (torch.int32, 0x7FA5A5A5), U8: (torch.uint8, 0xA5)}[g.dtype]
    return bool((g.buf.view(it) == v).all())


def _slots(counts):
    return [(b, j) for b, c in enumerate(counts) for j in range(c)]


def _check_f32(out, u8_expected, counts, t):
    want = ref.collate(u8_expected, counts, t.mean, t.std)
    got = out.cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    real = np.zeros(want.shape[:2], bool)
    for b, j in _slots(counts):
        real[b, j] = True
    assert (got[~real] == 0.0).all()                                                 # pad_sequence slots: exactly 0.0


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", CASES)
def test_case_equals_pillow_byte_for_byte(P, expected, name):
    case = ref.cases()[name]
    t, plan, sources = _plan(P, case)
    src = _pack(plan, sources)
    out, u8, _ = _call(t, plan, src)
    diff = int((u8.cpu().numpy() != expected[name]).sum())
    print(f"case {name}: {diff} differing bytes of {expected[name].size}")
    assert diff == 0
    _check_f32(out, expected[name], case["counts"], t)
    # the public path: packing, upload and launch by `transform` itself
    studies, i = [], 0
    for c in case["counts"]:
        studies.append(sources[i:i + c])
        i += c
    kw = dict(crops=[im["crop"] for im in case["images"]], angles=[im["angle"] for im in case["images"]]) if case["train"] else {}
    out2, u82 = t.transform(studies, "cuda", return_uint8=True, **kw)
    assert torch.equal(u82, u8) and torch.equal(out2, out)


def test_output_equals_collate_images_of_the_uint8_output(P, expected):
    case = ref.cases()["k"]
    t, plan, sources = _plan(P, case)
    out, u8, _ = _call(t, plan, _pack(plan, sources))
    studies, i = [], 0
    for c in case["counts"]:
        studies.append(u8[i:i + c].cpu())
        i += c
    want = P.collate_images(studies, "cuda")
    assert want.shape == out.shape == (3, 3, 3, 48, 48)
    np.testing.assert_allclose(out.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-5)
    # the cross-attention mask rule of the reference (first pixel of the image != 0, quirk Q3) sees exactly the real images
    assert (out[:, :, 0, 0, 0] != 0).cpu().tolist() == [[True, True, False], [True, False, False], [True, True, True]]
    assert bool((out[0, 2] == 0).all()) and bool((out[1, 1:] == 0).all())


def test_rotation_fill_normalises_to_minus_mean_over_std(P, expected):
    case = ref.cases()["h"]
    t, plan, sources = _plan(P, case)
    out, u8, _ = _call(t, plan, _pack(plan, sources))
    fill = -np.asarray(t.mean, np.float64) / np.asarray(t.std, np.float64)
    y, x = np.meshgrid(np.arange(48), np.arange(48), indexing="ij")
    filled = 0
    for i, im in enumerate(case["images"]):
        a0, a1, a2, a3, a4, a5 = ref.rotation_integers(im["angle"], 48)
        xin, yin = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
        outside = ~((xin >= 0) & (xin < 48) & (yin >= 0) & (yin < 48))
        if abs(im["angle"]) == 5.0:                                                  # 24 sin(5 deg) = 2.1 pixels: the corners read outside
            assert outside[0, 0] and outside[47, 47] and outside[0, 47] and outside[47, 0]
        filled += int(outside.sum())
        assert (u8[i].cpu().numpy()[outside] == 0).all()
        got = out[i, 0].cpu().numpy()[:, outside]                                    # [3, pixels outside]
        np.testing.assert_allclose(got, np.broadcast_to(fill[:, None], got.shape), rtol=1e-6, atol=0)
        assert (got != 0).all()
    assert filled > 100


def test_grey_equals_replicated_rgb(P):
    for name in ("a", "c", "h"):
        case = ref.cases()[name]
        grey = ref.case_sources(case)
        t, plan, _ = _plan(P, case, grey)
        _, u8g, _ = _call(t, plan, _pack(plan, grey), want_f32=False)
        rgb = [np.ascontiguousarray(np.repeat(s[:, :, None], 3, axis=2)) for s in grey]
        t, plan3, _ = _plan(P, case, rgb)
        assert plan3.shapes[0][2] == 3
        _, u8c, _ = _call(t, plan3, _pack(plan3, rgb), want_f32=False)
        assert torch.equal(u8g, u8c)


def test_repeatable_and_stream_independent(P, expected):
    case = ref.cases()["k"]
    t, plan, sources = _plan(P, case)
    src = _pack(plan, sources)
    out1, u81, _ = _call(t, plan, src)
    out2, u82, _ = _call(t, plan, src)
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32)) and torch.equal(u81, u82)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out3, u83, _ = _call(t, plan, src)
        studies = [sources[0:2], sources[2:3], sources[3:6]]
        out4, u84 = t.transform(studies, "cuda", return_uint8=True)
    s.synchronize()
    assert torch.equal(out1.view(torch.int32), out3.view(torch.int32)) and torch.equal(u81, u83)
    assert torch.equal(out1.view(torch.int32), out4.view(torch.int32)) and torch.equal(u81, u84)


def test_either_output_alone(P, expected):
    case = ref.cases()["k"]
    t, plan, sources = _plan(P, case)
    src = _pack(plan, sources)
    out, none, (of, ou, ws) = _call(t, plan, src, want_u8=False)
    assert none is None and _untouched(ou)
    _check_f32(out, expected["k"], case["counts"], t)
    none, u8, (of, ou, ws) = _call(t, plan, src, want_f32=False)
    assert none is None and _untouched(of)
    assert int((u8.cpu().numpy() != expected["k"]).sum()) == 0
    assert t.transform([sources[0:2], sources[2:3], sources[3:6]], "cuda").shape == (3, 3, 3, 48, 48)


def test_source_kinds(P, expected):
    """numpy arrays, torch CPU tensors, torch device tensors and PIL images, mixed in one batch"""
    case = ref.cases()["k"]
    t, plan, s = _plan(P, case)
    imgs = [s[0], torch.from_numpy(s[1]), torch.from_numpy(s[2]).cuda(), s[3], torch.from_numpy(s[4]).cuda(), torch.from_numpy(s[5])]
    try:
        from PIL import Image
        imgs[3] = Image.fromarray(s[3])
    except ImportError:
        pass
    out, u8 = t.transform([imgs[0:2], imgs[2:3], imgs[3:6]], "cuda", return_uint8=True)
    assert int((u8.cpu().numpy() != expected["k"]).sum()) == 0
    _check_f32(out, expected["k"], case["counts"], t)
    out, u8 = t.transform([[i for i in imgs if isinstance(i, torch.Tensor) and i.is_cuda]], "cuda", return_uint8=True)       # device sources only
    assert int((u8.cpu().numpy() != expected["k"][[2, 4]]).sum()) == 0


def test_random_train_transform_is_seeded(P):
    case = ref.cases()["k"]
    s = ref.case_sources(case)
    t = P.StudyImageTransform(48, train=True)
    studies = [s[0:2], s[2:3], s[3:6]]
    a, ua = t.transform(studies, "cuda", generator=torch.Generator().manual_seed(11), return_uint8=True)
    b, ub = t.transform(studies, "cuda", generator=torch.Generator().manual_seed(11), return_uint8=True)
    assert torch.equal(ua, ub) and torch.equal(a, b)
    plan = t.plan([x.shape for x in s], generator=torch.Generator().manual_seed(11), counts=[2, 1, 3])
    crops, angles = t.draw(plan.resized, torch.Generator().manual_seed(11))
    want = np.stack([ref.transform_u8(x, 48, True, c, ang) for x, c, ang in zip(s, crops, angles)])
    assert int((ua.cpu().numpy() != want).sum()) == 0


# ------------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_return_the_error_code_and_write_nothing(P):
    from cxrmate_amd._lib import CxrError
    case = ref.cases()["k"]
    t, plan, sources = _plan(P, case)
    src = _pack(plan, sources)
    bad = [dict(n_images=0), dict(n_images=-1), dict(S=0), dict(S=-48), dict(std=(0.229, 0.0, 0.225)), dict(std=(0.0, 0.224, 0.225)),
           dict(both_null=True), dict(ws_bytes=plan.inter_bytes - 1), dict(ws_bytes=0), dict(B=0), dict(Nmax=0), dict(n_bands=0),
           dict(B=1, Nmax=2)]                                                        # fewer slots than images
    for kw in bad:
        guards = []
        with pytest.raises(CxrError, match="cxr_image_transform failed with code -1"):
            _call(t, plan, src, guards, **kw)
        torch.cuda.synchronize()
        assert len(guards) == 3 and all(_untouched(g) for g in guards), kw


def test_a_descriptor_outside_its_buffers_is_not_followed(P, expected):
    """A descriptor whose source, table or intermediate range leaves the buffers as passed disables that image only: NaN / 0 for it, the other
    images as usual, nothing outside the outputs touched (the call itself cannot see device memory, so it succeeds)."""
    import copy
    case = ref.cases()["k"]
    t, plan, sources = _plan(P, case)
    src = _pack(plan, sources)
    for field, value in ((0, 1 << 27), (9, 1 << 30), (11, -5), (13, 1 << 27), (4, 8), (7, 1000), (3, 2), (1, 1 << 20)):
        p = copy.copy(plan)
        p.desc = plan.desc.copy()
        p.desc[3 * 24 + field] = value                                               # image 3 = slot [2, 0]
        out, u8, _ = _call(t, p, src)
        got = u8.cpu().numpy()
        keep = [0, 1, 2, 4, 5]
        assert int((got[keep] != expected["k"][keep]).sum()) == 0, field
        assert (got[3] == 0).all() and bool(torch.isnan(out[2, 0]).all()), field
        assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2, 1:]).all())


# ------------------------------------------------------------------------------------------------ end to end
def test_encoder_accepts_the_transform_output(P):
    from cxrmate_amd import modelling
    from cxrmate_amd.config import tiny_config
    cfg = tiny_config(vocab_size=1000, decoder_layers=2, image_size=96)
    m = modelling.MultiCXREncoderDecoderModel(cfg, device="cuda:0", seed=3)
    s = ref.case_sources(ref.cases()["k"])
    images = P.StudyImageTransform(96).transform([s[0:2], s[2:3], s[3:6]], "cuda")
    assert images.shape == (3, 3, 3, 96, 96)
    with torch.no_grad():
        feats, _ = m._enc.forward(images.view(-1, 3, 96, 96).contiguous())
    torch.cuda.synchronize()
    assert feats.shape == (9 * cfg.encoder.grid(2) ** 2, cfg.encoder.projection_size)
    assert bool(torch.isfinite(feats.float()).all())
