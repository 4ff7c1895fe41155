"""CPU: the surface of the device image transforms that needs no GPU -- the C ABI declaration, the wrapper refusing host tensors, the workspace
formula, everything `StudyImageTransform.plan` decides on the host (resized sizes, crop offsets, coefficient tables, rotation integers, the
random draws) and the tests' own numpy restatement (tests/image_transform_ref.py): against the fixture recorded from Pillow, byte for byte, and
against the installed Pillow when there is one."""
import ctypes

import numpy as np
import pytest
import torch

import image_transform_ref as ref
from cxrmate_amd import ops, pixels
from cxrmate_amd._lib import CxrError, parse_header

CASES = sorted(ref.cases())


def test_header_declares_the_entry_point():
    protos = parse_header()
    v, L, I, F = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
    want = [("src", v), ("src_bytes", L), ("desc", v), ("n_images", I), ("n_bands", I), ("tables", v), ("n_table_ints", L), ("B", I), ("Nmax", I),
            ("S", I), ("mean0", F), ("mean1", F), ("mean2", F), ("std0", F), ("std1", F), ("std2", F), ("out_f32", v), ("out_u8", v),
            ("workspace", v), ("workspace_bytes", L), ("inter_bytes", L), ("stream", v)]
    assert "cxr_image_transform" in protos
    assert [(n, t) for t, n in protos["cxr_image_transform"]] == want
    assert [n for n in protos if "image_transform" in n] == ["cxr_image_transform"]              # exactly one entry point was added


def test_wrapper_refuses_host_tensors():
    t = pixels.StudyImageTransform(48)
    p = t.plan([(50, 60, 1)])
    with pytest.raises(CxrError):
        ops.image_transform(torch.zeros(p.src_bytes, dtype=torch.uint8), torch.from_numpy(p.desc), torch.from_numpy(p.tables), 1, p.n_bands, 1, 1,
                            48, t.mean, t.std, p.inter_bytes)
    with pytest.raises(CxrError):
        t.transform([[ref.source(50, 60, 1)]], "cpu")


def test_workspace_formula():
    assert ops.image_transform_workspace_bytes([]) == 0
    assert ops.image_transform_workspace_bytes([(131, 48, 1)]) == 6288                            # 131 * 48 = 6288 = 393 * 16
    assert ops.image_transform_workspace_bytes([(107, 58, 3), (40, 48, 1)]) == 18624 + 1920       # 107 * 58 * 3 = 18618 -> 18624
    assert ops.image_transform_workspace_bytes([(3056, 384, 1)] * 64) == 64 * 3056 * 384
    p = pixels.StudyImageTransform(48).plan([(131, 107, 1), (107, 131, 3)])
    assert p.inter == [(131, 48, 1), (107, 58, 3)] and p.inter_bytes == 6288 + 18624
    assert ops.IMAGE_TRANSFORM_DESC_INTS == 24 and ops.IMAGE_TRANSFORM_BAND_BYTES == 49152


# ------------------------------------------------------------------------------------------------ plan
def test_plan_resized_sizes():
    S = 384
    assert pixels.resized_hw(3056, 2544, S) == (461, 384) and pixels.resized_hw(2544, 3056, S) == (384, 461)
    assert pixels.resized_hw(2022, 2577, S) == (384, 489)
    assert pixels.resized_hw(384, 384, S) == (384, 384) and pixels.resized_hw(500, 384, S) == (500, 384)
    assert pixels.resized_hw(200, 300, S) == (384, 576)                                          # upscale
    assert pixels.resized_hw(131, 107, 48) == (58, 48) and pixels.resized_hw(40, 30, 48) == (64, 48)
    for H, W, S in ((3056, 2544, 384), (97, 61, 48), (61, 97, 48), (333, 400, 48), (1, 7, 48)):
        assert pixels.resized_hw(H, W, S) == ref.resized_hw(H, W, S)
    p = pixels.StudyImageTransform(48).plan([(131, 107), (107, 131, 3), (48, 48, 1)])
    assert p.resized == [(58, 48), (48, 58), (48, 48)] and p.shapes[0] == (131, 107, 1)


def test_plan_center_crop_rounds_half_to_even():
    assert pixels.center_crop_offsets(461, 384, 384) == (38, 0)                                  # 77 / 2 = 38.5 -> 38
    assert pixels.center_crop_offsets(384, 463, 384) == (0, 40)                                  # 79 / 2 = 39.5 -> 40
    assert pixels.center_crop_offsets(58, 48, 48) == (5, 0) and pixels.center_crop_offsets(48, 59, 48) == (0, 6)      # 5.5 -> 6
    p = pixels.StudyImageTransform(48).plan([(131, 107, 1), (107, 131, 1), (400, 333, 1)])
    assert p.crops == [(5, 0), (0, 5), (4, 0)] and p.rotations is None                           # 57 - 48 = 9 -> 4.5 -> 4


@pytest.mark.parametrize("sizes", [(3056, 461), (30, 48), (2544, 384), (48, 48), (400, 57), (77, 48)])
def test_plan_tables_equal_the_restatement(sizes):
    ksize, xmin, n, k = pixels.resample_table(*sizes)
    rk, rxmin, rn, rweights = ref.coefficients(*sizes)
    assert ksize == rk and k.shape == (sizes[1], ksize) and k.dtype == np.int32
    assert np.array_equal(xmin, rxmin) and np.array_equal(n, rn) and np.array_equal(k, rweights)
    assert pixels.resample_table(*sizes) is pixels.resample_table(*sizes)                        # cached per (in, out)


def test_plan_table_shapes_by_hand():
    """3056 -> 461: scale 6.63, support 6.63, ksize = 2 * 7 + 1 = 15. 30 -> 48: an upscale has fs = 1, support 1, ksize 3. Output 0 is centred
    at 0.3125: (int)(0.3125 - 1 + 0.5) = 0 (truncation, not floor) and (int)(0.3125 + 1 + 0.5) = 1, one tap, normalised to 1. Output 1 is centred at
    0.9375: taps 0 and 1 with tri(-0.4375) = 0.5625 and tri(0.5625) = 0.4375, which sum to 1 already."""
    assert pixels.resample_table(3056, 461)[0] == 15 and pixels.resample_table(30, 48)[0] == 3
    _, xmin, n, k = pixels.resample_table(30, 48)
    assert xmin[0] == 0 and n[0] == 1 and k[0].tolist() == [4194304, 0, 0]
    assert xmin[1] == 0 and n[1] == 2 and k[1].tolist() == [2359296, 1835008, 0]                   # 0.5625 and 0.4375 of 2^22
    _, xmin, n, k = pixels.resample_table(48, 48)                                                # a pass that resamples nothing: a copy
    assert np.array_equal(xmin, np.arange(48)) and (k[:, 0] == 4194304).all() and (k[:, 1:] == 0).all()
    _, xmin, n, k = pixels.resample_table(3056, 461)
    assert (xmin >= 0).all() and (xmin + n <= 3056).all() and (n <= 15).all() and (k >= 0).all()
    assert abs(k.sum(axis=1) - 4194304).max() <= 8                                               # 15 roundings of at most half a unit each


def test_plan_device_tables_layout():
    p = pixels.StudyImageTransform(48).plan([(131, 107, 1), (131, 107, 3)], counts=[2])
    d = p.desc[:48].reshape(2, 24)
    assert d[0, :9].tolist() == [0, 131, 107, 1, 112, 58, 48, 5, 0] and d[1, :9].tolist() == [131 * 112 // 16, 131, 107, 3, 336, 58, 48, 5, 0]
    assert d[0, 9:13].tolist() == d[1, 9:13].tolist()                                            # the tables of a size pair are stored once
    assert d[0, 16:22].tolist() == [65536, 0, 32768, 0, 65536, 32768]                            # test mode: the identity
    assert p.desc[48:50].tolist() == [0, 1]                                                      # slot map
    assert p.desc[50:].reshape(-1, 2).tolist() == [[0, 0], [1, 0]] and p.n_bands == 2            # one band each: 49152 // 112 >= 131 rows
    ksize, xmin, n, k = pixels.resample_table(107, 48)
    off = d[0, 9]
    assert d[0, 10] == ksize
    assert np.array_equal(p.tables[off:off + 96].reshape(48, 2), np.stack([xmin, n], 1))
    assert np.array_equal(p.tables[off + 96:off + 96 + 48 * ksize].reshape(ksize, 48), k.T)
    assert p.tables.size == 48 * (2 + ksize) + 58 * (2 + pixels.resample_table(131, 58)[0])
    big = pixels.StudyImageTransform(384).plan([(3056, 2544, 1)])
    assert big.pitches == [2544] and big.n_bands == -(-3056 // (49152 // 2544))                  # 19 rows per band


def test_plan_rotation_integers():
    assert pixels.rotation_integers(0.0, 48) == (65536, 0, 32768, 0, 65536, 32768) == pixels.ROTATION_IDENTITY
    for ang in ref.ANGLES + [1e-4, 1e-3, -2.5, 3.14159, 4.999, 89.9, -89.9]:
        for S in (48, 96, 384):
            assert list(pixels.rotation_integers(ang, S)) == ref.rotation_integers(ang, S)
    a = pixels.rotation_integers(5.0, 384)
    assert a[0] == a[4] == int(np.floor(np.cos(np.radians(5.0)) * 65536 + 0.5)) and a[1] == -a[3] < 0       # r = -radians(angle): sin r < 0
    for bad in (90.0, -90.0, 180.0, 360.0, 1e9, float("nan")):
        with pytest.raises(ValueError):
            pixels.rotation_integers(bad, 48)
    t = pixels.StudyImageTransform(48, train=True)
    with pytest.raises(ValueError):
        t.plan([(131, 107, 1)], crops=[(0, 0)], angles=[90.0])
    with pytest.raises(ValueError):
        t.plan([(131, 107, 1)], crops=[(11, 0)], angles=[0.0])                                   # oh - S = 10
    p = t.plan([(131, 107, 1)], crops=[(10, 0)], angles=[-5.0])
    assert p.crops == [(10, 0)] and list(p.rotations[0]) == ref.rotation_integers(-5.0, 48)
    assert p.desc[16:22].tolist() == ref.rotation_integers(-5.0, 48)
    with pytest.raises(ValueError):
        pixels.StudyImageTransform(48).plan([(131, 107, 1)], crops=[(0, 0)], angles=[0.0])       # test mode takes neither


def test_random_draws_contract():
    t = pixels.StudyImageTransform(48, train=True, degrees=5.0)
    shapes = [(131, 107, 1), (107, 131, 3), (48, 48, 1), (400, 333, 1)] * 8
    p1 = t.plan(shapes, generator=torch.Generator().manual_seed(7))
    p2 = t.plan(shapes, generator=torch.Generator().manual_seed(7))
    p3 = t.plan(shapes, generator=torch.Generator().manual_seed(8))
    assert p1.crops == p2.crops and p1.rotations == p2.rotations and np.array_equal(p1.desc, p2.desc)
    assert p1.crops != p3.crops or p1.rotations != p3.rotations
    for (top, left), (oh, ow) in zip(p1.crops, p1.resized):
        assert 0 <= top <= oh - 48 and 0 <= left <= ow - 48
    crops, angles = t.draw(p1.resized, torch.Generator().manual_seed(7))
    assert crops == p1.crops and all(-5.0 <= a <= 5.0 for a in angles) and len(set(angles)) > 1
    assert {c[0] for c in crops[0::4]} != {0} and {c[1] for c in crops[1::4]} != {0}             # the free axis is really drawn
    # the order of the draws: top, left, angle -- and nothing for the crop of an image that is S x S already
    g = torch.Generator().manual_seed(3)
    top = int(torch.randint(0, 11, (1,), generator=g))
    left = int(torch.randint(0, 1, (1,), generator=g))
    a0 = float(torch.empty(1).uniform_(-5.0, 5.0, generator=g))
    a1 = float(torch.empty(1).uniform_(-5.0, 5.0, generator=g))
    crops, angles = t.draw([(58, 48), (48, 48)], torch.Generator().manual_seed(3))
    assert crops == [(top, left), (0, 0)] and angles == [a0, a1]
    # explicit values are honoured
    p = t.plan([(131, 107, 1)], crops=[(3, 0)], angles=[0.37])
    assert p.crops == [(3, 0)] and list(p.rotations[0]) == ref.rotation_integers(0.37, 48)


def test_plan_refuses_bad_input():
    t = pixels.StudyImageTransform(48)
    for shapes, counts in (([], None), ([(10, 10, 2)], None), ([(0, 10, 1)], None), ([(10, 10, 1)], [2]), ([(10, 50000, 1)], None)):
        with pytest.raises(ValueError):
            t.plan(shapes, counts=counts)
    with pytest.raises(ValueError):
        pixels.StudyImageTransform(0)
    with pytest.raises(ValueError):
        pixels.StudyImageTransform(48, std=(0.2, 0.0, 0.2))
    with pytest.raises(ValueError):
        t.transform([[np.zeros((10, 10), np.float32)]], "cpu")


# ------------------------------------------------------------------------------------------------ the restatement
def test_source_is_the_closed_formula():
    s = ref.source(5, 7, 3, 2)
    assert s.shape == (5, 7, 3) and s.dtype == np.uint8 and ref.source(5, 7, 1).shape == (5, 7)
    for (y, x, c) in ((0, 0, 0), (4, 6, 2), (3, 5, 1)):
        assert s[y, x, c] == (7 * x + 13 * y + ((x * y) >> 6) + 5 * ((x ^ y) & 15) + 31 * c + 34) & 255


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_fixture(name):
    fixture, meta = ref.load_fixture()
    case = ref.cases()[name]
    assert meta["cases"][name]["counts"] == case["counts"]
    for a, b in zip(meta["cases"][name]["images"], case["images"]):
        assert a == {**b, "crop": list(b["crop"]) if b["crop"] is not None else None}             # the recorded parameters are the case list's
    got = ref.case_expected(case)
    assert got.shape == fixture[name].shape and int((got != fixture[name]).sum()) == 0


def test_fixture_covers_every_case_and_half_to_even():
    fixture, meta = ref.load_fixture()
    assert sorted(fixture) == CASES and meta["pillow"]
    assert set("abcdefghjkl") | {"i_test", "i_train"} == set(CASES)
    # a and b resize to 58 x 48 / 48 x 58: an even difference. The odd ones, where Python's round goes to the even neighbour:
    c = ref.cases()["c"]["images"][0]                                                            # 57 - 48 = 9: 4.5 rounds down to 4
    assert ref.resized_hw(c["H"], c["W"], 48) == (57, 48) and ref.center_crop_offsets(57, 48, 48) == (4, 0)
    j = ref.cases()["j"]["images"][0]                                                            # 461 - 384 = 77: 38.5 rounds to 38
    assert ref.center_crop_offsets(*ref.resized_hw(j["H"], j["W"], 384), 384) == (38, 0)
    l0, l1 = ref.cases()["l"]["images"]                                                          # 59 - 48 = 11: 5.5 rounds up to 6
    assert ref.center_crop_offsets(*ref.resized_hw(l0["H"], l0["W"], 48), 48) == (6, 0)
    assert ref.resized_hw(l1["H"], l1["W"], 48) == (48, 59) and ref.center_crop_offsets(48, 59, 48) == (0, 6)


def test_grey_equals_replicated_rgb_in_the_restatement():
    g = ref.source(131, 107, 1, 1)
    rgb = np.repeat(g[:, :, None], 3, axis=2)
    for train, crop, ang in ((False, None, 0.0), (True, (3, 0), 4.2)):
        assert np.array_equal(ref.transform_u8(g, 48, train, crop, ang), ref.transform_u8(rgb, 48, train, crop, ang))


@pytest.mark.parametrize("name", [c for c in CASES if c not in ("j", "k")])
def test_restatement_equals_live_pillow(name):
    pytest.importorskip("PIL")
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_golden_image_transform", os.path.join(ref.GOLDEN, "make_golden_image_transform.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    case = ref.cases()[name]
    for src, p, want in zip(ref.case_sources(case), case["images"], ref.case_expected(case)):
        got = gen.pillow_transform(src, p)
        got = got if got.ndim == 3 else np.repeat(got[:, :, None], 3, axis=2)
        assert int((got != want).sum()) == 0
