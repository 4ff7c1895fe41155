"""GPU: every attention kernel against the float64 reference of tests/attention_ref.py, element by element, on inputs where each key and each
query matters (needle: every query is aimed at one key; poison: a key that must not be seen would dominate the row and carries V = 4096; ramp:
the running maximum rises at every 32-key step). The bounds are derived from the kernels' rounding points in attention_ref's docstring:

  context (MFMA kernels)   |out - ref| <= (2^-8 + 2 eta) * sum_j p f |v|, then the bf16 bracket      (VALU decode kernel: 2 eta * sum_j p f |v|)
  LSE                      |out - ref| <= ln sum_j p_j e^(ln2 eps2_j) + 2^-22 + depth(Tk) 2^-24 + 4 fp32 steps of |ref|
  dV / dK / dQ             the matching absolute sums times (2^-8 + eta_p + ...), from the kernel's own bf16 O and fp32 LSE
  eps2_j = 23 * 2^-24 * scale log2(e) sum_d |q_d k_jd|, eps2 = max_j eps2_j, eta = expm1(2 ln2 eps2) + 2^-21 + 2 depth(Tk) 2^-24, depth(T) = 32 + T/8

Inputs are views of taller and wider buffers whose other elements are bf16 NaN patterns; outputs are views of guarded buffers.

Rows without a visible key (a whole image key-padded) cannot reach the loss -- the decoder's self-attention row i always sees key i unless
position i is itself padding, whose label the loss ignores and which no other row may attend to; a study's cross-attention keys are masked
per zero-padded image and every study has a real image -- so today's behaviour is pinned: the forward attends uniformly, the backward gives
such a row no gradient (test_rows_without_a_visible_key).

MEASURED on the MI355X, the worst case of each kernel (test_no_bound_is_loose prints them and asserts that each is at least 0.02; every case
asserts its own figure below 1). bf16 outputs of the MFMA kernels: the largest fraction of the derived tolerance that an element needs once
half a bf16 step at the output, its own rounding, is taken off (stricter than the bracket); LSE: max |err| / bound.
  attn_fwd2_kernel<2 | 4, 0 | 1 | 2>   context 0.655, LSE 0.120 (cases: 0.041 .. 0.120)
  attn_fwd_kernel                      context 0.557, LSE 0.089
  attn_bwd_dq_kernel, dq2<4, 0>        dQ 0.722
  attn_bwd_dkdv_kernel<4>              dK 0.796, dV 0.889
  attn_cross_mfma_kernel<1 | 2 | 3>, <5, true>, split + merge     0.377
  attn_cross_mfma_kernel<.., QPROJ>    0.044 (the bound of the projected query's rounding is a worst-case sum over 64 dimensions)
  attn_decode_kernel (+ merge)         1.000 of the BRACKET: with P in fp32 the tolerance is some 1e-5 of sum p |v|, far below half a bf16 step, so
                                       the figure of this kernel is |err| against the bracket's half-width. A correctly rounded output whose
                                       reference lies half-way between two bf16 values reaches 1 exactly; no output may exceed it.
"""
import functools

import numpy as np
import pytest
import torch
import attention_ref as R
from bounds_util import Guarded, assert_bf16_bracket, assert_f32_bound

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SCALE = 0.125


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import ops as _ops
    from cxrmate_amd._lib import LIB
    LIB.load()
    return _ops


def embed(t, rows=(1, 2), cols=(8, 8)):
    """t bf16 CPU [B, T, D] -> the same values on the GPU as a view of a [B, T + 3, D + 16] buffer whose other elements are bf16 NaNs"""
    B, T, D = t.shape
    buf = torch.empty(B, T + sum(rows), D + sum(cols), dtype=BF, device="cuda")
    buf.view(torch.int16).fill_(R.NAN_BF16)
    view = buf[:, rows[0]:rows[0] + T, cols[0]:cols[0] + D]
    view.copy_(t)
    return view


def guarded_like(B, T, D):
    return Guarded((B, T + 3, D + 16), BF, (slice(None), slice(1, 1 + T), slice(8, 8 + D)))


FIGURES = {}                 # kernel -> the MEASURED figures of the cases run so far (test_no_bound_is_loose)


def bracket(out, ref, tol, what, kernel, fp32_only=False):
    """assert_bf16_bracket, then the case's figure. MFMA kernels: the largest fraction of the derived tolerance that an element needs once half a
    bf16 step at the output, its own rounding, is taken off; it must stay below 1, which is stricter than the bracket. fp32_only (the VALU decode
    kernel, whose tolerance is some 1e-5 of sum p |v| and cannot show through a bf16 output): the largest |err| as a fraction of the bracket."""
    frac, used = R.bf16_figures(out, ref, tol)
    print(f"MEASURED {what}: {frac:.4f} of the bracket, {used:.4f} of the tolerance")
    assert_bf16_bracket(out, ref, tol, what)
    FIGURES.setdefault(kernel, []).append(frac if fp32_only else used)
    assert (frac <= 1.0) if fp32_only else (used < 1.0), f"{what}: {used:.4f} of the tolerance beyond the output's own rounding"


def finite(t, what):
    assert bool(torch.isfinite(t.float()).all()), f"{what}: non-finite output"


def dropout_factor(ops, drop, Bq, H, Tq, Tk):
    if drop is None:
        return None
    p, seed, site, t0 = drop
    return ops.dropout_mask(Bq * H * Tq, Tk, p, seed, site, Tq, t0, factor=True).view(Bq, H, Tq, Tk).cpu().double().numpy()


def drop_args(p):
    return None if not p else (p, torch.full((1,), 271828, dtype=torch.int32, device="cuda"), 18, 5)


@functools.lru_cache(maxsize=2)
def tiled_case(family, B, H, Tq, Tk, masked, causal, shift):
    skip = (0,) if causal and shift == 0 else ()                    # (masking key 0 there would leave query 0 without a visible key)
    kpm = R.make_kpm(B, Tk, skip=skip) if masked else None
    c = R.make_inputs(family, B, H, Tq, Tk, kpm, causal, shift, poison=masked or (causal and shift < Tk - Tq), seed=B + H)
    c["kpm"], c["skip"] = kpm, set(skip)
    assert bool(c["vis"].any(2).all()), "a query without a visible key"
    return c


def check_coverage(c, B, H, Tq, Tk, masked):
    """the generators reach what they promise: single masked keys at every edge position; keys 0, 31, 32, 63, 64 and Tk - 1 are needle targets in
    every case, and every key that some query sees is one wherever the case has queries enough"""
    if masked:
        assert R.flipped_positions(c["kpm"]) >= set(R.edge_positions(Tk)) - c.get("skip", set()), "mask positions"
    if c["covered"] is not None:
        seen = set(np.nonzero(c["vis"].any((0, 1)))[0].tolist())
        listed = set(R.listed_positions(Tk)) & seen
        assert listed <= c["covered"], f"needle targets miss {sorted(listed - c['covered'])}"
        causal = bool((c["vis"].any(1) & ~c["vis"].all(1)).any())               # some key is seen by some rows of an image only
        if B * H * Tq >= (3 if causal else 2 if masked else 1) * Tk:           # enough queries: every key that some query sees
            assert seen <= c["covered"], f"needle targets miss keys {sorted(seen - c['covered'])[:8]}"


# ------------------------------------------------------------------------------------------------ forward
# family, B, H, Tq, Tk, masked (key padding: B = 3), causal, causal_shift (None: Tk - Tq), dropout p
FWD = [
    ("gauss", 3, 3, 1, 1, False, False, None, 0.0),
    ("needle", 2, 2, 31, 31, False, False, None, 0.0),
    ("needle", 1, 3, 33, 32, False, False, None, 0.0),
    ("ramp", 1, 1, 64, 33, False, False, None, 0.0),
    ("needle", 1, 2, 65, 63, False, False, None, 0.0),
    ("ramp_down", 1, 1, 128, 64, False, False, None, 0.0),
    ("needle", 1, 2, 129, 65, False, False, None, 0.0),
    ("ramp", 1, 1, 257, 97, False, False, None, 0.0),
    ("needle", 1, 3, 257, 145, False, False, None, 0.0),
    ("gauss", 1, 1, 129, 145, False, False, None, 0.0),
    ("ramp", 1, 2, 33, 1152, False, False, None, 0.0),
    ("ramp_down", 1, 1, 129, 1152, False, False, None, 0.0),
    ("needle", 2, 3, 257, 1152, False, False, None, 0.0),
    ("needle", 3, 2, 33, 97, True, False, None, 0.0),
    ("needle", 3, 2, 129, 145, True, False, None, 0.0),        # key padding alone at Tq > 128: skipped and partly masked tiles of <4, 1>
    ("needle", 3, 2, 65, 65, True, True, 0, 0.0),
    ("needle", 3, 2, 64, 145, True, True, None, 0.0),          # shift 81
    ("needle", 3, 2, 129, 145, True, True, 5, 0.0),            # keys past 133 are hidden from every query
    ("ramp", 3, 1, 257, 257, True, True, 0, 0.0),
    ("ramp_down", 3, 1, 128, 128, True, True, 0, 0.0),
    ("gauss", 3, 2, 31, 1152, True, False, None, 0.0),
    ("needle", 1, 2, 128, 128, False, True, 0, 0.0),
    ("needle", 3, 3, 1, 33, False, True, None, 0.0),           # one query per (image, head), shift 32
    ("needle", 3, 2, 65, 97, True, True, None, 0.1),           # shift 32
    ("gauss", 1, 2, 129, 145, False, False, None, 0.1),
    ("needle", 1, 2, 64, 97, False, False, None, 0.1),
]
FWD_V1 = [FWD[8], FWD[12], FWD[16], FWD[18], FWD[23]]


def run_forward(ops, case, ver):
    family, B, H, Tq, Tk, masked, causal, shift, pdrop = case
    shift = Tk - Tq if shift is None else shift
    D = H * 64
    c = tiled_case(family, B, H, Tq, Tk, masked, causal, shift)
    check_coverage(c, B, H, Tq, Tk, masked)
    q, k, v = embed(c["q"]), embed(c["k"]), embed(c["v"])
    kpm = c["kpm"].cuda() if masked else None
    drop = drop_args(pdrop)
    out, out2 = guarded_like(B, Tq, D), guarded_like(B, Tq, D)
    try:
        ops.attention_config(ver, 0)
        _, lse = ops.attention(q, k, v, H, SCALE, kpm=kpm, causal=causal, causal_shift=shift, need_lse=True, out=out.view, drop=drop)
        ops.attention(q, k, v, H, SCALE, kpm=kpm, causal=causal, causal_shift=shift, need_lse=False, out=out2.view, drop=drop)
    finally:
        ops.attention_config(2, 0)
    what = f"attention v{ver} {family} B{B} H{H} {Tq}x{Tk}{' kpm' if masked else ''}{f' causal{shift:+d}' if causal else ''}{' drop' if pdrop else ''}"
    out.check(what), out2.check(what)
    finite(out.view, what), finite(lse, what)
    assert torch.equal(out.view, out2.view), f"{what}: the context depends on need_lse"
    ref = R.forward(c["q"], c["k"], c["v"], H, SCALE, c["vis"], fac=dropout_factor(ops, drop, B, H, Tq, Tk))
    r_lse = R.f32_ratio(lse, ref["LSE"], ref["tol_LSE"], 4)
    print(f"MEASURED {what} LSE: max |err| / bound {r_lse:.4f}")
    bracket(out.view, ref["O"], ref["tol_O"], what + " context", f"forward v{ver} context")
    assert_f32_bound(lse, ref["LSE"], ref["tol_LSE"].ravel(), 4, what + " LSE")
    FIGURES.setdefault(f"forward v{ver} LSE", []).append(r_lse)


@pytest.mark.parametrize("case", FWD, ids=lambda c: "-".join(str(x) for x in c))
def test_attention_forward(ops, case):
    """attn_fwd2_kernel<2 | 4, MODE 0 | 1 | 2>: context within (2^-8 + 2 eta) * sum_j p f |v| and the bf16 bracket, LSE within
    ln2 eps2 + 2^-22 + depth(Tk) 2^-24 + 4 fp32 steps (attention_ref); guards intact, outputs finite, the same context with and without the LSE."""
    run_forward(ops, case, 2)


@pytest.mark.parametrize("case", FWD_V1, ids=lambda c: "-".join(str(x) for x in c))
def test_attention_forward_32_rows_per_wave(ops, case):
    """attn_fwd_kernel (attention_config(1, .)): the same bounds"""
    run_forward(ops, case, 1)


def test_attention_e4m3_context_is_the_quantised_bf16_context_on_needles(ops):
    B, H, Tq, Tk = 1, 3, 257, 145
    c = tiled_case("needle", B, H, Tq, Tk, False, False, Tk - Tq)
    q, k, v = embed(c["q"]), embed(c["k"]), embed(c["v"])
    out, _ = ops.attention(q, k, v, H, SCALE)
    scale = float(out.float().abs().max()) / 300.0
    want = ops.quantize_fp8(out.view(-1, H * 64), scale)
    got = ops.attention_q8(q, k, v, H, SCALE, scale).view(-1, H * 64)
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


# ------------------------------------------------------------------------------------------------ backward
# family, B, H, Tq, Tk, masked, causal, causal_shift, dropout p
BWD = [
    ("needle", 1, 1, 1089, 145, False, False, None, 0.0),      # attn_bwd_dq2_kernel<4, 0>; two key blocks, the second with 17 keys
    ("gauss", 2, 2, 70, 129, False, False, None, 0.0),
    ("needle", 1, 2, 97, 128, False, False, None, 0.0),
    ("needle", 1, 2, 65, 161, False, False, None, 0.0),
    ("ramp", 1, 1, 129, 160, False, False, None, 0.0),
    ("ramp_down", 1, 1, 33, 127, False, False, None, 0.0),
    ("needle", 3, 2, 65, 97, True, True, None, 0.1),
    ("gauss", 1, 2, 129, 145, False, False, None, 0.1),
    ("needle", 3, 2, 33, 127, True, False, None, 0.0),
    ("needle", 3, 2, 64, 145, True, True, None, 0.0),
    ("needle", 3, 2, 129, 145, True, True, 5, 0.0),
    ("ramp", 3, 1, 130, 130, True, True, 0, 0.0),
    ("needle", 1, 2, 128, 128, False, True, 0, 0.0),
]


def run_backward(ops, case, ver, strided=True):
    family, B, H, Tq, Tk, masked, causal, shift, pdrop = case
    shift = Tk - Tq if shift is None else shift
    D = H * 64
    c = tiled_case(family, B, H, Tq, Tk, masked, causal, shift)
    check_coverage(c, B, H, Tq, Tk, masked)
    drop = drop_args(pdrop)
    fac = dropout_factor(ops, drop, B, H, Tq, Tk)
    fw = R.forward(c["q"], c["k"], c["v"], H, SCALE, c["vis"], fac=fac)
    o16, lse32, do16 = torch.as_tensor(fw["O"]).to(BF), torch.as_tensor(fw["LSE"]).float(), R.grad_output(B, Tq, D, seed=Tq)
    ref = R.backward(c["q"], c["k"], c["v"], o16, do16, lse32, H, SCALE, c["vis"], fac=fac)
    q, k, v, o, do = embed(c["q"]), embed(c["k"]), embed(c["v"]), embed(o16), embed(do16)
    kpm = c["kpm"].cuda() if masked else None
    gq, gk, gv = guarded_like(B, Tq, D), guarded_like(B, Tk, D), guarded_like(B, Tk, D)
    try:
        ops.attention_config(0, ver)
        ops.attention_bwd(q, k, v, o, do, lse32.cuda(), H, SCALE, kpm=kpm, causal=causal, causal_shift=shift, drop=drop,
                          dq_out=gq.view, dk_out=gk.view, dv_out=gv.view)
        if not strided:
            plain = ops.attention_bwd(q, k, v, o, do, lse32.cuda(), H, SCALE, kpm=kpm, causal=causal, causal_shift=shift, drop=drop)
    finally:
        ops.attention_config(0, 2)
    what = f"attention_bwd v{ver} {family} B{B} H{H} {Tq}x{Tk}{' kpm' if masked else ''}{f' causal{shift:+d}' if causal else ''}{' drop' if pdrop else ''}"
    for name, g in (("dq", gq), ("dk", gk), ("dv", gv)):
        g.check(f"{what} {name}")
        finite(g.view, f"{what} {name}")
        bracket(g.view, ref[name], ref["tol_" + name], f"{what} {name}", f"backward v{ver} {name}")
    if not strided:
        for got, g in zip(plain, (gq, gk, gv)):
            assert got.is_contiguous() and torch.equal(got, g.view)


@pytest.mark.parametrize("case", BWD, ids=lambda c: "-".join(str(x) for x in c))
def test_attention_backward(ops, case):
    """attn_bwd_dq_kernel / attn_bwd_dq2_kernel<4, 0> and attn_bwd_dkdv_kernel<4>, fed the reference's context (as bf16) and LSE (as fp32), writing
    strided dQ / dK / dV: each element within the bound of attention_ref.backward and the bf16 bracket."""
    run_backward(ops, case, 2)


@pytest.mark.parametrize("case", [BWD[0], BWD[6]], ids=lambda c: "-".join(str(x) for x in c))
def test_attention_backward_first_generation_and_contiguous_outputs(ops, case):
    """attention_config(., 1): attn_bwd_dq_kernel also for unmasked Tq > 1024; contiguous outputs are bit-equal to the strided ones"""
    run_backward(ops, case, 1, strided=False)


# ------------------------------------------------------------------------------------------------ rows without a visible key
@pytest.mark.parametrize("family", ["gauss", "needle"])
def test_rows_without_a_visible_key(ops, family):
    """One image with every key padded (module docstring): the forward attends uniformly to all keys (context = mean of V, within the bounds),
    the backward gives those rows no gradient: dQ of the image is zero, dK and dV of the image are zero."""
    B, H, Tq, Tk, D = 3, 2, 33, 97, 128
    kpm = R.make_kpm(B, Tk, half=False)
    kpm[1, :] = 0
    c = R.make_inputs(family, B, H, Tq, Tk, kpm, poison=True, seed=4)
    q, k, v = embed(c["q"]), embed(c["k"]), embed(c["v"])
    out = guarded_like(B, Tq, D)
    _, lse = ops.attention(q, k, v, H, SCALE, kpm=kpm.cuda(), need_lse=True, out=out.view)
    fw = R.forward(c["q"], c["k"], c["v"], H, SCALE, c["vis"])
    what = f"all keys of image 1 masked, {family}"
    out.check(what), finite(out.view, what), finite(lse, what)
    uniform = R.heads64(c["v"], H)[1].mean(1)                                                    # [H, 64]
    assert np.allclose(fw["O"][1].reshape(Tq, H, 64), uniform[None], rtol=0, atol=1e-12)
    bracket(out.view, fw["O"], fw["tol_O"], what + " context", "forward v2 context")
    assert_f32_bound(lse, fw["LSE"], fw["tol_LSE"].ravel(), 4, what + " LSE")
    o16, lse32, do16 = torch.as_tensor(fw["O"]).to(BF), torch.as_tensor(fw["LSE"]).float(), R.grad_output(B, Tq, D)
    ref = R.backward(c["q"], c["k"], c["v"], o16, do16, lse32, H, SCALE, c["vis"])
    gq, gk, gv = guarded_like(B, Tq, D), guarded_like(B, Tk, D), guarded_like(B, Tk, D)
    ops.attention_bwd(q, k, v, embed(o16), embed(do16), lse32.cuda(), H, SCALE, kpm=kpm.cuda(), dq_out=gq.view, dk_out=gk.view, dv_out=gv.view)
    for name, g in (("dq", gq), ("dk", gk), ("dv", gv)):
        g.check(f"{what} {name}")
        assert float(g.view[1].float().abs().max()) == 0.0, f"{what}: {name} of the masked image is not zero"
        bracket(g.view, ref[name], ref["tol_" + name], f"{what} {name}", f"backward v2 {name}")


# ------------------------------------------------------------------------------------------------ the helper itself
def test_reference_agrees_with_autograd_of_the_fp32_reference():
    from test_kernels_gpu import ref_attention
    B, H, Tq, Tk = 3, 2, 40, 97
    kpm = R.make_kpm(B, Tk)
    c = R.make_inputs("gauss", B, H, Tq, Tk, kpm, True, Tk - Tq, seed=2)
    fw = R.forward(c["q"], c["k"], c["v"], H, SCALE, c["vis"])
    qr, kr, vr = (c[n].float().requires_grad_(True) for n in "qkv")
    o, lse = ref_attention(qr, kr, vr, H, SCALE, kpm, True, Tk - Tq)
    do = R.grad_output(B, Tq, H * 64)
    o.backward(do.float())
    assert np.abs(o.detach().numpy() - fw["O"]).max() < 1e-5 and np.abs(lse.detach().numpy() - fw["LSE"]).max() < 1e-5
    bw = R.backward(c["q"], c["k"], c["v"], torch.as_tensor(fw["O"]).to(BF), do, torch.as_tensor(fw["LSE"]).float(), H, SCALE, c["vis"])
    for name, t in (("dq", qr), ("dk", kr), ("dv", vr)):
        # the helper takes Delta from the bf16-rounded context, as the kernels do: 2^-9 relative on O, i.e. about 1e-2 absolute on a gradient here
        assert np.abs(t.grad.numpy() - bw[name]).max() < 3e-2 * max(1.0, np.abs(bw[name]).max()), name


# ------------------------------------------------------------------------------------------------ single-query decode kernel
# family, Bkv, share, Tk, wg_keys, head_major, mask form (None | bytes | bytes8 = rows 8-byte aligned | bits), dropout p
DEC = [
    ("gauss", 1, 1, 1, 0, False, None, 0.0),
    ("needle", 3, 2, 7, 0, False, "bytes", 0.0),
    ("needle", 3, 4, 31, 0, True, "bits", 0.0),
    ("needle", 3, 1, 33, 0, False, "bits", 0.0),
    ("needle", 3, 2, 33, 0, False, "bytes8", 0.0),
    ("ramp", 3, 2, 261, 0, False, "bytes8", 0.0),
    ("needle", 3, 4, 261, 0, False, "bytes", 0.0),
    ("needle", 3, 2, 261, 0, True, "bits", 0.1),
    ("needle", 3, 1, 1152, 0, False, "bits", 0.0),
    ("needle", 3, 2, 1152, -576, True, "bytes", 0.0),
    ("ramp", 3, 2, 1152, 576, False, "bits", 0.0),
    ("needle", 3, 1, 1152, 288, False, "bytes", 0.0),
    ("ramp_down", 3, 2, 1152, 256, False, "bytes8", 0.0),
    ("needle", 3, 4, 1152, 0, False, "bits", 0.0),
    ("needle", 3, 2, 72, -576, False, "bytes", 0.0),
    ("needle", 3, 1, 300, 256, True, "bits", 0.0),
    ("ramp", 3, 2, 300, -256, False, "bytes", 0.0),
    ("needle", 1, 2, 1152, 0, False, None, 0.0),
]


def decode_inputs(family, Bkv, share, H, Tk, masked):
    kpm = R.make_kpm(Bkv, Tk) if masked else None
    c = R.make_inputs(family, Bkv, H, 1, Tk, kpm, poison=masked, seed=share, Bq=Bkv * share)
    c["kpm"] = kpm
    return c


def mask_forms(ops, kpm, form):
    """-> (kpm bytes | None, kpm_bits | None) on the GPU"""
    if form is None:
        return None, None
    Bkv, Tk = kpm.shape
    if form == "bytes":                                               # rows at odd addresses inside a wider buffer
        buf = torch.full((Bkv, Tk + 5), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[:, 3:3 + Tk]
        view.copy_(kpm)
        return view, None
    if form == "bytes8":                                              # 8-byte aligned rows, the bytes behind a row differ from its last key
        ld = (Tk + 7) // 8 * 8 + 8
        buf = torch.full((Bkv, ld), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[:, :Tk]
        view.copy_(kpm)
        return view, None
    words = (Tk + 31) // 32
    packed = ops.pack_mask_bits(kpm.cuda())
    want = np.zeros((Bkv, words), np.uint32)
    kn = kpm.numpy() != 0
    for j in range(Tk):
        want[:, j // 32] |= kn[:, j].astype(np.uint32) << np.uint32(j % 32)
    assert np.array_equal(packed.cpu().numpy().view(np.uint32), want), "pack_mask_bits"
    bits = torch.full((Bkv + 2, words + 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")      # the words as rows of a wider buffer
    view = bits[1:1 + Bkv, 1:1 + words]
    view.copy_(packed)
    return None, view


@pytest.mark.parametrize("case", DEC, ids=lambda c: "-".join(str(x) for x in c))
def test_attention_decode(ops, case):
    """attn_decode_kernel (+ attn_decode_merge_kernel): the probabilities stay in fp32, so the context lies within 2 eta * sum_j p f |v| and the bf16
    bracket; every workgroup geometry, K/V layout and mask form; the decode-activation-layout output is bit-equal to the row-major one."""
    family, Bkv, share, Tk, wg, head_major, form, pdrop = case
    H, D, Bq = 3, 192, Bkv * share
    c = decode_inputs(family, Bkv, share, H, Tk, form is not None)
    check_coverage(c, Bq, H, 1, Tk, form is not None)
    q, k, v = embed(c["q"])[:, 0], embed(c["k"]), embed(c["v"])
    if head_major:
        k, v = (t.reshape(Bkv, Tk, H, 64).permute(0, 2, 1, 3).contiguous() for t in (k, v))
    kb, bits = mask_forms(ops, c["kpm"], form)
    drop = drop_args(pdrop)
    if drop is not None:
        drop = drop[:3] + (33,)
    fac = None if drop is None else ops.dropout_mask(Bq * H, Tk, pdrop, drop[1], drop[2], 1, 33, factor=True).view(Bq, H, 1, Tk).cpu().double().numpy()
    out = Guarded.rows(Bq, D, BF, ld=D + 16)
    ops.attention_decode(q, k, v, H, SCALE, kpm=kb, kpm_bits=bits, out=out.view, drop=drop, head_major=head_major, wg_keys=wg)
    what = f"attention_decode {family} Bkv{Bkv} x{share} Tk{Tk} wg{wg}{' head-major' if head_major else ''} {form}{' drop' if pdrop else ''}"
    out.check(what), finite(out.view, what)
    ref = R.forward(c["q"], c["k"], c["v"], H, SCALE, c["vis"], fac=fac, mfma=False, share=share)
    bracket(out.view, ref["O"][:, 0], ref["tol_O"][:, 0], what, "decode", fp32_only=True)
    if Bq <= 64:
        dal = ops.attention_decode(q, k, v, H, SCALE, kpm=kb, kpm_bits=bits, drop=drop, head_major=head_major, wg_keys=wg, out_dal=True)
        assert torch.equal(ops.dec_from_dal(dal, Bq, D), out.view)


# ------------------------------------------------------------------------------------------------ cross-attention on the matrix cores
# family, Bkv, share, Tk, masked, dropout p. Key blocks of 32: <= 12 -> <1>, <= 24 -> <2>, <= 36 -> <3>, <= 60 -> <5, true>, more -> splits + merge
CROSS = [
    ("needle", 3, 1, 384, True, 0.0),
    ("needle", 3, 2, 416, True, 0.1),
    ("ramp", 3, 4, 768, True, 0.0),
    ("needle", 3, 2, 800, False, 0.0),
    ("needle", 3, 4, 1152, True, 0.1),
    ("ramp_down", 3, 1, 1184, True, 0.0),
    ("needle", 3, 2, 1920, True, 0.0),
    ("needle", 3, 4, 1952, True, 0.1),
    ("gauss", 3, 2, 1152, True, 0.0),
    ("ramp", 1, 1, 1952, False, 0.0),
]


@pytest.mark.parametrize("case", CROSS, ids=lambda c: "-".join(str(x) for x in c))
def test_attention_cross_mfma(ops, case):
    """attn_cross_mfma_kernel<1 | 2 | 3> and <5, true>, the split + merge form: context within (2^-8 + 2 eta) * sum_j p f |v| and the bf16 bracket;
    single masked keys at every 32-bit word edge; K / V packed from strided views; decode-activation-layout output bit-equal."""
    family, Bkv, share, Tk, masked, pdrop = case
    H, D, Bq = 3, 192, Bkv * share
    c = decode_inputs(family, Bkv, share, H, Tk, masked)
    check_coverage(c, Bq, H, 1, Tk, masked)
    q, k, v = embed(c["q"])[:, 0], embed(c["k"]), embed(c["v"])
    bits = mask_forms(ops, c["kpm"], "bits")[1] if masked else None
    pk = ops.pack_cross_kv(k, v, H)
    drop = drop_args(pdrop)
    if drop is not None:
        drop = drop[:3] + (9,)
    fac = None if drop is None else ops.dropout_mask(Bq * H, Tk, pdrop, drop[1], drop[2], 1, 9, factor=True).view(Bq, H, 1, Tk).cpu().double().numpy()
    out = Guarded.rows(Bq, D, BF, ld=D + 16)
    ops.attention_cross_mfma(q, pk, Bkv, Tk, H, SCALE, kpm_bits=bits, out=out.view, drop=drop)
    what = f"attention_cross_mfma {family} Bkv{Bkv} x{share} Tk{Tk}{' bits' if masked else ''}{' drop' if pdrop else ''}"
    out.check(what), finite(out.view, what)
    ref = R.forward(c["q"], c["k"], c["v"], H, SCALE, c["vis"], fac=fac, share=share)
    bracket(out.view, ref["O"][:, 0], ref["tol_O"][:, 0], what, "cross mfma")
    dal = ops.attention_cross_mfma(q, pk, Bkv, Tk, H, SCALE, kpm_bits=bits, drop=drop, out_dal=True)
    assert torch.equal(ops.dec_from_dal(dal, Bq, D), out.view)


# family, Bkv, share, Tk, masked, dropout p: <1, false, true> (<= 12 blocks), <2, ..>, <3, ..>, <5, true, true>
CROSS_Q = [
    ("needle", 3, 1, 384, True, 0.0),
    ("needle", 3, 2, 416, True, 0.1),
    ("ramp", 3, 4, 768, True, 0.0),
    ("needle", 3, 2, 800, False, 0.0),
    ("needle", 3, 4, 1152, True, 0.1),
    ("needle", 3, 1, 1184, True, 0.0),
    ("gauss", 3, 2, 1920, True, 0.0),
]


@pytest.mark.parametrize("case", CROSS_Q, ids=lambda c: "-".join(str(x) for x in c))
def test_attention_cross_mfma_with_the_query_projection(ops, case):
    """attention_cross_mfma_q against the float64 chain LayerNorm -> query Linear -> attention. The hidden rows are built so that the projected
    query is (about) the family's query: W = a permutation plus small dense noise, gamma = powers of two (the folded weight stays exact), so the
    only new rounding is that of the projected query to bf16; attention_ref.project_query bounds it and forward() turns it into expm1(2 eps_q) A."""
    family, Bkv, share, Tk, masked, pdrop = case
    H, D, Bq = 12, 768, Bkv * share
    c = decode_inputs(family, Bkv, share, H, Tk, masked)
    g = torch.Generator().manual_seed(Tk)
    perm = torch.randperm(D, generator=g)
    w = (0.01 * torch.randn(D, D, generator=g))
    w[torch.arange(D), perm] += 1.0
    w = w.to(BF)
    gamma = 2.0 ** torch.randint(-1, 2, (D,), generator=g).float()
    beta, bias = 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    raw = (c["q"][:, 0].float()[:, torch.argsort(perm)] / gamma).to(BF)              # W diag(gamma) raw ~ the family's query, before the LayerNorm
    q64, q_err = R.project_query(raw, w, gamma, beta, bias, 1e-12)
    k, v = embed(c["k"]), embed(c["v"])
    bits = mask_forms(ops, c["kpm"], "bits")[1] if masked else None
    pk = ops.pack_cross_kv(k, v, H)
    x_dal, st = ops.dec_to_dal(raw.cuda(), want_stats=True)
    wf, bcf = ops.dec_pack_weight(w.cuda(), gamma.cuda(), beta.cuda(), bias.cuda())
    drop = drop_args(pdrop)
    if drop is not None:
        drop = drop[:3] + (5,)
    fac = None if drop is None else ops.dropout_mask(Bq * H, Tk, pdrop, drop[1], drop[2], 1, 5, factor=True).view(Bq, H, 1, Tk).cpu().double().numpy()
    out = Guarded.rows(Bq, D, BF, ld=D + 16)
    ops.attention_cross_mfma_q(x_dal, Bq, st, 1e-12, wf, bcf, pk, Bkv, Tk, H, SCALE, kpm_bits=bits, out=out.view, drop=drop, out_dal=False)
    what = f"attention_cross_mfma_q {family} Bkv{Bkv} x{share} Tk{Tk}{' bits' if masked else ''}{' drop' if pdrop else ''}"
    out.check(what), finite(out.view, what)
    ref = R.forward(torch.as_tensor(q64)[:, None], c["k"], c["v"], H, SCALE, c["vis"], fac=fac, share=share, q_err=q_err[:, None])
    bracket(out.view, ref["O"][:, 0], ref["tol_O"][:, 0], what, "cross mfma, query projection")
    dal = ops.attention_cross_mfma_q(x_dal, Bq, st, 1e-12, wf, bcf, pk, Bkv, Tk, H, SCALE, kpm_bits=bits, drop=drop, out_dal=True)
    assert torch.equal(ops.dec_from_dal(dal, Bq, D), out.view)


def test_no_bound_is_loose():
    """Runs last: over the cases of this session, the worst figure of every kernel is at least 0.02 of its bound (each case has already asserted
    that it is below 1). A bound that no case comes near would not be worth having."""
    for kernel, values in sorted(FIGURES.items()):
        print(f"MEASURED worst of {len(values)} cases, {kernel}: {max(values):.4f}")
    loose = {k: max(v) for k, v in FIGURES.items() if max(v) < 0.02}
    assert not loose, f"bounds nobody comes near: {loose}"
