"""Shared helpers of the GPU kernel tests: sentinel-guarded output buffers and elementwise bounds derived from the output's rounding."""
import numpy as np
import torch

BF = torch.bfloat16
F32 = torch.float32
I64 = torch.int64
PAD = 8                     # guard elements before a 1-D output (keeps 16-byte alignment for every element size used here)

# sentinel bit patterns (a NaN for the float types, so that a stray read-modify-write shows up as well)
_SENT = {BF: (torch.int16, -0x5A5B), F32: (torch.int32, 0x7FA5A5A5), I64: (I64, -0x5A5A5A5A5A5A5A5B), torch.uint8: (torch.uint8, 0xA5)}


class Guarded:
    """A buffer of `shape` filled with the sentinel of `dtype`; `view` = buf[index] is the output the call may write."""

    def __init__(self, shape, dtype, index):
        it, v = _SENT[dtype]
        self.dtype = dtype
        self.buf = torch.empty(shape, dtype=dtype, device="cuda")
        self.buf.view(it).fill_(v)
        self.mask = torch.ones(shape, dtype=torch.bool, device="cuda")
        self.mask[index] = False
        self.view = self.buf[index]

    @classmethod
    def flat(cls, n, dtype):
        return cls((n + 2 * PAD,), dtype, (slice(PAD, PAD + n),))

    @classmethod
    def rows(cls, R, C, dtype, ld=None, extra_rows=2):
        """[R, C] rows inside an [R + 2 extra, ld] buffer (ld > C: gaps after every row)"""
        ld = ld or C
        return cls((R + 2 * extra_rows, ld), dtype, (slice(extra_rows, extra_rows + R), slice(0, C)))

    def check(self, what=""):
        torch.cuda.synchronize()
        it, v = _SENT[self.dtype]
        bad = int((self.buf.view(it)[self.mask] != v).sum())
        assert bad == 0, f"{what}: {bad} guard elements overwritten"


def bits(t):
    return t.contiguous().view({BF: torch.int16, F32: torch.int32}[t.dtype]).cpu()


def ulp32(x):
    """spacing of fp32 at |x| (float64 array)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def bf16_floor(v):
    """largest bf16 <= v (float64 array) -> float64"""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    f = np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)
    t = (f.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    down = t > f                                                     # negative and not representable: one bf16 step away from zero
    t = np.where(down, (t.view(np.uint32) + np.uint32(0x10000)).view(np.float32), t)
    return t.astype(np.float64)


def bf16_ceil(v):
    return -bf16_floor(-np.asarray(v, dtype=np.float64))


def assert_bf16_bracket(out, ref, tol, what):
    """out (bf16) lies between the bf16 value just below ref - tol and the bf16 value just above ref + tol. Returns the largest |out - ref| as a
    fraction of the bracket's half-width on that side."""
    o = out.float().cpu().double().numpy().ravel()
    r = np.asarray(ref, dtype=np.float64).ravel()
    tol = np.asarray(tol, dtype=np.float64)
    tol = tol.ravel() if tol.size == r.size else np.broadcast_to(tol, r.shape)
    lo, hi = bf16_floor(r - tol), bf16_ceil(r + tol)
    bad = ~((o >= lo) & (o <= hi))
    assert not bad.any(), f"{what}: {int(bad.sum())} outside the bf16 bracket, first at ref {r[bad][0]!r}: got {o[bad][0]!r}"
    return float(np.max(np.abs(o - r) / np.maximum(hi - r, r - lo)))


def assert_f32_bound(out, ref, tol, ulps, what):
    o = out.cpu().double().numpy().ravel()
    r = np.asarray(ref, dtype=np.float64).ravel()
    err = np.abs(o - r)
    lim = tol + ulps * ulp32(r)
    bad = ~(err <= lim)
    assert not bad.any(), f"{what}: {int(bad.sum())} beyond {tol} + {ulps} ulp, worst err {np.nanmax(err):.3e} at ref {r[np.nanargmax(err)]!r}"
    return float(err.max())


def all_bf16(finite=True):
    b = (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16).view(BF)
    return b[torch.isfinite(b.float())] if finite else b


def gelu64(x):
    """exact (erf) GELU and its derivative in float64"""
    x = torch.as_tensor(x, dtype=torch.float64)
    phi = 0.5 * torch.special.erfc(-x / np.sqrt(2.0))
    return (x * phi).numpy(), (phi + x * torch.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)).numpy()
