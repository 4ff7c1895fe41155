"""CPU: the minimax GELU of every GEMM epilogue (csrc/common.h, CXR_GELU_A1/A3/A5) against the exact erf GELU, in float64, with the constants
read from the header the kernels are compiled from. The documented bounds are 2.52e-5 on the value and 1.099e-4 on the derivative."""
import math
import os
import re

import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cxrmate_amd", "csrc", "common.h")


def gelu_constants():
    text = open(HEADER).read()
    out = {}
    for name in ("A1", "A3", "A5"):
        m = re.search(r"#define\s+CXR_GELU_" + name + r"\s+\(?\s*([-+0-9.eE]+)f\s*\)?", text)
        assert m, f"CXR_GELU_{name} not found in {HEADER}"
        out[name] = float(m.group(1))
    return out


def gelu_approx(x, c):
    """The header's formula in float64: Phi ~ sigmoid(x p(xc^2)), xc = clamp(x, +-8); derivative s (1 + xc (1 - s) p'(xc)), p' = d(xc p)/dxc."""
    xc = x.clamp(-8.0, 8.0)
    x2 = xc * xc
    s = torch.sigmoid(x * (c["A1"] + x2 * (c["A3"] + x2 * c["A5"])))
    dp = c["A1"] + x2 * (3.0 * c["A3"] + x2 * 5.0 * c["A5"])
    return x * s, s * (1.0 + xc * (1.0 - s) * dp)


def gelu_exact(x):
    phi = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    return x * phi, phi + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def test_gelu_constants_meet_the_documented_bounds():
    c = gelu_constants()
    x = torch.linspace(-12.0, 12.0, 2_400_001, dtype=torch.float64)
    # plus the tails the epilogues see: every bf16 magnitude out to the top of the range
    big = torch.logspace(1, 38.5, 4000, dtype=torch.float64)
    x = torch.cat([x, big, -big])
    v, d = gelu_approx(x, c)
    rv, rd = gelu_exact(x)
    ev, ed = float((v - rv).abs().max()), float((d - rd).abs().max())
    assert ev <= 2.52e-5, f"value error {ev:.4e} at x = {float(x[(v - rv).abs().argmax()]):.6g}"
    assert ed <= 1.099e-4, f"derivative error {ed:.4e} at x = {float(x[(d - rd).abs().argmax()]):.6g}"
    # and the bounds are tight (a constant changed in its third significant digit breaks them)
    assert ev > 2.4e-5 and ed > 1.0e-4, (ev, ed)
