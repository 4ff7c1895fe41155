"""CPU: the C ABI of the patch-embedding data gradient (pixel_values.grad) and the argument checks of its wrapper. The library's export check
(test_cpu_host.py) covers the built symbol; these pin the declaration and the argument types the ctypes binding derives from it."""
import ctypes

import pytest
import torch

from cxrmate_amd._lib import CxrError, parse_header


def test_header_declares_patch_embed_dgrad_with_parsable_arguments():
    protos = parse_header()
    assert "cxr_patch_embed_dgrad_f32" in protos
    args = protos["cxr_patch_embed_dgrad_f32"]
    assert [n for _, n in args] == ["de", "w", "dpx", "Bn", "Cin", "H", "W", "Co", "ks", "stride", "pad", "Ho", "Wo", "kpad", "stream"]
    types = dict((n, t) for t, n in args)
    for n in ("de", "w", "dpx", "stream"):
        assert types[n] is ctypes.c_void_p, n
    for n in ("Bn", "Cin", "H", "W", "Co", "ks", "stride", "pad", "Ho", "Wo", "kpad"):
        assert types[n] is ctypes.c_int, n


def _operands(rows=2 * 24 * 24, Co=64, kpad=192):
    return torch.zeros((rows, Co), dtype=torch.bfloat16), torch.zeros((Co, kpad), dtype=torch.bfloat16)


def test_wrapper_refuses_cpu_tensors():
    from cxrmate_amd import ops
    de, w = _operands()
    with pytest.raises(CxrError, match="no CPU path"):
        ops.patch_embed_dgrad(de, w, 2, 96, 96, 7, 4, 2)


def test_wrapper_refuses_misshaped_operands():
    from cxrmate_amd import ops
    de, w = _operands()
    with pytest.raises(ValueError):
        ops.patch_embed_dgrad(de[:-1], w, 2, 96, 96, 7, 4, 2)          # one row short of Bn * Ho * Wo
    with pytest.raises(ValueError):
        ops.patch_embed_dgrad(de, w, 2, 96, 100, 7, 4, 2)               # Wo = 25: another row count
    with pytest.raises(AssertionError):
        ops.patch_embed_dgrad(de.float(), w, 2, 96, 96, 7, 4, 2)        # dtype
    with pytest.raises(AssertionError):
        ops.patch_embed_dgrad(de, w[:, :128], 2, 96, 96, 7, 4, 2)       # fewer than 3 * 7 * 7 columns (and not contiguous)
