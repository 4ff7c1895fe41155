"""CPU: the C ABI of the attention-probability entry point (output_attentions). The library's export check (test_cpu_host.py) then covers
the built symbol; these pin the declaration itself and the argument types the ctypes binding derives from it."""
import ctypes

from cxrmate_amd._lib import parse_header


def test_header_declares_attn_probs_with_parsable_arguments():
    protos = parse_header()
    assert "cxr_attn_probs_f32" in protos
    args = protos["cxr_attn_probs_f32"]
    names = [n for _, n in args]
    assert names == ["Q", "K", "LSE", "kpm", "P", "q_bs", "q_rs", "k_bs", "k_rs", "kpm_bs", "p_bs", "p_hs", "p_rs", "B", "H", "Tq", "Tk",
                     "scale", "causal", "causal_shift", "drop_p", "drop_seed", "drop_site", "drop_t0", "stream"]
    types = dict((n, t) for t, n in args)
    for n in ("Q", "K", "LSE", "kpm", "P", "drop_seed", "stream"):
        assert types[n] is ctypes.c_void_p, n
    for n in ("q_bs", "q_rs", "k_bs", "k_rs", "kpm_bs", "p_bs", "p_hs", "p_rs"):
        assert types[n] is ctypes.c_long, n
    for n in ("B", "H", "Tq", "Tk", "causal", "causal_shift", "drop_t0"):
        assert types[n] is ctypes.c_int, n
    assert types["scale"] is ctypes.c_float and types["drop_p"] is ctypes.c_float and types["drop_site"] is ctypes.c_uint


def test_attention_probs_wrapper_refuses_cpu_tensors():
    import pytest
    import torch
    from cxrmate_amd import ops
    q = torch.zeros((1, 4, 768), dtype=torch.bfloat16)
    lse = torch.zeros((1, 12, 4), dtype=torch.float32)
    with pytest.raises(Exception):
        ops.attention_probs(q, q, lse, 12, 0.125)
