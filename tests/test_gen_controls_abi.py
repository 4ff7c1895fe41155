"""CPU: the C ABI of the generation-control entry points (csrc/logits_proc.hip, the log-prob beam step in csrc/decode.hip). The library's export
check (test_cpu_host.py) then covers the built symbols; these pin the declarations and the argument types the ctypes binding derives from them."""
import ctypes

import pytest
import torch

from cxrmate_amd._lib import CxrError, parse_header


def test_header_declares_logits_process_with_parsable_arguments():
    protos = parse_header()
    assert "cxr_logits_process_f32" in protos
    args = protos["cxr_logits_process_f32"]
    assert [n for _, n in args] == ["logits", "ld", "ids", "ids_ld", "R", "V", "cur", "eos", "penalty", "ngram", "min_length", "stream"]
    types = dict((n, t) for t, n in args)
    for n in ("logits", "ids", "stream"):
        assert types[n] is ctypes.c_void_p, n
    for n in ("ld", "ids_ld", "R", "eos"):
        assert types[n] is ctypes.c_long, n
    for n in ("V", "cur", "ngram", "min_length"):
        assert types[n] is ctypes.c_int, n
    assert types["penalty"] is ctypes.c_float


def test_header_declares_logprob_beam_step_like_beam_step():
    protos = parse_header()
    assert "cxr_beam_step_lp" in protos and "cxr_beam_step" in protos
    lp, plain = protos["cxr_beam_step_lp"], protos["cxr_beam_step"]
    assert [t for t, _ in lp] == [t for t, _ in plain]
    assert [n for _, n in lp][1:] == [n for _, n in plain][1:] and lp[0][1] == "logprobs"


def test_wrappers_refuse_cpu_tensors():
    from cxrmate_amd import ops
    x = torch.zeros((2, 16), dtype=torch.float32)
    ids = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(CxrError, match="no CPU path"):
        ops.logits_process_(x, ids, 4, eos=2, penalty=1.3, ngram=2, min_length=6)
    nb, B, L = 2, 1, 4
    with pytest.raises(CxrError, match="no CPU path"):
        ops.beam_step(x, torch.zeros((nb, B, L), dtype=torch.int64), torch.zeros((nb, B, L), dtype=torch.int64), torch.zeros((B, nb)),
                      torch.zeros((B, nb)), torch.zeros((B, nb), dtype=torch.uint8), torch.ones((2, B), dtype=torch.int32),
                      torch.zeros((2, B), dtype=torch.int32), torch.zeros(nb * B, dtype=torch.int64), 1, 4, 2, 1.0,
                      ws=torch.zeros(64), logprobs=True)


def test_logits_process_refuses_long_histories():
    from cxrmate_amd import ops
    x = torch.zeros((1, 16), dtype=torch.float32)
    ids = torch.zeros((1, 600), dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.logits_process_(x, ids, 513, ngram=2)
