"""CPU: the C ABI of the decode-step map / hidden-state entry points (csrc/attn_decode_probs.hip), the Record / StepPlan keys of the step graphs
and the resolution of output_attentions / output_hidden_states from keywords and a GenerationConfig."""
import ctypes

import pytest
import torch

from cxrmate_amd._lib import CxrError, parse_header
from cxrmate_amd.generation import GENERATION_DEFAULTS, UNSET, Controls, Record, StepPlan, resolve_generation_options


def test_header_declares_decode_probs_with_parsable_arguments():
    protos = parse_header()
    assert "cxr_attn_decode_probs_f32" in protos
    args = protos["cxr_attn_decode_probs_f32"]
    assert [n for _, n in args] == ["Q", "K", "kpm", "P", "q_bs", "k_bs", "k_rs", "kpm_bs", "p_bs", "p_hs", "p_ks", "B", "H", "Tk", "scale", "kv_share",
                                    "kpm_bits", "drop_p", "drop_seed", "drop_site", "drop_t", "row_groups", "stream"]
    types = dict((n, t) for t, n in args)
    for n in ("Q", "K", "kpm", "P", "drop_seed", "stream"):
        assert types[n] is ctypes.c_void_p, n
    for n in ("q_bs", "k_bs", "k_rs", "kpm_bs", "p_bs", "p_hs", "p_ks"):
        assert types[n] is ctypes.c_long, n
    for n in ("B", "H", "Tk", "kv_share", "kpm_bits", "drop_t", "row_groups"):
        assert types[n] is ctypes.c_int, n
    assert types["scale"] is ctypes.c_float and types["drop_p"] is ctypes.c_float and types["drop_site"] is ctypes.c_uint


def test_header_declares_hidden_record_with_parsable_arguments():
    protos = parse_header()
    assert "cxr_dec_hidden_record_f32" in protos
    args = protos["cxr_dec_hidden_record_f32"]
    assert [n for _, n in args] == ["x", "x_mt", "M", "K", "gamma", "beta", "eps", "out", "o_rs", "row_groups", "stream"]
    types = dict((n, t) for t, n in args)
    for n in ("x", "gamma", "beta", "out", "stream"):
        assert types[n] is ctypes.c_void_p, n
    for n in ("x_mt", "M", "K", "row_groups"):
        assert types[n] is ctypes.c_int, n
    assert types["o_rs"] is ctypes.c_long and types["eps"] is ctypes.c_float


def test_wrappers_refuse_cpu_tensors():
    from cxrmate_amd import ops
    q = torch.zeros((4, 768), dtype=torch.bfloat16)
    k = torch.zeros((2, 9, 768), dtype=torch.bfloat16)
    with pytest.raises(CxrError, match="no CPU path"):
        ops.attention_decode_probs(q, k, 12, 0.125, out=torch.zeros((4, 12, 1, 9)), row_groups=2)
    with pytest.raises(CxrError, match="no CPU path"):
        ops.dec_hidden_record(torch.zeros((16, 768), dtype=torch.bfloat16), 4, torch.ones(768), torch.zeros(768), 1e-12, out=torch.zeros((4, 768)))


def _plan(record):
    return StepPlan(kind="greedy", special=(3,), mask_token_id=None, bos=1, eos=2, pad=4, max_length=16, train=False, controls=Controls(), record=record)


def test_record_flags_key_the_step_plans():
    plans = [_plan(Record()), _plan(Record(attentions=True)), _plan(Record(hidden=True)), _plan(Record(attentions=True, hidden=True)),
             _plan(Record(attentions=True, row_groups=4))]
    assert len({hash(p) for p in plans}) == len(plans) == len(set(plans))
    for i, a in enumerate(plans):
        for b in plans[i + 1:]:
            assert a != b
    assert _plan(Record(attentions=True)) == plans[1] and _plan(Record(False, False, 1)) == plans[0]


def test_record_on_keeps_its_meaning():
    assert not Record().on and not Record(attentions=True).on and not Record(hidden=True).on and not Record(attentions=True, hidden=True).on
    assert Record(logits=True).on and Record(scores=True).on and Record(True, False, 4, True, True).on
    assert Record() == (False, False, 1, False, False)            # the two flags follow the fields of before, both off by default
    assert Record(attentions=True).maps and Record(hidden=True).maps and not Record(True, True).maps
    assert Record(hidden=True).any and Record(scores=True).any and not Record().any


def test_options_come_from_keywords_and_generation_config():
    from transformers import GenerationConfig
    assert GENERATION_DEFAULTS["output_attentions"] is False and GENERATION_DEFAULTS["output_hidden_states"] is False
    o = resolve_generation_options({})
    assert o["output_attentions"] is False and o["output_hidden_states"] is False
    o = resolve_generation_options(dict(output_attentions=True, output_hidden_states=UNSET))
    assert o["output_attentions"] is True and o["output_hidden_states"] is False
    gc = GenerationConfig(output_attentions=True, output_hidden_states=True, return_dict_in_generate=True)
    o = resolve_generation_options({}, gc)
    assert o["output_attentions"] is True and o["output_hidden_states"] is True and o["return_dict_in_generate"] is True
    # a keyword the caller passed wins, even when it equals the default
    o = resolve_generation_options(dict(output_attentions=False, output_hidden_states=UNSET), gc)
    assert o["output_attentions"] is False and o["output_hidden_states"] is True
