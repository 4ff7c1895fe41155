"""CPU: the C ABI of the token-constraint kernel (csrc/logits_proc.hip cxr_logits_constrain_f32) and of the early-stopping beam step (csrc/decode.hip
cxr_beam_step_es), the option validation of generate() (the library's messages), the merge of a generation_config object, and the CPU restatement
of the early-stopping beam search against the reference's recorded searches (tests/golden/gen_constraints.npz)."""
import ctypes
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gen_constraints_ref as ref
import golden_util as gu
from cxrmate_amd import generation as gen
from cxrmate_amd._lib import CxrError, parse_header


def test_header_declares_logits_constrain_with_parsable_arguments():
    protos = parse_header()
    assert "cxr_logits_constrain_f32" in protos
    args = protos["cxr_logits_constrain_f32"]
    old = protos["cxr_logits_process_f32"]
    assert args[:len(old) - 1] == old[:-1]                               # the arguments of cxr_logits_process_f32 come first, unchanged
    assert [n for _, n in args][len(old) - 1:] == ["seq_tok", "seq_off", "seq_bias", "n_bias", "n_seq", "forced", "n_forced_bos", "n_forced_eos",
                                                   "max_length", "suppress", "n_suppress", "begin_suppress", "n_begin", "begin_index", "stream"]
    types = dict((n, t) for t, n in args)
    for n in ("seq_tok", "seq_off", "seq_bias", "forced", "suppress", "begin_suppress", "stream"):
        assert types[n] is ctypes.c_void_p, n
    for n in ("n_bias", "n_seq", "n_forced_bos", "n_forced_eos", "max_length", "n_suppress", "n_begin", "begin_index"):
        assert types[n] is ctypes.c_int, n


def test_header_declares_early_stopping_beam_step():
    protos = parse_header()
    assert "cxr_beam_step_es" in protos
    es, idx = protos["cxr_beam_step_es"], protos["cxr_beam_step_idx"]
    names = [n for _, n in es]
    assert set(n for _, n in idx) <= set(names)                          # everything cxr_beam_step_idx takes ...
    assert [n for n in names if n not in set(m for _, m in idx)] == ["allfin", "div_run", "early_stopping"]      # ... and the three new ones
    types = dict((n, t) for t, n in es)
    assert types["allfin"] is ctypes.c_void_p and types["div_run"] is ctypes.c_float and types["early_stopping"] is ctypes.c_int
    for n, t in idx:
        assert types[t] is n, t


def test_wrappers_refuse_cpu_tensors():
    from cxrmate_amd import ops
    x = torch.zeros((2, 16), dtype=torch.float32)
    ids = torch.zeros((2, 4), dtype=torch.int64)
    tables = ops.ConstraintTables("cpu", sequence_bias=[((3,), 0.5), ((1, 3), -0.5)], bad_words=[(4,)], forced_eos=[2], suppress=[5], max_length=9)
    assert (tables.n_bias, tables.n_seq, tables.n_forced_bos, tables.n_forced_eos) == (2, 3, 0, 1)
    with pytest.raises(CxrError, match="no CPU path"):
        ops.logits_constrain_(x, ids, 4, eos=2, penalty=1.3, ngram=2, min_length=6, tables=tables)
    with pytest.raises(ValueError):
        ops.logits_constrain_(torch.zeros((1, 16)), torch.zeros((1, 600), dtype=torch.int64), 513, tables=tables)
    nb, B, L = 2, 1, 4
    with pytest.raises(CxrError, match="no CPU path"):
        ops.beam_step(x, torch.zeros((nb, B, L), dtype=torch.int64), torch.zeros((nb, B, L), dtype=torch.int64), torch.zeros((B, nb)),
                      torch.zeros((B, nb)), torch.zeros((B, nb), dtype=torch.uint8), torch.ones((2, B), dtype=torch.int32),
                      torch.zeros((2, B), dtype=torch.int32), torch.zeros(nb * B, dtype=torch.int64), 1, 4, 2, 1.0,
                      ws=torch.zeros(64), early=(1, 0.0, torch.zeros((2, B), dtype=torch.int32)))


def test_constraint_tables_sort_entries_stably_by_last_token():
    from cxrmate_amd import ops
    t = ops.ConstraintTables("cpu", sequence_bias=[((7, 6), 1.0), ((9,), 2.0), ((5, 6), 3.0), ((6,), 4.0), ((1, 2, 9), 5.0)], bad_words=[(8, 3), (3,)])
    off = t.seq_off.tolist()
    entries = [tuple(t.seq_tok[off[i]:off[i + 1]].tolist()) for i in range(t.n_seq)]
    # per group: by last id; a token's length-1 entry first, then its multi-token entries in the caller's order
    assert entries == [(6,), (7, 6), (5, 6), (9,), (1, 2, 9), (3,), (8, 3)]
    assert t.seq_bias.tolist() == [4.0, 1.0, 3.0, 2.0, 5.0, float("-inf"), float("-inf")]


# ------------------------------------------------------------------------------------------------ validation (the library's messages)
def cons(**kw):
    return gen.token_constraints(1000, gu.EOS, 1, 20, **kw)


def test_validation_errors_carry_the_librarys_messages():
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor, SequenceBiasLogitsProcessor
    for bad in ([], "x", [[1], 3], [[-1]], [[1.5]]):
        with pytest.raises(ValueError) as want:
            NoBadWordsLogitsProcessor(bad, gu.EOS)
        with pytest.raises(ValueError) as got:
            cons(bad_words_ids=bad)
        assert str(got.value) == str(want.value), bad
    for bad in ({}, [], "x", {(1,): 1}, {1: 0.5}, {(): 0.5}, {(-2,): 0.5}, [[[1], 1]], [[[0], 0.5]], [[1, 0.5]]):
        with pytest.raises(ValueError) as want:
            SequenceBiasLogitsProcessor(bad)
        with pytest.raises(ValueError) as got:
            cons(sequence_bias=bad)
        assert str(got.value) == str(want.value), bad
    with pytest.raises(ValueError, match="non-empty list of lists"):     # (the library lets an empty id list through and fails at its first step)
        cons(sequence_bias=[[[], 0.5]])
    # an id outside the vocabulary: the library raises at its first step, the engine before decoding, with the same words
    x, ids = torch.zeros((1, 1000)), torch.zeros((1, 3), dtype=torch.int64)
    for kw, proc in ((dict(sequence_bias={(5, 1000): 0.5}), SequenceBiasLogitsProcessor({(5, 1000): 0.5})),
                     (dict(bad_words_ids=[[1], [7, 2000]]), NoBadWordsLogitsProcessor([[1], [7, 2000]], gu.EOS))):
        with pytest.raises(ValueError) as want:
            proc(ids, x)
        with pytest.raises(ValueError) as got:
            cons(**kw)
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError):                                      # only [eos] entries: nothing is left to ban (library: empty table)
        cons(bad_words_ids=[[gu.EOS]])
    with pytest.raises(ValueError, match="forced"):
        cons(forced_eos_token_id=1000)
    with pytest.raises(ValueError, match="early_stopping"):
        gen.early_stopping_mode("always", 1.0)
    assert [gen.early_stopping_mode(v, 2.0) for v in (False, None, True, "never")] == [0, 0, 1, 2]
    assert gen.early_stopping_mode("never", 0.0) == 0                    # "never" differs from False under a positive length penalty only


def test_token_constraints_description():
    assert cons() is None
    c = cons(sequence_bias=[[[5, 6], 0.5], [[7], -1.0], [[5, 6], 0.25]], bad_words_ids=[[gu.EOS], [3, gu.EOS], [9]], suppress_tokens=[4, 4, 2000],
             begin_suppress_tokens=[8], forced_bos_token_id=6, forced_eos_token_id=[gu.EOS, 7])
    bias, bad, fbos, feos, sup, begin, max_length, begin_index = c
    assert bias == (((5, 6), 0.25), ((7,), -1.0))                        # the library's dict: first position, last value
    assert bad == ((3, gu.EOS), (9,))                                    # the [eos] single is dropped, a word ending in EOS is kept
    assert (fbos, feos, sup, begin, max_length) == (6, (gu.EOS, 7), (4, 4, 2000), (8,), 20)
    assert begin_index == 2                                              # prompt of length 1 and forced_bos set: one later (utils.py:1278-1283)
    assert gen.token_constraints(1000, gu.EOS, 1, 20, begin_suppress_tokens=[8])[-1] == 1
    assert gen.token_constraints(1000, gu.EOS, 6, 20, begin_suppress_tokens=[8], forced_bos_token_id=6)[-1] == 6
    hash(c)


# ------------------------------------------------------------------------------------------------ the step plan (graph cache key)
def a_plan(bias=0.5, **kw):
    """A plan with every field away from its default, over a freshly built constraint description."""
    c = cons(sequence_bias=[[[5, 6], bias], [[7], -1.0]], bad_words_ids=[[3, gu.EOS]], suppress_tokens=[4], begin_suppress_tokens=[8],
             forced_bos_token_id=6, forced_eos_token_id=[gu.EOS])
    f = dict(kind="beam", special=(gu.SEP, gu.BOS), mask_token_id=gu.PAD, bos=gu.BOS, eos=gu.EOS, pad=gu.PAD, max_length=20, train=True,
             controls=gen.Controls(1.3, 3, 9, c), record=gen.Record(True, True, 4), top_k=5, temperature=0.7, top_p=0.9, num_beams=4,
             length_penalty=2.0, prompt_len=3, early_stopping=2)
    f.update(kw)
    return gen.StepPlan(**f)


def changed(v):
    """Another value of v's own type: the first leaf of a (named) tuple is changed."""
    if isinstance(v, bool):
        return not v
    if isinstance(v, (int, float)):
        return v + 1
    if isinstance(v, str):
        return v + "x"
    if isinstance(v, tuple):
        head = (changed(v[0]),) + tuple(v[1:]) if v else (1,)
        return type(v)(*head) if hasattr(v, "_fields") else head
    assert v is None, v
    return 0


def test_equal_options_give_equal_plans():
    a, b = a_plan(), a_plan()
    assert a.controls.cons is not b.controls.cons                        # two token_constraints() calls: equal, distinct descriptions
    assert a == b and hash(a) == hash(b)
    assert {(7, 8, 0, a): "graph"}[(7, 8, 0, b)] == "graph"              # the captured step of the first call is found by the second


@pytest.mark.parametrize("field", [f.name for f in dataclasses.fields(gen.StepPlan)])
def test_any_changed_field_gives_an_unequal_plan(field):
    a = a_plan()
    v = getattr(a, field)
    b = dataclasses.replace(a, **{field: changed(v)})
    assert a != b and (7, 8, 0, b) not in {(7, 8, 0, a): "graph"}
    if hasattr(v, "_fields"):                                            # every leaf of the controls / the record request counts
        for name in v._fields:
            assert dataclasses.replace(a, **{field: v._replace(**{name: changed(getattr(v, name))})}) != a, (field, name)


def test_one_sequence_bias_entry_changes_the_plan():
    a, b = a_plan(), a_plan(bias=0.25)
    assert a.controls.cons[0][0] == ((5, 6), 0.5) and b.controls.cons[0][0] == ((5, 6), 0.25)
    assert a != b and (7, 8, 0, b) not in {(7, 8, 0, a): "graph"}


def test_plan_refuses_values_compared_by_identity():
    for bad in ([gu.SEP], torch.tensor([gu.SEP]), {gu.SEP: 1}, ([gu.SEP],), len):
        with pytest.raises(TypeError):
            a_plan(special=bad)
    with pytest.raises(TypeError):
        a_plan(controls=gen.Controls(1.3, 3, 9, ([((5, 6), 0.5)],)))           # a list nested in the constraints
    with pytest.raises(TypeError):
        a_plan(eos=torch.tensor(gu.EOS))


def test_controls_say_what_a_step_launches():
    assert not gen.Controls().active and not gen.Controls().constrained
    for c in (gen.Controls(penalty=1.3), gen.Controls(ngram=2), gen.Controls(min_abs=5)):
        assert c.active and not c.constrained
    c = gen.Controls(cons=cons(suppress_tokens=[4]))
    assert c.active and c.constrained
    assert not gen.Record().on and gen.Record(logits=True).on and gen.Record(scores=True).on


# ------------------------------------------------------------------------------------------------ generation_config
def test_resolve_generation_options_precedence():
    from transformers import GenerationConfig
    d = gen.GENERATION_DEFAULTS
    assert gen.resolve_generation_options({}, None) == d
    assert gen.resolve_generation_options({k: gen.UNSET for k in d}, None) == d
    for cfg in (GenerationConfig(num_beams=4, max_length=33, early_stopping=True, bad_words_ids=[[5]], top_k=None),
                SimpleNamespace(num_beams=4, max_length=33, early_stopping=True, bad_words_ids=[[5]], top_k=None)):
        o = gen.resolve_generation_options({}, cfg)
        assert (o["num_beams"], o["max_length"], o["early_stopping"], o["bad_words_ids"]) == (4, 33, True, [[5]])
        assert o["top_k"] == 50 and o["repetition_penalty"] == 1.0       # None fields: the engine's defaults
        # a keyword the caller passed wins, even when it equals the default
        o = gen.resolve_generation_options(dict(num_beams=1, early_stopping=False, max_length=gen.UNSET, bad_words_ids=None), cfg)
        assert (o["num_beams"], o["early_stopping"], o["max_length"], o["bad_words_ids"]) == (1, False, 33, None)
    o = gen.resolve_generation_options({}, GenerationConfig(eos_token_id=[2], forced_eos_token_id=[2, 3], suppress_tokens=[7]))
    assert o["eos_token_id"] == 2 and o["forced_eos_token_id"] == [2, 3] and o["suppress_tokens"] == [7]


@pytest.mark.parametrize("field,value", [("num_beam_groups", 2), ("penalty_alpha", 0.6), ("typical_p", 0.9), ("min_p", 0.1), ("epsilon_cutoff", 3e-4),
                                         ("eta_cutoff", 3e-4), ("exponential_decay_length_penalty", (5, 1.1)), ("encoder_repetition_penalty", 1.2),
                                         ("encoder_no_repeat_ngram_size", 2), ("guidance_scale", 1.5)])
def test_resolve_generation_options_refuses_unsupported_fields(field, value):
    with pytest.raises(NotImplementedError, match=field):
        gen.resolve_generation_options({}, SimpleNamespace(**{field: value}))
    assert gen.resolve_generation_options({field: value}, None) == gen.GENERATION_DEFAULTS      # (as a plain keyword it never reaches the merge)


def test_resolve_generation_options_neutral_fields_and_beam_sampling():
    from transformers import GenerationConfig
    neutral = SimpleNamespace(num_beam_groups=1, typical_p=1.0, encoder_repetition_penalty=1.0, encoder_no_repeat_ngram_size=0, epsilon_cutoff=0.0,
                              guidance_scale=1.0, renormalize_logits=False)
    assert gen.resolve_generation_options({}, neutral) == gen.GENERATION_DEFAULTS
    with pytest.raises(NotImplementedError, match="do_sample"):
        gen.resolve_generation_options({}, GenerationConfig(do_sample=True, num_beams=4))
    with pytest.raises(NotImplementedError, match="do_sample"):
        gen.resolve_generation_options(dict(num_beams=2), SimpleNamespace(do_sample=True))
    assert gen.resolve_generation_options(dict(num_beams=1), GenerationConfig(do_sample=True, num_beams=4))["do_sample"] is True


# ------------------------------------------------------------------------------------------------ the restatement against the reference
def test_restated_early_stopping_search_reproduces_the_references_recorded_searches():
    """tests/golden/gen_constraints.npz holds the fp32 logits of every step of the reference's beam-4 generate under early_stopping True / "never" /
    False (length_penalty 2.0). The CPU restatement replays them: it must feed the recorded tokens at every step, stop on the reference's step and
    return its hypotheses bit for bit. The GPU tests then compare the device search with this restatement step by step."""
    G = gu.load("gen_constraints.npz")
    lp, L = float(G["es_length_penalty"]), int(G["es_steps"]) + 1
    steps = {}
    for name, mode in (("true", True), ("never", "never"), ("false", False)):
        logits, fed = torch.from_numpy(G["es_logits"]), torch.from_numpy(G["es_fed"])      # every recorded step is on offer in every mode
        want, want_sc = torch.from_numpy(G[f"es_{name}_all"]), torch.from_numpy(G[f"es_{name}_all_scores"])
        seqs, sc, trace = ref.beam_search(list(logits), 3, 4, gu.BOS, gu.EOS, gu.PAD, L, lp, mode, fed=fed)
        assert len(trace) == int(G[f"es_{name}_steps"]) and trace[-1]["stop"], name
        assert torch.equal(seqs[:, :, :want.shape[-1]], want) and bool((seqs[:, :, want.shape[-1]:] == gu.PAD).all()), name
        np.testing.assert_allclose(sc.numpy(), want_sc.numpy(), rtol=2e-6, atol=2e-5, err_msg=name)
        steps[name] = len(trace)
    assert steps["true"] < steps["false"] < steps["never"]               # early_stopping=True ends the search on an earlier step
    assert steps["true"] < L - 1
