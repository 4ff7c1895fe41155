"""CPU: the C ABI of the per-step output entry points (csrc/gen_record.hip, the beam-index beam step in csrc/decode.hip), and
compute_transition_scores (TF5 GenerationMixin semantics) on hand-made CPU tensors."""
import ctypes

import pytest
import torch

from cxrmate_amd._lib import CxrError, parse_header


def test_header_declares_gen_record_with_parsable_arguments():
    protos = parse_header()
    assert "cxr_gen_record_f32" in protos
    args = protos["cxr_gen_record_f32"]
    assert [n for _, n in args] == ["x", "ld", "R", "V", "nb", "logits_out", "scores_out", "log_softmax", "stream"]
    types = dict((n, t) for t, n in args)
    for n in ("x", "logits_out", "scores_out", "stream"):
        assert types[n] is ctypes.c_void_p, n
    for n in ("ld", "R"):
        assert types[n] is ctypes.c_long, n
    for n in ("V", "nb", "log_softmax"):
        assert types[n] is ctypes.c_int, n


def test_header_declares_beam_step_idx_as_beam_step_plus_histories():
    protos = parse_header()
    assert "cxr_beam_step_idx" in protos
    idx, plain = protos["cxr_beam_step_idx"], protos["cxr_beam_step"]
    names = [n for _, n in idx]
    assert names[:11] == [n for _, n in plain][:11]                       # logits .. ws
    assert names[11:13] == ["run_bidx", "fin_bidx"]
    assert names[13:] == [n for _, n in plain][11:-1] + ["logprobs", "stream"]
    types = dict((n, t) for t, n in idx)
    assert types["run_bidx"] is ctypes.c_void_p and types["fin_bidx"] is ctypes.c_void_p
    assert types["logprobs"] is ctypes.c_int and types["div"] is ctypes.c_float and types["eos"] is ctypes.c_long


def test_wrappers_refuse_cpu_tensors():
    from cxrmate_amd import ops
    x = torch.zeros((4, 16), dtype=torch.float32)
    with pytest.raises(CxrError, match="no CPU path"):
        ops.gen_record(x, logits_out=torch.zeros_like(x), nb=2)
    nb, B, L = 2, 2, 4
    with pytest.raises(CxrError, match="no CPU path"):
        ops.beam_step(x, torch.zeros((nb, B, L), dtype=torch.int64), torch.zeros((nb, B, L), dtype=torch.int64), torch.zeros((B, nb)),
                      torch.zeros((B, nb)), torch.zeros((B, nb), dtype=torch.uint8), torch.ones((2, B), dtype=torch.int32),
                      torch.zeros((2, B), dtype=torch.int32), torch.zeros(nb * B, dtype=torch.int64), 1, 4, 2, 1.0, ws=torch.zeros(64),
                      bidx=(torch.full((nb, B, L), -1, dtype=torch.int32), torch.full((nb, B, L), -1, dtype=torch.int32)))


def _mixin():
    from cxrmate_amd.generation import GenerationMixin
    return GenerationMixin()


def test_transition_scores_greedy_pick_each_rows_token():
    g = torch.Generator().manual_seed(0)
    R, T, V, P = 3, 4, 7, 2
    scores = tuple(torch.randn(R, V, generator=g) for _ in range(T))
    seq = torch.cat([torch.ones(R, P, dtype=torch.int64), torch.randint(0, V, (R, T), generator=g)], 1)
    got = _mixin().compute_transition_scores(seq, scores)
    want = torch.tensor([[float(scores[t][r, seq[r, P + t]]) for t in range(T)] for r in range(R)])
    assert got.shape == (R, T) and torch.equal(got, want)
    norm = _mixin().compute_transition_scores(seq, scores, normalize_logits=True)
    want = torch.tensor([[float(torch.log_softmax(scores[t][r], -1)[seq[r, P + t]]) for t in range(T)] for r in range(R)])
    torch.testing.assert_close(norm, want)


def test_transition_scores_follow_beam_indices_and_mask_ended_steps():
    """Beam rows: step t of hypothesis n is read from row beam_indices[n, t] of scores[t]; -1 (the hypothesis had ended) gives 0, and the
    columns are cut to the longest hypothesis (the last columns of `sequences`)."""
    g = torch.Generator().manual_seed(1)
    rows, T, V = 4, 5, 6                                                    # 2 studies x 2 beams, 5 steps run
    scores = tuple(torch.randn(rows, V, generator=g) for _ in range(T))
    bidx = torch.tensor([[0, 1, 0, -1, -1, -1],                             # ended after 3 tokens
                         [2, 3, 3, 2, -1, -1]], dtype=torch.int32)          # 4 tokens: the longest
    seq = torch.tensor([[1, 5, 4, 2, 0, 0],
                        [1, 3, 1, 0, 2, 0]])
    seq = seq[:, :1 + 4]                                                    # prompt 1 + longest hypothesis
    got = _mixin().compute_transition_scores(seq, scores, bidx)
    want = torch.zeros(2, 4)
    for n in range(2):
        for t in range(4):
            if bidx[n, t] >= 0:
                want[n, t] = scores[t][int(bidx[n, t]), int(seq[n, 1 + t])]
    assert got.shape == (2, 4) and torch.equal(got, want)
    assert float(got[0, 3]) == 0.0
    torch.testing.assert_close(got.sum(1), torch.stack([want[0, :3].sum(), want[1].sum()]))
