"""CPU: the BERTScore surface that needs no GPU -- C ABI declarations, wrappers refusing host tensors, the zero-floor flags, the baseline file,
the state-dict mapping and the metric's argument checks (reference tools/metrics/bertscore.py)."""
import ctypes

import numpy as np
import pytest
import torch

from cxrmate_amd import bertscore, ops
from cxrmate_amd._lib import CxrError, parse_header


def test_header_declares_the_entry_points():
    protos = parse_header()
    v, L, I, F = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
    want = {
        "cxr_roberta_embed_fwd": [("ids", v), ("B", L), ("T", I), ("word", v), ("vocab", L), ("type", v), ("posw", v), ("n_pos", L), ("gamma", v),
                                  ("beta", v), ("eps", F), ("padding_idx", L), ("out", v), ("pos_out", v), ("C", I), ("stream", v)],
        "cxr_bertscore_match": [("hidden", v), ("n_rows", L), ("D", I), ("sent", v), ("n_sent", I), ("pairs", v), ("weights", v), ("floors", v),
                                ("n_pairs", I), ("P", v), ("R", v), ("F", v), ("stream", v)],
        "cxr_layernorm_fwd_bf16": [("x", v), ("ldx", L), ("gamma", v), ("beta", v), ("y", v), ("ldy", L), ("stats", v), ("rows", L), ("C", I),
                                   ("eps", F), ("stream", v)],
    }
    for name, args in want.items():
        assert name in protos, name
        assert [(n, t) for t, n in protos[name]] == args, name


def test_wrappers_refuse_host_tensors():
    bf = torch.bfloat16
    with pytest.raises(CxrError):
        ops.roberta_embed(torch.ones(2, 5, dtype=torch.int64), torch.zeros(10, 1024, dtype=bf), torch.zeros(1, 1024, dtype=bf),
                          torch.zeros(514, 1024, dtype=bf), torch.ones(1024), torch.zeros(1024), 1e-5, 1)
    with pytest.raises(CxrError):
        ops.bertscore_match(torch.zeros(6, 1024, dtype=bf), torch.tensor([[0, 3], [3, 3]], dtype=torch.int32), torch.tensor([[0, 1]], dtype=torch.int32),
                            torch.ones(6), torch.zeros(1, 2, dtype=torch.uint8))
    with pytest.raises(CxrError):
        ops.layernorm(torch.zeros(4, 1024, dtype=bf), torch.ones(1024), torch.zeros(1024), 1e-5)


def test_floor_flags_hand_worked():
    # 5 pairs in chunks of 2: {0, 1}, {2, 3}, {4}
    hyp = [5, 3, 4, 4, 2]
    ref = [3, 6, 7, 2, 9]
    # chunk {0,1}: longest ref 6, longest hyp 5 -> pair 0: ref 3 < 6 floors P; pair 1: hyp 3 < 5 floors R
    # chunk {2,3}: longest ref 7, longest hyp 4 (a tie) -> pair 3: ref 2 < 7 floors P; nothing else
    # chunk {4}: alone, its own longest on both sides
    want = np.array([[1, 0], [0, 1], [0, 0], [1, 0], [0, 0]], dtype=np.uint8)
    got = bertscore.floor_flags(hyp, ref, 2)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert not bertscore.floor_flags(hyp, ref, 1).any()             # one pair per chunk: no padding anywhere


def test_baseline_file_and_tuple(tmp_path):
    p = tmp_path / "roberta-large.tsv"
    rows = ["LAYER,P,R,F"] + [f"{i},{0.8 + i / 1000:.6f},{0.81 + i / 1000:.6f},{0.82 + i / 1000:.6f}" for i in range(25)]
    p.write_text("\n".join(rows) + "\n")
    b = bertscore.load_baseline(str(p), 17)
    np.testing.assert_allclose(b.numpy(), [0.817, 0.827, 0.837], rtol=0, atol=1e-7)
    t = tmp_path / "tabbed.tsv"
    t.write_text("\n".join(r.replace(",", "\t") for r in rows) + "\n")
    assert torch.equal(bertscore.load_baseline(str(t), 17), b)
    assert torch.equal(bertscore.load_baseline((0.817, 0.827, 0.837), 17), b)
    with pytest.raises(ValueError):
        bertscore.load_baseline(str(p), 40)
    with pytest.raises(ValueError):
        bertscore.load_baseline((0.1, 0.2), 17)


def test_config_and_state_dict_mapping():
    cfg = bertscore.roberta_large_config()
    assert (cfg.vocab_size, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size) == (50265, 1024, 17, 16, 4096)
    assert (cfg.max_position_embeddings, cfg.type_vocab_size, cfg.layer_norm_eps, cfg.pad_token_id) == (514, 1, 1e-5, 1)
    assert not cfg.is_decoder and not cfg.add_cross_attention
    x = torch.zeros(1)
    for pre in ("roberta.", ""):
        sd = {pre + "embeddings.word_embeddings.weight": x, pre + "embeddings.position_ids": x, pre + "encoder.layer.0.output.dense.weight": x,
              pre + "encoder.layer.16.attention.self.query.bias": x, pre + "encoder.layer.17.output.dense.weight": x,
              pre + "encoder.layer.23.output.dense.weight": x, pre + "pooler.dense.weight": x}
        sd["lm_head.dense.weight"] = x
        got = bertscore.roberta_state_dict(sd, 17)
        assert list(got) == ["bert.embeddings.word_embeddings.weight", "bert.encoder.layer.0.output.dense.weight",
                             "bert.encoder.layer.16.attention.self.query.bias"], pre
    assert set(bertscore.roberta_param_shapes(bertscore.roberta_large_config(2))) >= {"bert.encoder.layer.1.output.LayerNorm.bias"}
    assert not any(k.startswith("cls.") for k in bertscore.roberta_param_shapes(cfg))


def test_metric_argument_checks(tmp_path):
    m = bertscore.BERTScoreRoBERTaLarge("test", None, 4, str(tmp_path), accumulate_over_dicoms=True, num_workers=2)
    assert (tmp_path / "bertscore").is_dir()
    with pytest.raises(AssertionError):
        m.update("not a list", [["a"]], [1], ["x"])
    with pytest.raises(AssertionError):
        m.update([1], [["a"]], [1], ["x"])
    with pytest.raises(AssertionError):
        m.update(["a"], "not a list", [1], ["x"])
    with pytest.raises(AssertionError):
        m.update(["a"], ["not a list of lists"], [1], ["x"])
    with pytest.raises(AssertionError):
        m.update(["a"], [[3]], [1], ["x"])
    m.update(["a", "b"], [["c"], ["d"]], [1, 2], ["x", "y"])
    assert m.reports == [{"prediction": "a", "label": ["c"], "study_id": 1, "dicom_id": "x"},
                         {"prediction": "b", "label": ["d"], "study_id": 2, "dicom_id": "y"}]
    with pytest.raises(RuntimeError, match="RobertaScorer"):
        m.compute(0)
    m.reset()
    assert m.reports == []
