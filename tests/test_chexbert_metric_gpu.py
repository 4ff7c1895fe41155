"""GPU: the CheXbert classification metric (reference tools/metrics/chexbert.py) -- `cxr_chexbert_scores` against the numbers recorded from the
reference and against a float64 restatement, its out-of-range convention, the metric's update / compute flow with a table look-up labeller and
with the real labeller, and `CheXbert.label_all` against `CheXbert.__call__`."""
import glob
import os

import numpy as np
import pytest
import torch

import chexbert_metric_ref as cref
import golden_util as gu
from bounds_util import _SENT, Guarded

pytestmark = pytest.mark.gpu
I64, F64 = torch.int64, torch.float64


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


class Guarded64:
    """A float64 output of `shape` inside a sentinel-guarded buffer (bounds_util.Guarded has no float64 sentinel: the 8-byte integer one is used and
    the output is its float64 view)."""

    def __init__(self, *shape):
        self.g = Guarded.flat(int(np.prod(shape)), I64)
        self.t = self.g.view.view(F64).view(*shape)

    def check(self, what):
        self.g.check(what)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.g.view == _SENT[I64][1]).all())

    def bits(self):
        return self.g.view.cpu().clone()


def _launch(pred, ref, pred_row, ref_row, off):
    """One call of the C entry point with every output and the workspace guarded -> (example, cls, avg, workspace) Guarded64."""
    from cxrmate_amd import ops
    from cxrmate_amd._lib import LIB
    dev = [torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in (pred, ref, pred_row, ref_row, off)]
    assert [t.dtype for t in dev] == [I64, I64, torch.int32, torch.int32, torch.int32]
    n_s = len(off) - 1
    outs = Guarded64(n_s, 8), Guarded64(14, 8), Guarded64(12), Guarded64(56 * n_s + 64)
    LIB.call("cxr_chexbert_scores", dev[0].data_ptr(), dev[0].shape[0], dev[1].data_ptr(), dev[1].shape[0], dev[2].data_ptr(), dev[3].data_ptr(),
             len(pred_row), dev[4].data_ptr(), n_s, outs[0].t.data_ptr(), outs[1].t.data_ptr(), outs[2].t.data_ptr(), outs[3].t.data_ptr(),
             outs[3].t.numel() * 8, ops._s())
    for o, name in zip(outs, ("example", "cls", "avg", "workspace")):
        o.check(f"chexbert_scores {name}")
    return outs


def _host(o):
    return o.t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("name", list("abcde"))
def test_kernel_vs_recorded_reference(cuda, name):
    """avg, cls and example equal what the reference returned / wrote for the same tables (rtol 1e-12, atol 1e-9: see cref.assert_close for the
    derivation), NaN positions included."""
    fx = cref.load_fixture()
    case = fx["cases"][name]
    example, cls, avg, _ = _launch(*cref.case_tables(case, fx["pathologies"]))
    res = case["result"]
    print(name, "avg", _host(avg).tolist())
    cref.assert_close(_host(avg), cref.nan_array([v for _, v in res[:12]]), f"{name} avg")
    cref.assert_close(_host(cls)[:, 4:].T.reshape(-1), cref.nan_array([v for _, v in res[12:68]]), f"{name} cls")
    cref.assert_close(_host(example), np.array([cref.nan_array(r[1:]) for r in case["csv"]["example_scores"]["rows"]]), f"{name} example")
    if name == "c":                                                 # no positive anywhere: the micro ratios stay NaN, everything else is filled
        assert np.isnan(_host(avg)[9:]).all() and not np.isnan(_host(avg)[:9]).any() and not np.isnan(_host(cls)).any()


def _big_case(S=5003, n_ref=701, seed=9):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 6, size=S)                             # 1-5 records per study
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    M = int(off[-1])
    pred = rng.choice(4, size=(M, 14), p=[0.45, 0.3, 0.15, 0.1]).astype(np.int64)
    ref = rng.choice(4, size=(n_ref, 14), p=[0.45, 0.3, 0.15, 0.1]).astype(np.int64)
    pred[:, 13] = pred[:, 13] == 1
    ref[:, 13] = ref[:, 13] == 1
    pred[:, 4] = np.where(pred[:, 4] == 1, 2, pred[:, 4])           # a pathology nobody predicts
    pred_row = rng.permutation(M).astype(np.int32)
    ref_row = np.repeat(rng.integers(0, n_ref, size=S), counts).astype(np.int32)          # the records of a study share its label row
    return pred, ref, pred_row, ref_row, off


def test_kernel_vs_float64_restatement_and_repeatable(cuda):
    args = _big_case()
    first = _launch(*args)
    want = cref.scores(*args)
    for got, w, what in zip(first, want, ("example", "cls", "avg")):
        err = np.nanmax(np.abs(_host(got) - w))
        print(what, "largest |difference|", err)
        cref.assert_close(_host(got), w, what)
    assert not np.isnan(_host(first[2])).any() and _host(first[1])[4, 5] == 0.0             # precision of the unpredicted pathology: 0 / 0 -> 0
    second = _launch(*args)
    for a, b, what in zip(first[:3], second[:3], ("example", "cls", "avg")):
        assert torch.equal(a.bits(), b.bits()), f"{what}: the second launch differs in bits"


def test_kernel_out_of_range_rows_and_rejected_sizes(cuda):
    from cxrmate_amd._lib import CxrError
    pred, ref, pred_row, ref_row, off = _big_case(S=40, n_ref=11, seed=4)
    good = cref.scores(pred, ref, pred_row, ref_row, off)[0]
    bad_p, bad_r = pred_row.copy(), ref_row.copy()
    bad_p[off[7]] = pred.shape[0]                                   # one past the prediction table
    bad_r[off[21] - 1] = -1                                         # before the label table (study 20's last record)
    bad_r[off[33]] = 10 ** 9
    example, cls, avg, _ = _launch(pred, ref, bad_p, bad_r, off)   # the guards are checked inside
    ex = _host(example)
    hit = np.zeros(40, dtype=bool)
    hit[[7, 20, 33]] = True
    assert np.isnan(ex[hit]).all()
    cref.assert_close(ex[~hit], good[~hit], "neighbours of the NaN studies")
    assert np.isnan(_host(cls)[:, :4]).all() and np.isnan(_host(avg)).all()                 # the table as a whole has no scores
    bad_off = off.copy()
    bad_off[40] = len(pred_row) + 3                                 # an offset past the records
    ex = _host(_launch(pred, ref, pred_row, ref_row, bad_off)[0])
    assert np.isnan(ex[39]).all()
    cref.assert_close(ex[:39], good[:39], "studies before the bad offset")
    for kw in (dict(S=0), dict(M=0)):                               # rejected, nothing written
        outs = [Guarded64(40, 8), Guarded64(14, 8), Guarded64(12)]
        with pytest.raises(CxrError, match="cxr_chexbert_scores failed with code -1"):
            _launch_into(outs, pred, ref, pred_row, ref_row, off, **kw)
        assert all(o.untouched() for o in outs), kw


def _launch_into(outs, pred, ref, pred_row, ref_row, off, S=None, M=None):
    from cxrmate_amd import ops
    from cxrmate_amd._lib import LIB
    dev = [torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in (pred, ref, pred_row, ref_row, off)]
    ws = torch.empty(56 * (len(off) - 1) + 64, dtype=F64, device="cuda")
    LIB.call("cxr_chexbert_scores", dev[0].data_ptr(), dev[0].shape[0], dev[1].data_ptr(), dev[1].shape[0], dev[2].data_ptr(), dev[3].data_ptr(),
             len(pred_row) if M is None else M, dev[4].data_ptr(), len(off) - 1 if S is None else S, outs[0].t.data_ptr(), outs[1].t.data_ptr(),
             outs[2].t.data_ptr(), ws.data_ptr(), ws.numel() * 8, ops._s())


def test_wrapper_equals_the_entry_point(cuda):
    from cxrmate_amd import ops
    args = _big_case(S=300, n_ref=40, seed=6)
    direct = _launch(*args)
    got = ops.chexbert_scores(*(torch.as_tensor(a).cuda() for a in args))
    assert [tuple(t.shape) for t in got] == [(300, 8), (14, 8), (12,)] and all(t.dtype == F64 for t in got)
    for a, b in zip(direct, got):
        assert torch.equal(a.t, b)


# ------------------------------------------------------------------------------------------------ metric, table look-up labeller
def _csv(save_dir, split, epoch, kind):
    import pandas as pd
    files = glob.glob(os.path.join(save_dir, f"{split}_epoch-{epoch}_{kind}_[0-9]*.csv"))
    assert len(files) == 1, (kind, files)
    return pd.read_csv(files[0])


@pytest.mark.parametrize("name", list("abcde"))
def test_metric_returns_the_reference_dict(cuda, tmp_path, name):
    from cxrmate_amd.metrics import CheXbertClassificationMetrics
    fx = cref.load_fixture()
    case = fx["cases"][name]
    acc = case["accumulate_over_dicoms"]
    lab = cref.LookupLabeller(case["table"], cuda)
    metric = CheXbertClassificationMetrics("test", None, None, None, case["mbatch_size"], str(tmp_path), acc, chexbert=lab)
    for c in case["calls"]:
        metric.update(c["predictions"], c["labels"], c["study_ids"], c.get("dicom_ids"))
    out = metric.compute(epoch=7)
    res = case["result"]
    assert list(out) == [k for k, _ in res] and len(out) == (70 if acc else 69)
    assert all(type(v) is float for v in out.values())
    print(name, {k: out[k] for k in list(out)[:12]})
    cref.assert_close(list(out.values()), cref.nan_array([v for _, v in res]), f"case {name}")
    n_records = sum(len(c["predictions"]) for c in case["calls"])
    n_labels = len({c_[0] for c in case["calls"] for c_ in c["labels"]})
    assert lab.calls == [n_records, n_labels]                        # every prediction, then every DISTINCT label text, once
    for kind in ("y_hat", "y", "class_scores", "example_scores"):
        df, want = _csv(metric.save_dir, "test", 7, kind), case["csv"][kind]
        assert list(df.columns) == want["columns"] and len(df) == len(want["rows"]), kind
        rows = [list(r) for r in df.itertuples(index=False, name=None)]
        if kind in ("y_hat", "y"):
            assert rows == want["rows"], kind                        # ids and class indices, in the reference's row order
        else:
            ids = 1 if kind == "example_scores" else 0
            assert [r[:ids] for r in rows] == [r[:ids] for r in want["rows"]]
            cref.assert_close(np.array([r[ids:] for r in rows], dtype=np.float64), np.array([cref.nan_array(r[ids:]) for r in want["rows"]]), kind)
    metric.reset()
    assert metric.reports == []


# ------------------------------------------------------------------------------------------------ labeller
REPORTS = [
    "The lungs are clear.",
    "  The lungs are clear.\nNo pleural effusion. ",
    "Mild cardiomegaly is stable.",
    "Support devices in place.",
    "Normal.",
    "No acute cardiopulmonary process.",
    "Small left pleural effusion.",
    "There is a small right pleural effusion with adjacent atelectasis. No pneumothorax is seen.",
    "Heart size is normal. The mediastinal and hilar contours are unremarkable. The lungs are clear without focal consolidation.",
    "The endotracheal tube ends above the carina. The enteric tube passes into the stomach and out of view.",
    "No focal consolidation, pleural effusion or pneumothorax.",
    "Moderate pulmonary edema has worsened since the prior study. Bilateral pleural effusions are unchanged.",
    "New right lower lobe consolidation, likely pneumonia.",
    "Low lung volumes.",
    "Stable cardiomegaly. No evidence of pulmonary edema. Old healed left rib fractures are noted.",
    "Left basilar atelectasis.",
    "The right chest tube has been removed. There is no pneumothorax.",
    "The cardiomediastinal silhouette is within normal limits. No acute osseous abnormality.",
    "Patchy bibasilar opacities may reflect atelectasis or infection in the appropriate clinical setting. Follow up is recommended.",
    "Clear lungs.",
    "A left pectoral pacemaker is in place with leads in the right atrium and right ventricle. The lungs are hyperinflated. There is no focal "
    "consolidation, effusion or pneumothorax. The heart is mildly enlarged.",
    "No change.",
    "Mild vascular congestion without frank edema.",
    "Lungs clear. Heart normal.",
]
MARGIN = 6e-2           # fp32 top-2 margin above which the bf16 trunk must agree (tests/test_reward_scst_gpu.py::test_chexbert_labeller_heads)


def _tiny_labeller(cuda):
    import transformers
    from cxrmate_amd.chexbert import CheXbert
    tok = transformers.PreTrainedTokenizerFast(tokenizer_file=os.path.join(gu.GOLDEN, "tokenizer.json"), unk_token="[UNK]", pad_token="[PAD]",
                                               cls_token="[BOS]", sep_token="[SEP]", mask_token="[MASK]")
    cfg = gu.BertConfig(vocab_size=600, num_hidden_layers=2, is_decoder=False, add_cross_attention=False, cls_projection_size=0)
    return CheXbert(cuda, tokenizer=tok, config=cfg), tok, cfg


def _oracle_margins(cb, tok, cfg, texts):
    """fp32 oracle, one report at a time (no padding): top-2 margin of every head's logits, [len(texts), 14]."""
    from cxrmate_amd.chexbert import HEAD_CLASSES
    from oracle import bert as obert
    sd = {k: v.detach().float().cpu() for k, v in cb.model.state_dict().items()}
    out = []
    for t in texts:
        e = tok([t.strip().replace("\n", " ").strip()], padding="longest", return_tensors="pt", truncation=True, max_length=cfg.max_position_embeddings)
        with torch.no_grad():
            h = obert.embeddings(e["input_ids"], e.get("token_type_ids"), None, sd, "bert.embeddings.", cfg.layer_norm_eps)
            c = obert.bert_layers(h, sd, "bert.", cfg, torch.zeros(1, 1, 1, e["input_ids"].shape[1]), None, None, cfg.layer_norm_eps)[:, 0]
            row = []
            for i in range(len(HEAD_CLASSES)):
                top2 = torch.nn.functional.linear(c, sd[f"linear_heads.{i}.weight"], sd[f"linear_heads.{i}.bias"])[0].topk(2).values
                row.append(float(top2[0] - top2[1]))
        out.append(row)
    return torch.tensor(out)


def test_label_all_equals_call_on_unsorted_mini_batches(cuda):
    """`label_all` (one tokenizer call, longest-first mini-batches, order restored on the device) against `__call__` on consecutive mini-batches of
    the same 24 reports in their given order: equal on every head whose fp32-oracle top-2 margin exceeds 6e-2, and at most 10 % of the 336 heads may
    fall under that margin. For this list and the seeded tiny labeller the fp32 oracle alone puts 26 of 336 heads (7.7 %) under it (computed on
    the CPU with oracle.bert before this list was committed)."""
    cb, tok, cfg = _tiny_labeller(cuda)
    mb = 4
    texts = list(REPORTS)
    got = cb.label_all(texts, mb)
    assert texts == REPORTS                                          # the caller's list is left alone
    assert got.shape == (24, 14) and got.dtype == I64 and got.is_cuda
    want = torch.cat([cb(list(REPORTS[lo:lo + mb])) for lo in range(0, len(REPORTS), mb)])
    safe = _oracle_margins(cb, tok, cfg, REPORTS) > MARGIN
    share = 1.0 - float(safe.float().mean())
    print(f"heads under the margin: {int((~safe).sum())} of {safe.numel()} ({share:.3f}); heads differing at all: {int((got != want).sum())}")
    assert share <= 0.10
    assert torch.equal(got.cpu()[safe], want.cpu()[safe])
    assert int(got[:, :13].max()) <= 3 and int(got[:, 13].max()) <= 1 and int(got.min()) >= 0
    assert cb.label_all([], mb).shape == (0, 14)
    assert torch.equal(cb.label_all(texts[:5], 100), cb.label_all(texts[:5], 100))


def test_metric_with_the_real_labeller(cuda, tmp_path):
    """The whole flow on the tiny labeller: the scores equal the float64 restatement applied to the labels the metric itself produced (its y_hat / y
    CSVs), a repeated DICOM is dropped, and a label text shared by several records is labelled once."""
    from cxrmate_amd.metrics import PATHOLOGIES, CheXbertClassificationMetrics
    cb, _, _ = _tiny_labeller(cuda)
    handed, produced = [], []
    inner = cb.label_all

    def spy(texts, mbatch_size):
        handed.append(list(texts))
        produced.append(inner(texts, mbatch_size))
        return produced[-1]

    cb.label_all = spy
    metric = CheXbertClassificationMetrics("val", None, None, None, 3, str(tmp_path), accumulate_over_dicoms=True, chexbert=cb)
    preds = REPORTS[:9]
    labels = [[REPORTS[10]], [REPORTS[10]], [REPORTS[11]], [REPORTS[12]], [REPORTS[12]], [REPORTS[12]], [REPORTS[13]], [REPORTS[10]], [REPORTS[14]]]
    studies = [52, 52, 51, 50, 50, 50, 53, 54, 54]
    dicoms = ["a", "b", "c", "d", "e", "f", "g", "h", "i"]
    metric.update(preds[:5], labels[:5], studies[:5], dicoms[:5])
    metric.update(preds[5:], labels[5:], studies[5:], dicoms[5:])
    metric.update([REPORTS[20], REPORTS[21]], [[REPORTS[10]], [REPORTS[11]]], [52, 51], ["a", "c"])      # repeated DICOMs (DDP padding)
    out = metric.compute(epoch=2)
    assert [len(h) for h in handed] == [11, 5]                       # 11 predictions; 5 distinct label texts for 11 records
    assert len(out) == 70 and out["num_study_ids"] == 5.0 and out["num_dicom_ids"] == 9.0
    yh, y = _csv(metric.save_dir, "val", 2, "y_hat"), _csv(metric.save_dir, "val", 2, "y")
    assert list(yh.columns) == ["dicom_id", "study_id"] + PATHOLOGIES and list(yh.dicom_id) == dicoms and list(y.study_id) == studies
    assert handed[1] == [REPORTS[i] for i in (10, 11, 12, 13, 14)]
    assert np.array_equal(yh[PATHOLOGIES].to_numpy(), produced[0].cpu().numpy()[:9])         # the first record of a DICOM stays: the first nine
    assert np.array_equal(y[PATHOLOGIES].to_numpy(), produced[1].cpu().numpy()[[0, 0, 1, 2, 2, 2, 3, 0, 4]])
    group = np.array([sorted(set(studies)).index(s) for s in studies])
    order = np.argsort(group, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(group))]).astype(np.int32)
    example, cls, avg = cref.scores(yh[PATHOLOGIES].to_numpy(), y[PATHOLOGIES].to_numpy(), order, order, off)
    cref.assert_close(list(out.values())[:12], avg, "avg")
    cref.assert_close(list(out.values())[12:68], cls[:, 4:].T.reshape(-1), "cls")
    ex = _csv(metric.save_dir, "val", 2, "example_scores")
    assert list(ex.study_id) == [50, 51, 52, 53, 54]                 # grouped as pandas groupby orders them
    cref.assert_close(ex.to_numpy(dtype=np.float64)[:, 1:], example, "example")
    cs = _csv(metric.save_dir, "val", 2, "class_scores")
    assert len(cs) == 1 and list(cs.columns) == list(out)[12:68]
