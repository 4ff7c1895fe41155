"""float64 pure-Python restatement of the COCO NLG scorers as the reference's `COCONLGMetricsMIMICCXR` (tools/metrics/coco.py) calls them --
pycocoevalcap 1.2's `bleu_scorer.py`, `rouge.py` and `cider_scorer.py` -- for the metric tests. `Bleu`, `Rouge` and `Cider` carry the library's
`compute_score(gts, res)` signatures (gts / res: {id: [str]}, one hypothesis per id); tokens may be any hashable, so the array-level helpers run
the same code on word ids. Every record has exactly one reference."""
import json
import math
import os
from collections import defaultdict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COLUMNS = ("bleu_1", "bleu_2", "bleu_3", "bleu_4", "rouge", "cider")


def load_fixture():
    with open(os.path.join(GOLDEN, "coco_nlg.json")) as f:
        return json.load(f)


def _words(text, sep=None):
    return text.split(sep) if isinstance(text, str) else list(text)


def precook(words, n=4):
    """{k-gram tuple: count} for k = 1..n, filled order by order and position by position (the library's insertion order)."""
    counts = defaultdict(int)
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            counts[tuple(words[i:i + k])] += 1
    return counts


# ------------------------------------------------------------------------------------------------ BLEU (bleu_scorer.py, option='closest')
def bleu_pair(hyp, ref, n=4):
    """-> ([bleu_1..n], [c_1..c_n]) for one hypothesis / reference token list"""
    ch, cr = precook(hyp, n), precook(ref, n)
    correct = [0] * n
    for gram, count in ch.items():
        correct[len(gram) - 1] += min(count, cr.get(gram, 0))
    tiny, small = 1e-15, 1e-9
    out, bleu = [], 1.0
    for k in range(n):
        bleu *= (float(correct[k]) + tiny) / (float(max(0, len(hyp) - k)) + small)
        out.append(bleu ** (1.0 / (k + 1)))
    ratio = (len(hyp) + tiny) / (len(ref) + small)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out, correct


class Bleu:
    def __init__(self, n=4):
        self._n = n

    def compute_score(self, gts, res, verbose=0):
        """-> (corpus BLEU-1..n, [per-record list for each order]); the reference keeps the second only"""
        assert list(gts.keys()) == list(res.keys())
        n = self._n
        per = [[] for _ in range(n)]
        tot_c, tot_g, testlen, reflen = [0] * n, [0] * n, 0, 0
        for i in gts:
            assert len(res[i]) == 1 and len(gts[i]) == 1
            hyp, ref = _words(res[i][0]), _words(gts[i][0])
            scores, correct = bleu_pair(hyp, ref, n)
            for k in range(n):
                per[k].append(scores[k])
                tot_c[k] += correct[k]
                tot_g[k] += max(0, len(hyp) - k)
            testlen += len(hyp)
            reflen += len(ref)
        corpus, bleu = [], 1.0
        for k in range(n):
            bleu *= float(tot_c[k] + 1e-15) / (tot_g[k] + 1e-9)
            corpus.append(bleu ** (1.0 / (k + 1)))
        ratio = (testlen + 1e-15) / (reflen + 1e-9)
        if ratio < 1:
            corpus = [b * math.exp(1 - 1 / ratio) for b in corpus]
        return corpus, per


# ------------------------------------------------------------------------------------------------ ROUGE-L (rouge.py, beta = 1.2)
def lcs(a, b):
    """length of the longest common subsequence of two token lists (row DP; a row is the running maximum of its candidates)"""
    if not len(a) or not len(b):
        return 0
    ids = {}
    ia = np.array([ids.setdefault(t, len(ids)) for t in a], dtype=np.int64)
    ib = np.array([ids.setdefault(t, len(ids)) for t in b], dtype=np.int64)
    row = np.zeros(len(ib) + 1, dtype=np.int64)
    for t in ia:
        cand = np.maximum(row[1:], row[:-1] + (ib == t))
        row[1:] = np.maximum.accumulate(cand)
    return int(row[-1])


def rouge_pair(hyp, ref, beta=1.2):
    """-> (score, lcs) for two token lists (already split on single blanks)"""
    length = lcs(ref, hyp)
    if not len(hyp) or not len(ref):                # never from str.split(" "), which yields at least one token; the kernel's convention
        return 0.0, 0
    p, r = length / float(len(hyp)), length / float(len(ref))
    if p != 0 and r != 0:
        return ((1 + beta ** 2) * p * r) / float(r + beta ** 2 * p), length
    return 0.0, length


class Rouge:
    def compute_score(self, gts, res):
        assert list(gts.keys()) == list(res.keys())
        scores = []
        for i in gts:
            assert len(res[i]) == 1 and len(gts[i]) == 1
            scores.append(rouge_pair(_words(res[i][0], " "), _words(gts[i][0], " "))[0])
        return float(np.mean(np.array(scores))), np.array(scores)


# ------------------------------------------------------------------------------------------------ CIDEr-D (cider_scorer.py, n = 4, sigma = 6)
def cider_scores(hyps, refs, n=4, sigma=6.0, log=np.log):
    """-> float64 [M] for M hypothesis / reference token lists; `log` lets a test perturb the two logarithms"""
    chyp, cref = [precook(h, n) for h in hyps], [precook(r, n) for r in refs]
    df = defaultdict(float)
    for c in cref:
        for gram in c:
            df[gram] += 1
    ref_len = log(float(len(cref)))

    def counts2vec(counts):
        vec = [defaultdict(float) for _ in range(n)]
        norm = [0.0] * n
        length = 0
        for gram, tf in counts.items():
            k = len(gram) - 1
            vec[k][gram] = float(tf) * (ref_len - log(max(1.0, df[gram])))
            norm[k] += pow(vec[k][gram], 2)
            if k == 1:
                length += tf
        return vec, [np.sqrt(v) for v in norm], length

    out = []
    for ch, cr in zip(chyp, cref):
        vh, nh, lh = counts2vec(ch)
        vr, nr, lr = counts2vec(cr)
        delta = float(lh - lr)
        val = np.array([0.0 for _ in range(n)])
        for k in range(n):
            for gram in vh[k]:
                val[k] += min(vh[k][gram], vr[k][gram]) * vr[k][gram]
            if nh[k] != 0 and nr[k] != 0:
                val[k] /= nh[k] * nr[k]
            val[k] *= np.e ** (-(delta ** 2) / (2 * sigma ** 2))
        out.append(np.mean(val) * 10.0)
    return np.array(out, dtype=np.float64)


class Cider:
    def __init__(self, n=4, sigma=6.0):
        self._n, self._sigma = n, sigma

    def compute_score(self, gts, res):
        assert list(gts.keys()) == list(res.keys())
        for i in gts:
            assert len(res[i]) == 1 and len(gts[i]) == 1
        scores = cider_scores([_words(res[i][0]) for i in gts], [_words(gts[i][0]) for i in gts], self._n, self._sigma)
        return float(np.mean(scores)) if len(scores) else float("nan"), scores


# ------------------------------------------------------------------------------------------------ array level: what the kernel sees
def scores_arrays(ids_a, off_a, ids_b, off_b, pairs, log=np.log):
    """The kernel's `scores` float64 [M, 6] and `ints` int32 [M, 9] from its own inputs (CSR streams of word ids, records as text pairs)."""
    ids_a, ids_b = np.asarray(ids_a).tolist(), np.asarray(ids_b).tolist()
    text_a = [ids_a[off_a[t]:off_a[t + 1]] for t in range(len(off_a) - 1)]
    text_b = [ids_b[off_b[t]:off_b[t + 1]] for t in range(len(off_b) - 1)]
    M = len(pairs)
    scores, ints = np.zeros((M, 6), dtype=np.float64), np.zeros((M, 9), dtype=np.int32)
    for m, (h, r) in enumerate(np.asarray(pairs).tolist()):
        bleu, correct = bleu_pair(text_a[h], text_a[r])
        rouge, length = rouge_pair(text_b[h], text_b[r])
        scores[m, :4], scores[m, 4] = bleu, rouge
        ints[m] = [len(text_a[h]), len(text_a[r]), *correct, length, len(text_b[h]), len(text_b[r])]
    if M:
        scores[:, 5] = cider_scores([text_a[h] for h, _ in pairs], [text_a[r] for _, r in pairs], log=log)
    return scores, ints


def study_means(scores, order, study_off):
    """-> (study [S, C], avg [C]): the mean over the records of each study, then over the studies"""
    S = len(study_off) - 1
    study = np.array([np.asarray(scores)[np.asarray(order)[study_off[s]:study_off[s + 1]]].mean(0) for s in range(S)],
                     dtype=np.float64).reshape(S, np.asarray(scores).shape[1])
    return study, study.mean(0)


def stage(predictions, labels):
    """Texts (already blank-collapsed) -> the kernel's staging: every distinct text once, one word dict, both token streams.
    -> dict(ids_a, off_a, ids_b, off_b, pairs, ref_mult), all int32"""
    texts, words = {}, {}
    pairs = np.array([[texts.setdefault(p, len(texts)), texts.setdefault(l, len(texts))] for p, l in zip(predictions, labels)],
                     dtype=np.int32).reshape(-1, 2)
    streams = []
    for sep in (None, " "):
        ids, off = [], [0]
        for t in texts:
            ids += [words.setdefault(w, len(words)) for w in t.split(sep)]
            off.append(len(ids))
        streams += [np.array(ids, dtype=np.int32), np.array(off, dtype=np.int32)]
    ref_mult = np.bincount(pairs[:, 1], minlength=len(texts)).astype(np.int32)
    return dict(ids_a=streams[0], off_a=streams[1], ids_b=streams[2], off_b=streams[3], pairs=pairs, ref_mult=ref_mult)


# tolerances (tests/test_coco_nlg_gpu.py derives them): BLEU / ROUGE rtol 1e-12 with no atol; CIDEr rtol 32 * M * 2^-52 with atol 1e-14
def cider_rtol(M):
    return 32.0 * max(M, 1) * 2.0 ** -52


def assert_scores_close(got, want, M, what):
    """Columns 0..4 (BLEU, ROUGE) at rtol 1e-12 / atol 0, column 5 (CIDEr) at rtol 32 * M * 2^-52 / atol 1e-14; zeros are exact zeros on both sides."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, 6), np.asarray(want, dtype=np.float64).reshape(-1, 6)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got == 0.0, want == 0.0), f"{what}: zeros differ at {np.argwhere((got == 0.0) != (want == 0.0))[:5].tolist()}"
    np.testing.assert_allclose(got[:, :5], want[:, :5], rtol=1e-12, atol=0.0, err_msg=f"{what}: bleu / rouge")
    np.testing.assert_allclose(got[:, 5], want[:, 5], rtol=cider_rtol(M), atol=1e-14, err_msg=f"{what}: cider")


# ------------------------------------------------------------------------------------------------ fixture cases -> records
def case_records(case):
    """The scored records of a recorded case, the way the reference forms them (dicts keyed by the DICOM / study id: the last record's texts at
    the first one's position; blanks collapsed) -> dict(prediction, label, key, study_id, order, study_off, studies); the studies in the order the
    means take them (sorted when accumulating)."""
    import re
    acc = case["accumulate_over_dicoms"]
    pred, lab, sid = {}, {}, {}
    for c in case["calls"]:
        for i, k in enumerate(c["dicom_ids"] if acc else c["study_ids"]):
            pred[k] = re.sub(" +", " ", c["predictions"][i])
            lab[k] = re.sub(" +", " ", c["labels"][i][0])
            sid.setdefault(k, c["study_ids"][i])
    keys = list(pred)
    studies = sorted(set(sid.values())) if acc else list(dict.fromkeys(sid.values()))
    rank = {s: i for i, s in enumerate(studies)}
    group = np.array([rank[sid[k]] for k in keys], dtype=np.int64)
    return {"prediction": [pred[k] for k in keys], "label": [lab[k] for k in keys], "key": keys, "study_id": [sid[k] for k in keys],
            "order": np.argsort(group, kind="stable").astype(np.int32), "studies": studies,
            "study_off": np.concatenate([[0], np.cumsum(np.bincount(group, minlength=len(studies)))]).astype(np.int32)}


def case_expected(case):
    """What the reference recorded for a case, as arrays over the six device columns (NaN where the case did not ask for a column):
    -> (scores [M, 6] from the CSV rows, avg [6] from the returned dict)"""
    cols = case["csv"]["columns"]
    rows = case["csv"]["rows"]
    scores = np.full((len(rows), 6), np.nan)
    avg = np.full(6, np.nan)
    res = dict(case["result"])
    for j, c in enumerate(COLUMNS):
        if c in cols:
            scores[:, j] = [r[cols.index(c)] for r in rows]
            avg[j] = res[c]
    return scores, avg


# ------------------------------------------------------------------------------------------------ the large synthetic case
def large_case(seed=0, M=3000, n_labels=700, vocab=80000, max_len=400):
    """Kernel inputs at the size of a test epoch, as word ids: `n_labels` distinct label texts shared by M records (ref_mult > 1), words drawn
    from a Zipf law over a vocabulary above 65 535 whose frequent words sit anywhere in the id range (16-bit packing of ids would collide),
    lengths 0..max_len on both sides, hypotheses that are noisy copies of their labels (words dropped, replaced, inserted) so that n-grams of every
    order match, some empty. The split(" ") stream repeats the split() stream with the empty token (id `vocab`) where str.split(" ") has one:
    alone in an empty text, now and then after the last word. Records are grouped into studies of 1-3, the studies' records interleaved.
    -> dict(ids_a, off_a, ids_b, off_b, pairs, ref_mult, order, study_off), all int32"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(vocab)

    def words(n):
        return perm[np.minimum(rng.zipf(1.25, size=n), vocab) - 1]

    labels = [words(int(rng.integers(0, max_len + 1))) for _ in range(n_labels)]
    label_of = rng.integers(0, n_labels, size=M)
    label_of[:n_labels] = rng.permutation(n_labels)[:M]                   # every label is used
    texts, pairs, label_text = [], [], {}
    for m in range(M):
        lab = labels[label_of[m]]
        u = rng.random(len(lab))
        hyp = np.where(u < 0.15, words(len(lab)), lab)[u > 0.1]           # 10% of the words dropped, 15% replaced
        if len(hyp) and rng.random() < 0.5:                               # a few words inserted
            at = int(rng.integers(0, len(hyp)))
            hyp = np.concatenate([hyp[:at], words(int(rng.integers(1, 6))), hyp[at:]])
        if rng.random() < 0.02:
            hyp = hyp[:0]
        if int(label_of[m]) not in label_text:
            label_text[int(label_of[m])] = len(texts)
            texts.append(lab)
        pairs.append((len(texts), label_text[int(label_of[m])]))
        texts.append(hyp[:max_len])
    ids_a, off_a, ids_b, off_b = [], [0], [], [0]
    for t in texts:
        ids_a += t.tolist()
        off_a.append(len(ids_a))
        ids_b += t.tolist() + ([vocab] if len(t) == 0 or rng.random() < 0.1 else [])
        off_b.append(len(ids_b))
    pairs = np.array(pairs, dtype=np.int32).reshape(-1, 2)
    sizes = []
    while sum(sizes) < M:
        sizes.append(min(int(rng.integers(1, 4)), M - sum(sizes)))
    group = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))      # record -> study
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    return dict(ids_a=i32(ids_a), off_a=i32(off_a), ids_b=i32(ids_b), off_b=i32(off_b), pairs=pairs,
                ref_mult=np.bincount(pairs[:, 1], minlength=len(texts)).astype(np.int32), order=i32(np.argsort(group, kind="stable")),
                study_off=i32(np.concatenate([[0], np.cumsum(sizes)])))


def ulp_shifted_log(sign_of):
    """A logarithm off by one ulp: log(x) moved up or down by one ulp according to sign_of(x) in {-1, 0, +1} -- a function of x alone, as any real
    implementation's error is. The kernel's `log` may differ from numpy's by that much at every argument."""
    def log(x):
        v = np.log(x)
        s = sign_of(x)
        return np.nextafter(v, np.inf) if s > 0 else np.nextafter(v, -np.inf) if s < 0 else v
    return log
