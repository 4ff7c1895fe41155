"""float64 reference of scaled-dot-product attention (head_dim 64) and of its backward, written from the operation's definition, with the
per-element error bounds of the HIP kernels and the seeded input families of tests/test_attention_fp64_gpu.py. CPU only (torch / numpy).

Layout: tensors are bf16 [B, T, H*64] as the kernels take them; every float64 array here is [B, H, T, 64] (or [B, H, Tq, Tk]).

Visibility   vis[b, i, j] = kpm[b, j] != 0  and  (not causal or j <= i + causal_shift). A query row WITHOUT a visible key attends uniformly to
             all Tk keys in the forward (the kernels' finite "masked" score, like finfo.min in the reference model) and contributes nothing to
             the backward (see attention_bwd.hip); forward() / backward() follow that.

Bounds       Let u = 2^-24 (half an fp32 step, relative) and, per query row, s2abs = scale*log2(e) * max_j sum_d |q_d k_jd| over its visible keys.
  eps2  = 23 u s2abs                      error of a score in the exp2 domain. The 64 products of bf16 values are exact in fp32; they are summed by
                                          four chained MFMAs of 16 terms, each taken as no worse than a pairwise fp32 sum of its 16 products
                                          (depth 4) plus the addition to the accumulator: 20 roundings (the VALU decode kernel: 8 chained
                                          additions and a 3-step butterfly); then the multiplication by scale*log2(e), the subtraction of the
                                          running maximum, one to spare
  depth(T) = 32 + T/8                     longest chain of fp32 additions that any kernel here applies to T terms (per-lane sums of 8..32 terms,
                                          one chained MFMA per 16 terms, one rescale per 32, the lane / wave / split merges)
  eta   = expm1(2 ln2 eps2) + 2^-21 + 2 depth(Tk) u
                                          relative error of a probability: with every score within eps2 the softmax ratio moves by at most
                                          e^(2 ln2 eps2); exp2 itself and the reciprocal are good to an fp32 step each; the sums to depth*u
  context:  tol = (2^-8 + 2 eta) A        A[i,d] = sum_j p_ij f_ij |v_jd|. The MFMA kernels round the (dropout-scaled) probability to bf16 before
                                          P.V: half a bf16 step, 2^-8 relative, per term; the VALU decode kernel keeps it in fp32 (no 2^-8 term).
                                          eta enters twice, for the numerator and for the denominator. The bf16 rounding of the output itself is
                                          what assert_bf16_bracket allows.
  LSE:      tol = ln sum_j p_j e^(ln2 eps2_j) + 2^-22 + depth(Tk) u  (+ 4 fp32 steps of |ref| in assert_f32_bound)
                                          eps2_j = 23 u scale log2(e) sum_d |q_d k_jd| of key j: with score errors d_j the log-sum-exp moves by
                                          ln sum_j p_j e^(d_j), the error of a key weighs as much as the key; exp2 and log2 to an fp32 step; the sum of
                                          positive terms to depth*u relative = absolute in the logarithm; the steps of |ref| are the roundings of
                                          m + log2(l) and of the product with ln2.
  backward, from the kernel's own inputs (q, k, v, bf16 O, dO, fp32 LSE):
    eps2' = eps2 + 3 u (|LSE| log2(e) + s2abs)      the LSE is multiplied by log2(e) and subtracted in fp32
    eta_p = expm1(ln2 eps2') + 2^-22                 relative error of the recomputed P
    dV:  tol = sum_i (2^-8 + eta_p + depth(Tq) u) p f |dO|                      (P f is rounded to bf16 before dO^T.P)
    E_ij = p_ij [ (2^-8 + eta_p + 4u) |f dP - Delta| + 67 u (f sum_d |dO v| + sum_d |dO O|) ]
                                          error of one dS entry: P's error and the bf16 rounding of dS on the exact value, plus the fp32
                                          accumulation errors of dP = dO.V and of Delta = rowsum(dO O), which do not cancel with it
    dK:  tol = scale sum_i (E + (depth(Tq) + 2) u |dS|) |q|        dQ:  tol = scale sum_j (E + (depth(Tk) + 2) u |dS|) |k|
"""
import math

import numpy as np
import torch

BF = torch.bfloat16
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
U = 2.0 ** -24
HALF_BF16 = 2.0 ** -8
N_SCORE = 23.0                                                         # roundings behind a score (module docstring)
POISON_Q, POISON_K, POISON_V, POISON_DIM = 8.0, 80.0, 4096.0, 63       # scale 0.125: a poisoned key scores 80 natural-log units
NAN_BF16 = 0x7FA5                                                      # int16 pattern of a bf16 NaN


def heads64(t, H):
    """bf16 / float [B, T, H*64] -> float64 numpy [B, H, T, 64]"""
    B, T, D = t.shape
    assert D == H * 64
    return t.detach().cpu().double().view(B, T, H, 64).permute(0, 2, 1, 3).contiguous().numpy()


def tokens(a):
    """float64 [B, H, T, 64] -> [B, T, H*64]"""
    B, H, T, _ = a.shape
    return np.ascontiguousarray(a.transpose(0, 2, 1, 3)).reshape(B, T, H * 64)


def depth(T):
    return 32.0 + T / 8.0


# ------------------------------------------------------------------------------------------------ masks
def edge_positions(Tk):
    """keys 0, Tk-1 and both sides of every 32-key word edge (31 | 32, 63 | 64, ...)"""
    p = {0, Tk - 1}
    for w in range(32, Tk, 32):
        p.update((w - 1, w))
    return sorted(x for x in p if 0 <= x < Tk)


def listed_positions(Tk):
    """the key positions every needle case must aim at: 0, 31, 32, 63, 64 and Tk - 1"""
    return sorted({p for p in (0, 31, 32, 63, 64, Tk - 1) if 0 <= p < Tk})


def make_kpm(B, Tk, half=True, skip=()):
    """uint8 [B, Tk], 1 = attend. Image 0: the second half of the row is padding (whole tiles to skip). Images 1..: SINGLE keys masked at the edge
    positions, dealt out in turn so that the two sides of an edge fall into different images. Needs B >= 3 and Tk >= 2. skip: positions left alone
    (key 0 under a causal mask with shift 0, where it is the only key that query 0 sees)."""
    assert B >= 3 and Tk >= 2
    kpm = torch.ones(B, Tk, dtype=torch.uint8)
    if half:
        kpm[0, Tk // 2:] = 0
    for n, p in enumerate(edge_positions(Tk)):
        if p not in skip:
            kpm[1 + n % (B - 1), p] = 0
    assert bool((kpm.sum(1) > 0).all())
    return kpm


def flipped_positions(kpm):
    """key positions that are masked as a single key (both neighbours attend) in some image"""
    k = kpm.numpy() != 0
    Tk = k.shape[1]
    left = np.concatenate([np.ones((k.shape[0], 1), bool), k[:, :-1]], 1)
    right = np.concatenate([k[:, 1:], np.ones((k.shape[0], 1), bool)], 1)
    return set(np.nonzero((~k & left & right).any(0))[0].tolist()) if Tk > 1 else set()


def visibility(B, Tq, Tk, kpm=None, causal=False, shift=0):
    vis = np.ones((B, Tq, Tk), bool)
    if kpm is not None:
        vis &= (kpm.cpu().numpy() != 0)[:, None, :]
    if causal:
        vis &= (np.arange(Tk)[None, :] <= np.arange(Tq)[:, None] + shift)[None]
    return vis


# ------------------------------------------------------------------------------------------------ input families
def needle_targets(vis, H, causal, shift):
    """t[b, h, i]: the key that query (b, h, i) is aimed at. Walks the queries in order and gives each the first key position (0, 31, 32, 63, 64, Tk-1, then the other word edges, then the rest) that no
    query has been aimed at yet and that this query sees; then cycles. Causal: the LAST such key (the fewest rows see it; the first time round that
    is the diagonal key i + shift) after the six listed ones, and every third row is aimed at the HIDDEN key just past its diagonal (a leak of it would dominate the row).
    -> (targets, set of positions that are some query's visible target)"""
    B, Tq, Tk = vis.shape
    first = listed_positions(Tk) + [p for p in edge_positions(Tk) if p not in listed_positions(Tk)]
    order = first + [p for p in range(Tk) if p not in set(first)]
    rank = np.empty(Tk, np.int64)
    rank[order] = np.arange(Tk)
    todo = np.ones(Tk, bool)
    nlisted = len(listed_positions(Tk))
    t = np.zeros((B, H, Tq), np.int64)
    n = 0
    for b in range(B):
        for h in range(H):
            for i in range(Tq):
                row = vis[b, i]
                n += 1
                d = i + shift
                if causal and i % 3 == 1 and d + 1 < Tk:
                    t[b, h, i] = d + 1
                    continue                                         # hidden: does not count as covered
                else:
                    cand = np.nonzero(row & todo)[0]
                    if cand.size:
                        must = cand[rank[cand] < nlisted]
                        t[b, h, i] = (must[-1] if must.size else cand[-1]) if causal else cand[np.argmin(rank[cand])]
                    else:
                        seen = np.nonzero(row)[0]
                        t[b, h, i] = seen[(7 * n) % seen.size] if seen.size else (7 * n) % Tk
                if row[t[b, h, i]]:
                    todo[t[b, h, i]] = False
    return t, set(np.nonzero(~todo)[0].tolist())


def make_inputs(family, B, H, Tq, Tk, kpm=None, causal=False, shift=0, poison=False, seed=0, Bq=None):
    """-> dict(q [Bq, Tq, D], k, v [B, Tk, D] bf16 CPU, covered = the needle's visibly targeted key positions | None).
    family: gauss | needle | ramp | ramp_down. Bq = B * share for the decode kernels (query row b + g*B reads K/V row b).
    poison: head dimension 63 is POISON_Q in every query, POISON_K in every key that NO query of its image may see (key-padding mask, or causally
    beyond the last query) and 0 in the others; those keys carry V = POISON_V. Their score is 80 natural-log units, far above every visible one.
    With B <= 3 images, dimension 60 + b is POISON_K in every key of image b and POISON_Q in the queries of the OTHER images (0 in its own): a key
    read from another image's rows scores 80 units above the image's own keys."""
    Bq = Bq or B
    share = Bq // B
    g = torch.Generator().manual_seed(1000 * seed + 17 * Tq + Tk + (3 if causal else 0))
    D = H * 64
    k = torch.randn(B, Tk, D, generator=g)
    v = torch.randn(B, Tk, D, generator=g)
    q = torch.randn(Bq, Tq, D, generator=g)
    vis = visibility(B, Tq, Tk, kpm, causal, shift)
    covered = None
    if family in ("ramp", "ramp_down"):
        # scores = scale * 8 * ramp_j (+ small noise): -40 .. +40 natural-log units over the keys with scale 0.125; dimension 0 of each head
        r = torch.linspace(-40.0, 40.0, Tk) if Tk > 1 else torch.zeros(1)
        r = r if family == "ramp" else -r
        k = 0.5 * k
        q = 0.25 * q
        k.view(B, Tk, H, 64)[..., 0] = r.view(1, Tk, 1)
        q.view(Bq, Tq, H, 64)[..., 0] = 8.0
    k = k.to(BF)
    if family == "needle":
        kh = k.float().view(B, Tk, H, 64)
        qh = q.view(Bq, Tq, H, 64)
        vis_q = np.concatenate([vis] * share, 0)
        t, covered = needle_targets(vis_q, H, causal, shift)
        for b in range(Bq):
            for h in range(H):
                qh[b, :, h] = kh[b % B, torch.as_tensor(t[b, h]), h] + 0.25 * qh[b, :, h]
    if poison:
        dead = ~vis.any(1)                                           # [B, Tk]: no query of the image sees the key
        dead &= vis.any(2).any(1)[:, None]                           # (an image whose every key is masked keeps ordinary keys: uniform rows)
        dead = torch.as_tensor(dead)
        kh, vh = k.view(B, Tk, H, 64), v.view(B, Tk, H, 64)
        kh[..., POISON_DIM] = 0
        kh[..., POISON_DIM] = torch.where(dead.view(B, Tk, 1), torch.tensor(POISON_K, dtype=BF), kh[..., POISON_DIM])
        vh[dead] = POISON_V
        q.view(Bq, Tq, H, 64)[..., POISON_DIM] = POISON_Q
        if 1 < B <= 3:
            kh[..., 60:63] = 0
            q.view(Bq, Tq, H, 64)[..., 60:63] = 0
            for b in range(B):
                kh[b, :, :, 60 + b] = POISON_K
                for bq in range(Bq):
                    if bq % B != b:
                        q.view(Bq, Tq, H, 64)[bq, :, :, 60 + b] = POISON_Q
    return dict(q=q.to(BF), k=k, v=v.to(BF), covered=covered, vis=vis)


def grad_output(Bq, Tq, D, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    return torch.randn(Bq, Tq, D, generator=g).to(BF)


# ------------------------------------------------------------------------------------------------ forward
def forward(q, k, v, H, scale, vis, fac=None, mfma=True, share=1, q_err=None):
    """q [Bq, Tq, D], k / v [B, Tk, D] bf16, vis bool [B, Tq, Tk], fac = dropout factor float [Bq, H, Tq, Tk] | None.
    q_err [Bq, Tq, D] | None: elementwise bound on the error of the query the kernel really uses (project_query): its scores then differ by at
    most eps_q = scale max_j sum_d q_err_d |k_jd|, every probability by a factor within e^(+-2 eps_q), the context by expm1(2 eps_q) A.
    -> dict of float64 arrays: P [Bq,H,Tq,Tk], O, tol_O, A [Bq,Tq,D], LSE, tol_LSE [Bq,H,Tq]"""
    Q, K, V = heads64(q, H), np.concatenate([heads64(k, H)] * share, 0), np.concatenate([heads64(v, H)] * share, 0)
    vis = np.concatenate([vis] * share, 0)[:, None]                  # [Bq, 1, Tq, Tk]
    Tk = K.shape[2]
    S = scale * (Q @ K.transpose(0, 1, 3, 2))
    none = ~vis.any(-1, keepdims=True)                               # rows without a visible key: uniform over all Tk keys
    live = vis | none
    Sm = np.where(live, np.where(none, 0.0, S), -np.inf)
    m = Sm.max(-1, keepdims=True)
    e = np.exp(Sm - m)
    l = e.sum(-1, keepdims=True)
    P = e / l
    LSE = (m + np.log(l))[..., 0]
    LSE = np.where(none[..., 0], (-1.0e30 + np.log2(Tk)) * LN2, LSE)         # what the kernels' finite sentinel gives
    Pf = P if fac is None else P * np.asarray(fac, np.float64)
    QE = np.zeros_like(Q) if q_err is None else heads64(torch.as_tensor(q_err), H)
    s2abs = scale * LOG2E * np.where(vis, (np.abs(Q) + QE) @ np.abs(K).transpose(0, 1, 3, 2), 0.0).max(-1)     # [Bq, H, Tq]
    eps2 = N_SCORE * U * s2abs
    eta = np.expm1(2.0 * LN2 * eps2) + 2.0 ** -21 + 2.0 * depth(Tk) * U
    eps_q = scale * np.where(vis, QE @ np.abs(K).transpose(0, 1, 3, 2), 0.0).max(-1)
    A = Pf @ np.abs(V)
    tol_O = ((HALF_BF16 if mfma else 0.0) + 2.0 * eta + np.expm1(2.0 * eps_q))[..., None] * A
    eps2_j = N_SCORE * U * scale * LOG2E * np.where(vis, (np.abs(Q) + QE) @ np.abs(K).transpose(0, 1, 3, 2), 0.0)
    tol_LSE = np.log((P * np.exp(LN2 * eps2_j)).sum(-1)) + 2.0 ** -22 + depth(Tk) * U
    return dict(P=P, Pf=Pf, S=S, O=tokens(Pf @ V), A=tokens(A), tol_O=tokens(tol_O), LSE=LSE, tol_LSE=tol_LSE, eps2=eps2, s2abs=s2abs,
                vis=np.broadcast_to(vis & ~none, P.shape), Q=Q, K=K, V=V)


def project_query(raw, w, gamma, beta, bias, eps):
    """q = LayerNorm(raw; gamma, beta, eps) @ w^T + bias in float64, and the bound on the error of the bf16 query that attn_cross_mfma_kernel<.., QPROJ>
    forms from the packed operands. raw bf16 [M, K], w bf16 [N, K], gamma / beta / bias fp32. gamma must hold powers of two, so that the folded weight
    W' = w diag(gamma) is exact in bf16 and the only bf16 rounding is that of q itself. The kernel computes rstd (sum_k W'_nk x_k - mean colsum_n) +
    bias'_n in fp32: <= 800 additions behind each of the two sums (768 terms, 12 wave partials, the epilogue), <= 120 behind the mean (relative to
    mean |x|), 200 u relative on rstd and the epilogue's products; then q is rounded to bf16 (2^-9 relative). -> (q, q_err) float64 [M, N]"""
    x, W = raw.double().numpy(), w.double().numpy()
    g, b, c = (t.double().numpy() for t in (gamma, beta, bias))
    assert np.all(np.log2(g) == np.round(np.log2(g)))
    mean = x.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(x.var(1, keepdims=True) + eps)
    Wf = W * g[None, :]
    q = ((x - mean) * rstd) @ Wf.T + (W @ b + c)[None, :]
    pre = U * rstd * (800.0 * (np.abs(x) @ np.abs(Wf).T) + 800.0 * np.abs(mean) * np.abs(Wf).sum(1)[None, :]
                      + 120.0 * np.abs(x).mean(1, keepdims=True) * np.abs(Wf.sum(1))[None, :])
    pre = pre + 200.0 * U * (np.abs(q) + np.abs(W @ b + c)[None, :]) + 800.0 * U * (np.abs(W) @ np.abs(b))[None, :]
    return q, pre + 2.0 ** -9 * (np.abs(q) + pre)


# ------------------------------------------------------------------------------------------------ backward
def backward(q, k, v, o, do, lse, H, scale, vis, fac=None):
    """From the kernel's inputs: q, k, v, o (the bf16 context), do bf16 [B, T, D], lse fp32 [B, H, Tq]. -> dict of float64 [B, T, D]:
    dq, dk, dv and tol_dq, tol_dk, tol_dv (module docstring)."""
    Q, K, V, O, dO = (heads64(t, H) for t in (q, k, v, o, do))
    Tq, Tk = Q.shape[2], K.shape[2]
    L = lse.detach().cpu().double().numpy()[..., None]
    vis = vis[:, None]
    S = scale * (Q @ K.transpose(0, 1, 3, 2))
    P = np.where(vis, np.exp(np.minimum(S - L, 700.0)), 0.0)
    f = 1.0 if fac is None else np.asarray(fac, np.float64)
    Pf = P * f
    dP = dO @ V.transpose(0, 1, 3, 2)
    delta = (dO * O).sum(-1, keepdims=True)
    dS = P * (f * dP - delta)
    dV, dK, dQ = Pf.transpose(0, 1, 3, 2) @ dO, scale * (dS.transpose(0, 1, 3, 2) @ Q), scale * (dS @ K)
    s2abs = scale * LOG2E * np.where(vis, np.abs(Q) @ np.abs(K).transpose(0, 1, 3, 2), 0.0).max(-1, keepdims=True)
    eps2 = N_SCORE * U * s2abs + 3.0 * U * (np.abs(L) * LOG2E + s2abs)
    eta_p = np.where(vis.any(-1, keepdims=True), np.expm1(LN2 * np.minimum(eps2, 1.0)) + 2.0 ** -22, 0.0)        # (no visible key: P = 0 exactly)
    tol_dV = ((HALF_BF16 + eta_p + depth(Tq) * U) * Pf).transpose(0, 1, 3, 2) @ np.abs(dO)
    E = P * ((HALF_BF16 + eta_p + 4.0 * U) * np.abs(f * dP - delta)
             + 67.0 * U * (f * (np.abs(dO) @ np.abs(V).transpose(0, 1, 3, 2)) + np.abs(dO * O).sum(-1, keepdims=True)))
    tol_dK = scale * ((E + (depth(Tq) + 2.0) * U * np.abs(dS)).transpose(0, 1, 3, 2) @ np.abs(Q))
    tol_dQ = scale * ((E + (depth(Tk) + 2.0) * U * np.abs(dS)) @ np.abs(K))
    return dict(dq=tokens(dQ), dk=tokens(dK), dv=tokens(dV), tol_dq=tokens(tol_dQ), tol_dk=tokens(tol_dK), tol_dv=tokens(tol_dV),
                sum_dv=tokens(np.abs(Pf).transpose(0, 1, 3, 2) @ np.abs(dO)), sum_dk=tokens(scale * (np.abs(dS).transpose(0, 1, 3, 2) @ np.abs(Q))),
                sum_dq=tokens(scale * (np.abs(dS) @ np.abs(K))))


def f32_ratio(out, ref, tol, ulps):
    """largest |out - ref| / (tol + ulps fp32 steps of |ref|): the figure that goes with assert_f32_bound"""
    o = out.detach().cpu().double().numpy().ravel()
    r = np.asarray(ref, np.float64).ravel()
    step = np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(o - r) / (np.broadcast_to(np.asarray(tol, np.float64), ref.shape).ravel() + ulps * step)))


def bf16_figures(out, ref, tol):
    """-> (largest |out - ref| as a fraction of the half-width of assert_bf16_bracket's bracket, largest fraction of `tol` that is needed to
    explain an element once half a bf16 step at the output, its own rounding, is taken off). Elements with ref == tol == 0 must be 0 and count as 0."""
    from bounds_util import bf16_ceil, bf16_floor
    o = out.detach().float().cpu().double().numpy().ravel()
    r = np.asarray(ref, np.float64).ravel()
    t = np.broadcast_to(np.asarray(tol, np.float64), np.asarray(ref).shape).ravel()
    err = np.abs(o - r)
    half = np.maximum(bf16_ceil(r + t) - r, r - bf16_floor(r - t))
    frac = np.where(half > 0, err / np.where(half > 0, half, 1.0), 0.0)
    step = np.where(o != 0, 2.0 ** (np.floor(np.log2(np.where(o != 0, np.abs(o), 1.0))) - 8.0), 0.0)
    need = np.maximum(err - step, 0.0)
    used = np.where(t > 0, need / np.where(t > 0, t, 1.0), 0.0)
    return float(frac.max()), float(used.max())
