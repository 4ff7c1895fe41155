"""GPU: the small C-ABI kernels (casts, copy / reduction plumbing, log-softmax, top-k, cosine, segment argmax, decode-step inputs) against
float64 references computed from the exact inputs the kernel saw. Exact operations are compared bit for bit; the others get elementwise
bounds derived from the output's rounding. Every output lives inside a larger buffer filled with a sentinel bit pattern (padding before and
after, row gaps, rows / columns the call must not touch) and every sentinel must be bit-unchanged after the call."""
import numpy as np
import pytest
import torch
from bounds_util import Guarded, all_bf16, assert_bf16_bracket, bf16_ceil, bits, gelu64, ulp32

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
I64 = torch.int64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import ops as _ops
    from cxrmate_amd._lib import LIB
    LIB.load()
    return _ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ casts
LENGTHS = [1, 3, 4, 5, 1023, 1025, 8192 * 1024 + 13]           # the last one is past one grid-stride pass of both cast kernels


def test_cast_bf16_to_f32_is_the_bit_shift_of_every_pattern(ops):
    x = all_bf16(finite=False)
    g = Guarded.flat(x.numel(), F32)
    ops.cast_to_f32(x.cuda(), g.view)
    g.check("bf16->f32 all patterns")
    exp = x.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).bitwise_left_shift(16)
    assert torch.equal(bits(g.view), exp)                           # every pattern, NaNs and their payloads included
    assert torch.isnan(g.view[torch.isnan(x.float()).cuda()]).all()


@pytest.mark.parametrize("n", LENGTHS)
def test_cast_bf16_to_f32_lengths(ops, n):
    x = torch.randint(-32768, 32768, (n,), generator=_gen(n), dtype=torch.int32).to(torch.int16).view(BF)
    g = Guarded.flat(n, F32)
    ops.cast_to_f32(x.cuda(), g.view)
    g.check(f"bf16->f32 n={n}")
    assert torch.equal(bits(g.view), x.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).bitwise_left_shift(16))


def _f32_edge_patterns():
    p = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x7F7E, 0x0001, 0x0080, 0xC2F6):     # even / odd last kept bit, normal, denormal, negative
        p += [(hi << 16) | lo for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)]
    p += [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000, 0x00400000,   # +-0, fp32 denormals
          0x7F800000, 0xFF800000,                                                                                      # +-inf
          0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F7FFF, 0xFF7F8000, 0xFF7FFFFF, 0x7F7F0000]                          # around overflow to inf
    return np.array(p, dtype=np.uint32)


def test_cast_f32_to_bf16_rounding_matches_torch(ops):
    r = torch.randint(0, 2 ** 32, (1 << 20,), generator=_gen(1), dtype=I64).to(torch.int32)
    edge = torch.from_numpy(_f32_edge_patterns().view(np.int32))
    nan = torch.tensor([0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FFFFFFF, 0x7F80FFFF], dtype=I64).to(torch.int32)
    x = torch.cat([edge, r, nan]).view(F32)
    g = Guarded.flat(x.numel(), BF)
    ops.cast_to_bf16(x.cuda(), g.view)
    g.check("f32->bf16")
    out = g.view.cpu()
    isn = torch.isnan(x)
    # NaN stays NaN (its payload is the hardware's business); everything else is round-to-nearest-even, bit for bit
    assert torch.isnan(out.float()[isn]).all()
    ref = x[~isn].to(BF)
    diff = (bits(out[~isn]) != bits(ref)).nonzero()
    assert diff.numel() == 0, [(hex(int(x[~isn].view(torch.int32)[i]) & 0xFFFFFFFF), hex(int(bits(out[~isn])[i]) & 0xFFFF)) for i in diff[:5, 0]]


@pytest.mark.parametrize("n", LENGTHS)
def test_cast_f32_to_bf16_lengths(ops, n):
    x = torch.randn(n, generator=_gen(n)) * 3
    x[:: 7] = (x[:: 7].to(BF).float().view(torch.int32) | 0x8000).view(F32)       # exact ties
    g = Guarded.flat(n, BF)
    ops.cast_to_bf16(x.cuda(), g.view)
    g.check(f"f32->bf16 n={n}")
    assert torch.equal(bits(g.view), bits(x.to(BF)))


# ------------------------------------------------------------------------------------------------ copy / reduction plumbing (bit-exact)
def _rbf(*shape, seed=0):
    return torch.randn(*shape, generator=_gen(seed)).to(BF)


@pytest.mark.parametrize("rows,C,ldo", [(5, 8, 24), (3, 768, 776), (22000, 768, 768)])       # the last: > 8192 * 256 vector chunks
def test_add_bf16(ops, rows, C, ldo):
    a, b = _rbf(rows, C, seed=1), _rbf(rows, C, seed=2)
    ref = (a.float() + b.float()).to(BF)
    g = Guarded.rows(rows, C, BF, ld=ldo)
    ops.add(a.cuda(), b.cuda(), out=g.view)
    g.check(f"add {rows}x{C}")
    assert torch.equal(bits(g.view), bits(ref))
    # in place (out is a), on a strided view
    ga = Guarded.rows(rows, C, BF, ld=ldo)
    ga.view.copy_(a.cuda())
    torch.cuda.synchronize()
    ops.add(ga.view, b.cuda(), out=ga.view)
    ga.check(f"add in place {rows}x{C}")
    assert torch.equal(bits(ga.view), bits(ref))


@pytest.mark.parametrize("B,L,C,case", [(3, 20, 768, "cls"), (4, 9, 64, "cache"), (8, 3000, 768, "big")])
def test_copy_rows_bf16(ops, B, L, C, case):
    if case == "cls":                   # class-token concat: src [B, L, C] -> dst[:, 1:, :] of [B, L + 1, C]; and the split back
        src = _rbf(B, L, C, seed=3).cuda()
        g = Guarded((B, L + 1, C), BF, (slice(None), slice(1, None), slice(None)))
        ops.copy_rows(src, g.view)
        g.check("class-token concat")
        assert torch.equal(bits(g.view), bits(src))
        full = _rbf(B, L + 1, C, seed=4).cuda()
        g2 = Guarded((B + 1, L, C), BF, (slice(0, B), slice(None), slice(None)))
        ops.copy_rows(full[:, 1:, :], g2.view)
        g2.check("class-token split")
        assert torch.equal(bits(g2.view), bits(full[:, 1:, :]))
    elif case == "cache":               # KV-cache append: [:, past:past+Tn, :] of a [B, Tmax, C] cache
        past, Tn, Tmax = 5, 3, 12
        src = _rbf(B, Tn, C, seed=5).cuda()
        g = Guarded((B, Tmax, C), BF, (slice(None), slice(past, past + Tn), slice(None)))
        ops.copy_rows(src, g.view)
        g.check("cache append")
        assert torch.equal(bits(g.view), bits(src))
    else:                               # B * rows * C / 8 = 2.3e6 vector chunks: past the 8192-workgroup grid cap
        src = _rbf(B, L, C, seed=6).cuda()
        g = Guarded((B, L + 1, C), BF, (slice(None), slice(1, None), slice(None)))
        ops.copy_rows(src, g.view)
        g.check("copy_rows grid-stride")
        assert torch.equal(bits(g.view), bits(src))


@pytest.mark.parametrize("idx,rows", [([2, 0, 1, 3], 7), ([1, 1, 1, 0], 10), ([3, 2, 1, 0], 1), ([0, 0, 2, 2], 9)])
def test_gather_batch_bf16(ops, idx, rows):
    B, Tmax, C = 4, 10, 768
    src = _rbf(B, Tmax + 2, C, seed=7).cuda()                        # (source rows are longer: its own batch stride)
    g = Guarded((B + 1, Tmax, C), BF, (slice(0, B), slice(0, rows), slice(None)))
    dst = g.buf[:B]                                                    # rows >= `rows` of the destination stay untouched
    ops.gather_batch(src, torch.tensor(idx, device="cuda"), rows, dst)
    g.check(f"gather_batch idx={idx} rows={rows}")
    assert torch.equal(bits(g.view), bits(src[idx, :rows]))


def test_bcast_row_and_sum_row0(ops):
    B, L, C = 5, 7, 768
    row = torch.randn(C, generator=_gen(8)) * 2
    g = Guarded((B, L, C), BF, (slice(None), 0, slice(None)))
    ops.bcast_row(row.cuda(), g.buf)
    g.check("bcast_row")
    assert torch.equal(bits(g.view), bits(row.to(BF).expand(B, C)))
    # sum_row0_into accumulates into its output: out += sum_b src[b, 0, :], summed sequentially in fp32 over b
    for C in (768, 100, 1):
        src = _rbf(B, L, C, seed=9).cuda()
        start = torch.randn(C, generator=_gen(10)) * 5
        go = Guarded.flat(C, F32)
        go.view.copy_(start.cuda())
        ops.sum_row0_into(src, go.view)
        go.check(f"sum_row0 C={C}")
        s = torch.zeros(C, dtype=F32)
        for b in range(B):
            s = s + src[b, 0].float().cpu()
        assert torch.equal(bits(go.view), bits(start + s)), f"sum_row0 C={C}"


# ------------------------------------------------------------------------------------------------ GELU backward (misc.hip)
@pytest.mark.parametrize("dy_kind", ["ones", "random"])
def test_gelu_bwd_over_every_bf16(ops, dy_kind):
    u = all_bf16()
    dy = torch.ones(u.numel(), dtype=BF) if dy_kind == "ones" else _rbf(u.numel(), seed=11)
    dx = ops.gelu_bwd(dy.cuda(), u.cuda())
    _, d = gelu64(u.double())
    dyd = dy.double().numpy()
    err = assert_bf16_bracket(dx, dyd * d, 1.1e-4 * np.abs(dyd), f"gelu_bwd dy={dy_kind}")
    print(f"MEASURED gelu_bwd dy={dy_kind}: max |err| / bracket half-width {err:.3f}")


# ------------------------------------------------------------------------------------------------ log_softmax_rows_
def _log_softmax_case(V, seed):
    g = _gen(seed)
    R = 6
    x = torch.randn(R, V, generator=g, dtype=torch.float64) * 4
    if V > 1:
        x[1, torch.randperm(V, generator=g)[: max(1, V // 3)]] = -np.inf       # banned tokens
        x[1, 0] = 2.0
    x[2] += 1e4
    x[3] -= 1e4
    x[4, -1] = x[4].max() + 3.0                                                   # maximum in the last column
    if V > 2:
        x[5, : V // 2] = -np.inf
    return x.float()


@pytest.mark.parametrize("V", [1, 255, 257, 30000])
@pytest.mark.parametrize("with_add", [False, True])
def test_log_softmax_rows(ops, V, with_add):
    x = _log_softmax_case(V, V)
    R = x.shape[0]
    add = (torch.randn(R, generator=_gen(12)) * 3 + torch.tensor([0, 0, 1e4, -1e4, 0, 0])).float() if with_add else None
    ld = V + 13
    g = Guarded((R + 2, ld), F32, (slice(1, R + 1), slice(0, V)))
    g.buf[1:R + 1, :V] = x.cuda()
    ops.log_softmax_rows_(g.view, None if add is None else add.cuda())
    g.check(f"log_softmax V={V}")                                                  # padding columns and rows untouched
    xd = x.double()
    lse = torch.logsumexp(xd, 1, keepdim=True)
    a = add.double()[:, None] if add is not None else torch.zeros(R, 1, dtype=torch.float64)
    ref = (xd - lse + a).numpy()
    out = g.view.cpu().double().numpy()
    fin = np.isfinite(ref)
    assert np.array_equal(np.isneginf(out), ~fin), f"V={V}: -inf entries must stay -inf, and only they"
    # |out - ref| <= 8 ulp_f32(max(|x|, |off|)) + 1e-6 with off = lse - add the row's offset: the kernel subtracts one fp32 offset from x
    off = (lse - a).numpy()
    scale = np.maximum(np.abs(np.where(fin, xd.numpy(), 0.0)), np.abs(off))
    err = np.abs(np.where(fin, out - ref, 0.0))
    lim = 8 * ulp32(scale) + 1e-6
    assert (err <= lim).all(), f"V={V}: worst {float((err / lim).max()):.2f} x bound, err {float(err.max()):.3e}"
    print(f"MEASURED log_softmax V={V} add={with_add}: max |err| {float(err.max()):.3e}, max err / bound {float((err / lim).max()):.3f}")


# ------------------------------------------------------------------------------------------------ topk_rows
def _topk_direct(ops, x, K):
    from cxrmate_amd._lib import LIB
    R, n = x.shape
    gv, gi = Guarded.flat(R * K, F32), Guarded.flat(R * K, I64)
    LIB.call("cxr_topk_rows", x.data_ptr(), x.stride(0), R, n, K, gv.view.data_ptr(), gi.view.data_ptr(), ops._s())
    gv.check(f"topk values n={n} K={K}")
    gi.check(f"topk indices n={n} K={K}")
    return gv.view.view(R, K).cpu(), gi.view.view(R, K).cpu()


@pytest.mark.parametrize("n", [1, 17, 256, 257, 4 * 30000])
def test_topk_rows_equals_stable_sort(ops, n):
    g = _gen(n)
    R = 4
    x = torch.randn(R, n, generator=g)
    x[1] = torch.randint(0, 3, (n,), generator=g).float()                # many exact ties
    x[2, torch.randperm(n, generator=g)[: (n + 1) // 2]] = -np.inf        # banned entries
    x[3] = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(-np.inf), x[3].round())
    xd = torch.empty(R, n + 5).cuda()[:, :n]                              # strided rows
    xd.copy_(x.cuda())
    sv, si = torch.sort(x, dim=1, descending=True, stable=True)
    for K in sorted({1, 2, 8, 16, n} & set(range(1, min(16, n) + 1))):
        v, i = _topk_direct(ops, xd, K)
        assert torch.equal(i, si[:, :K]), f"n={n} K={K}: indices {i.tolist()} vs {si[:, :K].tolist()}"
        assert torch.equal(bits(v), bits(sv[:, :K].contiguous())), f"n={n} K={K}: values"


# ------------------------------------------------------------------------------------------------ cosine_rows
COS_ULPS = 4         # bound: 4 ulp_f32 of 1 (measured worst case: 1 ulp; the test prints it)


@pytest.mark.parametrize("C", [1, 63, 65, 128, 768])
def test_cosine_rows(ops, C):
    from cxrmate_amd._lib import LIB
    g = _gen(C)
    R = 11                                                                 # not a multiple of the 4 rows per workgroup
    a = torch.randn(R, C, generator=g, dtype=torch.float64)
    b = torch.randn(R, C, generator=g, dtype=torch.float64)
    a[0] = 0                                                               # zero row
    a[1] = torch.randn(C, generator=g, dtype=torch.float64) * 1e-40        # denormal-scale row
    b[2] = a[2] * 3.5                                                      # parallel
    b[3] = -a[3] * 0.25                                                    # antiparallel
    a[4] = torch.randn(C, generator=g, dtype=torch.float64) * 1e-6         # norms around eps
    a, b = a.float(), b.float()
    ab = torch.empty(R, C + 3).cuda()[:, :C]
    bb = torch.empty(R, 2 * C + 4).cuda()[:, C + 4:]
    ab.copy_(a.cuda())
    bb.copy_(b.cuda())
    go = Guarded.flat(R, F32)
    LIB.call("cxr_cosine_rows_f32", ab.data_ptr(), ab.stride(0), bb.data_ptr(), bb.stride(0), go.view.data_ptr(), R, C, 1e-8, ops._s())
    go.check(f"cosine C={C}")
    ref = torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=1, eps=1e-8).numpy()
    out = go.view.cpu().double().numpy()
    err = np.abs(out - ref)
    lim = COS_ULPS * float(np.spacing(np.float32(1)))
    assert (err <= lim).all(), f"C={C}: err {err.tolist()} > {lim:.3e}"
    print(f"MEASURED cosine C={C}: max |err| {float(err.max()):.3e} ({float(err.max()) / float(np.spacing(np.float32(1))):.2f} ulp of 1)")


# ------------------------------------------------------------------------------------------------ segment_argmax
CHEXBERT_OFFSETS = [4 * i for i in range(14)] + [54]                  # 13 heads of 4 classes + 1 of 2


@pytest.mark.parametrize("offsets", [CHEXBERT_OFFSETS, "random"])
def test_segment_argmax_ties_take_the_first_maximum(ops, offsets):
    from cxrmate_amd._lib import LIB
    g = _gen(13)
    if offsets == "random":
        w = torch.randint(1, 9, (30,), generator=g)
        w[::5] = 1                                                      # width-1 segments
        offsets = [0] + torch.cumsum(w, 0).tolist()
    R, nseg, W = 37, len(offsets) - 1, offsets[-1]
    x = torch.randint(-2, 2, (R, W), generator=g).float()               # planted exact ties everywhere
    x[::3] = torch.randn(R, W, generator=g)[::3]
    x[5, :] = -np.inf
    ld = W + 3
    xd = torch.empty(R, ld).cuda()[:, :W]
    xd.copy_(x.cuda())
    off = torch.tensor(offsets, dtype=torch.int32, device="cuda")
    go = Guarded.flat(R * nseg, I64)
    LIB.call("cxr_segment_argmax_f32", xd.data_ptr(), ld, off.data_ptr(), nseg, go.view.data_ptr(), R, ops._s())
    go.check("segment_argmax")
    ref = torch.stack([x[:, offsets[s]:offsets[s + 1]].argmax(1) for s in range(nseg)], 1)
    assert torch.equal(go.view.view(R, nseg).cpu(), ref)


# ------------------------------------------------------------------------------------------------ decode-step inputs (+ embeddings)
VOCAB, MASK_TOK, LMAX, C = 300, 9, 520, 768
SEC = [3, 5, 7, 11, 13]                         # token-type sections (distinct, so that an off-by-one index shows)
SP0, SP1 = [20, 21], [22, 23, 24, 25]           # separator sets of the two row halves (n0 != n1)


def _embed_tables():
    g = _gen(14)
    word = (torch.randn(VOCAB, C, generator=g) * 0.5).to(BF)
    typ = (torch.randn(16, C, generator=g) * 0.5).to(BF)
    posw = (torch.randn(512, C, generator=g) * 0.5).to(BF)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    return word, typ, posw, gamma, beta


def _step_ids(rows, strip, T, half, seed):
    """ids [rows, LMAX] with the separator / mask patterns of interest planted in the fed window [strip, strip + T)"""
    g = _gen(seed)
    ids = torch.randint(30, VOCAB, (rows, LMAX), generator=g)
    for r in range(rows):
        sp = SP0 if r < half else SP1
        win = ids[r, strip:strip + T]
        k = r % 7
        if k == 0 and T >= 1:
            win[0] = sp[0]                                              # separator at column 0
        elif k == 1 and T >= 2:
            win[T - 2] = sp[-1]                                         # at T-2: counts
        elif k == 2:
            win[T - 1] = sp[0]                                          # at T-1: the last position does not count
        elif k == 3 and T >= 3:
            win[0], win[(T - 1) // 2] = sp[-1], sp[0]                   # several: the later separator id wins
        elif k == 4:
            for j, s in enumerate(sp):
                if j < T - 1:
                    win[(j * 37) % (T - 1)] = s
        elif k == 5:
            win[torch.randperm(T, generator=g)[: T // 2]] = MASK_TOK    # mask tokens, including the chunk edges
            for e in (0, 63, 64, T - 1):
                if e < T:
                    win[e] = MASK_TOK
        # k == 6: nothing planted
        if k in (1, 3) and T > 64:
            win[63], win[64] = MASK_TOK, MASK_TOK
    return ids


def _step_refs(ids, strip, cur, half, longi):
    from oracle import token_ops
    fed = ids[:, strip:cur].numpy()
    T = cur - strip
    rows = fed.shape[0]
    tt = np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        sp = SP0 if r < half else SP1
        tt[r] = token_ops.token_ids_to_token_type_ids_past(fed[r:r + 1], sp, SEC[:len(sp) + 1])[0, 0]
    mask = (fed != MASK_TOK).astype(np.uint8)
    pos = token_ops.position_ids_from_mask(mask)[:, -1] if longi else np.full(rows, T - 1, dtype=np.int64)
    return fed[:, -1].copy(), tt, mask, pos


def _step_buffers(rows):
    return dict(new_id=Guarded.flat(rows, I64), tt=Guarded.flat(rows, I64), pos=Guarded.flat(rows, I64),
                mask=Guarded((rows + 1, LMAX), torch.uint8, (slice(0, rows), slice(None))),
                tt_hist=Guarded((rows + 1, LMAX), I64, (slice(0, rows), slice(None))),
                pos_hist=Guarded((rows + 1, LMAX), I64, (slice(0, rows), slice(None))))


def _check_step(bufs, ids, strip, cur, half, longi, what):
    new_id, tt, mask, pos = _step_refs(ids, strip, cur, half, longi)
    T = cur - strip
    rows = ids.shape[0]
    for name in ("new_id", "tt"):
        bufs[name].check(f"{what} {name}")
    assert np.array_equal(bufs["new_id"].view.cpu().numpy(), new_id), f"{what}: new_id"
    assert np.array_equal(bufs["tt"].view.cpu().numpy(), tt), f"{what}: token type"
    # histories change only in column cur; the mask only in [0, T)
    hist_cols = slice(cur, cur + 1)
    for name, ref in (("tt_hist", tt), ("pos_hist", pos if longi else None)):
        b = bufs[name]
        if ref is None:
            b.check(f"{what} {name} (unused)")
            continue
        b.mask[:rows, hist_cols] = False
        b.check(f"{what} {name}")
        assert np.array_equal(b.buf[:rows, cur].cpu().numpy(), ref), f"{what}: {name}"
    if longi:
        bufs["mask"].mask[:rows, :T] = False
        bufs["mask"].check(f"{what} mask")
        assert np.array_equal(bufs["mask"].buf[:rows, :T].cpu().numpy(), mask), f"{what}: mask"
        bufs["pos"].check(f"{what} pos")
        assert np.array_equal(bufs["pos"].view.cpu().numpy(), pos), f"{what}: position"
    else:
        bufs["mask"].check(f"{what} mask (unused)")
        bufs["pos"].check(f"{what} pos (unused)")
    return new_id, tt, pos


def _step_args(ops, ids_d, strip, cur, half, longi, bufs):
    rows = ids_d.shape[0]
    return (ids_d, strip, cur, SP0, SP1, SEC, half, MASK_TOK if longi else -1, bufs["new_id"].view.view(rows, 1), bufs["tt"].view.view(rows, 1),
            bufs["pos"].view.view(rows, 1) if longi else None, bufs["mask"].buf if longi else None, bufs["tt_hist"].buf,
            bufs["pos_hist"].buf if longi else None)


def _embed_ref(tables, new_id, tt, pos):
    word, typ, posw, gamma, beta = tables
    s = word.double()[new_id] + typ.double()[tt] + posw.double()[pos]
    mu = s.mean(1, keepdim=True)
    var = ((s - mu) ** 2).mean(1, keepdim=True)
    return ((s - mu) / torch.sqrt(var + 1e-12) * gamma.double() + beta.double()).numpy()


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 511, 512])
@pytest.mark.parametrize("strip", [0, 1])
def test_decode_step_inputs_and_embed(ops, T, strip):
    tables = _embed_tables()
    tables_d = [t.cuda() for t in tables]
    cur = strip + T
    for i, (rows, longi, out_dal) in enumerate([(1, True, True), (16, True, True), (17, False, True), (33, True, True), (48, True, False),
                                                (64, False, True), (64, True, False)]):
        half = rows // 2 if rows > 1 else rows
        ids = _step_ids(rows, strip, T, half, seed=T * 131 + strip * 7 + i)
        ids_d = ids.cuda()
        what = f"T={T} strip={strip} rows={rows} longi={longi}"
        bufs = _step_buffers(rows)
        ops.decode_step_inputs(*_step_args(ops, ids_d, strip, cur, half, longi, bufs))
        _check_step(bufs, ids, strip, cur, half, longi, what + " inputs")
        bufs = _step_buffers(rows)
        out = ops.decode_step_embed(*_step_args(ops, ids_d, strip, cur, half, longi, bufs), *tables_d, 1e-12, out_dal=out_dal)
        new_id, tt, pos = _check_step(bufs, ids, strip, cur, half, longi, what + " embed")
        emb = ops.dec_from_dal(out, rows, C) if out_dal else out
        ref = _embed_ref(tables, torch.from_numpy(new_id), torch.from_numpy(tt), torch.from_numpy(pos))
        assert_bf16_bracket(emb, ref, 2e-5 * (np.abs(ref) + 1.0), what + " embedding")


def test_decode_embedding_dropout_matches_the_teacher_forced_embedding(ops):
    """The decode step keys its embedding dropout on (row, T - 1), bert_embed on (row / T, pos_offset + row % T): for the same sequence and
    position both drop the same elements, with values within one bf16 ulp (the train-mode re-scoring of sampled tokens relies on it)."""
    tables = _embed_tables()
    tables_d = [t.cuda() for t in tables]
    rows, strip, T = 12, 1, 40
    cur = strip + T
    ids = _step_ids(rows, strip, T, rows, seed=99)
    seed = torch.tensor([12345], dtype=torch.int32, device="cuda")
    bufs = _step_buffers(rows)
    dec = ops.decode_step_embed(*_step_args(ops, ids.cuda(), strip, cur, rows, False, bufs), *tables_d, 1e-12, drop=(0.3, seed, 1), out_dal=False)
    bufs2 = _step_buffers(rows)
    nodrop = ops.decode_step_embed(*_step_args(ops, ids.cuda(), strip, cur, rows, False, bufs2), *tables_d, 1e-12, out_dal=False)
    tt_last = bufs["tt"].view.clone()
    fed = ids[:, strip:cur].cuda().contiguous()
    tt_full = torch.zeros(rows, T, dtype=I64, device="cuda")
    tt_full[:, -1] = tt_last
    tf, _, _ = ops.bert_embed(fed.view(-1), tt_full.view(-1), None, *tables_d, 1e-12, T, pos_offset=0, drop=(0.3, seed, 1))
    tf_last = tf.view(rows, T, C)[:, -1]
    nz = nodrop != 0
    dropped = (dec == 0) & nz
    assert 0.2 < float(dropped.float().mean()) < 0.4
    assert torch.equal(dropped, (tf_last == 0) & nz), "different dropout masks for the same (sequence, position)"
    d, t = dec.float().double().cpu().numpy(), tf_last.float().double().cpu().numpy()
    one_ulp = np.abs(bf16_ceil(np.nextafter(np.abs(d), np.inf)) - np.abs(d))
    assert (np.abs(d - t) <= one_ulp).all(), "decode and teacher-forced embeddings differ by more than one bf16 ulp"


# ------------------------------------------------------------------------------------------------ argument checks
def test_wrappers_reject_bad_arguments_before_launching(ops):
    from cxrmate_amd._lib import CxrError, LIB

    def rejected(fn, *outs):
        before = [o.clone() for o in outs]
        with pytest.raises(CxrError, match="code -1"):
            fn()
        torch.cuda.synchronize()
        for o, b in zip(outs, before):
            assert torch.equal(o.view(torch.uint8), b.view(torch.uint8)), "output changed by a rejected call"

    f32, bf = torch.ones(64, device="cuda"), torch.ones(64, device="cuda", dtype=BF)
    o32, obf = torch.full((64,), 7.0, device="cuda"), torch.full((64,), 7.0, device="cuda", dtype=BF)
    rejected(lambda: ops.cast_to_bf16(f32[:0], obf[:0]), obf)
    rejected(lambda: ops.cast_to_f32(bf[:0], o32[:0]), o32)
    a = torch.ones(4, 12, device="cuda", dtype=BF)
    o = torch.full((4, 12), 3.0, device="cuda", dtype=BF)
    rejected(lambda: ops.add(a, a, out=o), o)                                             # C % 8 != 0
    s3, d3 = torch.ones(2, 3, 12, device="cuda", dtype=BF), torch.full((2, 3, 12), 3.0, device="cuda", dtype=BF)
    rejected(lambda: ops.copy_rows(s3, d3), d3)                                           # C % 8 != 0
    rejected(lambda: ops.gather_batch(s3, torch.tensor([1, 0], device="cuda"), 0, d3), d3)   # rows = 0
    e3 = torch.full((0, 3, 16), 3.0, device="cuda", dtype=BF)
    rejected(lambda: ops.bcast_row(f32[:16], e3), o32)                                    # B = 0
    acc = torch.full((16,), 2.0, device="cuda")
    rejected(lambda: ops.sum_row0_into(e3, acc), acc)                                     # B = 0
    rejected(lambda: ops.gelu_bwd(bf[:12], bf[:12]), obf)                                 # n % 8 != 0
    x = torch.full((2, 0), 1.0, device="cuda")
    rejected(lambda: ops.log_softmax_rows_(x), o32)                                       # V = 0
    xs = torch.randn(2, 40, device="cuda")
    rejected(lambda: ops.topk_rows(xs, 17), o32)                                          # K > 16
    rejected(lambda: ops.topk_rows(xs[:, :5], 6), o32)                                    # K > n
    rejected(lambda: ops.cosine_rows(xs[:, :0], xs[:, :0]), o32)                          # C = 0
    off = torch.tensor([0], dtype=torch.int32, device="cuda")
    lo = torch.full((4,), 5, dtype=I64, device="cuda")
    rejected(lambda: LIB.call("cxr_segment_argmax_f32", xs.data_ptr(), 40, off.data_ptr(), 0, lo.data_ptr(), 2, ops._s()), lo)   # no segment
    tables_d = [t.cuda() for t in _embed_tables()]
    ids = torch.randint(30, VOCAB, (4, LMAX)).cuda()
    bufs = _step_buffers(4)
    outs = [b.buf for b in bufs.values()]
    rejected(lambda: ops.decode_step_inputs(*_step_args(ops, ids, 5, 5, 2, True, bufs)), *outs)                 # T = cur - strip = 0
    rejected(lambda: ops.decode_step_embed(*_step_args(ops, ids, 0, 513, 2, True, bufs), *tables_d, 1e-12), *outs)   # T > 512
    args = list(_step_args(ops, ids, 0, 20, 2, True, bufs))
    args[3] = [20, 21, 22, 23, 24]                                                                              # 5 separators
    rejected(lambda: ops.decode_step_embed(*args, *tables_d, 1e-12), *outs)
