"""GPU: output_attentions / output_hidden_states of generate() and of the cached forward (past_key_values).

  kernels (csrc/attn_decode_probs.hip) : ops.attention_decode_probs against fp32 torch softmax of the same bf16 q / k (masked entries exactly 0,
                                         row sums within 1e-3, |P - ref| <= 2e-5 + 2e-3 |ref|, uniform all-masked rows, strided slots, row groups);
                                         its dropout against the context of ops.attention_decode; ops.dec_hidden_record against an fp64 LayerNorm
                                         (allowed 4 x the error of torch's own fp32 layer_norm), the widening mode bit-exact
  cached == teacher-forced             : step t of generate against the fed position's row of forward(output_attentions, output_hidden_states) on
                                         the finished sequences, three models, at the model tolerances of test_attn_outputs_gpu.py
  nothing else changes                 : sequences, scores, logits, sequences_scores, beam_indices torch.equal with and without the flags
  beams, replay, cached forward        : device == host loop, study-major rows, graph replay, a hand-written loop over forward(past_key_values=)

Measured on MI355X (rel-rms of generate's maps / states against the teacher-forced pass, worst layer, step and field): multi 7.1e-3, single
7.0e-3, longitudinal 7.1e-3, image_size 128 7.0e-3 (cap 2.5e-2); cached forward loop against generate 3.1e-3.
"""
import pytest
import torch

import golden_util as gu
from cxrmate_amd.config import tiny_config
from test_attn_outputs_gpu import ACT_COS, ACT_RMS, _case, _ref_probs
from test_gen_scores_gpu import model_case

pytestmark = pytest.mark.gpu

H, D = 12, 768
SCALE = 64 ** -0.5
MAPS = dict(return_dict_in_generate=True, output_attentions=True, output_hidden_states=True)
FIELDS = ["decoder_attentions", "cross_attentions", "decoder_hidden_states"]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cxrmate_amd import modelling
    return modelling


@pytest.fixture(scope="module")
def G():
    return gu.load("gen_scores.npz")


# ------------------------------------------------------------------------------------------------ kernel: probabilities
B = 4
TKS = [1, 2, 63, 64, 65, 72, 255, 256, 257, 300, 512, 1152, 1728]


def _qk(Tk, share, layout, seed=0):
    """q [B, D]; k [B / share, Tk, D] as a slice of a longer cache ("cache") or a column block of a [Bkv, S, 4 D] buffer ("block")"""
    g = torch.Generator(device="cuda").manual_seed(seed + Tk)
    Bkv = B // share
    q = torch.randn((B, D), generator=g, device="cuda").to(torch.bfloat16)
    if layout == "cache":
        k = torch.randn((Bkv, Tk + 5, D), generator=g, device="cuda").to(torch.bfloat16)[:, :Tk, :]
    else:
        k = torch.randn((Bkv, Tk, 4 * D), generator=g, device="cuda").to(torch.bfloat16)[:, :, 2 * D:3 * D]
    return q, k


def _mask(Tk, Bkv):
    kpm = torch.ones((Bkv, Tk), dtype=torch.uint8, device="cuda")
    kpm[0, max(1, (2 * Tk) // 3):] = 0                       # right padding
    kpm[0, Tk // 3] = 0 if Tk > 3 else 1                     # an interior masked key
    kpm[Bkv - 1, :] = 0                                      # every key masked: uniform rows
    return kpm


def _ref(q, k, kpm, share):
    """fp32 torch softmax on the same bf16 q / k, decode row b + g * Bkv reading K row b: -> (P [B, H, 1, Tk], visible-or-dead)"""
    idx = torch.arange(B, device="cuda") % (B // share)
    return _ref_probs(q.unsqueeze(1), k[idx], H, SCALE, None if kpm is None else kpm[idx], False, 0)


def _study_major(t, groups):
    return t.view(groups, t.shape[0] // groups, *t.shape[1:]).transpose(0, 1).reshape(t.shape)


@pytest.mark.parametrize("Tk", TKS)
def test_decode_probs_match_fp32_torch(M, Tk):
    from cxrmate_amd import ops
    n = 0
    for share in (1, 2, 4):
        Bkv = B // share
        for layout, mask, groups in (("cache", "none", 1), ("block", "bytes", 2), ("cache", "bits", 4), ("block", "bits", 1)):
            q, k = _qk(Tk, share, layout, seed=n)
            n += 1
            kpm = None if mask == "none" else _mask(Tk, Bkv)
            kw = dict(kpm=kpm) if mask != "bits" else dict(kpm_bits=ops.pack_mask_bits(kpm))
            # a strided slot inside a sentinel-filled buffer: rows, heads and keys all padded
            big = torch.full((B + 1, H + 1, Tk + 9), -7.0, device="cuda")
            slot = big[:B, :H, 4:4 + Tk]
            p = ops.attention_decode_probs(q, k, H, SCALE, out=slot, row_groups=groups, **kw)
            assert p.shape == (B, H, 1, Tk) and p.dtype == torch.float32
            what = (Tk, share, layout, mask, groups)
            assert bool((big[B:] == -7).all()) and bool((big[:, H:] == -7).all()) and bool((big[..., :4] == -7).all()) \
                and bool((big[..., 4 + Tk:] == -7).all()), what
            ref, vis = _ref(q, k, kpm, share)
            ref, vis = _study_major(ref, groups), _study_major(vis, groups)
            assert torch.isfinite(p).all(), what
            assert bool((p[~vis] == 0).all()), ("masked entries must be exactly 0", what)
            assert float((p.sum(-1) - 1).abs().max()) <= 1e-3, what
            err = (p - ref).abs() - (2e-5 + 2e-3 * ref.abs())
            assert float(err.max()) <= 0, (what, f"max |P - ref| {float((p - ref).abs().max()):.3e}")
            if kpm is not None:                              # decode rows reading the all-masked K row, wherever the permutation put them
                dead = _study_major((torch.arange(B, device="cuda") % Bkv) == Bkv - 1, groups)
                assert torch.allclose(p[dead], torch.full_like(p[dead], 1.0 / Tk), rtol=1e-6, atol=0), what
            # a fresh contiguous output is the same map
            assert torch.equal(ops.attention_decode_probs(q, k, H, SCALE, row_groups=groups, **kw), p), what


def test_decode_probs_refuse_bad_arguments(M):
    from cxrmate_amd import ops
    from cxrmate_amd._lib import CxrError
    q, k = _qk(64, 1, "cache")
    with pytest.raises(CxrError):
        ops.attention_decode_probs(q, k, H, SCALE, drop=(1.5, torch.zeros(1, dtype=torch.int32, device="cuda"), 1, 0))
    with pytest.raises(CxrError):                            # a K view whose rows are not 16-byte aligned
        kk = torch.zeros((B, 64, D + 4), dtype=torch.bfloat16, device="cuda")[:, :, 4:]
        ops.attention_decode_probs(q, kk, H, SCALE)


# ------------------------------------------------------------------------------------------------ kernel: dropout
@pytest.mark.parametrize("Tk,share,mask", [(72, 1, "bytes"), (257, 1, "bytes"), (1152, 2, "bits"), (1728, 4, "bits")])
def test_dropout_maps_reproduce_the_decode_context(M, Tk, share, mask):
    from cxrmate_amd import ops
    Bkv = B // share
    g = torch.Generator(device="cuda").manual_seed(Tk)
    q = torch.randn((B, D), generator=g, device="cuda").to(torch.bfloat16)
    kv = torch.randn((Bkv, Tk, 4 * D), generator=g, device="cuda").to(torch.bfloat16)
    k, v = kv[:, :, 2 * D:3 * D], kv[:, :, 3 * D:]
    kpm = _mask(Tk, Bkv)
    kpm[Bkv - 1, :] = 1                                       # (every row keeps visible keys: the dropped share is counted over them)
    kw = dict(kpm=kpm) if mask == "bytes" else dict(kpm_bits=ops.pack_mask_bits(kpm))
    seed = torch.tensor([123457], dtype=torch.int32, device="cuda")
    drop = (0.1, seed, 18, 5)
    ctx = ops.attention_decode(q, k, v, H, SCALE, drop=drop, **kw)
    p = ops.attention_decode_probs(q, k, H, SCALE, drop=drop, **kw)
    idx = torch.arange(B, device="cuda") % Bkv
    vf = v.float().view(Bkv, Tk, H, 64)[idx]
    got = torch.einsum("bhj,bjhd->bhd", p[:, :, 0, :], vf).reshape(B, D)
    r = gu.rel_rms(got.cpu().numpy(), ctx.float().cpu().numpy())
    print(f"P.V vs decode context, Tk {Tk} share {share}: rel-rms {r:.5f}")
    assert r <= 1e-2, f"P.V vs decode context: rel-rms {r:.4f}"
    p0 = ops.attention_decode_probs(q, k, H, SCALE, **kw)
    nz = p0 > 0
    frac = float((p[nz] == 0).float().mean())
    assert 0.07 < frac < 0.13, frac
    kept = nz & (p > 0)
    assert torch.allclose(p[kept], p0[kept] / 0.9, rtol=1e-6, atol=0)
    p2 = ops.attention_decode_probs(q, k, H, SCALE, drop=(0.1, seed + 1, 18, 5), **kw)
    got2 = torch.einsum("bhj,bjhd->bhd", p2[:, :, 0, :], vf).reshape(B, D)
    assert gu.rel_rms(got2.cpu().numpy(), ctx.float().cpu().numpy()) > 3e-2


# ------------------------------------------------------------------------------------------------ kernel: hidden states
@pytest.mark.parametrize("rows", [1, 16, 17, 33, 48, 64])
def test_hidden_record_matches_fp64_layernorm(M, rows):
    """The kernel sums a row in another order than torch's layer_norm: it is allowed 4 x the error torch's own fp32 layer_norm has against
    the same fp64 reference (max |difference| over the outputs)."""
    from cxrmate_amd import ops
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = (torch.randn((rows, D), generator=g, device="cuda") * 3.0 + 0.5).to(torch.bfloat16)
    gamma = torch.randn(D, generator=g, device="cuda") * 0.2 + 1.0
    beta = torch.randn(D, generator=g, device="cuda") * 0.1
    eps = 1e-12
    xd, _ = ops.dec_to_dal(x)
    for groups in (1, 2, 4):
        if rows % groups:
            continue
        for gm, bt in ((gamma, beta), (torch.ones_like(gamma), torch.zeros_like(beta))):
            big = torch.full((rows + 1, D + 8), -7.0, device="cuda")
            out = ops.dec_hidden_record(xd, rows, gm, bt, eps, out=big[:rows, :D], row_groups=groups)
            assert bool((big[rows:] == -7).all()) and bool((big[:, D:] == -7).all())
            ref = _study_major(torch.nn.functional.layer_norm(x.double(), (D,), gm.double(), bt.double(), eps), groups)
            own = _study_major(torch.nn.functional.layer_norm(x.float(), (D,), gm, bt, eps), groups)
            e_torch = float((own.double() - ref).abs().max())
            e_kernel = float((out.double() - ref).abs().max())
            print(f"rows {rows} groups {groups}: torch fp32 layer_norm error {e_torch:.3e}, kernel {e_kernel:.3e}")
            assert e_kernel <= 4 * e_torch, (rows, groups, e_kernel, e_torch)
        wide = ops.dec_hidden_record(xd, rows, row_groups=groups)             # widening only: bit-exact
        assert wide.dtype == torch.float32 and torch.equal(wide, _study_major(x.float(), groups))


# ------------------------------------------------------------------------------------------------ cached == teacher-forced
GEN = {"multi": dict(special_token_ids=[gu.SEP]), "single": dict(special_token_ids=[gu.SEP]),
       "longitudinal": dict(special_token_ids=[gu.PMT_SEP, gu.BOS, gu.SEP], mask_token_id=gu.PAD)}
PROMPT = torch.tensor([[gu.PMT, 21, 22, gu.PMT_SEP], [gu.PMT, gu.PAD, 23, gu.PMT_SEP]])      # no leading BOS: prepended, then stripped again


def _gen_kwargs(m, name, x, eos=None, new=8):
    with torch.no_grad():
        eo = m._encode(x)
    kw = dict(GEN[name], encoder_outputs=eo, bos_token_id=gu.BOS, eos_token_id=eos, pad_token_id=gu.PAD, max_new_tokens=new, num_beams=1)
    if name == "longitudinal":
        kw["decoder_input_ids"] = PROMPT.cuda()
    return kw


def _teacher_forced(m, name, out, eo):
    """forward with the flags over the finished sequences, fed the per-step token types / positions that generate recorded"""
    seq = out["sequences"]
    fed = m._fed(seq, gu.BOS)
    rec = out["recorded_inputs"]
    tf_in = fed[:, :-1]
    kw = dict(decoder_token_type_ids=torch.cat(rec["tt"], 1))
    assert kw["decoder_token_type_ids"].shape == tf_in.shape
    if rec["pos"][0] is not None:
        kw["decoder_position_ids"] = torch.cat(rec["pos"], 1)
    if name == "longitudinal":
        kw["decoder_attention_mask"] = (tf_in != gu.PAD).long()
    with torch.no_grad():
        return m(encoder_outputs=eo, decoder_input_ids=tf_in, output_attentions=True, output_hidden_states=True, **kw), tf_in.shape[1]


def _close(a, b, what, worst):
    a, b = a.float().cpu().numpy(), b.float().cpu().numpy()
    r, c = gu.rel_rms(a, b), gu.cosine(a, b)
    worst[0] = max(worst[0], r)
    assert r <= ACT_RMS and c >= ACT_COS, f"{what}: rel_rms {r:.4f} cosine {c:.6f}"


def _compare_with_forward(out, tf, Tp, T, what, alive=None):
    """step t of generate against position Tp + t - 1 (step 0: positions 0 .. Tp - 1) of the teacher-forced maps / states; alive [rows, steps]:
    the (row, step) pairs compared (default: all)."""
    steps = len(out["decoder_attentions"])
    assert steps == len(out["cross_attentions"]) == len(out["decoder_hidden_states"]) == T - Tp + 1
    L = len(tf.decoder_attentions)
    worst = [0.0]
    for t in range(steps):
        pos = slice(0, Tp) if t == 0 else slice(Tp + t - 1, Tp + t)
        Tk = Tp + t
        rows = slice(None) if alive is None else alive[:, t]
        assert len(out["decoder_attentions"][t]) == len(out["cross_attentions"][t]) == L and len(out["decoder_hidden_states"][t]) == L + 1
        for l in range(L):
            sa, ca = out["decoder_attentions"][t][l], out["cross_attentions"][t][l]
            rsa, rca = tf.decoder_attentions[l][:, :, pos, :Tk], tf.cross_attentions[l][:, :, pos, :]
            assert sa.dtype == ca.dtype == torch.float32 and sa.shape == rsa.shape and ca.shape == rca.shape, (what, t, l, sa.shape, rsa.shape)
            assert not sa.requires_grad and not ca.requires_grad
            for a, r in ((sa, rsa), (ca, rca)):
                assert torch.equal(a[rows] == 0, r[rows] == 0), (what, t, l, "masked entries are exactly 0 in both")
                assert float((a[rows].sum(-1) - 1).abs().max()) <= 1e-3 and float((r[rows].sum(-1) - 1).abs().max()) <= 1e-3
            _close(sa[rows], rsa[rows], f"{what} self step {t} layer {l}", worst)
            _close(ca[rows], rca[rows], f"{what} cross step {t} layer {l}", worst)
        for i in range(L + 1):
            hs, rhs = out["decoder_hidden_states"][t][i], tf.decoder_hidden_states[i][:, pos, :]
            assert hs.dtype == torch.float32 and hs.shape == rhs.shape and not hs.requires_grad
            _close(hs[rows], rhs[rows], f"{what} hidden step {t} state {i}", worst)
    print(f"{what}: worst rel-rms of generate's maps / states against the teacher-forced pass {worst[0]:.5f}")
    return worst[0]


@pytest.mark.parametrize("name", ["multi", "single", "longitudinal"])
def test_generate_maps_equal_teacher_forced(M, name):
    g, pre, m, x, _ = _case(M, name)
    kw = _gen_kwargs(m, name, x)
    out = m.generate(**kw, record_inputs=True, output_scores=True, **MAPS)
    assert list(out.keys()) == ["sequences", "scores", "recorded_inputs"] + FIELDS
    assert out.encoder_attentions is None and out.encoder_hidden_states is None
    assert len(out["scores"]) == len(out["decoder_attentions"]) == 8
    rows, P = out["sequences"].shape[0], out["sequences"].shape[1] - 8
    Tp = P - 1 if name == "longitudinal" else P
    assert Tp == (4 if name == "longitudinal" else 1)
    S = out["cross_attentions"][0][0].shape[-1]
    assert out["decoder_attentions"][0][0].shape == (rows, H, Tp, Tp) and out["cross_attentions"][0][0].shape == (rows, H, Tp, S)
    assert out["decoder_hidden_states"][0][0].shape == (rows, Tp, D)
    for t in range(1, 8):
        assert out["decoder_attentions"][t][1].shape == (rows, H, 1, Tp + t) and out["cross_attentions"][t][1].shape == (rows, H, 1, S)
        assert out["decoder_hidden_states"][t][2].shape == (rows, 1, D)
    tf, T = _teacher_forced(m, name, out, kw["encoder_outputs"])
    _compare_with_forward(out, tf, Tp, T, name)
    if name == "longitudinal":                               # the padded prompt token is hidden from every later query of its row
        assert all(bool((out["decoder_attentions"][t][0][1, :, :, 1] == 0).all()) for t in range(8))
    if name == "multi":                                      # the zero-padded image's keys
        assert bool((out["cross_attentions"][3][0] == 0).any())


def test_generate_maps_with_rows_that_finish_early(M):
    g, pre, m, x, _ = _case(M, "multi")
    free = m.generate(**_gen_kwargs(m, "multi", x, new=12))
    gen = free[:, 1:]
    # an EOS that some rows reach early: the most frequent token of the free-running decode that not every row emits at the same step
    eos = None
    for tok in gen.flatten().tolist():
        first = torch.where((gen == tok).any(1), (gen == tok).int().argmax(1), torch.full((gen.shape[0],), 99, device=gen.device))
        if int(first.min()) < int(first.max()) and int(first.min()) < 10:
            eos = tok
            break
    assert eos is not None, gen
    kw = _gen_kwargs(m, "multi", x, eos=eos, new=12)
    out = m.generate(**kw, record_inputs=True, output_scores=True, **MAPS)
    seq = out["sequences"]
    steps = seq.shape[1] - 1
    assert len(out["scores"]) == len(out["decoder_attentions"]) == steps
    is_eos = seq[:, 1:] == eos
    done_at = torch.where(is_eos.any(1), is_eos.int().argmax(1), torch.full((seq.shape[0],), steps, device=seq.device))
    assert int(done_at.min()) < steps - 1, (seq, "some row must finish early")
    alive = torch.arange(steps, device=seq.device).view(1, -1) <= done_at.view(-1, 1)       # step t feeds token t - 1: still a real one
    tf, T = _teacher_forced(m, "multi", out, kw["encoder_outputs"])
    _compare_with_forward(out, tf, 1, T, "multi with EOS", alive=alive)


def test_generate_maps_on_the_packed_cross_attention_branch(M):
    """image_size 128: S = 2 x 64 keys, a multiple of 32 -- the cached steps read the fragment-ordered cross K / V and project the query inside
    the cross-attention kernel; the record's q2 comes from its own launch."""
    from cxrmate_amd import weights
    cfg = tiny_config(vocab_size=1000, decoder_layers=2, depth=(1, 2, 3), image_size=128)
    m = M.MultiCXREncoderDecoderModel(cfg, seed=None)
    m.load_state_dict(weights.init_encoder_decoder(cfg, seed=11, perturb=0.05))
    x = gu.distinct_study_pixels(5, 0.3, size=128).cuda()
    kw = _gen_kwargs(m, "multi", x)
    out = m.generate(**kw, record_inputs=True, **MAPS)
    ses = next(iter(m._decode_sessions.values()))
    assert ses.cache.cpk[0] is not None and out["cross_attentions"][1][0].shape == (3, H, 1, 128)
    plain = m.generate(**kw)
    assert torch.equal(plain, out["sequences"])
    tf, T = _teacher_forced(m, "multi", out, kw["encoder_outputs"])
    _compare_with_forward(out, tf, 1, T, "multi, image_size 128")


# ------------------------------------------------------------------------------------------------ nothing else changes
CALLS = {
    "greedy": dict(num_beams=1),
    "top-k sampling": dict(num_beams=1, do_sample=True, top_k=20),
    "device beam-4": dict(num_beams=4),
    "host beam-3": dict(num_beams=3),
    "two sequences per study": dict(num_beams=1, do_sample=True, top_k=20, num_return_sequences=2),
    "train mode": dict(num_beams=1, eos_token_id=None),         # (no EOS: under dropout the case's first token may be the EOS, and every step is to run)
}


@pytest.mark.parametrize("call", list(CALLS))
def test_flags_change_nothing_else(M, G, call):
    m, kw, P = model_case(M, G, "mb")
    kw = dict(kw, max_length=12, return_dict_in_generate=True, output_scores=True, output_logits=True, **CALLS[call])
    if call == "train mode":
        m.train()

    def run(**flags):
        torch.manual_seed(31)
        return m.generate(**kw, **flags)
    base, both = run(), run(output_attentions=True, output_hidden_states=True)
    off = run(output_attentions=False, output_hidden_states=False)
    attn, hid = run(output_attentions=True), run(output_hidden_states=True)
    m.eval()
    today = ["sequences", "sequences_scores", "scores", "logits", "beam_indices"] if "beam" in call else ["sequences", "scores", "logits"]
    assert list(base.keys()) == today and list(off.keys()) == today
    assert list(both.keys()) == today + FIELDS
    assert list(attn.keys()) == today + FIELDS[:2] and list(hid.keys()) == today + FIELDS[2:]
    for other in (both, attn, hid, off):
        for k in today:
            a, b = base[k], other[k]
            if isinstance(a, tuple):
                assert len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b)), (call, k)
            else:
                assert torch.equal(a, b), (call, k)
    steps, rows = len(base["scores"]), base["scores"][0].shape[0]
    assert len(both["decoder_attentions"]) == len(both["cross_attentions"]) == len(both["decoder_hidden_states"]) == steps
    assert both["decoder_attentions"][-1][0].shape == (rows, H, 1, steps) and both["decoder_hidden_states"][-1][0].shape == (rows, 1, D)
    for t in range(steps):
        for l in range(2):
            assert torch.equal(both["decoder_attentions"][t][l], attn["decoder_attentions"][t][l])
            assert torch.equal(both["cross_attentions"][t][l], attn["cross_attentions"][t][l])
            assert torch.equal(both["decoder_hidden_states"][t][l], hid["decoder_hidden_states"][t][l])
    if call == "train mode":                                  # post-dropout maps: some visible entries are dropped
        ca = both["cross_attentions"][1][0]
        assert bool((ca == 0).any()) and float(ca.sum(-1).mean()) == pytest.approx(1.0, abs=0.05) and float((ca.sum(-1) - 1).abs().max()) > 1e-3


def test_flags_without_the_dict_output_change_nothing(M, G):
    m, kw, P = model_case(M, G, "mb")
    kw = dict(kw, max_length=12, num_beams=1)
    a = m.generate(**kw)
    b = m.generate(**kw, output_attentions=True, output_hidden_states=True)
    assert isinstance(b, torch.Tensor) and torch.equal(a, b)
    from transformers import GenerationConfig
    c = m.generate(**kw, generation_config=GenerationConfig(output_attentions=True, return_dict_in_generate=True))
    assert list(c.keys()) == ["sequences", "scores"] + FIELDS[:2] and torch.equal(c["sequences"], a)


# ------------------------------------------------------------------------------------------------ beams
def _maps_close(a, b, what):
    worst = [0.0]
    assert len(a["decoder_attentions"]) == len(b["decoder_attentions"]), what
    for f in FIELDS:
        for t, (sa, sb) in enumerate(zip(a[f], b[f])):
            for l, (x, y) in enumerate(zip(sa, sb)):
                assert x.shape == y.shape, (what, f, t, l, x.shape, y.shape)
                if f != "decoder_hidden_states":
                    assert torch.equal(x == 0, y == 0), (what, f, t, l)
                _close(x, y, f"{what} {f} step {t} layer {l}", worst)
    return worst[0]


def test_device_beam_maps_equal_the_host_loop(M, G):
    """The fixture's beam case: its decisions clear the bf16 error bound, so the device search and the host loop choose the same beams (asserted
    first); the running beams of step t are then the same rows, study-major, in both."""
    m, kw, P = model_case(M, G, "mb")
    kw = dict(kw, num_beams=4, output_scores=True, **MAPS)
    dev = m.generate(**kw)
    m.device_beam_search = False
    host = m.generate(**kw)
    m.device_beam_search = True
    assert torch.equal(dev["sequences"], host["sequences"]) and torch.equal(dev["beam_indices"], host["beam_indices"])
    assert list(dev.keys()) == list(host.keys()) == ["sequences", "sequences_scores", "scores", "beam_indices"] + FIELDS
    assert len(dev["scores"]) == len(dev["decoder_attentions"]) and dev["decoder_attentions"][1][0].shape[0] == 3 * 4
    w = _maps_close(dev, host, "device vs host beam-4")
    print(f"device vs host beam-4 maps: worst rel-rms {w:.5f}")
    # a beam call that asks only for the maps still returns the beam indices (TF5 _beam_search returns them for every dict output)
    only = m.generate(**dict(kw, output_scores=False))
    assert list(only.keys()) == ["sequences", "sequences_scores", "beam_indices"] + FIELDS and only["sequences_scores"] is None
    assert torch.equal(only["beam_indices"], dev["beam_indices"])


def test_return_sequences_rows_are_study_major(M, G):
    """top_k = 1 sampling draws the argmax: every sample of a study repeats the greedy decode, so rows b * n + j hold study b's greedy maps"""
    m, kw, P = model_case(M, G, "mg")
    kw = dict(kw, max_length=10, num_beams=1, **MAPS)
    greedy = m.generate(**kw)
    n = 2
    out = m.generate(**kw, do_sample=True, top_k=1, num_return_sequences=n)
    assert torch.equal(out["sequences"], greedy["sequences"].repeat_interleave(n, 0))
    rep = {f: tuple(tuple(x.repeat_interleave(n, 0) for x in st) for st in greedy[f]) for f in FIELDS}
    _maps_close(out, rep, "two sequences per study vs greedy")


# ------------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_returns_equal_maps_and_copies(M, G):
    m, kw, P = model_case(M, G, "mg")
    kw = dict(kw, max_length=12, num_beams=1, **MAPS)
    first = m.generate(**kw)                                  # captures the step graphs
    keep = {f: [[x.clone() for x in st] for st in first[f]] for f in FIELDS}
    second = m.generate(**kw)                                 # replays them
    for f in FIELDS:
        for sa, sb in zip(first[f], second[f]):
            assert all(torch.equal(x, y) for x, y in zip(sa, sb)), f
    other = dict(kw, pixel_values=torch.flip(kw["pixel_values"], dims=(0,)) * 1.5)
    third = m.generate(**other)
    assert not torch.equal(third["cross_attentions"][1][0], first["cross_attentions"][1][0])
    for f in FIELDS:                                          # what the first call returned is its own copy
        for sa, sb in zip(first[f], keep[f]):
            assert all(torch.equal(x, y) for x, y in zip(sa, sb)), f


# ------------------------------------------------------------------------------------------------ cached forward
def test_cached_forward_loop_returns_the_maps(M, G):
    m, kw, P = model_case(M, G, "sg")
    gen = m.generate(**dict(kw, max_length=9, eos_token_id=None), num_beams=1, record_inputs=True, **MAPS)
    seq = gen["sequences"]
    with torch.no_grad():
        eo = m._encode(kw["pixel_values"])
        past, outs = None, []
        for t in range(seq.shape[1] - 1):
            tt = m.token_ids_to_token_type_ids(seq[:, :t + 1], [gu.SEP])
            fed, tt_new = (seq[:, :1], tt) if past is None else (seq[:, t:t + 1], tt[:, -1:])
            o = m(encoder_outputs=eo, decoder_input_ids=fed, decoder_token_type_ids=tt_new, past_key_values=past, use_cache=True,
                  output_attentions=True, output_hidden_states=True)
            past = o.past_key_values
            outs.append(o)
    rows, S = seq.shape[0], gen["cross_attentions"][0][0].shape[-1]
    worst = [0.0]
    for t, o in enumerate(outs):
        assert list(o.keys()) == ["loss", "logits", "past_key_values", "decoder_hidden_states", "decoder_attentions", "cross_attentions",
                                  "encoder_last_hidden_state"]
        assert len(o.decoder_hidden_states) == 3 and len(o.decoder_attentions) == 2 and len(o.cross_attentions) == 2
        assert o.decoder_attentions[0].shape == (rows, H, 1, t + 1) and o.cross_attentions[0].shape == (rows, H, 1, S)
        assert o.decoder_hidden_states[0].shape == (rows, 1, D) and o.decoder_attentions[0].dtype == torch.float32
        for l in range(2):
            _close(o.decoder_attentions[l], gen["decoder_attentions"][t][l], f"cached forward self {t} {l}", worst)
            _close(o.cross_attentions[l], gen["cross_attentions"][t][l], f"cached forward cross {t} {l}", worst)
        for i in range(3):
            _close(o.decoder_hidden_states[i], gen["decoder_hidden_states"][t][i], f"cached forward hidden {t} {i}", worst)
    print(f"cached forward vs generate: worst rel-rms {worst[0]:.5f}")
    # only one of the flags on the cached path, then none: the keys of today
    with torch.no_grad():
        o = m(encoder_outputs=eo, decoder_input_ids=seq[:, -1:], decoder_token_type_ids=tt[:, -1:], past_key_values=past, output_hidden_states=True)
        plain = m(encoder_outputs=eo, decoder_input_ids=seq[:, -1:], decoder_token_type_ids=tt[:, -1:], past_key_values=o.past_key_values)
    assert "decoder_attentions" not in o and "cross_attentions" not in o and len(o.decoder_hidden_states) == 3
    assert list(plain.keys()) == ["loss", "logits", "past_key_values", "encoder_last_hidden_state"]
