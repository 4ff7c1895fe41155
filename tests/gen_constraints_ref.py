"""CPU restatements for the token-constraint and early-stopping tests (test_gen_constraints_gpu.py / _abi.py), written from transformers 5.15.0
(TF5 generation/logits_process.py, generation/utils.py) with plain torch ops. They run on whatever device their inputs live on.

  restate()       : the nine processors of cxr_logits_constrain_f32 in the order of TF5 generation/utils.py:1123-1293
  beam_search()   : TF5 _beam_search (:3208-3560) over GIVEN per-step logits with early_stopping False / True / "never", with a per-step trace
"""
import torch

NEG = -1.0e9


def sequence_entries_(x, h, entries):
    """SequenceBiasLogitsProcessor.__call__ (:1288-1319) for entries ((ids, bias), ...) with unique ids tuples (the library's dict): the bias row
    starts at 0, takes the length-1 biases, then every multi-token entry in order (its bias where the history ends in its prefix, else 0); the
    row is added to the scores once."""
    cur = h.shape[1]
    bias = torch.zeros_like(x)
    single = torch.zeros(x.shape[1], dtype=torch.float32, device=x.device)
    for k, b in entries:
        if len(k) == 1:
            single[k[0]] = b
    bias += single
    for k, b in entries:
        if len(k) == 1 or len(k) > cur:
            continue
        pre = torch.tensor(k[:-1], dtype=h.dtype, device=h.device)
        hit = (h[:, cur - len(pre):] == pre).all(dim=1)
        bias[:, k[-1]] += torch.where(hit, torch.tensor(b, dtype=torch.float32, device=x.device), torch.tensor(0.0, device=x.device))
    return x + bias


def restate(x, ids, cur, eos, penalty=1.0, n=0, min_length=0, sequence_bias=(), bad_words=(), forced_bos=None, forced_eos=(), suppress=(),
            begin_suppress=(), max_length=0, begin_index=-1):
    """fp32 rows x [R, V], history ids[:, :cur] -> processed copy. bad_words: ids tuples, single [eos] entries already dropped."""
    x = x.clone()
    h = ids[:, :cur]
    R, V = x.shape
    inf = float("-inf")
    if sequence_bias:
        x = sequence_entries_(x, h, sequence_bias)
    if penalty != 1.0 and cur > 0:
        s = torch.gather(x, 1, h)
        x.scatter_(1, h, torch.where(s < 0, s * penalty, s / penalty))
    if n > 0 and cur >= n:
        win = h.unfold(1, n, 1)                                          # [R, cur - n + 1, n]
        match = (win[..., :-1] == h[:, cur - n + 1:].unsqueeze(1)).all(-1)
        ban = torch.zeros((R, V + 1), dtype=torch.bool, device=x.device)
        ban.scatter_(1, torch.where(match, win[..., -1], V), True)
        x = x.masked_fill(ban[:, :-1], inf)
    if bad_words:
        x = sequence_entries_(x, h, tuple((k, inf) for k in bad_words))
    if cur < min_length and eos >= 0:
        x[:, eos] = inf
    if forced_bos is not None and cur == 1:
        x = torch.full_like(x, inf)
        x[:, forced_bos] = 0.0
    if len(forced_eos) and cur == max_length - 1:
        x = torch.full_like(x, inf)
        x[:, list(forced_eos)] = 0.0
    for lst, on in ((suppress, True), (begin_suppress, cur == begin_index)):
        keep = [t for t in lst if 0 <= t < V]
        if on and keep:
            x[:, keep] = inf
    return x


def _gather(t, idx):
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.gather(t, 1, idx.expand(-1, -1, *t.shape[2:]))


def beam_search(logits_steps, B, nb, bos, eos, pad, max_length, length_penalty=1.0, early_stopping=False, fed=None):
    """TF5 _beam_search over recorded logits (step t: fp32 [B * nb, V], study-major rows, as the library's own loop produced them), prompt = BOS.
    early_stopping: False | True | "never" (_check_early_stop_heuristic :3008, _beam_search_has_unfinished_sequences :3055,
    _update_finished_beams :3150-3204). fed [steps, B * nb]: asserted to be the last token of the running beams at every step.
    -> (sequences [B, nb, max_length], beam_scores [B, nb], trace): one trace dict per executed step with the running beams the step started
    from, parent / token / score of the new running beams, the finished set after the step, and `stop` (the loop ends after this step)."""
    P = 1
    keep = 2 * nb
    running = torch.full((B, nb, max_length), pad, dtype=torch.int64)
    running[:, :, 0] = bos
    sequences = running.clone()
    run_scores = torch.zeros((B, nb))
    run_scores[:, 1:] = NEG
    beam_scores = torch.full((B, nb), NEG)
    finished = torch.zeros((B, nb), dtype=torch.bool)
    unsat = torch.ones((B, 1), dtype=torch.bool)
    top_mask = torch.arange(keep) < nb
    cur = P
    trace = []
    for t, logits in enumerate(logits_steps):
        V = logits.shape[-1]
        if fed is not None:
            assert torch.equal(running[:, :, cur - 1].reshape(-1), fed[t]), t
        logp = torch.log_softmax(logits.float(), dim=-1).view(B, nb, V) + run_scores[:, :, None]
        topk_lp, topk_idx = torch.topk(logp.view(B, nb * V), k=keep)
        beam_of = topk_idx // V
        topk_seq = _gather(running, beam_of)
        topk_seq[:, :, cur] = topk_idx % V
        hits = (topk_seq[:, :, cur] == eos) | (cur + 1 >= max_length)
        run_lp = topk_lp + hits.float() * NEG
        nxt = torch.topk(run_lp, k=nb)[1]
        running_in = running[:, :, :cur].clone()
        running, run_scores = _gather(topk_seq, nxt), _gather(run_lp, nxt)
        just = hits & top_mask[None, :]
        fin_lp = topk_lp / ((cur + 1 - P) ** length_penalty)
        full = finished.all(dim=1, keepdim=True) & (early_stopping is True)
        fin_lp = fin_lp + full.float() * NEG
        fin_lp = fin_lp + (~unsat).float() * NEG
        fin_lp = fin_lp + (~just).float() * NEG
        m_sc = torch.cat((beam_scores, fin_lp), dim=1)
        best = torch.topk(m_sc, k=nb)[1]
        sequences = _gather(torch.cat((sequences, topk_seq), dim=1), best)
        beam_scores = _gather(m_sc, best)
        finished = _gather(torch.cat((finished, just), dim=1), best)
        cur += 1
        length = (max_length - P) if (early_stopping == "never" and length_penalty > 0.0) else (cur - P)
        best_run = run_scores[:, :1] / (length ** length_penalty)
        worst = torch.where(finished, beam_scores.min(dim=1, keepdim=True)[0], torch.tensor(NEG))
        unsat = unsat & torch.any(best_run > worst, dim=-1, keepdim=True)
        going = bool(unsat.any()) and not (bool(finished.all()) and early_stopping is True) and not bool(hits.all())
        trace.append(dict(running_in=running_in, parent=_gather(beam_of, nxt).clone(), token=running[:, :, cur - 1].clone(),
                          running_scores=run_scores.clone(), sequences=sequences.clone(), beam_scores=beam_scores.clone(),
                          finished=finished.clone(), unsat=unsat[:, 0].clone(), stop=not going))
        if not going:
            break
    return sequences, beam_scores, trace
