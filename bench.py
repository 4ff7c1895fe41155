#!/usr/bin/env python3
"""Headline benchmark of the CXRMate hot path on MI355X (contract: README of the build driver).

    python bench.py --gpus 1 --steps 10 --warmup 3                      # the headline alone: set-up, warm-up, the timed TF steps, one line
    python bench.py --gpus 1 --steps 10 --warmup 3 --dump-outputs DIR    # + what the last timed TF step computed, as DIR/*.npy
    python bench.py --gpus 1 --steps 10 --warmup 3 --full               # + the NT GEMM roofline and every key below the headline
    python bench.py --gpus N ...                                  # no torchrun environment: starts N ranks itself (before any GPU call)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run measures the headline `value` and nothing else. `--full` adds the TF step's `roofline` (one extra profiled step after the timed ones) and,
unless a --no-* option drops them, `scst` (also with N ranks), then on one GPU `forward_only`, `tf_single`, `tf_dropin`, `scst_dropin`, `scst_c5`,
`beam_generation` and `cpu_baseline`; the headline steps, and what --dump-outputs writes, are the same with and without it.

BASELINE.json `metric` = "SCST steps/sec + TF tokens/sec/GPU, 2-image 384x384 studies":
  * headline (`value`): teacher-forcing tokens/s of the MULTI-image model (reference modules/lightning_modules/multi.py:182-210): 32 studies x 2
    images 384x384 per GPU, T = 256, CvT-21 + 6-layer BERT decoder, vocab 30000; one step = forward, cross-entropy, backward, AdamW under
    model.train(), bf16 MFMA with fp32 accumulation and fp32 master weights, synthetic data, random-init weights. Weak scaling (pure data
    parallel, study-level sharding), gradients all-reduced over RCCL.
  * `scst`: SCST steps/s at the per-GPU shape of configs[3] (16 studies x 2 images, 255 sampled + 255 greedy tokens, CXR-BERT stand-in reward,
    REINFORCE + AdamW on the decoder), with the roofline of its cached decode token-step. Since round 5 its `value` is the step with the reference's
    string round trip -- generated ids -> strings -> tokenizer -> reward (scst/gt_prompt.py:90-91,120-128,192-197) -- with the reward tokenizer
    TRUNCATED AT R = 128 tokens (the reference's own limit is 512: the same step at 512 is `scst.string_round_trip.r512`); the step with
    synthetic reward ids in place of the string round trip (rounds 1-4) stands beside it as `scst.synthetic_ids`. Since round 6 the labels change
    every step in all variants: their rows are tokenised and embedded inside the timed step.
  * `tf_single`: configs[1] (single-image studies, batch 32), `forward_only`: bf16 MFMA utilisation of the encoder + decoder FORWARD (the
    north_star's >= 40 % target is defined on it), `cpu_baseline`: the oracle/ restatement of the reference path on the host cores.
  (`scst` and everything in this list: --full only.)
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic work: forward FLOPs, training = 3x forward for trainable parts
ENC_FWD_GF_PER_IMAGE = 50.04
MFMA_BF16_PEAK_TF = 2500.0
MFMA_FP8_PEAK_TF = 5000.0        # dense e4m3 (MI355X_MICROARCH.md; not the 2:1-sparsity headline)
HBM_PEAK_GBS = 8000.0


def dec_fwd_gf(n_images, T):
    return 8.15 * n_images + T * (146.4 + 10.6 * n_images + 0.0184 * T) * 1e-3


def decode_step_bytes(rows, studies, n_images, t_ctx, layers=6, d=768, vocab=30000):
    """Algorithmic bytes of ONE cached decode token-step: decoder weights once (bf16), cross-attention K/V of every study once
    (the sampled and the greedy row of a study share them), self-attention K/V of every row up to context t, fp32 logits."""
    weights = 160e6
    cross = studies * layers * 2 * (n_images * 576) * d * 2
    self_kv = rows * layers * 2 * t_ctx * d * 2
    return weights + cross + self_kv + rows * vocab * 4


# CXR_BENCH_REHEARSAL=1: the SAME control flow (rank spawn, affinity masks, rendezvous, per-rank seeds, barriers, max-over-ranks timing, all-reduces,
# the SCST gather, the one JSON line of rank 0) on the tiny parity-test configuration, so that `bench.py --gpus N` can be rehearsed with N ranks
# sharing ONE GPU (CXR_SINGLE_DEVICE=1 CXR_DIST_BACKEND=gloo) -- tests/test_dp_gpu.py. The line it prints says "rehearsal": it is never a number.
REHEARSAL = os.environ.get("CXR_BENCH_REHEARSAL") == "1"
IMG = 96 if REHEARSAL else 384


def bench_config(lora=False):
    from cxrmate_amd.config import EncoderDecoderConfig, tiny_config
    if REHEARSAL:
        return tiny_config(vocab_size=1000, decoder_layers=2, image_size=IMG, lora_r=8 if lora else 0)
    return EncoderDecoderConfig()


def synth_batch(B, T, vocab, device, seed, n_images=1):
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(B, 3, IMG, IMG, generator=g) if n_images == 1 else torch.randn(B, n_images, 3, IMG, IMG, generator=g)
    full = torch.randint(12, vocab, (B, T + 1), generator=g)
    full[:, 0] = 1
    full[:, T // 2] = 3
    inp, lab = full[:, :-1].contiguous(), full[:, 1:].contiguous()
    am = torch.ones(B, T, dtype=torch.int64)
    return px.to(device), inp.to(device), am.to(device), lab.to(device)


def cpu_baseline(T, vocab, n_images, budget_s=25.0, threads=None):
    """The CPU restatement of the reference path (oracle/, fp32): multi-image TF fwd + bwd + AdamW on a bounded sample. Thread count: measured
    best on the GPU host for this small-batch workload (8/16/32/64/128 threads gave 259/291/222/106/29 tokens/s); reported as `cores`."""
    threads = threads or int(os.environ.get("CXR_CPU_THREADS", min(16, os.cpu_count() or 1)))
    torch.set_num_threads(threads)
    from cxrmate_amd import weights
    from cxrmate_amd.config import EncoderDecoderConfig
    from oracle import bert as obert, cvt as ocvt, generate as ogen
    cfg = EncoderDecoderConfig()
    cfg.decoder.vocab_size = vocab
    sd = weights.init_encoder_decoder(cfg, seed=0)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype == torch.float32 and not weights.is_buffer(k)
              and k not in weights.tied_aliases(cfg.decoder)}
    sd2 = dict(sd)
    sd2.update(leaves)
    opt = torch.optim.AdamW(list(leaves.values()), lr=5e-5)
    B = 1
    px, inp, am, lab = synth_batch(B, T, vocab, "cpu", 123, n_images)
    tt = torch.from_numpy(__import__("oracle.token_ops", fromlist=["x"]).token_ids_to_token_type_ids(inp.numpy(), [3]))

    def step():
        opt.zero_grad(set_to_none=True)
        h, mask = ocvt.encoder_forward(px, sd2, cfg.encoder)
        logits = obert.decoder_forward(inp, sd2, cfg.decoder, h, mask, am, tt, None)
        loss = ogen.tf_cross_entropy(logits, lab, 4)
        loss.backward()
        opt.step()

    step()                                  # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        step()
        n += 1
        dt = time.perf_counter() - t0
        if dt > budget_s * 0.6 or n >= 8:
            break
    return {"value": n * B * T / dt, "unit": "tokens/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{n} TF steps (fwd+bwd+AdamW), batch {B} study x {n_images} images 384x384, T={T}, fp32, oracle/ restatement of the reference path"}


def timed(step, steps, world, dev):
    """barrier + synchronize, exactly `steps` steps, synchronize + barrier; MAX over ranks. -> (seconds, last result)"""
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    return dt, out


def decode_traffic(c5=False):
    """HBM-side bytes per cached token-step from the committed PMC passes (profiles/r06_pmc_decode_hbm_traffic.json, r06_pmc_decode_c5_hbm_traffic.json: rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE in separate runs over one sample+greedy decode of the configs[3] / configs[4] shape, kernels launched one by one -- counters cannot
    be collected live, and hipGraph replays under --pmc take tens of minutes): the decode-step kernels only (the encoder / prefill kernels of the
    same run are left out)."""
    for name in (("r06_pmc_decode_c5_hbm_traffic.json", "r03_pmc_decode_c5_hbm_traffic.json") if c5 else ("r06_pmc_decode_hbm_traffic.json", "r03_pmc_decode_hbm_traffic.json", "r02_pmc_decode_hbm_traffic.json")):
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", name)
        if os.path.exists(path):
            pmc = json.load(open(path))
            fams = ("dec_gemm", "attn_decode", "token_selection", "step_inputs_embedding")
            return (sum(pmc[f]["hbm_bytes_per_unit"] for f in fams if f in pmc),
                    f"profiles/{name} (FETCH_SIZE x2 + WRITE_SIZE per token-step of dec_gemm + attn_decode + token selection + step inputs kernels, "
                    "separate --pmc passes)")
    return None, None


def scst_bench(args, rank, world, dev, steps, c5=False):
    """BASELINE.json configs[3] per-GPU shape: 16 studies x 2 images, prompt [PMT][NPF][PMT-SEP][NPI][BOS], 255 sampled + 255 greedy tokens
    (EOS disabled so the work is deterministic), CXR-BERT stand-in reward on R = 128 synthetic WordPiece ids, REINFORCE + AdamW on the whole
    decoder, RCCL all-reduce of 80.9 M gradients + all-gather of the sequences.
    c5: BASELINE.json configs[4] -- 3 images per study, a 128-token prior-report prompt [PMT] 62 x token [PMT-SEP] 63 x token [BOS], the frozen
    encoder's linear layers as e4m3 (OCP) MFMA GEMMs (per-tensor scales calibrated on another synthetic batch)."""
    from cxrmate_amd.config import EncoderDecoderConfig
    from cxrmate_amd.modelling import LongitudinalPromptMultiCXREncoderDecoderModel
    from cxrmate_amd.reward import CXRBERTReward
    from cxrmate_amd.scst import scst_step
    from cxrmate_amd.training import FusedAdamW
    cfg = bench_config(lora=True)
    B, N = (2 if REHEARSAL else 16), (3 if c5 else 2)
    model = LongitudinalPromptMultiCXREncoderDecoderModel(cfg, device=dev, seed=0)
    if not args.eval_mode:
        model.train()          # the reference never leaves train mode inside training_step
    for p in model.decoder.parameters():
        p.requires_grad_(True)                                   # scst/gt_prompt.py:38-40
    opt = FusedAdamW(model, lr=5e-6)
    reward = CXRBERTReward(dev, seed=1)
    g = torch.Generator().manual_seed(2000 + rank)
    images = torch.randn(B, N, 3, IMG, IMG, generator=g).to(dev)
    enc_ms = None

    def enc_time():
        with torch.no_grad():
            for _ in range(2):
                model.encoder(images)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                model.encoder(images)
            e1.record()
            torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 5

    t16 = enc_time()                                             # the step's frozen-encoder forward on its own (train-mode BatchNorm, no_grad)
    if c5:
        prompt = torch.cat([torch.full((B, 1), 8), torch.randint(12, 30000, (B, 62), generator=g), torch.full((B, 1), 9),
                            torch.randint(12, 30000, (B, 63), generator=g), torch.full((B, 1), 1)], 1).to(dev)
        model.enable_fp8_encoder(torch.randn(4, N, 3, 384, 384, generator=g).to(dev))
        enc_ms = {"bf16": t16, "e4m3": enc_time(), "images": B * N}
    else:
        prompt = torch.tensor([[8, 10, 9, 11, 1]] * B, device=dev)
        enc_ms = {"bf16": t16, "images": B * N}
    # labels change every step, as in training (a new mini-batch of studies): a pool of label id matrices, one per step; the label rows are embedded
    # INSIDE the timed step (once per step: the reference embeds them in both of its reward calls, tools/rewards/cxrbert.py:49-64)
    n_pool = 64
    label_pool = torch.randint(1000, 30000, (n_pool, B, 128), generator=g).to(dev)
    ones = torch.ones(B, 128, dtype=torch.int64, device=dev)
    step_no = {"k": 0}

    def retok(ids):                                               # ids [B, L] -> synthetic "re-tokenised" R=128 WordPiece ids
        pred = torch.zeros(ids.shape[0], 128, dtype=torch.int64, device=dev)
        n = min(128, ids.shape[1])
        pred[:, :n] = ids[:, :n] % 30522
        return pred

    def reward_fn(ids):
        return reward.reward_from_ids(retok(ids), ones, label_pool[step_no["k"] % n_pool], ones)

    def reward_pair(a, b):                           # sampled + greedy + THIS STEP'S label rows as ONE 3B-row CXR-BERT forward (labels embedded once per step)
        from cxrmate_amd import ops
        e = reward.embed_ids(torch.cat([retok(a), retok(b), label_pool[step_no["k"] % n_pool]], 0), torch.cat([ones, ones, ones], 0))
        r = ops.cosine_rows(e[:2 * B], torch.cat([e[2 * B:], e[2 * B:]], 0))
        return r[:B], r[B:]

    reward_fn.pair = reward_pair

    special = dict(bos=1, eos=None, sep=3, pad=4, pmt_sep=9)

    def step():
        step_no["k"] += 1
        return scst_step(model, opt, reward_fn, images, prompt, None, special, decoder_max_len=args.new_tokens + 1)

    for _ in range(max(2, args.warmup)):                          # the first two steps capture the decode hipGraphs (sample + greedy)
        step()
    dt, out = timed(step, steps, world, dev)
    # what the label rows cost: the reward forward with and without them, alone on the stream (HIP events; inside the step they ride in one launch chain)
    with torch.no_grad():
        pa = torch.cat([retok(label_pool[1]), retok(label_pool[2])], 0)

        def fwd_ms(with_labels):
            ids = torch.cat([pa, label_pool[3]], 0) if with_labels else pa
            m_ = torch.ones_like(ids)
            for _ in range(2):
                reward.embed_ids(ids, m_)
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            for _ in range(5):
                reward.embed_ids(ids, m_)
            a1.record()
            torch.cuda.synchronize()
            return a0.elapsed_time(a1) / 5
        label_forward = {"reward_forward_2B_rows_ms": fwd_ms(False), "reward_forward_3B_rows_with_labels_ms": fwd_ms(True),
                         "separate_B_row_label_forward_ms": None}
        lab1 = label_pool[4]
        for _ in range(2):
            reward.embed_ids(lab1, ones)
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        for _ in range(5):
            reward.embed_ids(lab1, ones)
        a1.record()
        torch.cuda.synchronize()
        label_forward["separate_B_row_label_forward_ms"] = a0.elapsed_time(a1) / 5
        label_forward["label_forward_ms"] = label_forward["reward_forward_3B_rows_with_labels_ms"] - label_forward["reward_forward_2B_rows_ms"]
        label_forward["what"] = ("labels change every step; their B rows are embedded inside the timed step, once per step, in the same forward as the 2B prediction "
                                 "rows (the reference embeds them in each of its two reward calls per step)")
    # the cached decode of one step, timed live with HIP events on the launch stream (the graph replays run on torch's current stream)
    with torch.no_grad():
        eo = model.encoder(images)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.sample_and_greedy(eo, prompt, [1, 3], [9, 1, 3], 4, args.new_tokens + 1 + prompt.shape[1], 1, None, 4)
        e1.record()
        torch.cuda.synchronize()
    strings = None
    if not c5 and not REHEARSAL:
        try:
            strings = scst_string_round_trip(args, model, opt, images, prompt, special, dev, B, steps=steps, world=world)
        except Exception as e:                                    # transformers / the fixture tokenizer missing (the same on every rank): the synthetic-id
            strings = {"error": str(e)}                           # number stands alone and `headline_is` says so
    n_tok = args.new_tokens
    dec_ms = e0.elapsed_time(e1)
    t_ctx = prompt.shape[1] + n_tok / 2.0                          # mean self-attention context over the decode
    step_bytes = decode_step_bytes(2 * B, B, N, t_ctx)
    achieved = step_bytes / (dec_ms * 1e-3 / n_tok) / 1e9
    if c5:
        return {"metric": "scst_steps_per_sec", "value": world * steps / dt, "unit": "steps/s (16 studies x 3 images per GPU per step; all GPUs)",
                "steps": steps, "ms_per_step": dt / steps * 1e3, "studies_per_sec": world * B * steps / dt, "new_tokens_sampled_and_greedy": n_tok,
                "prompt_tokens": int(prompt.shape[1]), "encoder_forward_ms": enc_ms,
                "encoder_roofline": {"bound": "mfma", "kernel": "frozen CvT-21 forward, 99.5 % of its MACs in gemm_fp8_kernel (v_mfma_scale_f32_32x32x64_f8f6f4, e4m3)",
                                     "achieved": ENC_FWD_GF_PER_IMAGE * enc_ms["images"] / enc_ms["e4m3"], "peak": MFMA_FP8_PEAK_TF, "unit": "TFLOP/s",
                                     "frac": ENC_FWD_GF_PER_IMAGE * enc_ms["images"] / enc_ms["e4m3"] / MFMA_FP8_PEAK_TF,
                                     "bf16_achieved": ENC_FWD_GF_PER_IMAGE * enc_ms["images"] / enc_ms["bf16"],
                                     "what": "algorithmic encoder FLOPs (BASELINE.md section 2) of the step's 48 images / HIP-event time of the forward, train-mode BatchNorm"},
                "decode_ms_per_step": dec_ms, "labels": "change every step (embedded inside the timed step)", "label_forward": label_forward,
                "us_per_token_step": dec_ms * 1e3 / n_tok, "loss": float(out["loss"].item()),
                "workload": "BASELINE.json configs[4] per-GPU shape: 16 studies x 3 images, 128-token prior-report prompt, frozen encoder with e4m3 "
                            "(OCP) MFMA linear layers (static per-tensor scales), sample + greedy as one 32-row cached decode, REINFORCE + AdamW; "
                            "the reference runs this path at batch 1 (scst/gen_prompt.py:38), the batch here is the C4 batch",
                "roofline": {"bound": "hbm", "kernel": "cached decode token-step, 32 rows, 1728 encoder keys", "achieved": achieved, "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": decode_traffic(True)[0], "traffic_unit": "bytes per token-step",
                             "traffic_source": decode_traffic(True)[1], "algorithmic_bytes_per_token_step": step_bytes,
                             "profile": "profiles/r06_scst_c5_decode_kernel_stats.csv (rocprofv3 --kernel-trace --stats of scripts/scst_c5_decode_profile.py)"}}
    # The HEADLINE of this key is the reference's step: decode -> strings -> tokenizer -> reward (scst/gt_prompt.py:90-91,120-128,192-197) at R = 128
    # reward tokens. The same step with R = 128 SYNTHETIC ids in place of the string round trip (what rounds 1-4 reported as `value`) stands beside
    # it as `synthetic_ids`: equal GPU work, no host string work.
    synth = {"value": world * steps / dt, "ms_per_step": dt / steps * 1e3, "steps": steps, "loss": float(out["loss"].item()),
             "labels": "change every step (embedded inside the timed step)", "label_forward": label_forward,
             "what": "retok(ids) % 30522 on the device in place of decode -> strings -> tokenizer (rounds 1-4 headline; since round 6 with new labels every step)"}
    head_dt = (strings["ms_per_step"] * 1e-3 * steps) if (strings and strings.get("ms_per_step")) else dt
    if strings and strings.get("ms_per_step"):
        strings["vs_synthetic_ids_step"] = strings["ms_per_step"] / synth["ms_per_step"]
    return {"metric": "scst_steps_per_sec", "value": world * steps / head_dt, "unit": "steps/s (16 studies x 2 images per GPU per step; all GPUs)",
            "headline_is": "string_round_trip" if head_dt is not dt else "synthetic_ids",
            "steps_per_sec_per_gpu": steps / head_dt, "steps": steps, "ms_per_step": head_dt / steps * 1e3, "studies_per_sec": world * B * steps / head_dt,
            "new_tokens_sampled_and_greedy": n_tok, "synthetic_ids": synth,
            "labels": "change every step: new label strings / ids per step, tokenised and embedded inside the timed step (once per step)",
            "reward": "CXR-BERT stand-in (BERT-base + CLS projection head: architecture assumed, PARITY UNPINNED -- SURVEY.md 8c), reward tokenizer truncated at "
                      "R = 128 on both paths (SURVEY.md 8d; the reference's limit is 512: `string_round_trip.r512`), ONE 48-row forward per step (sampled + greedy "
                      "+ this step's label rows together)",
            "workload": "BASELINE.json configs[3] per-GPU shape: sample (top-k 50) + greedy baseline as one 32-row cached decode replayed from "
                        "hipGraphs, REINFORCE through one teacher-forced pass, AdamW on the 80.9 M decoder parameters",
            "mode": "eval" if args.eval_mode else "model.train(): batch-statistics BatchNorm in the frozen encoder, dropout 0.1 in both decodes and in "
                    "the re-scoring pass (same seed)", "loss": float(out["loss"].item()), "string_round_trip": strings,
            "encoder_forward_ms": enc_ms,
            "encoder_roofline": {"bound": "mfma", "kernel": "frozen CvT-21 forward of the step's 32 images (bf16 NT GEMMs: row-strip / W-stationary / persistent / tiled)",
                                 "achieved": ENC_FWD_GF_PER_IMAGE * enc_ms["images"] / enc_ms["bf16"], "peak": MFMA_BF16_PEAK_TF, "unit": "TFLOP/s",
                                 "frac": ENC_FWD_GF_PER_IMAGE * enc_ms["images"] / enc_ms["bf16"] / MFMA_BF16_PEAK_TF,
                                 "what": "algorithmic encoder FLOPs (BASELINE.md section 2) of the step's images / HIP-event time of the forward, no_grad, train-mode BatchNorm"},
            "roofline": {"bound": "hbm", "kernel": "cached decode token-step (one hipGraph of ~48 kernels: dec_gemm_kernel x32, attn_cross_mfma_kernel (query projection inside) x6, attn_decode_kernel x6, "
                         "embedding, step inputs, token selection), 32 rows", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": decode_traffic()[0], "traffic_unit": "bytes per token-step",
                         "traffic_source": decode_traffic()[1], "algorithmic_bytes_per_token_step": step_bytes,
                         "decode_ms_per_step": dec_ms, "us_per_token_step": dec_ms * 1e3 / n_tok,
                         "decode_share_of_step": dec_ms / (head_dt / steps * 1e3),
                         "profile": "profiles/r06_scst_decode_kernel_stats.csv (rocprofv3 --kernel-trace --stats of scripts/scst_decode_profile.py)"}}


def beam_bench(args, dev, host_loop_too=True):
    """BASELINE.json configs[2] (test-set generation, the reference's evaluation path): 8 studies x 2 images, beam 4, up to 256 tokens, no EOS
    (all steps run: deterministic work). Device-side beam search: 32 beam-major rows on the cached-step kernels, the beams of a study sharing its
    cross-attention K/V, bookkeeping + cache reorder as two launches per token, steps replayed from hipGraphs. The encoder forward is inside the
    timed region, as in the reference's test_step."""
    from cxrmate_amd.config import EncoderDecoderConfig
    from cxrmate_amd.modelling import MultiCXREncoderDecoderModel
    cfg = EncoderDecoderConfig()
    B, N, L, nb = 8, 2, 256, 4
    model = MultiCXREncoderDecoderModel(cfg, device=dev, seed=0)
    model.eval()
    g = torch.Generator().manual_seed(3000)
    images = torch.randn(B, N, 3, 384, 384, generator=g).to(dev)

    def run():
        return model.generate(pixel_values=images, special_token_ids=[3], max_length=L, bos_token_id=1, eos_token_id=None, pad_token_id=4,
                              num_beams=nb, return_dict_in_generate=True, use_cache=True, output_scores=True)

    def clock(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            o = run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, o

    run(); run()                                                   # captures the step graphs
    dt, o = clock(3)
    res = {"metric": "beam_generation_studies_per_sec", "value": B / dt, "unit": "studies/s", "ms_per_batch": dt * 1e3,
           "generated_tokens_per_sec": B * (L - 1) / dt, "us_per_token_step": dt * 1e6 / (L - 1),
           "workload": "BASELINE.json configs[2]: cxrmate-multi-tf generate(num_beams=4, max_length=256), 8 studies x 2 images per batch, encoder "
                       "included, EOS disabled (255 steps always run)", "mean_sequence_score": float(o["sequences_scores"].mean())}
    if host_loop_too:                                              # the library-style host loop on the same kernels (A/B: what device-side bookkeeping buys)
        model.device_beam_search = False
        run()
        dt_h, _ = clock(1)
        model.device_beam_search = True
        res["host_loop_ms_per_batch"] = dt_h * 1e3
    return res


from cxrmate_amd.strings import FoldedVocabTokenizer as _InVocabTokenizer      # the 400-entry fixture byte-BPE in front of a random-init model that emits ids up to 30000


def scst_string_round_trip(args, model, opt, images, prompt, special, dev, B, steps=3, world=1):
    """The SCST step with the reference's REAL reward path (scst/gt_prompt.py:90-91,120-128,192-197): generated ids -> findings /
    impression strings (split_and_decode_sections + tokenizer.decode) -> CXR-BERT tokenizer -> BERT-base forwards, through reward.ReportReward on
    pinned host copies. Tokenizer: the synthetic byte-BPE of tests/golden (no real vocabulary offline). The tokenizer call truncates at R = 128
    (the reference's own limit is 512, tools/rewards/cxrbert.py:38): the reward BERT then sees as many tokens as on the synthetic-id
    path, so the two step times differ by the host's string work only. The same step at the reference's 512 limit is reported as `r512`."""
    import transformers
    from cxrmate_amd.reward import CXRBERTReward
    tok = transformers.PreTrainedTokenizerFast(tokenizer_file=os.path.join(ROOT, "tests", "golden", "tokenizer.json"), unk_token="[UNK]",
                                               pad_token="[PAD]", cls_token="[BOS]", sep_token="[SEP]", mask_token="[MASK]", bos_token="[BOS]",
                                               eos_token="[EOS]")
    # labels change every step, as in training: a pool of report-like label strings, B different ones per step (so neither the reward's label cache
    # nor the tokenizer sees a repeated batch inside the timed region); they are tokenised and embedded inside the timed step, once per step
    findings = ["The lungs are clear without focal consolidation.", "There is a small left pleural effusion.", "Heart size is mildly enlarged.",
                "No pneumothorax is seen.", "Bibasilar atelectasis is noted.", "The mediastinal contours are unremarkable.",
                "Interval placement of a right internal jugular catheter.", "Mild pulmonary vascular congestion."]
    impressions = ["No acute cardiopulmonary process.", "Findings suggest mild pulmonary edema.", "Stable appearance of the chest.",
                   "Small effusion, otherwise unremarkable.", "Possible early pneumonia in the right lower lobe."]

    def labels_of(k):
        return [[f"{findings[(k * 7 + b) % 8]} {findings[(k * 3 + 2 * b + 1) % 8]} Study {k * B + b}. {impressions[(k + b) % 5]}"] for b in range(B)]

    def run(max_length, n_steps):
        reward = CXRBERTReward(dev, tokenizer=tok, seed=1, max_length=max_length)
        return _scst_string_steps(args, model, opt, images, prompt, special, dev, B, reward, labels_of, tok, n_steps, world, max_length)
    res = run(128, steps)
    if os.environ.get("CXR_BENCH_R512", "1") != "0":
        # the same step with the reward tokenizer's limit at the reference's own 512 (tools/rewards/cxrbert.py:38): the 255 generated tokens decode through
        # the 400-entry byte-BPE fixture to strings of more than 128 reward tokens, so the reward BERT and the host tokenizer do more work here
        try:
            r512 = run(512, max(2, min(steps, 4)))
            res["r512"] = {k: r512[k] for k in ("ms_per_step", "steps_per_sec", "steps", "reward_tokens", "reward_token_rows", "string_worker")}
        except Exception as e:
            res["r512"] = {"error": str(e)}
    return res


def _scst_string_steps(args, model, opt, images, prompt, special, dev, B, reward, labels_of, tok, steps, world, max_length):
    from cxrmate_amd.reward import ReportReward
    from cxrmate_amd.scst import scst_step
    labels = labels_of(0)
    # The CPU part of the reward (ids -> strings -> reward-tokenizer ids) runs in a child process beside this process's kernel launches
    # (reward.ReportReward(worker=True); CXR_STRING_WORKER=0: in-process). Host / GPU timeline of the step, scripts/r5/scst_timeline.py: in-process the GPU
    # idles ~3 ms between the re-scoring forward and the reward forward while the host turns ids into strings into ids (105.7 ms per step); with the child
    # process the host only waits for the child's answer (103.9 ms). Same-box alternations of the bench key: -0.9 to -1.8 ms. Any failure of the child falls
    # back to the in-process path (time-outs on every wait).
    rfn = ReportReward(model, _InVocabTokenizer(tok), reward, labels, 1, 3, 2, worker=os.environ.get("CXR_STRING_WORKER", "1") != "0")

    k = {"k": 0}
    widths = []
    embed_ids = reward.embed_ids

    def counting_embed(ids, mask):                                # (bookkeeping only: rows x tokens of every reward forward)
        widths.append(tuple(ids.shape))
        return embed_ids(ids, mask)
    reward.embed_ids = counting_embed

    def step():
        k["k"] += 1
        rfn.labels = labels_of(k["k"])                            # a new mini-batch's labels
        return scst_step(model, opt, rfn, images, prompt, None, special, decoder_max_len=args.new_tokens + 1, reward_on_host=True)

    try:
        step()
        used0 = rfn.worker_used
        del widths[:]
        dt, out = timed(step, steps, world, dev)
        served = rfn.worker_used - used0
    finally:
        rfn.close()
    dt /= steps
    return {"ms_per_step": dt * 1e3, "steps_per_sec": world / dt, "steps": steps, "loss": float(out["loss"].item()), "reward_tokens": max_length,
            "reward_token_rows": {"forwards_per_step": len(widths) / max(steps, 1), "rows_x_tokens_of_the_last_forward": list(widths[-1]) if widths else None},
            "labels": "B new label strings every step, tokenised beside the children's string work and embedded in the predictions' forward",
            "string_worker": {"steps_served_by_the_child_process": served, "of": steps},
            "host_ms": {"ids_to_strings": getattr(rfn, "last_decode_ms", None), "strings_to_ids": getattr(reward, "last_tokenize_ms", None),
                        "note": "in-process path only (the child process does this work when it serves a step)"},
            "what": "scst_step(reward_on_host=True) with reward.ReportReward: async pinned copies of the sequences; all sections decoded by one call into the tokenizers "
                    "library and both halves re-tokenised by one call (truncated to R = 128) -- in four child processes, two per half of the rows (strings.StringWorker; "
                    "CXR_STRING_WORKERS = 2: one per half; CXR_STRING_WORKER=0 or any failure of a child: in this process) beside the launches of the re-scoring forward + warper threshold --, token ids uploaded through a pinned staging buffer, "
                    "one 48-row CXR-BERT forward (sampled + greedy + this step's label rows); synthetic byte-BPE tokenizer (tests/golden/tokenizer.json) on the random-init model's strings"}


DUMP_SAMPLE = 1 << 22          # master weights written by --dump-outputs: this many (16 MB of fp32), drawn with replacement, seed 0


def tf_bench(args, rank, world, dev, model, n_images, steps, profile_gemm, dump=False):
    """One teacher-forcing optimisation step = forward, CE, backward, (all-reduce,) AdamW. -> dict with tokens/s, ms/step and, optionally, the
    live GEMM profile and (dump=True) what the last timed step handed back: its loss and a fixed sample of the updated fp32 master weights."""
    from cxrmate_amd import ops
    from cxrmate_amd.training import FusedAdamW, GraphedTFStep, tf_train_step
    B, T, V = args.batch, args.seq_len, model.config.decoder.vocab_size
    opt = FusedAdamW(model, lr=5e-5)
    px, inp, am, lab = synth_batch(B, T, V, dev, 1000 + rank, n_images)
    tt = model.token_ids_to_token_type_ids(inp, [3])

    def eager_step():
        return tf_train_step(model, opt, px, inp, am, tt, lab, pad_token_id=4)

    if os.environ.get("CXR_BENCH_SYNC_EACH") == "1":            # lab switch: the host does not run ahead of the GPU across steps
        def step():
            out = eager_step()
            torch.cuda.synchronize()
            return out
    elif not args.graph:
        step = eager_step
    else:
        graphed = GraphedTFStep(model, opt, px, inp, am, tt, lab, pad_token_id=4)          # hipGraph capture (3 segments)
        step = lambda: graphed(px, inp, am, tt, lab)
    # untimed pre-warm-up: lazy kernel loading, caching-allocator growth on both streams, first-use buffers (transposed weights, LoRA merges)
    # and the device itself -- the first ~second of work on a fresh box runs 5-8 % slow, which 3 warm-up steps do not cover. A FIXED number of
    # steps (40 = ~1.6 s of the 39.5 ms headline step on one GPU), so that the same arguments put the same model state into the timed steps
    # (--dump-outputs) and every rank runs as many steps as the others (each one all-reduces); the W requested warm-up steps follow.
    n_fixed = int(os.environ.get("CXR_BENCH_PREWARM", "32" if world > 1 else "40"))     # (a rehearsal of the multi-rank flow on one GPU sets 2)
    for n_pre in range(n_fixed):
        step()
        if n_pre % 4 == 3:
            torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    dt, loss = timed(step, steps, world, dev)
    res = {"ms_per_step": dt / steps * 1e3, "tokens_per_s": world * B * T * steps / dt, "loss": float(loss.item()),
           "step_gflop_per_gpu": 3.0 * (ENC_FWD_GF_PER_IMAGE * n_images + dec_fwd_gf(n_images, T)) * B}
    if dump:                                # before the profiled step below moves the weights on
        w = model.flat32[: model._param_total]
        idx = torch.randint(0, w.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).to(w.device)
        res["dump"] = {"tf_loss": loss.detach().float().reshape(-1).cpu().numpy(),
                       "tf_master_weights_sample": w[idx].float().cpu().numpy()}
    if profile_gemm:
        # dominant kernel = gemm_nt_kernel (bf16 MFMA): live HIP-event timing of every launch in one extra step
        ops.GEMM_PROFILE = []
        eager_step()
        torch.cuda.synchronize()
        prof, ops.GEMM_PROFILE = ops.GEMM_PROFILE, None
        nt = [p for p in prof if p[3][0] != "tn"]                # dominant kernel: gemm_nt_kernel (forward + dX products)
        tn = [p for p in prof if p[3][0] == "tn"]                # weight-gradient kernel (runs concurrently on the side stream)
        res["gemm"] = dict(nt_ms=sum(p[1].elapsed_time(p[2]) for p in nt), nt_flops=sum(p[0] for p in nt), nt_bytes=sum(p[4] for p in nt),
                           nt_n=len(nt), tn_ms=sum(p[1].elapsed_time(p[2]) for p in tn), tn_flops=sum(p[0] for p in tn), tn_n=len(tn))
    del opt
    return res


def forward_only(args, dev, model, n_images):
    """bf16 MFMA utilisation of the encoder + decoder FORWARD (no saved activations, no loss): algorithmic FLOPs of BASELINE.md section 2 over
    HIP-event time on the launch stream."""
    B, T, V = args.batch, args.seq_len, model.config.decoder.vocab_size
    px, inp, am, lab = synth_batch(B, T, V, dev, 77, n_images)
    tt = model.token_ids_to_token_type_ids(inp, [3])
    with torch.no_grad():
        def fwd():
            return model(pixel_values=px, decoder_input_ids=inp, decoder_attention_mask=am, decoder_token_type_ids=tt).logits
        for _ in range(3):
            fwd()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 8
        e0.record()
        for _ in range(n):
            fwd()
        e1.record()
        torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    gf = (ENC_FWD_GF_PER_IMAGE * n_images + dec_fwd_gf(n_images, T)) * B
    tf = gf * 1e-3 / (ms * 1e-3)
    return {"ms": ms, "gflop": gf, "achieved": tf, "peak": MFMA_BF16_PEAK_TF, "unit": "TFLOP/s", "frac": tf / MFMA_BF16_PEAK_TF,
            "what": f"encoder + decoder forward, {B} studies x {n_images} images, T = {T}, "
                    + ("model.train()" if model.training else "model.eval()") + ", algorithmic FLOPs (2 x MAC) / HIP-event time"}


def tf_dropin(args, dev, n_images, steps=6):
    """What a reference caller gets from the drop-in boundary: the call sequence of the reference's TF training_step (modules/lightning_modules/
    single.py:449-475, multi.py:182-210) against cxrmate_amd's model class, with torch doing what the caller does itself -- fp32 `.logits` out
    of the model, `F.cross_entropy(logits.permute(0, 2, 1), labels, ignore_index=pad)`, `loss.backward()` through the autograd bridges,
    `torch.optim.AdamW(model.parameters())` (single.py:426-431). Same workload as the headline number."""
    from cxrmate_amd.config import EncoderDecoderConfig
    from cxrmate_amd.modelling import MultiCXREncoderDecoderModel, SingleCXREncoderDecoderModel
    cfg = EncoderDecoderConfig()
    B, T, V = args.batch, args.seq_len, cfg.decoder.vocab_size
    model = (MultiCXREncoderDecoderModel if n_images > 1 else SingleCXREncoderDecoderModel)(cfg, device=dev, seed=0)
    if not args.eval_mode:
        model.train()
    # configure_optimizers (single.py:426-431) with the optimiser class this build offers for it: torch.optim.AdamW's interface on the fused kernel
    # (cxrmate_amd/optim.py); CXR_DROPIN_TORCH_ADAMW=1 keeps torch's own class (its foreach kernels cost ~3.5 ms per step on 112 M parameters)
    from cxrmate_amd.optim import AdamW as FusedTorchAdamW
    torch_adamw = os.environ.get("CXR_DROPIN_TORCH_ADAMW") == "1"
    opt = (torch.optim.AdamW if torch_adamw else FusedTorchAdamW)(model.parameters(), lr=5e-5)
    px, inp, am, lab = synth_batch(B, T, V, dev, 1000, n_images)

    def step():
        tt = model.token_ids_to_token_type_ids(inp, [3])                       # single.py:458-461
        y_hat = model(pixel_values=px, decoder_input_ids=inp, decoder_attention_mask=am, decoder_token_type_ids=tt, return_dict=True).logits
        loss = torch.nn.functional.cross_entropy(y_hat.permute([0, 2, 1]), lab, ignore_index=4)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    for _ in range(3):
        step()
    dt, loss = timed(step, steps, 1, dev)
    return {"ms_per_step": dt / steps * 1e3, "tokens_per_s": B * T * steps / dt, "steps": steps, "loss": float(loss.item()),
            "optimizer": "torch.optim.AdamW" if torch_adamw else "cxrmate_amd.optim.AdamW (torch.optim.Optimizer subclass on the fused kernel)",
            "what": "reference TF caller sequence on the drop-in classes: model(...).logits (fp32 [B,T,30000], autograd bridges) -> "
                    "F.cross_entropy(logits.permute(0,2,1), labels, ignore_index=pad) -> loss.backward() -> optimizer.step(), "
                    f"{B} studies x {n_images} images, T = {T}, " + ("model.eval()" if args.eval_mode else "model.train()")}


def scst_dropin(args, dev, steps=3):
    """The reference's SCST caller sequence (modules/lightning_modules/longitudinal/scst/gt_prompt.py:62-142, sample :144-209, reinforce_loss
    :211-246) against the drop-in classes at the configs[3] per-GPU shape: tokenize_prompt -> encoder -> generate.__wrapped__(do_sample,
    output_scores) -> torch.stack(scores, -1) -> split_and_decode_sections -> reward(strings) -> greedy generate -> strings -> reward ->
    log_softmax / nll_loss over the [B, V, T] stack -> backward -> torch.optim.AdamW. Synthetic byte-BPE tokenizer (tests/golden); EOS
    disabled so that all 255 steps run, as in the fused `scst` number."""
    import transformers
    from cxrmate_amd.config import EncoderDecoderConfig
    from cxrmate_amd.modelling import LongitudinalPromptMultiCXREncoderDecoderModel
    from cxrmate_amd.reward import CXRBERTReward
    cfg = EncoderDecoderConfig()
    B, N = 16, 2
    model = LongitudinalPromptMultiCXREncoderDecoderModel(cfg, device=dev, seed=0)
    if not args.eval_mode:
        model.train()
    for p in model.encoder.parameters():
        p.requires_grad = False                                                  # scst/gt_prompt.py:34-40
    for p in model.decoder.parameters():
        p.requires_grad = True
    from cxrmate_amd.optim import AdamW as FusedTorchAdamW
    torch_adamw = os.environ.get("CXR_DROPIN_TORCH_ADAMW") == "1"
    opt = (torch.optim.AdamW if torch_adamw else FusedTorchAdamW)([p for p in model.parameters() if p.requires_grad], lr=5e-6)
    tok = transformers.PreTrainedTokenizerFast(tokenizer_file=os.path.join(ROOT, "tests", "golden", "tokenizer.json"), unk_token="[UNK]",
                                               pad_token="[PAD]", cls_token="[BOS]", sep_token="[SEP]", mask_token="[MASK]", bos_token="[BOS]",
                                               eos_token="[EOS]", additional_special_tokens=["[PMT]", "[PMT-SEP]", "[NPF]", "[NPI]"])
    dec_tok = _InVocabTokenizer(tok)
    reward_model = CXRBERTReward(dev, tokenizer=tok, seed=1)
    images = torch.randn(B, N, 3, 384, 384, generator=torch.Generator().manual_seed(2000)).to(dev)
    batch = {"previous_findings": [None] * B, "previous_impression": [None] * B,
             "findings": ["The lungs are clear without focal consolidation. No pleural effusion or pneumothorax."] * B,
             "impression": ["No acute cardiopulmonary process."] * B}
    bos, eos, sep, pad = tok.bos_token_id, None, tok.sep_token_id, tok.pad_token_id
    pmt_sep = tok.convert_tokens_to_ids("[PMT-SEP]")
    max_len = args.new_tokens + 1
    step_no = {"k": 0}

    def step():
        step_no["k"] += 1                                          # a new mini-batch's labels every step (no label cache hit inside the timed region)
        batch["impression"] = [f"No acute cardiopulmonary process. Study {step_no['k'] * B + b}." for b in range(B)]
        prompt = model.tokenize_prompt(batch["previous_findings"], batch["previous_impression"], tok, max_len, add_bos_token_id=True)
        ids = prompt["input_ids"].to(dev)
        encoder_outputs = model.encoder(images)
        sample = model.generate.__wrapped__(model, input_ids=ids, special_token_ids=[bos, sep], encoder_outputs=encoder_outputs, bos_token_id=bos,
                                            eos_token_id=eos, pad_token_id=pad, mask_token_id=pad, return_dict_in_generate=True, do_sample=True,
                                            num_beams=1, use_cache=True, output_scores=True, top_p=1.0, top_k=50, temperature=1.0,
                                            max_new_tokens=max_len - 1)
        if torch.all(sample["sequences"][:, 0] == 1):
            sample["sequences"] = sample["sequences"][:, 1:]
        logits = torch.stack(sample["scores"], dim=-1)
        _, f, i = model.split_and_decode_sections(sample["sequences"], [bos, sep, tok.eos_token_id], dec_tok)
        sampled = sample["sequences"][:, ids.shape[1]:]
        labels = [[f"{a} {b}"] for a, b in zip(batch["findings"], batch["impression"])]
        reward = reward_model([f"{a} {b}" for a, b in zip(f, i)], labels).to(dev)
        base = model.generate(encoder_outputs=encoder_outputs, decoder_input_ids=ids, special_token_ids=[pmt_sep, bos, sep], max_length=max_len + ids.shape[1],
                              bos_token_id=bos, eos_token_id=eos, pad_token_id=pad, mask_token_id=pad, num_beams=1, return_dict_in_generate=True,
                              use_cache=True)["sequences"]
        if torch.all(base[:, 0] == 1):
            base = base[:, 1:]
        _, bf, bi = model.split_and_decode_sections(base, [bos, sep, tok.eos_token_id], dec_tok)
        baseline = reward_model([f"{a} {b}" for a, b in zip(bf, bi)], labels).to(dev)
        adv = reward - baseline
        loss = torch.nn.functional.nll_loss(torch.nn.functional.log_softmax(logits, dim=1), sampled, ignore_index=pad, reduction="none")
        loss = (loss.sum(dim=-1) * adv).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    for _ in range(2):
        step()
    dt, loss = timed(step, steps, 1, dev)
    return {"ms_per_step": dt / steps * 1e3, "steps_per_sec": steps / dt, "steps": steps, "loss": float(loss.item()),
            "what": "reference SCST caller sequence (scst/gt_prompt.py:62-246) on the drop-in classes: tokenize_prompt, encoder, generate.__wrapped__("
                    "do_sample=True, output_scores=True, top_k=50), torch.stack(scores, -1) [16, 30000, 255] fp32, split_and_decode_sections + string reward "
                    "twice, greedy generate, log_softmax / nll_loss, backward, optimizer.step() on the decoder; 16 studies x 2 images, 255 new tokens; labels "
                    "change every step (embedded inside the step, once: the second reward call finds them cached)",
            "optimizer": "torch.optim.AdamW" if torch_adamw else "cxrmate_amd.optim.AdamW (torch.optim.Optimizer subclass on the fused kernel)"}


def spawn_ranks(n):
    """`--gpus N` without a torchrun environment: start N fresh ranks of this script (one per GPU) BEFORE this process touches the GPU, relay
    rank 0's output, exit with the worst return code."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    cores = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        if len(cores) >= 2 * n and "CXR_CPU_AFFINITY" not in os.environ:
            # every rank needs ~17 ms of host time per 43 ms step (Python + ctypes launches): its own slice of the host cores, so that eight
            # ranks do not migrate over each other's caches (applied by the child before it touches the GPU, see main())
            per = len(cores) // n
            env["CXR_CPU_AFFINITY"] = ",".join(str(c) for c in cores[r * per:(r + 1) * per])
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
    sys.exit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="studies per GPU")
    ap.add_argument("--seq-len", type=int, default=256)
    ap.add_argument("--images", type=int, default=2, help="images per study of the headline teacher-forcing workload")
    ap.add_argument("--full", action="store_true", help="after the headline, also measure the TF step's GEMM roofline, scst, forward_only, tf_single, "
                    "tf_dropin, scst_dropin, scst_c5, beam_generation and cpu_baseline (a plain run measures the headline alone)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--no-scst", action="store_true", help="with --full: skip the SCST measurements")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip every one-GPU key but scst and cpu_baseline")
    ap.add_argument("--no-dropin", action="store_true", help="with --full: skip tf_dropin / scst_dropin (the reference callers' call sequences on the drop-in classes)")
    ap.add_argument("--scst-steps", type=int, default=10)
    ap.add_argument("--graph", action="store_true", help="replay the TF step from hipGraphs (3 segments)")
    ap.add_argument("--eval-mode", action="store_true", help="run the steps under model.eval() (running-statistics BatchNorm, no dropout)")
    ap.add_argument("--new-tokens", type=int, default=255)
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last timed teacher-forcing step computed as DIR/<name>.npy "
                    "(fp32: its loss and a fixed, seeded sample of the updated master weights)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args.gpus)

    aff = os.environ.get("CXR_CPU_AFFINITY")
    if not aff and int(os.environ.get("WORLD_SIZE", "1")) > 1 and hasattr(os, "sched_getaffinity"):
        # launched by torch.distributed.run (the driver's N > 1 command): the same per-rank slice of the host cores spawn_ranks hands out
        cores, nloc = sorted(os.sched_getaffinity(0)), int(os.environ.get("LOCAL_WORLD_SIZE", os.environ["WORLD_SIZE"]))
        lr = int(os.environ.get("LOCAL_RANK", "0"))
        if len(cores) >= 2 * nloc and lr < nloc:
            per = len(cores) // nloc
            aff = ",".join(str(c) for c in cores[lr * per:(lr + 1) * per])
    if aff and hasattr(os, "sched_setaffinity"):
        try:
            os.sched_setaffinity(0, {int(c) for c in aff.split(",") if c != ""})
            # ... and as many CPU threads as the slice has cores: torch otherwise starts one per core of the HOST in every rank (eight ranks drawing
            # their initial weights at once took 55 s each on a rehearsal box, oversubscribed 8 x)
            torch.set_num_threads(max(1, len(os.sched_getaffinity(0))))
        except (OSError, ValueError):
            pass
    elif int(os.environ.get("WORLD_SIZE", "1")) > 1 and hasattr(os, "sched_getaffinity"):
        torch.set_num_threads(max(1, len(os.sched_getaffinity(0)) // int(os.environ.get("LOCAL_WORLD_SIZE", os.environ["WORLD_SIZE"]))))
    from cxrmate_amd import dp
    rank, local, world = dp.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but the process group has {world} rank(s): refusing to report a {world}-GPU number")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # the train-mode steps draw their dropout / DropPath seeds from torch's generator, which otherwise starts from a different seed in every
    # process: seeded per rank (like the synthetic batch), the same arguments give the same masks, and --dump-outputs the same arrays
    torch.manual_seed(1000 + rank)

    from cxrmate_amd.config import EncoderDecoderConfig
    from cxrmate_amd.modelling import MultiCXREncoderDecoderModel, SingleCXREncoderDecoderModel

    cfg = bench_config()
    B, T, V = args.batch, args.seq_len, cfg.decoder.vocab_size
    N = args.images
    model = (MultiCXREncoderDecoderModel if N > 1 else SingleCXREncoderDecoderModel)(cfg, device=dev, seed=0)
    if not args.eval_mode:
        model.train()
    main_res = tf_bench(args, rank, world, dev, model, N, args.steps, profile_gemm=args.full, dump=bool(args.dump_outputs) and rank == 0)
    if "dump" in main_res:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in main_res.pop("dump").items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), arr)
    ms_per_step, tokens_per_s = main_res["ms_per_step"], main_res["tokens_per_s"]
    mode = ("eval-mode BatchNorm (running statistics), dropout off" if args.eval_mode else
            "model.train(): batch-statistics BatchNorm + running-stat update, dropout 0.1 (hidden + attention probabilities), DropPath")
    out = {
        **({"rehearsal": "CXR_BENCH_REHEARSAL=1: tiny configuration (96 x 96 images, CvT depth (1,2,3), 2 decoder layers, vocab 1000) -- a rehearsal of "
                         "the multi-rank control flow, NOT a measurement"} if REHEARSAL else {}),
        "metric": "tf_tokens_per_sec", "value": tokens_per_s, "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic (randn 384x384 images, uniform token ids, random-init weights)",
        "config": {"workload": f"cxrmate-multi-tf teacher-forcing fwd/bwd + AdamW on {N}-image 384x384 studies (BASELINE.json metric; reference "
                               "modules/lightning_modules/multi.py:182-210)", "global_batch": B * world, "studies_per_gpu": B, "images_per_study": N,
                   "seq_len": T, "encoder": "CvT-21 @384", "decoder": "BERT 6 layers, vocab 30000", "parallelism": f"dp{world}",
                   "rccl_ranks": world, "launch": "hipGraph replay (3 segments, RCCL between)" if args.graph else "eager, weight-gradient kernels on a side stream",
                   "mode": mode, "loss": main_res["loss"], "tokens_per_sec_per_gpu": tokens_per_s / world,
                   "model_tflops_per_gpu": main_res["step_gflop_per_gpu"] * 1e-3 / (ms_per_step * 1e-3)},
    }
    if not args.full:                                        # a plain run: the headline alone
        return report(out, rank, world)
    gm = main_res["gemm"]
    traffic, traffic_src = None, None                        # HBM-side bytes per launch from the committed PMC passes (cannot be collected live)
    for name in ("r06_pmc_tf_hbm_traffic.json", "r04_pmc_tf_hbm_traffic.json", "r03_pmc_tf_hbm_traffic.json", "r02_pmc_tf_hbm_traffic.json", "r01_pmc_hbm_traffic.json"):
        try:
            pmc = json.load(open(os.path.join(ROOT, "profiles", name)))
            traffic = pmc["gemm_nt"]["hbm_bytes_per_launch"]
            traffic_src = f"profiles/{name} (FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes" + ("" if not name.startswith("r01") else "; collected on configs[1] in round 1") + ")"
            break
        except Exception:
            pass
    achieved = gm["nt_flops"] / (gm["nt_ms"] * 1e-3) / 1e12
    out["roofline"] = {"bound": "mfma", "kernel": "NT GEMM family (gemm_nt_kernel tile variants, gemm_nt_group_kernel, the row-strip kernel gemm_strip384_kernel for the 384- / "
                                 "192-wide outputs of CvT stages 3 / 2, and in the forward pass the persistent gemm_nt_pk_kernel / gemm_ws384_kernel; "
                                 "v_mfma_f32_16x16x32_bf16), timed while the weight-gradient stream runs beside it, as in the timed region", "achieved": achieved,
                       "peak": MFMA_BF16_PEAK_TF, "unit": "TFLOP/s", "frac": achieved / MFMA_BF16_PEAK_TF, "traffic": traffic,
                       "traffic_unit": "bytes per launch", "traffic_source": traffic_src, "algorithmic_bytes_per_launch": gm["nt_bytes"] / max(1, gm["nt_n"]),
                       "launches_per_step": gm["nt_n"], "avg_launch_us": gm["nt_ms"] * 1e3 / max(1, gm["nt_n"]),
                       "avg_launch_gflop": gm["nt_flops"] / max(1, gm["nt_n"]) * 1e-9, "gemm_share_of_step": gm["nt_ms"] / ms_per_step,
                       "weight_grad_kernel": {"kernel": "gemm_tn_kernel (128x128 tiles) / gemm_tn2_kernel (256x256 blocks, long token runs) / gemm_tn5_kernel (384x192 blocks, CvT stage 3)", "launches_per_step": gm["tn_n"],
                                              "achieved": gm["tn_flops"] / (gm["tn_ms"] * 1e-3) / 1e12 if gm["tn_ms"] else None,
                                              "avg_launch_us": gm["tn_ms"] * 1e3 / max(1, gm["tn_n"])}}
    # the second workload of BASELINE.json with a number of its own (configs[3]) is measured right behind the headline, in front of the auxiliary keys: on
    # some boxes of the pool its MFMA-heavy phases run up to 8 ms per step slower after the long MFMA-heavy prelude the auxiliary TF keys make
    # (profiles/r04_ab_wgrad_stream.txt, calls 33 / 34); the headline key is measured first either way
    if not args.no_scst:
        try:
            out["scst"] = scst_bench(args, rank, world, dev, args.scst_steps)
        except Exception as e:
            if world > 1:
                raise
            out["scst"] = {"metric": "scst_steps_per_sec", "value": None, "error": str(e)}
    if world == 1 and not args.no_extras:
        try:
            out["forward_only"] = forward_only(args, dev, model, N)
        except Exception as e:
            out["forward_only"] = {"error": str(e)}
    del model
    torch.cuda.empty_cache()
    if world == 1 and not args.no_extras:
        try:
            single = SingleCXREncoderDecoderModel(cfg, device=dev, seed=0)
            if not args.eval_mode:
                single.train()
            r1 = tf_bench(args, rank, world, dev, single, 1, max(4, args.steps // 2), profile_gemm=False)
            out["tf_single"] = {"metric": "tf_tokens_per_sec", "value": r1["tokens_per_s"], "unit": "tokens/s", "ms_per_step": r1["ms_per_step"],
                                "workload": "cxrmate-single-tf teacher-forcing fwd/bwd + AdamW, batch 32 x 1 image (BASELINE.json configs[1])",
                                "model_tflops_per_gpu": r1["step_gflop_per_gpu"] * 1e-3 / (r1["ms_per_step"] * 1e-3), "loss": r1["loss"]}
            del single
            torch.cuda.empty_cache()
        except Exception as e:
            out["tf_single"] = {"error": str(e)}
    if world == 1 and not args.no_extras and not args.no_dropin:
        try:
            out["tf_dropin"] = tf_dropin(args, dev, N)
            out["tf_dropin"]["vs_fused_step"] = out["tf_dropin"]["ms_per_step"] / ms_per_step
        except Exception as e:
            out["tf_dropin"] = {"error": str(e)}
        torch.cuda.empty_cache()
    if world == 1 and not args.no_extras and not args.no_scst and not args.no_dropin:
        try:
            out["scst_dropin"] = scst_dropin(args, dev)
            if out["scst"].get("ms_per_step"):
                out["scst_dropin"]["vs_fused_step"] = out["scst_dropin"]["ms_per_step"] / out["scst"]["ms_per_step"]
                srt = out["scst"].get("string_round_trip") or {}
                if srt.get("ms_per_step"):      # the like-for-like twin: the fused step WITH the decode -> re-tokenise string round trip the callers do
                    out["scst_dropin"]["vs_fused_string_round_trip_step"] = out["scst_dropin"]["ms_per_step"] / srt["ms_per_step"]
        except Exception as e:
            out["scst_dropin"] = {"error": str(e)}
        torch.cuda.empty_cache()
    if world == 1 and not args.no_extras and not args.no_scst:
        try:
            out["scst_c5"] = scst_bench(args, rank, world, dev, max(3, args.scst_steps // 2), c5=True)
        except Exception as e:
            out["scst_c5"] = {"metric": "scst_steps_per_sec", "value": None, "error": str(e)}
    if world == 1 and not args.no_extras:
        try:
            out["beam_generation"] = beam_bench(args, dev)
        except Exception as e:
            out["beam_generation"] = {"error": str(e)}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(T, V, N)
        except Exception as e:                              # the baseline must never take the GPU number down with it
            out["cpu_baseline"] = {"value": None, "unit": "tokens/s", "cores": torch.get_num_threads(), "kind": "port", "sample": f"failed: {e}"}
    report(out, rank, world)


def report(out, rank, world):
    """Rank 0 prints the ONE JSON line; the process group is torn down."""
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
