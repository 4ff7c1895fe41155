"""Autoregressive generation for the MI355X engines: greedy, top-k sampling and beam search with a KV cache.

Replaces what the reference obtains from transformers' GenerationMixin (TF5 = transformers/generation/utils.py @ 5.15.0:
generate :2260, _sample :2783, _beam_search :3208) together with the reference's own per-step input assembly
`prepare_inputs_for_generation` (modules/transformers/longitudinal_model/modelling_longitudinal.py:251-295 and the
single/multi variants). Behaviour kept: BOS is prepended when no row of the prompt starts with it (:850-907) and the
longitudinal model strips it again before feeding the decoder (:270-271); finished rows keep emitting PAD (:2932);
`generate.__wrapped__` (no torch.no_grad) returns `scores` that carry autograd -- implemented as sample-then-recompute:
the sampled sequence is re-scored by ONE teacher-forced pass whose per-step inputs are exactly those of the cached steps.
"""
from __future__ import annotations

import numbers
from dataclasses import dataclass, fields
from typing import NamedTuple

import numpy as np
import torch

from . import ops


class _Unset:
    """Signature default of the generate() options a `generation_config` object may supply: tells "not passed" from "passed the default"."""

    def __repr__(self):
        return "<unset>"


UNSET = _Unset()

# options of generate() a `generation_config` object may supply, with the engine's defaults (the effective values of a call that passes neither)
GENERATION_DEFAULTS = dict(
    max_length=None, max_new_tokens=None, bos_token_id=None, eos_token_id=None, pad_token_id=None, num_beams=1, do_sample=False, top_k=50, top_p=1.0,
    temperature=1.0, output_scores=False, return_dict_in_generate=False, use_cache=True, length_penalty=1.0, repetition_penalty=1.0,
    no_repeat_ngram_size=0, min_length=0, min_new_tokens=None, num_return_sequences=1, output_logits=False, bad_words_ids=None, suppress_tokens=None,
    begin_suppress_tokens=None, sequence_bias=None, forced_bos_token_id=None, forced_eos_token_id=None, early_stopping=False,
    output_attentions=False, output_hidden_states=False)

# fields of a `generation_config` object this engine cannot honour -> is the value neutral (the field then changes nothing in the library either)?
_UNSUPPORTED_FIELDS = {
    "num_beam_groups": lambda v: v <= 1, "diversity_penalty": lambda v: v == 0.0, "penalty_alpha": lambda v: v == 0.0, "typical_p": lambda v: v >= 1.0,
    "min_p": lambda v: False, "top_h": lambda v: False, "epsilon_cutoff": lambda v: v <= 0.0, "eta_cutoff": lambda v: v <= 0.0,
    "exponential_decay_length_penalty": lambda v: False, "encoder_repetition_penalty": lambda v: v == 1.0,
    "encoder_no_repeat_ngram_size": lambda v: v <= 0, "guidance_scale": lambda v: v == 1.0, "renormalize_logits": lambda v: v is False,
    "remove_invalid_values": lambda v: v is False, "constraints": lambda v: False, "force_words_ids": lambda v: False,
    "dola_layers": lambda v: False, "stop_strings": lambda v: False, "max_time": lambda v: False, "watermarking_config": lambda v: False,
    "prompt_lookup_num_tokens": lambda v: False}


def resolve_generation_options(kwargs, generation_config=None):
    """The effective options of one generate() call (pure host code). kwargs: the options the caller PASSED (an option left out, or given as UNSET,
    was not passed); generation_config: any object with attributes (transformers.GenerationConfig is the intended one), or None. Precedence: a
    keyword the caller passed wins, even when it equals the default; otherwise a non-None field of the object applies; otherwise the engine's
    default (GENERATION_DEFAULTS). A field of the OBJECT this engine cannot honour, set to a non-neutral value, raises NotImplementedError naming
    it (the same names passed as plain keywords stay ignored). -> dict with every key of GENERATION_DEFAULTS."""
    out = {}
    for name, default in GENERATION_DEFAULTS.items():
        if name in kwargs and kwargs[name] is not UNSET:
            out[name] = kwargs[name]
            continue
        field = getattr(generation_config, name, None) if generation_config is not None else None
        out[name] = default if field is None else field
    if generation_config is not None:
        for name, neutral in _UNSUPPORTED_FIELDS.items():
            v = getattr(generation_config, name, None)
            if v is not None and not neutral(v):
                raise NotImplementedError(f"generation_config.{name} = {v!r} is not supported by this engine")
        beams = out["num_beams"]
        if out["do_sample"] and beams is not None and int(beams) > 1:
            raise NotImplementedError("generation_config: do_sample with num_beams > 1 (beam sampling) is not supported by this engine")
        eos = out["eos_token_id"]
        if isinstance(eos, (list, tuple)) and not ("eos_token_id" in kwargs and kwargs["eos_token_id"] is not UNSET):
            if len(eos) != 1:
                raise NotImplementedError(f"generation_config.eos_token_id = {eos!r}: this engine stops on one EOS id")
            out["eos_token_id"] = eos[0]
    return out


def _is_id(t):
    return isinstance(t, (int, np.integer))


def token_constraints(vocab_size, eos_token_id, prompt_len, max_length, sequence_bias=None, bad_words_ids=None, suppress_tokens=None,
                      begin_suppress_tokens=None, forced_bos_token_id=None, forced_eos_token_id=None):
    """Validates the token-constraint options as the library's processors do (TF5 logits_process.py SequenceBiasLogitsProcessor._validate_arguments
    :1351, NoBadWordsLogitsProcessor :1450-1481, same messages) and -> a hashable description of them, or None when none is set:
    (sequence_bias entries ((ids, bias), ...) in the caller's order, bad words (ids, ...) without single [eos] entries, forced_bos id | None,
    forced_eos ids, suppress ids, begin_suppress ids, max_length, begin_index). prompt_len counts the prepended BOS. An id >= vocab_size in
    sequence_bias / bad_words_ids raises the library's ValueError here, before decoding (the library raises it at the first step); a forced id
    outside the vocabulary (an IndexError of the library's first forced step) is a ValueError too."""
    if all(o is None for o in (sequence_bias, bad_words_ids, suppress_tokens, begin_suppress_tokens, forced_bos_token_id, forced_eos_token_id)):
        return None

    def seq_table(table):                                    # the library's dict: a repeated key keeps its first position and its last bias
        if not isinstance(table, dict) and not isinstance(table, list) or len(table) == 0:
            raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {table}.")
        if isinstance(table, dict) and any(not isinstance(k, tuple) for k in table):
            raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {table}.")
        if isinstance(table, dict) and any(any((not _is_id(t) or t < 0) for t in k) or len(k) == 0 for k in table):
            raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {table}.")

        def pair_ok(e):
            return (isinstance(e, (list, tuple)) and len(e) == 2 and isinstance(e[0], list) and len(e[0]) > 0
                    and all(_is_id(t) and t > 0 for t in e[0]) and isinstance(e[1], float))
        if isinstance(table, list) and any(not pair_ok(e) for e in table):
            raise ValueError(f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, but is {table}.")
        if isinstance(table, dict) and any(not isinstance(b, float) for b in table.values()):
            raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {table}.")
        d = dict(table) if isinstance(table, dict) else {tuple(e[0]): e[1] for e in table}
        invalid = [int(t) for k in d for t in k if t >= vocab_size]
        if invalid:
            raise ValueError(f"The model vocabulary size is {vocab_size}, but the following tokens were being biased: {invalid}")
        return tuple((tuple(int(t) for t in k), float(b)) for k, b in d.items())

    bias = seq_table(sequence_bias) if sequence_bias is not None else ()
    bad = ()
    if bad_words_ids is not None:
        if not isinstance(bad_words_ids, list) or len(bad_words_ids) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids}.")
        if any(not isinstance(w, list) for w in bad_words_ids):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bad_words_ids}.")
        if any(any((not _is_id(t) or t < 0) for t in w) for w in bad_words_ids):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad_words_ids}.")
        words = [w for w in bad_words_ids if eos_token_id is None or w != [eos_token_id]]      # TF5 :1454-1464
        bad = tuple(k for k, _ in seq_table({tuple(w): float("-inf") for w in words}))

    def id_list(name, v, one_ok=False):
        if v is None:
            return ()
        if one_ok and _is_id(v):
            v = [v]
        if hasattr(v, "tolist"):
            v = v.tolist()
        if not isinstance(v, (list, tuple)) or any(not _is_id(t) or t < 0 for t in v):
            raise ValueError(f"`{name}` has to be a list of non-negative integers, but is {v}.")
        return tuple(int(t) for t in v)
    feos = id_list("forced_eos_token_id", forced_eos_token_id, one_ok=True)
    fbos = id_list("forced_bos_token_id", forced_bos_token_id, one_ok=True)
    if len(fbos) > 1:
        raise ValueError(f"`forced_bos_token_id` has to be one id, but is {forced_bos_token_id}.")
    out_of_range = [t for t in fbos + feos if t >= vocab_size]
    if out_of_range:
        raise ValueError(f"The model vocabulary size is {vocab_size}, but the following tokens were being forced: {out_of_range}")
    begin_index = prompt_len + (1 if (prompt_len <= 1 and fbos) else 0)                       # TF5 generation/utils.py:1278-1283
    return (bias, bad, fbos[0] if fbos else None, feos, id_list("suppress_tokens", suppress_tokens),
            id_list("begin_suppress_tokens", begin_suppress_tokens), int(max_length), int(begin_index))


def constraint_tables(cons, device):
    return ops.ConstraintTables(device, *cons)               # token_constraints() describes them in the order of the tables' arguments


class Controls(NamedTuple):
    """The generation controls of one call: repetition penalty (1.0: none), n-gram size (0: none), absolute minimum length (0: none) and the token
    constraints (what token_constraints() returns, or None)."""
    penalty: float = 1.0
    ngram: int = 0
    min_abs: int = 0
    cons: tuple | None = None

    @property
    def active(self):                                        # does a step launch the processors at all?
        return self.penalty != 1.0 or self.ngram > 0 or self.min_abs > 0 or self.cons is not None

    @property
    def constrained(self):                                   # ... and is it the constraint kernel, over the constraints' device tables?
        return self.cons is not None


RECORDED = ("scores", "logits")                                # the per-step outputs, in the order TF5's generate outputs list them
MAP_FIELDS = ("decoder_attentions", "cross_attentions", "decoder_hidden_states")      # ... and the per-step, per-layer ones that follow them


class Record(NamedTuple):
    """The per-step outputs a call asks for (output_logits / output_scores, output_attentions / output_hidden_states): which of them, and the
    number of row groups of the study-major permutation they are stored under (decode row g * (rows // row_groups) + study -> output row
    study * row_groups + g)."""
    logits: bool = False
    scores: bool = False
    row_groups: int = 1
    attentions: bool = False
    hidden: bool = False

    @property
    def on(self):
        return self.logits or self.scores

    @property
    def maps(self):                                          # attention maps / hidden states: extra launches inside the decoder step
        return self.attentions or self.hidden

    @property
    def any(self):
        return self.on or self.maps


def _plain(v):
    return v is None or isinstance(v, (str, numbers.Number)) or (isinstance(v, tuple) and all(_plain(e) for e in v))


@dataclass(frozen=True)
class StepPlan:
    """Everything the decode steps of one generate() call depend on besides their column: built once per call, handed to every DecodeSession.step,
    and -- being compared and hashed by VALUE -- the options' part of the key a captured step graph is stored under. Equal options give equal
    plans (the graphs are replayed), any different option an unequal one (never a graph captured for other options). Every field holds None,
    numbers, strings or tuples of them: a list, tensor, dict or function (unhashable, or compared by identity) is refused at construction."""
    kind: str                                  # "greedy" | "sample" | "pair" (first half of the rows sampled, second half argmax) | "beam"
    special: tuple                             # separator ids of the token types; "pair": (ids of the sampled half, ids of the greedy half)
    mask_token_id: int | None
    bos: int
    eos: int | None
    pad: int | None
    max_length: int
    train: bool                                # dropout on (model.training)
    controls: Controls = Controls()
    record: Record = Record()
    top_k: int = 0                             # "sample" / "pair": the warpers of the sampled rows
    temperature: float = 1.0
    top_p: float = 1.0
    num_beams: int = 1                         # "beam" (the other kinds leave these four alone: their graphs serve every prompt length)
    length_penalty: float = 1.0
    prompt_len: int = 0                        # columns before the first generated one, the prepended BOS included
    early_stopping: int = 0                    # early_stopping_mode(): 0 False, 1 True, 2 "never"

    def __post_init__(self):
        bad = [f.name for f in fields(self) if not _plain(getattr(self, f.name))]
        if bad:
            raise TypeError(f"StepPlan fields {bad}: a plan holds None, numbers, strings and tuples of them only")


def process_scores_(scores, ids, cur, eos, controls, tables=None):
    """The processors of one step, one launch: the three controls alone -> cxr_logits_process_f32; with token constraints ->
    cxr_logits_constrain_f32 over the constraints' device tables."""
    if controls.constrained:
        return ops.logits_constrain_(scores, ids, cur, eos, controls.penalty, controls.ngram, controls.min_abs, tables=tables)
    return ops.logits_process_(scores, ids, cur, eos, controls.penalty, controls.ngram, controls.min_abs)


def score_step_(logits, ids, cur, plan, lo, so, tables=None):
    """The per-step outputs and the processors of one step in TF5's order, in place on the fp32 rows `logits`: raw logits -> lo, [beam: log_softmax,]
    the processors over the history ids[:, :cur], processed scores -> so (lo / so: output slots or None; csrc/gen_record.hip stores them
    study-major). Without processors one launch records both (or nothing is launched) and a beam search takes its log_softmax in the launch
    that follows (ops.beam_step / log_softmax_rows_(add_row=)); with them the beam path processes log-probs (TF5 utils.py:3388-3389)."""
    beam, nb = plan.kind == "beam", plan.record.row_groups
    if not plan.controls.active:
        if lo is not None or so is not None:
            ops.gen_record(logits, lo, so, log_softmax=beam, nb=nb)
        return
    if lo is not None:
        ops.gen_record(logits, lo, nb=nb)
    if beam:
        ops.log_softmax_rows_(logits)
    process_scores_(logits, ids, cur, -1 if plan.eos is None else plan.eos, plan.controls, tables)
    if so is not None:
        ops.gen_record(logits, None, so, nb=nb)


def trim_at_eos(sequences, prompt_len, eos):
    """HF stops at the step on which the last row finishes: -> sequences up to the first EOS of the longest row (one host read)."""
    if eos is None:
        return sequences
    is_eos = sequences[:, prompt_len:] == eos
    lens = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, torch.full((sequences.shape[0],), is_eos.shape[1], device=sequences.device))
    return sequences[:, : prompt_len + int(lens.max())]


def early_stopping_mode(early_stopping, length_penalty):
    """early_stopping of generate() -> 0 (False), 1 (True), 2 ("never" with a positive length penalty: the only case in which "never" differs
    from False, TF5 generation/utils.py:3044-3048). Anything else raises the library's ValueError (configuration_utils.py:667)."""
    if early_stopping is None or early_stopping is False:
        return 0
    if early_stopping is True:
        return 1
    if isinstance(early_stopping, str) and early_stopping == "never":
        return 2 if float(length_penalty) > 0.0 else 0
    raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {early_stopping}.")


class DecodeSession:
    """Static state of one cached greedy / sampling decode (fixed batch, encoder length, maximum length) plus the hipGraphs of
    its single-token steps. A decode step is ~90 short kernels; launched eagerly it is bound by the host (~9 us per launch through
    Python/ctypes), so every step index is captured ONCE into a graph -- all buffers the kernels touch (token ids, masks, KV cache,
    logits, next-token word) are static, and the position-dependent scalars (cache row, attention length) are baked per step -- and
    replayed afterwards. Sessions are cached on the model and reused by every later generate() call of the same geometry (each SCST
    step decodes twice with identical shapes)."""

    def __init__(self, model, B, S, Lmax, has_mask, share=1):
        dev = model.device
        self.model, self.B, self.S, self.Lmax = model, B, S, Lmax
        D = model.config.decoder.hidden_size
        rows, B = B, B // share          # `share` decodes of the same studies (SCST: sample + greedy) read ONE copy of the encoder rows / cross K,V
        self.ids = torch.zeros((rows, Lmax), dtype=torch.int64, device=dev)
        self.unfinished = torch.ones(rows, dtype=torch.int32, device=dev)
        self.nxt = torch.zeros(rows, dtype=torch.int64, device=dev)
        self.enc16 = torch.empty((B, S, D), dtype=torch.bfloat16, device=dev)
        self.enc_mask8 = torch.empty((B, S), dtype=torch.uint8, device=dev) if has_mask else None
        self.enc_bits = torch.zeros((B, (S + 31) // 32), dtype=torch.int32, device=dev) if has_mask else None      # the same mask as bit words (decode kernels)
        self.cache = model._dec.new_cache(rows, Lmax, dev)
        L = model.config.decoder.num_hidden_layers
        if model._dec.cross_kv_fused():
            # cross-attention K / V of ALL layers as the column blocks of one [B, S, 2 L D] buffer: ONE projection GEMM at prefill, and the
            # teacher-forced re-scoring pass of an SCST step reads the same buffer instead of projecting the encoder output again
            self.cache.kv_all = torch.empty((B, S, 2 * L * D), dtype=torch.bfloat16, device=dev)
            self.cache.ck = [self.cache.kv_all[:, :, 2 * l * D:(2 * l + 1) * D] for l in range(L)]
            self.cache.cv = [self.cache.kv_all[:, :, (2 * l + 1) * D:(2 * l + 2) * D] for l in range(L)]
        else:
            self.cache.ck = [torch.empty((B, S, D), dtype=torch.bfloat16, device=dev) for _ in range(L)]
            self.cache.cv = [torch.empty((B, S, D), dtype=torch.bfloat16, device=dev) for _ in range(L)]
        if ops.attention_cross_mfma_ok(rows, B, S):             # static fragment-ordered K / V copies (captured by the step graphs)
            self.cache.cpk = [(torch.empty(B * S * D, dtype=torch.bfloat16, device=dev), torch.empty(B * S * D, dtype=torch.bfloat16, device=dev)) for _ in range(L)]
        self.seed = torch.zeros(1, dtype=torch.int32, device=dev)     # dropout seed of the running decode (train mode); graphs read it
        # uniforms of every sampling step of a decode, drawn by ONE torch call in reset(): a torch.rand inside a captured step costs three extra
        # tiny launches per replay (the generator's seed / offset refresh in front of the graph + the fill kernel itself)
        self.u_all = torch.zeros((Lmax, rows), dtype=torch.float32, device=dev)
        self.poll_host = torch.zeros(1, dtype=torch.int32).pin_memory()          # landing pad of the asynchronous stop poll (keep_going)
        self.polled = None                                 # event behind the copy of the last submitted flag
        # per-step inputs of the cached steps (one fused kernel writes them): last token, token type, position, attention mask, and the
        # token-type / position history the teacher-forced re-scoring of the sampled rows needs
        self.new_id = torch.zeros((rows, 1), dtype=torch.int64, device=dev)
        self.tt1 = torch.zeros((rows, 1), dtype=torch.int64, device=dev)
        self.pos1 = torch.zeros((rows, 1), dtype=torch.int64, device=dev)
        self.mask8 = torch.zeros((rows, (Lmax + 7) // 8 * 8), dtype=torch.uint8, device=dev)[:, :Lmax]      # 8-byte aligned rows: one load per lane
        self.tt_hist = torch.zeros((rows, Lmax), dtype=torch.int64, device=dev)
        self.pos_hist = torch.zeros((rows, Lmax), dtype=torch.int64, device=dev)
        self.graphs = {}
        self.pool = None
        self.version = -1
        self.fills = 0                                     # number of reset()s = prefills: every one overwrites the cross K / V (decoder.SharedCrossKV)
        self.beam = None                                   # device-side beam-search state (beam_state)
        self.rec_bufs = {}                                 # per-step outputs of generate (output_logits / output_scores): [Lmax, rows, V] fp32 each
        self.map_bufs = {}                                 # ... (output_attentions / output_hidden_states): map_buffers
        self.first_maps = None                             # the prefill step's maps / states (fresh tensors: their q_len is the fed prompt's)
        self.cons = {}                                     # token constraints (hashable description) -> their device tables (constraint_tables)
        self._cache_home = (list(self.cache.k), list(self.cache.v), list(self.cache.k2), list(self.cache.v2))

    def constraint_tables(self, cons):
        """Device tables of the token constraints `cons`, owned by the session: step graphs bake their addresses, so a table lives as long as the
        graphs keyed by it (the plan in a step's key carries `cons`). Built outside any capture; a ninth description drops the tables AND the graphs."""
        if cons not in self.cons:
            if len(self.cons) >= 8:
                self.cons.clear()
                self.graphs.clear()
            self.cons[cons] = constraint_tables(cons, self.ids.device)
        return self.cons[cons]

    def beam_state(self, nb, pad, bidx=False, allfin=False):
        """State of a device-side beam search over this session's rows (BEAM-MAJOR: row = beam * studies + study, so the beams of a study
        share its cross-attention K/V): `self.ids` viewed [nb, B, Lmax] holds the running beams; finished beams, scores and the stop flags
        live here (csrc/decode.hip beam_step_kernel). bidx: also the beam-index histories of the running and finished beams (int32 [nb, B, Lmax],
        -1 = no token chosen), allocated on first use. allfin: also the "finished set is full" flags of early_stopping=True (int32 [2, B])."""
        dev, B = self.ids.device, self.B // nb
        if self.beam is None or self.beam["nb"] != nb:
            self.beam = dict(nb=nb, sequences=torch.zeros((nb, B, self.Lmax), dtype=torch.int64, device=dev),
                             run_scores=torch.zeros((B, nb), dtype=torch.float32, device=dev),
                             beam_scores=torch.zeros((B, nb), dtype=torch.float32, device=dev),
                             finished=torch.zeros((B, nb), dtype=torch.uint8, device=dev),
                             unsat=torch.zeros((2, B), dtype=torch.int32, device=dev), allhit=torch.zeros((2, B), dtype=torch.int32, device=dev),
                             beam_idx=torch.zeros(self.B, dtype=torch.int64, device=dev),
                             ws=ops.beam_ws(self.B, self.model.config.decoder.vocab_size, nb, dev))
        st = self.beam
        st["run_scores"].fill_(-1.0e9); st["run_scores"][:, 0] = 0.0            # only beam 0 of the identical start rows may continue
        st["beam_scores"].fill_(-1.0e9); st["finished"].zero_()
        st["unsat"].fill_(1); st["allhit"].zero_()
        st["sequences"].copy_(self.ids.view(nb, B, self.Lmax))
        if bidx:
            if "run_bidx" not in st:                        # allocated once: graphs that captured them stay valid
                st["run_bidx"] = torch.empty((nb, B, self.Lmax), dtype=torch.int32, device=dev)
                st["fin_bidx"] = torch.empty((nb, B, self.Lmax), dtype=torch.int32, device=dev)
            st["run_bidx"].fill_(-1); st["fin_bidx"].fill_(-1)
        if allfin:
            if "allfin" not in st:
                st["allfin"] = torch.empty((2, B), dtype=torch.int32, device=dev)
            st["allfin"].zero_()
        return st

    def record_buffers(self, record):
        """Static slots of the per-step outputs a call asks for, by name: [Lmax, rows, V] fp32, step column c -> slot c (a step graph bakes its
        slot's address). Allocated on the first call that asks for them and never replaced, so graphs captured over them stay valid; calls
        without the flags neither allocate nor touch them."""
        V = self.model.config.decoder.vocab_size
        for name in RECORDED:
            if getattr(record, name) and name not in self.rec_bufs:
                self.rec_bufs[name] = torch.empty((self.Lmax, self.ids.shape[0], V), dtype=torch.float32, device=self.ids.device)
        return {name: self.rec_bufs[name] for name in RECORDED if getattr(record, name)}

    def map_buffers(self, record):
        """Static slots of the attention maps / hidden states of the single-token steps, step column c -> slot c: "self" fp32
        [Lmax, L, rows, H, Lmax], "cross" [Lmax, L, rows, H, S] (output_attentions), "hidden" [Lmax, L + 1, rows, D] (output_hidden_states).
        Like record_buffers: allocated on the first call that asks, never replaced, untouched by calls that do not ask. Bytes:
        4 * Lmax * rows * (L * H * (Lmax + S) + (L + 1) * D)."""
        cfg, rows, dev = self.model.config.decoder, self.ids.shape[0], self.ids.device
        L, H, D = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.hidden_size
        if record.attentions and "self" not in self.map_bufs:
            self.map_bufs["self"] = torch.zeros((self.Lmax, L, rows, H, self.Lmax), dtype=torch.float32, device=dev)
            self.map_bufs["cross"] = torch.zeros((self.Lmax, L, rows, H, self.S), dtype=torch.float32, device=dev)
        if record.hidden and "hidden" not in self.map_bufs:
            self.map_bufs["hidden"] = torch.zeros((self.Lmax, L + 1, rows, D), dtype=torch.float32, device=dev)
        return {name: self.map_bufs[name] for name in (("self", "cross") if record.attentions else ()) + (("hidden",) if record.hidden else ())}

    def step_record(self, record, cur, prefill):
        """The decoder.StepRecord of step column `cur`: its slots, or (prefill) fresh tensors, kept in first_maps. None without the flags."""
        if not record.maps:
            return None
        from .decoder import StepRecord
        if prefill:
            self.first_maps = StepRecord(record.attentions, record.hidden, row_groups=record.row_groups)
            return self.first_maps
        b = self.map_buffers(record)
        return StepRecord(record.attentions, record.hidden, b["self"][cur] if "self" in b else None, b["cross"][cur] if "cross" in b else None,
                          b["hidden"][cur] if "hidden" in b else None, record.row_groups)

    def records(self, record, first, steps):
        """One copy of the recorded outputs of steps first .. first+steps-1 (the session is reused by the next call): name -> tuple of [rows, V];
        with output_attentions / output_hidden_states also the MAP_FIELDS: per step a tuple over layers, step 0 the prefill's fresh tensors
        ([rows, H, Tp, Tp] / [rows, H, Tp, S] / [rows, Tp, D]), step t [rows, H, 1, Tp + t] / [rows, H, 1, S] / [rows, 1, D]."""
        out = {name: buf[first:first + steps].clone().unbind(0) for name, buf in self.record_buffers(record).items()}
        if record.maps:
            fm, b = self.first_maps, self.map_buffers(record)
            self.first_maps = None
            cp = {name: buf[first + 1:first + steps].clone() for name, buf in b.items()}      # [steps - 1, L (+ 1), rows, ...]
            if record.attentions:
                Tp = fm.self_attn[0].shape[3]
                out["decoder_attentions"] = (tuple(fm.self_attn),) + tuple(tuple(m[:, :, :Tp + t + 1].unsqueeze(2) for m in st.unbind(0))
                                                                           for t, st in enumerate(cp["self"].unbind(0)))
                out["cross_attentions"] = (tuple(fm.cross_attn),) + tuple(tuple(m.unsqueeze(2) for m in st.unbind(0)) for st in cp["cross"].unbind(0))
            if record.hidden:
                out["decoder_hidden_states"] = (tuple(fm.hidden),) + tuple(tuple(h.unsqueeze(1) for h in st.unbind(0)) for st in cp["hidden"].unbind(0))
        return out

    def _swap_caches(self, n=1):
        c = self.cache
        if n % 2:
            c.k, c.k2 = c.k2, c.k
            c.v, c.v2 = c.v2, c.v

    def reset(self, ids0, enc16, enc_mask8, plan):
        m = self.model
        m._dec.prepare()                           # weight-derived buffers (LoRA merge) are refreshed IN PLACE: captured pointers stay valid
        m._dec.refresh_decode_packs()              # ... as are the packed / LayerNorm-folded decode weights the replayed steps stream
        if self.version != m.flat16.data_ptr():    # parameters were re-packed (.to()/.cuda()): every captured pointer is stale
            self.graphs.clear()
            self.version = m.flat16.data_ptr()
        self.ids.fill_(0)
        self.ids[:, : ids0.shape[1]] = ids0
        self.unfinished.fill_(1)
        self.enc16.copy_(enc16)
        if self.enc_mask8 is not None:
            self.enc_mask8.copy_(enc_mask8)
            ops.pack_mask_bits(self.enc_mask8, out=self.enc_bits)
        self.cache.enc_bits = self.enc_bits
        self.cache.len = 0
        self.cache.cross_ready = False
        self.fills += 1
        self.cache.k, self.cache.v, self.cache.k2, self.cache.v2 = (list(t) for t in self._cache_home)      # beam search ping-pongs them
        if m.training:
            self.seed.copy_(m.next_dropout_seed())
        self.u_all.uniform_()                      # torch's CUDA generator: reproducible under torch.manual_seed
        self.polled = None
        # what the steps of `plan` bake the address of, made before the first of them is captured (never from inside a capture)
        self.record_buffers(plan.record)
        self.map_buffers(plan.record)
        if plan.controls.constrained:
            self.constraint_tables(plan.controls.cons)

    def keep_going(self, flag):
        """The stop poll of a decode loop, one poll behind: False when the flag the PREVIOUS call submitted has landed as 0; else flag() (int32 [1]
        on the device, 0 = every row is done) is copied to the pinned word and -> True. The copy is only waited for at the next poll, so the host
        keeps enqueueing steps while the GPU works (a blocking .item() drained the queue 32 times per decode); the caller trims the overshoot."""
        if self.polled is not None:
            self.polled.synchronize()
            if int(self.poll_host[0]) == 0:
                return False
        self.poll_host.copy_(flag(), non_blocking=True)
        self.polled = torch.cuda.Event()
        self.polled.record()
        return True

    def step(self, cur, strip, plan, n=1):
        """Append tokens cur .. cur+n-1 (0-based columns of self.ids; strip: leading columns the decoder is not fed) as the StepPlan `plan`
        describes: plan.kind selects sampling / argmax / beam bookkeeping, plan.controls the processors (the constraints' tables:
        constraint_tables, built before the first step), plan.record the per-step outputs (their slots: record_buffers, likewise). The n cached
        steps are ONE hipGraph, stored under (cur, n, strip, plan) (a replay costs ~9 us of launch overhead whatever it holds: per token at
        n = 1, per 8 tokens at n = 8)."""
        prefill = self.cache.len == 0
        if prefill or not self.model.graph_decode:
            for c in range(cur, cur + n):
                self._run(c, strip, plan, prefill and c == cur)
            return
        key = (cur, n, strip, plan)
        hit = self.graphs.get(key)
        captured = hit is None
        if captured:
            g = torch.cuda.CUDAGraph()
            if self.pool is None:
                self.pool = torch.cuda.graph_pool_handle()
            keep = self.cache.len
            torch.cuda.synchronize()
            with ops.graph_capture(g, pool=self.pool):
                for c in range(cur, cur + n):
                    self._run(c, strip, plan, False)
            self.cache.len = keep                      # capture does not execute: replay below performs the steps
            hit = (g, self.last_tt, self.last_pos)     # the last step's token-type / position outputs live in the session's history buffers
            self.graphs[key] = hit
        g, self.last_tt, self.last_pos = hit
        g.replay()
        if plan.kind == "beam" and not captured:       # the capture pass already walked the ping-pong of the reordered caches
            self._swap_caches(n)
        self.cache.len = cur + n - 1 - strip

    def _run(self, cur, strip, plan, prefill):
        """The launches of one step: decoder -> logits of column `cur`, score_step_ (records, processors), then by plan.kind one selection launch
        (top_k / temperature / top_p on the sampled rows; finished rows emit plan.pad once plan.eos was drawn) or the beam step (num_beams,
        length_penalty, prompt_len, max_length, early_stopping) and the cache reorder. prefill: the whole prompt is fed, by torch ops."""
        m, train, special = self.model, plan.train, plan.special
        eos = -1 if plan.eos is None else plan.eos
        # per-step outputs (csrc/gen_record.hip): raw logits before any processor, scores as TF5 stores them; slot `cur` of the session's buffers
        slots = self.record_buffers(plan.record)
        lo, so = (slots[name][cur] if name in slots else None for name in ("logits", "scores"))
        tables = self.cons[plan.controls.cons] if plan.controls.constrained else None
        extra = self.step_record(plan.record, cur, prefill)       # attention maps / hidden states: launches beside the step's own
        if prefill:
            fed = self.ids[:, strip:cur]
            new, mask, tt, pos = m._step_inputs(fed, special, plan.mask_token_id, prefill=True)
            new, tt, pos = new.contiguous(), tt.contiguous(), None if pos is None else pos.contiguous()
        else:                                                      # one launch: last token, token type, position, mask (+ their history)
            pair = plan.kind == "pair"
            sp0, sp1 = special if pair else (special, special)
            longi = m.kind == "longitudinal"
            step_args = (self.ids, strip, cur, list(sp0), list(sp1), [0, 1, 0, 1] if longi else None, self.B // 2 if pair else self.B,
                         plan.mask_token_id if longi else -1, self.new_id, self.tt1, self.pos1 if longi else None,
                         self.mask8 if longi else None, self.tt_hist, self.pos_hist if longi else None)
            mask = self.mask8[:, :cur - strip] if longi else None
            if (m._dec.fused_step_ok(self.cache, self.B, self.enc16) and len(sp0) <= 4 and len(sp1) <= 4
                    and cur - strip <= min(512, m.config.decoder.max_position_embeddings)):      # (the kernel indexes the position table with cur - strip - 1)
                # ... and the embeddings of the new token in the same launch, written in the decode kernels' activation layout
                ph, _, _ = m._dec._dropout_cfg(train, self.seed)
                x0 = ops.decode_step_embed(*step_args, *m._dec.embed_tables(), drop=(ph, self.seed, 1) if ph else None)
                logits = m._dec.decode_embedded(self.cache, x0, self.B, self.enc_mask8, mask, train=train, seed=self.seed, extra=extra)
                new = None
            else:
                ops.decode_step_inputs(*step_args)
                new, tt = self.new_id, self.tt1
                pos = self.pos1 if longi else None
        if new is not None:
            logits = m._dec.decode(self.cache, new, self.enc16, self.enc_mask8, mask, tt, pos, train=train, seed=self.seed, extra=extra)
        score_step_(logits, self.ids, cur, plan, lo, so, tables)
        if plan.kind == "beam":                                     # one launch: scoring, candidate search, bookkeeping; one more: cache reorder
            nb, es, st, c = plan.num_beams, plan.early_stopping, self.beam, self.cache
            ops.beam_step(logits, self.ids.view(nb, self.B // nb, self.Lmax), st["sequences"], st["run_scores"], st["beam_scores"], st["finished"],
                          st["unsat"], st["allhit"], st["beam_idx"], cur, plan.max_length, eos,
                          float(cur + 1 - plan.prompt_len) ** plan.length_penalty, ws=st["ws"], logprobs=plan.controls.active,
                          bidx=(st["run_bidx"], st["fin_bidx"]) if plan.record.any else None,
                          early=None if not es else (es, float(plan.max_length - plan.prompt_len) ** plan.length_penalty if es == 2 else 0.0,
                                                     st.get("allfin")))
            ops.gather_batch_multi(c.k + c.v, st["beam_idx"], c.len, c.k2 + c.v2)
            self._swap_caches()
            self.last_tt = self.last_pos = None
            return
        unf = self.unfinished if plan.eos is not None else None
        n_smp = {"greedy": 0, "sample": self.B, "pair": self.B // 2}[plan.kind]      # rows [0, n_smp) sample, the rest take the argmax
        col = self.ids[:, cur]                                                  # the selection kernels write straight into the id buffer
        if n_smp:                                                               # one launch for sampled + greedy rows
            ops.select_token(logits, mode=1, temperature=plan.temperature, top_k=plan.top_k, u=self.u_all[cur, :n_smp], unfinished=unf, eos=eos,
                             pad=plan.pad or 0, out=col, top_p=plan.top_p, n_sample=n_smp)
        else:
            ops.select_token(logits, unfinished=unf, eos=eos, pad=plan.pad or 0, out=col)
        if prefill:
            self.last_tt, self.last_pos = tt, pos
        else:                                                      # views of the history columns this step wrote (stable across graph replays)
            self.last_tt = self.tt_hist[:, cur:cur + 1]
            self.last_pos = self.pos_hist[:, cur:cur + 1] if m.kind == "longitudinal" else None


class GenerationMixin:
    graph_decode = True      # replay single-token decode steps from hipGraphs (DecodeSession)
    device_beam_search = True   # beam search with device-side bookkeeping (False: the host-loop restatement `_beam_search`, kept as an A/B check)

    def _session(self, B, S, Lmax, has_mask, share=1):
        cache = self.__dict__.setdefault("_decode_sessions", {})
        key = (B, S, Lmax, has_mask, share)
        if key not in cache:
            if len(cache) >= 4:
                cache.clear()
            cache[key] = DecodeSession(self, B, S, Lmax, has_mask, share)
        return cache[key]

    # ------------------------------------------------------------------------------------------ per-step inputs
    def _fed(self, ids, bos_token_id):
        if self.kind == "longitudinal" and bool(torch.all(ids[:, 0] == bos_token_id)):
            return ids[:, 1:]
        return ids

    def _step_inputs(self, fed, special_token_ids, mask_token_id, prefill):
        """-> (ids_new, attention_mask_full | None, token_type_ids, position_ids | None). `special_token_ids` is a list of ids, or a
        tuple of two such lists: the separator sets of the first and second half of the rows (sample + greedy decoded as one batch)."""
        sections = [0, 1, 0, 1] if self.kind == "longitudinal" else None
        fedc = fed.contiguous()
        if isinstance(special_token_ids, tuple) and special_token_ids and isinstance(special_token_ids[0], (tuple, list)):
            h = fedc.shape[0] // 2
            tt = torch.cat([ops.token_type_ids(fedc[:h], list(special_token_ids[0]), sections, past=not prefill),
                            ops.token_type_ids(fedc[h:], list(special_token_ids[1]), sections, past=not prefill)], dim=0)
        else:
            tt = ops.token_type_ids(fedc, list(special_token_ids), sections, past=not prefill)
        if self.kind == "longitudinal":
            mask, pos = ops.mask_position_ids(fedc, mask_token_id)
            return (fed, mask, tt, pos) if prefill else (fed[:, -1:], mask, tt, pos[:, -1:])
        return (fed, None, tt, None) if prefill else (fed[:, -1:], None, tt, None)

    # ------------------------------------------------------------------------------------------ generate
    def _generate(self, inputs=None, pixel_values=None, encoder_outputs=None, decoder_input_ids=None, input_ids=None,
                  special_token_ids=None, mask_token_id=None, max_length=UNSET, max_new_tokens=UNSET, bos_token_id=UNSET,
                  eos_token_id=UNSET, pad_token_id=UNSET, num_beams=UNSET, do_sample=UNSET, top_k=UNSET, top_p=UNSET, temperature=UNSET,
                  output_scores=UNSET, return_dict_in_generate=UNSET, use_cache=UNSET, length_penalty=UNSET, return_margins=False,
                  forced_tokens=None, record_inputs=False, repetition_penalty=UNSET, no_repeat_ngram_size=UNSET, min_length=UNSET,
                  min_new_tokens=UNSET, num_return_sequences=UNSET, output_logits=UNSET, bad_words_ids=UNSET, suppress_tokens=UNSET,
                  begin_suppress_tokens=UNSET, sequence_bias=UNSET, forced_bos_token_id=UNSET, forced_eos_token_id=UNSET, early_stopping=UNSET,
                  output_attentions=UNSET, output_hidden_states=UNSET, generation_config=None, **unused):
        """Options left at UNSET take the non-None field of `generation_config` (any object with attributes), else the engine's default
        (GENERATION_DEFAULTS, resolve_generation_options). Token constraints (bad_words_ids, suppress_tokens, begin_suppress_tokens, sequence_bias,
        forced_bos_token_id, forced_eos_token_id) follow transformers 5.15.0's processors, in its order, in one launch per step
        (csrc/logits_proc.hip); early_stopping is False, True or "never" (beam search). output_attentions / output_hidden_states (with
        return_dict_in_generate): decoder_attentions, cross_attentions / decoder_hidden_states of every step (MAP_FIELDS), fp32, study-major;
        the encoder returns neither, so encoder_attentions / encoder_hidden_states read None."""
        from .modelling import ModelOutput
        args = locals()
        o = resolve_generation_options({k: args[k] for k in GENERATION_DEFAULTS}, generation_config)
        bos_token_id, eos_token_id, pad_token_id = o["bos_token_id"], o["eos_token_id"], o["pad_token_id"]
        do_sample, output_scores, return_dict_in_generate = o["do_sample"], o["output_scores"], o["return_dict_in_generate"]
        es = early_stopping_mode(o["early_stopping"], 1.0 if o["length_penalty"] is None else o["length_penalty"])
        if inputs is not None and pixel_values is None:
            pixel_values = inputs
        if special_token_ids is None:
            raise ValueError("special_token_ids is required (reference prepare_inputs_for_generation signature)")
        if self.kind == "longitudinal" and mask_token_id is None:
            raise ValueError("mask_token_id is required for the longitudinal model")
        top_k, temperature, top_p = o["top_k"], o["temperature"], 1.0 if o["top_p"] is None else float(o["top_p"])
        n_ret = 1 if o["num_return_sequences"] is None else int(o["num_return_sequences"])
        num_beams = 1 if o["num_beams"] is None else int(o["num_beams"])
        if n_ret > 1 and num_beams == 1 and not do_sample:            # TF5 configuration_utils.py:788-805
            raise ValueError(f"Greedy methods (do_sample != True) without beam search do not support `num_return_sequences` different than 1 "
                             f"(got {n_ret}).")
        if num_beams > 1 and n_ret > num_beams:
            raise ValueError(f"`num_return_sequences` ({n_ret}) has to be smaller or equal to `num_beams` ({num_beams}).")
        penalty = 1.0 if o["repetition_penalty"] is None else float(o["repetition_penalty"])
        if not penalty > 0.0:
            raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {o['repetition_penalty']}")
        ngram = int(o["no_repeat_ngram_size"] or 0)
        if ngram <= 0 or ngram > ops.LOGITS_PROCESS_MAX_HIST:       # TF5 adds the processor for sizes > 0 only; a size above the longest history
            ngram = 0                                                # can never complete an n-gram
        with torch.no_grad():
            if encoder_outputs is None:
                encoder_outputs = self._encode(pixel_values)
        enc, enc_mask = self._encoder_rows(encoder_outputs)
        dev = self.device
        B = enc.shape[0]
        prompt = decoder_input_ids if decoder_input_ids is not None else input_ids
        start = torch.full((B, 1), bos_token_id, dtype=torch.int64, device=dev)
        if prompt is None:
            ids = start
        else:
            prompt = prompt.to(device=dev, dtype=torch.int64)
            ids = torch.cat([start, prompt], dim=-1) if bool((prompt[:, 0] != bos_token_id).all()) else prompt
        prompt_len = ids.shape[1]
        max_length = o["max_length"]
        if o["max_new_tokens"] is not None:
            max_length = prompt_len + o["max_new_tokens"]
        if max_length is None:
            max_length = 20 + prompt_len
        # generation controls (TF5 logits processors): min_new_tokens takes precedence over min_length as an absolute length (TF5:gen:1760);
        # EOS bans only while the history is shorter than it, so a minimum the prompt already reaches launches nothing
        min_abs = (prompt_len + int(o["min_new_tokens"])) if o["min_new_tokens"] is not None else int(o["min_length"] or 0)
        min_abs = min_abs if (eos_token_id is not None and min_abs > prompt_len) else 0
        # token constraints (TF5 logits processors, validated as the library validates them): with any of them set, ONE launch of the constraint
        # kernel applies them and the three controls above; with none, the launch (or no launch) of before
        cons = token_constraints(self.config.decoder.vocab_size, eos_token_id, prompt_len, max_length, o["sequence_bias"], o["bad_words_ids"],
                                 o["suppress_tokens"], o["begin_suppress_tokens"], o["forced_bos_token_id"], o["forced_eos_token_id"])
        controls = Controls(penalty, ngram, min_abs, cons)
        if controls.active and max_length - 1 > ops.LOGITS_PROCESS_MAX_HIST:      # refused before decoding, not at the step that gets there
            raise ValueError(f"repetition_penalty / no_repeat_ngram_size / min_length / min_new_tokens and the token constraints take histories of "
                             f"at most {ops.LOGITS_PROCESS_MAX_HIST} ids: max_length {max_length} is too long")
        if controls.active and do_sample and output_scores:
            raise NotImplementedError("repetition_penalty / no_repeat_ngram_size / min_length / min_new_tokens / token constraints together with "
                                      "do_sample=True and output_scores=True are not supported: the differentiable scores are not processed")
        enc16, enc_mask8 = self._decoder_feed(enc, enc_mask)
        # per-step outputs (TF5 GenerateOutput fields): recorded only when the dict output asks for them
        want_logits = bool(o["output_logits"]) and bool(return_dict_in_generate)
        want_scores = bool(output_scores) and bool(return_dict_in_generate)
        want_attn = bool(o["output_attentions"]) and bool(return_dict_in_generate)
        want_hidden = bool(o["output_hidden_states"]) and bool(return_dict_in_generate)
        common = dict(special=tuple(special_token_ids), mask_token_id=mask_token_id, bos=bos_token_id, eos=eos_token_id, max_length=int(max_length),
                      train=bool(self.training), controls=controls)
        rec_out = {}
        if num_beams > 1:
            if do_sample:
                raise NotImplementedError("beam sampling is not used by the reference")
            # device-side search: beam counts with a shared-K/V attention kernel, and a cache the one-launch reorder can address (16 tensors = 8 layers)
            on_device = self.device_beam_search and num_beams in (2, 4) and 2 * self.config.decoder.num_hidden_layers <= 16
            # (the device search decodes beam-major rows, stored study-major over num_beams row groups; the host loop's rows are study-major already)
            plan = StepPlan(kind="beam", **common, pad=0 if pad_token_id is None else pad_token_id,
                            record=Record(want_logits, want_scores, num_beams if on_device else 1, want_attn, want_hidden), num_beams=num_beams,
                            length_penalty=float(o["length_penalty"]), prompt_len=prompt_len, early_stopping=es)
            with torch.no_grad():
                seqs, seq_scores = (self._beam_search_session if on_device else self._beam_search)(ids, enc16, enc_mask8, plan, n_ret, rec_out)
            if return_dict_in_generate:         # TF5 GenerateBeamEncoderDecoderOutput field order: rec_out holds scores, logits, beam_indices
                maps = {k: rec_out.pop(k) for k in MAP_FIELDS if k in rec_out}                # ... and the maps / states, which follow them
                return ModelOutput(sequences=seqs, sequences_scores=seq_scores if output_scores else None, **rec_out, **maps)
            return seqs

        rec, keep_inputs = {"tt": [], "pos": []}, (output_scores and do_sample) or record_inputs
        margins = []
        # greedy scores and every call's logits are recorded per step: never served by / decoded along the SCST speculative greedy pass
        record = Record(want_logits, want_scores and not do_sample, n_ret, want_attn, want_hidden)
        warpers = dict(top_k=int(top_k or 0), temperature=float(temperature), top_p=top_p) if do_sample else {}
        plan = StepPlan(kind="sample" if do_sample else "greedy", **common, pad=pad_token_id, record=record, **warpers)
        plain = forced_tokens is None and not return_margins and not record_inputs and not controls.active and n_ret == 1 and not record.any
        if n_ret > 1:
            # sampling of n sequences per study: B * n rows, sample-major (row j * B + b) over ONE copy of the encoder rows when the decode
            # kernels can share them (2 or 4 query rows per K/V stream), else over repeated rows; returned study-major (TF5 repeat_interleave)
            ids = ids.repeat(n_ret, 1)
            if n_ret not in (2, 4) or forced_tokens is not None or return_margins:
                enc16 = enc16.repeat(n_ret, 1, 1)
                enc_mask8 = None if enc_mask8 is None else enc_mask8.repeat(n_ret, 1)
        # ---- the SCST caller's pair of decodes (reference scst/gt_prompt.py:162-180 then :94-112): a sampling call with scores, followed by a
        # greedy call over the SAME encoder outputs and prompt. A cached decode step costs the same for 16 and for 32 rows (it streams the
        # decoder weights), so the sampling call decodes the greedy rows too -- with the arguments the greedy call of the PREVIOUS step used --
        # and the greedy call that follows, if it asks for exactly that, gets the finished rows (`speculative_baseline = False` switches it off).
        # the speculative result is tied to the very tensor OBJECTS of the sampling call (held alive here, so the allocator cannot hand their
        # addresses to another batch), their in-place version counters, and the weights' state: FusedAdamW moves shadow_version, torch.optim's
        # in-place updates move the version counter the parameter views share with the flat master buffer
        spec_objs = (enc, prompt, enc_mask)
        spec_ver = (enc._version, None if prompt is None else prompt._version, None if enc_mask is None else enc_mask._version,
                    getattr(self, "shadow_version", 0), self.flat32._version, bool(self.training))
        if plain and not do_sample and prompt is not None:
            want = (tuple(special_token_ids), mask_token_id, int(max_length), bos_token_id, eos_token_id, pad_token_id)
            hit = getattr(self, "_spec_result", None)
            self._spec_result = None
            self._spec_pattern = want                            # what the next sampling call may decode along
            if (hit is not None and all(a is b for a, b in zip(hit[0], spec_objs)) and hit[3] == spec_ver and hit[1] == want
                    and getattr(self, "speculative_baseline", True)):
                return ModelOutput(sequences=hit[2], scores=None) if return_dict_in_generate else hit[2]
        pattern = getattr(self, "_spec_pattern", None)
        if (plain and do_sample and output_scores and prompt is not None and pattern is not None and getattr(self, "speculative_baseline", True)
                and pattern[2] == int(max_length) and pattern[1] == mask_token_id and pattern[3:] == (bos_token_id, eos_token_id, pad_token_id)):
            with torch.no_grad():
                ids, base, rec = self.sample_and_greedy(encoder_outputs, prompt, list(special_token_ids), list(pattern[0]), mask_token_id, int(max_length),
                                                        bos_token_id, eos_token_id, pad_token_id, top_k=top_k, temperature=temperature, top_p=top_p)
            self._spec_result = (spec_objs, pattern, base, spec_ver)
        elif forced_tokens is None and not return_margins:
            ids = self._generate_session(ids, enc16, enc_mask8, plan, rec if keep_inputs else None, rec_out)
        else:
            ids, margins = self._generate_eager(ids, enc16, enc_mask8, plan, forced_tokens, rec if keep_inputs else None, rec_out)
        order = None
        if n_ret > 1:
            # the decode's rows are sample-major (row j * B + b); the re-scoring pass runs over the SAME rows in the same order -- dropout masks are
            # keyed by row, so each sampled token is scored by the forward that drew it -- over repeated encoder rows (gradient reaches enc); its
            # scores, the sequences and the recorded inputs are then put study-major (TF5 repeat_interleave)
            Bs = ids.shape[0] // n_ret
            order = torch.arange(ids.shape[0], device=ids.device).view(n_ret, Bs).t().reshape(-1)
            enc = enc.repeat(n_ret, *([1] * (enc.dim() - 1)))
            enc_mask = None if enc_mask is None else enc_mask.repeat(n_ret, *([1] * (enc_mask.dim() - 1)))

        scores = rec_out.get("scores")
        if output_scores and do_sample:
            scores = self._rescore_sampled(ids, prompt_len, rec, enc, enc_mask, special_token_ids, mask_token_id, bos_token_id,
                                           top_k, temperature, top_p, order=order)
        if order is not None:
            ids = ids[order]
            rec = {k: ([None if t is None else t[order] for t in v] if k in ("tt", "pos") else v) for k, v in rec.items()}
        if return_dict_in_generate:
            out = ModelOutput(sequences=ids, scores=scores)
            if want_logits:
                out["logits"] = rec_out["logits"]
            if record_inputs:
                out["recorded_inputs"] = rec
            if margins:
                out["greedy_tokens"] = torch.stack([m[0] for m in margins], 1)
                out["greedy_margins"] = torch.stack([m[1] for m in margins], 1)
            for k in MAP_FIELDS:                            # TF5 GenerateEncoderDecoderOutput order among themselves, keys only when asked for
                if k in rec_out:
                    out[k] = rec_out[k]
            return out
        return ids

    def _generate_eager(self, ids, enc16, enc_mask8, plan, forced_tokens, rec=None, rec_out=None):
        """Eagerly launched greedy loop with per-step argmax / margin capture and optional teacher forcing (parity tests). rec: the per-step
        token-type / position inputs are recorded as _generate_session records them (a sampling call with forced_tokens then returns the processed
        scores of the FORCED ids: the reference's sampled sequence can be pushed through the grad-enabled generate body). plan.record / rec_out:
        the per-step logits / processed scores, as _generate_session records them."""
        dev = self.device
        B = ids.shape[0]
        eos, pad, max_length = plan.eos, plan.pad, plan.max_length
        margins = []
        got = {name: [] for name in RECORDED if getattr(plan.record, name)}
        kept = self._kept_maps(plan.record)
        tables = constraint_tables(plan.controls.cons, dev) if plan.controls.constrained else None
        with torch.no_grad():
            cache = self._dec.new_cache(B, max_length, dev)
            unfinished = torch.ones(B, dtype=torch.int32, device=dev)
            step = 0
            seed = self.next_dropout_seed() if self.training else None
            while ids.shape[1] < max_length:
                fed = self._fed(ids, plan.bos)
                new, mask, tt, pos = self._step_inputs(fed, plan.special, plan.mask_token_id, prefill=cache.len == 0)
                if rec is not None:
                    rec["tt"].append(tt.clone())
                    rec["pos"].append(None if pos is None else pos.clone())
                    rec["seed"] = seed
                extra = self._step_record_kept(plan.record)
                logits = self._dec.decode(cache, new.contiguous(), enc16, enc_mask8, mask, tt.contiguous(), None if pos is None else pos.contiguous(),
                                          seed=seed, extra=extra)
                self._keep_maps(kept, extra)
                self._score_step_kept(logits, ids, ids.shape[1], plan, tables, got)      # the whole running history (BOS, prompt, generated)
                if forced_tokens is not None:
                    greedy_tok, mg = ops.select_token(logits, need_margin=True)
                    margins.append((greedy_tok, mg))
                    nxt = forced_tokens[:, step].to(dev).clone()
                    if eos is not None:
                        nxt = torch.where(unfinished.bool(), nxt, torch.full_like(nxt, pad))
                        unfinished = unfinished & (nxt != eos).int()
                else:
                    nxt, mg = ops.select_token(logits, unfinished=unfinished if eos is not None else None, eos=eos if eos is not None else -1,
                                               pad=pad or 0, need_margin=True)
                    margins.append((nxt.clone(), mg))
                ids = torch.cat([ids, nxt[:, None]], dim=-1)
                step += 1
                if forced_tokens is not None and step >= forced_tokens.shape[1]:
                    break
                if eos is not None and forced_tokens is None and int(unfinished.max()) == 0:
                    break
        rec_out.update({name: tuple(k_) for name, k_ in got.items()})
        rec_out.update({name: tuple(k_) for name, k_ in kept.items()})
        return ids, margins

    # the maps / states of a loop without static buffers (_generate_eager, _beam_search): every step's StepRecord returns fresh tensors
    @staticmethod
    def _kept_maps(record):
        return {name: [] for name in ((MAP_FIELDS[:2] if record.attentions else ()) + (MAP_FIELDS[2:] if record.hidden else ()))}

    @staticmethod
    def _step_record_kept(record):
        if not record.maps:
            return None
        from .decoder import StepRecord
        return StepRecord(record.attentions, record.hidden, row_groups=record.row_groups)

    @staticmethod
    def _keep_maps(kept, extra):
        for name, got in (("decoder_attentions", "self_attn"), ("cross_attentions", "cross_attn"), ("decoder_hidden_states", "hidden")):
            if name in kept:
                kept[name].append(tuple(getattr(extra, got)))

    @staticmethod
    def _score_step_kept(logits, ids, cur, plan, tables, got):
        """score_step_ of a loop without static buffers (_generate_eager, _beam_search): each output `got` has a list for goes to a fresh tensor."""
        slots = {name: torch.empty(logits.shape, dtype=torch.float32, device=logits.device) for name in got}
        score_step_(logits, ids, cur, plan, slots.get("logits"), slots.get("scores"), tables)
        for name, t in slots.items():
            got[name].append(t)

    def _generate_session(self, ids, enc16, enc_mask8, plan, rec=None, rec_out=None):
        """Greedy / top-k sampling / the SCST pair over a DecodeSession (static buffers, graph-replayed steps, EOS polled every 8 steps).
        plan.record: the per-step raw logits / processed scores are recorded into the session's slots, rows put study-major over its row groups,
        and handed out in rec_out as one tuple of [rows, V] tensors per returned step."""
        B, prompt_len = ids.shape
        max_length, eos = plan.max_length, plan.eos
        strip = 1 if (self.kind == "longitudinal" and bool(torch.all(ids[:, 0] == plan.bos))) else 0
        with torch.no_grad():
            ses = self._session(B, enc16.shape[1], max_length, enc_mask8 is not None, share=B // enc16.shape[0])
            ses.reset(ids, enc16, enc_mask8, plan)
            if rec is not None:
                rec["seed"] = ses.seed.clone() if self.training else None
                # the session's cross-attention K / V of every layer (valid until the session's next decode) and the weight version they belong to
                rec["cross_kv"] = None if ses.cache.kv_all is None else (ses.cache.kv_all, tuple(ses.enc16.shape), self._weights_stamp(), ses, ses.fills)
            cur = prompt_len
            first_tt = first_pos = None
            while cur < max_length:
                # the prefill step alone, then chunks of up to 8 cached steps per graph replay, aligned to the EOS polling period
                n = 1 if cur == prompt_len else min(8 - (cur - prompt_len) % 8, max_length - cur)
                ses.step(cur, strip, plan, n)
                if rec is not None and cur == prompt_len:            # the prefill step's inputs cover the whole prompt
                    first_tt, first_pos = ses.last_tt.clone(), None if ses.last_pos is None else ses.last_pos.clone()
                cur += n
                # "any row unfinished?" every 8 steps; the overshoot is trimmed below
                if eos is not None and (cur - prompt_len) % 8 == 0 and not ses.keep_going(lambda: ses.unfinished.max().reshape(1)):
                    break
            out = ses.ids[:, :cur].clone()
            if rec is not None:
                # cached steps appended their token type / position to the session's history columns: ONE copy, then per-step views
                # (the session is reused by the next generate() call, so the history must not be handed out itself)
                rec["tt"].append(first_tt)
                rec["pos"].append(first_pos)
                if cur > prompt_len + 1:
                    th = ses.tt_hist[:, prompt_len + 1:cur].clone()
                    ph_ = ses.pos_hist[:, prompt_len + 1:cur].clone() if first_pos is not None else None
                    for c in range(th.shape[1]):
                        rec["tt"].append(th[:, c:c + 1])
                        rec["pos"].append(None if ph_ is None else ph_[:, c:c + 1])
            out = trim_at_eos(out, prompt_len, eos)
            rec_out.update(ses.records(plan.record, prompt_len, out.shape[1] - prompt_len))
        return out

    @torch.no_grad()
    def _weights_stamp(self):
        """Changes whenever the decoder weights may have: the bf16 shadow's version (fused AdamW) and the fp32 master's autograd version (torch edits)."""
        return (getattr(self, "shadow_version", 0), self.flat32._version)

    def _session_cross_kv(self, rec, enc, own=False):
        """The cross-attention K / V of all layers a decode session projected at prefill (rec["cross_kv"]), if they still belong to `enc`'s shape and
        to the current weights -- the teacher-forced re-scoring pass of the same SCST step then skips its own projection GEMM. Else None.
        The result is a LOAN of the session's static buffer (decoder.SharedCrossKV): valid until that session's next prefill. own=True hands out a
        private copy instead (one 0.15-ms copy at the benchmark shape instead of a 16-GFLOP projection) -- for the autograd bridge, whose backward runs
        whenever the caller gets to it: the reference's SCST caller decodes its greedy baseline on the same geometry BETWEEN the sampling call and
        loss.backward() (scst/gt_prompt.py:84-132)."""
        ckv = rec.get("cross_kv") if rec else None
        if ckv is None or ckv[1] != tuple(enc.shape) or ckv[2] != self._weights_stamp():
            return None
        from .decoder import SharedCrossKV
        loan = SharedCrossKV(ckv[0], ckv[3], ckv[4])
        if not loan.valid():
            return None                                    # the session has decoded another batch since: project again
        return SharedCrossKV(ckv[0].clone(), None, 0) if own else loan

    def sample_and_greedy(self, encoder_outputs, prompt_ids, special_sample, special_greedy, mask_token_id, max_length, bos_token_id,
                          eos_token_id, pad_token_id, top_k=50, temperature=1.0, top_p=1.0):
        """The two decodes of one SCST step (reference scst/gt_prompt.py:162-180 sample, :94-112 greedy baseline) as ONE batch of 2B
        rows over the same studies: a cached decode step is bound by streaming the decoder weights, so both halves share every weight
        read and every launch. Rows [0,B) are sampled (top-k, temperature) with the separator set `special_sample`, rows [B,2B) take the
        argmax with `special_greedy`; each half sees exactly the per-step inputs its own generate() call would have produced.
        -> (sampled sequences [B,L], greedy sequences [B,L], recorded per-step token-type / position ids of the sampled half)."""
        enc, enc_mask = self._encoder_rows(encoder_outputs)
        dev = self.device
        B = enc.shape[0]
        prompt = prompt_ids.to(device=dev, dtype=torch.int64)
        start = torch.full((B, 1), bos_token_id, dtype=torch.int64, device=dev)
        first = prompt[:, 0].tolist()                                        # (the one host read of this call: the prompt's first column)
        prepend = all(v != bos_token_id for v in first)
        ids = torch.cat([start, prompt], dim=-1) if prepend else prompt
        enc16, enc_mask8 = self._decoder_feed(enc, enc_mask)                 # B rows serve the 2B decode rows
        plan = StepPlan(kind="pair", special=(tuple(special_sample), tuple(special_greedy)), mask_token_id=mask_token_id, bos=bos_token_id,
                        eos=eos_token_id, pad=pad_token_id, max_length=max_length, train=bool(self.training), top_k=int(top_k or 0),
                        temperature=float(temperature), top_p=float(top_p))
        rec = {"tt": [], "pos": []}
        out = self._generate_session(torch.cat([ids, ids], dim=0), enc16, enc_mask8, plan, rec, {})
        rec = {"tt": [t[:B] for t in rec["tt"]], "pos": [None if p_ is None else p_[:B] for p_ in rec["pos"]], "seed": rec.get("seed"),
               "cross_kv": rec.get("cross_kv")}
        # each half ends where ITS last row finished (HF stops per generate() call)
        return trim_at_eos(out[:B], ids.shape[1], eos_token_id), trim_at_eos(out[B:], ids.shape[1], eos_token_id), rec

    def _encoder_rows(self, encoder_outputs):
        """-> (encoder hidden states, their attention mask | None); the single-image model attends to every row."""
        enc_mask = encoder_outputs.get("attention_mask") if isinstance(encoder_outputs, dict) else None
        return encoder_outputs[0], None if self.kind == "single" else enc_mask

    def _decoder_feed(self, enc, enc_mask):
        """-> the decode kernels' views of the encoder output: bf16 rows (detached) and the mask as bytes."""
        enc16 = (enc if enc.dtype == torch.bfloat16 else ops.cast_to_bf16(enc.float().contiguous())).detach().contiguous()
        return enc16, None if enc_mask is None else enc_mask.to(device=self.device, dtype=torch.uint8).contiguous()

    generate = torch.no_grad()(_generate)          # `.generate.__wrapped__` is the grad-enabled body (reference scst/gt_prompt.py:162)

    def compute_transition_scores(self, sequences, scores, beam_indices=None, normalize_logits=False):
        """Score of every generated token (TF5 GenerationMixin.compute_transition_scores, generation/utils.py:1433): -> [rows, steps] with
        out[n, j] = scores[j][beam_indices[n, j], sequences[n, -steps + j]], 0 where beam_indices < 0 (a hypothesis that had ended). Without
        beam_indices row n of every step belongs to sequence n (greedy / sampling). normalize_logits: log_softmax over the vocabulary first.
        steps = the longest history in beam_indices (len(scores) without them); the tokens are the last `steps` columns of `sequences`."""
        stacked = torch.stack(tuple(scores), 0)                                      # [T, R, V]
        T, _, V = stacked.shape
        if normalize_logits:
            stacked = torch.log_softmax(stacked, dim=-1)
        if beam_indices is None:
            beam_indices = torch.arange(stacked.shape[1], device=sequences.device).view(-1, 1).expand(-1, T)
        ended = beam_indices < 0
        steps = int((~ended).sum(-1).max())
        rows = beam_indices[:, :steps].long().masked_fill(ended[:, :steps], 0).to(stacked.device)
        toks = sequences[:, sequences.shape[-1] - steps:].to(stacked.device)
        flat = stacked[:steps].reshape(steps, -1)                                   # [steps, R * V]
        out = flat.gather(1, (rows * V + toks).t()).t()
        return out.masked_fill(ended[:, :steps].to(out.device), 0.0)

    # ------------------------------------------------------------------------------------------ differentiable scores
    def _rescore_sampled(self, ids, prompt_len, rec, enc, enc_mask, special_token_ids, mask_token_id, bos_token_id, top_k, temperature, top_p=1.0,
                         order=None):
        """Processed scores of every sampling step, [B,V] each, with autograd through the decoder (and encoder_outputs). ids, rec and enc are in the
        decode's row order; order: the row permutation of the returned scores (num_return_sequences: decode order -> study-major)."""
        fed = self._fed(ids, bos_token_id)
        stripped = ids.shape[1] - fed.shape[1]
        n_new = ids.shape[1] - prompt_len
        steps = len(rec["tt"])
        n_new = min(n_new, steps)
        tf_in = fed[:, : (prompt_len - stripped) + n_new - 1]
        tt = torch.cat(rec["tt"][:n_new], dim=1)
        pos = torch.cat(rec["pos"][:n_new], dim=1) if rec["pos"][0] is not None else None
        mask = (tf_in != mask_token_id).to(torch.uint8) if self.kind == "longitudinal" else None
        # the LM head runs on the sampled positions only: sc [B, n_new, V] is the (contiguous) output itself, and its gradient goes back as it is --
        # a slice of full-length logits costs a 490-MB zero fill + copy in backward at the benchmark shape
        first = prompt_len - stripped - 1
        sc = self._decode_tf(tf_in, enc, None if self.kind == "single" else enc_mask, mask, tt, pos, seed=rec.get("seed"),
                             cross_kv=self._session_cross_kv(rec, enc, own=True), logit_from=first)
        if temperature is not None and float(temperature) != 1.0:
            sc = sc / float(temperature)
        if top_k or top_p < 1.0:
            with torch.no_grad():                                            # sc is already temperature-scaled: warpers see temperature 1
                flat = sc.detach().reshape(-1, sc.shape[-1]).contiguous()
                thr = ops.topk_threshold(flat, int(top_k or 0), top_p, 1.0).view(sc.shape[0], sc.shape[1], 1)
            # The token that WAS sampled at a step is inside that step's kept set by construction (reference: the scores are the ones it was
            # drawn from). These scores are recomputed by a teacher-forced pass whose logits differ from the cached step's in the last bf16
            # bits, so a token drawn at the very edge of the top-k can fall just below the recomputed threshold (a few per 4080 draws at the
            # benchmark shape). It keeps its score -- a -inf there would turn the caller's REINFORCE loss into inf - inf -- and takes the place of
            # the k-th entry, so the row still has top_k finite entries, as the reference's rows do (same rule as csrc/loss.hip kept_threshold).
            drawn = ids[:, prompt_len: prompt_len + n_new].unsqueeze(-1).clamp(min=0)
            with torch.no_grad():
                below = sc.detach().gather(2, drawn) < thr
                thr = torch.where(below, torch.nextafter(thr, torch.full_like(thr, float("inf"))), thr)
            drop = sc < thr                                                  # TopK (+ TopP) LogitsWarper semantics (ties at the threshold kept)
            drop = drop.scatter(2, drawn, False)
            sc = sc.masked_fill(drop, float("-inf"))
        # one unbind (its backward is ONE stack of the steps' gradients; 255 separate slices each scattered their gradient into a zero tensor of
        # the full [B, T, V] size: 85 ms per SCST step at the benchmark shape). Each step remembers where it came from so that the caller's
        # `torch.stack(scores, dim=-1)` is a view of `sc` again (modelling.BoundaryTensor).
        from .modelling import _as_boundary
        sc = sc.contiguous() if order is None else sc[order]
        return tuple(_as_boundary(s_t, kind="step", base=sc, t=t) for t, s_t in enumerate(sc.unbind(1)))

    # ------------------------------------------------------------------------------------------ beam search
    def _beam_search_session(self, ids, enc16, enc_mask8, plan, n_ret=1, rec_out=None):
        """Beam search (TF5 generation/utils.py:3208-3560, do_sample=False; plan.early_stopping as early_stopping_mode() numbers it) over a
        DecodeSession: beams*B rows decoded by the cached-step kernels (the beams of a study share its cross-attention K/V: ONE copy of the encoder
        rows, as in the SCST sample+greedy batch), the whole per-step bookkeeping in one kernel launch (ops.beam_step), the cache reorder in
        another, the steps replayed from hipGraphs eight at a time, and the stop condition polled asynchronously every 8 steps (the stopped state
        is frozen on the device, so overshoot steps change nothing). The host loop `_beam_search` does the same with ~40 tensor ops and two
        synchronisations per token. Returns the n_ret best finished hypotheses of every study, study-major, and their scores. plan.record:
        rec_out receives the per-step raw logits / processed log-probs (score_step_) of the steps the search ran ([B * nb, V] each, study-major)
        and the beam indices of the returned hypotheses (int32 [B * n_ret, generated length]), as TF5 returns them."""
        B, prompt_len = ids.shape
        nb, max_length, es = plan.num_beams, plan.max_length, plan.early_stopping
        strip = 1 if (self.kind == "longitudinal" and bool(torch.all(ids[:, 0] == plan.bos))) else 0
        with torch.no_grad():
            ses = self._session(B * nb, enc16.shape[1], max_length, enc_mask8 is not None, share=nb)
            ses.reset(ids.repeat(nb, 1), enc16, enc_mask8, plan)
            ses.ids[:, prompt_len:] = plan.pad
            st = ses.beam_state(nb, plan.pad, bidx=plan.record.any, allfin=es == 1)

            def going():                                                # flags of the last executed step (column cur - 1)
                par = (cur - 1) & 1
                flag = (st["unsat"][par].max() > 0) & (st["allhit"][par].min() == 0)
                if es == 1:                                             # early_stopping=True: every study's finished set is full
                    flag = flag & (st["allfin"][par].min() == 0)
                return flag.to(torch.int32).reshape(1)
            cur = prompt_len
            while cur < max_length:
                n = 1 if cur == prompt_len else min(8 - (cur - prompt_len) % 8, max_length - cur)
                ses.step(cur, strip, plan, n)
                cur += n
                if (cur - prompt_len) % 8 == 0 and cur < max_length and not ses.keep_going(going):
                    break
            # the finished set is held best first: [n, B] -> study-major rows
            out = st["sequences"][:n_ret].transpose(0, 1).reshape(B * n_ret, st["sequences"].shape[2]).clone()
            scores = st["beam_scores"][:, :n_ret].reshape(-1).clone()
            if plan.record.any:
                # steps the search ran (later launches are frozen): every running beam has a parent in each of their columns
                steps = int((st["run_bidx"][0, 0, prompt_len:] >= 0).sum())
                rec_out.update(ses.records(plan.record, prompt_len, steps))
                bidx = st["fin_bidx"][:n_ret].transpose(0, 1).reshape(B * n_ret, -1)[:, prompt_len:]
                rec_out["beam_indices"] = self._trim_beam_indices(bidx)
        return trim_at_eos(out, prompt_len, plan.eos), scores

    @staticmethod
    def _trim_beam_indices(bidx):
        """TF5:gen:3517-3523: the history columns up to the longest returned hypothesis."""
        return bidx[:, :int((bidx >= 0).sum(1).max())].clone()

    def _beam_search(self, ids, enc16, enc_mask8, plan, n_ret=1, rec_out=None):
        """TF5 generation/utils.py:3208-3560 with do_sample=False, one EOS id, early_stopping False / True / "never" (plan.early_stopping = 0 / 1 / 2,
        early_stopping_mode()); the n_ret best hypotheses per study.
        plan.record / rec_out as in _beam_search_session (one row group: the rows are study-major), the beam-index histories kept by torch ops."""
        dev = ids.device
        B = ids.shape[0]
        nb, keep = plan.num_beams, 2 * plan.num_beams
        eos, pad, max_length, es, length_penalty, record = plan.eos, plan.pad, plan.max_length, plan.early_stopping, plan.length_penalty, plan.record.any
        V = self.config.decoder.vocab_size
        ids = ids.repeat_interleave(nb, dim=0)
        enc16 = enc16.repeat_interleave(nb, dim=0).contiguous()
        enc_mask8 = None if enc_mask8 is None else enc_mask8.repeat_interleave(nb, dim=0).contiguous()
        cur = prompt_len = ids.shape[1]
        running = torch.full((B, nb, max_length), pad, dtype=torch.int64, device=dev)
        running[:, :, :cur] = ids.view(B, nb, cur)
        sequences = running.clone()
        run_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
        run_scores[:, 1:] = -1e9
        beam_scores = torch.full((B, nb), -1e9, dtype=torch.float32, device=dev)
        finished = torch.zeros((B, nb), dtype=torch.bool, device=dev)
        unsat = torch.ones((B, 1), dtype=torch.bool, device=dev)
        top_mask = torch.arange(keep, device=dev) < nb
        batch_off = (torch.arange(B, device=dev) * nb).view(B, 1)
        cache = self._dec.new_cache(B * nb, max_length, dev)
        seed = self.next_dropout_seed() if self.training else None
        tables = constraint_tables(plan.controls.cons, dev) if plan.controls.constrained else None
        got = {name: [] for name in RECORDED if getattr(plan.record, name)}
        kept = self._kept_maps(plan.record)
        if record:                                                 # beam-index histories (TF5:gen:3348-3351), absolute token columns
            run_bidx = torch.full((B, nb, max_length), -1, dtype=torch.int32, device=dev)
            fin_bidx = run_bidx.clone()

        def gather(t, idx):
            while idx.dim() < t.dim():
                idx = idx.unsqueeze(-1)
            return torch.gather(t, 1, idx.expand(-1, -1, *t.shape[2:]))

        while True:
            flat = running[:, :, :cur].reshape(B * nb, cur)
            fed = self._fed(flat, plan.bos)
            new, mask, tt, pos = self._step_inputs(fed, plan.special, plan.mask_token_id, prefill=cache.len == 0)
            extra = self._step_record_kept(plan.record)
            logits = self._dec.decode(cache, new.contiguous(), enc16, enc_mask8, mask, tt.contiguous(), None if pos is None else pos.contiguous(),
                                      seed=seed, extra=extra)
            self._keep_maps(kept, extra)
            self._score_step_kept(logits, flat.contiguous(), cur, plan, tables, got)
            if plan.controls.active:                                                          # processed log-probs (TF5:gen:3388-3389) + running beam score
                logits.add_(run_scores.view(-1, 1))
            else:
                ops.log_softmax_rows_(logits, add_row=run_scores.view(-1).contiguous())          # log_softmax + running beam score
            topk_lp, topk_idx = ops.topk_rows(logits.view(B, nb * V), keep)
            beam_of = topk_idx // V
            topk_seq = gather(running, beam_of)
            topk_seq[:, :, cur] = topk_idx % V
            hits = (topk_seq[:, :, cur] == (-1 if eos is None else eos)) | (cur + 1 >= max_length)
            run_lp = topk_lp + hits.float() * -1.0e9
            nxt = torch.topk(run_lp, k=nb)[1]
            running, run_scores = gather(topk_seq, nxt), gather(run_lp, nxt)
            beam_idx = (gather(beam_of, nxt) + batch_off).view(-1)
            if record:                                              # TF5:gen:3116-3127, :3150
                topk_bidx = gather(run_bidx, beam_of)
                topk_bidx[:, :, cur] = (beam_of + batch_off).to(torch.int32)
                run_bidx = gather(topk_bidx, nxt)
            just = hits & top_mask[None, :]
            fin_lp = topk_lp / ((cur + 1 - prompt_len) ** length_penalty)
            if es == 1:                                             # a full finished set takes no more hypotheses (TF5:gen:3184-3185)
                fin_lp = fin_lp + finished.all(dim=1, keepdim=True).float() * -1.0e9
            fin_lp = fin_lp + (~unsat).float() * -1.0e9 + (~just).float() * -1.0e9
            m_seq = torch.cat((sequences, topk_seq), dim=1)
            m_sc = torch.cat((beam_scores, fin_lp), dim=1)
            m_fin = torch.cat((finished, just), dim=1)
            best = torch.topk(m_sc, k=nb)[1]
            sequences, beam_scores, finished = gather(m_seq, best), gather(m_sc, best), gather(m_fin, best)
            if record:                                              # TF5:gen:3197-3202
                fin_bidx = gather(torch.cat((fin_bidx, topk_bidx), dim=1), best)
            cache.reorder(beam_idx.contiguous())
            cur += 1
            best_run = run_scores[:, :1] / (((max_length if es == 2 else cur) - prompt_len) ** length_penalty)     # TF5:gen:3044-3048
            worst_fin = torch.where(finished, beam_scores.min(dim=1, keepdim=True)[0], torch.full_like(beam_scores, -1.0e9))
            unsat = unsat & torch.any(best_run > worst_fin, dim=-1, keepdim=True)
            if not (bool(unsat.any()) and not (es == 1 and bool(finished.all())) and not bool(hits.all())):     # TF5:gen:3055-3075
                break
        out = sequences[:, 0, :] if n_ret == 1 else sequences[:, :n_ret, :].reshape(B * n_ret, -1)
        sc = beam_scores[:, 0] if n_ret == 1 else beam_scores[:, :n_ret].reshape(-1)
        if record:
            rec_out.update({name: tuple(k_) for name, k_ in got.items()})
            rec_out.update({name: tuple(k_) for name, k_ in kept.items()})
            rec_out["beam_indices"] = self._trim_beam_indices(fin_bidx[:, :n_ret, prompt_len:].reshape(B * n_ret, -1))
        return trim_at_eos(out, prompt_len, eos), sc
