// Generation controls on the decode hot path (TF5 generation/logits_process.py @ 5.15.0): RepetitionPenaltyLogitsProcessor :306,
// NoRepeatNGramLogitsProcessor :1021-1110, MinLengthLogitsProcessor :101 / MinNewTokensLengthLogitsProcessor :164 (the latter folded into an
// absolute min_length by the caller), applied in that order (TF5 generation/utils.py:1174-1235) to fp32 score rows in place. The history of
// row r is ids[r, 0 .. cur): the whole running sequence (BOS, prompt, generated tokens). No host reads, no allocation: capturable.
#include "common.h"
#include "../../include/cxrmate_hip.h"

constexpr int LP_THREADS = 256;
constexpr int LP_MAX_HIST = CXR_LOGITS_PROC_MAX_HIST;   // history ids per row (the decoder's position table)
constexpr int LP_PER_THREAD = LP_MAX_HIST / LP_THREADS;

// The three controls as device functions, shared by both kernels below. x: the row's scores, h: its history ids[r, 0 .. cur).
//  (1) repetition penalty: every history id's ORIGINAL score is gathered first (registers), then, after a barrier, the penalised value is
//      scattered back. A history holds duplicates; all of them write the same value, as torch's gather + scatter does. x < 0 ? x * p : x / p,
//      with a true division (bit-exact against the library).
//  (2) n-gram ban: start position s in [0, cur - n] is a complete window of the history; if its first n - 1 ids equal the last n - 1 ids of
//      the history, its last id is banned (-inf). n = 1 bans every id of the history. Nothing is banned while cur < n.
//  (3) min length: eos -> -inf while cur < min_length.
// Every branch is uniform over the workgroup (kernel arguments only), so the barriers inside are reached by all threads or by none.
__device__ __forceinline__ void lp_repetition_penalty(float* __restrict__ x, const long* __restrict__ h, int V, int cur, float penalty, int tid) {
    float v[LP_PER_THREAD];
    long t[LP_PER_THREAD];
#pragma unroll
    for (int j = 0; j < LP_PER_THREAD; ++j) {
        const int i = tid + LP_THREADS * j;
        t[j] = i < cur ? h[i] : -1;
        const bool ok = t[j] >= 0 && t[j] < V;
        v[j] = ok ? x[t[j]] : 0.f;
        if (!ok) t[j] = -1;
    }
    __syncthreads();                                    // every original value is read before any is written
#pragma unroll
    for (int j = 0; j < LP_PER_THREAD; ++j)
        if (t[j] >= 0) x[t[j]] = v[j] < 0.f ? v[j] * penalty : v[j] / penalty;
}

__device__ __forceinline__ void lp_ngram_ban(float* __restrict__ x, const long* __restrict__ h, int V, int cur, int ngram, int tid) {
    const int nwin = cur - ngram + 1, pre = cur - ngram + 1;     // windows; first column of the history's last n - 1 ids
    for (int s = tid; s < nwin; s += LP_THREADS) {
        bool match = true;
        for (int k = 0; k < ngram - 1 && match; ++k) match = h[s + k] == h[pre + k];
        if (match) {
            const long tok = h[s + ngram - 1];
            if (tok >= 0 && tok < V) x[tok] = -INFINITY;
        }
    }
}

__device__ __forceinline__ void lp_min_length(float* __restrict__ x, int V, long eos, int tid) {
    if (tid == 0 && eos >= 0 && eos < V) x[eos] = -INFINITY;
}

// One workgroup per row.
__global__ __launch_bounds__(LP_THREADS) void logits_process_kernel(float* __restrict__ logits, long ld, const long* __restrict__ ids, long ids_ld,
                                                                    int V, int cur, long eos, float penalty, int ngram, int min_length) {
    const int tid = threadIdx.x;
    float* x = logits + (long)blockIdx.x * ld;
    const long* h = ids + (long)blockIdx.x * ids_ld;
    if (penalty != 1.0f) lp_repetition_penalty(x, h, V, cur, penalty, tid);
    if (ngram > 0 && cur >= ngram) {
        __syncthreads();                                    // a ban overrides the penalised value of the same id
        lp_ngram_ban(x, h, V, cur, ngram, tid);
    }
    if (cur < min_length && eos >= 0 && eos < V) {
        __syncthreads();                                    // after a penalised write of the same id (a ban writes -inf too: no order needed)
        lp_min_length(x, V, eos, tid);
    }
}

extern "C" int cxr_logits_process_f32(float* logits, long ld, const long* ids, long ids_ld, long R, int V, int cur, long eos, float penalty,
                                      int ngram, int min_length, hipStream_t stream) {
    if (R <= 0 || V <= 0 || cur < 0 || cur > LP_MAX_HIST || ld < V || ids_ld < cur || ngram < 0 || !(penalty > 0.f) || !logits || !ids)
        return CXR_ERR_ARG;
    if (R > 0x7fffffffL || ngram > LP_MAX_HIST) return CXR_ERR_ARG;
    CXR_LAUNCH(logits_process_kernel, dim3((unsigned)R), dim3(LP_THREADS), 0, stream, logits, ld, ids, ids_ld, V, cur, eos, penalty, ngram,
               min_length);
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Token constraints (TF5 generation/logits_process.py @ 5.15.0: SequenceBiasLogitsProcessor :1211, NoBadWordsLogitsProcessor :1395,
// ForcedBOSTokenLogitsProcessor :1556, ForcedEOSTokenLogitsProcessor :1601, SuppressTokensAtBeginLogitsProcessor :1816,
// SuppressTokensLogitsProcessor :1869) together with the three controls above, in the order of TF5 generation/utils.py:1123-1293:
//   sequence_bias -> repetition_penalty -> no_repeat_ngram -> bad_words -> min_length -> forced_bos -> forced_eos -> suppress -> begin_suppress
// in ONE launch, in place, one workgroup per row.
struct ConstrainArgs {
    float* logits; long ld; const long* ids; long ids_ld;
    int V, cur; long eos; float penalty; int ngram, min_length;
    const long* seq_tok; const int* seq_off; const float* seq_bias;   // entry e = seq_tok[seq_off[e] .. seq_off[e + 1]), bias seq_bias[e]
    int n_bias, n_seq;                                                // entries [0, n_bias): sequence_bias; [n_bias, n_seq): bad words (-inf)
    const long* forced; int n_forced_bos, n_forced_eos, max_length;   // forced[0 .. n_forced_bos) then n_forced_eos ids
    const long* suppress; int n_suppress;
    const long* begin_suppress; int n_begin, begin_index;
};

// Sequence entries [lo, hi), sorted by the host stably by (last id, length > 1): a token's entries are one run, its length-1 entry first, the
// multi-token ones in the caller's order. The thread that owns the FIRST entry of a run walks the run and sums the biases of the entries that
// hit (length 1: always; length k <= cur: the history ends in the entry's first k - 1 ids) in fp32 from 0, as the library accumulates its bias
// row, then adds the sum to the token ONCE. No two threads touch the same token; nothing is written when no entry hits (x + 0 = x).
__device__ __forceinline__ void lp_sequence_entries(float* __restrict__ x, const long* __restrict__ h, int V, int cur, const long* __restrict__ tok,
                                                    const int* __restrict__ off, const float* __restrict__ bias, int lo, int hi, int tid) {
    for (int e = lo + tid; e < hi; e += LP_THREADS) {
        const long last = tok[off[e + 1] - 1];
        if (e > lo && tok[off[e] - 1] == last) continue;             // (off[e] - 1 = last id of entry e - 1): not the head of its run
        if (last < 0 || last >= V) continue;
        float sum = 0.f; bool any = false;
        for (int f = e; f < hi && tok[off[f + 1] - 1] == last; ++f) {
            const int b = off[f], k = off[f + 1] - b;
            bool match = k <= cur || k == 1;
            for (int j = 0; j < k - 1 && match; ++j) match = h[cur - (k - 1) + j] == tok[b + j];
            if (match) { sum += bias[f]; any = true; }
        }
        if (any) x[last] = x[last] + sum;
    }
}

// Listed ids -> -inf (duplicates write the same value; ids outside [0, V) are ignored, as torch.isin over the vocabulary ignores them).
__device__ __forceinline__ void lp_suppress(float* __restrict__ x, int V, const long* __restrict__ list, int n, int tid) {
    for (int i = tid; i < n; i += LP_THREADS) {
        const long t = list[i];
        if (t >= 0 && t < V) x[t] = -INFINITY;
    }
}

// The whole row -> -inf, then (after a barrier) the listed ids -> 0.
__device__ __forceinline__ void lp_force(float* __restrict__ x, int V, const long* __restrict__ list, int n, int tid) {
    for (int i = tid; i < V; i += LP_THREADS) x[i] = -INFINITY;
    __syncthreads();
    for (int i = tid; i < n; i += LP_THREADS) {
        const long t = list[i];
        if (t >= 0 && t < V) x[t] = 0.f;
    }
}

// A barrier stands between every two phases that may touch the same token (a later phase reads or overwrites what an earlier one wrote).
__global__ __launch_bounds__(LP_THREADS) void logits_constrain_kernel(const ConstrainArgs a) {
    const int tid = threadIdx.x, V = a.V, cur = a.cur;
    float* x = a.logits + (long)blockIdx.x * a.ld;
    const long* h = a.ids + (long)blockIdx.x * a.ids_ld;
    if (a.n_bias > 0) {
        lp_sequence_entries(x, h, V, cur, a.seq_tok, a.seq_off, a.seq_bias, 0, a.n_bias, tid);
        __syncthreads();                                    // the penalty acts on the biased score
    }
    if (a.penalty != 1.0f) {
        lp_repetition_penalty(x, h, V, cur, a.penalty, tid);
        __syncthreads();
    }
    if (a.ngram > 0 && cur >= a.ngram) {
        lp_ngram_ban(x, h, V, cur, a.ngram, tid);
        __syncthreads();
    }
    if (a.n_seq > a.n_bias) {
        lp_sequence_entries(x, h, V, cur, a.seq_tok, a.seq_off, a.seq_bias, a.n_bias, a.n_seq, tid);
        __syncthreads();
    }
    if (cur < a.min_length && a.eos >= 0 && a.eos < V) {
        lp_min_length(x, V, a.eos, tid);
        __syncthreads();
    }
    if (a.n_forced_bos > 0 && cur == 1) {                   // a forced row overwrites every earlier ban
        lp_force(x, V, a.forced, a.n_forced_bos, tid);
        __syncthreads();
    }
    if (a.n_forced_eos > 0 && cur == a.max_length - 1) {
        lp_force(x, V, a.forced + a.n_forced_bos, a.n_forced_eos, tid);
        __syncthreads();
    }
    if (a.n_suppress > 0) lp_suppress(x, V, a.suppress, a.n_suppress, tid);          // suppression overrides a forced 0
    if (a.n_begin > 0 && cur == a.begin_index) lp_suppress(x, V, a.begin_suppress, a.n_begin, tid);   // (both write -inf: no order needed)
}

extern "C" int cxr_logits_constrain_f32(float* logits, long ld, const long* ids, long ids_ld, long R, int V, int cur, long eos, float penalty,
                                        int ngram, int min_length, const long* seq_tok, const int* seq_off, const float* seq_bias, int n_bias,
                                        int n_seq, const long* forced, int n_forced_bos, int n_forced_eos, int max_length, const long* suppress,
                                        int n_suppress, const long* begin_suppress, int n_begin, int begin_index, hipStream_t stream) {
    if (R <= 0 || V <= 0 || cur < 0 || cur > LP_MAX_HIST || ld < V || ids_ld < cur || ngram < 0 || !(penalty > 0.f) || !logits || !ids)
        return CXR_ERR_ARG;
    if (R > 0x7fffffffL || ngram > LP_MAX_HIST) return CXR_ERR_ARG;
    if (n_bias < 0 || n_seq < n_bias || (n_seq > 0 && (!seq_tok || !seq_off || !seq_bias))) return CXR_ERR_ARG;
    if (n_forced_bos < 0 || n_forced_bos > 1 || n_forced_eos < 0 || (n_forced_bos + n_forced_eos > 0 && !forced)) return CXR_ERR_ARG;
    if (n_suppress < 0 || (n_suppress > 0 && !suppress) || n_begin < 0 || (n_begin > 0 && !begin_suppress)) return CXR_ERR_ARG;
    const ConstrainArgs a{logits, ld, ids, ids_ld, V, cur, eos, penalty, ngram, min_length, seq_tok, seq_off, seq_bias, n_bias, n_seq, forced,
                          n_forced_bos, n_forced_eos, max_length, suppress, n_suppress, begin_suppress, n_begin, begin_index};
    CXR_LAUNCH(logits_constrain_kernel, dim3((unsigned)R), dim3(LP_THREADS), 0, stream, a);
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}
