// Generation controls on the decode hot path (TF5 generation/logits_process.py @ 5.15.0): RepetitionPenaltyLogitsProcessor :306,
// NoRepeatNGramLogitsProcessor :1021-1110, MinLengthLogitsProcessor :101 / MinNewTokensLengthLogitsProcessor :164 (the latter folded into an
// absolute min_length by the caller), applied in that order (TF5 generation/utils.py:1174-1235) to fp32 score rows in place. The history of
// row r is ids[r, 0 .. cur): the whole running sequence (BOS, prompt, generated tokens). No host reads, no allocation: capturable.
#include "common.h"

constexpr int LP_THREADS = 256;
constexpr int LP_MAX_HIST = 512;          // history ids per row (the decoder's position table)
constexpr int LP_PER_THREAD = LP_MAX_HIST / LP_THREADS;

// One workgroup per row.
//  (1) repetition penalty: every history id's ORIGINAL score is gathered first (registers), then, after a barrier, the penalised value is
//      scattered back. A history holds duplicates; all of them write the same value, as torch's gather + scatter does. x < 0 ? x * p : x / p,
//      with a true division (bit-exact against the library).
//  (2) n-gram ban: start position s in [0, cur - n] is a complete window of the history; if its first n - 1 ids equal the last n - 1 ids of
//      the history, its last id is banned (-inf). n = 1 bans every id of the history. Nothing is banned while cur < n.
//  (3) min length: eos -> -inf while cur < min_length.
__global__ __launch_bounds__(LP_THREADS) void logits_process_kernel(float* __restrict__ logits, long ld, const long* __restrict__ ids, long ids_ld,
                                                                    int V, int cur, long eos, float penalty, int ngram, int min_length) {
    const int tid = threadIdx.x;
    float* x = logits + (long)blockIdx.x * ld;
    const long* h = ids + (long)blockIdx.x * ids_ld;
    if (penalty != 1.0f) {
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
    if (ngram > 0 && cur >= ngram) {
        __syncthreads();                                    // a ban overrides the penalised value of the same id
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
    if (cur < min_length && eos >= 0 && eos < V) {
        __syncthreads();                                    // after a penalised write of the same id (a ban writes -inf too: no order needed)
        if (tid == 0) x[eos] = -INFINITY;
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
