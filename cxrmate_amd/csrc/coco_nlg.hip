// COCO NLG scores (reference tools/metrics/coco.py:106-196 driving the COCO caption toolkit's bleu_scorer / rouge / cider_scorer): per-record BLEU-1..4,
// ROUGE-L and CIDEr-D, their per-study means and the mean over studies, in float64 on integer word ids.
//
// Every distinct text is staged once, as two CSR token streams: `a` holds its str.split() tokens (BLEU, CIDEr), `b` its str.split(" ") tokens
// (ROUGE-L). A scored record is a (hypothesis text, reference text) pair.
//
// N-gram identity is exact. Per order k = 1..4 (the table is cleared and reused):
//   insert  every k-gram of every text goes into a 64-bit open-addressing table (atomicCAS, linear probing, load <= 1/2) under the key
//           (slot of its leading (k-1)-gram) << 32 | last word id; the slot it lands in is the k-gram's id (`gid`). Equal keys <=> equal k-grams,
//           by induction over k, so no two different n-grams ever share an id, whatever the vocabulary.
//   count   one workgroup per text, its ids in LDS: tf[p] = occurrences of the k-gram at p in its text when p is its FIRST occurrence, else 0.
//           First occurrences of a text that is somebody's reference add ref_mult to df[gid] (integer atomicAdd).
//   pair    one workgroup per record, the reference's ids in LDS: for every first occurrence in the hypothesis the reference's count of that
//           k-gram, from which c_k (clipped matches, integer) and CIDEr's val_k and the two norms follow.
// Slots differ from run to run, so no floating-point sum is ordered by slot: every sum runs over positions in the text (thread t adds its
// positions t, t + 256, ... in order, the 256 partial sums fold through LDS in a fixed tree). No floating-point atomics: launches are bit-identical.
//   lcs     one workgroup per record: anti-diagonal wavefront over the `b` streams, three uint16 diagonals in LDS (48 KB).
//   record  one thread per record: BLEU from the integers, ROUGE-L from the LCS, CIDEr = mean_k(val_k) * 10.
//   study / average   mean over the records of each study (in `order`), then one workgroup per column over the studies in a fixed tree.
// A record whose text indices fall outside [0, n_texts) gets NaN scores and -1 integers; a study whose offsets or record indices fall outside
// their arrays gets NaN. The offsets of both streams are validated on the host before anything is launched (one small copy and a stream wait: this
// is an epoch-end call), so no kernel reads through an unchecked offset.
#include "common.h"
#include "../../include/cxrmate_hip.h"

#include <vector>

#pragma clang fp contract(off)      // the float64 expressions below are evaluated as written, operation for operation, like the definition

namespace {

constexpr int NLG_MAX_LEN = CXR_COCO_NLG_MAX_LEN; // longest supported text, in tokens of either stream
constexpr int NLG_THREADS = 256;
constexpr int NLG_COLS = 6;                       // bleu_1..4, rouge, cider
constexpr int NLG_INTS = 9;                       // len_hyp, len_ref, c_1..c_4, lcs, rouge len_hyp, rouge len_ref
constexpr unsigned long long NLG_EMPTY = ~0ull;   // never a key: a slot index has its top bit clear

__device__ __forceinline__ unsigned int nlg_hash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned int)k;
}

// sum of one double per thread in a fixed tree; every thread gets the result. `red` holds NLG_THREADS doubles.
__device__ __forceinline__ double nlg_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int w = NLG_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(NLG_THREADS) void nlg_insert_kernel(const int* __restrict__ ids, const int* __restrict__ off, int n_texts, int k,
                                                                 const int* __restrict__ prev, int* __restrict__ gid,
                                                                 unsigned long long* __restrict__ table, unsigned int mask) {
    for (int t = blockIdx.x; t < n_texts; t += gridDim.x) {
        const int lo = off[t], hi = off[t + 1];
        for (int p = lo + (int)threadIdx.x; p < hi; p += NLG_THREADS) {
            int slot = -1;
            if (p + k <= hi) {
                const unsigned long long key = ((unsigned long long)(k > 1 ? (unsigned int)prev[p] : 0u) << 32) | (unsigned int)ids[p + k - 1];
                unsigned int h = nlg_hash(key) & mask;
                for (unsigned int probe = 0; probe <= mask; ++probe) {             // load <= 1/2: ends long before the bound
                    const unsigned long long old = atomicCAS(&table[h], NLG_EMPTY, key);
                    if (old == NLG_EMPTY || old == key) { slot = (int)h; break; }
                    h = (h + 1) & mask;
                }
            }
            gid[p] = slot;
        }
    }
}

__global__ __launch_bounds__(NLG_THREADS) void nlg_count_kernel(const int* __restrict__ off, int n_texts, int k, const int* __restrict__ gid,
                                                                const int* __restrict__ ref_mult, int* __restrict__ tf, int* __restrict__ df) {
    __shared__ int s[NLG_MAX_LEN];
    for (int t = blockIdx.x; t < n_texts; t += gridDim.x) {
        const int lo = off[t], len = off[t + 1] - lo;
        const int n = max(0, len - k + 1);
        __syncthreads();
        for (int q = threadIdx.x; q < n; q += NLG_THREADS) s[q] = gid[lo + q];
        __syncthreads();
        const int mult = ref_mult[t];
        for (int p = threadIdx.x; p < len; p += NLG_THREADS) {
            int out = 0;
            if (p < n && s[p] >= 0) {
                const int g = s[p];
                bool first = true;
                for (int q = 0; q < p; ++q)
                    if (s[q] == g) { first = false; break; }
                if (first) {
                    for (int q = p; q < n; ++q) out += s[q] == g;
                    if (mult > 0) atomicAdd(&df[g], mult);
                }
            }
            tf[lo + p] = out;
        }
    }
}

__global__ __launch_bounds__(NLG_THREADS) void nlg_pair_kernel(const int* __restrict__ off, int n_texts, const int* __restrict__ pairs, int M, int k,
                                                               const int* __restrict__ gid, const int* __restrict__ tf, const int* __restrict__ df,
                                                               double* __restrict__ val, int* __restrict__ ints) {
    __shared__ int s[NLG_MAX_LEN];
    __shared__ double red[NLG_THREADS];
    __shared__ int redi[NLG_THREADS];
    const double log_m = log((double)M);
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        const int h = pairs[2 * m], r = pairs[2 * m + 1];
        if (h < 0 || h >= n_texts || r < 0 || r >= n_texts) {                      // uniform over the workgroup
            if (threadIdx.x == 0) { val[4 * (long)m + k - 1] = __builtin_nan(""); ints[NLG_INTS * (long)m + 1 + k] = -1; }
            continue;
        }
        const int ho = off[h], lh = off[h + 1] - ho, ro = off[r], lr = off[r + 1] - ro;
        const int nh = max(0, lh - k + 1), nr = max(0, lr - k + 1);
        __syncthreads();
        for (int q = threadIdx.x; q < nr; q += NLG_THREADS) s[q] = gid[ro + q];
        __syncthreads();
        double norm_r = 0.0;
        for (int q = threadIdx.x; q < nr; q += NLG_THREADS) {
            const int t = tf[ro + q];
            if (t > 0) {
                const double w = log_m - log(fmax(1.0, (double)df[s[q]]));
                const double v = (double)t * w;
                norm_r += v * v;
            }
        }
        double norm_h = 0.0, acc = 0.0;
        int clip = 0;
        for (int p = threadIdx.x; p < nh; p += NLG_THREADS) {
            const int t = tf[ho + p];
            if (t > 0) {
                const int g = gid[ho + p];
                int cr = 0;
                for (int q = 0; q < nr; ++q) cr += s[q] == g;
                const double w = log_m - log(fmax(1.0, (double)df[g]));
                const double vh = (double)t * w, vr = (double)cr * w;
                norm_h += vh * vh;
                acc += fmin(vh, vr) * vr;
                clip += min(t, cr);
            }
        }
        norm_r = sqrt(nlg_block_sum(norm_r, red));
        norm_h = sqrt(nlg_block_sum(norm_h, red));
        acc = nlg_block_sum(acc, red);
        redi[threadIdx.x] = clip;
        __syncthreads();
        for (int w = NLG_THREADS / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) redi[threadIdx.x] += redi[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (norm_h != 0.0 && norm_r != 0.0) acc /= norm_h * norm_r;
            const double delta = (double)(max(0, lh - 1) - max(0, lr - 1));        // `length` counts bigrams (the library's `if n == 1`)
            acc *= exp(-(delta * delta) / (2.0 * 36.0));
            val[4 * (long)m + k - 1] = acc;
            ints[NLG_INTS * (long)m + 1 + k] = redi[0];
        }
    }
}

// L[i][j] (i over the hypothesis, j over the reference, 1-based) on the anti-diagonal d = i + j, stored by i; diagonals d - 1 and d - 2 are kept
__global__ __launch_bounds__(NLG_THREADS) void nlg_lcs_kernel(const int* __restrict__ ids, const int* __restrict__ off, int n_texts,
                                                              const int* __restrict__ pairs, int M, int* __restrict__ ints) {
    __shared__ unsigned short diag[3][NLG_MAX_LEN + 1];
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        const int h = pairs[2 * m], r = pairs[2 * m + 1];
        int* o = ints + NLG_INTS * (long)m;
        if (h < 0 || h >= n_texts || r < 0 || r >= n_texts) {
            if (threadIdx.x == 0) { o[6] = -1; o[7] = -1; o[8] = -1; }
            continue;
        }
        const int ho = off[h], lh = off[h + 1] - ho, ro = off[r], lr = off[r + 1] - ro;
        __syncthreads();
        for (int d = 2; d <= lh + lr; ++d) {
            unsigned short* cur = diag[d % 3];
            const unsigned short* m1 = diag[(d + 2) % 3];
            const unsigned short* m2 = diag[(d + 1) % 3];
            const int ilo = max(1, d - lr), ihi = min(lh, d - 1);
            for (int i = ilo + (int)threadIdx.x; i <= ihi; i += NLG_THREADS) {
                const int j = d - i;
                int v;
                if (ids[ho + i - 1] == ids[ro + j - 1]) v = ((i > 1 && j > 1) ? (int)m2[i - 1] : 0) + 1;
                else v = max(i > 1 ? (int)m1[i - 1] : 0, j > 1 ? (int)m1[i] : 0);
                cur[i] = (unsigned short)v;
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            o[6] = (lh > 0 && lr > 0) ? (int)diag[(lh + lr) % 3][lh] : 0;
            o[7] = lh;
            o[8] = lr;
        }
    }
}

__global__ __launch_bounds__(NLG_THREADS) void nlg_record_kernel(const int* __restrict__ off, int n_texts, const int* __restrict__ pairs, int M,
                                                                 const double* __restrict__ val, int* __restrict__ ints, double* __restrict__ scores) {
    const int m = blockIdx.x * NLG_THREADS + threadIdx.x;
    if (m >= M) return;
    int* o = ints + NLG_INTS * (long)m;
    double* sc = scores + NLG_COLS * (long)m;
    const int h = pairs[2 * m], r = pairs[2 * m + 1];
    if (h < 0 || h >= n_texts || r < 0 || r >= n_texts) {
        o[0] = -1; o[1] = -1;
        for (int c = 0; c < NLG_COLS; ++c) sc[c] = __builtin_nan("");
        return;
    }
    const int lh = off[h + 1] - off[h], lr = off[r + 1] - off[r];
    o[0] = lh; o[1] = lr;
    double b = 1.0, bleu[4];
    for (int k = 1; k <= 4; ++k) {
        b *= ((double)o[1 + k] + 1e-15) / ((double)max(0, lh - k + 1) + 1e-9);
        bleu[k - 1] = pow(b, 1.0 / (double)k);
    }
    const double ratio = ((double)lh + 1e-15) / ((double)lr + 1e-9);
    if (ratio < 1.0) {
        const double bp = exp(1.0 - 1.0 / ratio);
        for (int k = 0; k < 4; ++k) bleu[k] *= bp;
    }
    for (int k = 0; k < 4; ++k) sc[k] = bleu[k];
    double rouge = 0.0;
    if (o[7] > 0 && o[8] > 0) {
        const double p = (double)o[6] / (double)o[7], rc = (double)o[6] / (double)o[8];
        const double beta2 = 1.2 * 1.2;
        if (p != 0.0 && rc != 0.0) rouge = ((1.0 + beta2) * p * rc) / (rc + beta2 * p);
    }
    sc[4] = rouge;
    const double* v = val + 4 * (long)m;
    sc[5] = ((((v[0] + v[1]) + v[2]) + v[3]) / 4.0) * 10.0;
}

__global__ __launch_bounds__(NLG_THREADS) void nlg_study_kernel(const double* __restrict__ scores, const int* __restrict__ order, int M,
                                                                const int* __restrict__ study_off, int S, double* __restrict__ study) {
    const long idx = (long)blockIdx.x * NLG_THREADS + threadIdx.x;
    if (idx >= (long)S * NLG_COLS) return;
    const int s = (int)(idx / NLG_COLS), c = (int)(idx % NLG_COLS);
    const int lo = study_off[s], hi = study_off[s + 1];
    bool ok = lo >= 0 && hi <= M && lo < hi;
    double a = 0.0;
    if (ok) {
        for (int i = lo; i < hi; ++i) {
            const int rec = order[i];
            if (rec < 0 || rec >= M) { ok = false; break; }
            a += scores[NLG_COLS * (long)rec + c];
        }
    }
    study[idx] = ok ? a / (double)(hi - lo) : __builtin_nan("");
}

__global__ __launch_bounds__(NLG_THREADS) void nlg_average_kernel(const double* __restrict__ study, int S, double* __restrict__ avg) {
    __shared__ double red[NLG_THREADS];
    const int c = blockIdx.x;
    double a = 0.0;
    for (int s = threadIdx.x; s < S; s += NLG_THREADS) a += study[NLG_COLS * (long)s + c];
    a = nlg_block_sum(a, red);
    if (threadIdx.x == 0) avg[c] = a / (double)S;                                   // S == 0: 0 / 0, the mean of nothing is NaN
}

struct NlgWorkspace {
    long cap, table, df, gid0, gid1, tf, val, total;      // table capacity (slots) and byte offsets
};

inline NlgWorkspace nlg_workspace(long n_ids, long M) {
    NlgWorkspace w;
    w.cap = 1024;
    while (w.cap < 2 * n_ids) w.cap <<= 1;
    const long ids_bytes = ((n_ids * 4 + 7) / 8) * 8;
    w.table = 0;
    w.df = w.table + w.cap * 8;
    w.gid0 = w.df + w.cap * 4;
    w.gid1 = w.gid0 + ids_bytes;
    w.tf = w.gid1 + ids_bytes;
    w.val = w.tf + ids_bytes;
    w.total = w.val + M * 4 * 8;
    return w;
}

// offsets [n_texts + 1]: start at 0, never decrease, stay inside the stream, no text longer than NLG_MAX_LEN
bool nlg_offsets_ok(const std::vector<int>& off, long n_ids) {
    if (off.front() != 0 || off.back() > n_ids) return false;
    for (size_t t = 0; t + 1 < off.size(); ++t)
        if (off[t + 1] < off[t] || off[t + 1] - off[t] > NLG_MAX_LEN) return false;
    return true;
}

}  // namespace

// workspace: see nlg_workspace -- cap = the power of two >= max(1024, 2 * n_ids_a); cap * 12 + 3 * round_up(n_ids_a * 4, 8) + M * 32 bytes
extern "C" int cxr_coco_nlg_scores(const int* ids_a, long n_ids_a, const int* off_a, const int* ids_b, long n_ids_b, const int* off_b, int n_texts,
                                   const int* pairs, const int* ref_mult, int M, const int* order, const int* study_off, int S, double* scores,
                                   int* ints, double* study, double* avg, void* workspace, long workspace_bytes, hipStream_t stream) {
    if (n_texts < 0 || M < 0 || S < 0 || n_ids_a < 0 || n_ids_b < 0 || n_ids_a > (1l << 28) || n_ids_b > (1l << 28) || !avg) return CXR_ERR_ARG;
    if ((n_ids_a > 0 && !ids_a) || (n_ids_b > 0 && !ids_b) || (S > 0 && (!study_off || !study)) || (S > 0 && M > 0 && !order)) return CXR_ERR_ARG;
    if (M > 0 && (n_texts == 0 || !off_a || !off_b || !pairs || !ref_mult || !scores || !ints)) return CXR_ERR_ARG;
    const NlgWorkspace w = nlg_workspace(n_ids_a, M);
    if (M > 0 && (!workspace || workspace_bytes < w.total || (((size_t)workspace) % 8))) return CXR_ERR_ARG;
    if (M > 0) {
        std::vector<int> ha(n_texts + 1), hb(n_texts + 1);
        if (hipMemcpyAsync(ha.data(), off_a, ha.size() * sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(hb.data(), off_b, hb.size() * sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {
            g_cxr_last_hip_error = (int)hipGetLastError();
            return CXR_ERR_LAUNCH;
        }
        if (!nlg_offsets_ok(ha, n_ids_a) || !nlg_offsets_ok(hb, n_ids_b)) return CXR_ERR_ARG;

        char* base = (char*)workspace;
        unsigned long long* table = (unsigned long long*)(base + w.table);
        int* df = (int*)(base + w.df);
        int* gid[2] = {(int*)(base + w.gid0), (int*)(base + w.gid1)};
        int* tf = (int*)(base + w.tf);
        double* val = (double*)(base + w.val);
        const dim3 text_grid(n_texts < (1 << 20) ? n_texts : (1 << 20)), pair_grid(M < (1 << 20) ? M : (1 << 20)), block(NLG_THREADS);
        for (int k = 1; k <= 4; ++k) {
            int* cur = gid[k & 1];
            const int* prev = gid[(k + 1) & 1];
            if (hipMemsetAsync(table, 0xff, (size_t)w.cap * 8, stream) != hipSuccess || hipMemsetAsync(df, 0, (size_t)w.cap * 4, stream) != hipSuccess) {
                g_cxr_last_hip_error = (int)hipGetLastError();
                return CXR_ERR_LAUNCH;
            }
            CXR_LAUNCH(nlg_insert_kernel, text_grid, block, 0, stream, ids_a, off_a, n_texts, k, prev, cur, table, (unsigned int)(w.cap - 1));
            CXR_LAUNCH_CHECK();
            CXR_LAUNCH(nlg_count_kernel, text_grid, block, 0, stream, off_a, n_texts, k, (const int*)cur, ref_mult, tf, df);
            CXR_LAUNCH_CHECK();
            CXR_LAUNCH(nlg_pair_kernel, pair_grid, block, 0, stream, off_a, n_texts, pairs, M, k, (const int*)cur, (const int*)tf, (const int*)df, val,
                       ints);
            CXR_LAUNCH_CHECK();
        }
        CXR_LAUNCH(nlg_lcs_kernel, pair_grid, block, 0, stream, ids_b, off_b, n_texts, pairs, M, ints);
        CXR_LAUNCH_CHECK();
        CXR_LAUNCH(nlg_record_kernel, dim3(cdiv(M, NLG_THREADS)), block, 0, stream, off_a, n_texts, pairs, M, (const double*)val, ints, scores);
        CXR_LAUNCH_CHECK();
    }
    if (S > 0) {
        CXR_LAUNCH(nlg_study_kernel, dim3(cdiv((long)S * NLG_COLS, NLG_THREADS)), dim3(NLG_THREADS), 0, stream, (const double*)scores, order, M,
                   study_off, S, study);
        CXR_LAUNCH_CHECK();
    }
    CXR_LAUNCH(nlg_average_kernel, dim3(NLG_COLS), dim3(NLG_THREADS), 0, stream, (const double*)study, S, avg);
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}
