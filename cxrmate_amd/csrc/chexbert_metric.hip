// CheXbert classification scores (reference tools/metrics/chexbert.py:191-336) from the labeller's class-index tables, on the device.
//
// Records arrive grouped by study (CSR offsets); a record names its row in the prediction table and its row in the label table (a distinct label
// text is labelled once and shared). Positive is class index 1; blank (0), negative (2) and uncertain (3) are negative.
//   pass 1  16 lanes per study, one per pathology (14 used): tp / fp / fn counted as integers over the study's records, each error type = count / n
//           (the reference's mean over the DICOMs of a study; exact, the counts are small integers). The study's four sums over the 14 pathologies
//           are taken in pathology order (the same value in every lane), then its accuracy / precision / recall / f1. The per-(error type, pathology)
//           means go to the workspace column-major ([56][S]) for pass 2.
//   pass 2  one workgroup per column (56 error-type columns + the 4 ratio columns of `example`): every thread adds its rows s = tid, tid + 256, ... in
//           order, the 256 partial sums are folded through LDS in a fixed tree. No atomics: two launches give the same bits.
//   pass 3  one wave: the 14 x 8 class table, the macro means, the micro ratios.
// Ratios of `example` and `cls` with a zero denominator are 0 (the reference's fillna(0)); the micro ratios are plain divisions and stay NaN there.
// A study whose offsets or row indices point outside their tables gets NaN in all its outputs (nothing is read through the index); the NaN then
// reaches every column sum, as it should: such a table has no scores.
#include "common.h"
#include "../../include/cxrmate_hip.h"

namespace {

constexpr int CM_P = 14;                 // pathologies
constexpr int CM_COLS = 4 * CM_P;        // error-type columns of the workspace: (tp, tn, fp, fn) x pathology
constexpr int CM_RED = CM_COLS + 4;      // + accuracy, precision, recall, f1 of `example`

__device__ __forceinline__ double ratio0(double num, double den) { return den == 0.0 ? 0.0 : num / den; }      // NaN operands stay NaN

__global__ __launch_bounds__(256) void chexbert_study_kernel(const long* __restrict__ pred, int n_pred, const long* __restrict__ ref, int n_ref,
                                                             const int* __restrict__ pred_row, const int* __restrict__ ref_row, int M,
                                                             const int* __restrict__ study_off, int S, double* __restrict__ example,
                                                             double* __restrict__ per) {
    const int c = threadIdx.x & 15;
    const int s = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = s < S;
    int lo = 0, hi = 0;
    if (live) { lo = study_off[s]; hi = study_off[s + 1]; }
    bool ok = live && lo >= 0 && hi <= M && lo < hi;
    int tp = 0, fp = 0, fn = 0;
    if (ok) {
        for (int r = lo; r < hi; ++r) {
            const int pr = pred_row[r], rr = ref_row[r];
            if (pr < 0 || pr >= n_pred || rr < 0 || rr >= n_ref) { ok = false; break; }          // uniform over the study's 16 lanes
            if (c < CM_P) {
                const bool p = pred[(long)pr * CM_P + c] == 1, y = ref[(long)rr * CM_P + c] == 1;
                tp += p && y; fp += p && !y; fn += !p && y;
            }
        }
    }
    const double nan = __builtin_nan("");
    const double n = (double)(hi - lo);
    double e[4];
    e[0] = ok ? (double)tp / n : nan;
    e[1] = ok ? (double)(hi - lo - tp - fp - fn) / n : nan;
    e[2] = ok ? (double)fp / n : nan;
    e[3] = ok ? (double)fn / n : nan;
    if (live && c < CM_P) {
#pragma unroll
        for (int k = 0; k < 4; ++k) per[(long)(k * CM_P + c) * S + s] = e[k];
    }
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    const int base = (threadIdx.x & 63) & ~15;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < CM_P; ++j) t[k] += __shfl(e[k], base + j, 64);                       // pathology order, the same sum in every lane
    if (live && c == 0) {
        double* o = example + (long)s * 8;
        o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
        o[4] = ratio0(t[0] + t[1], t[0] + t[1] + t[2] + t[3]);
        o[5] = ratio0(t[0], t[0] + t[2]);
        o[6] = ratio0(t[0], t[0] + t[3]);
        o[7] = ratio0(t[0], t[0] + 0.5 * (t[2] + t[3]));
    }
}

__global__ __launch_bounds__(256) void chexbert_column_kernel(const double* __restrict__ per, const double* __restrict__ example, int S,
                                                              double* __restrict__ colsum) {
    __shared__ double red[256];
    const int col = blockIdx.x;
    const double* src = col < CM_COLS ? per + (long)col * S : example + 4 + (col - CM_COLS);
    const long stride = col < CM_COLS ? 1 : 8;
    double a = 0.0;
    for (int s = threadIdx.x; s < S; s += 256) a += src[(long)s * stride];
    red[threadIdx.x] = a;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) colsum[col] = red[0];
}

__global__ __launch_bounds__(64) void chexbert_final_kernel(const double* __restrict__ colsum, int S, double* __restrict__ cls, double* __restrict__ avg) {
    __shared__ double tab[CM_P][8];
    const int c = threadIdx.x;
    if (c < CM_P) {
        const double tp = colsum[c], tn = colsum[CM_P + c], fp = colsum[2 * CM_P + c], fn = colsum[3 * CM_P + c];
        double v[8] = {tp, tn, fp, fn, ratio0(tn + tp, tp + tn + fp + fn), ratio0(tp, tp + fp), ratio0(tp, tp + fn), ratio0(tp, tp + 0.5 * (fp + fn))};
#pragma unroll
        for (int k = 0; k < 8; ++k) { tab[c][k] = v[k]; cls[c * 8 + k] = v[k]; }
    }
    __syncthreads();
    if (c == 0) {
        double m[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < CM_P; ++j)
            for (int k = 0; k < 8; ++k) m[k] += tab[j][k];
        for (int k = 0; k < 4; ++k) {
            avg[k] = colsum[CM_COLS + k] / (double)S;            // *_example: mean over the studies
            avg[4 + k] = m[4 + k] / (double)CM_P;                // *_macro: mean over the pathologies
        }
        const double tp = m[0], tn = m[1], fp = m[2], fn = m[3];
        avg[8] = (tp + tn) / (tp + tn + fp + fn);                // *_micro: never filled, 0 / 0 stays NaN
        avg[9] = tp / (tp + fp);
        avg[10] = tp / (tp + fn);
        avg[11] = tp / (tp + 0.5 * (fp + fn));
    }
}

}  // namespace

// workspace: the [56][S] means of pass 1, then the 60 column sums (64 doubles reserved)
static inline long chexbert_workspace_bytes(int S) { return ((long)CM_COLS * S + 64) * (long)sizeof(double); }

extern "C" int cxr_chexbert_scores(const long* pred, int n_pred, const long* ref, int n_ref, const int* pred_row, const int* ref_row, int M,
                                   const int* study_off, int S, double* example, double* cls, double* avg, void* workspace, long workspace_bytes,
                                   hipStream_t stream) {
    if (!pred || !ref || !pred_row || !ref_row || !study_off || !example || !cls || !avg || !workspace || n_pred <= 0 || n_ref <= 0 || M <= 0 ||
        S <= 0 || workspace_bytes < chexbert_workspace_bytes(S) || (((size_t)workspace) % 8))
        return CXR_ERR_ARG;
    double* per = (double*)workspace;
    double* colsum = per + (long)CM_COLS * S;
    CXR_LAUNCH(chexbert_study_kernel, dim3(cdiv(S, 16)), dim3(256), 0, stream, pred, n_pred, ref, n_ref, pred_row, ref_row, M, study_off, S, example,
               per);
    CXR_LAUNCH_CHECK();
    CXR_LAUNCH(chexbert_column_kernel, dim3(CM_RED), dim3(256), 0, stream, (const double*)per, (const double*)example, S, colsum);
    CXR_LAUNCH_CHECK();
    CXR_LAUNCH(chexbert_final_kernel, dim3(1), dim3(64), 0, stream, (const double*)colsum, S, cls, avg);
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}
