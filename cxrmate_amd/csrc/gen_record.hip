// Per-step outputs of generate() (TF5 generation/utils.py @ 5.15.0): `logits` (the raw next-token logits, _sample :2904, _beam_search :3394) and
// `scores` (the processed scores, _sample :2902; on the beam path the processed log-probs, :3396, recorded BEFORE the running beam scores are
// added). One pass over the fp32 score rows of the current step writes up to two contiguous [R, V] slots: a copy of the raw rows, and either
// a copy of the (already processed) rows or their log_softmax. Output rows can be permuted from the beam-major order of the device decode
// (row = beam * S + study) to the study-major order the library returns (study * nb + beam). No host reads, no allocation: capturable.
#include "common.h"
#include "../../include/cxrmate_hip.h"

constexpr int GR_THREADS = 256;

// Running (max, sum exp(x - max)) of one lane. -inf entries (banned tokens) contribute nothing, as in torch's log_softmax.
__device__ __forceinline__ void gr_push(float x, float& m, float& s) {
    if (x == -INFINITY) return;
    if (x > m) { s = s * __expf(m - x) + 1.f; m = x; }
    else s += __expf(x - m);
}
__device__ __forceinline__ void gr_merge(float om, float os, float& m, float& s) {
    if (om == -INFINITY) return;
    if (m == -INFINITY) { m = om; s = os; return; }
    const float n = fmaxf(m, om);
    s = s * __expf(m - n) + os * __expf(om - n);
    m = n;
}

// One workgroup per input row. VEC: 16-byte accesses (V, ld multiples of 4, 16-byte aligned base pointers). The row is read from HBM once for
// its statistics; the write pass reads it again from the cache (a 30000-entry row is 120 KB).
template <bool VEC>
__global__ __launch_bounds__(GR_THREADS) void gen_record_kernel(const float* __restrict__ x, long ld, int V, int S, int nb,
                                                                float* __restrict__ lo, float* __restrict__ so, int lsm) {
    __shared__ float shm[GR_THREADS / 64], shs[GR_THREADS / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* row = x + (long)r * ld;
    const long orow = (long)((r % S) * nb + r / S) * V;
    float off = 0.f;
    if (so && lsm) {
        float m = -INFINITY, s = 0.f;
        if (VEC) {
            for (int v = tid * 4; v < V; v += GR_THREADS * 4) {
                const float4 t = *reinterpret_cast<const float4*>(row + v);
                gr_push(t.x, m, s); gr_push(t.y, m, s); gr_push(t.z, m, s); gr_push(t.w, m, s);
            }
        } else {
            for (int v = tid; v < V; v += GR_THREADS) gr_push(row[v], m, s);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) gr_merge(__shfl_xor(m, o, 64), __shfl_xor(s, o, 64), m, s);
        if ((tid & 63) == 0) { shm[tid >> 6] = m; shs[tid >> 6] = s; }
        __syncthreads();
        m = shm[0]; s = shs[0];
#pragma unroll
        for (int w = 1; w < GR_THREADS / 64; ++w) gr_merge(shm[w], shs[w], m, s);
        off = m + __logf(s);                // a row of -inf only: -inf + log 0 = -inf, and x - off = NaN, as torch gives
    }
    if (VEC) {
        for (int v = tid * 4; v < V; v += GR_THREADS * 4) {
            const float4 t = *reinterpret_cast<const float4*>(row + v);
            if (lo) *reinterpret_cast<float4*>(lo + orow + v) = t;
            if (so) *reinterpret_cast<float4*>(so + orow + v) = lsm ? make_float4(t.x - off, t.y - off, t.z - off, t.w - off) : t;
        }
    } else {
        for (int v = tid; v < V; v += GR_THREADS) {
            const float t = row[v];
            if (lo) lo[orow + v] = t;
            if (so) so[orow + v] = lsm ? t - off : t;
        }
    }
}

extern "C" int cxr_gen_record_f32(const float* x, long ld, long R, int V, int nb, float* logits_out, float* scores_out, int log_softmax,
                                  hipStream_t stream) {
    if (!x || R <= 0 || V <= 0 || ld < V || nb <= 0 || R % nb != 0 || R > 0x7fffffffL || (!logits_out && !scores_out)) return CXR_ERR_ARG;
    const int S = (int)(R / nb);
    const bool vec = V % 4 == 0 && ld % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)logits_out & 15) == 0 && ((uintptr_t)scores_out & 15) == 0;
    const int lsm = log_softmax ? 1 : 0;
    if (vec) CXR_LAUNCH(gen_record_kernel<true>, dim3((unsigned)R), dim3(GR_THREADS), 0, stream, x, ld, V, S, (int)nb, logits_out, scores_out, lsm);
    else CXR_LAUNCH(gen_record_kernel<false>, dim3((unsigned)R), dim3(GR_THREADS), 0, stream, x, ld, V, S, (int)nb, logits_out, scores_out, lsm);
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}
