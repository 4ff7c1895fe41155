// BERTScore greedy matching (bert_score.utils.greedy_cos_idf, idf=False, all_layers=False) over the trunk's last hidden states.
//
// One workgroup per (hyp, ref) pair; the Lh x Lr cosine matrix never leaves the registers:
//   sim[j,k] = <h_j, r_k> * inv|h_j| * inv|r_k|, the dot products on the matrix cores (v_mfma_f32_16x16x32_bf16, the raw bf16 rows in, fp32
//   accumulate) and the inverse norms in fp32 from the same bf16 values. Rounding the normalised vectors to bf16 instead would add ~1e-3 of cosine
//   error, which the baseline rescale (x - b) / (1 - b) multiplies by ~6.
//   Each wave owns 16-row hyp blocks (block hb = wave, wave + 4, ...): the block's rows stay in registers as A fragments for the whole pass over
//   the ref rows, which stream through 16 at a time as B fragments. Row maxima are kept in registers; column maxima in LDS, one copy per wave
//   (no atomics), merged at the end.
//   P = sum_j w_j max_k sim[j,k] / sum_j w_j over hyp tokens, R the same over ref tokens with the max over j, F = 2PR / (P + R) (NaN -> 0); a pair
//   with an empty side (length 2: <s></s>) gets P = R = 0 after F was formed, exactly as the reference orders it.
//   Zero floor: the reference pads each chunk of pairs to the chunk's longest hyp / ref and multiplies sim by the mask, so padded entries are exact
//   zeros inside the max. floor[pair][0] != 0 floors the row maxima at 0 (this pair's ref is shorter than its chunk's longest ref), floor[pair][1]
//   the column maxima (this pair's hyp is shorter than its chunk's longest hyp). The host computes both.
#include "common.h"
#include "../../include/cxrmate_hip.h"

namespace {

constexpr int BS_MAXLEN = 512;          // tokens per side (RoBERTa's model_max_length)

template <int D>
__global__ __launch_bounds__(256) void bertscore_match_kernel(const bf16_t* __restrict__ H, long n_rows, const int* __restrict__ sent, int n_sent,
                                                              const int* __restrict__ pairs, const float* __restrict__ w,
                                                              const unsigned char* __restrict__ floors, float* __restrict__ P,
                                                              float* __restrict__ R, float* __restrict__ F) {
    constexpr int KS = D / 32;                  // 32-wide k steps per dot product
    constexpr int CH = D / 8;                   // 16-byte chunks per row
    __shared__ float inv_h[BS_MAXLEN], inv_r[BS_MAXLEN];
    __shared__ float colmax[4][BS_MAXLEN];
    __shared__ float red[4][4];
    const int pair = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hs = pairs[2 * pair], rs = pairs[2 * pair + 1];
    bool ok = hs >= 0 && hs < n_sent && rs >= 0 && rs < n_sent;
    long ho = 0, ro = 0;
    int Lh = 0, Lr = 0;
    if (ok) {
        ho = sent[2 * hs]; Lh = sent[2 * hs + 1]; ro = sent[2 * rs]; Lr = sent[2 * rs + 1];
        ok = Lh >= 1 && Lh <= BS_MAXLEN && Lr >= 1 && Lr <= BS_MAXLEN && ho >= 0 && ro >= 0 && ho + Lh <= n_rows && ro + Lr <= n_rows;
    }
    if (!ok) {                                  // a table entry outside the buffer: NaN result, nothing read (uniform over the workgroup)
        if (threadIdx.x == 0) P[pair] = R[pair] = F[pair] = __builtin_nanf("");
        return;
    }
    const bool floor_p = floors[2 * pair] != 0, floor_r = floors[2 * pair + 1] != 0;

    // inverse norms of every row of both sentences (fp32 from the bf16 values), one wave per row
    for (int t = wave; t < Lh + Lr; t += 4) {
        const bf16_t* row = H + (t < Lh ? ho + t : ro + (t - Lh)) * (long)D;
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < (CH + 63) / 64; ++i) {
            const int ch = lane + i * 64;
            if (ch < CH) {
                float v[8];
                unpack8(*reinterpret_cast<const uint4*>(row + ch * 8), v);
#pragma unroll
                for (int j = 0; j < 8; ++j) ss = fmaf(v[j], v[j], ss);
            }
        }
        ss = group_sum<64>(ss);
        if (lane == 0) {
            if (t < Lh) inv_h[t] = 1.0f / sqrtf(ss);
            else inv_r[t - Lh] = 1.0f / sqrtf(ss);
        }
    }
    for (int i = threadIdx.x; i < 4 * BS_MAXLEN; i += 256) (&colmax[0][0])[i] = -INFINITY;
    __syncthreads();

    const int r16 = lane & 15, kg = lane >> 4;  // operand maps of 16x16x32: row / column r16, k = 8 kg + j; accumulator: column r16, rows 4 kg + i
    const int nbh = (Lh + 15) / 16, nbr = (Lr + 15) / 16;
    float num_p = 0.f;
    for (int hb = wave; hb < nbh; hb += 4) {
        const int hrow = min(hb * 16 + r16, Lh - 1);                  // rows past the sentence re-read its last row; their results are masked
        const bf16_t* ap = H + (ho + hrow) * (long)D + kg * 8;
        bf16x8_t a[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = *reinterpret_cast<const bf16x8_t*>(ap + s * 32);
        float ih[4], rmax[4];
        bool rv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rr = hb * 16 + kg * 4 + i;
            rv[i] = rr < Lh;
            ih[i] = inv_h[min(rr, Lh - 1)];
            rmax[i] = -INFINITY;
        }
        for (int rb = 0; rb < nbr; ++rb) {
            const int col = rb * 16 + r16;
            const bf16_t* bp = H + (ro + min(col, Lr - 1)) * (long)D + kg * 8;
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s], *reinterpret_cast<const bf16x8_t*>(bp + s * 32), acc, 0, 0, 0);
            const bool cv = col < Lr;
            const float ir = inv_r[min(col, Lr - 1)];
            float cm = -INFINITY;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float s = acc[i] * ih[i] * ir;
                if (rv[i] && cv) { rmax[i] = fmaxf(rmax[i], s); cm = fmaxf(cm, s); }
            }
            cm = fmaxf(cm, __shfl_xor(cm, 16, 64));                   // the column's 16 rows sit in the four lane groups
            cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
            if (kg == 0 && cv) colmax[wave][col] = fmaxf(colmax[wave][col], cm);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float m = group_max<16>(rmax[i]);                     // over the 16 columns of the lane group
            if (r16 == 0 && rv[i]) num_p = fmaf(w[ho + hb * 16 + kg * 4 + i], floor_p ? fmaxf(m, 0.f) : m, num_p);
        }
    }
    __syncthreads();
    float num_r = 0.f, den_r = 0.f, den_p = 0.f;
    for (int c = threadIdx.x; c < Lr; c += 256) {
        float m = fmaxf(fmaxf(colmax[0][c], colmax[1][c]), fmaxf(colmax[2][c], colmax[3][c]));
        if (floor_r) m = fmaxf(m, 0.f);
        const float wc = w[ro + c];
        num_r = fmaf(wc, m, num_r);
        den_r += wc;
    }
    for (int j = threadIdx.x; j < Lh; j += 256) den_p += w[ho + j];
    num_p = group_sum<64>(num_p); num_r = group_sum<64>(num_r); den_r = group_sum<64>(den_r); den_p = group_sum<64>(den_p);
    if (lane == 0) { red[wave][0] = num_p; red[wave][1] = den_p; red[wave][2] = num_r; red[wave][3] = den_r; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        float p = s[0] / s[1], r = s[2] / s[3];                          // 0 / 0 = NaN when a side has no weighted token (as the reference)
        float f = 2.f * p * r / (p + r);
        if (f != f) f = 0.f;
        if (Lh == 2 || Lr == 2) { p = 0.f; r = 0.f; }                     // empty candidate / reference: raw P and R are 0, F as formed above
        P[pair] = p; R[pair] = r; F[pair] = f;
    }
}

}  // namespace

extern "C" int cxr_bertscore_match(const void* hidden, long n_rows, int D, const int* sent, int n_sent, const int* pairs, const float* weights,
                                   const unsigned char* floors, int n_pairs, float* P, float* R, float* F, hipStream_t stream) {
    if (!hidden || !sent || !pairs || !weights || !floors || !P || !R || !F || n_rows <= 0 || n_sent <= 0 || n_pairs <= 0 ||
        (((size_t)hidden) % 16))
        return CXR_ERR_ARG;
    if (D == 768)
        CXR_LAUNCH(bertscore_match_kernel<768>, dim3(n_pairs), dim3(256), 0, stream, (const bf16_t*)hidden, n_rows, sent, n_sent, pairs, weights,
                   floors, P, R, F);
    else if (D == 1024)
        CXR_LAUNCH(bertscore_match_kernel<1024>, dim3(n_pairs), dim3(256), 0, stream, (const bf16_t*)hidden, n_rows, sent, n_sent, pairs, weights,
                   floors, P, R, F);
    else
        return CXR_ERR_ARG;
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}
