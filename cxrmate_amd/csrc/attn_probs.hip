// Attention probabilities written out (output_attentions): P[b,h,i,j] = exp(scale * q_i.k_j - LSE[b,h,i]) as fp32 [B, H, Tq, Tk], from the
// log-sum-exp that the flash forward (attention.hip) already wrote. Replaces the softmax + dropout of TF5 eager_attention_forward
// (TF5:bert:126-131) when a caller asks for the maps; the forward itself never forms them.
//
// Consistency with the forward, element for element:
//   * q.k is the same swapped v_mfma_f32_32x32x16_bf16 product (S^T = K.Q^T, same operand fragments, same accumulation order);
//   * key j is visible to query i iff kpm[b,j] != 0 and (not causal or j <= i + causal_shift); invisible entries are exactly 0;
//   * a row without any visible key is uniform over all Tk keys: the forward scores such keys ATT_NEG, which makes its softmax uniform, as
//     finfo.min does in the reference. Its LSE then sits at ATT_NEG * ln 2 (the key count is below fp32 resolution there), so the row is
//     recognised from the LSE and written as 1 / Tk. (Under the causal rule the forward's own context for such a row averages only the keys
//     of the 64-key tiles it visits; in the decoder that needs a padded first token, which no report has.)
//   * dropout: keep = dropout_keep(dropout_row_key(seed, site, b*H + h, i + t0), j, thr16), the forward's hash, and kept entries are scaled
//     by 1 / (1 - p), so P.V reproduces the context of the same pass.
//
// Bound by its output writes (B*H*Tq*Tk*4 bytes). Workgroup = 4 waves; a wave owns 32 query rows and walks 64-key tiles of one key chunk;
// each tile (32 rows x 64 keys fp32, 8 KB) goes through an XOR-swizzled LDS tile so that every global store is 16 bytes per lane and a
// full 256-byte row segment per 16 lanes.
#include "common.h"
#include "../../include/cxrmate_hip.h"

#define ATT_NEG (-1.0e30f)            // attention.hip's masked-score sentinel (log2 units)

constexpr int AP_WAVES = 4;
constexpr int AP_CHUNK = 128;         // keys per workgroup (grid.x = query blocks x key chunks): 4 KB of Q fragments per 16 KB written

struct ProbArgs {
    const bf16_t* Q; const bf16_t* K; const float* LSE; const unsigned char* kpm; float* P;
    long q_bs, q_rs, k_bs, k_rs, kpm_bs, p_bs, p_hs, p_rs;
    int B, H, Tq, Tk, nchunks;
    float scale_log2e;
    int causal, causal_shift;
    const uint32_t* drop_seed; uint32_t drop_site, drop_thr16; float drop_inv; int drop_t0;     // drop_thr16 == 0: off
    int vec;                          // P rows 16-byte aligned (Tk % 4 == 0 and aligned base / strides): float4 stores
};

__global__ __launch_bounds__(AP_WAVES * 64) void attn_probs_kernel(const ProbArgs a) {
    __shared__ __attribute__((aligned(16))) float Pt[AP_WAVES][32 * 64];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int head = blockIdx.y, b = blockIdx.z;
    const int qblk = blockIdx.x / a.nchunks, chunk = blockIdx.x % a.nchunks;
    const int row0 = qblk * (AP_WAVES * 32) + wave * 32;
    if (row0 >= a.Tq) return;                                       // wave-uniform; no workgroup barrier follows
    const int ql = lane & 31, hh = lane >> 5;
    const int qrow = row0 + ql;
    const int qc = qrow < a.Tq ? qrow : a.Tq - 1;

    bf16x8_t qf[4];                                                 // B operand of S^T = K.Q^T: Q[q][16s + 8hh + 0..7]
    {
        const bf16_t* qp = a.Q + (long)b * a.q_bs + (long)qc * a.q_rs + head * 64 + hh * 8;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8_t*>(qp + s * 16);
    }
    const float lse2 = a.LSE[((long)b * a.H + head) * a.Tq + qc] * 1.4426950408889634f;
    const bool dead = lse2 < 0.5f * ATT_NEG;                        // no visible key: uniform row
    const float uni = 1.0f / (float)a.Tk;
    const uint32_t drop_key = a.drop_thr16 ? dropout_row_key(*a.drop_seed, a.drop_site, (uint32_t)(b * a.H + head), (uint32_t)(qrow + a.drop_t0)) : 0u;

    const bf16_t* kbase = a.K + (long)b * a.k_bs + head * 64;
    const unsigned char* mrow = a.kpm ? a.kpm + (long)b * a.kpm_bs : nullptr;
    float* prow0 = a.P + (long)b * a.p_bs + (long)head * a.p_hs + (long)row0 * a.p_rs;
    float* Tw = Pt[wave];
    const int rows_valid = a.Tq - row0 < 32 ? a.Tq - row0 : 32;

    const int k_begin = chunk * AP_CHUNK;
    const int k_end = k_begin + AP_CHUNK < a.Tk ? k_begin + AP_CHUNK : a.Tk;
    for (int kv0 = k_begin; kv0 < k_end; kv0 += 64) {
        // visibility of the tile's 64 keys by key padding and Tk (wave-uniform bits); the causal rule is per row, below
        const int key = kv0 + lane;
        const bool live = key < a.Tk && (mrow == nullptr || mrow[key] != 0);
        const unsigned long long live_bits = __ballot(live);

        f32x16_t st[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            int kr = kv0 + kt * 32 + ql;
            kr = kr < a.Tk ? kr : a.Tk - 1;
            const bf16_t* kp = kbase + (long)kr * a.k_rs + hh * 8;
            bf16x8_t kf[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) kf[s] = *reinterpret_cast<const bf16x8_t*>(kp + s * 16);
#pragma unroll
            for (int i = 0; i < 16; ++i) st[kt][i] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s], qf[s], st[kt], 0, 0, 0);
        }
        // lane (ql, hh), register r of sub-tile kt holds key kv0 + kt*32 + (r & 3) + 8*(r >> 2) + 4*hh of query row qrow
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kl = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                const int j = kv0 + kl;
                bool ok = (live_bits >> kl) & 1ull;
                if (a.causal) ok = ok && (j <= qrow + a.causal_shift);
                float p = ok ? __builtin_amdgcn_exp2f(fmaf(st[kt][r], a.scale_log2e, -lse2)) : 0.f;
                if (dead) p = j < a.Tk ? uni : 0.f;
                if (a.drop_thr16) p = dropout_keep(drop_key, (uint32_t)j, a.drop_thr16) ? p * a.drop_inv : 0.f;
                st[kt][r] = p;
            }
        // registers -> LDS: the 4 consecutive keys of (kt, rg) are 16-byte chunk c = kt*8 + 2*rg + hh of the row's 16; chunk slots XOR-swizzled
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int c = kt * 8 + 2 * rg + hh;
                float4 v = make_float4(st[kt][4 * rg], st[kt][4 * rg + 1], st[kt][4 * rg + 2], st[kt][4 * rg + 3]);
                *reinterpret_cast<float4*>(Tw + ql * 64 + ((c ^ (ql & 15)) << 2)) = v;
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // LDS -> rows: 16 lanes per row (256 contiguous bytes), 4 rows per instruction
        const int cc = lane & 15;
        const int col = kv0 + cc * 4;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int r = it * 4 + (lane >> 4);
            const float4 v = *reinterpret_cast<const float4*>(Tw + r * 64 + ((cc ^ (r & 15)) << 2));
            if (r < rows_valid) {
                float* dst = prow0 + (long)r * a.p_rs + col;
                if (a.vec && col + 4 <= a.Tk) {
                    *reinterpret_cast<float4*>(dst) = v;
                } else {
                    if (col < a.Tk) dst[0] = v.x;
                    if (col + 1 < a.Tk) dst[1] = v.y;
                    if (col + 2 < a.Tk) dst[2] = v.z;
                    if (col + 3 < a.Tk) dst[3] = v.w;
                }
            }
        }
    }
}

extern "C" int cxr_attn_probs_f32(const void* Q, const void* K, const float* LSE, const void* kpm, float* P, long q_bs, long q_rs, long k_bs,
                                  long k_rs, long kpm_bs, long p_bs, long p_hs, long p_rs, int B, int H, int Tq, int Tk, float scale, int causal,
                                  int causal_shift, float drop_p, const unsigned int* drop_seed, unsigned int drop_site, int drop_t0, hipStream_t stream) {
    if (!Q || !K || !LSE || !P || B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0) return CXR_ERR_ARG;
    if (drop_p < 0.f || drop_p >= 1.f || (drop_p > 0.f && !drop_seed)) return CXR_ERR_ARG;
    if ((q_rs % 8) || (k_rs % 8) || (q_bs % 8) || (k_bs % 8) || (((size_t)Q) % 16) || (((size_t)K) % 16)) return CXR_ERR_ARG;
    if (p_rs < Tk || (((size_t)P) % 4)) return CXR_ERR_ARG;
    ProbArgs a;
    a.Q = (const bf16_t*)Q; a.K = (const bf16_t*)K; a.LSE = LSE; a.kpm = (const unsigned char*)kpm; a.P = P;
    a.q_bs = q_bs; a.q_rs = q_rs; a.k_bs = k_bs; a.k_rs = k_rs; a.kpm_bs = kpm_bs; a.p_bs = p_bs; a.p_hs = p_hs; a.p_rs = p_rs;
    a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.nchunks = cdiv(Tk, AP_CHUNK);
    a.scale_log2e = scale * 1.4426950408889634f; a.causal = causal; a.causal_shift = causal_shift;
    a.drop_seed = drop_seed; a.drop_site = drop_site; a.drop_thr16 = drop_p > 0.f ? dropout_thr16(drop_p) : 0u;
    a.drop_inv = 1.0f / (1.0f - drop_p); a.drop_t0 = drop_t0;
    a.vec = (((size_t)P) % 16 == 0) && (p_rs % 4 == 0) && (p_hs % 4 == 0) && (p_bs % 4 == 0);
    const dim3 grid(cdiv(Tq, AP_WAVES * 32) * a.nchunks, H, B), block(AP_WAVES * 64);
    CXR_LAUNCH(attn_probs_kernel, grid, block, 0, stream, a);
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}
