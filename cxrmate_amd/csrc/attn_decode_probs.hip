// What a cached decode step hands out when generate() / forward(past_key_values=) is asked for output_attentions / output_hidden_states
// (TF5 generation/utils.py @ 5.15.0 _sample :2906-2921, _beam_search :3398-3412 collect model_outputs.decoder_attentions / cross_attentions /
// decoder_hidden_states of every step). The step's own kernels never form these: the single-query attention kernels (csrc/decode.hip
// attn_decode_kernel, attn_cross_mfma_kernel and its QPROJ form) keep a running softmax state, and in the fused step the hidden state between
// layers exists only as an un-normalised activation in the decode activation layout with its LayerNorm folded into the next Linear. Two
// kernels, launched BESIDE the step's own (which stay exactly as they are):
//
// attn_decode_probs_kernel: P[r, h, 0, j] = softmax_j(scale * q_{r,h} . k_j) as fp32, one query per row, from bf16 Q [B, H*64] and a strided
// bf16 K view [Bkv, Tk, H*64] (KV-cache rows, a column block of kv_all, cache.ck[l]). Conventions, element for element those of
// attn_decode_kernel and of attn_probs.hip:
//   * query rows b + g*Bkv (g < B/Bkv in {1, 2, 4}) share K row b and its mask row;
//   * key j is visible iff j < Tk and its mask entry (byte, or bit j%32 of word j/32 of cxr_pack_mask_bits) is non-zero; invisible entries
//     are exactly 0 (their score is the finite sentinel -1e30: exp2 of it underflows to 0);
//   * a row without any visible key is uniform 1/Tk (every score is the sentinel, every exp2 is 1), as finfo.min gives in the reference;
//   * dropout: keep = dropout_keep(dropout_row_key(seed, site, row*H + h, drop_t), j, thr16), kept entries scaled by 1/(1-p): P.V is the
//     context the decode step computed;
//   * decode row g*(B/groups) + s is written to output row s*groups + g (study-major, as csrc/gen_record.hip stores the logits).
// Bound by reading K once (Bkv*Tk*H*64*2 bytes) and writing P: one workgroup per (K row, head) serves all query rows of the stream, 8 lanes
// per 128-byte key row (16 bytes each), and thread t of a pass over NT keys owns key k0 + t: it writes that key's scaled score into P while it
// keeps a running (max, sum), and after the workgroup has merged those it normalises the entries it wrote itself (a thread reads back its own
// stores: no fence, no LDS sized by Tk). Every store is a 4-byte vector store, 256 contiguous bytes per wave when the key stride is 1.
//
// dec_hidden_record_kernel: fp32 hidden state rows from M rows of width K in the decode activation layout: widened as they are (the embedding
// output is already normalised), or LayerNorm(gamma, beta, eps) of them with the row mean and variance computed here, in fp32, over the row
// (two passes: mean, then centred squares) -- independent of the producers' partial-statistics format. Same row permutation.
#include "common.h"
#include "../../include/cxrmate_hip.h"

struct DecProbArgs {
    const bf16_t* Q; const bf16_t* K; const unsigned char* kpm; float* P; const uint32_t* drop_seed;
    long q_bs, k_bs, k_rs, kpm_bs, p_bs, p_hs, p_ks;
    int B, Bkv, H, Tk, groups, kpm_bits, drop_t;
    float qscale, drop_inv; uint32_t drop_site, drop_thr16;
};

template <int G, int NT>
__global__ __launch_bounds__(NT) void attn_decode_probs_kernel(const DecProbArgs a) {
    constexpr int NW = NT / 64;
    __shared__ float sm[G][NW], sl[G][NW];
    const int tid = threadIdx.x, sub = tid & 7, grp = tid >> 3;
    const int h = blockIdx.x % a.H, b = blockIdx.x / a.H;                   // b indexes K (and the key-padding mask)
    const bf16_t* kb = a.K + (long)b * a.k_bs + h * 64 + sub * 8;
    const unsigned char* mrow = a.kpm ? a.kpm + (long)b * a.kpm_bs : nullptr;
    const int S = a.B / a.groups;

    uint4 qraw[G];
    float* prow[G];
    uint32_t drop_key[G];
    float m_run[G], l_run[G];
    const uint32_t dseed = a.drop_thr16 ? *a.drop_seed : 0u;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int row = b + g * a.Bkv;                                      // decode row; stored at row (row % S) * groups + row / S
        qraw[g] = *reinterpret_cast<const uint4*>(a.Q + (long)row * a.q_bs + h * 64 + sub * 8);
        prow[g] = a.P + (long)((row % S) * a.groups + row / S) * a.p_bs + (long)h * a.p_hs;
        drop_key[g] = dropout_row_key(dseed, a.drop_site, (uint32_t)(row * a.H + h), (uint32_t)a.drop_t);
        m_run[g] = -1.0e30f; l_run[g] = 0.f;
    }

    // pass 1: scaled scores (exp2 domain) of key k0 + tid into P, running (max, sum) of this thread's own keys
    for (int k0 = 0; k0 < a.Tk; k0 += NT) {
        uint4 kr[8];
        const int key0 = k0 + grp * 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) {                                       // keys past the range re-read the last row and are never stored
            int key = key0 + u; key = key < a.Tk ? key : a.Tk - 1;
            kr[u] = ld_stream16(kb + (long)key * a.k_rs);
        }
        const int mykey = k0 + tid;                                         // = key0 + sub
        const bool live = mykey < a.Tk;
        bool ok = live;
        if (mrow != nullptr && live)
            ok = a.kpm_bits ? ((reinterpret_cast<const uint32_t*>(mrow)[mykey >> 5] >> (mykey & 31)) & 1u) != 0u : mrow[mykey] != 0;
        float mine[G];
#pragma unroll
        for (int g = 0; g < G; ++g) mine[g] = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float kv[8];
            unpack8(kr[u], kv);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float qv[8], d = 0.f;
                unpack8(qraw[g], qv);
#pragma unroll
                for (int j = 0; j < 8; ++j) d += qv[j] * kv[j];
                d = group_sum<8>(d);
                mine[g] = (u == sub) ? d : mine[g];
            }
        }
        if (live) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float s = ok ? mine[g] * a.qscale : -1.0e30f;         // masked: attn_decode_kernel's finite sentinel
                prow[g][(long)mykey * a.p_ks] = s;
                const float mn = fmaxf(m_run[g], s);
                l_run[g] = l_run[g] * __builtin_amdgcn_exp2f(m_run[g] - mn) + __builtin_amdgcn_exp2f(s - mn);
                m_run[g] = mn;
            }
        }
    }

    // merge the threads' states: butterfly over the wave, then the NW wave states through LDS
    float inv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float mw = group_max<64>(m_run[g]);
        const float lw = group_sum<64>(l_run[g] * __builtin_amdgcn_exp2f(m_run[g] - mw));
        if ((tid & 63) == 0) { sm[g][tid >> 6] = mw; sl[g][tid >> 6] = lw; }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float M = -1.0e30f, L = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, sm[g][w]);
#pragma unroll
        for (int w = 0; w < NW; ++w) L += sl[g][w] * __builtin_amdgcn_exp2f(sm[g][w] - M);
        m_run[g] = M;
        inv[g] = 1.0f / L;                                                  // L >= 1: the key of the maximum contributes exp2(0)
    }

    // pass 2: every thread normalises the entries it wrote itself
    for (int k0 = 0; k0 < a.Tk; k0 += NT) {
        const int mykey = k0 + tid;
        if (mykey >= a.Tk) break;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float* dst = prow[g] + (long)mykey * a.p_ks;
            float p = __builtin_amdgcn_exp2f(*dst - m_run[g]) * inv[g];
            if (a.drop_thr16) p = dropout_keep(drop_key[g], (uint32_t)mykey, a.drop_thr16) ? p * a.drop_inv : 0.f;
            *dst = p;
        }
    }
}

extern "C" int cxr_attn_decode_probs_f32(const void* Q, const void* K, const void* kpm, float* P, long q_bs, long k_bs, long k_rs, long kpm_bs,
                                         long p_bs, long p_hs, long p_ks, int B, int H, int Tk, float scale, int kv_share, int kpm_bits,
                                         float drop_p, const unsigned int* drop_seed, unsigned int drop_site, int drop_t, int row_groups,
                                         hipStream_t stream) {
    if (!Q || !K || !P || B <= 0 || H <= 0 || Tk <= 0 || Tk > 8192) return CXR_ERR_ARG;
    if ((kv_share != 1 && kv_share != 2 && kv_share != 4) || (B % kv_share) || row_groups <= 0 || (B % row_groups)) return CXR_ERR_ARG;
    if (drop_p < 0.f || drop_p >= 1.f || (drop_p > 0.f && !drop_seed)) return CXR_ERR_ARG;
    if ((q_bs % 8) || (k_bs % 8) || (k_rs % 8) || k_rs <= 0 || (((uintptr_t)Q) % 16) || (((uintptr_t)K) % 16) || (((uintptr_t)P) % 4)) return CXR_ERR_ARG;
    if (p_ks <= 0 || p_bs < 0 || p_hs < 0) return CXR_ERR_ARG;
    if (kpm_bits && (!kpm || (kpm_bs % 4) || (((uintptr_t)kpm) % 4))) return CXR_ERR_ARG;
    DecProbArgs a;
    a.Q = (const bf16_t*)Q; a.K = (const bf16_t*)K; a.kpm = (const unsigned char*)kpm; a.P = P; a.drop_seed = drop_seed;
    a.q_bs = q_bs; a.k_bs = k_bs; a.k_rs = k_rs; a.kpm_bs = kpm ? kpm_bs : 0; a.p_bs = p_bs; a.p_hs = p_hs; a.p_ks = p_ks;
    a.B = B; a.Bkv = B / kv_share; a.H = H; a.Tk = Tk; a.groups = row_groups; a.kpm_bits = kpm_bits ? 1 : 0; a.drop_t = drop_t;
    a.qscale = scale * 1.4426950408889634f; a.drop_inv = 1.0f / (1.0f - drop_p); a.drop_site = drop_site;
    a.drop_thr16 = drop_p > 0.f ? dropout_thr16(drop_p) : 0u;
    const dim3 grid(a.Bkv * H);
    // 256 keys per pass cover a KV cache of up to 256 tokens in one pass; the encoder's keys (576 per image) take 1024 per pass
#define DEC_PROBS(G_) do { if (Tk <= 256) CXR_LAUNCH((attn_decode_probs_kernel<G_, 256>), grid, dim3(256), 0, stream, a);     \
                           else CXR_LAUNCH((attn_decode_probs_kernel<G_, 1024>), grid, dim3(1024), 0, stream, a); } while (0)
    if (kv_share == 1) DEC_PROBS(1); else if (kv_share == 2) DEC_PROBS(2); else DEC_PROBS(4);
#undef DEC_PROBS
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}

// one wave per row; lane l reads the 16-byte chunks l, l + 64, ... (8 consecutive columns are contiguous in the decode activation layout)
__global__ __launch_bounds__(256) void dec_hidden_record_kernel(const bf16_t* __restrict__ x, int MT, int M, int K, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps, float* __restrict__ out, long o_rs,
                                                                int groups, int vec) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;                                                     // wave-uniform; no workgroup barrier follows
    const int S = M / groups;
    float* orow = out + (long)((m % S) * groups + m / S) * o_rs;
    const int chunks = K >> 3;
    float mean = 0.f, rstd = 1.f;
    if (gamma != nullptr) {
        float s = 0.f;
        for (int c = lane; c < chunks; c += 64) {
            float f[8];
            unpack8(*reinterpret_cast<const uint4*>(x + dal_off(m, c * 8, MT)), f);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += f[j];
        }
        mean = group_sum<64>(s) / (float)K;
        float v = 0.f;
        for (int c = lane; c < chunks; c += 64) {
            float f[8];
            unpack8(*reinterpret_cast<const uint4*>(x + dal_off(m, c * 8, MT)), f);
#pragma unroll
            for (int j = 0; j < 8; ++j) v += (f[j] - mean) * (f[j] - mean);
        }
        rstd = 1.0f / sqrtf(group_sum<64>(v) / (float)K + eps);
    }
    for (int c = lane; c < chunks; c += 64) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(x + dal_off(m, c * 8, MT)), f);
        if (gamma != nullptr) {
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = (f[j] - mean) * rstd * gamma[c * 8 + j] + beta[c * 8 + j];
        }
        float* dst = orow + c * 8;
        if (vec) {                                                          // 16-byte aligned rows: 32 contiguous bytes per lane
            reinterpret_cast<float4*>(dst)[0] = make_float4(f[0], f[1], f[2], f[3]);
            reinterpret_cast<float4*>(dst)[1] = make_float4(f[4], f[5], f[6], f[7]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) dst[j] = f[j];
        }
    }
}

extern "C" int cxr_dec_hidden_record_f32(const void* x, int x_mt, int M, int K, const float* gamma, const float* beta, float eps, float* out,
                                         long o_rs, int row_groups, hipStream_t stream) {
    if (!x || !out || M <= 0 || K <= 0 || (K % 32) || x_mt <= 0 || M > 16 * x_mt || (((uintptr_t)x) % 16) || (((uintptr_t)out) % 4)) return CXR_ERR_ARG;
    if (o_rs < K || row_groups <= 0 || (M % row_groups) || ((gamma == nullptr) != (beta == nullptr))) return CXR_ERR_ARG;
    const int vec = (((uintptr_t)out) % 16 == 0) && (o_rs % 4 == 0);
    CXR_LAUNCH(dec_hidden_record_kernel, dim3(cdiv(M, 4)), dim3(256), 0, stream, (const bf16_t*)x, x_mt, M, K, gamma, beta, eps, out, o_rs, row_groups, vec);
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}
