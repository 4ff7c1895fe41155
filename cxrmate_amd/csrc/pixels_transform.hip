// Image transforms of the reference's input pipeline on the device (modules/lightning_modules/single.py:229-262 + collate_fn of multi.py:155-164):
// Resize(S) as Pillow's antialiased bilinear resize executes it (a horizontal 8-bit pass, then a vertical one, 22-bit integer weights),
// CenterCrop / RandomCrop, RandomRotation (nearest neighbour, 16.16 fixed point), ToTensor + Normalize and pad_sequence, from the decoded
// full-size uint8 images. Everything up to the final normalise is integer arithmetic: the host builds the weight tables in double in Pillow's
// operation order (cxrmate_amd/pixels.py; this library is built with -ffp-contract=fast, so no double arithmetic happens here) and the kernels
// reproduce Pillow byte for byte.
//
// Two launches per call, whatever the number of images:
//   1. image_resize_h_kernel   one workgroup per band of source rows of one image (band table from the host). The band is contiguous in the packed
//                              source (row pitch padded to 16 B), so it is staged in LDS with 16-byte loads, each source byte fetched from HBM
//                              once; taps come from LDS; the uint8 intermediate [H, ow, C] goes to the workspace.
//   2. image_finish_kernel     one thread per output pixel of every [b, n] slot: the rotation's source pixel (identity in test mode), the crop
//                              offset, the vertical taps from the intermediate, normalise, fp32 NCHW and / or uint8 HWC; absent images = 0.0.
// An axis that needs no resampling goes through its table as well: the table of an (n -> n) pass is the single weight 2^22, which is a copy.
//
// Nothing a descriptor or table says is trusted with an address: a descriptor that does not fit its buffers disables its image (NaN / 0 output),
// and every tap range is clamped to its row.
#include "common.h"
#include "../../include/cxrmate_hip.h"

#define IT_DESC_INTS CXR_IMAGE_TRANSFORM_DESC_INTS       // int32 per image, see include/cxrmate_hip.h
#define IT_BAND_BYTES CXR_IMAGE_TRANSFORM_BAND_BYTES     // LDS per workgroup of the horizontal pass; a source row (pitch) must fit
#define IT_ROWS_PER_THREAD 8
#define IT_PREC 22

enum { D_SRC = 0, D_H, D_W, D_C, D_PITCH, D_OH, D_OW, D_TOP, D_LEFT, D_HTAB, D_HK, D_VTAB, D_VK, D_WS, D_A0 = 16 };

struct ItBuffers {
    long src_bytes, tab_ints, inter_bytes;
    int n_images, S;
};

// wave-uniform: does image `i`'s descriptor stay inside the buffers of this call?
__device__ __forceinline__ bool it_desc_ok(const int* __restrict__ d, const ItBuffers& bf) {
    const long H = d[D_H], W = d[D_W], C = d[D_C], pitch = d[D_PITCH], oh = d[D_OH], ow = d[D_OW], hk = d[D_HK], vk = d[D_VK];
    if (H <= 0 || W <= 0 || (C != 1 && C != 3) || pitch < W * C || (pitch & 15) || pitch > IT_BAND_BYTES) return false;
    if (oh < bf.S || ow < bf.S || hk <= 0 || vk <= 0 || d[D_TOP] < 0 || d[D_LEFT] < 0 || d[D_TOP] + bf.S > oh || d[D_LEFT] + bf.S > ow) return false;
    const long src = (long)d[D_SRC] * 16, ws = (long)d[D_WS] * 16, ht = d[D_HTAB], vt = d[D_VTAB];
    if (src < 0 || src + H * pitch > bf.src_bytes || ws < 0 || ws + H * ow * C > bf.inter_bytes) return false;
    if (ht < 0 || ht + ow * (2 + hk) > bf.tab_ints || vt < 0 || vt + oh * (2 + vk) > bf.tab_ints) return false;
    return true;
}

__device__ __forceinline__ unsigned char it_clip8(int acc) {
    const int v = acc >> IT_PREC;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- horizontal pass. Table of an axis at `tab`: bounds int32 [out][2] = (first tap, taps), then weights int32 [ksize][out] (tap-major: the
// lanes of a wave take neighbouring outputs, so a tap's weights are one coalesced read).
__global__ __launch_bounds__(256) void image_resize_h_kernel(const unsigned char* __restrict__ src, const int* __restrict__ desc,
                                                             const int* __restrict__ bands /*[n_bands][2] = (image, first row)*/,
                                                             const int* __restrict__ tables, unsigned char* __restrict__ inter, ItBuffers bf) {
    __shared__ __attribute__((aligned(16))) unsigned char band[IT_BAND_BYTES];
    const int img = bands[2 * blockIdx.x], row0 = bands[2 * blockIdx.x + 1];
    if (img < 0 || img >= bf.n_images) return;
    const int* d = desc + (long)img * IT_DESC_INTS;
    if (!it_desc_ok(d, bf)) return;
    const int H = d[D_H], W = d[D_W], C = d[D_C], pitch = d[D_PITCH], ow = d[D_OW], hk = d[D_HK];
    if (row0 < 0 || row0 >= H) return;
    int rows = IT_BAND_BYTES / pitch;
    rows = rows < H - row0 ? rows : H - row0;

    const unsigned char* g = src + (long)d[D_SRC] * 16 + (long)row0 * pitch;
    const int chunks = rows * (pitch >> 4);
    for (int i = threadIdx.x; i < chunks; i += 256) reinterpret_cast<uint4*>(band)[i] = ld_stream16(g + (long)i * 16);
    __syncthreads();

    const int* bounds = tables + d[D_HTAB];
    const int* wts = bounds + 2 * ow;
    unsigned char* o = inter + (long)d[D_WS] * 16 + (long)row0 * ow * C;
    const int owc = ow * C, groups = (rows + IT_ROWS_PER_THREAD - 1) / IT_ROWS_PER_THREAD;
    for (int item = threadIdx.x; item < owc * groups; item += 256) {
        const int grp = item / owc, xc = item - grp * owc;                    // xc = xo * C + c: neighbouring lanes write neighbouring bytes
        const int xo = xc / C, c = xc - xo * C;
        int xmin = bounds[2 * xo], n = bounds[2 * xo + 1];
        xmin = xmin < 0 ? 0 : (xmin > W ? W : xmin);
        n = n < 0 ? 0 : n;
        n = n > hk ? hk : n;
        n = n > W - xmin ? W - xmin : n;
        const int r0 = grp * IT_ROWS_PER_THREAD;
        const int nr = rows - r0 < IT_ROWS_PER_THREAD ? rows - r0 : IT_ROWS_PER_THREAD;
        int acc[IT_ROWS_PER_THREAD];
#pragma unroll
        for (int r = 0; r < IT_ROWS_PER_THREAD; ++r) acc[r] = 1 << (IT_PREC - 1);
        const unsigned char* p = band + r0 * pitch + xmin * C + c;
        for (int t = 0; t < n; ++t) {
            const int w = wts[(long)t * ow + xo];
#pragma unroll
            for (int r = 0; r < IT_ROWS_PER_THREAD; ++r)
                if (r < nr) acc[r] += (int)p[r * pitch + t * C] * w;
        }
#pragma unroll
        for (int r = 0; r < IT_ROWS_PER_THREAD; ++r)
            if (r < nr) o[(long)(r0 + r) * owc + xc] = it_clip8(acc[r]);
    }
}

// ---- vertical pass + crop + rotation + normalise + pad
__global__ __launch_bounds__(256) void image_finish_kernel(const unsigned char* __restrict__ inter, const int* __restrict__ desc,
                                                           const int* __restrict__ slot_image /*[B*Nmax]: image or -1*/,
                                                           const int* __restrict__ tables, float* __restrict__ out_f32,
                                                           unsigned char* __restrict__ out_u8, int n_slots, ItBuffers bf, float3 scale, float3 shift) {
    const int S = bf.S;
    const long ss = (long)S * S, total = ss * n_slots;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int slot = (int)(idx / ss);
        const int pix = (int)(idx - slot * ss), y = pix / S, x = pix - y * S;
        float* of = out_f32 ? out_f32 + (long)slot * 3 * ss + pix : nullptr;
        const int img = slot_image[slot];
        if (img < 0) {                                                        // pad_sequence slot: exactly 0.0 (quirk Q3)
            if (of) { of[0] = 0.f; of[ss] = 0.f; of[2 * ss] = 0.f; }
            continue;
        }
        const int* d = desc + (long)img * IT_DESC_INTS;
        unsigned char* ou = out_u8 ? out_u8 + ((long)img * ss + pix) * 3 : nullptr;
        if (img >= bf.n_images || !it_desc_ok(d, bf)) {
            const float nan = __uint_as_float(0x7fc00000u);
            if (of) { of[0] = nan; of[ss] = nan; of[2 * ss] = nan; }
            if (ou && img < bf.n_images) { ou[0] = 0; ou[1] = 0; ou[2] = 0; }
            continue;
        }
        // Pillow's affine_fixed (nearest): 16.16 fixed point, arithmetic shifts
        const long xin = ((long)d[D_A0 + 2] + (long)d[D_A0 + 1] * y + (long)d[D_A0 + 0] * x) >> 16;
        const long yin = ((long)d[D_A0 + 5] + (long)d[D_A0 + 4] * y + (long)d[D_A0 + 3] * x) >> 16;
        int u[3] = {0, 0, 0};                                                 // the rotation's fill colour
        if (xin >= 0 && xin < S && yin >= 0 && yin < S) {
            const int H = d[D_H], C = d[D_C], oh = d[D_OH], ow = d[D_OW], vk = d[D_VK];
            const int row = d[D_TOP] + (int)yin, col = d[D_LEFT] + (int)xin;
            const int* bounds = tables + d[D_VTAB];
            const int* wts = bounds + 2 * oh;
            int ymin = bounds[2 * row], n = bounds[2 * row + 1];
            ymin = ymin < 0 ? 0 : (ymin > H ? H : ymin);
            n = n < 0 ? 0 : n;
            n = n > vk ? vk : n;
            n = n > H - ymin ? H - ymin : n;
            const long owc = (long)ow * C;
            const unsigned char* p = inter + (long)d[D_WS] * 16 + ymin * owc + (long)col * C;
            if (C == 1) {
                int acc = 1 << (IT_PREC - 1);
                for (int t = 0; t < n; ++t) acc += (int)p[t * owc] * wts[(long)t * oh + row];
                u[0] = u[1] = u[2] = it_clip8(acc);
            } else {
                int a0 = 1 << (IT_PREC - 1), a1 = a0, a2 = a0;
                for (int t = 0; t < n; ++t) {
                    const int w = wts[(long)t * oh + row];
                    a0 += (int)p[t * owc] * w; a1 += (int)p[t * owc + 1] * w; a2 += (int)p[t * owc + 2] * w;
                }
                u[0] = it_clip8(a0); u[1] = it_clip8(a1); u[2] = it_clip8(a2);
            }
        }
        if (of) { of[0] = u[0] * scale.x + shift.x; of[ss] = u[1] * scale.y + shift.y; of[2 * ss] = u[2] * scale.z + shift.z; }
        if (ou) { ou[0] = (unsigned char)u[0]; ou[1] = (unsigned char)u[1]; ou[2] = (unsigned char)u[2]; }
    }
}

extern "C" int cxr_image_transform(const void* src, long src_bytes, const int* desc, int n_images, int n_bands, const int* tables, long n_table_ints,
                                   int B, int Nmax, int S, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                                   float* out_f32, void* out_u8, void* workspace, long workspace_bytes, long inter_bytes, hipStream_t stream) {
    if (!src || !desc || !tables || !workspace || (!out_f32 && !out_u8)) return CXR_ERR_ARG;
    if (n_images <= 0 || n_bands <= 0 || B <= 0 || Nmax <= 0 || S <= 0 || S > 16384 || (long)B * Nmax < n_images) return CXR_ERR_ARG;
    if (src_bytes <= 0 || n_table_ints <= 0 || inter_bytes <= 0 || workspace_bytes < inter_bytes) return CXR_ERR_ARG;
    if (std0 == 0.f || std1 == 0.f || std2 == 0.f) return CXR_ERR_ARG;
    if (((uintptr_t)src & 15) || ((uintptr_t)workspace & 15)) return CXR_ERR_ARG;
    ItBuffers bf;
    bf.src_bytes = src_bytes; bf.tab_ints = n_table_ints; bf.inter_bytes = inter_bytes; bf.n_images = n_images; bf.S = S;
    // (u/255 - mean)/std = u * (1/(255 std)) - mean/std, as cxr_pixels_u8_to_f32
    const float3 scale = make_float3(1.0f / (255.0f * std0), 1.0f / (255.0f * std1), 1.0f / (255.0f * std2));
    const float3 shift = make_float3(-mean0 / std0, -mean1 / std1, -mean2 / std2);
    const int* slot_image = desc + (long)n_images * IT_DESC_INTS;
    const int* bands = slot_image + (long)B * Nmax;
    CXR_LAUNCH(image_resize_h_kernel, dim3((unsigned)n_bands), dim3(256), 0, stream, (const unsigned char*)src, desc, bands, tables,
               (unsigned char*)workspace, bf);
    CXR_LAUNCH_CHECK();
    const long total = (long)B * Nmax * S * S;
    CXR_LAUNCH(image_finish_kernel, dim3((unsigned)(cdiv(total, 256) < 65536 ? cdiv(total, 256) : 65536)), dim3(256), 0, stream,
               (const unsigned char*)workspace, desc, slot_image, tables, out_f32, (unsigned char*)out_u8, B * Nmax, bf, scale, shift);
    CXR_LAUNCH_CHECK();
    return CXR_OK;
}
