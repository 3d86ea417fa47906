// Scan session (cer-mvs_amd/scan.py): what is done once per IMAGE of a scan instead of once per (reference view, source view) pair.
//   * image preparation: the reference driver's scale_operation + crop_operation (utils/data_utils.py:58-78) in one pass over the crop
//     window, uint8 HWC or fp32 CHW in, raw 0..255 fp32 CHW out (what the stem kernel's `raw` path reads);
//   * reference rows: the interior of one bordered block of the feature store, copied into the plain map the cost kernels take as f1s.
// Plain C++, vector stores, no atomics: the same bits on every run.
#include "common.hpp"

// ---- bilinear, align_corners=True, in torch's upsample_bilinear2d arithmetic (as upsample_ac in train_ops.hip): scale =
// (float)(in-1)/(out-1) (0 for out == 1) is computed ONCE, on the host, and handed to the kernel; src = scale * dst is one IEEE product
// (-ffp-contract=off), i0 = (int)src, the +1 neighbour clamped at the last row / column, lambda = src - i0.  Every thread that needs a row
// or column forms it from the same two numbers with the same single operation: which texels are picked is a function of (scale, dst)
// alone, the same on every run and in every launch shape.
static float prep_scale(int in_size, int out_size) { return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.0f; }

struct PrepTap {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ PrepTap prep_tap(float scale, int d, int in_size) {
    const float s = scale * (float)d;
    PrepTap t;
    t.i0 = min((int)s, in_size - 1);                         // (the clamp keeps every read inside the image whatever the product rounds to)
    t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
    t.l1 = s - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

struct PrepArgs {
    const void* src;          // U8: [H0][W0][3] bytes; else [3][H0][W0] floats
    float* dst;               // [3][H][W]
    int H0, W0;               // source image
    int H2, W2;               // size after the resize (int(s * H0), int(s * W0))
    int y0, x0;               // first row / column of the crop window inside the resized image
    int H, W;                 // crop window = output
    int swap;                 // U8 only: output channel c reads byte 2 - c (BGR -> RGB)
    float sy, sx;             // prep_scale(H0, H2), prep_scale(W0, W2)
};

template <bool U8>
__device__ __forceinline__ float prep_load(const PrepArgs& a, int c, int y, int x) {
    if (U8) return (float)reinterpret_cast<const unsigned char*>(a.src)[((long)y * a.W0 + x) * 3 + (a.swap ? 2 - c : c)];
    return reinterpret_cast<const float*>(a.src)[((long)c * a.H0 + y) * a.W0 + x];
}

// one thread: 4 neighbouring output columns of one row, all three channels (a 16-byte store per channel when W % 4 == 0).
// COPY: source and destination sizes are equal - the sample IS the source texel: no interpolation arithmetic, bit-identical.
template <bool U8, bool COPY>
__global__ __launch_bounds__(256) void image_prep_kernel(const PrepArgs a, int groups, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int g = (int)(idx % groups), y = (int)(idx / groups);
    const int xa = 4 * g;
    const bool vec = (a.W & 3) == 0;                         // (then every group is whole and every row start 16-byte aligned)
    PrepTap ty = {0, 0, 1.0f, 0.0f}, tx[4];
    if (!COPY) {
        ty = prep_tap(a.sy, y + a.y0, a.H0);
#pragma unroll
        for (int j = 0; j < 4; ++j) tx[j] = prep_tap(a.sx, min(xa + j, a.W - 1) + a.x0, a.W0);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = min(xa + j, a.W - 1);              // (lanes past the row end recompute the last column and store nothing)
            if (COPY) {
                v[j] = prep_load<U8>(a, c, y + a.y0, x + a.x0);
            } else {
                const float s00 = prep_load<U8>(a, c, ty.i0, tx[j].i0), s01 = prep_load<U8>(a, c, ty.i0, tx[j].i1);
                const float s10 = prep_load<U8>(a, c, ty.i1, tx[j].i0), s11 = prep_load<U8>(a, c, ty.i1, tx[j].i1);
                // torch's upsample_bilinear2d expression, every product and sum rounded on its own (-ffp-contract=off)
                v[j] = ty.l0 * (tx[j].l0 * s00 + tx[j].l1 * s01) + ty.l1 * (tx[j].l0 * s10 + tx[j].l1 * s11);
            }
        }
        float* o = a.dst + ((long)c * a.H + y) * a.W + xa;
        if (vec) {
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (xa + j < a.W) o[j] = v[j];
        }
    }
}

static int prep_launch(bool u8, const void* src, float* dst, int H0, int W0, int H2, int W2, int y0, int x0, int H, int W, int swap,
                       void* stream) {
    if (!src || !dst || H0 <= 0 || W0 <= 0 || H2 <= 0 || W2 <= 0 || H <= 0 || W <= 0) return CER_EINVAL;
    // the crop window lies inside the resized image: with that, every texel the kernel reads lies inside the source image
    if (y0 < 0 || x0 < 0 || (long)y0 + H > H2 || (long)x0 + W > W2) return CER_EINVAL;
    if ((long)H0 * W0 > 0x3fffffffL || (long)H2 * W2 > 0x3fffffffL) return CER_ESHAPE;
    if (!cer_aligned16(dst) && (W & 3) == 0) return CER_EALIGN;
    PrepArgs a = {src, dst, H0, W0, H2, W2, y0, x0, H, W, swap ? 1 : 0, prep_scale(H0, H2), prep_scale(W0, W2)};
    const int groups = (W + 3) / 4;
    const long total = (long)groups * H;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const bool copy = H2 == H0 && W2 == W0;
    hipStream_t st = (hipStream_t)stream;
    if (u8 && copy) hipLaunchKernelGGL((image_prep_kernel<true, true>), grid, block, 0, st, a, groups, total);
    else if (u8) hipLaunchKernelGGL((image_prep_kernel<true, false>), grid, block, 0, st, a, groups, total);
    else if (copy) hipLaunchKernelGGL((image_prep_kernel<false, true>), grid, block, 0, st, a, groups, total);
    else hipLaunchKernelGGL((image_prep_kernel<false, false>), grid, block, 0, st, a, groups, total);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_image_prep_u8(const unsigned char* src, float* dst, int H0, int W0, int H2, int W2, int y0, int x0, int H, int W,
                                 int swap_rb, void* stream) {
    return prep_launch(true, src, dst, H0, W0, H2, W2, y0, x0, H, W, swap_rb, stream);
}

extern "C" int cer_image_prep_f32(const float* src, float* dst, int H0, int W0, int H2, int W2, int y0, int x0, int H, int W,
                                  void* stream) {
    return prep_launch(false, src, dst, H0, W0, H2, W2, y0, x0, H, W, 0, stream);
}

// ---- reference rows: block layout of cer_feat_split_f16 (cost_lines.hip): 8 planes [texels][16 halves].  The bordered block holds
// (h + 2b) x (w + 2b) texels per plane, the plain map h x w; one thread moves 16 bytes (half a texel of one plane).
__global__ __launch_bounds__(256) void feat_ref_rows_kernel(const uint4* __restrict__ slot, uint4* __restrict__ out, int h, int w, int border,
                                                            long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long P = (long)h * w, wb = w + 2 * border, Pb = (h + 2 * border) * wb;
    const int q = (int)(idx & 1);
    const long e = idx >> 1, p = e / P, t = e - p * P;
    const long y = t / w, x = t - y * w;
    out[idx] = slot[((p * Pb + (y + border) * wb + x + border) << 1) + q];
}

extern "C" int cer_feat_ref_rows_f16(const void* slot, void* out, int h, int w, int border, void* stream) {
    if (!slot || !out || h <= 0 || w <= 0 || border < 0) return CER_EINVAL;
    if (!cer_aligned16(slot) || !cer_aligned16(out)) return CER_EALIGN;
    const long total = (long)h * w * 16;                     // 8 planes x 2 halves of a 32-byte texel
    if ((total + 255) / 256 > 0x7fffffffL) return CER_ESHAPE;
    hipLaunchKernelGGL(feat_ref_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(slot), reinterpret_cast<uint4*>(out), h, w, border, total);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}
