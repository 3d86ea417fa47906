// Training-mode hot path outside the convolutions (cer_mvs_amd/train.py): the train-branch correlation lookup (reference:
// CorrBlock.__call__ core/corr.py:102-143 with test_mode=False, pyramid core/corr.py:94-97, bilinear_sampler1
// utils/bilinear_sampler.py:6-25) and the bilinear upsample of the loss (loss.py:18-19, F.interpolate(align_corners=True)),
// each with its adjoint.  fp32, every output written whole, no atomics: the same bits on every run.
//
// Lookup.  The volume is DirectCorr's output as it lies in memory, [V, D, P] (D-major).  A block takes 64 pixels of one view:
// 256 threads load the block's 64 x D slice with lanes along pixels (256-byte coalesced rows), into one LDS row per pixel that
// also holds the pooled levels [level0 | level1 | ...] (formed in LDS, never written to HBM).  Rows are private to a pixel, so the
// adjoint needs no atomics: the taps of a (view, pixel, level) are accumulated by ONE thread, in tap order, into the level's
// segment of the row; the pooling adjoint then folds the levels into level 0 in a fixed order and writes D-major.
#include "common.hpp"

#define TL_PIX 64          // pixels per block
#define TL_MAX_D 128       // hypotheses per row (LDS: 64 rows of < 2 D floats, < 64 KiB)
#define TL_MAX_LEVELS 4
#define TL_MAX_TAPS 64     // L * (2r + 1)

struct TlRows {
    int off[TL_MAX_LEVELS];
    int len[TL_MAX_LEVELS];
    int pitch;             // floats per LDS row: odd, so that 64 lanes on 64 rows at one column hit 32 different banks (ds_*_b32)
};

static TlRows tl_rows(int D, int L) {
    TlRows t = {};
    int n = 0;
    for (int l = 0; l < L; ++l) {
        t.len[l] = D >> l;                                   // F.avg_pool2d([1,2]) level by level: floor halving
        t.off[l] = n;
        n += t.len[l];
    }
    t.pitch = n | 1;
    return t;
}

// core/corr.py:107: max((disp - origin) / incre + D//2, 0) - true division, then the add, then the lower clamp
__device__ __forceinline__ float tl_coord(float disp, float origin, float incre, int D) {
    return fmaxf(__fadd_rn(__fdiv_rn(__fsub_rn(disp, origin), incre), (float)(D / 2)), 0.0f);
}

// stage the block's 64 x D slice of the volume into the rows and form the pooled levels: (a + b) * 0.5 level by level, the
// association of lookup.hip's lk_elem (bit-identical to F.avg_pool2d and to the inference path's pooled levels)
__device__ __forceinline__ void tl_stage(const float* __restrict__ src, long P, int D, int L, const TlRows& tr, float* __restrict__ smem,
                                         int npix) {
    const int pix = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* row = smem + pix * tr.pitch;
    if (pix < npix)
        for (int d = wv; d < D; d += 4) row[d] = src[(long)d * P + pix];
    for (int l = 1; l < L; ++l) {
        __syncthreads();
        if (pix < npix) {
            const float* a = row + tr.off[l - 1];
            float* b = row + tr.off[l];
            for (int i = wv; i < tr.len[l]; i += 4) b[i] = (a[2 * i] + a[2 * i + 1]) * 0.5f;
        }
    }
    __syncthreads();
}

// out [V, L*(2r+1), P]: tap k = l*(2r+1) + (t+r) samples level l at x = t + c / 2^l (torch's rounding: the tap is added to the scaled
// coordinate), bilinear between floor(x) and floor(x)+1, zero outside [0, len_l - 1] (grid_sample, zeros padding, align_corners)
__global__ __launch_bounds__(256) void train_lookup_fwd_kernel(const float* __restrict__ corr, const float* __restrict__ origin,
                                                               const float* __restrict__ disp, float* __restrict__ out, long P, int D,
                                                               float incre, int L, int r, TlRows tr) {
    extern __shared__ float tl_smem[];
    const int v = blockIdx.y;
    const long p0 = (long)blockIdx.x * TL_PIX;
    const int npix = (int)min((long)TL_PIX, P - p0);
    tl_stage(corr + (long)v * D * P + p0, P, D, L, tr, tl_smem, npix);
    const int pix = threadIdx.x & 63;
    if (pix >= npix) return;                                 // (no barrier follows)
    const long p = p0 + pix;
    const float* row = tl_smem + pix * tr.pitch;
    const float c = tl_coord(disp[p], origin[p], incre, D);
    const int taps = 2 * r + 1, K = L * taps;
    for (int k = threadIdx.x >> 6; k < K; k += 4) {
        const int lv = k / taps;
        const float x = (float)(k - lv * taps - r) + c / (float)(1 << lv);
        const float fx = floorf(x);
        const int len = tr.len[lv];
        float val = 0.f;
        if (fx >= -1.0f && fx <= (float)(len - 1)) {         // else both texels are outside (NaN too)
            const int i0 = (int)fx;
            const float w = x - fx;
            const float* lvl = row + tr.off[lv];
            const float a = i0 >= 0 ? lvl[i0] : 0.f;
            const float b = i0 + 1 < len ? lvl[i0 + 1] : 0.f;
            val = a * (1.0f - w) + b * w;
        }
        out[((long)v * K + k) * P + p] = val;
    }
}

// grad_corr [V, D, P] from grad_out [V, L*(2r+1), P]: wave w accumulates the taps of levels w, w+4, ... of its lane's pixel into the
// level's segment of the pixel's row (tap order); behind one barrier level 0 gets  g0 + g1[d/2] * 0.5 + g2[d/4] * 0.25 + ...
__global__ __launch_bounds__(256) void train_lookup_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ origin,
                                                               const float* __restrict__ disp, float* __restrict__ gcorr, long P, int D,
                                                               float incre, int L, int r, TlRows tr) {
    extern __shared__ float tl_smem[];
    const int v = blockIdx.y;
    const long p0 = (long)blockIdx.x * TL_PIX;
    const int npix = (int)min((long)TL_PIX, P - p0);
    const int pix = threadIdx.x & 63;
    const long p = p0 + pix;
    float* row = tl_smem + pix * tr.pitch;
    const int taps = 2 * r + 1, K = L * taps;
    if (pix < npix) {
        const float c = tl_coord(disp[p], origin[p], incre, D);
        for (int lv = threadIdx.x >> 6; lv < L; lv += 4) {
            float* acc = row + tr.off[lv];
            const int len = tr.len[lv];
            for (int i = 0; i < len; ++i) acc[i] = 0.f;
            const float cl = c / (float)(1 << lv);
            const float* g = gout + ((long)v * K + (long)lv * taps) * P + p;
            for (int j = 0; j < taps; ++j) {
                const float x = (float)(j - r) + cl;
                const float fx = floorf(x);
                if (fx >= -1.0f && fx <= (float)(len - 1)) {
                    const int i0 = (int)fx;
                    const float w = x - fx;
                    const float gj = g[(long)j * P];
                    if (i0 >= 0) acc[i0] += gj * (1.0f - w);
                    if (i0 + 1 < len) acc[i0 + 1] += gj * w;
                }
            }
        }
    }
    __syncthreads();
    if (pix >= npix) return;
    for (int d = threadIdx.x >> 6; d < D; d += 4) {
        float s = row[d];
        float scale = 0.5f;
        for (int lv = 1; lv < L; ++lv, scale *= 0.5f) {
            const int i = d >> lv;
            if (i < tr.len[lv]) s += row[tr.off[lv] + i] * scale;
        }
        gcorr[((long)v * D + d) * P + p] = s;
    }
}

static int tl_check(const void* a, const void* b, const void* c, const void* o, int V, long P, int D, float incre, int L, int r) {
    if (!a || !b || !c || !o || V <= 0 || P <= 0 || D <= 0 || L <= 0 || r < 0 || !(incre > 0.0f)) return CER_EINVAL;
    if (L > TL_MAX_LEVELS || D > TL_MAX_D || (D >> (L - 1)) < 2 || L * (2 * r + 1) > TL_MAX_TAPS) return CER_ESHAPE;
    if ((P + TL_PIX - 1) / TL_PIX > 0x7fffffffL || V > 65535) return CER_ESHAPE;
    return CER_OK;
}

extern "C" int cer_train_lookup_fwd_f32(const float* corr, const float* origin, const float* disp, float* out, int V, long P, int D,
                                        float incre, int num_levels, int radius, void* stream) {
    const int rc = tl_check(corr, origin, disp, out, V, P, D, incre, num_levels, radius);
    if (rc != CER_OK) return rc;
    const TlRows tr = tl_rows(D, num_levels);
    const dim3 grid((unsigned)((P + TL_PIX - 1) / TL_PIX), (unsigned)V);
    hipLaunchKernelGGL(train_lookup_fwd_kernel, grid, dim3(256), (size_t)TL_PIX * tr.pitch * sizeof(float), (hipStream_t)stream, corr,
                       origin, disp, out, P, D, incre, num_levels, radius, tr);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_train_lookup_bwd_f32(const float* grad_out, const float* origin, const float* disp, float* grad_corr, int V, long P,
                                        int D, float incre, int num_levels, int radius, void* stream) {
    const int rc = tl_check(grad_out, origin, disp, grad_corr, V, P, D, incre, num_levels, radius);
    if (rc != CER_OK) return rc;
    const TlRows tr = tl_rows(D, num_levels);
    const dim3 grid((unsigned)((P + TL_PIX - 1) / TL_PIX), (unsigned)V);
    hipLaunchKernelGGL(train_lookup_bwd_kernel, grid, dim3(256), (size_t)TL_PIX * tr.pitch * sizeof(float), (hipStream_t)stream, grad_out,
                       origin, disp, grad_corr, P, D, incre, num_levels, radius, tr);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

// ---- bilinear upsample, align_corners=True (torch's upsample_bilinear2d): scale = (float)(in-1)/(out-1) (0 for out == 1),
// src = scale * dst, i0 = (int)src, the +1 neighbour clamped at the last row / column, lambda = src - i0.  The host computes the scale
// once and hands it to the kernels, so the host range table below and the kernels see the same source indices.
static float up_scale(int in_size, int out_size) { return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.0f; }

struct UpTap {
    int i0, i1;            // the two source texels (i1 == i0 at the last one)
    float l0, l1;          // their weights 1 - lambda, lambda
};

__host__ __device__ __forceinline__ UpTap up_tap(float scale, int dst, int in_size) {
    const float s = scale * (float)dst;
    UpTap t;
    t.i0 = min((int)s, in_size - 1);                         // (never binds: scale * (out-1) rounds to at most in-1 + an ulp)
    t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
    t.l1 = s - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

__global__ __launch_bounds__(256) void upsample_ac_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, long total, int h,
                                                              int w, int H, int W, float sy, float sx) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int X = (int)(idx % W);
    const long q = idx / W;
    const int Y = (int)(q % H);
    const long b = q / H;
    const UpTap ty = up_tap(sy, Y, h), tx = up_tap(sx, X, w);
    const float* s0 = in + (b * h + ty.i0) * w;
    const float* s1 = in + (b * h + ty.i1) * w;
    out[idx] = ty.l0 * (tx.l0 * s0[tx.i0] + tx.l1 * s0[tx.i1]) + ty.l1 * (tx.l0 * s1[tx.i0] + tx.l1 * s1[tx.i1]);
}

// adjoint, gather form, pass x: work[b, Y, j] = sum over the output columns X in range_x[j] (ascending) of the weight of j in X's footprint
// times grad_out[b, Y, X]
__global__ __launch_bounds__(256) void upsample_ac_bwd_x_kernel(const float* __restrict__ gout, float* __restrict__ work,
                                                                const int* __restrict__ range_x, long total, int w, int W, float sx) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % w);
    const long row = idx / w;                                // b * H + Y
    const float* g = gout + row * W;
    const int lo = max(range_x[2 * j], 0), hi = min(range_x[2 * j + 1], W);
    float acc = 0.f;
    for (int X = lo; X < hi; ++X) {
        const UpTap t = up_tap(sx, X, w);
        const float gx = g[X];
        if (t.i0 == j) acc += t.l0 * gx;
        if (t.i1 == j) acc += t.l1 * gx;
    }
    work[idx] = acc;
}

// pass y: grad_in[b, i, j] = sum over the output rows Y in range_y[i] (ascending) of the weight of i in Y's footprint times work[b, Y, j]
__global__ __launch_bounds__(256) void upsample_ac_bwd_y_kernel(const float* __restrict__ work, float* __restrict__ gin,
                                                                const int* __restrict__ range_y, long total, int h, int w, int H, float sy) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % w);
    const long q = idx / w;
    const int i = (int)(q % h);
    const long b = q / h;
    const float* src = work + b * H * (long)w + j;
    const int lo = max(range_y[2 * i], 0), hi = min(range_y[2 * i + 1], H);
    float acc = 0.f;
    for (int Y = lo; Y < hi; ++Y) {
        const UpTap t = up_tap(sy, Y, h);
        const float gy = src[(long)Y * w];
        if (t.i0 == i) acc += t.l0 * gy;
        if (t.i1 == i) acc += t.l1 * gy;
    }
    gin[idx] = acc;
}

extern "C" int cer_upsample_ac_ranges(int in_size, int out_size, int* range) {
    if (!range || in_size <= 0 || out_size <= 0) return CER_EINVAL;
    const float s = up_scale(in_size, out_size);
    for (int j = 0; j < in_size; ++j) {
        range[2 * j] = out_size;
        range[2 * j + 1] = 0;
    }
    for (int X = 0; X < out_size; ++X) {                     // i0 and i1 are non-decreasing in X: each texel's set of X is one range
        const UpTap t = up_tap(s, X, in_size);
        for (int k = 0; k < 2; ++k) {
            const int j = k ? t.i1 : t.i0;
            range[2 * j] = min(range[2 * j], X);
            range[2 * j + 1] = max(range[2 * j + 1], X + 1);
        }
    }
    for (int j = 0; j < in_size; ++j)
        if (range[2 * j] >= range[2 * j + 1]) range[2 * j] = range[2 * j + 1] = 0;      // texel in no footprint: empty range
    return CER_OK;
}

static int up_check(const void* a, const void* b, int n, int h, int w, int H, int W) {
    if (!a || !b || n <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return CER_EINVAL;
    const long total = (long)n * H * W;
    if ((total + 255) / 256 > 0x7fffffffL) return CER_ESHAPE;
    return CER_OK;
}

extern "C" int cer_upsample_bilinear_ac_f32(const float* in, float* out, int n, int h, int w, int H, int W, void* stream) {
    const int rc = up_check(in, out, n, h, w, H, W);
    if (rc != CER_OK) return rc;
    const long total = (long)n * H * W;
    hipLaunchKernelGGL(upsample_ac_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, total, h,
                       w, H, W, up_scale(h, H), up_scale(w, W));
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_upsample_bilinear_ac_bwd_f32(const float* grad_out, float* grad_in, float* work, const int* range_y, const int* range_x,
                                                int n, int h, int w, int H, int W, void* stream) {
    int rc = up_check(grad_out, grad_in, n, h, w, H, W);
    if (rc != CER_OK) return rc;
    if (!work || !range_y || !range_x) return CER_EINVAL;
    const long tx = (long)n * H * w, ty = (long)n * h * w;
    hipLaunchKernelGGL(upsample_ac_bwd_x_kernel, dim3((unsigned)((tx + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_out, work,
                       range_x, tx, w, W, up_scale(w, W));
    CER_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(upsample_ac_bwd_y_kernel, dim3((unsigned)((ty + 255) / 256)), dim3(256), 0, (hipStream_t)stream, work, grad_in,
                       range_y, ty, h, w, H, up_scale(h, H));
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}
