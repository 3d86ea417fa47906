// Point cloud of a fused scan on the device (cer-mvs_amd/fusion.py point_cloud / color_grid, scan.py reconstruct_scan): what fusion() does on
// the host after the vote loop (reference: fusion.py:262-279) - the masked pixels of every listed view back-projected to world points and
// paired with their colours - plus the two small producers in front of it: disparity -> depth and the colour planes at the depth grid.
//
// Order: the points of view order[0] first, then order[1], ...; row-major inside a view - what numpy's boolean indexing gives the host path.
// It is a pure function of the masks: compact.hpp's count / scan / emit over the set pixels, one tile of a view per block.  No atomics, no
// output cursor: the same bytes on every run, whatever the schedule.
#include "common.hpp"
#include "compact.hpp"

#define CLOUD_TILE CER_CLOUD_TILE                    // pixels of one view per block
#define CLOUD_ORDER_CHUNK 128                        // listed views per launch (they travel as kernel arguments: the list is host memory)

struct CloudOrder {
    int view[CLOUD_ORDER_CHUNK];
};

// the predicate of both passes over view m: pixel p is set
__device__ __forceinline__ auto cloud_set(const unsigned char* __restrict__ m, unsigned P) {
    return [=](unsigned p) { return p < P && m[p] != 0; };
}

// ---- count: partials[(k0 + blockIdx.y) * bpv + blockIdx.x] = set pixels of the block's tile
__global__ __launch_bounds__(256) void cloud_count_kernel(const CloudOrder ord, int k0, const unsigned char* __restrict__ masks, unsigned P,
                                                          int bpv, unsigned* __restrict__ partials) {
    compact_count<CLOUD_TILE>(compact_seg<CLOUD_TILE, unsigned>(), cloud_set(masks + (long)ord.view[blockIdx.y] * P, P), partials,
                              (long)(k0 + blockIdx.y) * bpv + blockIdx.x);
}

// ---- scan: one block; offsets[i] = sum of partials[0 .. i), offsets[n] = the total; view_base[k] = offsets[k * bpv] (k <= views)
__global__ __launch_bounds__(1024) void cloud_scan_kernel(const unsigned* __restrict__ partials, long n, int bpv, int views,
                                                          long long* __restrict__ offsets, long long* __restrict__ view_base) {
    compact_scan(partials, n, offsets);
    __syncthreads();                                 // the block's own global writes are visible to it behind the barrier
    for (int k = threadIdx.x; k <= views; k += 1024) view_base[k] = offsets[(long)k * bpv];
}

// ---- emit.  cams: per view CER_CLOUD_CAM_DOUBLES doubles = K^-1 [9] | rows 0-2 of E^-1 [12] (float32 inverses promoted on the host).
// The coordinate arithmetic is backproject()'s, in fp64: K^-1 (x d, y d, d), then E^-1 (., 1), rounded ONCE to float32.
__global__ __launch_bounds__(256) void cloud_emit_kernel(const CloudOrder ord, int k0, const unsigned char* __restrict__ masks,
                                                         const float* __restrict__ depth, const double* __restrict__ cams,
                                                         const float* __restrict__ colors, unsigned P, int w, int bpv,
                                                         const long long* __restrict__ offsets, long long capacity, float* __restrict__ xyz,
                                                         unsigned char* __restrict__ rgb) {
    const int view = ord.view[blockIdx.y];
    const double* c = cams + (long)view * CER_CLOUD_CAM_DOUBLES;         // wave-uniform: scalar loads
    const float* dep = depth + (long)view * P;
    const float* col = colors + (long)view * 3 * P;
    compact_emit<CLOUD_TILE>(compact_seg<CLOUD_TILE, unsigned>(), cloud_set(masks + (long)view * P, P), offsets,
                             (long)(k0 + blockIdx.y) * bpv + blockIdx.x, [&](unsigned p, long long idx) {
        if (idx >= capacity) return;                                     // (never past what the caller allocated)
        const unsigned yi = p / (unsigned)w, xi = p - yi * (unsigned)w;
        const double d = (double)dep[p];
        const double vx = (double)xi * d, vy = (double)yi * d;           // exact: an integer times a float32 in fp64
        const double cx = fma(c[2], d, fma(c[1], vy, c[0] * vx));
        const double cy = fma(c[5], d, fma(c[4], vy, c[3] * vx));
        const double cz = fma(c[8], d, fma(c[7], vy, c[6] * vx));
        const double X = fma(c[11], cz, fma(c[10], cy, c[9] * cx)) + c[12];
        const double Y = fma(c[15], cz, fma(c[14], cy, c[13] * cx)) + c[16];
        const double Z = fma(c[19], cz, fma(c[18], cy, c[17] * cx)) + c[20];
        float* o = xyz + idx * 3;
        o[0] = (float)X;
        o[1] = (float)Y;
        o[2] = (float)Z;
        unsigned char* q = rgb + idx * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) q[ch] = (unsigned char)(int)(col[(long)ch * P + p] * 255.0f);     // fusion(): (img * 255).astype(uint8)
    });
}

static int cloud_check(const void* masks, int N, int h, int w, const int* order, int n_order) {
    if (!masks || !order || N <= 0 || h <= 0 || w <= 0 || n_order <= 0) return CER_EINVAL;
    if ((long)h * w > 0x7fffffffL - CLOUD_TILE) return CER_ESHAPE;
    for (int k = 0; k < n_order; ++k)
        if (order[k] < 0 || order[k] >= N) return CER_EINVAL;
    return CER_OK;
}

static long cloud_bpv(int h, int w) { return ((long)h * w + CLOUD_TILE - 1) / CLOUD_TILE; }          // blocks (tiles) per view

// launch(ord, k0, nk) for every chunk of CLOUD_ORDER_CHUNK listed views: ord = order[k0 .. k0 + nk)
template <typename Launch>
static int cloud_for_chunks(const int* order, int n_order, Launch launch) {
    for (int k0 = 0; k0 < n_order; k0 += CLOUD_ORDER_CHUNK) {
        CloudOrder ord = {};
        const int nk = n_order - k0 < CLOUD_ORDER_CHUNK ? n_order - k0 : CLOUD_ORDER_CHUNK;
        for (int k = 0; k < nk; ++k) ord.view[k] = order[k0 + k];
        launch(ord, k0, nk);
        CER_RETURN_IF_LAUNCH_FAILED();
    }
    return CER_OK;
}

extern "C" long cer_cloud_partials(int n_order, int h, int w) {
    if (n_order <= 0 || h <= 0 || w <= 0) return CER_EINVAL;
    return (long)n_order * cloud_bpv(h, w);
}

extern "C" int cer_cloud_count_u8(const unsigned char* masks, int N, int h, int w, const int* order, int n_order, unsigned int* partials,
                                  long long* offsets, long long* view_base, void* stream) {
    int rc = cloud_check(masks, N, h, w, order, n_order);
    if (rc != CER_OK) return rc;
    if (!partials || !offsets || !view_base) return CER_EINVAL;
    const unsigned P = (unsigned)((long)h * w);
    const int bpv = (int)cloud_bpv(h, w);
    hipStream_t st = (hipStream_t)stream;
    rc = cloud_for_chunks(order, n_order, [&](const CloudOrder& ord, int k0, int nk) {
        hipLaunchKernelGGL(cloud_count_kernel, dim3((unsigned)bpv, (unsigned)nk), dim3(256), 0, st, ord, k0, masks, P, bpv, partials);
    });
    if (rc != CER_OK) return rc;
    hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(1024), 0, st, partials, (long)n_order * bpv, bpv, n_order, offsets, view_base);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_cloud_emit_f32(const unsigned char* masks, const float* depth_est, const double* cams, const float* colors, int N, int h,
                                  int w, const int* order, int n_order, const long long* offsets, long long total, long long capacity,
                                  float* xyz, unsigned char* rgb, void* stream) {
    const int rc = cloud_check(masks, N, h, w, order, n_order);
    if (rc != CER_OK) return rc;
    if (!depth_est || !cams || !colors || !offsets || total < 0 || capacity < 0) return CER_EINVAL;
    if (total != capacity) return CER_ESHAPE;        // the caller allocates exactly what the count pass found
    if (capacity == 0) return CER_OK;                // nothing to write: nothing is launched
    if (!xyz || !rgb) return CER_EINVAL;
    const unsigned P = (unsigned)((long)h * w);
    const int bpv = (int)cloud_bpv(h, w);
    hipStream_t st = (hipStream_t)stream;
    return cloud_for_chunks(order, n_order, [&](const CloudOrder& ord, int k0, int nk) {
        hipLaunchKernelGGL(cloud_emit_kernel, dim3((unsigned)bpv, (unsigned)nk), dim3(256), 0, st, ord, k0, masks, depth_est, cams, colors, P,
                           w, bpv, offsets, capacity, xyz, rgb);
    });
}

// ---- colour planes at the depth grid: prepared images [n, 3, H, W], values 0..255 -> [n, 3, h, w], values 0..1, H = k h, W = k w.
// v / 255 is an IEEE division on every tap; then torch's upsample_bilinear2d(align_corners=False) expression (what fusion._resize runs on
// the host): scale = (float)H / h, src = scale * (dst + 0.5) - 0.5 clamped at 0, i0 = (int)src, the +1 neighbour clamped at the last row /
// column, l1 = src - i0, l0 = 1 - l1, and ly0 * (lx0 a + lx1 b) + ly1 * (lx0 c + lx1 d) with every product and sum rounded on its own
// (-ffp-contract=off).  At an integer ratio the weights are 0, 1/2 or 1 - every product is exact, which is why this is the host's result
// bit for bit there (and why other ratios are refused).
struct GridTap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ GridTap grid_tap(float scale, int d, int in_size) {
    float s = scale * ((float)d + 0.5f) - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    GridTap t;
    t.i0 = min((int)s, in_size - 1);
    t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
    t.l1 = s - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}
// grid: x = 256-column blocks of a row, y = output row, z = plane (image * 3 + channel)
__global__ __launch_bounds__(256) void color_grid_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int h, int w,
                                                         float sy, float sx) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const long plane = blockIdx.z;
    const GridTap ty = grid_tap(sy, y, H), tx = grid_tap(sx, x, W);
    const float* s = src + plane * H * W;
    const float a = s[(long)ty.i0 * W + tx.i0] / 255.0f, b = s[(long)ty.i0 * W + tx.i1] / 255.0f;
    const float c = s[(long)ty.i1 * W + tx.i0] / 255.0f, d = s[(long)ty.i1 * W + tx.i1] / 255.0f;
    dst[(plane * h + y) * w + x] = ty.l0 * (tx.l0 * a + tx.l1 * b) + ty.l1 * (tx.l0 * c + tx.l1 * d);
}

extern "C" int cer_color_grid_f32(const float* prepared, float* colors, int n, int H, int W, int h, int w, void* stream) {
    if (!prepared || !colors || n <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0) return CER_EINVAL;
    if (H % h || W % w || H / h != W / w) return CER_ESHAPE;              // one integer ratio for both axes
    if (h > 65535 || (long)n * 3 > 65535) return CER_ESHAPE;              // rows and planes are grid dimensions
    hipLaunchKernelGGL(color_grid_kernel, dim3((unsigned)((w + 255) / 256), (unsigned)h, (unsigned)(n * 3)), dim3(256), 0, (hipStream_t)stream,
                       prepared, colors, H, W, h, w, (float)H / (float)h, (float)W / (float)w);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

// ---- disparity -> depth (inference.disp_to_depth): 0 where the disparity is 0, else the correctly rounded 1 / d
__global__ __launch_bounds__(256) void disp_to_depth_kernel(const float* __restrict__ disp, float* __restrict__ depth, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float d = disp[i];
    depth[i] = d == 0.0f ? 0.0f : 1.0f / d;
}

extern "C" int cer_disp_to_depth_f32(const float* disp, float* depth, long n, void* stream) {
    if (!disp || !depth || n <= 0) return CER_EINVAL;
    if ((n + 255) / 256 > 0x7fffffffL) return CER_ESHAPE;
    hipLaunchKernelGGL(disp_to_depth_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, disp, depth, n);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}
