// Rigid registration of two clouds (cer-mvs_amd/cloud_eval.py rigid_transform / pair_moments / icp): what point-to-point ICP needs
// beside cer_grid_nearest_f32 - the rigid motion of a cloud, and the reduction of the matched pairs to the 17 sums from which the host solves
// the least-squares motion (Kabsch).  fp64 arithmetic on float32 coordinates, every association written out (the Makefile's
// -ffp-contract=off keeps products and sums apart); no atomics, fixed grids and a fixed summation tree: the same bits on every run.
// Point-to-plane ICP (plane_moments) reduces the matched pairs and the target's normals to 30 sums - the 6x6 normal equations of
// the linearised step - through the same two passes.
#include "common.hpp"

#define MOM_TILE CER_MOMENT_TILE                     // pairs per block of the first pass
#define MOM_ITER (MOM_TILE / 256)
#define MOM_N CER_MOMENT_COUNT                       // 17 sums
#define PLN_N CER_PLANE_MOMENT_COUNT                 // 30 sums of the point-to-plane pairs
#define MOM_FINAL 1024                              // threads of the second pass's one block

struct AlignRows { double m[12]; };                  // the 3x4 motion, row-major, by value

// ---- transform.  out[i][r] = float(((T[r][0] * x + T[r][1] * y) + T[r][2] * z) + T[r][3]) with x, y, z promoted to fp64: three products,
// three sums and one conversion per coordinate, in that order; non-finite coordinates propagate by IEEE rules.
__global__ __launch_bounds__(256) void cloud_transform_kernel(const float* __restrict__ pts, long n, AlignRows T, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = (double)pts[3 * i], y = (double)pts[3 * i + 1], z = (double)pts[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[3 * i + r] = (float)(((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3]);
}

// ---- moments.  A pair is (a[i], b[idx[i]]) for idx[i] >= 0 and a finite a[i].  With A = double(a) - pivot, B = double(b) - pivot (one
// rounding per coordinate) and D = double(a) - double(b) (the difference of the promoted coordinates themselves, not A - B: exact unless the
// exponents are 29 apart, and free of the pivot's rounding), a pair's 17 terms are: 1 | A | B | A[r] * B[c] at 7 + 3 r + c | (Dx*Dx + Dy*Dy) +
// Dz*Dz - the d2 of cer_grid_nearest_f32, bit for bit.
//
// Summation shape (the tests count their error bound from it):
//   pass 1: block p owns pairs p * MOM_TILE .. + MOM_TILE - 1; thread t adds the terms of pairs t, t + 256, ... (MOM_ITER of them, ascending)
//           to 17 accumulators that start at 0; a wave adds its 64 lanes in a butterfly (lane ^ 1, 2, 4, 8, 16, 32: every lane ends with the
//           same bits, as a + b == b + a); the block's four wave sums are added as (w0 + w1) + (w2 + w3); partials[k * P + p] = sum k.
//   pass 2: one block of MOM_FINAL threads; thread t adds partials t, t + MOM_FINAL, ... (ascending) of every sum; the same butterfly; the
//           sixteen wave sums in a pairwise tree of depth four.
// The tree of a sum is fixed by m alone.
__device__ __forceinline__ double mom_wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// -> on threads 0 .. N - 1: the block's sum number threadIdx.x (N sums, NW waves; sh: NW * N doubles of LDS)
template <int N, int NW>
__device__ __forceinline__ double mom_block_sum(double (&acc)[N], double* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double v = mom_wave_sum(acc[k]);
        if (lane == 0) sh[wave * N + k] = v;
    }
    __syncthreads();
    double w[NW];
    if (threadIdx.x < N) {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = sh[i * N + threadIdx.x];
#pragma unroll
        for (int s = 1; s < NW; s *= 2) {
#pragma unroll
            for (int i = 0; i < NW; i += 2 * s) w[i] += w[i + s];
        }
        return w[0];
    }
    return 0.0;
}

__global__ __launch_bounds__(256) void moment_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const long long* __restrict__ idx, long m, double px, double py, double pz,
                                                          double* __restrict__ partials, long np) {
    __shared__ double sh[4 * MOM_N];
    double acc[MOM_N];
#pragma unroll
    for (int k = 0; k < MOM_N; ++k) acc[k] = 0.0;
    const long base = (long)blockIdx.x * MOM_TILE + threadIdx.x;
#pragma unroll 2
    for (int j = 0; j < MOM_ITER; ++j) {
        const long i = base + 256 * j;
        if (i >= m) break;
        const long long q = idx[i];
        const float ax = a[3 * i], ay = a[3 * i + 1], az = a[3 * i + 2];
        if (q < 0 || !(isfinite(ax) && isfinite(ay) && isfinite(az))) continue;
        const double X = (double)ax, Y = (double)ay, Z = (double)az;
        const double U = (double)b[3 * q], V = (double)b[3 * q + 1], W = (double)b[3 * q + 2];
        const double A[3] = {X - px, Y - py, Z - pz}, B[3] = {U - px, V - py, W - pz};
        const double dx = X - U, dy = Y - V, dz = Z - W;
        acc[0] += 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            acc[1 + r] += A[r];
            acc[4 + r] += B[r];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[7 + 3 * r + c] += A[r] * B[c];
        }
        acc[16] += (dx * dx + dy * dy) + dz * dz;
    }
    const double s = mom_block_sum<MOM_N, 4>(acc, sh);
    if (threadIdx.x < MOM_N) partials[(long)threadIdx.x * np + blockIdx.x] = s;
}

// pass 2 of N sums (the 17 of the pairs, the 30 of the planes); sh: (MOM_FINAL / 64) * N doubles of LDS
template <int N>
__device__ __forceinline__ void moment_final(const double* __restrict__ partials, long np, double* __restrict__ out, double* sh) {
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (long p = threadIdx.x; p < np; p += MOM_FINAL) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += partials[(long)k * np + p];
    }
    const double s = mom_block_sum<N, MOM_FINAL / 64>(acc, sh);
    if (threadIdx.x < N) out[threadIdx.x] = s;
}

__global__ __launch_bounds__(MOM_FINAL) void moment_final_kernel(const double* __restrict__ partials, long np, double* __restrict__ out) {
    __shared__ double sh[(MOM_FINAL / 64) * MOM_N];
    moment_final<MOM_N>(partials, np, out, sh);
}

__global__ __launch_bounds__(MOM_FINAL) void plane_moment_final_kernel(const double* __restrict__ partials, long np, double* __restrict__ out) {
    __shared__ double sh[(MOM_FINAL / 64) * PLN_N];
    moment_final<PLN_N>(partials, np, out, sh);
}

// ---- plane moments (point-to-plane ICP).  A pair is (a[i], b[q], n = nrm[q]) for q = idx[i] >= 0, a finite a[i] and a finite n
// that is not (0, 0, 0) - cer_grid_normals_f32's "no plane"; n is used as given, not normalised.  With A = double(a) - pivot and D = double(a) -
// double(b) (of the promoted coordinates, as above): r = (Dx*nx + Dy*ny) + Dz*nz, the plane residual; c = A x n = (A1*n2 - A2*n1, A2*n0 - A0*n2,
// A0*n1 - A1*n0); J = (c, n), the derivative of r by a small rotation about the pivot and by a translation.  A pair's 30 terms: 1 | J_i * J_j for
// i <= j, row-major (21) | J_i * r (6) | r * r | (Dx*Dx + Dy*Dy) + Dz*Dz.  The summation shape is the one above, sum for sum.
__global__ __launch_bounds__(256) void plane_moment_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                const float* __restrict__ nrm, const long long* __restrict__ idx, long m,
                                                                double px, double py, double pz, double* __restrict__ partials, long np) {
    __shared__ double sh[4 * PLN_N];
    double acc[PLN_N];
#pragma unroll
    for (int k = 0; k < PLN_N; ++k) acc[k] = 0.0;
    const long base = (long)blockIdx.x * MOM_TILE + threadIdx.x;
#pragma unroll 2
    for (int j = 0; j < MOM_ITER; ++j) {
        const long i = base + 256 * j;
        if (i >= m) break;
        const long long q = idx[i];
        const float ax = a[3 * i], ay = a[3 * i + 1], az = a[3 * i + 2];
        if (q < 0 || !(isfinite(ax) && isfinite(ay) && isfinite(az))) continue;
        const float nx = nrm[3 * q], ny = nrm[3 * q + 1], nz = nrm[3 * q + 2];
        if (!(isfinite(nx) && isfinite(ny) && isfinite(nz)) || (nx == 0.0f && ny == 0.0f && nz == 0.0f)) continue;
        const double X = (double)ax, Y = (double)ay, Z = (double)az;
        const double U = (double)b[3 * q], V = (double)b[3 * q + 1], W = (double)b[3 * q + 2];
        const double n0 = (double)nx, n1 = (double)ny, n2 = (double)nz;
        const double A0 = X - px, A1 = Y - py, A2 = Z - pz;
        const double dx = X - U, dy = Y - V, dz = Z - W;
        const double r = (dx * n0 + dy * n1) + dz * n2;
        const double J[6] = {A1 * n2 - A2 * n1, A2 * n0 - A0 * n2, A0 * n1 - A1 * n0, n0, n1, n2};
        acc[0] += 1.0;
#pragma unroll
        for (int u = 0, t = 1; u < 6; ++u) {
#pragma unroll
            for (int v = u; v < 6; ++v, ++t) acc[t] += J[u] * J[v];
        }
#pragma unroll
        for (int u = 0; u < 6; ++u) acc[22 + u] += J[u] * r;
        acc[28] += r * r;
        acc[29] += (dx * dx + dy * dy) + dz * dz;
    }
    const double s = mom_block_sum<PLN_N, 4>(acc, sh);
    if (threadIdx.x < PLN_N) partials[(long)threadIdx.x * np + blockIdx.x] = s;
}

// ---- entry points.  Sizes as the cer_grid_* entry points take them: negative -> CER_EINVAL, 2^31 and beyond -> CER_ESHAPE; then the matrix /
// pivot (null or a non-finite entry -> CER_EINVAL); zero -> nothing to do (CER_OK, nothing launched); then null pointers -> CER_EINVAL.
static int align_size_check(long n) {
    if (n < 0) return CER_EINVAL;
    if (n >= 0x80000000L) return CER_ESHAPE;
    return CER_OK;
}
static bool align_all_finite(const double* v, int n) {
    if (!v) return false;
    for (int i = 0; i < n; ++i)
        if (!(v[i] - v[i] == 0.0)) return false;
    return true;
}

extern "C" int cer_cloud_transform_f32(const float* points, long n, const double* T, float* out, void* stream) {
    const int rc = align_size_check(n);
    if (rc != CER_OK) return rc;
    if (!align_all_finite(T, 12)) return CER_EINVAL;
    if (n == 0) return CER_OK;
    if (!points || !out) return CER_EINVAL;
    const uintptr_t p = (uintptr_t)points, o = (uintptr_t)out, bytes = (uintptr_t)n * 12;
    if (p < o + bytes && o < p + bytes) return CER_EINVAL;                        // a thread's three stores would race other threads' loads
    AlignRows rows;
    for (int i = 0; i < 12; ++i) rows.m[i] = T[i];
    hipLaunchKernelGGL(cloud_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, n, rows, out);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" long cer_cloud_moment_partials(long m) {
    const int rc = align_size_check(m);
    return rc != CER_OK ? rc : (m + MOM_TILE - 1) / MOM_TILE;
}

extern "C" int cer_cloud_pair_moments_f64(const float* a, const float* b, const long long* idx, long m, const double* pivot, double* partials,
                                          double* out, void* stream) {
    const int rc = align_size_check(m);
    if (rc != CER_OK) return rc;
    if (!align_all_finite(pivot, 3)) return CER_EINVAL;
    if (m == 0) return CER_OK;                       // (no pair: the 17 zeros are the caller's to write)
    if (!a || !b || !idx || !partials || !out) return CER_EINVAL;
    const long np = (m + MOM_TILE - 1) / MOM_TILE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(moment_tile_kernel, dim3((unsigned)np), dim3(256), 0, st, a, b, idx, m, pivot[0], pivot[1], pivot[2], partials, np);
    CER_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(moment_final_kernel, dim3(1), dim3(MOM_FINAL), 0, st, (const double*)partials, np, out);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" long cer_cloud_plane_moment_partials(long m) { return cer_cloud_moment_partials(m); }

extern "C" int cer_cloud_plane_moments_f64(const float* a, const float* b, const float* nrm, const long long* idx, long m, const double* pivot,
                                           double* partials, double* out, void* stream) {
    const int rc = align_size_check(m);
    if (rc != CER_OK) return rc;
    if (!align_all_finite(pivot, 3)) return CER_EINVAL;
    if (m == 0) return CER_OK;                       // (no pair: the 30 zeros are the caller's to write)
    if (!a || !b || !nrm || !idx || !partials || !out) return CER_EINVAL;
    const long np = (m + MOM_TILE - 1) / MOM_TILE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(plane_moment_tile_kernel, dim3((unsigned)np), dim3(256), 0, st, a, b, nrm, idx, m, pivot[0], pivot[1], pivot[2], partials,
                       np);
    CER_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(plane_moment_final_kernel, dim3(1), dim3(MOM_FINAL), 0, st, (const double*)partials, np, out);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}
