// Mesh surface sampling on the device (ABI 1230, cer-mvs_amd/mesh.py face_areas / sample_mesh / sample_mesh_even / evaluate_mesh, DESIGN.md
// 3zg; tests/mesh_sample_reference.py): points on the surface of any indexed triangle mesh with a density proportional to area.  The area
// of every face in fp64, an INTEGER weight per face (the area scaled by a power of two and floored, so that the caller's prefix sum is exact
// whatever the shape of its scan), and per sample four random words - the caller's, or Philox4x32-10 on the sample's global index - that
// pick a face by a search in the prefix sums and a point in it by folding the unit square onto the triangle.
//
// Three kernels, one thread per face or per sample.  Integers, and fp64 with the association of cer_mvs.h; registers only: no block-shared
// memory, no barrier, no read-modify-write on memory, no fused multiply-add; every address has one writer, the same bytes on every run, and
// sample k is a pure function of (seed, k, mesh): it does not depend on n, on the grid or on the run.  An index outside its range is skipped,
// never read through, and the search cannot leave its table whatever the table holds.
#include "common.hpp"

__device__ __forceinline__ bool sample_finite(double x) { return x - x == 0.0; }

// the three corners of a face in fp64 -> true iff the indices are in range and distinct (the corners are read only then)
__device__ __forceinline__ bool sample_corners(const float* __restrict__ vertices, unsigned nv, const int* __restrict__ f, double* A, double* B,
                                               double* C, int* ia, int* ib, int* ic) {
    const int a = f[0], b = f[1], c = f[2];
    *ia = a;
    *ib = b;
    *ic = c;
    if ((unsigned)a >= nv || (unsigned)b >= nv || (unsigned)c >= nv || a == b || b == c || a == c) return false;
    const float *pa = vertices + 3l * a, *pb = vertices + 3l * b, *pc = vertices + 3l * c;
    for (int k = 0; k < 3; ++k) {
        A[k] = (double)pa[k];
        B[k] = (double)pb[k];
        C[k] = (double)pc[k];
    }
    return true;
}

// n = e1 x e2 with e1 = b - a, e2 = c - a, every product and difference rounded on its own
__device__ __forceinline__ void sample_cross(const double* A, const double* B, const double* C, double* nx, double* ny, double* nz) {
    const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const double e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
    *nx = e1y * e2z - e1z * e2y;
    *ny = e1z * e2x - e1x * e2z;
    *nz = e1x * e2y - e1y * e2x;
}

// ---- areas: one thread per face.  0 when an index is outside [0, nv), two indices are equal or one of the nine coordinates is not finite;
// otherwise 0.5 * sqrt((nx*nx + ny*ny) + nz*nz).
__global__ __launch_bounds__(256) void mesh_face_areas_kernel(const float* __restrict__ vertices, unsigned nv, const int* __restrict__ faces,
                                                              unsigned nf, double* __restrict__ areas) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nf) return;
    double A[3], B[3], C[3];
    int ia, ib, ic;
    double area = 0.0;
    if (sample_corners(vertices, nv, faces + 3l * f, A, B, C, &ia, &ib, &ic)) {
        bool finite = true;
        for (int k = 0; k < 3; ++k) finite = finite && sample_finite(A[k]) && sample_finite(B[k]) && sample_finite(C[k]);
        if (finite) {
            double nx, ny, nz;
            sample_cross(A, B, C, &nx, &ny, &nz);
            area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
        }
    }
    areas[f] = area;
}

// ---- weights: one thread per face.  floor(areas[f] * 2^shift) as an integer; the scaling by a power of two is exact.  An area that is
// not a number, is negative, or scales to 2^63 and beyond (no area of the table the shift was taken from does) gets 0.
__global__ __launch_bounds__(256) void mesh_face_weights_kernel(const double* __restrict__ areas, unsigned nf, int shift,
                                                                long long* __restrict__ weights) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nf) return;
    const double x = floor(ldexp(areas[f], shift));
    weights[f] = (x >= 0.0 && x < 9223372036854775808.0) ? (long long)x : 0ll;
}

// ---- Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1)
__device__ __forceinline__ void sample_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* x) {
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x[0] = c0;
    x[1] = c1;
    x[2] = c2;
    x[3] = c3;
}

// ---- samples: one thread per sample i, global index k = offset + i (64-bit, unsigned).  Words x0 .. x3: row i of words, or Philox with the
// counter (k & 0xffffffff, k >> 32, 0, 0) and the key (seed & 0xffffffff, seed >> 32).  Face: r = x0 * 2^32 + x1, t = floor(r * W / 2^64) with
// W = cum[nf - 1], f = the smallest index with cum[f] > t - a bisection on [0, nf - 1] that ends inside the table on any table.  Position:
// (a, b) = (x2, x3), mirrored to (2^32 - 1 - a, 2^32 - 1 - b) when a + b >= 2^32; u = (a + 0.5) * 2^-32, v likewise, w = (1 - u) - v, all
// exact and w >= 0; per axis float((w*A + u*B) + v*C).  A face whose indices are out of range or equal gives NaN (and colour 0).
__global__ __launch_bounds__(256) void mesh_sample_kernel(const float* __restrict__ vertices, unsigned nv, const int* __restrict__ faces,
                                                          unsigned nf, const long long* __restrict__ cum, unsigned long long seed,
                                                          unsigned long long offset, const unsigned* __restrict__ words, unsigned n,
                                                          const unsigned char* __restrict__ colors, float* __restrict__ points,
                                                          int* __restrict__ face, double* __restrict__ uv, float* __restrict__ normals,
                                                          unsigned char* __restrict__ out_colors) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    unsigned x[4];
    if (words != nullptr) {
        const unsigned* row = words + 4l * i;
        x[0] = row[0];
        x[1] = row[1];
        x[2] = row[2];
        x[3] = row[3];
    } else {
        const unsigned long long k = offset + (unsigned long long)i;
        sample_philox((unsigned)(k & 0xffffffffull), (unsigned)(k >> 32), 0u, 0u, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), x);
    }
    // the face
    const long long total = cum[nf - 1];
    const unsigned long long W = total > 0 ? (unsigned long long)total : 0ull;
    const unsigned long long r = ((unsigned long long)x[0] << 32) | (unsigned long long)x[1];
    const long long t = (long long)__umul64hi(r, W);                     // < W < 2^63
    unsigned lo = 0u, hi = nf - 1u;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2u;
        if (cum[mid] > t) hi = mid;
        else lo = mid + 1u;
    }
    const unsigned f = lo;
    // the position
    unsigned long long a = x[2], b = x[3];
    if (a + b >= 0x100000000ull) {
        a = 0xffffffffull - a;
        b = 0xffffffffull - b;
    }
    const double u = ((double)a + 0.5) * 0x1p-32, v = ((double)b + 0.5) * 0x1p-32;
    const double w = (1.0 - u) - v;
    double A[3], B[3], C[3];
    int ia, ib, ic;
    const bool ok = sample_corners(vertices, nv, faces + 3l * f, A, B, C, &ia, &ib, &ic);
    const float nan = __int_as_float(0x7fc00000);
    float* p = points + 3l * i;
    for (int k = 0; k < 3; ++k) p[k] = ok ? (float)((w * A[k] + u * B[k]) + v * C[k]) : nan;
    face[i] = (int)f;
    if (uv != nullptr) {
        uv[2l * i] = u;
        uv[2l * i + 1] = v;
    }
    if (normals != nullptr) {
        float* q = normals + 3l * i;
        if (ok) {
            double nx, ny, nz;
            sample_cross(A, B, C, &nx, &ny, &nz);
            const double len = sqrt((nx * nx + ny * ny) + nz * nz);
            q[0] = (float)(nx / len);
            q[1] = (float)(ny / len);
            q[2] = (float)(nz / len);
        } else {
            q[0] = nan;
            q[1] = nan;
            q[2] = nan;
        }
    }
    if (colors != nullptr && out_colors != nullptr) {
        unsigned char* o = out_colors + 3l * i;
        for (int k = 0; k < 3; ++k) {
            double c = 0.0;
            if (ok) {
                const double ca = (double)colors[3l * ia + k], cb = (double)colors[3l * ib + k], cc = (double)colors[3l * ic + k];
                c = floor(((w * ca + u * cb) + v * cc) + 0.5);
            }
            o[k] = (unsigned char)(c < 255.0 ? (int)c : 255);
        }
    }
}

// Checks, in the order of the section "Surface mesh": a negative size, too large, nothing to do, pointers.
static const long long SAMPLE_INT_MAX = 0x7fffffffLL;

extern "C" int cer_mesh_face_areas_f64(const float* vertices, long long nv, const int* faces, long long nf, double* areas, void* stream) {
    if (nv < 0 || nf < 0) return CER_EINVAL;
    if (nv > SAMPLE_INT_MAX || nf > SAMPLE_INT_MAX / 3) return CER_ESHAPE;
    if (nf == 0) return CER_OK;
    if (!faces || !areas || (nv && !vertices)) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_face_areas_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, (unsigned)nv, faces,
                       (unsigned)nf, areas);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_face_weights_i64(const double* areas, long long nf, int shift, long long* weights, void* stream) {
    if (nf < 0) return CER_EINVAL;
    if (nf > SAMPLE_INT_MAX / 3 || shift < CER_SAMPLE_SHIFT_MIN || shift > CER_SAMPLE_SHIFT_MAX) return CER_ESHAPE;
    if (nf == 0) return CER_OK;
    if (!areas || !weights) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_face_weights_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, areas, (unsigned)nf, shift,
                       weights);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_sample_f32(const float* vertices, long long nv, const int* faces, long long nf, const long long* cum,
                                   unsigned long long seed, unsigned long long offset, const unsigned* words, long long n,
                                   const unsigned char* colors, float* points, int* face, double* uv, float* normals,
                                   unsigned char* out_colors, void* stream) {
    if (nv < 0 || nf < 0 || n < 0) return CER_EINVAL;
    if (nv > SAMPLE_INT_MAX || nf > SAMPLE_INT_MAX / 3 || n > SAMPLE_INT_MAX || (n > 0 && nf == 0)) return CER_ESHAPE;
    if (n == 0) return CER_OK;
    if (!faces || !cum || !points || !face || (nv && !vertices)) return CER_EINVAL;      // (words, uv, normals: null iff absent)
    if ((colors == nullptr) != (out_colors == nullptr)) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, (unsigned)nv, faces,
                       (unsigned)nf, cum, seed, offset, words, (unsigned)n, colors, points, face, uv, normals, out_colors);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}
