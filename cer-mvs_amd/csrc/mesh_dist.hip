// Exact point-to-mesh distance on the device (ABI 1240, cer-mvs_amd/mesh.py MeshIndex / mesh_distances / evaluate_mesh(method="exact"),
// DESIGN.md 3zh; tests/mesh_dist_reference.py): for every query point the face of an indexed triangle mesh with the smallest
// (squared distance, face index) within a cut-off, the distance and optionally the closest point.  What cer_grid_nearest_f32 is for clouds.
//
// The index is cloud_eval.hip's sparse uniform grid with triangles in place of points: a face is entered in every cell of the box of cells
// that its three corners span (cer_mesh_tri_cells_i64 counts those cells per face, the caller's integer prefix sum places them,
// cer_mesh_tri_pairs_i64 writes the (key, face) pairs), one stable sort by key, cer_grid_cells_count_i64 / cer_grid_cells_i64 for the cell
// table, and 48-byte corner records (cer_mesh_tri_pack_f32).  cer_mesh_tri_nearest_f32 walks the rows of cells around a query with
// grid_walk.hpp, nearest cells first, against the best squared distance so far.  A face that lies in several visited cells is measured
// again: the result is the same, and nothing has to remember it.
//
// One thread per face or per query.  Integers, and fp64 with the association of cer_mvs.h: every product, sum and quotient rounds on its
// own (the Makefile's -ffp-contract=off), IEEE division and square root; registers only - no block-shared memory, no barrier, no
// read-modify-write on memory; every address has one writer, the same bytes on every run.  A vertex index outside [0, nv), a face id
// outside [0, nf) and a pair position outside [0, npairs) are skipped, never read through.
#include "common.hpp"
#include "grid_walk.hpp"

#define TRI_SENTINEL 0x7fffffffffffffffLL
#define TRI_MAX_RINGS 4096                           // ceil(max_dist / cell) beyond this: CER_ESHAPE (cloud_eval.hip's GRID_MAX_RINGS)

__device__ __forceinline__ bool tri_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// The box of cells of face f -> 0: the face is left out of the index (area not above 0, an index outside [0, nv), a repeated index, a
// coordinate that is not finite), 1: lo .. hi per axis, 2: a cell coordinate outside the key range.  Per axis the cell of the smallest and of
// the largest corner coordinate, c = floor((double(x) - origin) / cell): subtraction, division by a positive cell and floor are monotone,
// so every corner's cell - and the cell of every point of the triangle - lies between the two.
__device__ __forceinline__ int tri_box(const float* __restrict__ vertices, unsigned nv, const int* __restrict__ f, double area, double ox,
                                       double oy, double oz, double cell, int* lo, int* hi) {
    if (!(area > 0.0)) return 0;
    const int a = f[0], b = f[1], c = f[2];
    if ((unsigned)a >= nv || (unsigned)b >= nv || (unsigned)c >= nv || a == b || b == c || a == c) return 0;
    const float *pa = vertices + 3l * a, *pb = vertices + 3l * b, *pc = vertices + 3l * c;
    if (!tri_finite(pa[0], pa[1], pa[2]) || !tri_finite(pb[0], pb[1], pb[2]) || !tri_finite(pc[0], pc[1], pc[2])) return 0;
    const double o[3] = {ox, oy, oz}, B = (double)GRID_B;
    bool inside = true;
    for (int k = 0; k < 3; ++k) {
        const float mn = fminf(fminf(pa[k], pb[k]), pc[k]), mx = fmaxf(fmaxf(pa[k], pb[k]), pc[k]);
        const double cl = floor(((double)mn - o[k]) / cell), ch = floor(((double)mx - o[k]) / cell);
        inside = inside && fabs(cl) <= B && fabs(ch) <= B;
        lo[k] = inside ? (int)cl : 0;
        hi[k] = inside ? (int)ch : 0;
    }
    return inside ? 1 : 2;
}

__device__ __forceinline__ long long tri_box_cells(const int* lo, const int* hi) {                 // at most (2^21 - 1)^3 < 2^63
    return ((long long)(hi[0] - lo[0] + 1) * (long long)(hi[1] - lo[1] + 1)) * (long long)(hi[2] - lo[2] + 1);
}

// ---- cells: one thread per face.  cells[f] = the number of cells of the face's box, 0 for a face that is left out.  A box outside the key
// range raises flag[0], one of more than CER_TRI_MAX_CELLS cells flag[1] (every thread that sees one stores the same 1: a plain store);
// such a face gets 0 as well.
__global__ __launch_bounds__(256) void mesh_tri_cells_kernel(const float* __restrict__ vertices, unsigned nv, const int* __restrict__ faces,
                                                             unsigned nf, const double* __restrict__ areas, double ox, double oy, double oz,
                                                             double cell, long long* __restrict__ cells, int* __restrict__ flag) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nf) return;
    int lo[3], hi[3];
    const int kind = tri_box(vertices, nv, faces + 3l * f, areas[f], ox, oy, oz, cell, lo, hi);
    long long count = 0;
    if (kind == 2) flag[0] = 1;
    if (kind == 1) {
        count = tri_box_cells(lo, hi);
        if (count > (long long)CER_TRI_MAX_CELLS) {
            flag[1] = 1;
            count = 0;
        }
    }
    cells[f] = count;
}

// ---- pairs: one thread per face.  Face f owns the positions [cum[f - 1], cum[f]) of the pair list (cum: the inclusive prefix sums of
// cells) and writes (key of the cell, f) there, z-major, then y, then x.  A face whose box does not have exactly that many cells, more than
// the cap, or whose positions leave [0, npairs) writes nothing: the caller's keys start as the sentinel.
__global__ __launch_bounds__(256) void mesh_tri_pairs_kernel(const float* __restrict__ vertices, unsigned nv, const int* __restrict__ faces,
                                                             unsigned nf, const double* __restrict__ areas, double ox, double oy, double oz,
                                                             double cell, const long long* __restrict__ cum, long long npairs,
                                                             long long* __restrict__ keys, int* __restrict__ ids) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nf) return;
    int lo[3], hi[3];
    if (tri_box(vertices, nv, faces + 3l * f, areas[f], ox, oy, oz, cell, lo, hi) != 1) return;
    const long long count = tri_box_cells(lo, hi), start = f ? cum[f - 1] : 0ll;
    if (count > (long long)CER_TRI_MAX_CELLS || start < 0 || start > npairs - count || cum[f] - start != count) return;
    long long p = start;
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x, ++p) {
                keys[p] = grid_key(x, y, z);
                ids[p] = (int)f;
            }
}

// ---- pack: one thread per face.  rec[3f .. 3f + 2] = (x, y, z, 0) of the corners a, b, c - 48 bytes, three 16-byte loads per candidate
// in the search; zeros for a face whose indices are out of range (it is in no pair list).
__global__ __launch_bounds__(256) void mesh_tri_pack_kernel(const float* __restrict__ vertices, unsigned nv, const int* __restrict__ faces,
                                                            unsigned nf, uint4* __restrict__ rec) {
    const unsigned f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nf) return;
    const int* idx = faces + 3l * f;
    for (int k = 0; k < 3; ++k) {
        const int v = idx[k];
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if ((unsigned)v < nv) {
            const float* p = vertices + 3l * v;
            r = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]), 0u);
        }
        rec[3l * f + k] = r;
    }
}

// ---- the distance (cer_mvs.h, "Mesh distance"): Ericson's closest point on a triangle, the first region that holds decides.
// dot(x, y) = (x0*y0 + x1*y1) + x2*y2.  A corner region returns the corner itself; the others q = (a + v*ab) + w*ac per axis.
// d2 = (rx*rx + ry*ry) + rz*rz with r = q - p.  A 0 / 0 of a near-degenerate face gives NaN, which no comparison of the search accepts.
struct TriPoint { double d2, x, y, z; };

__device__ __forceinline__ double tri_dot(double x0, double x1, double x2, double y0, double y1, double y2) {
    return (x0 * y0 + x1 * y1) + x2 * y2;
}

__device__ __forceinline__ TriPoint tri_closest(double ax, double ay, double az, double bx, double by, double bz, double cx, double cy,
                                                double cz, double px, double py, double pz) {
    const double abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const double d1 = tri_dot(abx, aby, abz, apx, apy, apz), d2 = tri_dot(acx, acy, acz, apx, apy, apz);
    const double d3 = tri_dot(abx, aby, abz, bpx, bpy, bpz), d4 = tri_dot(acx, acy, acz, bpx, bpy, bpz);
    const double d5 = tri_dot(abx, aby, abz, cpx, cpy, cpz), d6 = tri_dot(acx, acy, acz, cpx, cpy, cpz);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    int corner = -1;                                                             // 0, 1, 2: the corner a, b, c itself
    double v = 0.0, w = 0.0;
    if (d1 <= 0.0 && d2 <= 0.0) corner = 0;
    else if (d3 >= 0.0 && d4 <= d3) corner = 1;
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) v = d1 / (d1 - d3), w = 0.0;
    else if (d6 >= 0.0 && d5 <= d6) corner = 2;
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) v = 0.0, w = d2 / (d2 - d6);
    else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        v = 1.0 - w;
    } else {
        const double den = (va + vb) + vc;
        v = vb / den;
        w = vc / den;
    }
    const double ex = (ax + v * abx) + w * acx, ey = (ay + v * aby) + w * acy, ez = (az + v * abz) + w * acz;
    TriPoint q;
    q.x = corner == 0 ? ax : corner == 1 ? bx : corner == 2 ? cx : ex;
    q.y = corner == 0 ? ay : corner == 1 ? by : corner == 2 ? cy : ey;
    q.z = corner == 0 ? az : corner == 1 ? bz : corner == 2 ? cz : ez;
    const double rx = q.x - px, ry = q.y - py, rz = q.z - pz;
    q.d2 = (rx * rx + ry * ry) + rz * rz;
    return q;
}

// ---- nearest.  One thread per query, walked in qorder (the queries' own cell keys: the lanes of a wave walk the same cells).  Winner =
// smallest (d2, face index); a face counts iff d2 <= double(max_dist)^2 (the best starts at (limit, INT_MAX)).  g.rec is not read: the
// candidates of a run of cells are pair_face[pb .. pe), each a face id whose three records are loaded from tri.
__global__ __launch_bounds__(256) void mesh_tri_nearest_kernel(GridView g, const int* __restrict__ pair_face, long long npairs,
                                                               const uint4* __restrict__ tri, unsigned nf, const float* __restrict__ queries,
                                                               const long long* __restrict__ qorder, long m, float max_dist,
                                                               int* __restrict__ face, float* __restrict__ dist, float* __restrict__ closest) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const long long q = qorder ? qorder[i] : i;
    if (q < 0 || q >= m) return;                                                 // (not a permutation of 0 .. m-1: not the caller's own order)
    const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
    double best = (double)max_dist * (double)max_dist;
    int best_face = 0x7fffffff;
    double bx = 0.0, by = 0.0, bz = 0.0;
    if (tri_finite(qx, qy, qz)) {
        const double X = (double)qx, Y = (double)qy, Z = (double)qz;
        grid_walk_home_first<false>(g, X, Y, Z, [&] { return best; }, [&](int xa, int xb, int y, int z) {
            long long j, pe;
            if (!grid_row_span(g, xa, xb, y, z, j, pe)) return;
            if (j < 0) j = 0;
            if (pe > npairs) pe = npairs;
            for (; j < pe; ++j) {
                const int f = pair_face[j];
                if ((unsigned)f >= nf) continue;
                const uint4 ta = tri[3l * f], tb = tri[3l * f + 1], tc = tri[3l * f + 2];
                const TriPoint t = tri_closest((double)__uint_as_float(ta.x), (double)__uint_as_float(ta.y), (double)__uint_as_float(ta.z),
                                               (double)__uint_as_float(tb.x), (double)__uint_as_float(tb.y), (double)__uint_as_float(tb.z),
                                               (double)__uint_as_float(tc.x), (double)__uint_as_float(tc.y), (double)__uint_as_float(tc.z), X, Y, Z);
                if (t.d2 < best || (t.d2 == best && f < best_face)) best = t.d2, best_face = f, bx = t.x, by = t.y, bz = t.z;
            }
        });
    }
    const bool found = best_face != 0x7fffffff;
    face[q] = found ? best_face : -1;
    dist[q] = found ? (float)__builtin_sqrt(best) : __builtin_inff();
    if (closest) {
        const float nan = __int_as_float(0x7fc00000);
        closest[3 * q] = found ? (float)bx : nan;
        closest[3 * q + 1] = found ? (float)by : nan;
        closest[3 * q + 2] = found ? (float)bz : nan;
    }
}

// ---- entry points.  Checks, in the order of the section "Surface mesh", all before any launch: (1) a negative size, a frame or a cut-off
// that is no number of its kind -> CER_EINVAL; (2) too large -> CER_ESHAPE; (3) nothing to do -> CER_OK, nothing launched; (4) null
// pointers -> CER_EINVAL, then records that are not 16-byte aligned -> CER_EALIGN.
static const long long TRI_INT_MAX = 0x7fffffffLL;
static unsigned tri_blocks(long long n) { return (unsigned)((n + 255) / 256); }

extern "C" int cer_mesh_tri_cells_i64(const float* vertices, long long nv, const int* faces, long long nf, const double* areas,
                                      const double* origin, double cell, long long* cells, int* flag, void* stream) {
    if (nv < 0 || nf < 0 || !cer_frame_ok(origin, cell)) return CER_EINVAL;
    if (nv > TRI_INT_MAX || nf > TRI_INT_MAX / 3) return CER_ESHAPE;
    if (nf == 0) return CER_OK;
    if (!faces || !areas || !cells || !flag || (nv && !vertices)) return CER_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(flag, 0, 2 * sizeof(int), st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(mesh_tri_cells_kernel, dim3(tri_blocks(nf)), dim3(256), 0, st, vertices, (unsigned)nv, faces, (unsigned)nf, areas, origin[0],
                       origin[1], origin[2], cell, cells, flag);
    CER_RETURN_IF_LAUNCH_FAILED();
    int raised[2] = {0, 0};                          // the one answer this call owes its caller: does every face fit the key range and the cap
    hipError_t e = hipMemcpyAsync(raised, flag, 2 * sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (raised[0] || raised[1]) return CER_ESHAPE;
    return CER_OK;
}

extern "C" int cer_mesh_tri_pairs_i64(const float* vertices, long long nv, const int* faces, long long nf, const double* areas,
                                      const double* origin, double cell, const long long* cum, long long npairs, long long* keys, int* ids,
                                      void* stream) {
    if (nv < 0 || nf < 0 || npairs < 0 || !cer_frame_ok(origin, cell)) return CER_EINVAL;
    if (nv > TRI_INT_MAX || nf > TRI_INT_MAX / 3 || npairs > TRI_INT_MAX) return CER_ESHAPE;
    if (nf == 0 || npairs == 0) return CER_OK;
    if (!faces || !areas || !cum || !keys || !ids || (nv && !vertices)) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_tri_pairs_kernel, dim3(tri_blocks(nf)), dim3(256), 0, (hipStream_t)stream, vertices, (unsigned)nv, faces, (unsigned)nf,
                       areas, origin[0], origin[1], origin[2], cell, cum, npairs, keys, ids);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_tri_pack_f32(const float* vertices, long long nv, const int* faces, long long nf, void* records, void* stream) {
    if (nv < 0 || nf < 0) return CER_EINVAL;
    if (nv > TRI_INT_MAX || nf > TRI_INT_MAX / 3) return CER_ESHAPE;
    if (nf == 0) return CER_OK;
    if (!faces || !records || (nv && !vertices)) return CER_EINVAL;
    if ((uintptr_t)records & 15) return CER_EALIGN;
    hipLaunchKernelGGL(mesh_tri_pack_kernel, dim3(tri_blocks(nf)), dim3(256), 0, (hipStream_t)stream, vertices, (unsigned)nv, faces, (unsigned)nf,
                       (uint4*)records);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_tri_nearest_f32(const void* records, long long nf, const int* pair_face, long long npairs, const long long* cell_keys,
                                        const long long* cell_start, long long ncells, const double* origin, double cell, const float* queries,
                                        const long long* qorder, long long m, float max_dist, int* face, float* dist, float* closest,
                                        void* stream) {
    if (nf < 0 || npairs < 0 || ncells < 0 || m < 0 || !cer_frame_ok(origin, cell) || !(max_dist >= 0.0f)) return CER_EINVAL;
    if (nf > TRI_INT_MAX / 3 || npairs > TRI_INT_MAX || m > TRI_INT_MAX || ncells > npairs) return CER_ESHAPE;
    const double rings = ceil((double)max_dist / cell);
    if (!(rings <= (double)TRI_MAX_RINGS)) return CER_ESHAPE;
    if (m == 0 || nf == 0 || npairs == 0 || ncells == 0) return CER_OK;          // (an empty side: the caller fills face = -1, dist = +inf, closest = NaN)
    if (!records || !pair_face || !cell_keys || !cell_start || !queries || !face || !dist) return CER_EINVAL;     // (qorder, closest: null iff absent)
    if ((uintptr_t)records & 15) return CER_EALIGN;
    const GridView g = {nullptr, cell_keys, cell_start, (long)ncells, origin[0], origin[1], origin[2], cell, (int)rings + 1};
    hipLaunchKernelGGL(mesh_tri_nearest_kernel, dim3(tri_blocks(m)), dim3(256), 0, (hipStream_t)stream, g, pair_face, npairs, (const uint4*)records,
                       (unsigned)nf, queries, qorder, (long)m, max_dist, face, dist, closest);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}
