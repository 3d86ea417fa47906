// Cloud-to-cloud evaluation on the device (cer-mvs_amd/cloud_eval.py): the exact nearest neighbour of every query point in a target cloud
// within a cut-off distance - what DTU's accuracy / completeness and Tanks-and-Temples' precision / recall / F-score are means and shares of.
//
// The target is indexed by a sparse uniform grid that exists only as sorted keys: cer_grid_keys_f32 gives every point the 63-bit key of its
// cell, the host sorts the keys (stable) and cer_grid_pack_f32 gathers the points into that order as 16-byte records (x, y, z, original index),
// cer_grid_cells_count_i64 / cer_grid_cells_i64 list the occupied cells with their first sorted point (compact.hpp's count / scan / emit over
// the heads of the sorted keys), and cer_grid_nearest_f32 searches.  No atomics anywhere: the same bytes on every run.
// On the same grid, cer_grid_thin_round_f32 / cer_grid_thin_compact_i32 are the rounds of the DTU script's greedy radius thinning (below),
// and cer_grid_knn_f32 / cer_grid_count_within_f32 the k nearest neighbours of a query and the number of points within a radius of it;
// cer_grid_normals_f32 turns those neighbours into a surface normal and a curvature (the plane through them, by PCA).
//
// Key layout: (z + B) << 42 | (y + B) << 21 | (x + B), B = CER_GRID_COORD_LIMIT - 1, cell coordinates in -B .. B: every field is at most
// 2^21 - 2, so no key reaches the sentinel (2^63 - 1, all 63 bits set) and key(x + 1, y, z) = key(x, y, z) + 1 never carries.  x is the
// lowest field: the cells x0 .. x1 of one (y, z) row are a contiguous run of the cell table and their points a contiguous run of the
// sorted points, found with two binary searches.
#include "common.hpp"
#include "compact.hpp"
#include "grid_walk.hpp"                             // the key, the view of the index and the row walk (shared with mesh_dist.hip)

#define GRID_TILE CER_GRID_TILE                      // sorted keys per block of the cell passes
#define GRID_ITER (GRID_TILE / 256)
#define GRID_SENTINEL 0x7fffffffffffffffLL
#define GRID_MAX_RINGS 4096                          // ceil(max_dist / cell) beyond this: CER_ESHAPE (the cell is far too small for the cut-off)

__device__ __forceinline__ bool grid_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ---- keys.  u = (double(p) - origin) / cell with an IEEE fp64 division, c = floor(u).  clamp: coordinates are clamped into -B .. B (the
// query side: its keys only order the queries, the search never reads them); otherwise a coordinate outside raises *flag (every thread that
// sees one stores the same 1: a plain store, no atomic) and the point takes the sentinel.
__global__ __launch_bounds__(256) void grid_keys_kernel(const float* __restrict__ pts, long n, double ox, double oy, double oz, double cell,
                                                        int clamp, long long* __restrict__ keys, int* __restrict__ flag) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    long long key = GRID_SENTINEL;
    if (grid_finite(x, y, z)) {
        double cx = floor(((double)x - ox) / cell), cy = floor(((double)y - oy) / cell), cz = floor(((double)z - oz) / cell);
        const double B = (double)GRID_B;
        if (clamp) {
            cx = fmin(fmax(cx, -B), B);
            cy = fmin(fmax(cy, -B), B);
            cz = fmin(fmax(cz, -B), B);
        }
        if (fabs(cx) <= B && fabs(cy) <= B && fabs(cz) <= B)
            key = grid_key((int)cx, (int)cy, (int)cz);
        else
            *flag = 1;
    }
    keys[i] = key;
}

// ---- pack: rec[i] = (x, y, z, order[i]) of point order[i] - 16 bytes, one load per candidate in the search
__global__ __launch_bounds__(256) void grid_pack_kernel(const float* __restrict__ pts, const long long* __restrict__ order, long n,
                                                        uint4* __restrict__ rec) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long j = order[i];
    rec[i] = make_uint4(__float_as_uint(pts[3 * j]), __float_as_uint(pts[3 * j + 1]), __float_as_uint(pts[3 * j + 2]), (unsigned)j);
}

// ---- cells.  A head is a sorted position whose key is not the sentinel and differs from its predecessor's.
__device__ __forceinline__ bool grid_head(const long long* __restrict__ keys, long n, long i) {
    if (i >= n) return false;
    const long long k = keys[i];
    return k != GRID_SENTINEL && (i == 0 || keys[i - 1] != k);
}

// the tile walk of the emit pass: bal[j] = the heads of the wave's row j; returns the wave's total
__device__ __forceinline__ unsigned grid_ballots(const long long* __restrict__ keys, long n, long seg, unsigned long long (&bal)[GRID_ITER]) {
    return compact_ballots(seg, [=](long i) { return grid_head(keys, n, i); }, bal);
}

__global__ __launch_bounds__(256) void grid_count_kernel(const long long* __restrict__ keys, long n, unsigned* __restrict__ partials) {
    compact_count<GRID_TILE>(compact_seg<GRID_TILE, long>(), [=](long i) { return grid_head(keys, n, i); }, partials, blockIdx.x);
}

// one block: offsets[i] = sum of partials[0 .. i), offsets[np] = totals[0] = the number of cells; totals[1] = the number of keys below the
// sentinel (the first sentinel's position in the sorted keys: a binary search by one thread)
__global__ __launch_bounds__(1024) void grid_scan_kernel(const unsigned* __restrict__ partials, long np, const long long* __restrict__ keys, long n,
                                                         long long* __restrict__ offsets, long long* __restrict__ totals) {
    const long long ncells = compact_scan(partials, np, offsets);
    if (threadIdx.x == 0) {
        totals[0] = ncells;
        totals[1] = grid_lower_bound(keys, 0, n, GRID_SENTINEL);
    }
}

// cell_keys[r] = key and cell_start[r] = sorted position of head r; cell_start[ncells] = the number of keys below the sentinel - written from
// the last real key's position, which need not be a head: the one emit kernel on compact.hpp's pieces, not on compact_emit
__global__ __launch_bounds__(256) void grid_emit_kernel(const long long* __restrict__ keys, long n, const long long* __restrict__ offsets,
                                                        long long ncells, long long* __restrict__ cell_keys, long long* __restrict__ cell_start) {
    const int lane = threadIdx.x & 63;
    const long seg = compact_seg<GRID_TILE, long>();
    unsigned long long bal[GRID_ITER];
    const unsigned tot = grid_ballots(keys, n, seg, bal);
    long long base = compact_wave_base(tot, offsets, blockIdx.x);
#pragma unroll
    for (int j = 0; j < GRID_ITER; ++j) {
        const long p = seg + 64 * j;
        const long long r = base + compact_rank(bal[j]);
        base += __popcll(bal[j]);
        if (p < n) {
            const long long k = keys[p];
            if (k != GRID_SENTINEL && (p == n - 1 || keys[p + 1] == GRID_SENTINEL)) cell_start[ncells] = p + 1;      // the last real key: one thread
        }
        if (!((bal[j] >> lane) & 1ull) || r >= ncells) continue;                 // (never past what the caller allocated)
        cell_keys[r] = keys[p];
        cell_start[r] = p;
    }
}

// ---- GridView, the row walk under every search and the argument for its exactness: grid_walk.hpp.

// The candidate loop of every search: visit(d2, w) for the records of cells xa .. xb of row (y, z), d2 = (dx*dx + dy*dy) + dz*dz in fp64 from
// (X, Y, Z) - the association every test pins - and w the record's fourth word; visit returns whether to stop, and so does the loop.
template <class Visit>
__device__ __forceinline__ bool grid_for_each(const GridView& g, int xa, int xb, int y, int z, double X, double Y, double Z, Visit visit) {
    long long j, pe;
    if (!grid_row_span(g, xa, xb, y, z, j, pe)) return false;
    for (; j < pe; ++j) {
        const uint4 t = g.rec[j];
        const double dx = (double)__uint_as_float(t.x) - X, dy = (double)__uint_as_float(t.y) - Y, dz = (double)__uint_as_float(t.z) - Z;
        if (visit((dx * dx + dy * dy) + dz * dz, t.w)) return true;
    }
    return false;
}

// The query of thread i: its position q in the caller's order (the queries are walked in the order of their own cell keys, qorder, so that
// the lanes of a wave walk the same cells at the same pace and their record loads hit the same cache lines) and its coordinates.
__device__ __forceinline__ long long grid_query(const float* __restrict__ queries, const long long* __restrict__ qorder, long i, float& qx,
                                                float& qy, float& qz) {
    const long long q = qorder ? qorder[i] : i;
    qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
    return q;
}

// ---- nearest.  One thread per query; winner = smallest (d2, original index), a candidate counts iff d2 <= the limit (the best starts at
// (limit, INT_MAX)).
__global__ __launch_bounds__(256) void grid_nearest_kernel(GridView g, const float* __restrict__ queries, const long long* __restrict__ qorder,
                                                           long m, float max_dist, long long* __restrict__ idx, float* __restrict__ dist) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    float qx, qy, qz;
    const long long q = grid_query(queries, qorder, i, qx, qy, qz);
    double best = (double)max_dist * (double)max_dist;
    int best_idx = 0x7fffffff;
    if (grid_finite(qx, qy, qz)) {
        const double X = (double)qx, Y = (double)qy, Z = (double)qz;
        grid_walk_home_first<false>(g, X, Y, Z, [&] { return best; }, [&](int xa, int xb, int y, int z) {
            grid_for_each(g, xa, xb, y, z, X, Y, Z, [&](double d2, unsigned w) {
                const int id = (int)w;
                if (d2 < best || (d2 == best && id < best_idx)) best = d2, best_idx = id;
                return false;
            });
        });
    }
    const bool found = best_idx != 0x7fffffff;
    idx[q] = found ? (long long)best_idx : -1;
    dist[q] = found ? (float)__builtin_sqrt(best) : __builtin_inff();
}

// ---- k nearest (CloudIndex.knn / knn_mean_distance).  One thread per query, walked in qorder as above.  The list is KMAX
// (d2, index) pairs in ascending lexicographic order that only compile-time indices in fully unrolled loops ever touch, so it lives in
// registers (a runtime index would send it to scratch).  For a runtime k <= KMAX the slots 0 .. KMAX-k-1 hold (-1, -1), below any candidate:
// they never move; the slots KMAX-k .. KMAX-1 start as (limit, INT_MAX), nearest's "empty".  The worst entry is always slot KMAX-1: a
// candidate counts iff it is lexicographically smaller than that slot, which drops out as the candidate sinks to its place.
template <int KMAX>
struct GridList { double d2[KMAX]; int idx[KMAX]; };

// A uniform value, moved into a vector register.  The list starts the same in every lane; left to itself the compiler keeps all of it in
// scalar registers up to the first insert - more of them than there are - and spills them.
__device__ __forceinline__ double grid_vreg(double v) { asm("" : "+v"(v)); return v; }
__device__ __forceinline__ int grid_vreg(int v) { asm("" : "+v"(v)); return v; }

// (d2, id) below (e2, ie), lexicographically; bitwise operators: three compares and no branch
__device__ __forceinline__ bool knn_less(double d2, int id, double e2, int ie) { return (d2 < e2) | ((d2 == e2) & (id < ie)); }

// The sink, written from the slots' side: with lo / hi = "the candidate is below slot s-1 / slot s" (monotone in s, the list being sorted),
// slot s takes slot s-1 where lo, the candidate where hi alone, and keeps its entry otherwise - one compare and two selects per slot, two
// lane masks alive at a time.
template <int KMAX>
__device__ __forceinline__ void knn_insert(GridList<KMAX>& l, double d2, int id) {
    bool hi = knn_less(d2, id, l.d2[KMAX - 1], l.idx[KMAX - 1]);
    if (!hi) return;
#pragma unroll
    for (int s = KMAX - 1; s > 0; --s) {
        const bool lo = knn_less(d2, id, l.d2[s - 1], l.idx[s - 1]);
        l.d2[s] = lo ? l.d2[s - 1] : hi ? d2 : l.d2[s];
        l.idx[s] = lo ? l.idx[s - 1] : hi ? id : l.idx[s];
        hi = lo;
    }
    l.d2[0] = hi ? d2 : l.d2[0];
    l.idx[0] = hi ? id : l.idx[0];
}

// The fill both list kernels share: the KMAX slots set up for a runtime k, then the walk, own cell first (it fills the list early, and the rows
// after it are cut to the k-th entry).  On return the live slots KMAX-k .. KMAX-1 hold the min(k, candidates) smallest (d2, index) pairs in
// ascending order and then (limit, INT_MAX); nothing is in them for a query that is not finite.
template <int KMAX>
__device__ __forceinline__ void knn_fill(const GridView& g, float qx, float qy, float qz, int k, float max_dist, GridList<KMAX>& l) {
    const double limit = (double)max_dist * (double)max_dist;
    const int first = KMAX - k;                                                  // the list's first live slot
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
        l.d2[s] = grid_vreg(s < first ? -1.0 : limit);
        l.idx[s] = grid_vreg(s < first ? -1 : 0x7fffffff);
    }
    if (grid_finite(qx, qy, qz)) {
        const double X = (double)qx, Y = (double)qy, Z = (double)qz;
        grid_walk_home_first<true>(g, X, Y, Z, [&] { return l.d2[KMAX - 1]; }, [&](int xa, int xb, int y, int z) {
            grid_for_each(g, xa, xb, y, z, X, Y, Z, [&](double d2, unsigned w) {
                knn_insert(l, d2, (int)w);
                return false;
            });
        });
    }
}

// idx / dist [m, k] (slot j of a row: the j-th smallest (d2, index); unused slots -1 / +inf), count [m], mean [m] (the fp64 mean of the
// row's sqrt(d2), summed in ascending order; +inf for an empty row); idx, dist and mean may each be null.  Every element is written once.
template <int KMAX>
__global__ __launch_bounds__(256) void grid_knn_kernel(GridView g, const float* __restrict__ queries, const long long* __restrict__ qorder, long m,
                                                       int k, float max_dist, long long* __restrict__ idx, float* __restrict__ dist,
                                                       int* __restrict__ count, double* __restrict__ mean) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    float qx, qy, qz;
    const long long q = grid_query(queries, qorder, i, qx, qy, qz);
    const int first = KMAX - k;
    GridList<KMAX> l;
    knn_fill(g, qx, qy, qz, k, max_dist, l);
    int c = 0;
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
        if (l.idx[s] == -1) continue;                                            // below the list's first live slot (read off the slot: no 32 flags kept)
        const bool used = l.idx[s] != 0x7fffffff;
        const double r = __builtin_sqrt(l.d2[s]);
        const long o = (long)q * k + (s - first);
        if (idx) idx[o] = used ? (long long)l.idx[s] : -1;
        if (dist) dist[o] = used ? (float)r : __builtin_inff();
        if (used) {
            sum = sum + r;
            ++c;
        }
    }
    count[q] = c;
    if (mean) mean[q] = c ? sum / (double)c : (double)__builtin_inff();
}

// ---- surface normals (CloudIndex.normals / estimate_normals): the plane through the k nearest neighbours of a query, by the
// eigenvectors of their covariance.  The search is grid_knn_kernel's (knn_fill); the epilogue below runs in the registers the walk leaves
// free: fp64 throughout, no LDS, no atomics, nothing indexed at run time, every output element written once by the query's thread.
#define NORMAL_DEGENERATE 1e-12                      // second eigenvalue / largest at or below this: a collinear neighbourhood, no normal
#define NORMAL_SWEEPS 16                             // cyclic Jacobi sweeps at most (a 3 x 3 matrix needs 4 to 7)

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix; r is the third axis (arp / arq: its entries against p / q) and
// v*p / v*q are columns p and q of the eigenvector matrix.  An off-diagonal entry that is exactly 0, or that no longer changes either of its
// two diagonal entries when added to them a hundred times over (below 2^-59 of both), is set to 0 without a rotation; false then.
__device__ __forceinline__ bool jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return false;
    const double g = 100.0 * fabs(apq);
    if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
        apq = 0.0;
        return false;
    }
    const double theta = (aqq - app) / (2.0 * apq);                              // (overflows to +-inf for a tiny apq: t = 0, the entry goes)
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const double p0 = v0p, q0 = v0q, p1 = v1p, q1 = v1q, p2 = v2p, q2 = v2q;
    v0p = c * p0 - s * q0, v0q = s * p0 + c * q0;
    v1p = c * p1 - s * q1, v1q = s * p1 + c * q1;
    v2p = c * p2 - s * q2, v2q = s * p2 + c * q2;
    return true;
}

// normal [m, 3] float, curvature [m] float, count [m], mom [m, 9] double (S1 x y z, S2 xx xy xz yy yz zz about the query); normal, curvature
// and mom may each be null.  points: the indexed cloud's original array (a record's fourth word indexes it); viewpoints [m, 3] or null.
template <int KMAX>
__global__ __launch_bounds__(256) void grid_normals_kernel(GridView g, const float* __restrict__ queries, const long long* __restrict__ qorder,
                                                           long m, int k, float max_dist, const float* __restrict__ points,
                                                           const float* __restrict__ viewpoints, float* __restrict__ normal,
                                                           float* __restrict__ curvature, int* __restrict__ count, double* __restrict__ mom) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    float qx, qy, qz;
    const long long q = grid_query(queries, qorder, i, qx, qy, qz);
    GridList<KMAX> l;
    knn_fill(g, qx, qy, qz, k, max_dist, l);
    // the moments about the query, the used slots in ascending order (they are one run of the list; the others read point 0 and add nothing)
    const double X = (double)qx, Y = (double)qy, Z = (double)qz;
    int c = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
        const bool used = (l.idx[s] != -1) & (l.idx[s] != 0x7fffffff);
        const long p = used ? (long)l.idx[s] : 0;
        const double dx = (double)points[3 * p] - X, dy = (double)points[3 * p + 1] - Y, dz = (double)points[3 * p + 2] - Z;
        const double xx = dx * dx, xy = dx * dy, xz = dx * dz, yy = dy * dy, yz = dy * dz, zz = dz * dz;
        sx = used ? sx + dx : sx, sy = used ? sy + dy : sy, sz = used ? sz + dz : sz;
        sxx = used ? sxx + xx : sxx, sxy = used ? sxy + xy : sxy, sxz = used ? sxz + xz : sxz;
        syy = used ? syy + yy : syy, syz = used ? syz + yz : syz, szz = used ? szz + zz : szz;
        c += used ? 1 : 0;
    }
    count[q] = c;
    if (mom) {
        double* o = mom + 9 * (long)q;
        o[0] = sx, o[1] = sy, o[2] = sz, o[3] = sxx, o[4] = sxy, o[5] = sxz, o[6] = syy, o[7] = syz, o[8] = szz;
    }
    if (!normal && !curvature) return;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, curv = __builtin_nanf("");
    if (c >= 3) {                                                                // (a query that is not finite has c = 0)
        const double n = (double)c, mx = sx / n, my = sy / n, mz = sz / n;
        double a00 = sxx / n - mx * mx, a01 = sxy / n - mx * my, a02 = sxz / n - mx * mz;
        double a11 = syy / n - my * my, a12 = syz / n - my * mz, a22 = szz / n - mz * mz;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
        for (int sweep = 0; sweep < NORMAL_SWEEPS; ++sweep) {
            bool turned = jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            turned |= jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            turned |= jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
            if (!turned) break;
        }
        // l0 <= l1 <= l2; the eigenvector of l0 is the column of the smallest diagonal entry (the lowest axis on a tie)
        const bool c0 = a00 <= a11 && a00 <= a22, c1 = !c0 && a11 <= a22;
        const double l0 = c0 ? a00 : c1 ? a11 : a22, l2 = fmax(fmax(a00, a11), a22);
        const double l1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));
        if (l2 > 0.0 && l1 > NORMAL_DEGENERATE * l2) {
            double ex = c0 ? v00 : c1 ? v01 : v02, ey = c0 ? v10 : c1 ? v11 : v12, ez = c0 ? v20 : c1 ? v21 : v22;
            const double len = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
            ex = ex / len, ey = ey / len, ez = ez / len;
            // canonical sign: the component of largest magnitude is positive (the lowest axis on a tie) ...
            const double ax = fabs(ex), ay = fabs(ey), az = fabs(ez);
            const double lead = (ax >= ay && ax >= az) ? ex : ay >= az ? ey : ez;
            bool flip = lead < 0.0;
            if (viewpoints) {                                                    // ... unless a finite viewpoint says which side the surface was seen from
                const float vx = viewpoints[3 * q], vy = viewpoints[3 * q + 1], vz = viewpoints[3 * q + 2];
                if (grid_finite(vx, vy, vz)) {
                    const double sg = flip ? -1.0 : 1.0;
                    const double dot = ((sg * ex) * ((double)vx - X) + (sg * ey) * ((double)vy - Y)) + (sg * ez) * ((double)vz - Z);
                    flip = flip != (dot < 0.0);
                }
            }
            nx = (float)(flip ? -ex : ex), ny = (float)(flip ? -ey : ey), nz = (float)(flip ? -ez : ez);
            curv = (float)(fmax(l0, 0.0) / ((l0 + l1) + l2));
        }
    }
    if (normal) normal[3 * q] = nx, normal[3 * q + 1] = ny, normal[3 * q + 2] = nz;
    if (curvature) curvature[q] = curv;
}

// ---- the number of indexed points within a radius: d2 <= double(radius)^2, inclusive.  The bound is constant and no row stops the walk.
__global__ __launch_bounds__(256) void grid_count_within_kernel(GridView g, const float* __restrict__ queries, const long long* __restrict__ qorder,
                                                                long m, float radius, int* __restrict__ count) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    float qx, qy, qz;
    const long long q = grid_query(queries, qorder, i, qx, qy, qz);
    const double limit = (double)radius * (double)radius;
    int c = 0;
    if (grid_finite(qx, qy, qz)) {
        const double X = (double)qx, Y = (double)qy, Z = (double)qz;
        grid_walk_rows(g, grid_home(g, X, Y, Z), [=] { return limit; }, [&](int xa, int xb, int y, int z) {
            return grid_for_each(g, xa, xb, y, z, X, Y, Z, [&](double d2, unsigned) {
                c += d2 <= limit ? 1 : 0;
                return false;
            });
        });
    }
    count[q] = c;
}

// ---- greedy radius thinning (cloud_eval.radius_thin): the maximal independent set of the radius graph under a visiting order,
// what the sequential "a point that is still in the set stays and removes everybody within the radius" loop of the DTU script yields.  The
// cloud is indexed in VISITING order, so the fourth word of a record is the point's rank and state[] is indexed by rank.  A round looks,
// for every undecided point, at its neighbours of lower rank with d2 <= limit: one of them KEPT -> REMOVED (the walk stops there); else one
// of them UNDECIDED -> no change; else -> KEPT.  States only ever move from UNDECIDED to their final value, so the round updates state[]
// in place with plain byte loads and stores: a reader that sees a stale UNDECIDED waits a round, one that sees a final value sees the
// right one.  The fixed point does not depend on the schedule; only the number of rounds may.  (state is read and written by the same
// launch: neither const nor __restrict__.)
#define THIN_UNDECIDED 0
#define THIN_KEPT 1
#define THIN_REMOVED 2

// One thread per entry of the active list (sorted positions, ascending: the lanes of a wave sit in the same cells; NULL: 0 .. m-1).  The walk
// runs against the fixed limit radius^2 over the neighbours of lower rank (the rank is in the record: tested first, before d2 is needed, and
// the state byte is loaded last) and stops at the first KEPT one; wait: one of them is UNDECIDED.
__global__ __launch_bounds__(256) void grid_thin_round_kernel(GridView g, const int* __restrict__ active, long m, float radius,
                                                              unsigned char* state) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const uint4 me = g.rec[active ? (long)active[i] : i];
    const unsigned rank = me.w;
    if (state[rank] != THIN_UNDECIDED) return;                                   // decided since the list was compacted
    const double limit = (double)radius * (double)radius;
    const double X = (double)__uint_as_float(me.x), Y = (double)__uint_as_float(me.y), Z = (double)__uint_as_float(me.z);
    bool kept_near = false, wait = false;
    grid_walk_rows(g, grid_home(g, X, Y, Z), [=] { return limit; }, [&](int xa, int xb, int y, int z) {
        return kept_near = grid_for_each(g, xa, xb, y, z, X, Y, Z, [&](double d2, unsigned w) {
            if (w >= rank || !(d2 <= limit)) return false;                       // later in the visiting order, the point itself, or too far
            const unsigned char s = state[w];
            wait |= s == THIN_UNDECIDED;
            return s == THIN_KEPT;
        });
    });
    if (kept_near) state[rank] = THIN_REMOVED;
    else if (!wait) state[rank] = THIN_KEPT;
}

// ---- the active list's compaction: compact.hpp's count / scan / emit with the predicate "still undecided"; the list keeps its order
__device__ __forceinline__ bool thin_undecided(const uint4* __restrict__ rec, const int* __restrict__ active, long m,
                                               const unsigned char* __restrict__ state, long i) {
    return i < m && state[rec[active ? (long)active[i] : i].w] == THIN_UNDECIDED;
}

__global__ __launch_bounds__(256) void thin_count_kernel(const uint4* __restrict__ rec, const int* __restrict__ active, long m,
                                                         const unsigned char* __restrict__ state, unsigned* __restrict__ partials) {
    compact_count<GRID_TILE>(compact_seg<GRID_TILE, long>(), [=](long i) { return thin_undecided(rec, active, m, state, i); }, partials,
                             blockIdx.x);
}

__global__ __launch_bounds__(1024) void thin_scan_kernel(const unsigned* __restrict__ partials, long np, long long* __restrict__ offsets,
                                                         long long* __restrict__ total) {
    const long long t = compact_scan(partials, np, offsets);
    if (threadIdx.x == 0) *total = t;
}

__global__ __launch_bounds__(256) void thin_emit_kernel(const uint4* __restrict__ rec, const int* __restrict__ active, long m,
                                                        const unsigned char* __restrict__ state, const long long* __restrict__ offsets,
                                                        int* __restrict__ out) {
    const auto set = [=](long i) { return thin_undecided(rec, active, m, state, i); };
    compact_emit<GRID_TILE>(compact_seg<GRID_TILE, long>(), set, offsets, blockIdx.x, [=](long p, long long r) {
        if (r < m) out[r] = active ? active[p] : (int)p;                         // (never past the list's own length: what the caller allocated)
    });
}

// ---- entry points.  Sizes: negative -> CER_EINVAL, 2^31 and beyond -> CER_ESHAPE, zero -> nothing to do (CER_OK, nothing launched, before
// the pointers are looked at); then null pointers -> CER_EINVAL.
static int grid_size_check(long n) {
    if (n < 0) return CER_EINVAL;
    if (n >= 0x80000000L) return CER_ESHAPE;
    return CER_OK;
}
static unsigned grid_blocks(long n, long per) { return (unsigned)((n + per - 1) / per); }

extern "C" long cer_grid_partials(long n) {
    const int rc = grid_size_check(n);
    return rc != CER_OK ? rc : (n + GRID_TILE - 1) / GRID_TILE;
}

extern "C" int cer_grid_keys_f32(const float* points, long n, const double* origin, double cell, int clamp, long long* keys, int* flag,
                                 void* stream) {
    const int rc = grid_size_check(n);
    if (rc != CER_OK) return rc;
    if (!cer_frame_ok(origin, cell)) return CER_EINVAL;
    if (n == 0) return CER_OK;
    if (!points || !keys || (!clamp && !flag)) return CER_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (!clamp && hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(grid_keys_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, st, points, n, origin[0], origin[1], origin[2], cell, clamp, keys,
                       flag);
    CER_RETURN_IF_LAUNCH_FAILED();
    if (!clamp) {                                    // the one answer this call owes its caller: was every cell coordinate inside the key range
        int raised = 0;
        hipError_t e = hipMemcpyAsync(&raised, flag, sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return (int)e;
        if (raised) return CER_ESHAPE;
    }
    return CER_OK;
}

extern "C" int cer_grid_pack_f32(const float* points, const long long* order, long n, void* records, void* stream) {
    const int rc = grid_size_check(n);
    if (rc != CER_OK) return rc;
    if (n == 0) return CER_OK;
    if (!points || !order || !records) return CER_EINVAL;
    if ((uintptr_t)records & 15) return CER_EALIGN;
    hipLaunchKernelGGL(grid_pack_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, points, order, n, (uint4*)records);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_grid_cells_count_i64(const long long* keys, long n, unsigned int* partials, long long* offsets, long long* totals,
                                        void* stream) {
    const int rc = grid_size_check(n);
    if (rc != CER_OK) return rc;
    if (n == 0) return CER_OK;
    if (!keys || !partials || !offsets || !totals) return CER_EINVAL;
    const long np = (n + GRID_TILE - 1) / GRID_TILE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grid_count_kernel, dim3((unsigned)np), dim3(256), 0, st, keys, n, partials);
    CER_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(grid_scan_kernel, dim3(1), dim3(1024), 0, st, partials, np, keys, n, offsets, totals);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_grid_cells_i64(const long long* keys, long n, const long long* offsets, long long ncells, long long* cell_keys,
                                  long long* cell_start, void* stream) {
    const int rc = grid_size_check(n);
    if (rc != CER_OK) return rc;
    if (ncells < 0) return CER_EINVAL;
    if (ncells > n) return CER_ESHAPE;               // more cells than points: not what the count pass found
    if (n == 0 || ncells == 0) return CER_OK;        // (no real key: cell_start[0] is the caller's to zero)
    if (!keys || !offsets || !cell_keys || !cell_start) return CER_EINVAL;
    hipLaunchKernelGGL(grid_emit_kernel, dim3(grid_blocks(n, GRID_TILE)), dim3(256), 0, (hipStream_t)stream, keys, n, offsets, ncells, cell_keys,
                       cell_start);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

// what every search checks, in the order the tests pin: the three sizes; frame and reach -> CER_EINVAL; more cells than records, !shape_ok,
// too many rings -> CER_ESHAPE; an empty side -> CER_OK (0: nothing to launch); null pointers; alignment.  Else -> the walk's rings (>= 1),
// and g is the index as the kernels take it.
static int grid_search_rings(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells,
                             const double* origin, double cell, long m, float reach, bool reach_ok, bool shape_ok, bool pointers_ok,
                             GridView& g) {
    int rc = grid_size_check(n);
    if (rc == CER_OK) rc = grid_size_check(m);
    if (rc == CER_OK) rc = grid_size_check(ncells);
    if (rc != CER_OK) return rc;
    if (!cer_frame_ok(origin, cell) || !reach_ok) return CER_EINVAL;
    if (ncells > n || !shape_ok) return CER_ESHAPE;
    const double rings = ceil((double)reach / cell);
    if (!(rings <= (double)GRID_MAX_RINGS)) return CER_ESHAPE;
    if (m == 0 || n == 0 || ncells == 0) return CER_OK;
    if (!records || !cell_keys || !cell_start || !pointers_ok) return CER_EINVAL;
    if ((uintptr_t)records & 15) return CER_EALIGN;
    g = {(const uint4*)records, cell_keys, cell_start, ncells, origin[0], origin[1], origin[2], cell, (int)rings + 1};
    return g.rings;
}

// the list kernels' three widths: launch(K) with K the integral constant 8, 16 or 32, the narrowest that holds k
template <class Launch>
static void knn_dispatch(int k, Launch launch) {
    if (k <= 8) launch(std::integral_constant<int, 8>());
    else if (k <= 16) launch(std::integral_constant<int, 16>());
    else launch(std::integral_constant<int, 32>());
}

extern "C" int cer_grid_nearest_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells,
                                    const double* origin, double cell, const float* queries, const long long* qorder, long m, float max_dist,
                                    long long* idx, float* dist, void* stream) {
    GridView g;
    const int rings = grid_search_rings(records, n, cell_keys, cell_start, ncells, origin, cell, m, max_dist, max_dist >= 0.0f, true,
                                        queries && idx && dist, g);
    if (rings <= 0) return rings;                            // (an empty target: the caller fills idx = -1, dist = +inf)
    hipLaunchKernelGGL(grid_nearest_kernel, dim3(grid_blocks(m, 256)), dim3(256), 0, (hipStream_t)stream, g, queries, qorder, m, max_dist, idx,
                       dist);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

// k < 1 joins the reach's CER_EINVAL, k > CER_KNN_MAX the shape's CER_ESHAPE, a null count the null pointers' CER_EINVAL
extern "C" int cer_grid_knn_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells,
                                const double* origin, double cell, const float* queries, const long long* qorder, long m, int k, float max_dist,
                                long long* idx, float* dist, int* count, double* mean, void* stream) {
    GridView g;
    const int rings = grid_search_rings(records, n, cell_keys, cell_start, ncells, origin, cell, m, max_dist, max_dist >= 0.0f && k >= 1,
                                        k <= CER_KNN_MAX, queries && count, g);
    if (rings <= 0) return rings;                            // (an empty side: the caller fills idx = -1, dist = mean = +inf, count = 0)
    knn_dispatch(k, [&](auto K) {
        hipLaunchKernelGGL(grid_knn_kernel<decltype(K)::value>, dim3(grid_blocks(m, 256)), dim3(256), 0, (hipStream_t)stream, g, queries, qorder, m,
                           k, max_dist, idx, dist, count, mean);
    });
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

// cer_grid_knn_f32's checks, with points beside count among the pointers that may not be null (normal, curvature, mom and viewpoints may)
extern "C" int cer_grid_normals_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells,
                                    const double* origin, double cell, const float* queries, const long long* qorder, long m, int k,
                                    float max_dist, const float* points, const float* viewpoints, float* normal, float* curvature, int* count,
                                    double* mom, void* stream) {
    GridView g;
    const int rings = grid_search_rings(records, n, cell_keys, cell_start, ncells, origin, cell, m, max_dist, max_dist >= 0.0f && k >= 1,
                                        k <= CER_KNN_MAX, queries && count && points, g);
    if (rings <= 0) return rings;                            // (an empty side: the caller fills normal = 0, curvature = NaN, count = 0, mom = 0)
    knn_dispatch(k, [&](auto K) {
        hipLaunchKernelGGL(grid_normals_kernel<decltype(K)::value>, dim3(grid_blocks(m, 256)), dim3(256), 0, (hipStream_t)stream, g, queries, qorder,
                           m, k, max_dist, points, viewpoints, normal, curvature, count, mom);
    });
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_grid_count_within_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells,
                                         const double* origin, double cell, const float* queries, const long long* qorder, long m,
                                         float radius, int* count, void* stream) {
    GridView g;
    const int rings = grid_search_rings(records, n, cell_keys, cell_start, ncells, origin, cell, m, radius, radius >= 0.0f, true,
                                        queries && count, g);
    if (rings <= 0) return rings;                            // (an empty side: the caller fills count = 0)
    hipLaunchKernelGGL(grid_count_within_kernel, dim3(grid_blocks(m, 256)), dim3(256), 0, (hipStream_t)stream, g, queries, qorder, m, radius,
                       count);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_grid_thin_round_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells,
                                       const double* origin, double cell, const int* active, long n_active, float radius,
                                       unsigned char* state, void* stream) {
    GridView g;
    const int rings = grid_search_rings(records, n, cell_keys, cell_start, ncells, origin, cell, n_active, radius,
                                        radius > 0.0f && cer_is_finite((double)radius), n_active <= n, state != nullptr, g);
    if (rings <= 0) return rings;                            // (active may be NULL: the list 0 .. n_active-1)
    hipLaunchKernelGGL(grid_thin_round_kernel, dim3(grid_blocks(n_active, 256)), dim3(256), 0, (hipStream_t)stream, g, active, n_active, radius,
                       state);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_grid_thin_compact_i32(const void* records, long n, const unsigned char* state, const int* active, long n_active,
                                         unsigned int* partials, long long* offsets, int* out, long long* total, void* stream) {
    int rc = grid_size_check(n);
    if (rc == CER_OK) rc = grid_size_check(n_active);
    if (rc != CER_OK) return rc;
    if (n_active > n) return CER_ESHAPE;
    if (n_active == 0) return CER_OK;                // (an empty list: *total is the caller's to zero)
    if (!records || !state || !partials || !offsets || !out || !total) return CER_EINVAL;
    if ((uintptr_t)records & 15) return CER_EALIGN;
    if (out == active) return CER_EINVAL;            // the emit pass reads the list while it writes the new one
    const long np = (n_active + GRID_TILE - 1) / GRID_TILE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(thin_count_kernel, dim3((unsigned)np), dim3(256), 0, st, (const uint4*)records, active, n_active, state, partials);
    CER_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(thin_scan_kernel, dim3(1), dim3(1024), 0, st, partials, np, offsets, total);
    CER_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(thin_emit_kernel, dim3((unsigned)np), dim3(256), 0, st, (const uint4*)records, active, n_active, state, offsets, out);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}
