// The sparse uniform grid's view and row walk, the one copy (cloud_eval.hip: the searches over a cloud's points and the thinning;
// mesh_dist.hip: the search over a mesh's triangles).  The index exists only as sorted keys and a table of the occupied cells; what is
// searched in a cell - 16-byte point records, or a run of face ids - is the caller's.  The text below moved here unchanged from
// cloud_eval.hip, whose device code is the same before and after (profiles/mesh_dist_asm_identity.txt).
//
// Key layout: (z + B) << 42 | (y + B) << 21 | (x + B), B = CER_GRID_COORD_LIMIT - 1, cell coordinates in -B .. B: every field is at most
// 2^21 - 2, so no key reaches the sentinel (2^63 - 1, all 63 bits set) and key(x + 1, y, z) = key(x, y, z) + 1 never carries.  x is the
// lowest field: the cells x0 .. x1 of one (y, z) row are a contiguous run of the cell table, found with two binary searches.
#pragma once
#include "common.hpp"

#define GRID_B (CER_GRID_COORD_LIMIT - 1)

__device__ __forceinline__ long long grid_key(int x, int y, int z) {
    return ((long long)(z + GRID_B) << 42) | ((long long)(y + GRID_B) << 21) | (long long)(x + GRID_B);
}

__device__ __forceinline__ long grid_lower_bound(const long long* __restrict__ a, long lo, long hi, long long k) {     // first i in [lo, hi) with a[i] >= k
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (a[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- what every search reads of the index, by value: the sorted records, the cell table, the frame, and the rings of rows a walk covers
struct GridView {
    const uint4* rec;
    const long long* cell_keys;
    const long long* cell_start;
    long ncells;
    double ox, oy, oz, cell;
    int rings;
};

// ---- the row walk under every search.  Exactness does not rest on the key arithmetic: a cell is skipped only when the TRUE
// bounds of the points it can hold prove that none of them can matter.  A target point in cell c of an axis has a computed u in [c, c + 1);
// u carries two fp64 roundings (relative 2^-52 of a magnitude below 2^21 + GRID_MAX_RINGS: absolute below 2e-9 cells), and so does the
// query's.  The per-axis gap between the query and any point of the cell is therefore at least (c - uq - GRID_EPS) cells above the query,
// (uq - (c + 1) - GRID_EPS) cells below it, with GRID_EPS = 1e-6 hundreds of times that error.  Rows and cells whose squared gap exceeds
// the caller's bound are skipped - strictly: for the search's best distance so far a tie on d2 with a lower index must still be seen, for
// the thinning's fixed radius^2 d2 == limit is a neighbour; the enumeration itself covers ceil(reach / cell) + 1 rings, one more than the
// mathematics needs.  The k-nearest search hands in the d2 of its k-th entry so far (the limit until k candidates are in): a skipped cell
// holds only points strictly beyond it, which cannot enter the list, and a tie on the k-th distance with a lower index is still seen (the
// normals' search, grid_normals_kernel, is that search); the count within a radius hands in the fixed radius^2 as the thinning does.
#define GRID_EPS 1e-6

// gap, in cells, between coordinate u and the points of cell c of that axis (0 when u is inside)
__device__ __forceinline__ double grid_gap(double u, double c) {
    const double g = u < c ? c - u - GRID_EPS : u - (c + 1.0) - GRID_EPS;
    return g > 0.0 ? g : 0.0;
}

// [pb, pe): the sorted records of cells xa .. xb of row (y, z) - one run, found with two binary searches; false when the row holds none
__device__ __forceinline__ bool grid_row_span(const GridView& g, int xa, int xb, int y, int z, long long& pb, long long& pe) {
    const long long ka = grid_key(xa, y, z), kb = grid_key(xb, y, z) + 1;
    const long a = grid_lower_bound(g.cell_keys, 0, g.ncells, ka);
    if (a == g.ncells || g.cell_keys[a] >= kb) return false;
    const long b = grid_lower_bound(g.cell_keys, a + 1, g.ncells, kb);
    pb = g.cell_start[a], pe = g.cell_start[b];
    return true;
}

// a point in cell units, and its cell: doubles, the point may lie anywhere
struct GridHome { double ux, uy, uz, fx, fy, fz; };
__device__ __forceinline__ GridHome grid_home(const GridView& g, double X, double Y, double Z) {
    const double ux = (X - g.ox) / g.cell, uy = (Y - g.oy) / g.cell, uz = (Z - g.oz) / g.cell;
    return {ux, uy, uz, floor(ux), floor(uy), floor(uz)};
}

// The rows of cells around the point of h that can hold a point within sqrt(bound()), near rows first (0, +1, -1, +2, -2, ... in z, then
// in y): row(xa, xb, y, z) gets the cells xa .. xb of row (y, z) and returns whether to stop.  bound() is read anew at every test.  Cell
// coordinates are doubles until they are clamped; farther than the rings from the key range: no row at all.
template <class Bound, class Row>
__device__ __forceinline__ void grid_walk_rows(const GridView& g, const GridHome& h, Bound bound, Row row) {
    const double ux = h.ux, uy = h.uy, uz = h.uz, fx = h.fx, fy = h.fy, fz = h.fz, cell = g.cell, B = (double)GRID_B, R = (double)g.rings;
    const int rings = g.rings;
    const double xlo = fmax(fx - R, -B), xhi = fmin(fx + R, B), ylo = fmax(fy - R, -B), yhi = fmin(fy + R, B);
    const double zlo = fmax(fz - R, -B), zhi = fmin(fz + R, B);
    if (!(xlo <= xhi && ylo <= yhi && zlo <= zhi)) return;
    const int cy = (int)fmin(fmax(fy, -B), B), cz = (int)fmin(fmax(fz, -B), B);
    for (int iz = 0; iz <= 2 * rings; ++iz) {
        const int z = cz + ((iz & 1) ? (iz + 1) / 2 : -(iz / 2));
        if ((double)z < zlo || (double)z > zhi) continue;
        const double gz = grid_gap(uz, (double)z) * cell, gz2 = gz * gz;
        if (gz2 > bound()) continue;
        for (int iy = 0; iy <= 2 * rings; ++iy) {
            const int y = cy + ((iy & 1) ? (iy + 1) / 2 : -(iy / 2));
            if ((double)y < ylo || (double)y > yhi) continue;
            const double gy = grid_gap(uy, (double)y) * cell, g2 = gz2 + gy * gy, b2 = bound();
            if (g2 > b2) continue;
            // cells of the row whose gap along x can be within sqrt(b2 - g2): c + 1 > ux - e and c <= ux + e, e padded by 1e-3 cells
            const double e = __builtin_sqrt(b2 - g2) / cell + 1e-3;
            const double xa = fmax(floor(ux - e), xlo), xb = fmin(floor(ux + e), xhi);
            if (xa > xb) continue;
            if (row((int)xa, (int)xb, y, z)) return;
        }
    }
}

// The walk of a search whose bound shrinks as it finds: scan(xa, xb, y, z) = "visit these cells" gets the point's own cell first - in a dense
// cloud it holds what the search is after, and every row after it is cut to what can still matter - and then the rows, the own row as the
// cells on either side of the own cell, so every record is visited once.  kOneSite: every row's cells go through one call of scan in a
// two-trip loop that is not unrolled, so a large scan (the k-nearest insert is KMAX unrolled steps) exists twice in a kernel, not four
// times; otherwise the sides are two calls beside the plain row's, which a small scan repays where rows are many.
template <bool kOneSite, class Bound, class Scan>
__device__ __forceinline__ void grid_walk_home_first(const GridView& g, double X, double Y, double Z, Bound bound, Scan scan) {
    const GridHome h = grid_home(g, X, Y, Z);
    const double B = (double)GRID_B;
    const bool home = fabs(h.fx) <= B && fabs(h.fy) <= B && fabs(h.fz) <= B;
    if (home) scan((int)h.fx, (int)h.fx, (int)h.fy, (int)h.fz);
    grid_walk_rows(g, h, bound, [&](int xa, int xb, int y, int z) {
        const bool own = home && (double)y == h.fy && (double)z == h.fz;         // the own row: its own cell is done
        const int hx = (int)h.fx;                                                // (read only where own)
        if constexpr (kOneSite) {
            int a0 = xa, b0 = xb, a1 = 1, b1 = 0;
            if (own) b0 = min(hx - 1, xb), a1 = max(hx + 1, xa), b1 = xb;
#pragma unroll 1
            for (int part = 0; part < 2; ++part) {
                const int a = part ? a1 : a0, b = part ? b1 : b0;
                if (a <= b) scan(a, b, y, z);
            }
        } else if (own) {
            if (xa < hx) scan(xa, hx - 1, y, z);
            if (xb > hx) scan(hx + 1, xb, y, z);
        } else scan(xa, xb, y, z);
        return false;
    });
}
