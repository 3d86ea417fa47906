// Surface mesh of a fused scan on the device (cer-mvs_amd/mesh.py, scan.py reconstruct_scan(mesh=...)): the fused depth maps
// integrated into a dense volume of truncated signed distances (one value and one count per NODE of a regular grid), and marching tetrahedra
// on that volume - the Kuhn split of every cell into the six tetrahedra around its 0-7 diagonal.
//
// Order: a vertex lives on a lattice edge (node a, d = 1..7 as a bit vector, from a to a + d) and has the slot node_index * 8 + d; a face has
// the slot (cell_index * 6 + tet) * 2 + s.  Every slot is a 0/1 flag at a fixed position: vertices and faces leave in slot order through
// compact.hpp's count / scan / emit, twice.  No atomics, no output cursor: the same bytes on every run, whatever the schedule.
//
// All coordinate arithmetic is fp64 with every association written out and no fused multiply-add (-ffp-contract=off): tests/mesh_reference.py
// restates it in numpy and the GPU tests compare bits.
//
// Per-vertex attributes (ABI 1180; tests/mesh_attr_reference.py): colours gathered from the views that see a vertex, and
// area-weighted normals from the faces of any indexed triangle mesh, under the same arithmetic rules.
//
// Cleaning (ABI 1190; tests/mesh_clean_reference.py): the connected components of any indexed triangle mesh by min-label
// sweeps without atomics or data-dependent waiting, and the sub-mesh of a face mask through the same ordered compaction.
//
// Simplification (ABI 1200; tests/mesh_simplify_reference.py): vertex clustering on the cells of cloud_eval.py's CloudIndex -
// one thread per cluster sums its members (and their faces' plane quadrics) in member order, faces are remapped, rotated and deduplicated
// through two stable sorts, and what survives leaves through the selection above.
//
// Edges and smoothing (ABI 1210; tests/mesh_smooth_reference.py): the unique-neighbour list of every vertex with a count per
// direction - six keys per face, the caller's sort, the ordered compaction over the heads of the runs - and Taubin / Laplacian smoothing,
// one gather kernel per step over that list.
#include "common.hpp"
#include "compact.hpp"

#define MESH_TILE CER_MESH_TILE                      // slots per block of the count and emit passes

// ---- the case table, derived (not copied): for tet t and the 4-bit mask of its inside corners in listing order, the number of triangles and
// up to six lattice edges, 6 bits each: (lower corner << 3) | d.  Triangle s takes edges 3 s .. 3 s + 2.
struct MeshTable {
    unsigned long long tri[6][16];                   // bits 0-35: six edge codes; bits 36-37: the number of triangles
    unsigned short corners[6];                       // the tet's four corners in listing order, 3 bits each
};

constexpr int MESH_TETS[6][4] = {{0, 1, 3, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 6, 4, 7}, {0, 4, 5, 7}, {0, 5, 1, 7}};

constexpr int mesh_axis(int corner, int a) { return (corner >> a) & 1; }
// the integer determinant of [B - A, C - A, D - A] on corner offsets
constexpr int mesh_det(int A, int B, int C, int D) {
    const int u[3] = {mesh_axis(B, 0) - mesh_axis(A, 0), mesh_axis(B, 1) - mesh_axis(A, 1), mesh_axis(B, 2) - mesh_axis(A, 2)};
    const int v[3] = {mesh_axis(C, 0) - mesh_axis(A, 0), mesh_axis(C, 1) - mesh_axis(A, 1), mesh_axis(C, 2) - mesh_axis(A, 2)};
    const int w[3] = {mesh_axis(D, 0) - mesh_axis(A, 0), mesh_axis(D, 1) - mesh_axis(A, 1), mesh_axis(D, 2) - mesh_axis(A, 2)};
    return u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0]);
}
// the lattice edge between corners X and Y of a Kuhn tet: one is the other plus a bit vector
constexpr unsigned long long mesh_edge(int X, int Y) { return (unsigned long long)(((X & Y) << 3) | (X ^ Y)); }
constexpr unsigned long long mesh_pack3(unsigned long long e0, unsigned long long e1, unsigned long long e2, bool swap) {
    return swap ? (e0 | e2 << 6 | e1 << 12) : (e0 | e1 << 6 | e2 << 12);
}
constexpr MeshTable mesh_make_table() {
    MeshTable T = {};
    for (int t = 0; t < 6; ++t) {
        T.corners[t] = (unsigned short)(MESH_TETS[t][0] | MESH_TETS[t][1] << 3 | MESH_TETS[t][2] << 6 | MESH_TETS[t][3] << 9);
        for (int m = 0; m < 16; ++m) {
            int ins[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int l = 0; l < 4; ++l) {
                if ((m >> l) & 1) ins[ni++] = MESH_TETS[t][l];
                else out[no++] = MESH_TETS[t][l];
            }
            unsigned long long code = 0;
            if (ni == 1) {
                const int A = ins[0], B = out[0], C = out[1], D = out[2];
                code = mesh_pack3(mesh_edge(A, B), mesh_edge(A, C), mesh_edge(A, D), mesh_det(A, B, C, D) < 0) | 1ull << 36;
            } else if (ni == 3) {
                const int A = out[0], B = ins[0], C = ins[1], D = ins[2];
                code = mesh_pack3(mesh_edge(A, B), mesh_edge(A, C), mesh_edge(A, D), mesh_det(A, B, C, D) > 0) | 1ull << 36;
            } else if (ni == 2) {
                const int A = ins[0], B = ins[1], C = out[0], D = out[1];
                const bool swap = mesh_det(A, B, C, D) < 0;
                const unsigned long long q0 = mesh_edge(A, C), q1 = mesh_edge(A, D), q2 = mesh_edge(B, D), q3 = mesh_edge(B, C);
                code = mesh_pack3(q0, q1, q2, swap) | mesh_pack3(q0, q2, q3, swap) << 18 | 2ull << 36;
            }
            T.tri[t][m] = code;
        }
    }
    return T;
}
__constant__ MeshTable mesh_table = mesh_make_table();

struct MeshGrid {
    double ox, oy, oz, voxel;
    int nx, ny, nz;
};

// linear index n of a lattice [., ny, nx], x fastest (the nodes, or the cells with nx - 1 and ny - 1) -> (i, j, k)
__device__ __forceinline__ void mesh_split(unsigned n, unsigned nx, unsigned ny, unsigned& i, unsigned& j, unsigned& k) {
    const unsigned row = n / nx;
    i = n - row * nx;
    k = row / ny;
    j = row - k * ny;
}

// world point -> camera -> homogeneous pixel (ux, uy, uz) of the view with camera doubles c: the one projection of the integration and of the
// vertex colours, every association written out.  The pixel is (ux / uz, uy / uz); the callers divide and test.
__device__ __forceinline__ void mesh_project(const double* c, double px, double py, double pz, double& ux, double& uy, double& uz) {
    const double cx = ((c[9] * px + c[10] * py) + c[11] * pz) + c[12];
    const double cy = ((c[13] * px + c[14] * py) + c[15] * pz) + c[16];
    const double cz = ((c[17] * px + c[18] * py) + c[19] * pz) + c[20];
    ux = (c[0] * cx + c[1] * cy) + c[2] * cz;
    uy = (c[3] * cx + c[4] * cy) + c[5] * cz;
    uz = (c[6] * cx + c[7] * cy) + c[8] * cz;
}

// ---- integration: one thread owns a node for the whole view loop, x along the lanes.  cams: per view CER_CLOUD_CAM_DOUBLES doubles =
// K [9] | rows 0-2 of E [12] (the float32 matrices promoted on the host): wave-uniform, scalar loads.  views: n_views DEVICE ints.
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const float* __restrict__ depths, const unsigned char* __restrict__ masks,
                                                             const double* __restrict__ cams, int N, int h, int w,
                                                             const int* __restrict__ views, int n_views, MeshGrid g, double trunc,
                                                             unsigned nodes, float* __restrict__ tsdf, int* __restrict__ weight) {
    const unsigned n = blockIdx.x * 256u + threadIdx.x;
    if (n >= nodes) return;
    unsigned i, j, k;
    mesh_split(n, (unsigned)g.nx, (unsigned)g.ny, i, j, k);
    const double px = g.ox + (double)i * g.voxel, py = g.oy + (double)j * g.voxel, pz = g.oz + (double)k * g.voxel;
    const long P = (long)h * w;
    const double dw = (double)w, dh = (double)h;
    double sum = 0.0;
    int cnt = 0;
    for (int v = 0; v < n_views; ++v) {
        const int view = views[v];
        if (view < 0 || view >= N) continue;                             // (uniform; the caller has checked the list: never taken)
        double ux, uy, uz;
        mesh_project(cams + (long)view * CER_CLOUD_CAM_DOUBLES, px, py, pz, ux, uy, uz);
        const double a = ux / uz + 0.5, b = uy / uz + 0.5;
        if (!(uz > 0.0 && a >= 0.0 && a < dw && b >= 0.0 && b < dh)) continue;       // (NaN fails every comparison)
        const long p = (long)view * P + (long)(int)floor(b) * w + (int)floor(a);
        if (masks && masks[p] == 0) continue;
        const double d = (double)depths[p];
        if (!(d > 0.0 && d - d == 0.0)) continue;                        // finite and positive
        const double sdf = d - uz;
        if (!(sdf >= -trunc)) continue;
        sum += sdf >= trunc ? 1.0 : sdf / trunc;
        ++cnt;
    }
    weight[n] = cnt;
    tsdf[n] = cnt ? (float)(sum / (double)cnt) : 1.0f;
}

// ---- cell pass: cells[cell] = the 8-bit mask of the corners with tsdf < 0 | 0x100 iff all eight corners are valid (weight >= min_weight and
// a finite tsdf).  Cells are [nz - 1, ny - 1, nx - 1], x fastest.
__global__ __launch_bounds__(256) void mesh_cells_kernel(const float* __restrict__ tsdf, const int* __restrict__ weight, int nx, int ny,
                                                         int min_weight, unsigned ncells, unsigned short* __restrict__ cells) {
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    if (c >= ncells) return;
    unsigned i, j, k;
    mesh_split(c, (unsigned)nx - 1, (unsigned)ny - 1, i, j, k);
    const long base = ((long)k * ny + j) * nx + i;
    unsigned m = 0, ok = 1;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const long n = base + (q & 1) + (long)((q >> 1) & 1) * nx + (long)((q >> 2) & 1) * nx * ny;
        const float f = tsdf[n];
        ok &= (unsigned)(weight[n] >= min_weight && f - f == 0.0f);
        m |= (unsigned)(f < 0.0f) << q;
    }
    cells[c] = (unsigned short)(m | ok << 8);
}

struct MeshDims {
    int nx, ny, nz;
    long vslots, fslots;                             // nodes * 8, cells * 12
};

// vertex slot p = node * 8 + d: set iff the endpoints' signs differ and a valid cell contains the edge.  The candidates are the cells that
// have node a as corner o with o & d == 0 (4 / 2 / 1 of them); in such a cell the other endpoint is corner o | d.
__device__ __forceinline__ bool mesh_vertex_set(const unsigned short* __restrict__ cells, const MeshDims& D, long p) {
    if (p >= D.vslots) return false;
    const unsigned d = (unsigned)p & 7u, n = (unsigned)(p >> 3);
    if (d == 0) return false;
    unsigned i, j, k;
    mesh_split(n, (unsigned)D.nx, (unsigned)D.ny, i, j, k);
    bool set = false;
#pragma unroll
    for (unsigned o = 0; o < 8; ++o) {
        if (o & d) continue;
        const int ci = (int)i - (int)(o & 1), cj = (int)j - (int)((o >> 1) & 1), ck = (int)k - (int)(o >> 2);
        if (ci < 0 || cj < 0 || ck < 0 || ci > D.nx - 2 || cj > D.ny - 2 || ck > D.nz - 2) continue;
        const unsigned m = cells[((long)ck * (D.ny - 1) + cj) * (D.nx - 1) + ci];
        set |= (m >> 8) && (((m >> o) ^ (m >> (o | d))) & 1u);
    }
    return set;
}

// the inside mask of tet t of a cell, in listing order
__device__ __forceinline__ unsigned mesh_tet_mask(unsigned m, unsigned t) {
    const unsigned c = mesh_table.corners[t];
    return ((m >> (c & 7)) & 1u) | ((m >> ((c >> 3) & 7)) & 1u) << 1 | ((m >> ((c >> 6) & 7)) & 1u) << 2 | ((m >> ((c >> 9) & 7)) & 1u) << 3;
}

// face slot q = (cell * 6 + tet) * 2 + s: set iff the cell is valid and its tet has more than s triangles
__device__ __forceinline__ bool mesh_face_set(const unsigned short* __restrict__ cells, const MeshDims& D, long q) {
    if (q >= D.fslots) return false;
    const long cell = q / 12;
    const unsigned r = (unsigned)(q - cell * 12);
    const unsigned m = cells[cell];
    if (!(m >> 8)) return false;
    return (r & 1u) < (unsigned)(mesh_table.tri[r >> 1][mesh_tet_mask(m, r >> 1)] >> 36);
}

// ---- count: grid = vertex blocks then face blocks, one partial each
__global__ __launch_bounds__(256) void mesh_count_kernel(const unsigned short* __restrict__ cells, MeshDims D, unsigned vblocks,
                                                         unsigned* __restrict__ partials) {
    const bool faces = blockIdx.x >= vblocks;                            // (uniform)
    const long seg = compact_seg<MESH_TILE, long>() - (faces ? (long)vblocks * MESH_TILE : 0);
    if (faces) compact_count<MESH_TILE>(seg, [&](long q) { return mesh_face_set(cells, D, q); }, partials, blockIdx.x);
    else compact_count<MESH_TILE>(seg, [&](long p) { return mesh_vertex_set(cells, D, p); }, partials, blockIdx.x);
}

// ---- scan: block 0 the vertex partials -> offsets[0 .. vblocks], totals[0] = nv; block 1 the face partials -> offsets[vblocks + 1 ..],
// totals[1] = nf
__global__ __launch_bounds__(1024) void mesh_scan_kernel(const unsigned* __restrict__ partials, long vblocks, long fblocks,
                                                         long long* __restrict__ offsets, long long* __restrict__ totals) {
    const bool faces = blockIdx.x != 0;
    const long long t = compact_scan(partials + (faces ? vblocks : 0), faces ? fblocks : vblocks, offsets + (faces ? vblocks + 1 : 0));
    if (threadIdx.x == 0) totals[blockIdx.x] = t;
}

// ---- vertex emit: vmap[slot] = the vertex's output index (written for every set slot: the faces read it), and the position if it is below
// the caller's capacity: origin + (idx + (d_a ? t : 0)) * voxel per axis with t = f0 / (f0 - f1), rounded ONCE to float32
__global__ __launch_bounds__(256) void mesh_vertex_emit_kernel(const float* __restrict__ tsdf, const unsigned short* __restrict__ cells,
                                                               MeshDims D, MeshGrid g, const long long* __restrict__ offsets,
                                                               long long capacity, int* __restrict__ vmap, float* __restrict__ vertices) {
    const auto set = [&](long p) { return mesh_vertex_set(cells, D, p); };
    compact_emit<MESH_TILE>(compact_seg<MESH_TILE, long>(), set, offsets, blockIdx.x, [&](long p, long long idx) {
        vmap[p] = (int)idx;
        if (idx >= capacity) return;                                     // (never past what the caller allocated)
        const unsigned d = (unsigned)p & 7u, n = (unsigned)(p >> 3);
        unsigned i, j, k;
        mesh_split(n, (unsigned)D.nx, (unsigned)D.ny, i, j, k);
        const long n1 = (long)n + (d & 1) + (long)((d >> 1) & 1) * D.nx + (long)(d >> 2) * D.nx * D.ny;
        const double f0 = (double)tsdf[n], f1 = (double)tsdf[n1];
        const double t = f0 / (f0 - f1);
        float* o = vertices + idx * 3;
        o[0] = (float)(g.ox + ((double)i + ((d & 1) ? t : 0.0)) * g.voxel);
        o[1] = (float)(g.oy + ((double)j + ((d & 2) ? t : 0.0)) * g.voxel);
        o[2] = (float)(g.oz + ((double)k + ((d & 4) ? t : 0.0)) * g.voxel);
    });
}

// ---- face emit: the three lattice edges of triangle s of the tet -> their vertex slots -> vmap
__global__ __launch_bounds__(256) void mesh_face_emit_kernel(const unsigned short* __restrict__ cells, MeshDims D,
                                                             const long long* __restrict__ offsets, long long capacity,
                                                             const int* __restrict__ vmap, int* __restrict__ faces) {
    const auto set = [&](long q) { return mesh_face_set(cells, D, q); };
    compact_emit<MESH_TILE>(compact_seg<MESH_TILE, long>(), set, offsets, blockIdx.x, [&](long q, long long idx) {
        if (idx >= capacity) return;                                     // (never past what the caller allocated)
        const long cell = q / 12;
        const unsigned r = (unsigned)(q - cell * 12);
        unsigned i, j, k;
        mesh_split((unsigned)cell, (unsigned)D.nx - 1, (unsigned)D.ny - 1, i, j, k);
        const long node = ((long)k * D.ny + j) * D.nx + i;
        const unsigned long long code = mesh_table.tri[r >> 1][mesh_tet_mask(cells[cell], r >> 1)] >> (18 * (r & 1u));
        int* o = faces + idx * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const unsigned c6 = (unsigned)(code >> (6 * e)) & 63u, a = c6 >> 3;
            const long na = node + (a & 1) + (long)((a >> 1) & 1) * D.nx + (long)(a >> 2) * D.nx * D.ny;
            o[e] = vmap[na * 8 + (c6 & 7u)];
        }
    });
}

// ---- vertex colours from the views: one thread owns a vertex for the whole view loop, laid out as tsdf_integrate_kernel is - the view's 21
// camera doubles and its list entry are wave-uniform (scalar loads), depth, mask and colour are gathered per pixel.  The projection is the
// integration's (mesh_project); a view colours the vertex iff it projects inside, the pixel is masked in, its depth is finite
// and positive and |d - uz| <= tol (the occlusion test).  The sample is bilinear over pixel centres at integer coordinates, taps clamped.
__device__ __forceinline__ double mesh_bilinear(const float* __restrict__ plane, long r0, long r1, int x0, int x1, double fx, double fy) {
    const double c00 = (double)plane[r0 + x0], c01 = (double)plane[r0 + x1], c10 = (double)plane[r1 + x0], c11 = (double)plane[r1 + x1];
    const double top = (1.0 - fx) * c00 + fx * c01;
    const double bot = (1.0 - fx) * c10 + fx * c11;
    return (1.0 - fy) * top + fy * bot;
}
__device__ __forceinline__ unsigned char mesh_byte(double sum, double cnt) {
    const double q = (sum / cnt) * 255.0;
    return q >= 255.0 ? (unsigned char)255 : (q > 0.0 ? (unsigned char)q : (unsigned char)0);       // (truncation; NaN fails both: 0)
}
__global__ __launch_bounds__(256) void mesh_vertex_color_kernel(const float* __restrict__ vertices, unsigned nv,
                                                                const float* __restrict__ depths, const unsigned char* __restrict__ masks,
                                                                const float* __restrict__ colors, const double* __restrict__ cams, int N,
                                                                int h, int w, const int* __restrict__ views, int n_views, double tol,
                                                                unsigned char* __restrict__ rgb, int* __restrict__ seen) {
    const unsigned n = blockIdx.x * 256u + threadIdx.x;
    if (n >= nv) return;
    const double px = (double)vertices[3l * n], py = (double)vertices[3l * n + 1], pz = (double)vertices[3l * n + 2];
    const long P = (long)h * w;
    const double dw = (double)w, dh = (double)h;
    double sr = 0.0, sg = 0.0, sb = 0.0;
    int cnt = 0;
    for (int v = 0; v < n_views; ++v) {
        const int view = views[v];
        if (view < 0 || view >= N) continue;                             // (uniform; the caller has checked the list: never taken)
        double ux, uy, uz;
        mesh_project(cams + (long)view * CER_CLOUD_CAM_DOUBLES, px, py, pz, ux, uy, uz);
        const double x = ux / uz, y = uy / uz;
        const double a = x + 0.5, b = y + 0.5;
        if (!(uz > 0.0 && a >= 0.0 && a < dw && b >= 0.0 && b < dh)) continue;       // (NaN fails every comparison)
        const long p = (long)view * P + (long)(int)floor(b) * w + (int)floor(a);
        if (masks && masks[p] == 0) continue;
        const double d = (double)depths[p];
        if (!(d > 0.0 && d - d == 0.0)) continue;                        // finite and positive
        if (!(fabs(d - uz) <= tol)) continue;                            // the occlusion test, inclusive
        const double xf = floor(x), yf = floor(y);                       // x in [-0.5, w - 0.5): xf in -1 .. w - 1
        const double fx = x - xf, fy = y - yf;
        const int xi = (int)xf, yi = (int)yf;
        const int x0 = xi < 0 ? 0 : xi, x1 = xi + 1 > w - 1 ? w - 1 : xi + 1;
        const int y0 = yi < 0 ? 0 : yi, y1 = yi + 1 > h - 1 ? h - 1 : yi + 1;
        const long r0 = (long)y0 * w, r1 = (long)y1 * w;
        const float* plane = colors + (long)view * 3 * P;
        sr += mesh_bilinear(plane, r0, r1, x0, x1, fx, fy);
        sg += mesh_bilinear(plane + P, r0, r1, x0, x1, fx, fy);
        sb += mesh_bilinear(plane + 2 * P, r0, r1, x0, x1, fx, fy);
        ++cnt;
    }
    seen[n] = cnt;
    unsigned char* o = rgb + 3l * n;
    const double k = (double)cnt;
    o[0] = cnt ? mesh_byte(sr, k) : (unsigned char)0;
    o[1] = cnt ? mesh_byte(sg, k) : (unsigned char)0;
    o[2] = cnt ? mesh_byte(sb, k) : (unsigned char)0;
}

// ---- vertex normals from the faces: one thread per vertex walks its corners order[starts[v] .. starts[v + 1] - 1] (a stable sort of the
// corner entries: corner ids 3 * face + corner ascend within a vertex) and adds the faces' (B - A) x (C - A) - twice the area, so the sum is
// area-weighted - in that order.  No atomics.  A corner id or a face index out of range is skipped, never read through.
__global__ __launch_bounds__(256) void mesh_vertex_normals_kernel(const float* __restrict__ vertices, unsigned nv, const int* __restrict__ faces,
                                                                  int corners, const int* __restrict__ starts, const int* __restrict__ order,
                                                                  float* __restrict__ normals) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    int e0 = starts[v], e1 = starts[v + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > corners ? corners : e1;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int e = e0; e < e1; ++e) {
        const int corner = order[e];
        if (corner < 0 || corner >= corners) continue;
        const int* f = faces + (long)(corner / 3) * 3;
        const int ia = f[0], ib = f[1], ic = f[2];
        if ((unsigned)ia >= nv || (unsigned)ib >= nv || (unsigned)ic >= nv) continue;
        const float *A = vertices + 3l * ia, *B = vertices + 3l * ib, *C = vertices + 3l * ic;
        const double ax = (double)A[0], ay = (double)A[1], az = (double)A[2];
        const double ux = (double)B[0] - ax, uy = (double)B[1] - ay, uz = (double)B[2] - az;
        const double wx = (double)C[0] - ax, wy = (double)C[1] - ay, wz = (double)C[2] - az;
        sx += uy * wz - uz * wy;
        sy += uz * wx - ux * wz;
        sz += ux * wy - uy * wx;
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    const bool ok = len > 0.0 && len - len == 0.0;                       // (an unreferenced vertex, cancelling faces, NaN, overflow: zeros)
    float* o = normals + 3l * v;
    o[0] = ok ? (float)(sx / len) : 0.0f;
    o[1] = ok ? (float)(sy / len) : 0.0f;
    o[2] = ok ? (float)(sz / len) : 0.0f;
}

// ---- connected components (ABI 1190; tests/mesh_clean_reference.py): labels[v] starts as v and falls to the smallest vertex
// index of v's component.  One sweep: the thread that owns v - the only writer of labels[v] - takes the minimum of labels[labels[u]] over v
// itself and every index u of the faces around v (the CSR list of the normals kernel) and stores it if it is smaller.  In place, no atomics:
// a label read from another vertex is this sweep's or the previous one's, either way the index of a vertex of the same component, so labels
// only fall and the only fixed point is labels[v] = the root.  Every loop below runs over the INPUT's corner list: no trip count depends on
// another thread's stores (no find-root walk, no spin, no grid barrier).  The flag word is the one address several threads store to, all of
// them the same 1.  A label, corner id or face index outside its range is never read through.
__device__ __forceinline__ int mesh_label2(const int* labels, unsigned nv, int u) {
    const int a = labels[u];
    if ((unsigned)a >= nv) return 0x7fffffff;
    const int b = labels[a];
    return (unsigned)b < nv ? b : 0x7fffffff;
}
__global__ __launch_bounds__(256) void mesh_label_sweep_kernel(const int* __restrict__ faces, int corners, const int* __restrict__ starts,
                                                               const int* __restrict__ order, unsigned nv, int* labels, int* flag) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    int e0 = starts[v], e1 = starts[v + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > corners ? corners : e1;
    const int own = labels[v];
    int m = mesh_label2(labels, nv, (int)v);
    for (int e = e0; e < e1; ++e) {
        const int corner = order[e];
        if (corner < 0 || corner >= corners) continue;
        const int* f = faces + (long)(corner / 3) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int u = f[c];
            if ((unsigned)u >= nv) continue;
            const int l = mesh_label2(labels, nv, u);
            m = l < m ? l : m;
        }
    }
    if (m < own) {
        labels[v] = m;
        *flag = 1;
    }
}

// ---- face selection (ABI 1190): the kept faces in their order, the vertices they name in theirs, indices renumbered.  Both are
// flags at fixed positions - face q: keep[q] and three indices in range; vertex p: a kept face among the faces around it, GATHERED through the
// CSR list (no scatter) - and leave through compact.hpp's count / scan / emit as the extraction's slots do: one count launch over the vertex
// tiles then the face tiles, mesh_scan_kernel, a vertex emit that writes position, old index and vmap[p], a face emit that reads vmap.
__device__ __forceinline__ bool mesh_face_kept(const int* __restrict__ faces, const unsigned char* __restrict__ keep, unsigned nv, long nf,
                                               long q) {
    if (q >= nf || keep[q] == 0) return false;
    const int* f = faces + q * 3;
    return (unsigned)f[0] < nv && (unsigned)f[1] < nv && (unsigned)f[2] < nv;
}
__device__ __forceinline__ bool mesh_vertex_used(const int* __restrict__ faces, const unsigned char* __restrict__ keep,
                                                 const int* __restrict__ starts, const int* __restrict__ order, unsigned nv, long nf, long p) {
    if (p >= (long)nv) return false;
    const int corners = (int)(3 * nf);
    int e0 = starts[p], e1 = starts[p + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > corners ? corners : e1;
    bool used = false;
    for (int e = e0; e < e1; ++e) {
        const int corner = order[e];
        if (corner < 0 || corner >= corners) continue;
        used |= mesh_face_kept(faces, keep, nv, nf, (long)(corner / 3));
    }
    return used;
}

// count: grid = vertex blocks then face blocks, one partial each; used[p] is stored for the emit, which does not walk the list again
__global__ __launch_bounds__(256) void mesh_select_count_kernel(const int* __restrict__ faces, const unsigned char* __restrict__ keep,
                                                                const int* __restrict__ starts, const int* __restrict__ order, unsigned nv,
                                                                long nf, unsigned vblocks, unsigned char* __restrict__ used,
                                                                unsigned* __restrict__ partials) {
    const bool fpart = blockIdx.x >= vblocks;                            // (uniform)
    const long seg = compact_seg<MESH_TILE, long>() - (fpart ? (long)vblocks * MESH_TILE : 0);
    if (fpart) compact_count<MESH_TILE>(seg, [&](long q) { return mesh_face_kept(faces, keep, nv, nf, q); }, partials, blockIdx.x);
    else compact_count<MESH_TILE>(seg, [&](long p) {
        const bool u = mesh_vertex_used(faces, keep, starts, order, nv, nf, p);
        if (p < (long)nv) used[p] = (unsigned char)u;
        return u;
    }, partials, blockIdx.x);
}

// vertex emit: vmap[p] = the vertex's new index (for every used vertex: the faces read it); below the caller's capacity the position's bits
// and the old index
__global__ __launch_bounds__(256) void mesh_select_vertex_emit_kernel(const float* __restrict__ vertices, unsigned nv,
                                                                      const unsigned char* __restrict__ used,
                                                                      const long long* __restrict__ offsets, long long capacity,
                                                                      int* __restrict__ vmap, float* __restrict__ out, int* __restrict__ index) {
    const auto set = [&](long p) { return p < (long)nv && used[p] != 0; };
    compact_emit<MESH_TILE>(compact_seg<MESH_TILE, long>(), set, offsets, blockIdx.x, [&](long p, long long idx) {
        vmap[p] = (int)idx;
        if (idx >= capacity) return;                                     // (never past what the caller allocated)
        const float* s = vertices + 3 * p;
        float* o = out + idx * 3;
        o[0] = s[0];
        o[1] = s[1];
        o[2] = s[2];
        index[idx] = (int)p;
    });
}

__global__ __launch_bounds__(256) void mesh_select_face_emit_kernel(const int* __restrict__ faces, const unsigned char* __restrict__ keep,
                                                                    unsigned nv, long nf, const long long* __restrict__ offsets,
                                                                    long long capacity, const int* __restrict__ vmap, int* __restrict__ out) {
    const auto set = [&](long q) { return mesh_face_kept(faces, keep, nv, nf, q); };
    compact_emit<MESH_TILE>(compact_seg<MESH_TILE, long>(), set, offsets, blockIdx.x, [&](long q, long long idx) {
        if (idx >= capacity) return;                                     // (never past what the caller allocated)
        const int* f = faces + q * 3;
        int* o = out + idx * 3;
        o[0] = vmap[f[0]];
        o[1] = vmap[f[1]];
        o[2] = vmap[f[2]];
    });
}

// ---- host side.  The order of the checks is the documented one (cer_mvs.h): negative sizes, too large, the frame, nothing to do, pointers.
// CER_OK and the node count, or the error of a negative or too large grid
static int mesh_nodes(int nx, int ny, int nz, long* nodes) {
    if (nx < 0 || ny < 0 || nz < 0) return CER_EINVAL;
    *nodes = 0;
    if (nx == 0 || ny == 0 || nz == 0) return CER_OK;
    const long lim = 0x7fffffffL - MESH_TILE;                            // nodes < 2^31 - tile
    if ((long)nx * ny >= lim || (long)nx * ny * nz >= lim) return CER_ESHAPE;
    *nodes = (long)nx * ny * nz;
    return CER_OK;
}
static MeshDims mesh_dims(int nx, int ny, int nz) {
    MeshDims D = {nx, ny, nz, (long)nx * ny * nz * 8, (long)(nx - 1) * (ny - 1) * (nz - 1) * 12};
    return D;
}
static long mesh_blocks(long slots) { return (slots + MESH_TILE - 1) / MESH_TILE; }

extern "C" long cer_mesh_partials(int nx, int ny, int nz) {
    long nodes = 0;
    const int rc = mesh_nodes(nx, ny, nz, &nodes);
    if (rc != CER_OK) return rc;
    if (nodes == 0 || nx == 1 || ny == 1 || nz == 1) return 0;
    const MeshDims D = mesh_dims(nx, ny, nz);
    return mesh_blocks(D.vslots) + mesh_blocks(D.fslots);
}

extern "C" int cer_tsdf_integrate_f32(const float* depths, const unsigned char* masks, const double* cams, int N, int h, int w,
                                      const int* views, int n_views, const double* origin, double voxel, int nx, int ny, int nz,
                                      double trunc, float* tsdf, int* weight, void* stream) {
    long nodes = 0;
    if (N < 0 || h < 0 || w < 0 || n_views < 0) return CER_EINVAL;
    const int rc = mesh_nodes(nx, ny, nz, &nodes);
    if (rc != CER_OK) return rc;
    if ((long)h * w > 0x7fffffffL) return CER_ESHAPE;
    if (!cer_frame_ok(origin, voxel) || !(cer_is_finite(trunc) && trunc > 0.0)) return CER_EINVAL;
    if (nodes == 0 || n_views == 0) return CER_OK;                       // (no views: weight 0 and tsdf 1 are the caller's to fill)
    if (!depths || !cams || !views || !tsdf || !weight || N == 0 || h == 0 || w == 0) return CER_EINVAL;
    const MeshGrid g = {origin[0], origin[1], origin[2], voxel, nx, ny, nz};
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depths, masks, cams, N,
                       h, w, views, n_views, g, trunc, (unsigned)nodes, tsdf, weight);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_cells_u16(const float* tsdf, const int* weight, int nx, int ny, int nz, int min_weight, unsigned short* cells,
                                  void* stream) {
    long nodes = 0;
    const int rc = mesh_nodes(nx, ny, nz, &nodes);
    if (rc != CER_OK) return rc;
    if (nodes == 0 || nx == 1 || ny == 1 || nz == 1) return CER_OK;
    if (!tsdf || !weight || !cells) return CER_EINVAL;
    const long ncells = (long)(nx - 1) * (ny - 1) * (nz - 1);
    hipLaunchKernelGGL(mesh_cells_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tsdf, weight, nx, ny,
                       min_weight, (unsigned)ncells, cells);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_count(const unsigned short* cells, int nx, int ny, int nz, unsigned int* partials, long long* offsets,
                              long long* totals, void* stream) {
    long nodes = 0;
    const int rc = mesh_nodes(nx, ny, nz, &nodes);
    if (rc != CER_OK) return rc;
    if (nodes == 0 || nx == 1 || ny == 1 || nz == 1) return CER_OK;      // (no cell: totals are the caller's to zero)
    if (!cells || !partials || !offsets || !totals) return CER_EINVAL;
    const MeshDims D = mesh_dims(nx, ny, nz);
    const long vb = mesh_blocks(D.vslots), fb = mesh_blocks(D.fslots);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)(vb + fb)), dim3(256), 0, st, cells, D, (unsigned)vb, partials);
    CER_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(2), dim3(1024), 0, st, partials, vb, fb, offsets, totals);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_emit_f32(const float* tsdf, const unsigned short* cells, const double* origin, double voxel, int nx, int ny, int nz,
                                 const long long* offsets, long long nv, long long nf, long long vcap, long long fcap, int* vmap,
                                 float* vertices, int* faces, void* stream) {
    long nodes = 0;
    if (nv < 0 || nf < 0 || vcap < 0 || fcap < 0) return CER_EINVAL;
    const int rc = mesh_nodes(nx, ny, nz, &nodes);
    if (rc != CER_OK) return rc;
    if (nv > 0x7fffffffLL || nf > 0x7fffffffLL) return CER_ESHAPE;       // indices are int32
    if (!cer_frame_ok(origin, voxel)) return CER_EINVAL;
    if (nodes == 0 || nx == 1 || ny == 1 || nz == 1 || (nv == 0 && nf == 0) || (vcap == 0 && fcap == 0)) return CER_OK;
    if (!tsdf || !cells || !offsets || !vmap || (vcap && !vertices) || (fcap && !faces)) return CER_EINVAL;
    const MeshDims D = mesh_dims(nx, ny, nz);
    const MeshGrid g = {origin[0], origin[1], origin[2], voxel, nx, ny, nz};
    const long vb = mesh_blocks(D.vslots), fb = mesh_blocks(D.fslots);
    hipStream_t st = (hipStream_t)stream;
    if (nv) {
        hipLaunchKernelGGL(mesh_vertex_emit_kernel, dim3((unsigned)vb), dim3(256), 0, st, tsdf, cells, D, g, offsets, vcap, vmap, vertices);
        CER_RETURN_IF_LAUNCH_FAILED();
    }
    if (nf && fcap) {
        hipLaunchKernelGGL(mesh_face_emit_kernel, dim3((unsigned)fb), dim3(256), 0, st, cells, D, offsets + vb + 1, fcap, vmap, faces);
        CER_RETURN_IF_LAUNCH_FAILED();
    }
    return CER_OK;
}

extern "C" int cer_mesh_vertex_colors_u8(const float* vertices, long long nv, const float* depths, const unsigned char* masks,
                                         const float* colors, const double* cams, int N, int h, int w, const int* views, int n_views,
                                         double tol, unsigned char* rgb, int* seen, void* stream) {
    if (nv < 0 || N < 0 || h < 0 || w < 0 || n_views < 0) return CER_EINVAL;
    if (nv > 0x7fffffffLL || (long)h * w > 0x7fffffffL) return CER_ESHAPE;
    if (!(cer_is_finite(tol) && tol > 0.0)) return CER_EINVAL;
    if (nv == 0 || n_views == 0) return CER_OK;                          // (no views: rgb 0 and seen 0 are the caller's to fill)
    if (!vertices || !depths || !colors || !cams || !views || !rgb || !seen || N == 0 || h == 0 || w == 0) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_vertex_color_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, (unsigned)nv,
                       depths, masks, colors, cams, N, h, w, views, n_views, tol, rgb, seen);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_vertex_normals_f32(const float* vertices, long long nv, const int* faces, long long nf, const int* starts,
                                           const int* order, float* normals, void* stream) {
    if (nv < 0 || nf < 0) return CER_EINVAL;
    if (nv > 0x7fffffffLL || nf > 0x7fffffffLL / 3) return CER_ESHAPE;   // corner ids 0 .. 3 nf - 1 are int32
    if (nv == 0) return CER_OK;
    if (!vertices || !starts || !normals || (nf && (!faces || !order))) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, (unsigned)nv,
                       faces, (int)(3 * nf), starts, order, normals);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

// ---- components and selection (ABI 1190).  Checks: a negative size, nv or 3 nf >= 2^31, nothing to do, pointers.
static int mesh_index_sizes(long long nv, long long nf) {
    if (nv < 0 || nf < 0) return CER_EINVAL;
    if (nv > 0x7fffffffLL || nf > 0x7fffffffLL / 3) return CER_ESHAPE;   // vertex indices and corner ids 0 .. 3 nf - 1 are int32
    return CER_OK;
}

extern "C" int cer_mesh_label_sweeps_i32(const int* faces, long long nf, const int* starts, const int* order, long long nv, int* labels,
                                         int* flags, int n_sweeps, void* stream) {
    if (n_sweeps < 0) return CER_EINVAL;
    const int rc = mesh_index_sizes(nv, nf);
    if (rc != CER_OK) return rc;
    if (nv == 0 || n_sweeps == 0) return CER_OK;
    if (!starts || !labels || !flags || (nf && (!faces || !order))) return CER_EINVAL;
    for (int i = 0; i < n_sweeps; ++i) {
        hipLaunchKernelGGL(mesh_label_sweep_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, (int)(3 * nf),
                           starts, order, (unsigned)nv, labels, flags + i);
        CER_RETURN_IF_LAUNCH_FAILED();
    }
    return CER_OK;
}

extern "C" long cer_mesh_select_partials(long long nv, long long nf) {
    const int rc = mesh_index_sizes(nv, nf);
    if (rc != CER_OK) return rc;
    if (nv == 0 || nf == 0) return 0;
    return mesh_blocks((long)nv) + mesh_blocks((long)nf);
}

extern "C" int cer_mesh_select_count(const int* faces, long long nf, const int* starts, const int* order, long long nv,
                                     const unsigned char* keep, unsigned char* used, unsigned int* partials, long long* offsets,
                                     long long* totals, void* stream) {
    const int rc = mesh_index_sizes(nv, nf);
    if (rc != CER_OK) return rc;
    if (nv == 0 || nf == 0) return CER_OK;                               // (no face, no vertex survives: totals are the caller's to zero)
    if (!faces || !starts || !order || !keep || !used || !partials || !offsets || !totals) return CER_EINVAL;
    const long vb = mesh_blocks((long)nv), fb = mesh_blocks((long)nf);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_select_count_kernel, dim3((unsigned)(vb + fb)), dim3(256), 0, st, faces, keep, starts, order, (unsigned)nv, (long)nf,
                       (unsigned)vb, used, partials);
    CER_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(2), dim3(1024), 0, st, partials, vb, fb, offsets, totals);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_select_emit_f32(const float* vertices, long long nv, const int* faces, long long nf, const unsigned char* keep,
                                        const unsigned char* used, const long long* offsets, long long nv_out, long long nf_out, int* vmap,
                                        float* out_vertices, int* index, int* out_faces, void* stream) {
    if (nv_out < 0 || nf_out < 0) return CER_EINVAL;
    const int rc = mesh_index_sizes(nv, nf);
    if (rc != CER_OK) return rc;
    if (nv == 0 || nf == 0 || (nv_out == 0 && nf_out == 0)) return CER_OK;
    if (!vertices || !faces || !keep || !used || !offsets || !vmap || (nv_out && (!out_vertices || !index)) || (nf_out && !out_faces))
        return CER_EINVAL;
    const long vb = mesh_blocks((long)nv), fb = mesh_blocks((long)nf);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_select_vertex_emit_kernel, dim3((unsigned)vb), dim3(256), 0, st, vertices, (unsigned)nv, used, offsets, nv_out, vmap,
                       out_vertices, index);
    CER_RETURN_IF_LAUNCH_FAILED();
    if (nf_out) {
        hipLaunchKernelGGL(mesh_select_face_emit_kernel, dim3((unsigned)fb), dim3(256), 0, st, faces, keep, (unsigned)nv, (long)nf,
                           offsets + vb + 1, nf_out, vmap, out_faces);
        CER_RETURN_IF_LAUNCH_FAILED();
    }
    return CER_OK;
}

// ---- simplification by vertex clustering (ABI 1200; tests/mesh_simplify_reference.py).  The clusters are the occupied cells of
// cloud_eval.py's CloudIndex over the vertices: order (int64 [nv], the stable sort of the cell keys), cell_start (int64 [ncells + 1]) and
// cell_keys (int64 [ncells]) are that class's arrays as they are.  Every kernel below has one writer per address and no atomics.
#define MESH_KEY_B (CER_GRID_COORD_LIMIT - 1)
#define MESH_KEY_MASK 0x1fffffLL

// cluster[order[p]] = the cell r with cell_start[r] <= p < cell_start[r + 1]; -1 at and beyond cell_start[ncells] (the non-finite vertices)
__global__ __launch_bounds__(256) void mesh_cluster_map_kernel(const long long* __restrict__ order, const long long* __restrict__ cell_start,
                                                               long nv, long ncells, int* __restrict__ cluster) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= nv) return;
    const long long v = order[p];
    if ((unsigned long long)v >= (unsigned long long)nv) return;         // (never written through)
    int r = -1;
    if (p < cell_start[ncells]) {
        long lo = 0, hi = ncells;                                        // the last r in [0, ncells) with cell_start[r] <= p
        while (hi - lo > 1) {
            const long mid = lo + (hi - lo) / 2;
            if (cell_start[mid] <= p) lo = mid; else hi = mid;
        }
        r = (int)lo;
    }
    cluster[v] = r;
}

// ---- representatives: ONE thread owns a cluster for its whole member walk - the sums are added in member order, which a wave-wide reduction
// would change.  Members are gathered by index; in the quadric form the faces around a member are the CSR corners of the normals kernel.  An
// index, corner id or face index outside its range is skipped, never read through.
template <bool QUADRIC>
__global__ __launch_bounds__(256) void mesh_cluster_reps_kernel(const float* __restrict__ vertices, long nv, const int* __restrict__ faces,
                                                                int corners, const int* __restrict__ starts, const int* __restrict__ corner_order,
                                                                const long long* __restrict__ order, const long long* __restrict__ cell_start,
                                                                const long long* __restrict__ cell_keys, long ncells, double ox, double oy,
                                                                double oz, double cell, double regularisation,
                                                                const unsigned char* __restrict__ colors, float* __restrict__ reps,
                                                                unsigned char* __restrict__ rep_colors, unsigned char* __restrict__ took) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= ncells) return;
    long p0 = cell_start[r], p1 = cell_start[r + 1];
    p0 = p0 < 0 ? 0 : p0;
    p1 = p1 > nv ? nv : p1;
    const long long key = cell_keys[r];
    const double bx = ox + ((double)((int)(key & MESH_KEY_MASK) - MESH_KEY_B) + 0.5) * cell;
    const double by = oy + ((double)((int)((key >> 21) & MESH_KEY_MASK) - MESH_KEY_B) + 0.5) * cell;
    const double bz = oz + ((double)((int)((key >> 42) & MESH_KEY_MASK) - MESH_KEY_B) + 0.5) * cell;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    double mxx = 0.0, mxy = 0.0, mxz = 0.0, myy = 0.0, myz = 0.0, mzz = 0.0, qx = 0.0, qy = 0.0, qz = 0.0;
    unsigned long long cr = 0, cg = 0, cb = 0;
    long count = 0;
    for (long p = p0; p < p1; ++p) {
        const long long v = order[p];
        if ((unsigned long long)v >= (unsigned long long)nv) continue;
        const float* P = vertices + 3 * v;
        sx += (double)P[0];
        sy += (double)P[1];
        sz += (double)P[2];
        ++count;
        if (colors) {
            const unsigned char* c = colors + 3 * v;
            cr += c[0];
            cg += c[1];
            cb += c[2];
        }
        if (!QUADRIC) continue;
        int e0 = starts[v], e1 = starts[v + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > corners ? corners : e1;
        for (int e = e0; e < e1; ++e) {
            const int corner = corner_order[e];
            if (corner < 0 || corner >= corners) continue;
            const int* f = faces + (long)(corner / 3) * 3;
            const int ia = f[0], ib = f[1], ic = f[2];
            if ((unsigned)ia >= (unsigned long)nv || (unsigned)ib >= (unsigned long)nv || (unsigned)ic >= (unsigned long)nv) continue;
            const float *A = vertices + 3l * ia, *B = vertices + 3l * ib, *C = vertices + 3l * ic;
            const double ax = (double)A[0], ay = (double)A[1], az = (double)A[2];
            const double ux = (double)B[0] - ax, uy = (double)B[1] - ay, uz = (double)B[2] - az;
            const double wx = (double)C[0] - ax, wy = (double)C[1] - ay, wz = (double)C[2] - az;
            const double nx = uy * wz - uz * wy;
            const double ny = uz * wx - ux * wz;
            const double nz = ux * wy - uy * wx;
            const double d = (nx * (ax - bx) + ny * (ay - by)) + nz * (az - bz);
            mxx += nx * nx;
            mxy += nx * ny;
            mxz += nx * nz;
            myy += ny * ny;
            myz += ny * nz;
            mzz += nz * nz;
            qx += nx * d;
            qy += ny * d;
            qz += nz * d;
        }
    }
    const double k = (double)count;
    const double mx = sx / k, my = sy / k, mz = sz / k;
    double rx = mx, ry = my, rz = mz;
    bool minimiser = false;
    if (QUADRIC) {
        const double lam = (regularisation * ((mxx + myy) + mzz)) / 3.0;
        const double a = mxx + lam, dd = myy + lam, ff = mzz + lam;
        const double tx = qx + lam * (mx - bx), ty = qy + lam * (my - by), tz = qz + lam * (mz - bz);
        const double c00 = dd * ff - myz * myz;
        const double c01 = mxz * myz - mxy * ff;
        const double c02 = mxy * myz - mxz * dd;
        const double c11 = a * ff - mxz * mxz;
        const double c12 = mxy * mxz - a * myz;
        const double c22 = a * dd - mxy * mxy;
        const double det = (a * c00 + mxy * c01) + mxz * c02;
        const double x = ((c00 * tx + c01 * ty) + c02 * tz) / det;
        const double y = ((c01 * tx + c11 * ty) + c12 * tz) / det;
        const double z = ((c02 * tx + c12 * ty) + c22 * tz) / det;
        const double half = cell / 2.0;
        minimiser = lam > 0.0 && det > 0.0 && det - det == 0.0 && x - x == 0.0 && y - y == 0.0 && z - z == 0.0 && fabs(x) <= half
                    && fabs(y) <= half && fabs(z) <= half;
        if (minimiser) {
            rx = bx + x;
            ry = by + y;
            rz = bz + z;
        }
    }
    float* o = reps + 3 * r;
    o[0] = (float)rx;
    o[1] = (float)ry;
    o[2] = (float)rz;
    took[r] = (unsigned char)minimiser;
    if (colors) {
        unsigned char* oc = rep_colors + 3 * r;
        const unsigned long long n = count > 0 ? (unsigned long long)count : 1ull;
        oc[0] = (unsigned char)(cr / n);
        oc[1] = (unsigned char)(cg / n);
        oc[2] = (unsigned char)(cb / n);
    }
}

// ---- faces: the cluster triple of every face, rotated so that its smallest id comes first (orientation kept), and a valid byte: the three
// indices in range, every one with a cluster, the three clusters distinct.  An invalid face gets (-1, -1, -1).
__global__ __launch_bounds__(256) void mesh_cluster_faces_kernel(const int* __restrict__ faces, long nf, const int* __restrict__ cluster, long nv,
                                                                 int* __restrict__ triples, unsigned char* __restrict__ valid) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nf) return;
    const int* f = faces + 3 * q;
    const int ia = f[0], ib = f[1], ic = f[2];
    int a = -1, b = -1, c = -1;
    if (ia >= 0 && ib >= 0 && ic >= 0 && ia < nv && ib < nv && ic < nv) {
        a = cluster[ia];
        b = cluster[ib];
        c = cluster[ic];
    }
    const bool ok = a >= 0 && b >= 0 && c >= 0 && a != b && b != c && a != c;
    int t0 = -1, t1 = -1, t2 = -1;
    if (ok) {
        if (a < b && a < c) {
            t0 = a, t1 = b, t2 = c;
        } else if (b < a && b < c) {
            t0 = b, t1 = c, t2 = a;
        } else {
            t0 = c, t1 = a, t2 = b;
        }
    }
    int* o = triples + 3 * q;
    o[0] = t0;
    o[1] = t1;
    o[2] = t2;
    valid[q] = (unsigned char)ok;
}

// ---- heads of the lexicographically sorted triples: perm[p] is the face at sorted position p (two stable sorts: equal triples keep ascending
// face index), keep[perm[p]] = valid && (p == 0 || triple[perm[p]] != triple[perm[p - 1]]) - the lowest face index of every distinct triple
__global__ __launch_bounds__(256) void mesh_face_heads_kernel(const int* __restrict__ triples, const unsigned char* __restrict__ valid,
                                                              const long long* __restrict__ perm, long nf, unsigned char* __restrict__ keep) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= nf) return;
    const long long q = perm[p];
    if ((unsigned long long)q >= (unsigned long long)nf) return;         // (never written through)
    bool head = valid[q] != 0;
    if (head && p > 0) {
        const long long w = perm[p - 1];
        if ((unsigned long long)w < (unsigned long long)nf) {
            const int *s = triples + 3 * q, *t = triples + 3 * w;
            head = s[0] != t[0] || s[1] != t[1] || s[2] != t[2];
        }
    }
    keep[q] = (unsigned char)head;
}

// Checks, in the order of the section "Surface mesh": a negative size, too large, the frame, nothing to do, pointers.
static int mesh_cluster_sizes(long long nv, long long nf, long long ncells) {
    if (nv < 0 || nf < 0 || ncells < 0) return CER_EINVAL;
    if (nv > 0x7fffffffLL || nf > 0x7fffffffLL / 3 || ncells > 0x7fffffffLL || ncells > nv) return CER_ESHAPE;
    return CER_OK;
}

extern "C" int cer_mesh_cluster_map_i32(const long long* order, const long long* cell_start, long long nv, long long ncells, int* cluster,
                                        void* stream) {
    const int rc = mesh_cluster_sizes(nv, 0, ncells);
    if (rc != CER_OK) return rc;
    if (nv == 0) return CER_OK;
    if (!order || !cell_start || !cluster) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_cluster_map_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, order, cell_start, (long)nv,
                       (long)ncells, cluster);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_cluster_reps_f32(const float* vertices, long long nv, const int* faces, long long nf, const int* starts,
                                         const int* corner_order, const long long* order, const long long* cell_start,
                                         const long long* cell_keys, long long ncells, const double* origin, double cell, int quadric,
                                         double regularisation, const unsigned char* colors, float* reps, unsigned char* rep_colors,
                                         unsigned char* took, void* stream) {
    const int rc = mesh_cluster_sizes(nv, nf, ncells);
    if (rc != CER_OK) return rc;
    if (!cer_frame_ok(origin, cell) || !(cer_is_finite(regularisation) && regularisation > 0.0)) return CER_EINVAL;
    if (ncells == 0) return CER_OK;
    if (!vertices || !order || !cell_start || !cell_keys || !reps || !took || (colors == nullptr) != (rep_colors == nullptr)) return CER_EINVAL;
    if (quadric && (!starts || (nf && (!faces || !corner_order)))) return CER_EINVAL;
    const dim3 grid((unsigned)((ncells + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    if (quadric)
        hipLaunchKernelGGL(mesh_cluster_reps_kernel<true>, grid, dim3(256), 0, st, vertices, (long)nv, faces, (int)(3 * nf), starts, corner_order,
                           order, cell_start, cell_keys, (long)ncells, origin[0], origin[1], origin[2], cell, regularisation, colors, reps,
                           rep_colors, took);
    else
        hipLaunchKernelGGL(mesh_cluster_reps_kernel<false>, grid, dim3(256), 0, st, vertices, (long)nv, faces, (int)(3 * nf), starts, corner_order,
                           order, cell_start, cell_keys, (long)ncells, origin[0], origin[1], origin[2], cell, regularisation, colors, reps,
                           rep_colors, took);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_cluster_faces_i32(const int* faces, long long nf, const int* cluster, long long nv, int* triples, unsigned char* valid,
                                          void* stream) {
    const int rc = mesh_cluster_sizes(nv, nf, 0);
    if (rc != CER_OK) return rc;
    if (nf == 0) return CER_OK;
    if (!faces || !triples || !valid || (nv && !cluster)) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_cluster_faces_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, (long)nf, cluster,
                       (long)nv, triples, valid);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_face_heads_u8(const int* triples, const unsigned char* valid, const long long* perm, long long nf, unsigned char* keep,
                                      void* stream) {
    const int rc = mesh_cluster_sizes(0, nf, 0);
    if (rc != CER_OK) return rc;
    if (nf == 0) return CER_OK;
    if (!triples || !valid || !perm || !keep) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_face_heads_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, triples, valid, perm,
                       (long)nf, keep);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

// ---- mesh edges and smoothing (ABI 1210; tests/mesh_smooth_reference.py).  The unique-neighbour list of every vertex,
// ascending, with a count per direction - the duplicate-free edge table - and Taubin / Laplacian smoothing as one gather kernel over it.
// Integers and fp64 with the associations of cer_mvs.h; every address has one writer, no atomics, the same bytes on every run.
//
// keys: one thread per face writes six 64-bit keys, two per directed edge a -> b: (a << 32) | (b << 1) in a's list ("along") and
// (b << 32) | (a << 1) | 1 in b's ("against"); -1 for an edge with equal ends or an index out of range.  Sorted ascending (the caller: equal
// keys are indistinguishable, so any sort), the keys of one (owner, other) pair form one run with the "along" keys in front.
__global__ __launch_bounds__(256) void mesh_edge_keys_kernel(const int* __restrict__ faces, long nf, unsigned nv, long long* __restrict__ keys) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nf) return;
    const int* f = faces + 3 * q;
    const int i[3] = {f[0], f[1], f[2]};
    long long* o = keys + 6 * q;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = i[c], b = i[c == 2 ? 0 : c + 1];
        const bool ok = (unsigned)a < nv && (unsigned)b < nv && a != b;
        o[2 * c] = ok ? ((long long)a << 32) | ((long long)b << 1) : -1ll;
        o[2 * c + 1] = ok ? ((long long)b << 32) | ((long long)a << 1) | 1ll : -1ll;
    }
}

// head of a run of the sorted keys: the first key of its (owner, other) pair
__device__ __forceinline__ bool mesh_edge_head(const long long* __restrict__ keys, long nk, long p) {
    if (p >= nk) return false;
    const long long k = keys[p];
    return k >= 0 && (p == 0 || (keys[p - 1] >> 1) != (k >> 1));
}

__global__ __launch_bounds__(256) void mesh_edge_count_kernel(const long long* __restrict__ keys, long nk, unsigned* __restrict__ partials) {
    compact_count<MESH_TILE>(compact_seg<MESH_TILE, long>(), [&](long p) { return mesh_edge_head(keys, nk, p); }, partials, blockIdx.x);
}

// emit: the head of a run writes its entry - owner, other and the run's keys by direction bit.  The run is walked forward from the head, so
// the entry has one writer; a run is as long as the edge has faces on it.
__global__ __launch_bounds__(256) void mesh_edge_emit_kernel(const long long* __restrict__ keys, long nk, const long long* __restrict__ offsets,
                                                             long long capacity, int* __restrict__ owner, int* __restrict__ nbrs,
                                                             int* __restrict__ along, int* __restrict__ against) {
    const auto set = [&](long p) { return mesh_edge_head(keys, nk, p); };
    compact_emit<MESH_TILE>(compact_seg<MESH_TILE, long>(), set, offsets, blockIdx.x, [&](long p, long long idx) {
        if (idx >= capacity) return;                                     // (never past what the caller allocated)
        const long long pair = keys[p] >> 1;
        int n0 = 0, n1 = 0;
        for (long q = p; q < nk; ++q) {
            const long long k = keys[q];
            if ((k >> 1) != pair) break;
            if (k & 1ll) ++n1; else ++n0;
        }
        owner[idx] = (int)(pair >> 31);
        nbrs[idx] = (int)(pair & 0x7fffffffll);
        along[idx] = n0;
        against[idx] = n1;
    });
}

// ---- smoothing, prepare: one thread per vertex reads its run once.  flags[v] = 1 (finite in the input) | 2 (frozen) | 4 (boundary: an entry
// with along + against == 1); walk[e] = the neighbour, or -1 where it is not finite in the input (the step then neither reads nor counts it);
// state[v] = the promoted position.  A neighbour outside 0 .. nv-1 is not read through and walks as -1.
__device__ __forceinline__ bool mesh_finite3(const float* __restrict__ p) {
    const float x = p[0], y = p[1], z = p[2];
    return x - x == 0.0f && y - y == 0.0f && z - z == 0.0f;
}
__global__ __launch_bounds__(256) void mesh_smooth_prepare_kernel(const float* __restrict__ vertices, unsigned nv, const int* __restrict__ starts,
                                                                  const int* __restrict__ nbrs, const int* __restrict__ along,
                                                                  const int* __restrict__ against, int nn, int fixed_boundary,
                                                                  int* __restrict__ walk, unsigned char* __restrict__ flags,
                                                                  double* __restrict__ state) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    int e0 = starts[v], e1 = starts[v + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > nn ? nn : e1;
    bool boundary = false, any = false;
    for (int e = e0; e < e1; ++e) {
        const int u = nbrs[e];
        const bool fin = (unsigned)u < nv && mesh_finite3(vertices + 3l * u);
        walk[e] = fin ? u : -1;
        any |= fin;
        boundary |= along[e] + against[e] == 1;
    }
    const float* p = vertices + 3l * v;
    const bool finite = mesh_finite3(p);
    const bool frozen = !finite || !any || (fixed_boundary != 0 && boundary);
    flags[v] = (unsigned char)((finite ? 1 : 0) | (frozen ? 2 : 0) | (boundary ? 4 : 0));
    double* s = state + 3l * v;
    s[0] = (double)p[0];
    s[1] = (double)p[1];
    s[2] = (double)p[2];
}

// ---- smoothing, one step: the hot path.  One thread per vertex walks its run; per axis s = 0.0, s = s + p[u] over the walked neighbours in
// ascending order, m = s / double(count), q = p + w * (m - p); a frozen vertex copies.  src and dst are different buffers: a step reads only
// the previous step's values.  Sums in registers; no LDS, no atomics.
__global__ __launch_bounds__(256) void mesh_smooth_step_kernel(const double* __restrict__ src, double* __restrict__ dst, unsigned nv,
                                                               const int* __restrict__ starts, const int* __restrict__ walk, int nn,
                                                               const unsigned char* __restrict__ flags, double w) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    const double* p = src + 3l * v;
    double qx = p[0], qy = p[1], qz = p[2];
    if (!(flags[v] & 2)) {
        int e0 = starts[v], e1 = starts[v + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > nn ? nn : e1;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int count = 0;
        for (int e = e0; e < e1; ++e) {
            const int u = walk[e];
            if ((unsigned)u >= nv) continue;
            const double* r = src + 3l * u;
            sx = sx + r[0];
            sy = sy + r[1];
            sz = sz + r[2];
            ++count;
        }
        if (count > 0) {
            const double n = (double)count;
            qx = qx + w * (sx / n - qx);
            qy = qy + w * (sy / n - qy);
            qz = qz + w * (sz / n - qz);
        }
    }
    double* o = dst + 3l * v;
    o[0] = qx;
    o[1] = qy;
    o[2] = qz;
}

// ---- smoothing, finish: the state rounded to float32 once; a frozen vertex gets its input bits back
__global__ __launch_bounds__(256) void mesh_smooth_finish_kernel(const double* __restrict__ state, const float* __restrict__ vertices,
                                                                 const unsigned char* __restrict__ flags, unsigned nv, float* __restrict__ out) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    const bool frozen = (flags[v] & 2) != 0;
    const double* s = state + 3l * v;
    const float* p = vertices + 3l * v;
    float* o = out + 3l * v;
    o[0] = frozen ? p[0] : (float)s[0];
    o[1] = frozen ? p[1] : (float)s[1];
    o[2] = frozen ? p[2] : (float)s[2];
}

// Checks, in the order of the section "Surface mesh": a negative size, too large (nv, 3 nf, 6 nf or nn >= 2^31), a non-finite weight, nothing
// to do, pointers.
static int mesh_edge_sizes(long long nv, long long nf, long long nn) {
    if (nv < 0 || nf < 0 || nn < 0) return CER_EINVAL;
    if (nv > 0x7fffffffLL || nf > 0x7fffffffLL / 6 || nn > 0x7fffffffLL) return CER_ESHAPE;   // positions 0 .. 6 nf - 1 and list entries are int32
    return CER_OK;
}

extern "C" long cer_mesh_edge_partials(long long nf) {
    const int rc = mesh_edge_sizes(0, nf, 0);
    if (rc != CER_OK) return rc;
    return mesh_blocks((long)(6 * nf));
}

extern "C" int cer_mesh_edge_keys_i64(const int* faces, long long nf, long long nv, long long* keys, void* stream) {
    const int rc = mesh_edge_sizes(nv, nf, 0);
    if (rc != CER_OK) return rc;
    if (nf == 0) return CER_OK;
    if (!faces || !keys) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_edge_keys_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, (hipStream_t)stream, faces, (long)nf, (unsigned)nv,
                       keys);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_edge_count(const long long* sorted_keys, long long nf, unsigned int* partials, long long* offsets, long long* totals,
                                   void* stream) {
    const int rc = mesh_edge_sizes(0, nf, 0);
    if (rc != CER_OK) return rc;
    if (nf == 0) return CER_OK;                                          // (no key, no entry: totals are the caller's to zero)
    if (!sorted_keys || !partials || !offsets || !totals) return CER_EINVAL;
    const long nk = (long)(6 * nf), blocks = mesh_blocks(nk);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_edge_count_kernel, dim3((unsigned)blocks), dim3(256), 0, st, sorted_keys, nk, partials);
    CER_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(2), dim3(1024), 0, st, partials, blocks, 0l, offsets, totals);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_edge_emit_i32(const long long* sorted_keys, long long nf, const long long* offsets, long long nn, int* owner, int* nbrs,
                                      int* along, int* against, void* stream) {
    const int rc = mesh_edge_sizes(0, nf, nn);
    if (rc != CER_OK) return rc;
    if (nf == 0 || nn == 0) return CER_OK;
    if (!sorted_keys || !offsets || !owner || !nbrs || !along || !against) return CER_EINVAL;
    const long nk = (long)(6 * nf);
    hipLaunchKernelGGL(mesh_edge_emit_kernel, dim3((unsigned)mesh_blocks(nk)), dim3(256), 0, (hipStream_t)stream, sorted_keys, nk, offsets, nn,
                       owner, nbrs, along, against);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_smooth_prepare_f32(const float* vertices, long long nv, const int* nbr_starts, const int* nbrs, const int* along,
                                           const int* against, long long nn, int fixed_boundary, int* walk, unsigned char* flags,
                                           double* state, void* stream) {
    const int rc = mesh_edge_sizes(nv, 0, nn);
    if (rc != CER_OK) return rc;
    if (nv == 0) return CER_OK;
    if (!vertices || !nbr_starts || !flags || !state || (nn && (!nbrs || !along || !against || !walk))) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_smooth_prepare_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, (unsigned)nv,
                       nbr_starts, nbrs, along, against, (int)nn, fixed_boundary, walk, flags, state);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_smooth_steps_f64(double* state_a, double* state_b, long long nv, const int* nbr_starts, const int* walk, long long nn,
                                         const unsigned char* flags, double w_even, double w_odd, int n_steps, void* stream) {
    if (n_steps < 0) return CER_EINVAL;
    const int rc = mesh_edge_sizes(nv, 0, nn);
    if (rc != CER_OK) return rc;
    if (!cer_is_finite(w_even) || !cer_is_finite(w_odd)) return CER_EINVAL;
    if (nv == 0 || n_steps == 0) return CER_OK;
    if (!state_a || !state_b || state_a == state_b || !nbr_starts || !flags || (nn && !walk)) return CER_EINVAL;
    for (int i = 0; i < n_steps; ++i) {                                  // stream order: step i reads what step i - 1 wrote, no host wait between
        hipLaunchKernelGGL(mesh_smooth_step_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const double*)((i & 1) ? state_b : state_a), (i & 1) ? state_a : state_b, (unsigned)nv, nbr_starts, walk, (int)nn, flags,
                           (i & 1) ? w_odd : w_even);
        CER_RETURN_IF_LAUNCH_FAILED();
    }
    return CER_OK;
}

extern "C" int cer_mesh_smooth_finish_f32(const double* state, const float* vertices, const unsigned char* flags, long long nv, float* out,
                                          void* stream) {
    const int rc = mesh_edge_sizes(nv, 0, 0);
    if (rc != CER_OK) return rc;
    if (nv == 0) return CER_OK;
    if (!state || !vertices || !flags || !out) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_smooth_finish_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, state, vertices, flags,
                       (unsigned)nv, out);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}
