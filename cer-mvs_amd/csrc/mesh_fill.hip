// Mesh hole filling on the device (ABI 1220, cer-mvs_amd/mesh.py mesh_holes / fill_holes; tests/mesh_fill_reference.py): the
// small boundary loops of any indexed triangle mesh closed by a triangle (three edges) or by a fan around the loop's mean (four and more).
// It starts from mesh.hip's unique-neighbour list with a count per direction (ABI 1210): the directed edge a->b is a boundary half-edge iff
// along == 1 and against == 0, a vertex is simple iff exactly one leaves it and exactly one enters it, and a hole is a cycle of the
// successor table through simple vertices only, named by its smallest index.
//
// Three kernels, each a serial walk per thread: the successor of every vertex from its run of the list, the length of the cycle at every
// vertex that is its head (0 elsewhere), and per hole the fan.  The offsets between the second and the third are the caller's (two
// exclusive sums over the heads).  Integers, and fp64 sums with the association of cer_mvs.h; registers only: no block-shared memory, no
// barrier, no read-modify-write on memory, no fused multiply-add; every address has one writer, the same bytes on every run.
// An index outside its range is skipped, never read or written through.
#include "common.hpp"

__device__ __forceinline__ bool fill_finite3(const float* __restrict__ p) {
    const float x = p[0], y = p[1], z = p[2];
    return x - x == 0.0f && y - y == 0.0f && z - z == 0.0f;
}

// ---- successor: one thread per vertex walks its run once.  next[v] = the head of the one boundary half-edge that leaves v if exactly one
// leaves and exactly one enters; -1 where none touches v; -2 ("pinched") otherwise.
__global__ __launch_bounds__(256) void mesh_hole_next_kernel(const int* __restrict__ starts, const int* __restrict__ nbrs,
                                                             const int* __restrict__ along, const int* __restrict__ against, unsigned nv, int nn,
                                                             int* __restrict__ next) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    int e0 = starts[v], e1 = starts[v + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > nn ? nn : e1;
    int leaving = 0, entering = 0, head = -1;
    for (int e = e0; e < e1; ++e) {
        const int a = along[e], g = against[e];
        if (a == 1 && g == 0) {
            ++leaving;
            head = nbrs[e];
        } else if (a == 0 && g == 1) {
            ++entering;
        }
    }
    const bool simple = leaving == 1 && entering == 1 && (unsigned)head < nv && (unsigned)head != v;
    next[v] = (leaving == 0 && entering == 0) ? -1 : simple ? head : -2;
}

// ---- heads: one thread per vertex with a successor follows the table for at most max_edges steps.  It stops at a negative entry (the
// chain ends at a pinched vertex: no hole), at an index below v (v is not the head), at a non-finite member (with vertices), or back at v:
// length[v] = the number of edges then, if it is at least 3, and 0 in every other case.  The successor is injective on simple vertices, so a
// walk cannot enter a cycle it did not start on; max_edges bounds it regardless.
__global__ __launch_bounds__(256) void mesh_hole_heads_kernel(const int* __restrict__ next, const float* __restrict__ vertices, unsigned nv,
                                                              int max_edges, int* __restrict__ length) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    int n = 0;
    int u = next[v];
    if (u >= 0 && (vertices == nullptr || fill_finite3(vertices + 3l * v))) {
        int steps = 1;
        bool ok = true;
        while ((unsigned)u != v) {
            if ((unsigned)u >= nv || (unsigned)u < v || steps >= max_edges) { ok = false; break; }
            if (vertices != nullptr && !fill_finite3(vertices + 3l * u)) { ok = false; break; }
            u = next[u];
            ++steps;
        }
        if (ok && steps >= 3) n = steps;
    }
    length[v] = n;
}

// ---- fill: one thread per hole walks its cycle a0 = head, a(k+1) = next[a_k] once more.  Three edges: the one face (a0, a2, a1).  Four
// and more: the centre c = nv + vertex_offsets[i], per axis s = 0.0, s = s + double(p[a_k]) for k ascending, float(s / double(n)); its
// colour, per channel the integer sum of the members' bytes / n; the faces (a(k+1), a_k, c) at nf + face_offsets[i] + k.  hole[] = i for
// every face written.  The rows 0 .. nv-1 and 0 .. nf-1 of the outputs are the caller's copies and are not touched.
__global__ __launch_bounds__(256) void mesh_hole_fill_kernel(const int* __restrict__ next, const int* __restrict__ heads,
                                                             const int* __restrict__ lengths, const long long* __restrict__ face_offsets,
                                                             const long long* __restrict__ vertex_offsets, unsigned nh,
                                                             const float* __restrict__ vertices, const unsigned char* __restrict__ colors,
                                                             unsigned nv, long long nf, long long added_vertices, long long added_faces,
                                                             float* __restrict__ out_vertices, int* __restrict__ out_faces,
                                                             int* __restrict__ hole, unsigned char* __restrict__ out_colors) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nh) return;
    const int a0 = heads[i], n = lengths[i];
    const long long fo = face_offsets[i];
    if ((unsigned)a0 >= nv || n < 3 || fo < 0) return;
    if (n == 3) {
        if (fo >= added_faces) return;                                   // (never past what the caller allocated)
        const int a1 = next[a0];
        if ((unsigned)a1 >= nv) return;
        const int a2 = next[a1];
        if ((unsigned)a2 >= nv) return;
        int* f = out_faces + 3 * (nf + fo);
        f[0] = a0;
        f[1] = a2;
        f[2] = a1;
        hole[nf + fo] = (int)i;
        return;
    }
    const long long vo = vertex_offsets[i];
    if (vo < 0 || vo >= added_vertices || fo + n > added_faces || vertices == nullptr || out_vertices == nullptr) return;
    const long long c = (long long)nv + vo;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    unsigned long long c0 = 0, c1 = 0, c2 = 0;
    int a = a0;
    for (int k = 0; k < n; ++k) {
        const int b = next[a];
        if ((unsigned)b >= nv) break;                                    // (a table that is not the heads kernel's: stay inside)
        const float* p = vertices + 3l * a;
        sx = sx + (double)p[0];
        sy = sy + (double)p[1];
        sz = sz + (double)p[2];
        if (colors != nullptr) {
            const unsigned char* q = colors + 3l * a;
            c0 += q[0];
            c1 += q[1];
            c2 += q[2];
        }
        int* f = out_faces + 3 * (nf + fo + k);
        f[0] = b;
        f[1] = a;
        f[2] = (int)c;
        hole[nf + fo + k] = (int)i;
        a = b;
    }
    const double count = (double)n;
    float* o = out_vertices + 3 * c;
    o[0] = (float)(sx / count);
    o[1] = (float)(sy / count);
    o[2] = (float)(sz / count);
    if (colors != nullptr && out_colors != nullptr) {
        unsigned char* q = out_colors + 3 * c;
        q[0] = (unsigned char)(c0 / (unsigned long long)n);
        q[1] = (unsigned char)(c1 / (unsigned long long)n);
        q[2] = (unsigned char)(c2 / (unsigned long long)n);
    }
}

// Checks, in the order of the section "Surface mesh": a negative size, too large, nothing to do, pointers.
static const long long FILL_INT_MAX = 0x7fffffffLL;

extern "C" int cer_mesh_hole_next_i32(const int* nbr_starts, const int* nbrs, const int* along, const int* against, long long nv, long long nn,
                                      int* next, void* stream) {
    if (nv < 0 || nn < 0) return CER_EINVAL;
    if (nv > FILL_INT_MAX || nn > FILL_INT_MAX) return CER_ESHAPE;
    if (nv == 0) return CER_OK;
    if (!nbr_starts || !next || (nn && (!nbrs || !along || !against))) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_hole_next_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nbr_starts, nbrs, along, against,
                       (unsigned)nv, (int)nn, next);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_hole_heads_i32(const int* next, const float* vertices, long long nv, int max_edges, int* length, void* stream) {
    if (nv < 0) return CER_EINVAL;
    if (nv > FILL_INT_MAX || max_edges < 3) return CER_ESHAPE;
    if (nv == 0) return CER_OK;
    if (!next || !length) return CER_EINVAL;                             // (vertices: null iff absent)
    hipLaunchKernelGGL(mesh_hole_heads_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, next, vertices, (unsigned)nv,
                       max_edges, length);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}

extern "C" int cer_mesh_hole_fill_f32(const int* next, const int* heads, const int* lengths, const long long* face_offsets,
                                      const long long* vertex_offsets, long long nh, const float* vertices, const unsigned char* colors,
                                      long long nv, long long nf, long long added_vertices, long long added_faces, float* out_vertices,
                                      int* out_faces, int* hole, unsigned char* out_colors, void* stream) {
    if (nh < 0 || nv < 0 || nf < 0 || added_vertices < 0 || added_faces < 0) return CER_EINVAL;
    if (nv > FILL_INT_MAX || nh > nv || added_vertices > nh || nv + added_vertices > FILL_INT_MAX || nf > FILL_INT_MAX / 3 ||
        added_faces > FILL_INT_MAX / 3 || nf + added_faces > FILL_INT_MAX / 3)
        return CER_ESHAPE;
    if (nh == 0) return CER_OK;
    if (!next || !heads || !lengths || !face_offsets || !vertex_offsets || !out_faces || !hole) return CER_EINVAL;
    if (added_vertices && (!vertices || !out_vertices)) return CER_EINVAL;
    if ((colors == nullptr) != (out_colors == nullptr)) return CER_EINVAL;
    hipLaunchKernelGGL(mesh_hole_fill_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, (hipStream_t)stream, next, heads, lengths,
                       face_offsets, vertex_offsets, (unsigned)nh, vertices, colors, (unsigned)nv, nf, added_vertices, added_faces, out_vertices,
                       out_faces, hole, out_colors);
    CER_RETURN_IF_LAUNCH_FAILED();
    return CER_OK;
}
