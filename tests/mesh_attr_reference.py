"""numpy restatement of the per-vertex mesh attributes (csrc/mesh.hip, cer-mvs_amd/mesh.py), written from the contract in
include/cer_mvs.h: colours gathered from the views that see a vertex, and area-weighted normals from the faces, fp64 with the associations of
the contract, vectorised over the vertices (colours: one pass per view; normals: one pass per corner rank within a vertex, so that every
vertex sums its faces in corner order).  Plus the linear paint the tests colour the sphere views with."""
import numpy as np


# ---------------------------------------------------------------- colours
def vertex_colors(vertices, depths, masks, colors, Ks, Es, tol, views=None):
    """vertices float32 [nv,3], depths float32 [N,h,w], masks uint8 [N,h,w] or None, colors float32 [N,3,h,w], Ks [N,3,3] / Es [N,4,4]
    float32 -> (rgb uint8 [nv,3], seen int32 [nv])"""
    p = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    depths = np.asarray(depths, dtype=np.float32)
    colors = np.asarray(colors, dtype=np.float32)
    N, h, w = depths.shape
    K = np.asarray(Ks, dtype=np.float32).astype(np.float64)
    E = np.asarray(Es, dtype=np.float32).astype(np.float64)
    nv = len(p)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    tol = np.float64(tol)
    total = np.zeros((nv, 3), dtype=np.float64)
    count = np.zeros(nv, dtype=np.int32)
    views = range(N) if views is None else views
    with np.errstate(all="ignore"):
        for v in views:
            e, k = E[v], K[v]
            cx = ((e[0, 0] * px + e[0, 1] * py) + e[0, 2] * pz) + e[0, 3]
            cy = ((e[1, 0] * px + e[1, 1] * py) + e[1, 2] * pz) + e[1, 3]
            cz = ((e[2, 0] * px + e[2, 1] * py) + e[2, 2] * pz) + e[2, 3]
            ux = (k[0, 0] * cx + k[0, 1] * cy) + k[0, 2] * cz
            uy = (k[1, 0] * cx + k[1, 1] * cy) + k[1, 2] * cz
            uz = (k[2, 0] * cx + k[2, 1] * cy) + k[2, 2] * cz
            x, y = ux / uz, uy / uz
            a, b = x + 0.5, y + 0.5
            ok = (uz > 0.0) & (a >= 0.0) & (a < np.float64(w)) & (b >= 0.0) & (b < np.float64(h))
            xi = np.where(ok, np.floor(a), 0.0).astype(np.int64)
            yi = np.where(ok, np.floor(b), 0.0).astype(np.int64)
            if masks is not None:
                ok &= np.asarray(masks)[v][yi, xi] != 0
            d = depths[v][yi, xi].astype(np.float64)
            ok &= np.isfinite(d) & (d > 0.0)
            ok &= np.abs(d - uz) <= tol
            xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
            x0, y0 = np.floor(xs), np.floor(ys)
            fx, fy = xs - x0, ys - y0
            xa, xb = np.clip(x0.astype(np.int64), 0, w - 1), np.clip(x0.astype(np.int64) + 1, 0, w - 1)
            ya, yb = np.clip(y0.astype(np.int64), 0, h - 1), np.clip(y0.astype(np.int64) + 1, 0, h - 1)
            for ch in range(3):
                plane = colors[v, ch]
                c00, c01 = plane[ya, xa].astype(np.float64), plane[ya, xb].astype(np.float64)
                c10, c11 = plane[yb, xa].astype(np.float64), plane[yb, xb].astype(np.float64)
                top = (1.0 - fx) * c00 + fx * c01
                bot = (1.0 - fx) * c10 + fx * c11
                val = (1.0 - fy) * top + fy * bot
                total[:, ch] = np.where(ok, total[:, ch] + val, total[:, ch])
            count = count + ok.astype(np.int32)
        q = (total / count.astype(np.float64)[:, None]) * 255.0
        byte = np.where(q >= 255.0, 255.0, np.where(q > 0.0, np.floor(q), 0.0))     # truncation of a positive q; NaN fails both: 0
    rgb = np.where((count > 0)[:, None], byte, 0.0).astype(np.uint8)
    return rgb, count


# ---------------------------------------------------------------- normals
def vertex_faces(faces, nv):
    """(starts int32 [nv + 1], order int32 [3 nf]): the corner ids 3 * face + corner stably sorted by their vertex"""
    keys = np.asarray(faces, dtype=np.int64).reshape(-1)
    order = np.argsort(keys, kind="stable")
    starts = np.searchsorted(keys[order], np.arange(nv + 1), side="left")
    return starts.astype(np.int32), order.astype(np.int32)


def vertex_normals(vertices, faces):
    """float32 [nv,3]: per vertex the sum of (B - A) x (C - A) over its corners in corner order, divided by its length; zeros without one"""
    p = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = len(p)
    with np.errstate(all="ignore"):
        A, B, C = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        U, W = B - A, C - A
        n = np.stack([U[:, 1] * W[:, 2] - U[:, 2] * W[:, 1], U[:, 2] * W[:, 0] - U[:, 0] * W[:, 2], U[:, 0] * W[:, 1] - U[:, 1] * W[:, 0]], 1)
        starts, order = vertex_faces(f, nv)
        deg = np.diff(starts)
        s = np.zeros((nv, 3), dtype=np.float64)
        for r in range(int(deg.max()) if nv and len(f) else 0):                  # the r-th corner of every vertex that has one
            who = np.nonzero(deg > r)[0]
            s[who] = s[who] + n[order[starts[who] + r] // 3]
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = (length > 0.0) & np.isfinite(length)
        out = np.where(ok[:, None], s / np.where(ok, length, 1.0)[:, None], 0.0)
    return out.astype(np.float32)


# ---------------------------------------------------------------- the linear paint
def paint(p):
    """the colour 0.5 + 0.25 * p of a surface point p"""
    return 0.5 + 0.25 * np.asarray(p, dtype=np.float64)


def painted_views(depths, masks, Ks, Es, fill=None):
    """colors float32 [N,3,h,w]: every masked pixel painted with ``paint`` of the surface point it sees (its depth back-projected through
    the float32 matrices in fp64).  A pixel that sees no surface is 0, or with ``fill`` painted as the point of its ray at depth ``fill``:
    the bilinear sample uses all four taps whatever their masks, so at a silhouette the background's colour enters a vertex's colour."""
    depths = np.asarray(depths, dtype=np.float32)
    if fill is not None:
        depths = np.where(np.asarray(masks) != 0, depths, np.float32(fill))
        masks = np.ones(depths.shape, np.uint8)
    N, h, w = depths.shape
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    pix = np.stack([u, v, np.ones_like(u)], -1)
    out = np.zeros((N, 3, h, w), dtype=np.float32)
    for i in range(N):
        K = np.asarray(Ks[i], dtype=np.float32).astype(np.float64)
        E = np.asarray(Es[i], dtype=np.float32).astype(np.float64)
        cam = (pix @ np.linalg.inv(K).T) * depths[i].astype(np.float64)[..., None]
        world = (cam - E[:3, 3]) @ E[:3, :3]                                       # R^T (cam - t), R orthonormal
        hit = np.asarray(masks[i]) != 0
        out[i] = np.where(hit[None], np.moveaxis(paint(world), -1, 0), 0.0).astype(np.float32)
    return out
