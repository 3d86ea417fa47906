"""Surface mesh of a fused scan on the device (csrc/mesh.hip, C ABI 1170): the fused depth maps of ``fusion.fuse_depth_maps``
integrated into a dense volume of truncated signed distances (``tsdf_volume``), and marching tetrahedra on that volume (``extract_mesh``).
Vertex and face order are a pure function of the volume - every output slot is a flag at a fixed position, compacted without atomics - and
all coordinate arithmetic is fp64 with fixed associations: tests/mesh_reference.py restates it in numpy, bit for bit.  Per-vertex attributes
(C ABI 1180; tests/mesh_attr_reference.py): ``vertex_colors`` from the views that see a vertex, ``vertex_normals`` from the
faces of any indexed triangle mesh, and both through the PLY writer and reader.  Cleaning (C ABI 1190, DESIGN.md 3zc;
tests/mesh_clean_reference.py): ``mesh_components``, ``select_faces`` and ``remove_small_components`` for any indexed triangle mesh.
Simplification (C ABI 1200; tests/mesh_simplify_reference.py): ``simplify_vertex_clustering``, likewise.
Edges (C ABI 1210; tests/mesh_smooth_reference.py): ``mesh_edges`` / ``edge_table``, the report ``mesh_topology`` and
``smooth_mesh`` (Taubin, Laplacian), likewise.
Hole filling (csrc/mesh_fill.hip, C ABI 1220; tests/mesh_fill_reference.py): ``mesh_holes`` and ``fill_holes``, likewise.
Surface sampling (csrc/mesh_sample.hip, C ABI 1230; tests/mesh_sample_reference.py): ``face_areas``, ``sample_mesh``,
``sample_mesh_even`` and ``evaluate_mesh``, likewise.
Exact point-to-mesh distance (csrc/mesh_dist.hip, C ABI 1240; tests/mesh_dist_reference.py): ``MeshIndex``, ``mesh_distances``
and ``evaluate_mesh(method="exact")``, likewise.

Every argument check that needs no device runs before the library is loaded."""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L

CAM_DOUBLES = 24                                             # cer_mvs.h CER_CLOUD_CAM_DOUBLES
MESH_TILE = 2048                                             # cer_mvs.h CER_MESH_TILE
NODE_LIMIT = 2 ** 31 - MESH_TILE

Grid = namedtuple("Grid", "origin voxel dims")
Grid.__doc__ = """origin (3 floats), voxel (> 0), dims = (nx, ny, nz): node (i, j, k) sits at origin + (i, j, k) * voxel; volumes are [nz, ny, nx]"""


def _grid(grid, who):
    """the checked grid: (origin as a ctypes double[3], voxel, (nx, ny, nz))"""
    try:
        origin, voxel, dims = grid
        origin = [float(v) for v in origin]
        voxel = float(voxel)
        dims = tuple(int(v) for v in dims)
        same = all(int(v) == v for v in grid[2])
    except (TypeError, ValueError) as e:
        raise ValueError(f"{who}: grid = (origin [3], voxel, (nx, ny, nz)) expected") from e
    if len(origin) != 3 or len(dims) != 3 or not same:
        raise ValueError(f"{who}: grid = (origin [3], voxel, (nx, ny, nz)) expected")
    if not all(math.isfinite(v) for v in origin):
        raise ValueError(f"{who}: the grid's origin must be finite")
    if not (math.isfinite(voxel) and voxel > 0.0):
        raise ValueError(f"{who}: the grid's voxel must be a positive finite number")
    if min(dims) < 0:
        raise ValueError(f"{who}: the grid's dims must not be negative")
    if dims[0] * dims[1] * dims[2] >= NODE_LIMIT:
        raise ValueError(f"{who}: {dims[0]} x {dims[1]} x {dims[2]} nodes is beyond 2^31 - {MESH_TILE}")
    return (ctypes.c_double * 3)(*origin), voxel, dims


def grid_for(points, voxel=None, resolution=256, margin=None, max_nodes=2 ** 28, trunc=None):
    """The grid around a cloud: points float32 [n, 3] (a device cloud costs one host read of its bounding box).  ``voxel``, or the longest
    side of the box divided by ``resolution``; ``margin`` (world units, default ``trunc``, whose default is 3 voxels) is added on every side;
    the origin is snapped down to a multiple of ``voxel``, and the dims are the fewest nodes that reach the far corner.  fp64 on the host.
    ValueError: no finite point, a grid beyond ``max_nodes`` nodes."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("grid_for: points [n, 3] expected")
    if voxel is not None and not (math.isfinite(float(voxel)) and float(voxel) > 0.0):
        raise ValueError("grid_for: voxel must be a positive finite number")
    if voxel is None and not (isinstance(resolution, int) and resolution >= 1):
        raise ValueError("grid_for: resolution must be a positive integer")
    for name, v in (("margin", margin), ("trunc", trunc)):
        if v is not None and not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"grid_for: {name} must be a finite number >= 0")
    if points.shape[0] == 0:
        raise ValueError("grid_for: an empty cloud has no bounding box")
    finite = torch.isfinite(points).all(1)
    p = points[finite]
    if p.shape[0] == 0:
        raise ValueError("grid_for: no finite point")
    box = torch.stack([p.min(0).values, p.max(0).values]).double().cpu().numpy()         # the one host read
    lo, hi = box[0], box[1]
    if voxel is None:
        side = float((hi - lo).max())
        if not side > 0.0:
            raise ValueError("grid_for: the cloud's bounding box is a point; give a voxel")
        voxel = side / resolution
    voxel = float(voxel)
    if margin is None:
        margin = 3.0 * voxel if trunc is None else float(trunc)
    margin = float(margin)
    i0 = np.floor((lo - margin) / voxel)
    origin = i0 * voxel
    dims = np.ceil((hi + margin - origin) / voxel).astype(np.int64) + 1
    nodes = int(dims[0]) * int(dims[1]) * int(dims[2])
    if nodes > int(max_nodes):
        raise ValueError(f"grid_for: {int(dims[0])} x {int(dims[1])} x {int(dims[2])} = {nodes} nodes is beyond max_nodes = {int(max_nodes)}; "
                         "take a larger voxel or a lower resolution")
    return Grid(tuple(float(v) for v in origin), voxel, tuple(int(v) for v in dims))


def forward_cams(Ks, Es):
    """Per view K [9] | rows 0-2 of E [12] | padding, float64 [N, 24] (CPU): the float32 FORWARD matrices as given, promoted (the packing of
    ``fusion.cloud_cams``, which carries the inverses)."""
    Ks = torch.as_tensor(Ks).detach().to("cpu", torch.float32).numpy()
    Es = torch.as_tensor(Es).detach().to("cpu", torch.float32).numpy()
    if Ks.ndim != 3 or Ks.shape[1:] != (3, 3) or Es.shape != (Ks.shape[0], 4, 4):
        raise ValueError("forward_cams: Ks [N,3,3] and Es [N,4,4] expected")
    cams = np.zeros((Ks.shape[0], CAM_DOUBLES), dtype=np.float64)
    cams[:, :9] = Ks.reshape(-1, 9)
    cams[:, 9:21] = Es[:, :3].reshape(-1, 12)
    return torch.from_numpy(cams)


def _check_maps(depths, masks, who):
    if not isinstance(depths, torch.Tensor) or depths.dim() != 3 or depths.dtype != torch.float32:
        raise ValueError(f"{who}: depths float32 [N,h,w] expected")
    if masks is not None and (not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or masks.shape != depths.shape):
        raise ValueError(f"{who}: masks uint8 {list(depths.shape)} (or None) expected")
    if masks is not None and masks.device != depths.device:
        raise ValueError(f"{who}: depths and masks must be on one device")


def _check_views(views, N, who):
    views = list(range(N)) if views is None else [int(v) for v in views]
    if views and (min(views) < 0 or max(views) >= N):
        raise ValueError(f"{who}: views must list views in 0..{N - 1}")
    return views


def _check_trunc(trunc, who):
    trunc = float(trunc)
    if not (math.isfinite(trunc) and trunc > 0.0):
        raise ValueError(f"{who}: trunc must be a positive finite number")
    return trunc


def tsdf_volume(depths, masks, Ks, Es, grid, trunc, views=None):
    """The depth maps integrated into the grid's nodes: depths float32 [N,h,w] and masks uint8 [N,h,w] (or None: every pixel) on the device,
    Ks [N,3,3] / Es [N,4,4] float32 forward matrices, ``trunc`` in world units, ``views``: the views to integrate, in this order (None: all).
    Returns (tsdf float32 [nz,ny,nx], weight int32 [nz,ny,nx]) on the device: weight = the number of contributing views, tsdf = the mean of
    their clamped sdf / trunc (1 where no view contributes) - the contract is cer_mvs.h's, cer_tsdf_integrate_f32."""
    _check_maps(depths, masks, "tsdf_volume")
    origin, voxel, dims = _grid(grid, "tsdf_volume")
    trunc = _check_trunc(trunc, "tsdf_volume")
    N, h, w = (int(v) for v in depths.shape)
    cams = forward_cams(Ks, Es)
    if cams.shape[0] != N:
        raise ValueError(f"tsdf_volume: {N} cameras expected")
    views = _check_views(views, N, "tsdf_volume")
    if not depths.is_cuda:
        raise RuntimeError("tsdf_volume: depths must be a CUDA tensor (no CPU fallback)")
    dev = depths.device
    nx, ny, nz = dims
    tsdf = torch.ones(nz, ny, nx, device=dev, dtype=torch.float32)
    weight = torch.zeros(nz, ny, nx, device=dev, dtype=torch.int32)
    if not views or tsdf.numel() == 0:
        return tsdf, weight
    if h * w == 0:
        raise ValueError("tsdf_volume: empty depth maps")
    cams = cams.to(dev)
    vlist = torch.tensor(views, dtype=torch.int32).to(dev)
    L.check(L.load().cer_tsdf_integrate_f32(L.dev_ptr(depths.contiguous(), "depths"),
                                            L.dev_ptr(masks.contiguous(), "masks", torch.uint8) if masks is not None else None,
                                            L.dev_ptr(cams, "cams", torch.float64), N, h, w, L.dev_ptr(vlist, "views", torch.int32), len(views),
                                            origin, voxel, nx, ny, nz, trunc, L.dev_ptr(tsdf, "tsdf"), L.dev_ptr(weight, "weight", torch.int32),
                                            L.cur_stream()), "tsdf_integrate")
    return tsdf, weight


def _check_volumes(tsdf, weight, dims, who):
    nx, ny, nz = dims
    if not isinstance(tsdf, torch.Tensor) or tsdf.dtype != torch.float32 or tuple(tsdf.shape) != (nz, ny, nx):
        raise ValueError(f"{who}: tsdf float32 [{nz},{ny},{nx}] expected")
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.int32 or tuple(weight.shape) != (nz, ny, nx):
        raise ValueError(f"{who}: weight int32 [{nz},{ny},{nx}] expected")
    if tsdf.device != weight.device:
        raise ValueError(f"{who}: tsdf and weight must be on one device")


def mesh_counts(tsdf, weight, grid, min_weight=1):
    """The first half of ``extract_mesh``: (nv, nf, workspace) - the one synchronisation reads the two totals."""
    origin, voxel, dims = _grid(grid, "extract_mesh")
    _check_volumes(tsdf, weight, dims, "extract_mesh")
    min_weight = int(min_weight)
    if not tsdf.is_cuda:
        raise RuntimeError("extract_mesh: the volumes must be CUDA tensors (no CPU fallback)")
    nx, ny, nz = dims
    if min(dims) < 2:
        return 0, 0, None
    lib, dev = L.load(), tsdf.device
    tsdf, weight = tsdf.contiguous(), weight.contiguous()
    P = int(lib.cer_mesh_partials(nx, ny, nz))
    if P < 0:
        L.check(P, "mesh_partials")
    cells = torch.empty((nz - 1, ny - 1, nx - 1), device=dev, dtype=torch.int16)
    partials, offsets, totals = L.compaction_buffers(P, dev)
    pc = L.dev_ptr(cells, "cells", torch.int16)
    L.check(lib.cer_mesh_cells_u16(L.dev_ptr(tsdf, "tsdf"), L.dev_ptr(weight, "weight", torch.int32), nx, ny, nz, min_weight, pc,
                                   L.cur_stream()), "mesh_cells")
    L.check(lib.cer_mesh_count(pc, nx, ny, nz, L.dev_ptr(partials, "partials", torch.int32), L.dev_ptr(offsets, "offsets", torch.int64),
                               L.dev_ptr(totals, "totals", torch.int64), L.cur_stream()), "mesh_count")
    nv, nf = (int(v) for v in totals.cpu())                  # the one synchronisation: the outputs are allocated exactly
    if nv >= 2 ** 31 or nf >= 2 ** 31:
        raise ValueError(f"extract_mesh: {nv} vertices / {nf} faces is beyond int32 indices; take a larger voxel")
    return nv, nf, (tsdf, cells, offsets)


def mesh_emit(grid, nv, nf, workspace, vertex_capacity=None, face_capacity=None, vertices=None, faces=None):
    """The second half: the vertices and faces of ``mesh_counts``'s workspace.  With capacities below the totals the leading rows are written
    and nothing behind them (``vertices`` / ``faces``: the caller's arrays, at least that large)."""
    origin, voxel, dims = _grid(grid, "extract_mesh")
    vcap = nv if vertex_capacity is None else int(vertex_capacity)
    fcap = nf if face_capacity is None else int(face_capacity)
    if vcap < 0 or fcap < 0:
        raise ValueError("extract_mesh: capacities must not be negative")
    tsdf, cells, offsets = workspace
    dev = tsdf.device
    vertices = torch.empty(vcap, 3, device=dev, dtype=torch.float32) if vertices is None else vertices
    faces = torch.empty(fcap, 3, device=dev, dtype=torch.int32) if faces is None else faces
    if vertices.shape[0] < vcap or faces.shape[0] < fcap:
        raise ValueError("extract_mesh: the output arrays are smaller than the capacities")
    nx, ny, nz = dims
    vmap = torch.empty(nz * ny * nx * 8, device=dev, dtype=torch.int32)
    L.check(L.load().cer_mesh_emit_f32(L.dev_ptr(tsdf, "tsdf"), L.dev_ptr(cells, "cells", torch.int16), origin, voxel, nx, ny, nz,
                                       L.dev_ptr(offsets, "offsets", torch.int64), nv, nf, vcap, fcap, L.dev_ptr(vmap, "vmap", torch.int32),
                                       L.dev_ptr(vertices, "vertices") if vcap else None,
                                       L.dev_ptr(faces, "faces", torch.int32) if fcap else None, L.cur_stream()), "mesh_emit")
    return vertices, faces


def extract_mesh(tsdf, weight, grid, min_weight=1):
    """Marching tetrahedra on a volume: tsdf float32 / weight int32 [nz,ny,nx] on the device -> (vertices float32 [nv,3], faces int32 [nf,3])
    on the device.  A node is valid iff weight >= min_weight and tsdf is finite, inside iff tsdf < 0; a cell is meshed iff its eight corners
    are valid.  Every face normal points from inside to outside; every vertex is referenced; the order is the slot order of cer_mvs.h
    (cer_mesh_count).  The mesh is open where nodes are unobserved.  Workspace: 2 bytes per cell and 32 bytes per node."""
    nv, nf, ws = mesh_counts(tsdf, weight, grid, min_weight)
    if ws is None or (nv == 0 and nf == 0):
        dev = tsdf.device
        return torch.empty(0, 3, device=dev, dtype=torch.float32), torch.empty(0, 3, device=dev, dtype=torch.int32)
    return mesh_emit(grid, nv, nf, ws)


def mesh_from_depth_maps(depths, masks, Ks, Es, grid, trunc=None, views=None, min_weight=1, info=None):
    """``tsdf_volume`` then ``extract_mesh``.  ``trunc`` defaults to 3 voxels.  ``info`` (a dict) gains the grid, trunc, nv, nf and the number
    of observed nodes (weight >= min_weight)."""
    _, voxel, _ = _grid(grid, "mesh_from_depth_maps")
    trunc = 3.0 * voxel if trunc is None else _check_trunc(trunc, "mesh_from_depth_maps")
    tsdf, weight = tsdf_volume(depths, masks, Ks, Es, grid, trunc, views)
    vertices, faces = extract_mesh(tsdf, weight, grid, min_weight)
    if info is not None:
        info.update(grid=Grid(tuple(float(v) for v in grid[0]), float(grid[1]), tuple(int(v) for v in grid[2])), trunc=trunc,
                    nv=int(vertices.shape[0]), nf=int(faces.shape[0]), observed=int((weight >= int(min_weight)).sum()))
    return vertices, faces


# ---------------------------------------------------------------- per-vertex attributes (C ABI 1180)
def _check_vertices(vertices, who):
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"{who}: vertices float32 [nv, 3] expected")
    if vertices.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: {vertices.shape[0]} vertices is beyond int32 indices")


def vertex_colors(vertices, depths, masks, colors, Ks, Es, tol, views=None):
    """A colour per vertex from the views that see it: vertices float32 [nv,3], depths float32 [N,h,w], masks uint8 [N,h,w] (or None: every
    pixel) and colors float32 [N,3,h,w] (the planes ``fusion.point_cloud`` takes) on the device, Ks / Es the float32 forward matrices,
    ``views``: the views to ask, in this order (None: all).  A view sees a vertex iff it projects inside the image (``tsdf_volume``'s
    projection), the pixel is masked in, its depth d is finite and positive and ``|d - uz| <= tol`` (world units): the depth maps' own
    occlusion reasoning.  Each such view adds its bilinear sample.  Returns (rgb uint8 [nv,3], seen int32 [nv]) on the device: the mean
    colour times 255, truncated and clamped ((0, 0, 0) where ``seen`` is 0), and the number of views - the contract is cer_mvs.h's,
    cer_mesh_vertex_colors_u8."""
    who = "vertex_colors"
    _check_vertices(vertices, who)
    _check_maps(depths, masks, who)
    N, h, w = (int(v) for v in depths.shape)
    if not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32 or tuple(colors.shape) != (N, 3, h, w):
        raise ValueError(f"{who}: colors float32 [{N},3,{h},{w}] expected")
    if colors.device != depths.device or vertices.device != depths.device:
        raise ValueError(f"{who}: vertices, depths and colors must be on one device")
    tol = float(tol)
    if not (math.isfinite(tol) and tol > 0.0):
        raise ValueError(f"{who}: tol must be a positive finite number")
    cams = forward_cams(Ks, Es)
    if cams.shape[0] != N:
        raise ValueError(f"{who}: {N} cameras expected")
    views = _check_views(views, N, who)
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    dev, nv = vertices.device, int(vertices.shape[0])
    rgb = torch.zeros(nv, 3, device=dev, dtype=torch.uint8)
    seen = torch.zeros(nv, device=dev, dtype=torch.int32)
    if not views or nv == 0:
        return rgb, seen
    if h * w == 0:
        raise ValueError(f"{who}: empty depth maps")
    cams = cams.to(dev)
    vlist = torch.tensor(views, dtype=torch.int32).to(dev)
    L.check(L.load().cer_mesh_vertex_colors_u8(L.dev_ptr(vertices.contiguous(), "vertices"), nv, L.dev_ptr(depths.contiguous(), "depths"),
                                               L.dev_ptr(masks.contiguous(), "masks", torch.uint8) if masks is not None else None,
                                               L.dev_ptr(colors.contiguous(), "colors"), L.dev_ptr(cams, "cams", torch.float64), N, h, w,
                                               L.dev_ptr(vlist, "views", torch.int32), len(views), tol, L.dev_ptr(rgb, "rgb", torch.uint8),
                                               L.dev_ptr(seen, "seen", torch.int32), L.cur_stream()), "mesh_vertex_colors")
    return rgb, seen


def vertex_faces(faces, nv):
    """The faces around every vertex as a CSR list over the 3 nf corner entries ``faces.reshape(-1)`` (corner id = 3 * face + corner):
    faces int32 [nf,3] with indices in 0 .. nv-1 (ValueError otherwise) -> (starts int32 [nv + 1], order int32 [3 nf]) on the faces'
    device: ``order[starts[v] : starts[v + 1]]`` are the corner ids that name vertex v, ascending (a stable sort).  Torch ops only."""
    return _corner_list(_corner_keys(faces, nv), int(nv))


def _corner_keys(faces, nv):
    """``vertex_faces``' checks -> the flat corner entries"""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError("vertex_faces: faces int32 [nf, 3] expected")
    nv = int(nv)
    if nv < 0 or nv >= 2 ** 31 or 3 * faces.shape[0] >= 2 ** 31:
        raise ValueError("vertex_faces: nv and 3 nf must be in 0 .. 2^31 - 1")
    keys = faces.reshape(-1)
    if keys.numel() and (int(keys.min()) < 0 or int(keys.max()) >= nv):
        raise ValueError(f"vertex_faces: faces must hold indices in 0 .. {nv - 1}")
    return keys


def _corner_list(keys, nv):
    """``vertex_faces`` on the flat corner entries; entries below 0 sort in front of starts[0] and are in nobody's list"""
    ordered, order = torch.sort(keys, stable=True)
    starts = torch.searchsorted(ordered, torch.arange(nv + 1, device=keys.device, dtype=torch.int32))
    return starts.to(torch.int32), order.to(torch.int32)


def vertex_normals(vertices, faces):
    """Area-weighted vertex normals of any indexed triangle mesh (Open3D's ``compute_vertex_normals``): vertices float32 [nv,3] and faces
    int32 [nf,3] on the device -> float32 [nv,3] on the device: the sum of (B - A) x (C - A) over the corners that name the vertex, in
    corner order, normalised; (0, 0, 0) for an unreferenced vertex, cancelling faces and NaN - cer_mvs.h, cer_mesh_vertex_normals_f32."""
    _check_vertices(vertices, "vertex_normals")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError("vertex_normals: faces int32 [nf, 3] expected")
    if faces.device != vertices.device:
        raise ValueError("vertex_normals: vertices and faces must be on one device")
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    starts, order = vertex_faces(faces, nv)
    if not vertices.is_cuda:
        raise RuntimeError("vertex_normals: vertices must be a CUDA tensor (no CPU fallback)")
    normals = torch.zeros(nv, 3, device=vertices.device, dtype=torch.float32)
    if nv == 0:
        return normals
    L.check(L.load().cer_mesh_vertex_normals_f32(L.dev_ptr(vertices.contiguous(), "vertices"), nv,
                                                 L.dev_ptr(faces.contiguous(), "faces", torch.int32) if nf else None, nf,
                                                 L.dev_ptr(starts, "starts", torch.int32), L.dev_ptr(order, "order", torch.int32) if nf else None,
                                                 L.dev_ptr(normals, "normals"), L.cur_stream()), "mesh_vertex_normals")
    return normals


# ---------------------------------------------------------------- components and small-piece removal (C ABI 1190)
SWEEP_BATCH = 8                                              # sweeps per host read of the flags: a read costs less than a sweep of a large mesh


def _check_faces(faces, who):
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces int32 [nf, 3] expected")


def _count_option(value, name, who):
    """an int >= 1 (bool, float, 0 and negative values refused), or None"""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError(f"{who}: {name} must be an integer >= 1")
    return value


def _label_roots(faces, nv, starts, order):
    """labels int32 [nv]: every vertex's root (the smallest index of its component), and the number of sweeps run up to and including the
    first that changed nothing"""
    dev, nf = faces.device, int(faces.shape[0])
    labels = torch.arange(nv, device=dev, dtype=torch.int32)
    if nv == 0 or nf == 0:
        return labels, 0
    lib, done = L.load(), 0
    pf, ps, po = L.dev_ptr(faces, "faces", torch.int32), L.dev_ptr(starts, "starts", torch.int32), L.dev_ptr(order, "order", torch.int32)
    while done < nv + 1:
        n = min(SWEEP_BATCH, nv + 1 - done)
        flags = torch.zeros(n, device=dev, dtype=torch.int32)
        L.check(lib.cer_mesh_label_sweeps_i32(pf, nf, ps, po, nv, L.dev_ptr(labels, "labels", torch.int32), L.dev_ptr(flags, "flags", torch.int32),
                                              n, L.cur_stream()), "mesh_label_sweeps")
        changed = flags.cpu().tolist()                       # the batch's one host read
        if 0 in changed:
            return labels, done + changed.index(0) + 1
        done += n
    raise RuntimeError(f"mesh_components: the labels of {nv} vertices still changed in sweep {done}")


def _components(faces, nv, starts, order):
    """(vertex_component, face_component, n_faces, n_vertices, sweeps) of checked, contiguous device faces and their corner list"""
    dev = faces.device
    labels, sweeps = _label_roots(faces, nv, starts, order)
    roots = torch.nonzero(labels == torch.arange(nv, device=dev, dtype=torch.int32)).reshape(-1).to(torch.int32)      # ascending
    nc = int(roots.shape[0])
    vertex_component = torch.searchsorted(roots, labels).to(torch.int32)
    face_component = vertex_component[faces[:, 0].long()]
    n_faces = torch.bincount(face_component, minlength=nc)
    n_vertices = torch.bincount(vertex_component, minlength=nc)
    return vertex_component, face_component, n_faces, n_vertices, sweeps


def mesh_components(faces, nv, info=None):
    """The connected components of any indexed triangle mesh: faces int32 [nf,3] with indices in 0 .. nv-1 (ValueError otherwise) on the
    device -> (vertex_component int32 [nv], face_component int32 [nf], n_faces int64 [nc], n_vertices int64 [nc]) on the device.  Two
    vertices are connected iff a chain of faces links them through shared vertex indices - vertex connectivity, not Open3D's shared-edge
    adjacency of ``cluster_connected_triangles``: two pieces that touch in one vertex are ONE component.  Components are numbered by their
    smallest vertex index, ascending; an unreferenced vertex is a component with no face; a face belongs to its first index's component.
    ``info`` (a dict) gains "components" and "sweeps", the label sweeps run up to and including the first that changed nothing - the
    contract is cer_mvs.h's, cer_mesh_label_sweeps_i32."""
    _check_faces(faces, "mesh_components")
    starts, order = vertex_faces(faces, nv)
    nv = int(nv)
    if not faces.is_cuda:
        raise RuntimeError("mesh_components: faces must be a CUDA tensor (no CPU fallback)")
    vc, fc, n_faces, n_vertices, sweeps = _components(faces.contiguous(), nv, starts, order)
    if info is not None:
        info.update(components=int(n_faces.shape[0]), sweeps=sweeps)
    return vc, fc, n_faces, n_vertices


def _check_attribute(a, nv, name, dtype, who):
    if a is not None and (not isinstance(a, torch.Tensor) or a.dtype != dtype or tuple(a.shape) != (nv, 3)):
        raise ValueError(f"{who}: {name} {str(dtype).replace('torch.', '')} [{nv}, 3] (or None) expected")


def _check_mesh(vertices, faces, normals, colors, who):
    _check_vertices(vertices, who)
    _check_faces(faces, who)
    nv = int(vertices.shape[0])
    _check_attribute(normals, nv, "normals", torch.float32, who)
    _check_attribute(colors, nv, "colors", torch.uint8, who)
    for name, a in (("faces", faces), ("normals", normals), ("colors", colors)):
        if a is not None and a.device != vertices.device:
            raise ValueError(f"{who}: vertices and {name} must be on one device")


def _select(vertices, faces, keep, starts, order, normals, colors):
    """``select_faces`` on checked device arrays (vertices and faces contiguous, keep uint8 [nf]) and the faces' corner list"""
    dev, nv, nf = vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    lib = L.load()
    P = int(lib.cer_mesh_select_partials(nv, nf))
    if P < 0:
        L.check(P, "mesh_select_partials")
    nvo = nfo = 0
    if P:
        used = torch.empty(nv, device=dev, dtype=torch.uint8)
        partials, offsets, totals = L.compaction_buffers(P, dev)
        pf, pk, pu = L.dev_ptr(faces, "faces", torch.int32), L.dev_ptr(keep, "keep", torch.uint8), L.dev_ptr(used, "used", torch.uint8)
        L.check(lib.cer_mesh_select_count(pf, nf, L.dev_ptr(starts, "starts", torch.int32), L.dev_ptr(order, "order", torch.int32), nv, pk, pu,
                                          L.dev_ptr(partials, "partials", torch.int32), L.dev_ptr(offsets, "offsets", torch.int64),
                                          L.dev_ptr(totals, "totals", torch.int64), L.cur_stream()), "mesh_select_count")
        nvo, nfo = (int(v) for v in totals.cpu())            # the one synchronisation: the outputs are allocated exactly
    out_v = torch.empty(nvo, 3, device=dev, dtype=torch.float32)
    out_f = torch.empty(nfo, 3, device=dev, dtype=torch.int32)
    index = torch.empty(nvo, device=dev, dtype=torch.int32)
    if nvo or nfo:
        vmap = torch.empty(nv, device=dev, dtype=torch.int32)
        L.check(lib.cer_mesh_select_emit_f32(L.dev_ptr(vertices, "vertices"), nv, pf, nf, pk, pu, L.dev_ptr(offsets, "offsets", torch.int64), nvo, nfo,
                                             L.dev_ptr(vmap, "vmap", torch.int32), L.dev_ptr(out_v, "vertices") if nvo else None,
                                             L.dev_ptr(index, "index", torch.int32) if nvo else None,
                                             L.dev_ptr(out_f, "faces", torch.int32) if nfo else None, L.cur_stream()), "mesh_select_emit")
    gather = index.long()
    return (out_v, out_f, index, None if normals is None else normals.index_select(0, gather),
            None if colors is None else colors.index_select(0, gather))


def select_faces(vertices, faces, keep, normals=None, colors=None):
    """The sub-mesh of a face mask (Open3D's ``remove_triangles_by_mask`` then ``remove_unreferenced_vertices``): vertices float32 [nv,3],
    faces int32 [nf,3] with indices in 0 .. nv-1 (ValueError otherwise) and keep bool / uint8 [nf] on the device, ``normals`` float32 [nv,3]
    and ``colors`` uint8 [nv,3] optional -> (vertices', faces', index int32 [nv'], normals' | None, colors' | None) on the device.  Kept
    faces keep their order, with indices renumbered; a vertex survives iff a kept face names it, and survivors keep their order; ``index``
    holds the old index of every surviving vertex and the attributes are gathered with it - cer_mvs.h, cer_mesh_select_count."""
    who = "select_faces"
    _check_mesh(vertices, faces, normals, colors, who)
    nf = int(faces.shape[0])
    if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (nf,):
        raise ValueError(f"{who}: keep bool or uint8 [{nf}] expected")
    if keep.device != vertices.device:
        raise ValueError(f"{who}: vertices and keep must be on one device")
    starts, order = vertex_faces(faces, vertices.shape[0])
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    return _select(vertices.contiguous(), faces.contiguous(), keep.to(torch.uint8).contiguous(), starts, order, normals, colors)


def remove_small_components(vertices, faces, min_faces=None, keep_largest=None, normals=None, colors=None, info=None):
    """The mesh without its small pieces: component c of ``mesh_components`` is kept iff n_faces[c] >= ``min_faces`` (where given) and c is
    among the first ``keep_largest`` components sorted by (n_faces descending, id ascending) (where given); at least one of the two must be
    given, each an int >= 1 (ValueError otherwise).  Then ``select_faces`` on the kept components' faces, and its five results.  ``info`` (a
    dict) gains "components", "removed_components" (those not kept, faceless ones included), "removed_faces", "removed_vertices" and
    "sweeps"."""
    who = "remove_small_components"
    min_faces = _count_option(min_faces, "min_faces", who)
    keep_largest = _count_option(keep_largest, "keep_largest", who)
    if min_faces is None and keep_largest is None:
        raise ValueError(f"{who}: give min_faces or keep_largest (or both)")
    _check_mesh(vertices, faces, normals, colors, who)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    starts, order = vertex_faces(faces, nv)
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    vertices, faces = vertices.contiguous(), faces.contiguous()
    _, face_component, n_faces, _, sweeps = _components(faces, nv, starts, order)
    nc = int(n_faces.shape[0])
    kept = torch.ones(nc, device=faces.device, dtype=torch.bool)
    if min_faces is not None:
        kept &= n_faces >= min_faces
    if keep_largest is not None:
        by_size = torch.sort(n_faces, descending=True, stable=True).indices                  # ties: the smaller id first
        first = torch.zeros(nc, device=faces.device, dtype=torch.bool)
        first[by_size[:keep_largest]] = True
        kept &= first
    keep = kept[face_component.long()].to(torch.uint8)
    out = _select(vertices, faces, keep, starts, order, normals, colors)
    if info is not None:
        info.update(components=nc, removed_components=nc - int(kept.sum()), removed_faces=nf - int(out[1].shape[0]),
                    removed_vertices=nv - int(out[0].shape[0]), sweeps=sweeps)
    return out


# ---------------------------------------------------------------- simplification by vertex clustering (C ABI 1200)
REPRESENTATIVES = ("quadric", "mean")
SIMPLIFY_KEYS = ("voxels", "cell", "representative", "regularisation")


def _positive(value, name, who):
    """a positive finite number as a float (bool refused)"""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not (math.isfinite(value) and value > 0):
        raise ValueError(f"{who}: {name} must be a positive finite number")
    return float(value)


def _representative(value, who):
    if not isinstance(value, str) or value not in REPRESENTATIVES:
        raise ValueError(f"{who}: representative must be one of {list(REPRESENTATIVES)}")
    return value


def simplify_vertex_clustering(vertices, faces, cell, representative="quadric", regularisation=1e-3, colors=None, info=None):
    """Vertex clustering (Rossignac-Borrel; Open3D's ``simplify_vertex_clustering``) of any indexed triangle mesh: vertices float32 [nv,3] and
    faces int32 [nf,3] with indices in 0 .. nv-1 (ValueError otherwise) on the device, ``colors`` uint8 [nv,3] optional -> (vertices', faces',
    cluster int32 [nv], colors' | None) on the device.  The vertices inside one cell of edge ``cell`` (the occupied cells of
    ``cloud_eval.CloudIndex(vertices, cell)``: origin at the per-axis minimum of the finite vertices; more than 2^20 cells along an axis is
    its ValueError) become one vertex: with ``representative`` "mean" their mean, with "quadric" (Lindstrom) the point that minimises the
    summed squared distances to the planes of the faces around them, regularised towards the mean with weight ``regularisation`` (a finite
    number > 0) times the quadric's mean eigenvalue, and the mean itself where that point is not well defined or leaves the cell.  Colours
    are the members' integer mean.  A face stays iff its three vertices fall into three different cells; it is rotated so that its smallest
    new index comes first (orientation kept); of faces that are then equal the one with the lowest index stays (opposite orientations are
    different faces); faces keep their order.  A cell that no surviving face names is dropped.  ``cluster[v]``: the output index of v's cell,
    -1 for a non-finite vertex or a dropped cell.  ``info`` (a dict) gains "clusters" (occupied cells), "degenerate_faces" (not valid),
    "duplicate_faces", "dropped_clusters" and "quadric" (cells that took the minimiser).

    Guaranteed: distinct indices per face, no two faces equal up to rotation, every vertex referenced, and if every directed edge of the
    input has its reverse, so has every directed edge of the output.  NOT guaranteed: manifoldness - one directed edge may appear in two
    faces, and the Euler characteristic changes.  Normals are not carried: call ``vertex_normals`` on the result.  The contract is
    cer_mvs.h's, "Mesh simplification"."""
    who = "simplify_vertex_clustering"
    _check_mesh(vertices, faces, None, colors, who)
    cell = _positive(cell, "cell", who)
    regularisation = _positive(regularisation, "regularisation", who)
    quadric = _representative(representative, who) == "quadric"
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    if quadric:
        starts, corner_order = vertex_faces(faces, nv)
    else:                                                    # the mean walks no face: the range check alone
        _corner_keys(faces, nv)
        starts = corner_order = None
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    from .cloud_eval import CloudIndex
    dev, lib = vertices.device, L.load()
    vertices, faces = vertices.contiguous(), faces.contiguous()
    colors = None if colors is None else colors.contiguous()
    index = CloudIndex(vertices, cell)                       # keys, the stable sort and the cell table: the clusters and their member order
    nc = int(index.cells)
    p_order, p_start = L.dev_ptr(index.order, "order", torch.int64), L.dev_ptr(index.cell_start, "cell_start", torch.int64)
    pv, pf = L.dev_ptr(vertices, "vertices"), L.dev_ptr(faces, "faces", torch.int32)
    cluster = torch.empty(nv, device=dev, dtype=torch.int32)
    L.check(lib.cer_mesh_cluster_map_i32(p_order, p_start, nv, nc, L.dev_ptr(cluster, "cluster", torch.int32), L.cur_stream()), "mesh_cluster_map")
    reps = torch.empty(nc, 3, device=dev, dtype=torch.float32)
    took = torch.zeros(nc, device=dev, dtype=torch.uint8)
    rep_colors = None if colors is None else torch.empty(nc, 3, device=dev, dtype=torch.uint8)
    L.check(lib.cer_mesh_cluster_reps_f32(pv, nv, pf, nf, L.dev_ptr(starts, "starts", torch.int32), L.dev_ptr(corner_order, "order", torch.int32),
                                          p_order, p_start, L.dev_ptr(index.cell_keys, "cell_keys", torch.int64), nc, index.origin, cell,
                                          int(quadric), regularisation, L.dev_ptr(colors, "colors", torch.uint8), L.dev_ptr(reps, "reps"),
                                          L.dev_ptr(rep_colors, "rep_colors", torch.uint8), L.dev_ptr(took, "took", torch.uint8), L.cur_stream()),
            "mesh_cluster_reps")
    triples = torch.empty(nf, 3, device=dev, dtype=torch.int32)
    valid = torch.empty(nf, device=dev, dtype=torch.uint8)
    keep = torch.empty(nf, device=dev, dtype=torch.uint8)
    pt, pk = L.dev_ptr(triples, "triples", torch.int32), L.dev_ptr(valid, "valid", torch.uint8)
    L.check(lib.cer_mesh_cluster_faces_i32(pf, nf, L.dev_ptr(cluster, "cluster", torch.int32), nv, pt, pk, L.cur_stream()), "mesh_cluster_faces")
    t = triples.long()
    by_bc = torch.sort((t[:, 1] << 31) | t[:, 2], stable=True).indices                     # lexicographic: (b, c) first, then a, both stable
    perm = by_bc[torch.sort(t[:, 0][by_bc], stable=True).indices].contiguous()
    L.check(lib.cer_mesh_face_heads_u8(pt, pk, L.dev_ptr(perm, "perm", torch.int64), nf, L.dev_ptr(keep, "keep", torch.uint8), L.cur_stream()),
            "mesh_face_heads")
    t_starts, t_order = _corner_list(triples.reshape(-1), nc)                              # (the -1 of an invalid face is in nobody's list)
    out_v, out_f, kept, _, out_c = _select(reps, triples, keep, t_starts, t_order, None, rep_colors)
    nvo = int(out_v.shape[0])
    new_of = torch.full((nc + 1,), -1, device=dev, dtype=torch.int32)                      # the last slot answers cluster == -1
    new_of[kept.long()] = torch.arange(nvo, device=dev, dtype=torch.int32)
    cluster = new_of[cluster.long()]
    if info is not None:
        n_valid, n_kept = int(valid.sum()), int(out_f.shape[0])
        info.update(clusters=nc, degenerate_faces=nf - n_valid, duplicate_faces=n_valid - n_kept, dropped_clusters=nc - nvo,
                    quadric=int(took.sum()))
    return out_v, out_f, cluster, out_c


# ---------------------------------------------------------------- edges, topology report and smoothing (C ABI 1210)
SMOOTH_METHODS = ("taubin", "laplacian")
SMOOTH_BOUNDARIES = ("fixed", "free")
SMOOTH_KEYS = ("iterations", "method", "lam", "mu", "boundary")
DEFAULT_MU = -0.53
FLAG_FINITE, FLAG_FROZEN, FLAG_BOUNDARY = 1, 2, 4            # cer_mvs.h, cer_mesh_smooth_prepare_f32


def _edge_checks(faces, nv, who):
    """``vertex_faces``' checks in its wording, and 6 nf < 2^31 -> (nv, nf)"""
    if isinstance(faces, torch.Tensor) and faces.dim() == 2 and 6 * faces.shape[0] >= 2 ** 31:        # (before the range check reads the faces)
        raise ValueError(f"{who}: 6 nf must be in 0 .. 2^31 - 1")
    _corner_keys(faces, nv)
    return int(nv), int(faces.shape[0])


def _edges(faces, nv):
    """``mesh_edges`` on checked, contiguous device faces -> (nbr_starts, nbrs, along, against, owner int32 [nn])"""
    dev, nf = faces.device, int(faces.shape[0])
    lib = L.load()
    nn = 0
    if nf:
        P = int(lib.cer_mesh_edge_partials(nf))
        if P < 0:
            L.check(P, "mesh_edge_partials")
        keys = torch.empty(6 * nf, device=dev, dtype=torch.int64)
        L.check(lib.cer_mesh_edge_keys_i64(L.dev_ptr(faces, "faces", torch.int32), nf, nv, L.dev_ptr(keys, "keys", torch.int64), L.cur_stream()),
                "mesh_edge_keys")
        keys = torch.sort(keys).values                       # equal keys are indistinguishable: no stability needed
        partials, offsets, totals = L.compaction_buffers(P, dev)
        pk = L.dev_ptr(keys, "keys", torch.int64)
        L.check(lib.cer_mesh_edge_count(pk, nf, L.dev_ptr(partials, "partials", torch.int32), L.dev_ptr(offsets, "offsets", torch.int64),
                                        L.dev_ptr(totals, "totals", torch.int64), L.cur_stream()), "mesh_edge_count")
        nn = int(totals[0].cpu())                            # the one synchronisation: the outputs are allocated exactly
    owner, nbrs, along, against = (torch.empty(nn, device=dev, dtype=torch.int32) for _ in range(4))
    if nn:
        L.check(lib.cer_mesh_edge_emit_i32(pk, nf, L.dev_ptr(offsets, "offsets", torch.int64), nn, L.dev_ptr(owner, "owner", torch.int32),
                                           L.dev_ptr(nbrs, "nbrs", torch.int32), L.dev_ptr(along, "along", torch.int32),
                                           L.dev_ptr(against, "against", torch.int32), L.cur_stream()), "mesh_edge_emit")
    starts = torch.searchsorted(owner, torch.arange(nv + 1, device=dev, dtype=torch.int32)).to(torch.int32)
    return starts, nbrs, along, against, owner


def mesh_edges(faces, nv):
    """The unique-neighbour list of every vertex of any indexed triangle mesh - its duplicate-free edge table with a count per direction:
    faces int32 [nf,3] with indices in 0 .. nv-1 (ValueError otherwise, ``vertex_faces``' rule; 6 nf < 2^31) on the device -> (nbr_starts
    int32 [nv + 1], nbrs int32 [nn], along int32 [nn], against int32 [nn]) on the device.  Face (i0, i1, i2) has the directed edges i0->i1,
    i1->i2, i2->i0; one with equal ends is skipped.  ``nbrs[nbr_starts[v] : nbr_starts[v + 1]]`` are the distinct vertices u that share an
    edge with v, ascending; ``along`` counts the directed edges v->u and ``against`` the directed edges u->v, so the entry (u, v) mirrors
    (v, u) with the counts swapped and nn is even - the contract is cer_mvs.h's, "Mesh edges and smoothing"."""
    nv, _ = _edge_checks(faces, nv, "mesh_edges")
    if not faces.is_cuda:
        raise RuntimeError("mesh_edges: faces must be a CUDA tensor (no CPU fallback)")
    return _edges(faces.contiguous(), nv)[:4]


def edge_table(nbr_starts, nbrs, along, against):
    """The undirected edges of ``mesh_edges``' list: its entries with v < u, ordered by (v, u) -> (lo int32 [ne], hi int32 [ne], n_lo_hi
    int32 [ne], n_hi_lo int32 [ne]): the ends and the number of directed edges lo->hi and hi->lo.  A torch mask."""
    nv, nn = int(nbr_starts.shape[0]) - 1, int(nbrs.shape[0])
    counts = (nbr_starts[1:] - nbr_starts[:-1]).long()
    owner = torch.repeat_interleave(torch.arange(nv, device=nbrs.device, dtype=torch.int32), counts, output_size=nn)
    mask = owner < nbrs
    return owner[mask], nbrs[mask], along[mask], against[mask]


TOPOLOGY_KEYS = ("vertices", "faces", "edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "boundary_vertices",
                 "unreferenced_vertices", "degenerate_faces", "boundary_loops", "euler", "closed", "edge_manifold", "oriented")


def _boundary_mask(nv, owner, along, against):
    """bool [nv]: the vertices on an edge with one face"""
    on = ((along + against) == 1).to(torch.int32)
    return torch.zeros(nv, device=owner.device, dtype=torch.int32).scatter_reduce_(0, owner.long(), on, "amax") > 0     # (a maximum: order-free)


def mesh_topology(faces, nv):
    """What a mesh is, as a dict of Python ints and bools (TOPOLOGY_KEYS): faces int32 [nf,3] with indices in 0 .. nv-1 (``mesh_edges``'
    checks) on the device.  With n = the number of faces on an undirected edge (both directions): "edges"; "boundary_edges": n == 1;
    "nonmanifold_edges": n > 2; "inconsistent_edges": n == 2 with both faces running along it in one direction; "boundary_vertices": on a
    boundary edge; "unreferenced_vertices": named by no face; "degenerate_faces": a repeated index; "boundary_loops": the connected
    components of the graph of boundary edges (``mesh_components``' label sweeps on the faces (a, b, b) of the boundary edges, counting the
    components that own an edge); "euler": V - E + F with V the referenced vertices and F every face; "closed": no boundary edge and at
    least one face; "edge_manifold": no non-manifold edge; "oriented": edge-manifold and no inconsistent edge.  Torch reductions over the
    edge table whose figures come back in one host read (after ``mesh_edges``' own), plus the sweeps' reads where there is a boundary."""
    nv, nf = _edge_checks(faces, nv, "mesh_topology")
    if not faces.is_cuda:
        raise RuntimeError("mesh_topology: faces must be a CUDA tensor (no CPU fallback)")
    faces = faces.contiguous()
    dev = faces.device
    starts, nbrs, along, against, owner = _edges(faces, nv)
    half = owner < nbrs                                      # every edge once
    total = along + against
    one_way = (along == 0) | (against == 0)
    boundary = _boundary_mask(nv, owner, along, against)
    referenced = torch.zeros(nv, device=dev, dtype=torch.bool)
    referenced[faces.reshape(-1).long()] = True
    degenerate = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])
    figures = torch.stack([half.sum(), (half & (total == 1)).sum(), (half & (total > 2)).sum(), (half & (total == 2) & one_way).sum(), boundary.sum(),
                           referenced.sum(), degenerate.sum()]).cpu().tolist()          # the one host read
    ne, nb, nm, ni, nbv, nref, ndeg = (int(v) for v in figures)
    loops = 0
    if nb:
        is_b = half & (total == 1)
        lo, hi = owner[is_b], nbrs[is_b]
        bfaces = torch.stack([lo, hi, hi], 1).contiguous()
        bstarts, border = _corner_list(bfaces.reshape(-1), nv)
        labels, _ = _label_roots(bfaces, nv, bstarts, border)
        loops = int(((labels == torch.arange(nv, device=dev, dtype=torch.int32)) & boundary).sum())   # a root that owns an edge
    return dict(vertices=nv, faces=nf, edges=ne, boundary_edges=nb, nonmanifold_edges=nm, inconsistent_edges=ni, boundary_vertices=nbv,
                unreferenced_vertices=nv - nref, degenerate_faces=ndeg, boundary_loops=loops, euler=nref - ne + nf, closed=nb == 0 and nf >= 1,
                edge_manifold=nm == 0, oriented=nm == 0 and ni == 0)


def _smooth_arguments(iterations, method, lam, mu, boundary, who):
    """``smooth_mesh``'s scalar arguments, checked -> (iterations, method, lam, mu, boundary)"""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
        raise ValueError(f"{who}: iterations must be an integer >= 1")
    if not isinstance(method, str) or method not in SMOOTH_METHODS:
        raise ValueError(f"{who}: method must be one of {list(SMOOTH_METHODS)}")
    if not isinstance(boundary, str) or boundary not in SMOOTH_BOUNDARIES:
        raise ValueError(f"{who}: boundary must be one of {list(SMOOTH_BOUNDARIES)}")
    number = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)
    if not number(lam) or not 0.0 < lam <= 1.0:
        raise ValueError(f"{who}: lam must be a finite number in (0, 1]")
    if not number(mu) or not (mu < -lam or (method == "laplacian" and mu == DEFAULT_MU)):       # (the default left alone where it is not read)
        raise ValueError(f"{who}: mu must be a finite number below -lam")
    return int(iterations), method, float(lam), float(mu), boundary


def smooth_mesh(vertices, faces, iterations, method="taubin", lam=0.5, mu=-0.53, boundary="fixed", info=None):
    """Taubin's lambda|mu smoothing (Open3D's ``filter_smooth_taubin``) or plain Laplacian smoothing (``filter_smooth_laplacian``) of any
    indexed triangle mesh: vertices float32 [nv,3] and faces int32 [nf,3] with indices in 0 .. nv-1 (``mesh_edges``' checks) on the device
    -> vertices' float32 [nv,3] on the device; the faces are untouched.  One step with weight w moves every movable vertex to
    p + w * (mean of its finite neighbours in ``mesh_edges``' list - p), in fp64, from the previous step's positions; "laplacian": one step
    with ``lam`` per iteration, which shrinks the surface; "taubin": a step with ``lam`` then a step with ``mu`` < -lam, which undoes the
    shrinkage.  ``iterations``: an int >= 1; ``lam``: finite, in (0, 1]; ``mu``: finite, < -lam (read for "taubin" only, but checked whenever it is
    given: under "laplacian" only the default passes without being below -lam).  A
    vertex is frozen - it never moves and returns its input bits - iff it is non-finite in the input, has no finite neighbour or, with
    ``boundary`` "fixed", lies on a boundary edge (``mesh_topology``'s "boundary_vertices"); "free" moves boundary vertices like any other.
    Non-finite vertices are left out of every neighbour's mean.  The result is rounded to float32 once, after the last step.  ``info`` (a
    dict) gains "moved" (vertices not frozen), "frozen_boundary" (boundary vertices with "fixed", 0 with "free"), "steps" and "edges".  The
    contract is cer_mvs.h's, "Mesh edges and smoothing"."""
    who = "smooth_mesh"
    _check_mesh(vertices, faces, None, None, who)
    iterations, method, lam, mu, boundary = _smooth_arguments(iterations, method, lam, mu, boundary, who)
    nv, _ = _edge_checks(faces, vertices.shape[0], who)
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    dev, lib = vertices.device, L.load()
    vertices = vertices.contiguous()
    starts, nbrs, along, against, _ = _edges(faces.contiguous(), nv)
    nn = int(nbrs.shape[0])
    steps = iterations * (2 if method == "taubin" else 1)
    fixed = boundary == "fixed"
    walk = torch.empty(nn, device=dev, dtype=torch.int32)
    flags = torch.zeros(nv, device=dev, dtype=torch.uint8)
    state = torch.empty(2, nv, 3, device=dev, dtype=torch.float64)
    out = torch.empty(nv, 3, device=dev, dtype=torch.float32)
    ps, pw, pf = L.dev_ptr(starts, "nbr_starts", torch.int32), L.dev_ptr(walk, "walk", torch.int32) if nn else None, L.dev_ptr(flags, "flags", torch.uint8)
    pa, pb = L.dev_ptr(state[0], "state", torch.float64), L.dev_ptr(state[1], "state", torch.float64)
    if nv:
        L.check(lib.cer_mesh_smooth_prepare_f32(L.dev_ptr(vertices, "vertices"), nv, ps, L.dev_ptr(nbrs, "nbrs", torch.int32) if nn else None,
                                                L.dev_ptr(along, "along", torch.int32) if nn else None,
                                                L.dev_ptr(against, "against", torch.int32) if nn else None, nn, int(fixed), pw, pf, pa,
                                                L.cur_stream()), "mesh_smooth_prepare")
        L.check(lib.cer_mesh_smooth_steps_f64(pa, pb, nv, ps, pw, nn, pf, lam, mu if method == "taubin" else lam, steps, L.cur_stream()),
                "mesh_smooth_steps")
        L.check(lib.cer_mesh_smooth_finish_f32(pb if steps & 1 else pa, L.dev_ptr(vertices, "vertices"), pf, nv, L.dev_ptr(out, "out"),
                                               L.cur_stream()), "mesh_smooth_finish")
    if info is not None:
        frozen, on_boundary = (int(v) for v in torch.stack([((flags & FLAG_FROZEN) != 0).sum(), ((flags & FLAG_BOUNDARY) != 0).sum()]).cpu())
        info.update(moved=nv - frozen, frozen_boundary=on_boundary if fixed else 0, steps=steps, edges=nn // 2)
    return out


def _smooth_option(value):
    """the "smooth" option, checked -> (iterations, method, lam, mu, boundary)"""
    if not isinstance(value, dict):
        return _smooth_arguments(value, "taubin", 0.5, -0.53, "fixed", "mesh: smooth")
    if set(value) - set(SMOOTH_KEYS) or "iterations" not in value:
        raise ValueError(f"mesh: smooth must be an integer >= 1 or a dictionary with \"iterations\" and keys of {list(SMOOTH_KEYS)}")
    return _smooth_arguments(value["iterations"], value.get("method", "taubin"), value.get("lam", 0.5), value.get("mu", -0.53),
                             value.get("boundary", "fixed"), "mesh: smooth")


# ---------------------------------------------------------------- hole filling (csrc/mesh_fill.hip, C ABI 1220)
FILL_INFO_KEYS = ("holes", "added_vertices", "added_faces", "pinched_vertices", "boundary_edges_before")
NEXT_PINCHED = -2                                            # cer_mvs.h, cer_mesh_hole_next_i32


def _max_edges(value, who):
    """an int >= 3 (bool and float refused), held to what a C int carries - no cycle is longer than nv < 2^31"""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 3:
        raise ValueError(f"{who}: max_edges must be an integer >= 3")
    return min(int(value), 2 ** 31 - 1)


def _hole_tables(faces, nv, max_edges, vertices):
    """``mesh_edges``, then the two walks on checked, contiguous device arrays -> (next int32 [nv], length int32 [nv], along, against)"""
    dev, lib = faces.device, L.load()
    starts, nbrs, along, against, _ = _edges(faces, nv)
    nn = int(nbrs.shape[0])
    nxt = torch.empty(nv, device=dev, dtype=torch.int32)
    length = torch.empty(nv, device=dev, dtype=torch.int32)
    if nv:
        pn = L.dev_ptr(nxt, "next", torch.int32)
        L.check(lib.cer_mesh_hole_next_i32(L.dev_ptr(starts, "nbr_starts", torch.int32), L.dev_ptr(nbrs, "nbrs", torch.int32) if nn else None,
                                           L.dev_ptr(along, "along", torch.int32) if nn else None,
                                           L.dev_ptr(against, "against", torch.int32) if nn else None, nv, nn, pn, L.cur_stream()), "mesh_hole_next")
        L.check(lib.cer_mesh_hole_heads_i32(pn, L.dev_ptr(vertices, "vertices"), nv, max_edges, L.dev_ptr(length, "length", torch.int32),
                                            L.cur_stream()), "mesh_hole_heads")
    return nxt, length, along, against


def mesh_holes(faces, nv, max_edges, vertices=None):
    """The small boundary loops of any indexed triangle mesh: faces int32 [nf,3] with indices in 0 .. nv-1 (``mesh_edges``' checks) on the
    device, ``max_edges`` an int >= 3, ``vertices`` float32 [nv,3] optional -> (head int32 [nh], length int32 [nh]) on the device, heads
    ascending.  With ``mesh_edges``' counts the directed edge a->b is a boundary half-edge iff along(a, b) == 1 and against(a, b) == 0; a
    vertex is simple iff exactly one leaves it and exactly one enters it, and its successor is the head of the one that leaves.  A hole is a
    cycle of successors through simple vertices only, 3 .. ``max_edges`` edges long, named by its smallest index; with ``vertices`` a cycle
    that holds a non-finite vertex is not one.  A cycle through a pinched vertex (a bow tie, the ends of an inconsistent edge, beside a
    non-manifold edge) or a longer one - the outer rim of an open scan - is left alone.  The contract is cer_mvs.h's, "Mesh hole filling"."""
    who = "mesh_holes"
    max_edges = _max_edges(max_edges, who)
    nv, _ = _edge_checks(faces, nv, who)
    if vertices is not None:
        _check_vertices(vertices, who)
        if int(vertices.shape[0]) != nv:
            raise ValueError(f"{who}: vertices float32 [{nv}, 3] (or None) expected")
        if vertices.device != faces.device:
            raise ValueError(f"{who}: vertices and faces must be on one device")
    if not faces.is_cuda:
        raise RuntimeError(f"{who}: faces must be a CUDA tensor (no CPU fallback)")
    _, length, _, _ = _hole_tables(faces.contiguous(), nv, max_edges, None if vertices is None else vertices.contiguous())
    heads = torch.nonzero(length).reshape(-1)                # ascending
    return heads.to(torch.int32), length[heads]


def fill_holes(vertices, faces, max_edges, colors=None, info=None):
    """The mesh with its small holes closed: vertices float32 [nv,3] and faces int32 [nf,3] with indices in 0 .. nv-1 (``mesh_edges``'
    checks) on the device, ``max_edges`` an int >= 3, ``colors`` uint8 [nv,3] optional -> (vertices', faces', hole int32 [nf'], colors' |
    None) on the device.  The nv vertices and nf faces come first, bit-identical and in order; then the fill of every hole of
    ``mesh_holes(faces, nv, max_edges, vertices)``, hole by hole in head order.  A hole a0 -> a1 -> a2 of three edges gets the one face
    (a0, a2, a1) and no vertex; a hole a0 .. a(n-1) of four and more gets one new vertex c - per axis the fp64 sum of its members in cycle
    order divided by n, rounded to float32 once - and the fan (a(k+1), a_k, c), k = 0 .. n-1; the new vertices sit behind the old ones in head
    order, and the colour of c is the members' integer mean per channel.  ``hole[f]``: -1 for an input face, otherwise the position of its
    hole in ``mesh_holes``' list.  Every fill face runs against the half-edge it closes: a hole in an oriented mesh leaves the mesh
    oriented, and every filled boundary edge becomes interior.  ``info`` (a dict) gains "holes" (filled), "added_vertices", "added_faces",
    "pinched_vertices" (touched by a boundary half-edge but not simple) and "boundary_edges_before"; how many loops there are in all is
    ``mesh_topology``'s "boundary_loops".

    A loop and the rim of an island are the same thing topologically - a small floating piece of k boundary edges <= ``max_edges`` gets a
    cap as well: call ``remove_small_components`` first.  A fan around the mean suits the near-planar, near-convex loops that unobserved
    nodes leave; it is not curvature-aware.  Normals are not carried: call ``vertex_normals`` on the result.  ValueError (the one raised
    after the device's counts are known): more than 2^31 - 1 vertices or face corners in the result.  The contract is cer_mvs.h's,
    "Mesh hole filling"."""
    who = "fill_holes"
    _check_mesh(vertices, faces, None, colors, who)
    max_edges = _max_edges(max_edges, who)
    nv, nf = _edge_checks(faces, vertices.shape[0], who)
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    dev = vertices.device
    vertices, faces = vertices.contiguous(), faces.contiguous()
    colors = None if colors is None else colors.contiguous()
    nxt, length, along, against = _hole_tables(faces, nv, max_edges, vertices)
    heads = torch.nonzero(length).reshape(-1)                # ascending
    nh = int(heads.shape[0])
    lens = length[heads]
    n_faces = torch.where(lens == 3, torch.ones_like(lens), lens).long()
    n_vertices = (lens > 3).long()
    face_offsets = (torch.cumsum(n_faces, 0) - n_faces).contiguous()                        # exclusive
    vertex_offsets = (torch.cumsum(n_vertices, 0) - n_vertices).contiguous()
    figures = torch.stack([n_faces.sum(), n_vertices.sum(), (nxt == NEXT_PINCHED).sum(), ((along + against) == 1).sum()]).cpu().tolist()
    added_faces, added_vertices, pinched, boundary_entries = (int(x) for x in figures)      # the one host read after mesh_edges' own
    if nv + added_vertices >= 2 ** 31 or 3 * (nf + added_faces) >= 2 ** 31:
        raise ValueError(f"{who}: {nv + added_vertices} vertices / {nf + added_faces} faces is beyond int32 indices")
    out_v = torch.empty(nv + added_vertices, 3, device=dev, dtype=torch.float32)
    out_f = torch.empty(nf + added_faces, 3, device=dev, dtype=torch.int32)
    hole = torch.empty(nf + added_faces, device=dev, dtype=torch.int32)
    out_c = None if colors is None else torch.empty(nv + added_vertices, 3, device=dev, dtype=torch.uint8)
    out_v[:nv] = vertices
    out_f[:nf] = faces
    hole[:nf] = -1
    if colors is not None:
        out_c[:nv] = colors
    if nh:
        heads32, lens = heads.to(torch.int32), lens.contiguous()
        L.check(L.load().cer_mesh_hole_fill_f32(L.dev_ptr(nxt, "next", torch.int32), L.dev_ptr(heads32, "heads", torch.int32),
                                                L.dev_ptr(lens, "lengths", torch.int32), L.dev_ptr(face_offsets, "face_offsets", torch.int64),
                                                L.dev_ptr(vertex_offsets, "vertex_offsets", torch.int64), nh,
                                                L.dev_ptr(vertices, "vertices") if added_vertices else None,
                                                L.dev_ptr(colors, "colors", torch.uint8), nv, nf, added_vertices, added_faces,
                                                L.dev_ptr(out_v, "vertices") if added_vertices else None, L.dev_ptr(out_f, "faces", torch.int32),
                                                L.dev_ptr(hole, "hole", torch.int32), L.dev_ptr(out_c, "colors", torch.uint8), L.cur_stream()),
                "mesh_hole_fill")
    if info is not None:
        info.update(holes=nh, added_vertices=added_vertices, added_faces=added_faces, pinched_vertices=pinched,
                    boundary_edges_before=boundary_entries // 2)                            # (every edge is in the list from both ends)
    return out_v, out_f, hole, out_c


def _fill_option(value):
    """the "fill_holes" option, checked -> max_edges"""
    if isinstance(value, bool) or not isinstance(value, int) or value < 3:
        raise ValueError("mesh: fill_holes must be an integer >= 3 (the longest loop to close, in edges)")
    return value


# ---------------------------------------------------------------- surface sampling (csrc/mesh_sample.hip, C ABI 1230)
SAMPLE_INFO_KEYS = ("n", "area", "faces_with_weight", "shift")
SAMPLE_MAX = 2 ** 31 - 1                                     # samples per call, and 3 nf
SAMPLE_OPTION_KEYS = ("n", "density", "spacing", "seed")


def _sample_mesh_checks(vertices, faces, colors, who):
    """the mesh of the sampling calls, checked without a device -> (nv, nf)"""
    _check_mesh(vertices, faces, None, colors, who)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    if 3 * nf > SAMPLE_MAX:
        raise ValueError(f"{who}: 3 nf must be in 0 .. 2^31 - 1")
    return nv, nf


def _word64(value, name, who):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) < 2 ** 64:
        raise ValueError(f"{who}: {name} must be an integer in 0 .. 2^64 - 1")
    return int(value)


def _sample_count(value, name, who):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= SAMPLE_MAX:
        raise ValueError(f"{who}: {name} must be an integer in 0 .. 2^31 - 1")
    return int(value)


def _areas(vertices, faces, nv, nf):
    """``face_areas`` on checked, contiguous device arrays"""
    areas = torch.empty(nf, device=vertices.device, dtype=torch.float64)
    if nf:
        L.check(L.load().cer_mesh_face_areas_f64(L.dev_ptr(vertices, "vertices") if nv else None, nv, L.dev_ptr(faces, "faces", torch.int32), nf,
                                                 L.dev_ptr(areas, "areas", torch.float64), L.cur_stream()), "mesh_face_areas")
    return areas


def face_areas(vertices, faces):
    """The area of every face of any indexed triangle mesh: vertices float32 [nv,3] and faces int32 [nf,3] on the device -> float64 [nf] on
    the device.  In fp64 on the float32 coordinates: e1 = b - a, e2 = c - a, n = e1 x e2 with every product and difference rounded on its
    own, area = 0.5 * sqrt((nx*nx + ny*ny) + nz*nz).  A face with an index outside 0 .. nv-1, with a repeated index or with a non-finite
    coordinate has area 0: it is not refused.  The contract is cer_mvs.h's, "Mesh surface sampling"."""
    who = "face_areas"
    nv, nf = _sample_mesh_checks(vertices, faces, None, who)
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    return _areas(vertices.contiguous(), faces.contiguous(), nv, nf)


def _sample_table(vertices, faces, nv, nf):
    """the prefix sums of the integer weights on checked, contiguous device arrays -> (cum int64 [nf] | None, W, shift, faces with weight);
    W == 0 (and no table) for a mesh without area.  Two host reads: the largest area, then the total with the count."""
    if nf == 0:
        return None, 0, 0, 0
    areas = _areas(vertices, faces, nv, nf)
    amax = float(areas.max().cpu())                          # a maximum is exact under any association
    if not (amax > 0.0 and math.isfinite(amax)):
        return None, 0, 0, 0
    shift = 32 - math.frexp(amax)[1]                         # the largest weight lands in [2^31, 2^32)
    weights = torch.empty(nf, device=vertices.device, dtype=torch.int64)
    L.check(L.load().cer_mesh_face_weights_i64(L.dev_ptr(areas, "areas", torch.float64), nf, shift, L.dev_ptr(weights, "weights", torch.int64),
                                               L.cur_stream()), "mesh_face_weights")
    cum = torch.cumsum(weights, 0)                           # integers: exact whatever the scan's shape
    total, count = (int(x) for x in torch.stack([cum[-1], (weights > 0).sum()]).cpu().tolist())
    return cum.contiguous(), total, shift, count


def _draw(vertices, faces, nv, nf, cum, seed, offset, words, n, normals, colors, uv):
    """the sample kernel on checked, contiguous device arrays -> (points, face, normals | None, colors | None, uv | None)"""
    dev = vertices.device
    points = torch.empty(n, 3, device=dev, dtype=torch.float32)
    face = torch.empty(n, device=dev, dtype=torch.int32)
    out_n = torch.empty(n, 3, device=dev, dtype=torch.float32) if normals else None
    out_c = None if colors is None else torch.empty(n, 3, device=dev, dtype=torch.uint8)
    out_uv = torch.empty(n, 2, device=dev, dtype=torch.float64) if uv else None
    if n:
        L.check(L.load().cer_mesh_sample_f32(L.dev_ptr(vertices, "vertices") if nv else None, nv, L.dev_ptr(faces, "faces", torch.int32), nf,
                                             L.dev_ptr(cum, "cum", torch.int64), seed, offset, L.dev_ptr(words, "words", torch.uint32), n,
                                             L.dev_ptr(colors, "colors", torch.uint8), L.dev_ptr(points, "points"),
                                             L.dev_ptr(face, "face", torch.int32), L.dev_ptr(out_uv, "uv", torch.float64),
                                             L.dev_ptr(out_n, "normals"), L.dev_ptr(out_c, "colors", torch.uint8), L.cur_stream()), "mesh_sample")
    return points, face, out_n, out_c, out_uv


def sample_mesh(vertices, faces, n=None, density=None, seed=0, offset=0, words=None, normals=False, colors=None, uv=False, info=None):
    """Points on the surface of any indexed triangle mesh, drawn with a density proportional to area: vertices float32 [nv,3] and faces int32
    [nf,3] on the device -> (points float32 [n,3], face int32 [n], normals float32 [n,3] | None, colors uint8 [n,3] | None, uv float64 [n,2]
    | None) on the device.  Exactly one of ``n`` (an int >= 0), ``density`` (samples per unit area, a positive finite number: n = ceil(area *
    density)) and ``words`` (uint32 [n,4] on the device: the caller's own four random words per sample - a low-discrepancy sequence, or a
    test's planted values) fixes the count.

    Every face gets the integer weight floor(area * 2^shift), the shift chosen so that the largest weight lies in [2^31, 2^32): the prefix
    sums and their total W are exact, a face smaller than 2^-32 of the largest has weight 0 and is never drawn, and the sampling density is
    uniform to 2^-31 of the largest face per face.  Faces that ``face_areas`` gives area 0 (an index out of range, a repeated index, a
    non-finite coordinate) are never drawn either.  Sample i has the global index k = ``offset`` + i and, without ``words``, the words
    Philox4x32-10(counter (k, 0, 0) in 32-bit halves, key ``seed``); x0 and x1 pick the face - t = floor((x0 * 2^32 + x1) * W / 2^64), the
    first face whose prefix sum exceeds t - and x2 and x3 the point: (a, b) mirrored through the square's centre when a + b >= 2^32, u = (a +
    0.5) / 2^32, v = (b + 0.5) / 2^32, w = 1 - u - v, p = float((w*A + u*B) + v*C).  Sample k is a pure function of (seed, k, mesh):
    ``n=100`` gives the first 100 rows of ``n=1000``, and ``offset=50, n=50`` rows 50 .. 99.  ``normals``: the face's unit normal;
    ``colors`` uint8 [nv,3]: the corners' colours mixed with (w, u, v) and rounded; ``uv``: (u, v).  ``info`` (a dict) gains "n", "area"
    (what the weights stand for: W / 2^shift), "faces_with_weight" and "shift".

    ValueError: bad arguments (before any device work); n > 0 on a mesh whose largest area is 0 or that has no face; more than 2^31 - 1
    samples from a density.  n == 0 returns empties.  RuntimeError: tensors that are not on the device.  The contract is cer_mvs.h's,
    "Mesh surface sampling"."""
    who = "sample_mesh"
    nv, nf = _sample_mesh_checks(vertices, faces, colors, who)
    if sum(x is not None for x in (n, density, words)) != 1:
        raise ValueError(f"{who}: exactly one of n, density and words expected")
    if n is not None:
        n = _sample_count(n, "n", who)
    if density is not None:
        density = _positive(density, "density", who)
    if words is not None:
        if not isinstance(words, torch.Tensor) or words.dtype != torch.uint32 or words.dim() != 2 or words.shape[1] != 4:
            raise ValueError(f"{who}: words uint32 [n, 4] expected")
        if words.shape[0] > SAMPLE_MAX:
            raise ValueError(f"{who}: {words.shape[0]} rows of words is beyond 2^31 - 1 samples")
        if words.device != vertices.device:
            raise ValueError(f"{who}: vertices and words must be on one device")
        n = int(words.shape[0])
    seed, offset = _word64(seed, "seed", who), _word64(offset, "offset", who)
    for name, flag in (("normals", normals), ("uv", uv)):
        if not isinstance(flag, bool):
            raise ValueError(f"{who}: {name} must be True or False")
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    vertices, faces = vertices.contiguous(), faces.contiguous()
    colors = None if colors is None else colors.contiguous()
    cum, W, shift, count = _sample_table(vertices, faces, nv, nf)
    area = math.ldexp(float(W), -shift)
    if density is not None:
        wanted = math.ceil(area * density)
        if wanted > SAMPLE_MAX:
            raise ValueError(f"{who}: density {density} on an area of {area} asks for {wanted} samples, beyond 2^31 - 1")
        n = int(wanted)
    if n and W == 0:
        raise ValueError(f"{who}: {n} samples asked of a mesh without area ({nf} faces)")
    if info is not None:
        info.update(n=n, area=area, faces_with_weight=count, shift=shift)
    return _draw(vertices, faces, nv, nf, cum, seed, offset, None if words is None else words.contiguous(), n, normals, colors, uv)


def sample_mesh_even(vertices, faces, spacing, oversample=8.0, seed=0, normals=False, colors=None, info=None):
    """Evenly spaced points on the surface of a mesh (Poisson-disk sampling by elimination): ``sample_mesh`` draws n0 = ceil(``oversample`` *
    area / ``spacing``^2) samples, ``cloud_eval.radius_thin(points, spacing, order="index")`` thins them - the samples' own order already is a
    random order - and the kept rows come back in index order with their attributes -> (points float32 [m,3], face int32 [m], normals
    float32 [m,3] | None, colors uint8 [m,3] | None) on the device.  ``radius_thin``'s two properties hold: kept points are pairwise farther
    apart than ``spacing``, and every drawn sample has a kept one within ``spacing``.  With the default ``oversample`` a disk of that radius
    around a surface point holds about 8 pi drawn samples, so the surface itself is covered to about the spacing as well.  ``info`` (a
    dict) gains "drawn", "kept", ``sample_mesh``'s "area", "faces_with_weight" and "shift", and ``radius_thin``'s "rounds", "compactions"
    and "n_finite".  ValueError: bad arguments; n0 beyond 2^31 - 1; a mesh without area (n0 == 0 returns empties).  The set is
    ``radius_thin``'s: unique, whatever the schedule of the device."""
    from .cloud_eval import radius_thin
    who = "sample_mesh_even"
    nv, nf = _sample_mesh_checks(vertices, faces, colors, who)
    spacing, oversample = _positive(spacing, "spacing", who), _positive(oversample, "oversample", who)
    if not float(np.float32(spacing)) > 0.0 or not math.isfinite(float(np.float32(spacing))):
        raise ValueError(f"{who}: spacing must be a positive finite float32")
    seed = _word64(seed, "seed", who)
    if not isinstance(normals, bool):
        raise ValueError(f"{who}: normals must be True or False")
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    vertices, faces = vertices.contiguous(), faces.contiguous()
    colors = None if colors is None else colors.contiguous()
    cum, W, shift, count = _sample_table(vertices, faces, nv, nf)
    area = math.ldexp(float(W), -shift)
    n0 = math.ceil(oversample * area / (spacing * spacing))
    if n0 > SAMPLE_MAX:
        raise ValueError(f"{who}: spacing {spacing} on an area of {area} asks for {n0} samples, beyond 2^31 - 1; take a larger spacing")
    n0 = int(n0)
    points, face, out_n, out_c, _ = _draw(vertices, faces, nv, nf, cum, seed, 0, None, n0, normals, colors, False)
    thin = {}
    kept = radius_thin(points, spacing, order="index", info=thin)
    if info is not None:
        info.update(drawn=n0, kept=int(kept.shape[0]), area=area, faces_with_weight=count, shift=shift, **thin)
    return tuple(None if a is None else a.index_select(0, kept) for a in (points, face, out_n, out_c))


EVALUATE_METHODS = ("samples", "exact")


def evaluate_mesh(vertices, faces, gt, spacing, max_dist=20.0, tau=None, seed=0, align=None, oversample=8.0, method="samples"):
    """A mesh against a ground-truth cloud, by way of evenly spaced samples of its surface - the route of the Tanks-and-Temples and Open3D
    evaluations: ``sample_mesh_even(vertices, faces, spacing, oversample, seed)``, then ``cloud_eval.accuracy_completeness(samples, gt,
    max_dist, align=align)`` and, with ``tau``, ``cloud_eval.fscore(samples, gt, tau, align=align)`` -> one dict: the keys of both, and
    "samples" (how many points stand for the mesh) and "spacing".  ``gt`` float32 [m,3] on the mesh's device.

    ``method="samples"`` (the default) measures distances to SAMPLES of the surface, not to the surface.  On the mesh's side (accuracy,
    precision) a sample is a surface point and its figure is exact for that point.  On the ground truth's side (completeness, recall) the
    nearest sample is farther than the surface is, by up to about the spacing: those figures carry an upward bias of that size - take a
    spacing well below ``tau`` and below the accuracy that is to be resolved, or take ``method="exact"``.

    ``method="exact"``: the mesh's side is the same - the samples against ``gt`` - and the ground truth's side is the exact distance of
    every ``gt`` point to the surface, ``MeshIndex(vertices, faces).nearest(gt, ...)``: no bias, whatever the spacing.  With ``tau`` the
    search runs again under the float32 cut-off that ``fscore`` forms; with ``align`` the vertices go through ``rigid_transform`` before
    they are indexed, as the samples do before they are measured.  The dict gains "method".

    What remains future work: a hierarchy for meshes whose triangles are far larger than any workable cell (``MeshIndex`` refuses a face of
    more than 4096 cells), and a signed distance."""
    from .cloud_eval import accuracy_completeness, cloud_distances, fscore, metrics_from_distances, rigid_transform
    who = "evaluate_mesh"
    if not isinstance(gt, torch.Tensor) or gt.dim() != 2 or gt.shape[1] != 3 or gt.dtype != torch.float32:
        raise ValueError(f"{who}: gt float32 [m, 3] expected")
    if not (isinstance(max_dist, (int, float)) and not isinstance(max_dist, bool) and math.isfinite(max_dist) and max_dist > 0):
        raise ValueError(f"{who}: max_dist must be a positive finite number")
    if tau is not None:
        tau = _positive(tau, "tau", who)
    if not isinstance(method, str) or method not in EVALUATE_METHODS:
        raise ValueError(f"{who}: method must be one of {list(EVALUATE_METHODS)}")
    if isinstance(vertices, torch.Tensor) and gt.device != vertices.device:
        raise ValueError(f"{who}: vertices and gt must be on one device")
    samples = sample_mesh_even(vertices, faces, spacing, oversample=oversample, seed=seed)[0]
    if method == "samples":
        out = accuracy_completeness(samples, gt, max_dist, align=align)
        if tau is not None:
            out.update(fscore(samples, gt, tau, align=align))
        out.update(samples=int(samples.shape[0]), spacing=float(spacing))
        return out
    pred, moved = (samples, vertices) if align is None else (rigid_transform(samples, align), rigid_transform(vertices, align))
    gt = gt.contiguous()
    index = MeshIndex(moved, faces, max_dist=max_dist)
    out = metrics_from_distances(cloud_distances(pred, gt, max_dist), index.nearest(gt, max_dist)[0], max_dist)
    if tau is not None:
        tau32 = float(np.float32(tau))
        cut = float(np.nextafter(np.float32(tau32), np.float32(np.inf))) if tau32 < float(tau) else tau32      # fscore's cut: a float32 not below tau
        m = metrics_from_distances(cloud_distances(pred, gt, cut), index.nearest(gt, cut)[0], cut, tau=tau)
        out.update({k: m[k] for k in ("precision", "recall", "fscore", "tau", "n_pred", "n_gt")})
    out.update(samples=int(samples.shape[0]), spacing=float(spacing), method=method)
    return out


# ---------------------------------------------------------------- exact point-to-mesh distance (csrc/mesh_dist.hip, C ABI 1240)
DIST_INFO_KEYS = ("cell", "pairs", "faces_indexed", "cells")
TRI_MAX_CELLS = 4096                                         # cer_mvs.h CER_TRI_MAX_CELLS: the cells one face may be entered in
TRI_MAX_RINGS = 4096                                         # mesh_dist.hip TRI_MAX_RINGS: ceil(max_dist / cell) beyond this is refused
TRI_KEY_SENTINEL = 2 ** 63 - 1
# The default cell is max(DEFAULT_CELL_EDGES * sqrt(area / faces with weight), max_dist / DEFAULT_CELL_RINGS): some twenty faces per cell and
# two cells per face on a mesh of even triangles, and never more than DEFAULT_CELL_RINGS rings of rows for a query that finds nothing.
# Results do not depend on it.  Measured by tools/bench_mesh_dist.py against 1, 2 and 8 edges (profiles/mesh_dist_bench.json
# "cell_sweep_edge_factors"): 4 wins on both query sets; the first guess was 2.
DEFAULT_CELL_EDGES = 4.0
DEFAULT_CELL_RINGS = 32


def _dist_reach(value, who):
    """``max_dist`` as the float32 the kernel takes: a number >= 0 (+inf is a number; the index refuses what its cell cannot reach)"""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{who}: max_dist must be a number >= 0")
    value = float(np.float32(value))
    if not value >= 0.0:
        raise ValueError(f"{who}: max_dist must be a number >= 0")
    return value


def _dist_queries(queries, vertices, who):
    if not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != 3 or queries.dtype != torch.float32:
        raise ValueError(f"{who}: queries float32 [m, 3] expected")
    if queries.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: fewer than 2^31 queries expected")
    if queries.device != vertices.device:
        raise ValueError(f"{who}: vertices and queries must be on one device")


class MeshIndex:
    """Sparse uniform grid over the faces of any indexed triangle mesh (vertices float32 [nv,3], faces int32 [nf,3] on the device) with cell
    edge ``cell``, built once: what ``cloud_eval.CloudIndex`` is for a cloud.  A face is entered in every cell of the box of cells that its
    corners span; faces that ``face_areas`` gives area 0 (an index out of range, a repeated index, a non-finite coordinate, a computed area
    of 0) are not indexed and are never anybody's nearest face.  The grid's origin is the per-axis minimum of the vertices that indexed
    faces use, promoted to fp64.  ``cell=None``: max(4 * sqrt(area / faces with weight), ``max_dist`` / 32) with ``sample_mesh``'s exact
    "area" and "faces_with_weight" (the second term only with ``max_dist``); results do not depend on the cell.  Attributes: ``cell``,
    ``pairs`` (entries of faces in cells), ``faces_indexed``, ``cells`` (occupied).

    ValueError: bad arguments (before any device work); a face that spans more than 4096 cells, a mesh that spans more than 2^20 cells
    along an axis, or 2^31 pairs and more - each names the cell and advises a larger one.  RuntimeError: tensors that are not on the device.
    The contract is cer_mvs.h's, "Mesh distance"."""

    def __init__(self, vertices, faces, cell=None, max_dist=None, _stages=None, _keep_pairs=False):
        who = "MeshIndex"

        def stage(name):                                     # tools/bench_mesh_dist.py: an event at the end of every stage of the build
            if _stages is not None:
                event = torch.cuda.Event(enable_timing=True)
                event.record()
                _stages.append((name, event))
        nv, nf = _sample_mesh_checks(vertices, faces, None, who)
        if cell is not None:
            cell = _positive(cell, "cell", who)
        if max_dist is not None:
            max_dist = _dist_reach(max_dist, who)
        if not vertices.is_cuda:
            raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
        vertices, faces = vertices.contiguous(), faces.contiguous()
        dev, lib = vertices.device, L.load()
        self.nv, self.nf = nv, nf
        self.origin = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
        self.pairs = self.faces_indexed = self.cells = 0
        self.records = self.pair_face = self.cell_keys = self.cell_start = None
        if cell is None:
            _, W, shift, count = _sample_table(vertices, faces, nv, nf)
            cell = DEFAULT_CELL_EDGES * math.sqrt(math.ldexp(float(W), -shift) / count) if W > 0 and count > 0 else 0.0
            if max_dist is not None and math.isfinite(max_dist):
                cell = max(cell, max_dist / DEFAULT_CELL_RINGS)
            if not (cell > 0.0 and math.isfinite(cell)):
                cell = 1.0                                   # a mesh without area: nothing will be indexed
        self.cell = cell
        if nf == 0:
            return
        stage("start")
        areas = _areas(vertices, faces, nv, nf)
        indexed = areas > 0.0
        used = faces[indexed].reshape(-1).long()             # (area > 0: the three indices are in range)
        self.faces_indexed = int(used.shape[0]) // 3         # (read 1: sizes the gather)
        if self.faces_indexed == 0:
            return
        lo = vertices.index_select(0, used).amin(0).double().cpu()                                      # (read 2: the origin travels as an argument)
        self.origin = (ctypes.c_double * 3)(*[float(v) for v in lo])
        pv, pf, pa = L.dev_ptr(vertices, "vertices"), L.dev_ptr(faces, "faces", torch.int32), L.dev_ptr(areas, "areas", torch.float64)
        stage("areas_origin")
        counts = torch.empty(nf, device=dev, dtype=torch.int64)
        flag = torch.empty(2, device=dev, dtype=torch.int32)
        rc = lib.cer_mesh_tri_cells_i64(pv, nv, pf, nf, pa, self.origin, cell, L.dev_ptr(counts, "cells", torch.int64),
                                        L.dev_ptr(flag, "flag", torch.int32), L.cur_stream())
        if rc == -2:
            beyond, large = (int(v) for v in flag.cpu())
            if large and not beyond:
                raise ValueError(f"{who}: a face spans more than {TRI_MAX_CELLS} cells of {cell}; use a larger cell")
            raise ValueError(f"{who}: the mesh spans more than 2^20 cells of {cell} along an axis; use a larger cell")
        L.check(rc, "mesh_tri_cells")
        cum = torch.cumsum(counts, 0).contiguous()           # integers: exact whatever the scan's shape
        npairs = int(cum[-1])                                # (read 3: sizes the pair list)
        if npairs >= 2 ** 31:
            raise ValueError(f"{who}: {npairs} entries of faces in cells of {cell} is beyond 2^31 - 1; use a larger cell")
        stage("cells_scan")
        keys = torch.full((npairs,), TRI_KEY_SENTINEL, device=dev, dtype=torch.int64)
        ids = torch.full((npairs,), -1, device=dev, dtype=torch.int32)
        L.check(lib.cer_mesh_tri_pairs_i64(pv, nv, pf, nf, pa, self.origin, cell, L.dev_ptr(cum, "cum", torch.int64), npairs,
                                           L.dev_ptr(keys, "keys", torch.int64), L.dev_ptr(ids, "ids", torch.int32), L.cur_stream()), "mesh_tri_pairs")
        stage("pairs")
        self._pairs_unsorted = (keys, ids) if _keep_pairs else None              # (what the tests hold to the restatement)
        keys, perm = torch.sort(keys, stable=True)           # faces stay ascending inside a cell
        self.pair_face = ids.index_select(0, perm).contiguous()
        del perm, ids
        stage("sort")
        P = int(lib.cer_grid_partials(npairs))
        partials, offsets, totals = L.compaction_buffers(P, dev, extra=1)
        pk = L.dev_ptr(keys, "keys", torch.int64)
        L.check(lib.cer_grid_cells_count_i64(pk, npairs, L.dev_ptr(partials, "partials", torch.int32), L.dev_ptr(offsets, "offsets", torch.int64),
                                             L.dev_ptr(totals, "totals", torch.int64), L.cur_stream()), "grid_cells_count")
        self.cells, self.pairs = (int(v) for v in totals.cpu())                                          # (read 4: sizes the cell table)
        self.cell_keys = torch.empty(self.cells, device=dev, dtype=torch.int64)
        self.cell_start = torch.empty(self.cells + 1, device=dev, dtype=torch.int64)
        L.check(lib.cer_grid_cells_i64(pk, npairs, L.dev_ptr(offsets, "offsets", torch.int64), self.cells,
                                       L.dev_ptr(self.cell_keys, "cell_keys", torch.int64), L.dev_ptr(self.cell_start, "cell_start", torch.int64),
                                       L.cur_stream()), "grid_cells")
        stage("cell_table")
        self.records = torch.empty(nf, 12, device=dev, dtype=torch.int32)
        L.check(lib.cer_mesh_tri_pack_f32(pv, nv, pf, nf, L.dev_ptr(self.records, "records", torch.int32), L.cur_stream()), "mesh_tri_pack")
        stage("pack")

    def info(self):
        return dict(cell=self.cell, pairs=self.pairs, faces_indexed=self.faces_indexed, cells=self.cells)

    def _walk_order(self, queries, m):                       # CloudIndex._walk_order: the queries' positions in the order of their own cell keys
        qkeys = torch.empty(m, device=queries.device, dtype=torch.int64)
        L.check(L.load().cer_grid_keys_f32(L.dev_ptr(queries, "queries"), m, self.origin, self.cell, 1, L.dev_ptr(qkeys, "keys", torch.int64), None,
                                           L.cur_stream()), "grid_keys")
        return torch.sort(qkeys, stable=True).indices

    def nearest(self, queries, max_dist, closest=False, sort_queries=True):
        """-> (dist float32 [m], face int32 [m]) and, with ``closest``, the closest point float32 [m,3], in the queries' order: the indexed
        face with the smallest (dist2, face index) among those with dist2 <= double(max_dist)^2, dist2 in fp64 as cer_mvs.h's section
        "Mesh distance" pins it; dist = float32(sqrt(dist2)); (inf, -1, NaN) where there is none or the query is not finite.
        ``sort_queries``: walk the queries in the order of their own cells (faster; the result is the same)."""
        who = "MeshIndex.nearest"
        max_dist = _dist_reach(max_dist, who)
        for name, flag in (("closest", closest), ("sort_queries", sort_queries)):
            if not isinstance(flag, bool):
                raise ValueError(f"{who}: {name} must be True or False")
        if not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != 3 or queries.dtype != torch.float32:
            raise ValueError(f"{who}: queries float32 [m, 3] expected")
        if queries.shape[0] >= 2 ** 31:
            raise ValueError(f"{who}: fewer than 2^31 queries expected")
        if not queries.is_cuda:
            raise RuntimeError(f"{who}: queries must be a CUDA tensor (no CPU fallback)")
        if max_dist / self.cell > TRI_MAX_RINGS:                                  # (ceil(x) > 4096 iff x > 4096; +inf lands here)
            raise ValueError(f"{who}: max_dist {max_dist} is more than {TRI_MAX_RINGS} cells of {self.cell}; index the mesh with a larger cell")
        queries = queries.contiguous()
        m, dev = int(queries.shape[0]), queries.device
        empty = m == 0 or self.pairs == 0 or self.cells == 0                     # (the entry point launches nothing for an empty side)
        make = (lambda shape, dt, fill: torch.full(shape, fill, device=dev, dtype=dt)) if empty else \
            (lambda shape, dt, fill: torch.empty(shape, device=dev, dtype=dt))
        dist, face = make((m,), torch.float32, float("inf")), make((m,), torch.int32, -1)
        near = make((m, 3), torch.float32, float("nan")) if closest else None
        if not empty:
            qorder = self._walk_order(queries, m) if sort_queries else None
            L.check(L.load().cer_mesh_tri_nearest_f32(
                L.dev_ptr(self.records, "records", torch.int32), self.nf, L.dev_ptr(self.pair_face, "pair_face", torch.int32), self.pairs,
                L.dev_ptr(self.cell_keys, "cell_keys", torch.int64), L.dev_ptr(self.cell_start, "cell_start", torch.int64), self.cells, self.origin,
                self.cell, L.dev_ptr(queries, "queries"), L.dev_ptr(qorder, "qorder", torch.int64), m, max_dist,
                L.dev_ptr(face, "face", torch.int32), L.dev_ptr(dist, "dist"), L.dev_ptr(near, "closest"), L.cur_stream()), "mesh_tri_nearest")
        return (dist, face, near) if closest else (dist, face)


def mesh_distances(vertices, faces, queries, max_dist, cell=None, info=None):
    """float32 [m]: the distance from every query point (float32 [m,3] on the mesh's device) to the surface of the mesh within ``max_dist``
    (inf where there is none) - ``MeshIndex(vertices, faces, cell, max_dist).nearest(queries, max_dist)[0]``.  ``cell`` defaults as
    ``MeshIndex`` says; ``info`` (a dict) gains "cell", "pairs", "faces_indexed" and "cells".  ValueError: bad arguments (before any device
    work), and what ``MeshIndex`` refuses.  RuntimeError: tensors that are not on the device.  The contract is cer_mvs.h's,
    "Mesh distance"."""
    who = "mesh_distances"
    _sample_mesh_checks(vertices, faces, None, who)
    _dist_queries(queries, vertices, who)
    max_dist = _dist_reach(max_dist, who)
    if cell is not None:
        cell = _positive(cell, "cell", who)
    if info is not None and not isinstance(info, dict):
        raise ValueError(f"{who}: info must be a dictionary or None")
    if not vertices.is_cuda:
        raise RuntimeError(f"{who}: vertices must be a CUDA tensor (no CPU fallback)")
    index = MeshIndex(vertices, faces, cell, max_dist)
    if info is not None:
        info.update(index.info())
    return index.nearest(queries, max_dist)[0]


def _sample_option(value):
    """the "sample" option, checked -> (kind, amount, seed), kind one of "n", "density", "spacing\""""
    text = ("mesh: sample must be an integer n >= 1 or a dictionary with \"n\", \"density\" or \"spacing\" (exactly one of them) and "
            "optionally \"seed\"")
    if not isinstance(value, dict):
        if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= SAMPLE_MAX:
            raise ValueError(text)
        return "n", value, 0
    kinds = [k for k in ("n", "density", "spacing") if k in value]
    if set(value) - set(SAMPLE_OPTION_KEYS) or len(kinds) != 1:
        raise ValueError(text)
    kind, amount = kinds[0], value[kinds[0]]
    if kind == "n":
        if isinstance(amount, bool) or not isinstance(amount, int) or not 1 <= amount <= SAMPLE_MAX:
            raise ValueError("mesh: sample: n must be an integer in 1 .. 2^31 - 1")
    else:
        amount = _positive(amount, f"sample: {kind}", "mesh")
    seed = value.get("seed", 0)
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError("mesh: sample: seed must be an integer in 0 .. 2^64 - 1")
    return kind, amount, seed


MESH_OPTION_KEYS = ("voxel", "resolution", "trunc", "min_weight", "margin", "colors", "normals", "min_component", "keep_largest", "simplify",
                    "smooth", "topology", "fill_holes", "sample")


def mesh_options(mesh):
    """``reconstruct_scan``'s ``mesh`` argument, checked: True or a dict with keys of MESH_OPTION_KEYS -> a dict.  "colors": True or
    {"tol": a positive finite number} (default: the mesh's trunc); "normals": True; "min_component" (``remove_small_components``'s
    ``min_faces``) and "keep_largest": an int >= 1 each; "simplify": a positive finite number k - ``simplify_vertex_clustering`` with a cell
    of k mesh voxels - or {"voxels": k | "cell": world units, "representative": "quadric" | "mean", "regularisation": a positive finite
    number}, "voxels" and "cell" exclusive; "smooth": an int n >= 1 - ``smooth_mesh`` with n Taubin iterations and its defaults - or
    {"iterations": n, "method", "lam", "mu", "boundary"} with ``smooth_mesh``'s values; "topology": True; "fill_holes": an int n >= 3 -
    ``fill_holes`` with ``max_edges`` = n; "sample": an int n >= 1 - ``sample_mesh`` with n samples and seed 0 - or {"n": samples |
    "density": samples per unit area | "spacing": world units (``sample_mesh_even``), "seed": an int}, exactly one of the three."""
    if mesh is True:
        return {}
    if not isinstance(mesh, dict):
        raise ValueError("mesh: True or a dictionary of options expected")
    extra = sorted(set(mesh) - set(MESH_OPTION_KEYS))
    if extra:
        raise ValueError(f"mesh: unknown option(s) {extra}; known: {list(MESH_OPTION_KEYS)}")
    if "voxel" in mesh and "resolution" in mesh:
        raise ValueError("mesh: give voxel or resolution, not both")
    if "colors" in mesh and mesh["colors"] is not True:
        col = mesh["colors"]
        if not isinstance(col, dict) or set(col) - {"tol"}:
            raise ValueError("mesh: colors must be True or {\"tol\": a positive finite number}")
        if "tol" in col and not (isinstance(col["tol"], (int, float)) and not isinstance(col["tol"], bool) and math.isfinite(col["tol"]) and col["tol"] > 0):
            raise ValueError("mesh: colors: tol must be a positive finite number")
    if "normals" in mesh and mesh["normals"] is not True:
        raise ValueError("mesh: normals must be True")
    for key in ("min_component", "keep_largest"):
        if key in mesh and _count_option(mesh[key], key, "mesh") is None:
            raise ValueError(f"mesh: {key} must be an integer >= 1")
    if "simplify" in mesh:
        _simplify_option(mesh["simplify"])
    if "smooth" in mesh:
        _smooth_option(mesh["smooth"])
    if "topology" in mesh and mesh["topology"] is not True:
        raise ValueError("mesh: topology must be True")
    if "fill_holes" in mesh:
        _fill_option(mesh["fill_holes"])
    if "sample" in mesh:
        _sample_option(mesh["sample"])
    return dict(mesh)


def _simplify_option(value):
    """the "simplify" option, checked -> (voxels | None, cell | None, representative, regularisation)"""
    if not isinstance(value, dict):
        return _positive(value, "simplify", "mesh"), None, "quadric", 1e-3
    if set(value) - set(SIMPLIFY_KEYS) or ("voxels" in value) == ("cell" in value):
        raise ValueError(f"mesh: simplify must be a positive finite number or a dictionary with \"voxels\" or \"cell\" (one of them) and keys of {list(SIMPLIFY_KEYS)}")
    voxels = _positive(value["voxels"], "simplify: voxels", "mesh") if "voxels" in value else None
    cell = _positive(value["cell"], "simplify: cell", "mesh") if "cell" in value else None
    return (voxels, cell, _representative(value.get("representative", "quadric"), "mesh: simplify"),
            _positive(value.get("regularisation", 1e-3), "simplify: regularisation", "mesh"))


def mesh_of_scan(xyz, est, masks, Ks, Es, refs, options, colors=None):
    """``reconstruct_scan``'s mesh step: the grid around the fused cloud, then ``mesh_from_depth_maps`` over the emitted views -> (vertices,
    faces, info, attributes).  With the options "colors" / "normals": ``vertex_colors`` over the same views from the ``colors`` planes
    [N,3,h,w] (tol: the option's, or the mesh's trunc) / ``vertex_normals``; ``attributes`` then holds "mesh_colors" / "mesh_normals" (device
    tensors) and ``info`` gains "coloured", the number of vertices that a view sees.  With "min_component" / "keep_largest":
    ``remove_small_components`` right after the extraction, before the attributes; ``info``'s "nv" and "nf" then describe the returned mesh
    and it gains "extracted": (nv, nf) of the extraction, and the removal's figures.  With "simplify": ``simplify_vertex_clustering`` after
    the removal and before the attributes; ``info``'s "nv" and "nf" describe the returned mesh and it gains "simplified_from": (nv, nf) before,
    and the simplification's figures.  With "smooth": ``smooth_mesh`` after the removal and before "simplify" and the attributes; ``info``
    gains "smoothed", ``smooth_mesh``'s info.  With "topology": ``info`` gains "topology", ``mesh_topology`` of the returned mesh.  With
    "fill_holes": ``fill_holes`` after the removal - an island's rim is a loop too - and before "smooth", "simplify" and the attributes, so
    that fewer vertices are frozen on a boundary and colours and normals belong to the returned mesh; ``info``'s "nv" and "nf" describe the
    returned mesh and it gains "filled", ``fill_holes``' info.  With "sample": last of all, on the returned mesh, ``sample_mesh`` ("n",
    "density") or ``sample_mesh_even`` ("spacing"); ``attributes`` gains "mesh_samples" (float32 [n,3]) and "mesh_sample_faces" (int32 [n])
    and, when colours were asked for, "mesh_sample_colors" (uint8 [n,3], mixed from the vertex colours); ``info`` gains "sampled", the
    call's info."""
    opt = dict(options)
    min_weight = opt.pop("min_weight", 1)
    trunc = opt.pop("trunc", None)
    want_colors, want_normals = opt.pop("colors", None), opt.pop("normals", None)
    min_component, keep_largest = opt.pop("min_component", None), opt.pop("keep_largest", None)
    simplify = opt.pop("simplify", None)
    smooth, want_topology = opt.pop("smooth", None), opt.pop("topology", None)
    fill, sample = opt.pop("fill_holes", None), opt.pop("sample", None)
    grid = grid_for(xyz, trunc=trunc, **opt)
    info, attributes = {}, {}
    v, f = mesh_from_depth_maps(est, masks, Ks, Es, grid, trunc=trunc, views=refs, min_weight=min_weight, info=info)
    if min_component is not None or keep_largest is not None:            # before the attributes: they are computed on what is returned
        info["extracted"] = (info["nv"], info["nf"])
        v, f, _, _, _ = remove_small_components(v, f, min_faces=min_component, keep_largest=keep_largest, info=info)
        info.update(nv=int(v.shape[0]), nf=int(f.shape[0]))
    if fill is not None:                                                 # after the removal: an island's rim is a loop too
        info["filled"] = {}
        v, f, _, _ = fill_holes(v, f, _fill_option(fill), info=info["filled"])
        info.update(nv=int(v.shape[0]), nf=int(f.shape[0]))
    if smooth is not None:                                               # denoise first, then reduce
        iterations, method, lam, mu, boundary = _smooth_option(smooth)
        info["smoothed"] = {}
        v = smooth_mesh(v, f, iterations, method=method, lam=lam, mu=mu, boundary=boundary, info=info["smoothed"])
    if simplify is not None:                                             # after the removal, before the attributes
        voxels, cell, representative, regularisation = _simplify_option(simplify)
        info["simplified_from"] = (info["nv"], info["nf"])
        v, f, _, _ = simplify_vertex_clustering(v, f, voxels * info["grid"].voxel if cell is None else cell, representative=representative,
                                                regularisation=regularisation, info=info)
        info.update(nv=int(v.shape[0]), nf=int(f.shape[0]))
    if want_colors is not None:
        if colors is None:
            raise ValueError("mesh: colors asked for without colour planes")
        tol = info["trunc"] if want_colors is True else float(want_colors.get("tol", info["trunc"]))
        attributes["mesh_colors"], seen = vertex_colors(v, est, masks, colors, Ks, Es, tol, views=refs)
        info["coloured"] = int((seen > 0).sum())
    if want_normals is not None:
        attributes["mesh_normals"] = vertex_normals(v, f)
    if want_topology is not None:
        info["topology"] = mesh_topology(f, int(v.shape[0]))
    if sample is not None:                                               # last: the samples belong to the returned mesh and its colours
        kind, amount, seed = _sample_option(sample)
        info["sampled"] = {}
        vertex_cols = attributes.get("mesh_colors")
        if kind == "spacing":
            points, face, _, cols = sample_mesh_even(v, f, amount, seed=seed, colors=vertex_cols, info=info["sampled"])
        else:
            points, face, _, cols, _ = sample_mesh(v, f, seed=seed, colors=vertex_cols, info=info["sampled"], **{kind: amount})
        attributes["mesh_samples"], attributes["mesh_sample_faces"] = points, face
        if cols is not None:
            attributes["mesh_sample_colors"] = cols
    return v, f, info, attributes


_PLY_NORMALS = "property float nx\nproperty float ny\nproperty float nz\n"
_PLY_COLORS = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _ply_head(nv, nf, normals, colors):
    """the header of one of the four forms: x y z [nx ny nz] [red green blue] per vertex, ``fusion.write_ply``'s order"""
    return ("ply\nformat binary_little_endian 1.0\n" f"element vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n"
            + (_PLY_NORMALS if normals else "") + (_PLY_COLORS if colors else "")
            + f"element face {nf}\nproperty list uchar int vertex_indices\nend_header\n")


def _ply_vertex(normals, colors):
    return np.dtype([("p", "<f4", (3,))] + ([("n", "<f4", (3,))] if normals else []) + ([("c", "u1", (3,))] if colors else []))


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_mesh_ply(path, vertices, faces, normals=None, colors=None):
    """Binary little-endian PLY: float x, y, z per vertex, then float nx, ny, nz with ``normals`` ([nv, 3]) and uchar red, green, blue with
    ``colors`` (uint8 [nv, 3]), and per face a uchar count of 3 and three int32 ``vertex_indices``."""
    v, f = _host(vertices), _host(faces)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("write_mesh_ply: vertices [nv, 3] and faces [nf, 3] expected")
    if f.size and (not np.issubdtype(f.dtype, np.integer) or f.min() < 0 or f.max() >= len(v)):
        raise ValueError("write_mesh_ply: faces must hold integer indices into vertices")
    nrm, col = (None if a is None else _host(a) for a in (normals, colors))
    if nrm is not None and nrm.shape != v.shape:
        raise ValueError(f"write_mesh_ply: normals [{len(v)}, 3] expected")
    if col is not None and (col.shape != v.shape or col.dtype != np.uint8):
        raise ValueError(f"write_mesh_ply: colors uint8 [{len(v)}, 3] expected")
    rec = np.empty(len(f), dtype=_PLY_FACE)
    rec["n"], rec["v"] = 3, f
    ver = np.empty(len(v), dtype=_ply_vertex(nrm is not None, col is not None))
    ver["p"] = v
    if nrm is not None:
        ver["n"] = nrm
    if col is not None:
        ver["c"] = col
    with open(path, "wb") as fh:
        fh.write(_ply_head(len(v), len(f), nrm is not None, col is not None).encode("ascii"))
        fh.write(ver.tobytes())
        fh.write(rec.tobytes())


def read_mesh_ply(path, attributes=False):
    """What ``write_mesh_ply`` wrote, in any of its four forms: (vertices float32 [nv, 3], faces int32 [nf, 3]), or with ``attributes``
    (vertices, faces, normals float32 [nv, 3] | None, colors uint8 [nv, 3] | None)"""
    raw = open(path, "rb").read()
    head, sep, body = raw.partition(b"end_header\n")
    text = head.decode("ascii", "replace")
    lines = text.split("\n")
    try:
        nv = int(next(ln for ln in lines if ln.startswith("element vertex ")).split()[2])
        nf = int(next(ln for ln in lines if ln.startswith("element face ")).split()[2])
    except StopIteration:
        nv = nf = -1
    has_n, has_c = "property float nx" in lines, "property uchar red" in lines
    if not sep or text + "end_header\n" != _ply_head(nv, nf, has_n, has_c):
        raise ValueError(f"{path}: not a mesh PLY of write_mesh_ply's form")
    vdt = _ply_vertex(has_n, has_c)
    if len(body) != nv * vdt.itemsize + nf * _PLY_FACE.itemsize:
        raise ValueError(f"{path}: {len(body)} bytes of data for {nv} vertices and {nf} faces")
    ver = np.frombuffer(body, dtype=vdt, count=nv)
    v = ver["p"].astype(np.float32)
    rec = np.frombuffer(body, dtype=_PLY_FACE, offset=nv * vdt.itemsize, count=nf)
    if nf and not (rec["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    f = rec["v"].astype(np.int32)
    if not attributes:
        return v, f
    return v, f, (ver["n"].astype(np.float32) if has_n else None), (ver["c"].copy() if has_c else None)
