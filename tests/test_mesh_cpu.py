"""Surface mesh on the device (csrc/mesh.hip, cer-mvs_amd/mesh.py), the parts that need no GPU: the entry points of ABI 1170 and
their argument checks in the documented order, the Python layer's ValueErrors and the PLY round trip, and the numpy restatement of
tests/mesh_reference.py - which the GPU tests hold the device to bit for bit - held to the properties of a correct mesher on the analytic
sphere cases, with every case of the tetrahedron table shown to occur in the volume the bit-equality test uses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_reference as M
from conftest import REPO

BIG = 1 << 31
NAN, INF = float("nan"), float("inf")
NAMES = ("cer_mesh_partials", "cer_tsdf_integrate_f32", "cer_mesh_cells_u16", "cer_mesh_count", "cer_mesh_emit_f32")


# ---------------------------------------------------------------- ABI
def test_mesh_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import mesh as ME
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    names = L.exported_symbols()
    for n in NAMES:
        assert n in names and re.search(r"\b(int|long) %s\(" % n, hdr), n
        if n != "cer_mesh_partials":
            assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P             # a stream: the last argument
    assert L.ABI_VERSION >= 1170 and "ABI 1170" in hdr
    lib = L.load()
    assert lib.cer_abi_version() == L.ABI_VERSION
    assert f"#define CER_MESH_TILE {ME.MESH_TILE}\n" in hdr and ME.CAM_DOUBLES == 24
    mk = open(os.path.join(REPO, "cer-mvs_amd", "csrc", "Makefile")).read()
    assert "mesh.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    assert re.search(r"^mesh\.o: CXXFLAGS \+= -fno-slp-vectorize$", mk, re.M) and "-ffast-math" not in mk
    tile = ME.MESH_TILE

    def blocks(v):
        return (v + tile - 1) // tile
    for dims, want in (((0, 5, 5), 0), ((1, 1, 1), 0), ((7, 1, 3), 0), ((2, 2, 2), blocks(64) + blocks(12)), ((65, 64, 64), blocks(266240 * 8) + blocks(64 * 63 * 63 * 12)),
                       ((-1, 2, 2), -1), ((2, 2, -5), -1), ((1 << 16, 1 << 15, 1), -2), ((1291, 1291, 1291), -2), ((2048, 1048575, 1), -2), ((2048, 1048574, 1), 0),
                       ((1290, 1290, 1290), blocks(1290 ** 3 * 8) + blocks(1289 ** 3 * 12))):
        assert lib.cer_mesh_partials(*dims) == want, dims


def test_mesh_entry_points_refuse_bad_arguments_in_the_documented_order():
    """every check runs before any launch (the pointers are fake: a launch would fault).  The order: (1) a negative size CER_EINVAL (-1); (2)
    too large CER_ESHAPE (-2); (3) origin null or non-finite, voxel / trunc not positive and finite CER_EINVAL; (4) nothing to do CER_OK; (5)
    null pointers CER_EINVAL - each case breaks one rule and every later one, and gets the earlier rule's answer."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    no_d = ctypes.POINTER(ctypes.c_double)()
    huge = (1 << 11, 1 << 10, 1 << 10)                                            # 2^31 nodes

    def bad_origin(i, v):
        p = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
        p[i] = v
        return p

    def integ(dep=fake, msk=fake, cams=fake, N=3, h=5, w=7, views=fake, nv=3, origin=org, voxel=1.0, dims=(4, 3, 2), trunc=2.0, tsdf=fake, wgt=fake):
        return lib.cer_tsdf_integrate_f32(dep, msk, cams, N, h, w, views, nv, origin, voxel, *dims, trunc, tsdf, wgt, null)
    inulls = dict(dep=null, cams=null, views=null, tsdf=null, wgt=null)
    for kw in (dict(N=-1), dict(h=-1), dict(w=-2), dict(nv=-1), dict(dims=(-1, 3, 2)), dict(dims=(4, 3, -2))):                    # 1
        assert integ(**kw) == -1 and integ(**kw, origin=no_d, **inulls) == -1, kw
    assert integ(dims=(-1, 1 << 20, 1 << 20)) == -1                               # (negative before too large)
    assert integ(dims=huge) == -2 and integ(dims=huge, origin=no_d, voxel=NAN, **inulls) == -2                                    # 2
    assert integ(h=1 << 16, w=1 << 16) == -2 and integ(h=1 << 16, w=1 << 16, trunc=-1.0) == -2
    assert integ(origin=no_d) == -1                                               # 3
    for i in range(3):
        for v in (NAN, INF, -INF):
            assert integ(origin=bad_origin(i, v)) == -1 and integ(origin=bad_origin(i, v), nv=0) == -1
    for v in (0.0, -1.0, NAN, INF):
        assert integ(voxel=v) == -1 and integ(trunc=v) == -1 and integ(voxel=v, dims=(0, 3, 2)) == -1 and integ(trunc=v, nv=0) == -1
    assert integ(nv=0) == 0 and integ(nv=0, **inulls) == 0 and integ(dims=(4, 0, 2), **inulls) == 0                               # 4
    assert integ(nv=0, N=0, h=0, w=0) == 0
    for name in inulls:                                                           # 5
        assert integ(**{name: null}) == -1, name
    assert integ(N=0) == -1 and integ(h=0) == -1 and integ(w=0) == -1              # (views listed, nothing to look at)
    assert integ(msk=null, **inulls) == -1

    def cells(tsdf=fake, wgt=fake, dims=(4, 3, 2), mw=1, out=fake):
        return lib.cer_mesh_cells_u16(tsdf, wgt, *dims, mw, out, null)

    def count(cel=fake, dims=(4, 3, 2), part=fake, off=fake, tot=fake):
        return lib.cer_mesh_count(cel, *dims, part, off, tot, null)
    cn, kn = dict(tsdf=null, wgt=null, out=null), dict(cel=null, part=null, off=null, tot=null)
    for call, nulls in ((cells, cn), (count, kn)):
        assert call(dims=(4, -3, 2)) == -1 and call(dims=(4, -3, 2), **nulls) == -1
        assert call(dims=huge) == -2 and call(dims=huge, **nulls) == -2
        for dims in ((0, 3, 2), (4, 1, 2), (1, 1, 1), (4, 3, 1)):                 # no node, or an axis of 1: no cell
            assert call(dims=dims) == 0 and call(dims=dims, **nulls) == 0
        for name in nulls:
            assert call(**{name: null}) == -1, name

    def emit(tsdf=fake, cel=fake, origin=org, voxel=1.0, dims=(4, 3, 2), off=fake, nv=5, nf=4, vcap=5, fcap=4, vmap=fake, ver=fake, fac=fake):
        return lib.cer_mesh_emit_f32(tsdf, cel, origin, voxel, *dims, off, nv, nf, vcap, fcap, vmap, ver, fac, null)
    en = dict(tsdf=null, cel=null, off=null, vmap=null, ver=null, fac=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(vcap=-1), dict(fcap=-1), dict(dims=(4, 3, -2))):
        assert emit(**kw) == -1 and emit(**kw, origin=no_d, **en) == -1, kw
    assert emit(dims=huge) == -2 and emit(nv=BIG) == -2 and emit(nf=BIG, origin=no_d, **en) == -2
    assert emit(origin=no_d) == -1 and emit(origin=bad_origin(2, NAN)) == -1 and emit(voxel=0.0, dims=(4, 1, 2)) == -1 and emit(voxel=INF, nv=0, nf=0) == -1
    for kw in (dict(dims=(0, 3, 2)), dict(dims=(4, 1, 2)), dict(nv=0, nf=0), dict(vcap=0, fcap=0)):
        assert emit(**kw) == 0 and emit(**kw, **en) == 0, kw
    for name in en:
        assert emit(**{name: null}) == -1, name


# ---------------------------------------------------------------- the Python layer
def test_python_layer_refuses_bad_arguments_without_a_device():
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    dep, msk = torch.zeros(3, 5, 7), torch.ones(3, 5, 7, dtype=torch.uint8)
    Ks, Es = torch.eye(3).repeat(3, 1, 1), torch.eye(4).repeat(3, 1, 1)
    grid = ME.Grid((0.0, 0.0, 0.0), 1.0, (4, 3, 2))
    with pytest.raises(ValueError, match="depths"):
        ME.tsdf_volume(dep.double(), msk, Ks, Es, grid, 2.0)
    with pytest.raises(ValueError, match="depths"):
        ME.tsdf_volume(dep[0], msk, Ks, Es, grid, 2.0)
    with pytest.raises(ValueError, match="masks"):
        ME.tsdf_volume(dep, msk.bool(), Ks, Es, grid, 2.0)
    with pytest.raises(ValueError, match="masks"):
        ME.tsdf_volume(dep, msk[:2], Ks, Es, grid, 2.0)
    with pytest.raises(ValueError, match="cameras|Ks"):
        ME.tsdf_volume(dep, msk, Ks[:2], Es[:2], grid, 2.0)
    with pytest.raises(ValueError, match="Ks"):
        ME.forward_cams(Ks, Es[:, :3])
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="trunc"):
            ME.tsdf_volume(dep, msk, Ks, Es, grid, bad)
        with pytest.raises(ValueError, match="voxel"):
            ME.tsdf_volume(dep, msk, Ks, Es, ME.Grid((0.0, 0.0, 0.0), bad, (4, 3, 2)), 2.0)
    with pytest.raises(ValueError, match="origin"):
        ME.tsdf_volume(dep, msk, Ks, Es, ME.Grid((0.0, NAN, 0.0), 1.0, (4, 3, 2)), 2.0)
    with pytest.raises(ValueError, match="dims"):
        ME.tsdf_volume(dep, msk, Ks, Es, ME.Grid((0.0, 0.0, 0.0), 1.0, (4, -3, 2)), 2.0)
    with pytest.raises(ValueError, match="2\\^31"):
        ME.tsdf_volume(dep, msk, Ks, Es, ME.Grid((0.0, 0.0, 0.0), 1.0, (2048, 1024, 1024)), 2.0)
    with pytest.raises(ValueError, match="grid"):
        ME.tsdf_volume(dep, msk, Ks, Es, ((0.0, 0.0), 1.0, (4, 3, 2)), 2.0)
    for views in ([3], [-1], [0, 1, 7]):
        with pytest.raises(ValueError, match="views"):
            ME.tsdf_volume(dep, msk, Ks, Es, grid, 2.0, views=views)
    with pytest.raises(RuntimeError, match="CUDA"):          # good arguments: the host tensors are what is refused
        ME.tsdf_volume(dep, msk, Ks, Es, grid, 2.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        ME.mesh_from_depth_maps(dep, None, Ks, Es, grid)
    ts, wg = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="tsdf"):
        ME.extract_mesh(ts.double(), wg, grid)
    with pytest.raises(ValueError, match="tsdf"):
        ME.extract_mesh(ts.reshape(4, 3, 2), wg, grid)
    with pytest.raises(ValueError, match="weight"):
        ME.extract_mesh(ts, wg.long(), grid)
    with pytest.raises(RuntimeError, match="CUDA"):
        ME.extract_mesh(ts, wg, grid)
    # mesh options of reconstruct_scan: refused before a model or a session is built
    for bad in ({"colour": True}, {"voxel": 1.0, "resolution": 64}, "yes", 3):
        with pytest.raises(ValueError, match="mesh"):
            reconstruct_scan(None, [0], [0], [0], ["a"], [[0]], [1.0], None, write=False, mesh=bad)
    assert ME.mesh_options(True) == {} and ME.mesh_options({"resolution": 48, "trunc": 0.1}) == {"resolution": 48, "trunc": 0.1}


def test_grid_for_snaps_the_origin_and_covers_the_cloud():
    from cer_mvs_amd import mesh as ME
    pts = torch.tensor([[0.31, -1.2, 5.0], [2.9, 0.4, 5.5], [NAN, 0.0, 0.0], [1.0, 0.0, 5.2]])
    g = ME.grid_for(pts, voxel=0.25, margin=0.5)
    assert isinstance(g, ME.Grid) and g.voxel == 0.25
    o, d = np.array(g.origin), np.array(g.dims)
    assert np.array_equal(o / 0.25, np.round(o / 0.25))                            # a multiple of the voxel
    lo, hi = np.array([0.31, -1.2, 5.0]) - 0.5, np.array([2.9, 0.4, 5.5]) + 0.5
    assert (o <= lo).all() and (o > lo - 0.25).all() and (o + (d - 1) * 0.25 >= hi).all() and (o + (d - 2) * 0.25 < hi).all()
    g2 = ME.grid_for(pts, resolution=10)                                           # voxel = longest side / 10, margin = trunc = 3 voxels
    assert abs(g2.voxel - 0.259) < 1e-6 and max(g2.dims) in (17, 18)
    assert ME.grid_for(pts, voxel=0.25, trunc=0.5) == g                            # margin defaults to trunc
    with pytest.raises(ValueError, match="max_nodes"):
        ME.grid_for(pts, voxel=0.01, max_nodes=10 ** 6)
    with pytest.raises(ValueError, match="finite"):
        ME.grid_for(torch.full((4, 3), NAN))
    with pytest.raises(ValueError, match="points"):
        ME.grid_for(torch.zeros(4, 2))
    with pytest.raises(ValueError, match="voxel"):
        ME.grid_for(pts, voxel=-1.0)
    with pytest.raises(ValueError, match="resolution"):
        ME.grid_for(pts, resolution=0)


def test_mesh_ply_round_trip_is_exact(tmp_path):
    from cer_mvs_amd import mesh as ME
    rng = np.random.default_rng(3)
    v = rng.normal(size=(57, 3)).astype(np.float32)
    v[5, 1], v[6, 2] = np.float32(-0.0), np.float32(1e-42)                        # (a negative zero and a denormal survive)
    f = rng.integers(0, 57, size=(101, 3)).astype(np.int32)
    ME.write_mesh_ply(tmp_path / "m.ply", v, f)
    raw = open(tmp_path / "m.ply", "rb").read()
    head = raw.split(b"end_header\n")[0].decode("ascii")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 57\n") and "element face 101\nproperty list uchar int vertex_indices\n" in head
    assert len(raw) == len(head) + len("end_header\n") + 57 * 12 + 101 * 13
    v2, f2 = ME.read_mesh_ply(tmp_path / "m.ply")
    assert v2.dtype == np.float32 and f2.dtype == np.int32
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f)
    ME.write_mesh_ply(tmp_path / "t.ply", torch.from_numpy(v), torch.from_numpy(f))             # tensors are taken too
    assert open(tmp_path / "t.ply", "rb").read() == raw
    ME.write_mesh_ply(tmp_path / "e.ply", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v0, f0 = ME.read_mesh_ply(tmp_path / "e.ply")
    assert v0.shape == (0, 3) and f0.shape == (0, 3)
    with pytest.raises(ValueError, match="indices"):
        ME.write_mesh_ply(tmp_path / "x.ply", v, f + 57)
    with pytest.raises(ValueError, match="expected"):
        ME.write_mesh_ply(tmp_path / "x.ply", v[:, :2], f)
    open(tmp_path / "bad.ply", "wb").write(raw[:-5])
    with pytest.raises(ValueError, match="bytes"):
        ME.read_mesh_ply(tmp_path / "bad.ply")
    open(tmp_path / "cloud.ply", "wb").write(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="not a mesh"):
        ME.read_mesh_ply(tmp_path / "cloud.ply")


# ---------------------------------------------------------------- the restatement, held to the prototype's properties
def test_forward_cams_packs_the_float32_matrices():
    from cer_mvs_amd import mesh as ME
    _, _, Ks, Es = M.sphere_views()
    cams = ME.forward_cams(Ks, Es).numpy()
    assert cams.shape == (10, 24) and cams.dtype == np.float64
    assert np.array_equal(cams[:, :9], Ks.reshape(10, 9).astype(np.float64)) and np.array_equal(cams[:, 9:21], Es[:, :3].reshape(10, 12).astype(np.float64))
    assert not cams[:, 21:].any()


@pytest.mark.parametrize("n, r, nv, nf, bound", [(12, 4.2, 970, 1936, 0.15), (9, 2.7, 400, 796, 0.2)])
def test_restatement_meshes_the_sphere_field(n, r, nv, nf, bound):
    tsdf, weight, grid, centre = M.sphere_field(n, r)
    v, f = M.extract_mesh(tsdf, weight, grid)
    assert v.dtype == np.float32 and f.dtype == np.int32
    once, closed, n_edges, boundary = M.edge_stats(f, len(v))
    out, flat = M.outward(v, f, centre)
    dist = M.sphere_distance(v, centre, r)
    print(f"{n}^3, r = {r}: {len(v)} vertices, {len(f)} faces, {n_edges} edges, {boundary} boundary edges, {flat} zero-area faces, within {dist:.4f} voxel")
    assert (len(v), len(f)) == (nv, nf)
    assert once and closed and boundary == 0                                      # every directed edge once and its reverse once
    assert len(v) - n_edges + len(f) == 2 == M.euler_characteristic(v, f)
    assert out and flat == 0
    assert np.array_equal(np.unique(f), np.arange(len(v)))                        # every vertex referenced
    assert dist <= bound
    # the vertex slots by their own rule are the slots the faces reference, in this order
    slots = M.vertex_slots(tsdf, weight, grid)
    assert len(slots) == len(v)
    node, d = slots >> 3, slots & 7
    i, j, k = node % n, (node // n) % n, node // (n * n)
    lo = np.stack([i, j, k], 1)
    hi = lo + np.stack([d & 1, (d >> 1) & 1, d >> 2], 1)
    assert ((v >= lo) & (v <= hi)).all()                                          # each vertex on its own lattice edge


@pytest.fixture(scope="module")
def integrated_sphere():
    depths, masks, Ks, Es = M.sphere_views()
    grid = M.sphere_grid()
    tsdf, weight = M.tsdf_volume(depths, masks, Ks, Es, grid, 2 * grid[1])
    return depths, masks, grid, tsdf, weight


def test_restatement_integrates_and_meshes_the_sphere_views(integrated_sphere):
    depths, masks, grid, tsdf, weight = integrated_sphere
    assert depths.shape == (10, 48, 64) and 0.05 < masks.mean() < 0.5
    assert tsdf.dtype == np.float32 and weight.dtype == np.int32 and tsdf.shape == weight.shape == (39, 43, 41)
    assert weight.max() <= 10 and (tsdf[weight == 0] == 1.0).all() and (np.abs(tsdf) <= 1.0).all()
    v, f = M.extract_mesh(tsdf, weight, grid)
    once, closed, n_edges, boundary = M.edge_stats(f, len(v))
    out, flat = M.outward(v, f, M.SPHERE_CENTRE)
    dist = M.sphere_distance(v, M.SPHERE_CENTRE, 1.0) / grid[1]
    print(f"integrated sphere, trunc 2 voxels: {len(v)} vertices, {len(f)} faces, {boundary} boundary edges, {flat} zero-area faces, within {dist:.3f} voxel")
    assert len(f) > 10000 and once and out
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    assert dist <= 1.0


def test_integration_order_of_views_is_the_summation_order(integrated_sphere):
    """the sum runs in list order: a permutation may change the last bit of a node, never its count; a repeated view counts twice"""
    depths, masks, grid, tsdf, weight = integrated_sphere
    small = M.small_sphere_grid()
    _, _, Ks, Es = M.sphere_views()
    a, wa = M.tsdf_volume(depths, masks, Ks, Es, small, 0.14, views=[0, 2, 4, 6])
    b, wb = M.tsdf_volume(depths, masks, Ks, Es, small, 0.14, views=[6, 4, 2, 0])
    c, wc = M.tsdf_volume(depths, masks, Ks, Es, small, 0.14, views=[0, 0, 2, 4, 6])
    assert np.array_equal(wa, wb) and np.abs(a - b).max() <= 2e-7 and wa.max() >= 2
    assert (wc >= wa).all() and (wc > wa).any()
    e, we = M.tsdf_volume(depths, masks, Ks, Es, small, 0.14, views=[])
    assert not we.any() and (e == 1.0).all()


# ---------------------------------------------------------------- table coverage
def test_case_table_is_oriented_and_consistent():
    """every mixed case of every tet: its triangles use each crossing edge of the tet - an edge between an inside and an outside corner -
    and only those; a mask and its complement give the same triangles with the opposite winding"""
    for tet in M.TETS:
        for m in range(1, 15):
            tris = M.tet_triangles(tet, m)
            ins = {c for l, c in enumerate(tet) if (m >> l) & 1}
            crossing = {M.edge(a, b) for a in tet for b in tet if a < b and ((a in ins) != (b in ins))}
            assert {e for t in tris for e in t} == crossing and len(tris) == (2 if len(ins) == 2 else 1)
            other = M.tet_triangles(tet, 15 - m)
            assert sorted(tuple(sorted(t)) for t in tris) == sorted(tuple(sorted(t)) for t in other) or len(ins) == 2
            if len(ins) != 2:
                (a, b, c), (x, y, z) = tris[0], other[0]
                assert (x, y, z) in ((a, c, b), (c, b, a), (b, a, c))              # the mirror image
        assert M.tet_triangles(tet, 0) == [] and M.tet_triangles(tet, 15) == []


@pytest.mark.parametrize("min_weight", [1, 2])
def test_every_case_of_every_tet_occurs_in_the_random_volume(min_weight):
    tsdf, weight, grid = M.random_volume()
    assert grid[2] == (9, 8, 7) and set(np.unique(weight)) == {0, 1, 2}
    assert np.isnan(tsdf).any() and np.isinf(tsdf).any() and (tsdf == 0).sum() == 6 and np.signbit(tsdf[tsdf == 0]).sum() == 3
    counts = M.tet_pattern_counts(tsdf, weight, grid, min_weight)
    print(f"min_weight {min_weight}: fewest occurrences of a mixed case {counts[:, 1:15].min()}, valid cells {counts[0].sum()}")
    assert (counts[:, 1:15] > 0).all()
    v, f = M.extract_mesh(tsdf, weight, grid, min_weight)
    assert len(f) == int((counts * np.array([0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0])).sum())
    assert M.edge_stats(f, len(v))[0] and np.array_equal(np.unique(f), np.arange(len(v)))
    assert len(M.vertex_slots(tsdf, weight, grid, min_weight)) == len(v)
