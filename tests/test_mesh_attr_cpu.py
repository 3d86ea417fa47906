"""Per-vertex mesh attributes (csrc/mesh.hip, cer-mvs_amd/mesh.py), the parts that need no GPU: the two entry points of ABI 1180
and their argument checks in the documented order, the Python layer's ValueErrors, the PLY round trip in its four forms, and the numpy
restatement of tests/mesh_attr_reference.py - which the GPU tests hold the device to bit for bit - held to what correct attributes look like
on the analytic sphere cases.  The bars below were set from the restatement's own figures (profiles/mesh_attr_parity.json), at roughly 1.5 - 2
times what it measures, rounded up."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_attr_reference as A
import mesh_reference as M
from conftest import REPO

BIG = 1 << 31
NAN, INF = float("nan"), float("inf")
NAMES = ("cer_mesh_vertex_colors_u8", "cer_mesh_vertex_normals_f32")

# measured on the restatement -> bar
NORMAL_ANGLE_BAR_DEG = 20.0        # 12^3 sphere field: the largest angle to the radial direction is 11.64 degrees
PAINT_BAR = 0.06                   # integrated sphere, background painted at the centre's depth: 0.0305
PAINT_BAR_BLACK_BACKGROUND = 0.55  # the same with pixels that see no surface left at 0: 0.326, all of it at the silhouettes
SEEN_SHARE = 0.9                   # measured: every vertex of that mesh is seen (1.0)


# ---------------------------------------------------------------- ABI
def test_attribute_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    names = L.exported_symbols()
    for n in NAMES:
        assert n in names and re.search(r"\bint %s\(" % n, hdr), n
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P                 # a stream: the last argument
    assert L.ABI_VERSION >= 1180 and "ABI 1180" in hdr and len(names) >= 105
    lib = L.load()
    assert lib.cer_abi_version() == L.ABI_VERSION
    src = open(os.path.join(REPO, "cer-mvs_amd", "csrc", "mesh.hip")).read()
    assert "mesh_vertex_color_kernel" in src and "mesh_vertex_normals_kernel" in src          # in mesh.hip: mesh.o's flags


def test_attribute_entry_points_refuse_bad_arguments_in_the_documented_order():
    """every check runs before any launch (the pointers are fake: a launch would fault).  The order: (1) a negative size CER_EINVAL (-1); (2)
    nv, 3 nf or h w >= 2^31 CER_ESHAPE (-2); (3) tol not positive and finite CER_EINVAL; (4) nothing to do CER_OK; (5) null pointers
    CER_EINVAL - each case breaks one rule and every later one, and gets the earlier rule's answer."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None

    def col(ver=fake, nv=5, dep=fake, msk=fake, clr=fake, cams=fake, N=3, h=5, w=7, views=fake, n=3, tol=0.5, rgb=fake, seen=fake):
        return lib.cer_mesh_vertex_colors_u8(ver, nv, dep, msk, clr, cams, N, h, w, views, n, tol, rgb, seen, null)
    cn = dict(ver=null, dep=null, clr=null, cams=null, views=null, rgb=null, seen=null)
    for kw in (dict(nv=-1), dict(N=-1), dict(h=-1), dict(w=-2), dict(n=-1)):                                                      # 1
        assert col(**kw) == -1 and col(**kw, tol=NAN, **cn) == -1, kw
    assert col(nv=-1, h=1 << 16, w=1 << 16) == -1                                   # (negative before too large)
    assert col(nv=BIG) == -2 and col(nv=BIG, tol=-1.0, **cn) == -2                                                                  # 2
    assert col(h=1 << 16, w=1 << 15) == -2 and col(h=1 << 16, w=1 << 15, tol=0.0, n=0) == -2
    for v in (0.0, -1.0, NAN, INF, -INF):                                                                                         # 3
        assert col(tol=v) == -1 and col(tol=v, nv=0) == -1 and col(tol=v, n=0, **cn) == -1, v
    assert col(nv=0) == 0 and col(nv=0, **cn) == 0 and col(n=0) == 0 and col(n=0, **cn) == 0                                        # 4
    assert col(n=0, N=0, h=0, w=0) == 0 and col(nv=BIG - 1, n=0) == 0
    for name in cn:                                                                                                               # 5
        assert col(**{name: null}) == -1, name
    assert col(N=0) == -1 and col(h=0) == -1 and col(w=0) == -1                     # (views listed, nothing to look at)
    assert col(msk=null, **cn) == -1                                                # (masks may be null; the others may not)

    def nrm(ver=fake, nv=5, fac=fake, nf=4, starts=fake, order=fake, out=fake):
        return lib.cer_mesh_vertex_normals_f32(ver, nv, fac, nf, starts, order, out, null)
    nn = dict(ver=null, fac=null, starts=null, order=null, out=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nv=-1, nf=BIG)):                                                                     # 1
        assert nrm(**kw) == -1 and nrm(**kw, **nn) == -1, kw
    assert nrm(nv=BIG) == -2 and nrm(nv=BIG, **nn) == -2                                                                            # 2
    assert nrm(nf=(BIG + 2) // 3) == -2 and nrm(nf=(BIG + 2) // 3, nv=0) == -2 and nrm(nf=1 << 62, **nn) == -2
    assert nrm(nv=0) == 0 and nrm(nv=0, **nn) == 0 and nrm(nv=0, nf=0) == 0 and nrm(nv=0, nf=BIG // 3) == 0                         # 4
    for name in nn:                                                                                                               # 5
        assert nrm(**{name: null}) == -1, name
    assert nrm(nf=0, ver=null) == -1 and nrm(nf=0, starts=null) == -1 and nrm(nf=0, out=null) == -1 and nrm(nf=0, **nn) == -1


# ---------------------------------------------------------------- the Python layer
def test_attribute_python_layer_refuses_bad_arguments_without_a_device():
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    ver = torch.zeros(4, 3)
    dep, msk, clr = torch.ones(3, 5, 7), torch.ones(3, 5, 7, dtype=torch.uint8), torch.zeros(3, 3, 5, 7)
    Ks, Es = torch.eye(3).repeat(3, 1, 1), torch.eye(4).repeat(3, 1, 1)
    for bad in (ver.double(), ver[:, :2], ver[0], ver.numpy()):
        with pytest.raises(ValueError, match="vertices"):
            ME.vertex_colors(bad, dep, msk, clr, Ks, Es, 0.5)
    with pytest.raises(ValueError, match="depths"):
        ME.vertex_colors(ver, dep.double(), msk, clr, Ks, Es, 0.5)
    with pytest.raises(ValueError, match="masks"):
        ME.vertex_colors(ver, dep, msk.bool(), clr, Ks, Es, 0.5)
    with pytest.raises(ValueError, match="masks"):
        ME.vertex_colors(ver, dep, msk[:2], clr, Ks, Es, 0.5)
    for bad in (clr.double(), clr[:2], clr[:, :2], clr.permute(0, 2, 3, 1), torch.zeros(3, 3, 5, 8)):
        with pytest.raises(ValueError, match="colors"):
            ME.vertex_colors(ver, dep, msk, bad, Ks, Es, 0.5)
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="tol"):
            ME.vertex_colors(ver, dep, msk, clr, Ks, Es, bad)
    with pytest.raises(ValueError, match="cameras|Ks"):
        ME.vertex_colors(ver, dep, msk, clr, Ks[:2], Es[:2], 0.5)
    for views in ([3], [-1], [0, 1, 7]):
        with pytest.raises(ValueError, match="views"):
            ME.vertex_colors(ver, dep, msk, clr, Ks, Es, 0.5, views=views)
    with pytest.raises(RuntimeError, match="CUDA"):           # good arguments: the host tensors are what is refused
        ME.vertex_colors(ver, dep, None, clr, Ks, Es, 0.5)
    fac = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    for bad in (fac.long(), fac[:, :2], fac[0], fac.numpy()):
        with pytest.raises(ValueError, match="faces"):
            ME.vertex_normals(ver, bad)
        with pytest.raises(ValueError, match="faces"):
            ME.vertex_faces(bad, 4)
    with pytest.raises(ValueError, match="vertices"):
        ME.vertex_normals(ver.double(), fac)
    for bad in (torch.tensor([[0, 1, 4]], dtype=torch.int32), torch.tensor([[0, -1, 2]], dtype=torch.int32)):
        with pytest.raises(ValueError, match="indices"):
            ME.vertex_normals(ver, bad)
        with pytest.raises(ValueError, match="indices"):
            ME.vertex_faces(bad, 4)
    with pytest.raises(ValueError, match="indices"):
        ME.vertex_faces(fac, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        ME.vertex_normals(ver, fac)
    # the options of reconstruct_scan(mesh=...): refused before a model or a session is built
    for bad in ({"colours": True}, {"colors": False}, {"colors": 1}, {"colors": {"tolerance": 1.0}}, {"colors": {"tol": 0.0}}, {"colors": {"tol": NAN}},
                {"colors": {"tol": "1"}}, {"normals": False}, {"normals": {"k": 3}}, {"normal": True}):
        with pytest.raises(ValueError, match="mesh"):
            ME.mesh_options(bad)
        with pytest.raises(ValueError, match="mesh"):
            reconstruct_scan(None, [0], [0], [0], ["a"], [[0]], [1.0], None, write=False, mesh=bad)
    for good in ({"colors": True}, {"colors": {"tol": 0.25}}, {"colors": {}}, {"normals": True}, {"resolution": 48, "colors": True, "normals": True}):
        assert ME.mesh_options(good) == good
    assert "colours" not in ME.MESH_OPTION_KEYS and {"colors", "normals"} <= set(ME.MESH_OPTION_KEYS)


def test_vertex_faces_is_the_stable_sort_of_the_corners():
    from cer_mvs_amd import mesh as ME
    rng = np.random.default_rng(8)
    f = rng.integers(0, 23, size=(57, 3)).astype(np.int32)
    f[f == 11] = 12                                                               # vertex 11 is unreferenced
    f[5] = (4, 4, 9)                                                              # a face that repeats an index
    starts, order = ME.vertex_faces(torch.from_numpy(f), 25)
    assert starts.dtype == torch.int32 and order.dtype == torch.int32 and starts.shape == (26,) and order.shape == (171,)
    rs, ro = A.vertex_faces(f, 25)
    assert np.array_equal(starts.numpy(), rs) and np.array_equal(order.numpy(), ro)
    keys = f.reshape(-1)
    for v in range(25):
        mine = order.numpy()[rs[v]:rs[v + 1]]
        assert (keys[mine] == v).all() and (np.diff(mine) > 0).all() and len(mine) == (keys == v).sum()
    assert rs[11] == rs[12] and rs[23] == rs[24] == rs[25] == 171
    s0, o0 = ME.vertex_faces(torch.zeros(0, 3, dtype=torch.int32), 6)
    assert s0.tolist() == [0] * 7 and o0.shape == (0,)
    s0, o0 = ME.vertex_faces(torch.zeros(0, 3, dtype=torch.int32), 0)
    assert s0.tolist() == [0] and o0.shape == (0,)


TODAYS_HEAD = ("ply\nformat binary_little_endian 1.0\nelement vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n"
               "element face {nf}\nproperty list uchar int vertex_indices\nend_header\n")


def test_mesh_ply_round_trip_with_attributes_is_exact(tmp_path):
    from cer_mvs_amd import mesh as ME
    rng = np.random.default_rng(3)
    v = rng.normal(size=(57, 3)).astype(np.float32)
    v[5, 1], v[6, 2] = np.float32(-0.0), np.float32(1e-42)
    f = rng.integers(0, 57, size=(101, 3)).astype(np.int32)
    n = rng.normal(size=(57, 3)).astype(np.float32)
    n[3], n[4, 0] = 0.0, np.float32(-0.0)
    c = rng.integers(0, 256, size=(57, 3)).astype(np.uint8)
    # the plain form: the bytes of the writer before the attributes
    ME.write_mesh_ply(tmp_path / "plain.ply", v, f)
    rec = np.empty(101, dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rec["n"], rec["v"] = 3, f
    assert (tmp_path / "plain.ply").read_bytes() == TODAYS_HEAD.format(nv=57, nf=101).encode("ascii") + v.astype("<f4").tobytes() + rec.tobytes()
    ME.write_mesh_ply(tmp_path / "plain2.ply", v, f, normals=None, colors=None)
    assert (tmp_path / "plain2.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
    for nrm, col, props, size in ((None, None, "x y z", 12), (n, None, "x y z nx ny nz", 24), (None, c, "x y z red green blue", 15),
                                  (n, c, "x y z nx ny nz red green blue", 27)):
        path = tmp_path / f"m{size}.ply"
        ME.write_mesh_ply(path, v, f, normals=nrm, colors=col)
        raw = path.read_bytes()
        head = raw.split(b"end_header\n")[0].decode("ascii")
        vertex_part = head.split("element face")[0]
        assert " ".join(ln.split()[2] for ln in vertex_part.split("\n") if ln.startswith("property")) == props
        assert len(raw) == len(head) + len("end_header\n") + 57 * size + 101 * 13
        v2, f2 = ME.read_mesh_ply(path)
        assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f)
        v3, f3, n3, c3 = ME.read_mesh_ply(path, attributes=True)
        assert v3.dtype == np.float32 and f3.dtype == np.int32
        assert np.array_equal(v3.view(np.uint32), v.view(np.uint32)) and np.array_equal(f3, f)
        assert (n3 is None) == (nrm is None) and (c3 is None) == (col is None)
        if nrm is not None:
            assert n3.dtype == np.float32 and np.array_equal(n3.view(np.uint32), n.view(np.uint32))
        if col is not None:
            assert c3.dtype == np.uint8 and np.array_equal(c3, c)
        if nrm is not None and col is not None:                                   # tensors are taken too
            ME.write_mesh_ply(tmp_path / "t.ply", torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(c))
            assert (tmp_path / "t.ply").read_bytes() == raw
            open(tmp_path / "short.ply", "wb").write(raw[:-5])
            with pytest.raises(ValueError, match="bytes"):
                ME.read_mesh_ply(tmp_path / "short.ply", attributes=True)
            open(tmp_path / "swapped.ply", "wb").write(raw.replace(b"property uchar red\nproperty uchar green\n", b"property uchar green\nproperty uchar red\n"))
            with pytest.raises(ValueError, match="not a mesh"):
                ME.read_mesh_ply(tmp_path / "swapped.ply", attributes=True)
    e3, e0 = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    ME.write_mesh_ply(tmp_path / "e.ply", e3, e0, normals=e3, colors=np.zeros((0, 3), np.uint8))
    v0, f0, n0, c0 = ME.read_mesh_ply(tmp_path / "e.ply", attributes=True)
    assert v0.shape == f0.shape == n0.shape == c0.shape == (0, 3)
    with pytest.raises(ValueError, match="normals"):
        ME.write_mesh_ply(tmp_path / "x.ply", v, f, normals=n[:-1])
    with pytest.raises(ValueError, match="colors"):
        ME.write_mesh_ply(tmp_path / "x.ply", v, f, colors=c[:, :2])
    with pytest.raises(ValueError, match="colors"):
        ME.write_mesh_ply(tmp_path / "x.ply", v, f, colors=c.astype(np.float32))


# ---------------------------------------------------------------- the restatement, held to what correct attributes look like
def test_restated_normals_on_hand_made_meshes():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0], [0, 0, 5], [7, 7, 7]], np.float32)
    one = A.vertex_normals(v, np.array([[0, 1, 2]], np.int32))
    assert np.array_equal(one[:3], np.tile(np.float32([0, 0, 1]), (3, 1))) and not one[3:].any()          # unreferenced: zeros
    both = A.vertex_normals(v, np.array([[0, 1, 2], [0, 2, 1]], np.int32))
    assert not both.any() and not np.signbit(both).any()                           # two faces that cancel
    flat = A.vertex_normals(v, np.array([[0, 1, 1], [3, 3, 3]], np.int32))
    assert not flat.any()                                                         # zero-area faces, repeated indices
    two = A.vertex_normals(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32))          # areas 3 and 7.5 (cross lengths 6 and 15): area-weighted
    assert np.allclose(two[0].astype(np.float64), np.array([15.0, 0.0, 6.0]) / np.sqrt(261.0), atol=1e-7)
    assert A.vertex_normals(v, np.zeros((0, 3), np.int32)).shape == (5, 3) and A.vertex_normals(v[:0], np.zeros((0, 3), np.int32)).shape == (0, 3)
    bad = v.copy()
    bad[1, 0] = NAN
    assert not A.vertex_normals(bad, np.array([[0, 1, 2]], np.int32)).any()        # NaN: zeros


def test_restated_normals_on_the_sphere_field():
    tsdf, weight, grid, centre = M.sphere_field(12, 4.2)
    v, f = M.extract_mesh(tsdf, weight, grid)
    assert len(v) == 970
    n = A.vertex_normals(v, f)
    assert n.dtype == np.float32 and n.shape == (970, 3)
    n64 = n.astype(np.float64)
    length = np.linalg.norm(n64, axis=1)
    radial = v.astype(np.float64) - centre
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    dots = (n64 * radial).sum(1)
    angle = float(np.degrees(np.arccos(np.clip(dots / length, -1.0, 1.0))).max())
    print(f"12^3 sphere: |len - 1| <= {np.abs(length - 1.0).max():.3e}, smallest dot {dots.min():.4f}, largest angle to the radial direction {angle:.3f} degrees")
    assert np.abs(length - 1.0).max() <= 2.0 ** -23                                # three components rounded to float32: within one float32 step of 1
    assert (dots > 0.0).all()
    assert angle <= NORMAL_ANGLE_BAR_DEG


@pytest.fixture(scope="module")
def integrated_sphere():
    depths, masks, Ks, Es = M.sphere_views()
    grid = M.sphere_grid()
    tsdf, weight = M.tsdf_volume(depths, masks, Ks, Es, grid, 2 * grid[1])
    v, f = M.extract_mesh(tsdf, weight, grid)
    return depths, masks, Ks, Es, grid, v, f


@pytest.mark.parametrize("fill, bar", [(4.0, PAINT_BAR), (None, PAINT_BAR_BLACK_BACKGROUND)])
def test_restated_colours_reproduce_a_linear_paint_on_the_integrated_sphere(integrated_sphere, fill, bar):
    """every view painted with 0.5 + 0.25 * p of the surface point p a pixel sees.  The bilinear sample uses all four taps whatever their masks,
    so what a pixel WITHOUT a surface holds enters the colours at the silhouettes: with those pixels painted as the point of their ray at
    the sphere centre's depth (4.0) the paint is continuous up to the silhouette's depth step and the error is the interpolation's and the
    mesh's distance to the sphere; with them left at 0 the silhouette vertices are darkened, and the bar says by how much."""
    depths, masks, Ks, Es, grid, v, f = integrated_sphere
    assert v.shape == (11563, 3)
    colors = A.painted_views(depths, masks, Ks, Es, fill=fill)
    assert colors.shape == (10, 3, 48, 64) and colors.dtype == np.float32
    on_surface = colors[np.broadcast_to(masks[:, None] != 0, colors.shape)]
    assert 0.0 < on_surface.min() and on_surface.max() < 1.0                        # the byte rule's clamps stay out of this case
    rgb, seen = A.vertex_colors(v, depths, masks, colors, Ks, Es, 2 * grid[1])
    assert rgb.dtype == np.uint8 and rgb.shape == (11563, 3) and seen.dtype == np.int32 and seen.shape == (11563,)
    err = np.abs(rgb.astype(np.float64) / 255.0 - A.paint(v))[seen > 0]
    share = float((seen > 0).mean())
    print(f"integrated sphere, background {fill}: {share:.4f} of the vertices seen, up to {seen.max()} views, largest colour error {err.max():.4f}")
    assert share >= SEEN_SHARE and seen.max() <= 10
    assert not rgb[seen == 0].any()
    assert err.max() <= bar


def test_restated_colours_respect_occlusion_and_order():
    """a vertex on the far side of the sphere projects into the views in front, whose depth there is the near side's: no colour from them"""
    depths, masks, Ks, Es = M.sphere_views()
    colors = A.painted_views(depths, masks, Ks, Es, fill=4.0)
    far = (M.SPHERE_CENTRE + np.array([[-1.0, 0.0, 0.0], [-0.98, 0.1, 0.1]])).astype(np.float32)          # seen from -x (view 1), hidden from +x (view 0)
    rgb0, seen0 = A.vertex_colors(far, depths, masks, colors, Ks, Es, 0.14, views=[0])
    rgb1, seen1 = A.vertex_colors(far, depths, masks, colors, Ks, Es, 0.14, views=[1])
    assert not seen0.any() and not rgb0.any() and (seen1 == 1).all()
    assert np.abs(rgb1 / 255.0 - A.paint(far)).max() < 0.02
    wide, seen_wide = A.vertex_colors(far, depths, masks, colors, Ks, Es, 2.5, views=[0])               # without the occlusion test: the near side's colour
    assert (seen_wide == 1).all() and np.abs(wide[:, 0] / 255.0 - A.paint(far)[:, 0]).min() > 0.3
    a, sa = A.vertex_colors(far, depths, masks, colors, Ks, Es, 0.14, views=[1, 7, 9])
    b, sb = A.vertex_colors(far, depths, masks, colors, Ks, Es, 0.14, views=[9, 7, 1])
    c, sc = A.vertex_colors(far, depths, masks, colors, Ks, Es, 0.14, views=[1, 1, 7, 9])
    assert np.array_equal(sa, sb) and (sa >= 2).all() and np.abs(a.astype(int) - b.astype(int)).max() <= 1 and (sc == sa + 1).all()
    e, se = A.vertex_colors(far, depths, masks, colors, Ks, Es, 0.14, views=[])
    assert not e.any() and not se.any()
