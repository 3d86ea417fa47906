"""Per-vertex mesh attributes on the MI355X (csrc/mesh.hip, cer-mvs_amd/mesh.py) against the numpy restatement of
tests/mesh_attr_reference.py.  Every comparison is exact: rgb bytes, seen counts, normals as float32 bits.  The restatement itself is held to
what correct attributes look like in tests/test_mesh_attr_cpu.py."""
import numpy as np
import pytest
import torch

import mesh_attr_reference as A
import mesh_reference as M

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev_colors(dev, vertices, depths, masks, colors, Ks, Es, tol, views=None):
    from cer_mvs_amd import mesh as ME
    rgb, seen = ME.vertex_colors(torch.from_numpy(vertices).to(dev), torch.from_numpy(depths).to(dev), None if masks is None else torch.from_numpy(masks).to(dev),
                                 torch.from_numpy(colors).to(dev), torch.from_numpy(Ks), torch.from_numpy(Es), tol, views)
    assert rgb.dtype == torch.uint8 and seen.dtype == torch.int32 and rgb.is_cuda and seen.is_cuda
    assert tuple(rgb.shape) == (len(vertices), 3) and tuple(seen.shape) == (len(vertices),)
    return rgb.cpu().numpy(), seen.cpu().numpy()


def dev_normals(dev, vertices, faces):
    from cer_mvs_amd import mesh as ME
    n = ME.vertex_normals(torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev))
    assert n.dtype == torch.float32 and n.is_cuda and tuple(n.shape) == (len(vertices), 3)
    return n.cpu().numpy()


def assert_same_colors(got, want, what=""):
    (rgb, seen), (rrgb, rseen) = got, want
    assert np.array_equal(seen, rseen), what
    assert np.array_equal(rgb, rrgb), what


# ---------------------------------------------------------------- colours
K0 = np.array([[2.0, 0.0, 3.0], [0.0, 2.0, 2.0], [0.0, 0.0, 1.0]], np.float32)       # view 0 and a vertex at z = 4: x = X / 2 + 3, y = Y / 2 + 2, uz = 4
K2 = np.array([[2.0, 1.0, 3.0], [0.0, 2.0, 2.0], [0.0, 0.0, 1.0]], np.float32)


def small_cams():
    """three 5 x 7 views with small-integer K and E (uz and d - uz are exact): view 0 at the origin looking down +z, view 1 turned round (every
    vertex behind it), view 2 shifted so that part of the vertices leave its image"""
    E0 = np.eye(4, dtype=np.float32)
    E1 = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)
    E1[:3, 3] = (0.0, 0.0, -4.0)                                                   # cz = -z - 4
    E2 = np.eye(4, dtype=np.float32)
    E2[:3, 3] = (4.0, 1.0, 1.0)                                                    # cz = z + 1
    return np.stack([K0, K0, K2]), np.stack([E0, E1, E2])


def lattice(zs=(4.0, 3.75)):
    """vertices over and around view 0's image: at z = 4, x = X / 2 + 3 runs from -0.875 to 6.875 in steps of 1 / 8 and y from -0.5 to 4.75"""
    X = np.arange(-7.75, 8.0, 0.25)
    Y = np.array([-5.0, -4.25, -4.0, -3.0, -1.0, 0.0, 0.5, 2.0, 3.9, 4.5, 5.5])
    g = np.stack(np.meshgrid(X, Y, np.array(zs), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float32)


def small_scene():
    rng = np.random.default_rng(17)
    Ks, Es = small_cams()
    depths = np.stack([rng.choice(np.float32([3.5, 3.75, 4.0, 4.25, 4.5]), size=(5, 7)), np.full((5, 7), 4.0, np.float32),
                       rng.choice(np.float32([4.5, 4.75, 5.0, 5.25]), size=(5, 7))]).astype(np.float32)
    for v in (0, 2):
        depths[v, 0, 1], depths[v, 1, 2], depths[v, 2, 3], depths[v, 3, 4], depths[v, 4, 0] = NAN, INF, 0.0, -4.0, -INF
    masks = (rng.uniform(size=(3, 5, 7)) > 0.2).astype(np.uint8)
    colors = rng.uniform(-0.3, 1.3, (3, 3, 5, 7)).astype(np.float32)                # above 1 and below 0: the byte rule's clamps
    colors[0, 1, 2, 5], colors[2, 0, 1, 1], colors[0, 2, 4, 6], colors[2, 2, 0, 0] = NAN, NAN, 7.5, -3.0
    return depths, masks, colors, Ks, Es


VIEW_LISTS = ((0, 1, 2), (2, 0, 1), None, (2, 2, 0), (1,), ())


@pytest.mark.parametrize("nv", [0, 257, 1386])
def test_colours_equal_the_restatement_on_small_views(dev, nv):
    """masked pixels, NaN / inf / 0 / negative depths, a view behind the vertices, one that part of them leave, view orders, a repeated
    view, no view, masks=None; colours above 1, below 0 and NaN; 257 vertices are a second, ragged block"""
    depths, masks, colors, Ks, Es = small_scene()
    ver = lattice()
    assert len(ver) == 1386
    ver = ver[np.random.default_rng(1).permutation(1386)[:nv]]
    most = 0
    for mk in (masks, None):
        for views in VIEW_LISTS:
            want = A.vertex_colors(ver, depths, mk, colors, Ks, Es, 0.5, views)
            got = dev_colors(dev, ver, depths, mk, colors, Ks, Es, 0.5, views)
            assert_same_colors(got, want, (nv, views, mk is None))
            if views in ((1,), ()):
                assert not got[0].any() and not got[1].any()                      # behind every vertex; nothing asked
            most = max(most, int(want[1].max()) if nv else 0)
    if nv:
        assert most >= 3                                                          # (2, 2, 0): a repeated view counts twice
        for view in (0, 2):                                                       # part of the vertices inside, part outside or refused
            _, s = A.vertex_colors(ver, depths, None, colors, Ks, Es, 0.5, (view,))
            assert (s == 0).any() and (s == 1).any()
        _, s_all = A.vertex_colors(ver, np.full_like(depths, 4.0), None, colors, Ks, Es, 0.5, (0,))
        _, s_bad = A.vertex_colors(ver, np.where(np.isfinite(depths) & (depths > 0), np.float32(4.0), depths), None, colors, Ks, Es, 0.5, (0,))
        _, s_msk = A.vertex_colors(ver, np.full_like(depths, 4.0), masks, colors, Ks, Es, 0.5, (0,))
        assert (s_bad < s_all).any() and (s_msk < s_all).any()                    # the bad pixels and the masks do remove views
        rgb, _ = A.vertex_colors(ver, depths, None, colors, Ks, Es, 0.5)
        assert (rgb == 255).any() and (rgb == 0).any()


def test_colour_taps_clamp_at_the_border_and_vanish_on_pixel_centres(dev):
    depths, _, colors, Ks, Es = small_scene()
    colors = np.nan_to_num(colors, nan=0.25)                                       # (a NaN tap with weight 0 is still NaN: none here)
    flat = np.full_like(depths, 4.0)
    ver = lattice(zs=(4.0,))
    x, y = ver[:, 0].astype(np.float64) / 2 + 3, ver[:, 1].astype(np.float64) / 2 + 2
    want = A.vertex_colors(ver, flat, None, colors, Ks, Es, 0.5, (0,))
    assert_same_colors(dev_colors(dev, ver, flat, None, colors, Ks, Es, 0.5, (0,)), want)
    rgb, seen = want
    inside = (x >= -0.5) & (x < 6.5) & (y >= -0.5) & (y < 4.5)
    assert np.array_equal(seen, inside.astype(np.int32))
    left, right = inside & (x < 0), inside & (x >= 6)
    top, bottom = inside & (y < 0), inside & (y >= 4)
    assert left.sum() >= 8 and right.sum() >= 8 and top.sum() >= 8 and bottom.sum() >= 8
    centre = inside & (x == np.floor(x)) & (y == np.floor(y))
    assert centre.sum() == 7 * 3                                                   # columns 0 .. 6 (X even), rows 0, 2, 3 (Y = -4, 0, 2)

    def byte(c):
        q = c.astype(np.float64) * 255.0
        return np.where(q >= 255.0, 255, np.where(q > 0.0, np.floor(np.clip(q, 0.0, 255.0)), 0)).astype(np.uint8)
    xi, yi = x[centre].astype(int), y[centre].astype(int)
    assert np.array_equal(rgb[centre], byte(colors[0][:, yi, xi].T))               # fx = fy = 0: the pixel's own colour
    # the clamped taps: left of column 0's centre the colour is column 0's, interpolated along y only
    xl, yl = np.zeros(int(left.sum()), int), y[left]
    inner = (yl >= 0) & (yl < 4)
    y0 = np.floor(yl[inner]).astype(int)
    fy = yl[inner] - y0
    col0 = colors[0][:, :, 0].astype(np.float64)
    expect = (1.0 - fy) * col0[:, y0] + fy * col0[:, y0 + 1]
    assert np.abs(rgb[left][inner] / 255.0 - np.clip(expect.T, 0.0, 1.0)).max() <= 1.0 / 255.0 + 1e-12


def test_colour_occlusion_bound_is_inclusive_and_exact(dev):
    _, _, colors, Ks, Es = small_scene()
    colors = np.nan_to_num(colors, nan=0.25)
    depths = np.full((3, 5, 7), 4.0, np.float32)
    depths[0, 2, 5], depths[0, 1, 1] = 4.5, 3.5
    below4 = np.nextafter(np.float32(4.0), np.float32(0.0))
    above4 = np.nextafter(np.float32(4.0), np.float32(8.0))
    ver = np.array([[4.0, 0.0, 4.0],        # pixel (5, 2): d - uz = 0.5 == tol: seen
                    [4.0, 0.0, below4],     # d - uz = 0.5 + 2^-22: not seen
                    [-4.0, -2.0, 4.0],      # pixel (1, 1): d - uz = -0.5: seen
                    [-4.0, -2.0, above4],   # -0.5 - 2^-21: not seen
                    [0.0, 0.0, 4.0]], np.float32)
    want = A.vertex_colors(ver, depths, None, colors, Ks, Es, 0.5, (0,))
    assert want[1].tolist() == [1, 0, 1, 0, 1]
    assert_same_colors(dev_colors(dev, ver, depths, None, colors, Ks, Es, 0.5, (0,)), want)
    tight = float(np.nextafter(0.5, 0.0))                                          # the same vertices a float64 step beyond the bound
    want = A.vertex_colors(ver, depths, None, colors, Ks, Es, tight, (0,))
    assert want[1].tolist() == [0, 0, 0, 0, 1]
    assert_same_colors(dev_colors(dev, ver, depths, None, colors, Ks, Es, tight, (0,)), want)
    # a depth map that is 2 in its left half and 4 in its right half, vertices at z = 4 behind both: the left half's take no colour
    halves = np.full((3, 5, 7), 4.0, np.float32)
    halves[:, :, :3] = 2.0
    ver = lattice(zs=(4.0,))
    x, y = ver[:, 0].astype(np.float64) / 2 + 3, ver[:, 1].astype(np.float64) / 2 + 2
    inside = (x >= -0.5) & (x < 6.5) & (y >= -0.5) & (y < 4.5)
    want = A.vertex_colors(ver, halves, None, colors, Ks, Es, 0.5, (0,))
    assert_same_colors(dev_colors(dev, ver, halves, None, colors, Ks, Es, 0.5, (0,)), want)
    behind_left = inside & (x + 0.5 < 3)
    assert behind_left.sum() > 50 and not want[1][behind_left].any() and not want[0][behind_left].any()
    assert (want[1][inside & ~behind_left] == 1).all()


@pytest.fixture(scope="module")
def sphere_mesh():
    depths, masks, Ks, Es = M.sphere_views()
    grid = M.sphere_grid(dims=(27, 29, 25), voxel=0.1)
    tsdf, weight = M.tsdf_volume(depths, masks, Ks, Es, grid, 0.2)
    v, f = M.extract_mesh(tsdf, weight, grid)
    return depths, masks, Ks, Es, v, f


@pytest.mark.parametrize("fill", [None, 4.0])
def test_colours_equal_the_restatement_on_the_painted_sphere(dev, sphere_mesh, fill):
    depths, masks, Ks, Es, v, f = sphere_mesh
    colors = A.painted_views(depths, masks, Ks, Es, fill=fill)
    want = A.vertex_colors(v, depths, masks, colors, Ks, Es, 0.2)
    got = dev_colors(dev, v, depths, masks, colors, Ks, Es, 0.2)
    print(f"painted sphere, background {fill}: {len(v)} vertices, {(want[1] > 0).mean():.4f} seen, up to {want[1].max()} views")
    assert len(v) > 5000 and (want[1] > 0).mean() > 0.9 and want[1].max() >= 4
    assert_same_colors(got, want)
    again = dev_colors(dev, v, depths, masks, colors, Ks, Es, 0.2)                   # two launches: the same bytes
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


# ---------------------------------------------------------------- normals
def test_normals_equal_the_restatement_on_hand_made_meshes(dev):
    from cer_mvs_amd import mesh as ME
    rng = np.random.default_rng(23)
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0], [0, 0, 5], [7, 7, 7]], np.float32)
    cases = {"one triangle, unreferenced vertices": [[0, 1, 2]], "a zero-area face": [[0, 1, 1], [3, 3, 3]], "two faces that cancel": [[0, 1, 2], [0, 2, 1]],
             "a face that repeats an index": [[0, 0, 1], [0, 1, 2], [2, 2, 2], [3, 0, 3]], "two areas": [[0, 1, 2], [0, 2, 3], [4, 3, 1]]}
    for what, faces in cases.items():
        faces = np.array(faces, np.int32)
        want = A.vertex_normals(v, faces)
        got = dev_normals(dev, v, faces)
        assert np.array_equal(bits(got), bits(want)), what
    one = dev_normals(dev, v, np.array([[0, 1, 2]], np.int32))
    assert np.array_equal(one[:3], np.tile(np.float32([0, 0, 1]), (3, 1))) and not bits(one[3:]).any()
    assert not bits(dev_normals(dev, v, np.array([[0, 1, 2], [0, 2, 1]], np.int32))).any()                 # (0, 0, 0), no negative zero
    # a fan of 40 triangles around vertex 0: forty terms summed in corner order
    ang = np.sort(rng.uniform(0.0, 2 * np.pi, 40))
    rim = np.stack([np.cos(ang) * rng.uniform(0.5, 2.0, 40), np.sin(ang) * rng.uniform(0.5, 2.0, 40), rng.normal(size=40) * 0.3], 1)
    fan_v = np.concatenate([[[0.05, -0.02, 0.4]], rim]).astype(np.float32)
    fan_f = np.array([[0, 1 + i, 1 + (i + 1) % 40] for i in range(40)], np.int32)
    want = A.vertex_normals(fan_v, fan_f)
    assert np.array_equal(bits(dev_normals(dev, fan_v, fan_f)), bits(want)) and want[0, 2] > 0.5
    shuffled = fan_f[rng.permutation(40)]                                          # another face order: another summation order, still the restatement's
    assert np.array_equal(bits(dev_normals(dev, fan_v, shuffled)), bits(A.vertex_normals(fan_v, shuffled)))
    # NaN and inf positions: zeros where they reach
    bad = v.copy()
    bad[1, 0], bad[3, 2] = NAN, INF
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 2, 0]], np.int32)
    want = A.vertex_normals(bad, faces)
    assert np.array_equal(bits(dev_normals(dev, bad, faces)), bits(want)) and not want[:4].any() and want[4].any()
    # no face: zeros for every vertex; no vertex: nothing
    none = dev_normals(dev, v, np.zeros((0, 3), np.int32))
    assert none.shape == (5, 3) and not bits(none).any()
    assert dev_normals(dev, v[:0], np.zeros((0, 3), np.int32)).shape == (0, 3)
    for faces in ([[0, 1, 5]], [[0, -1, 2]]):
        with pytest.raises(ValueError, match="indices"):
            ME.vertex_normals(torch.from_numpy(v).to(dev), torch.tensor(faces, dtype=torch.int32, device=dev))
    # the incidence lists of the device's torch ops are the restatement's
    starts, order = ME.vertex_faces(torch.from_numpy(fan_f).to(dev), 41)
    rs, ro = A.vertex_faces(fan_f, 41)
    assert starts.dtype == order.dtype == torch.int32 and np.array_equal(starts.cpu().numpy(), rs) and np.array_equal(order.cpu().numpy(), ro)


def test_normals_equal_the_restatement_on_the_sphere_field(dev):
    tsdf, weight, grid, centre = M.sphere_field(12, 4.2)
    v, f = M.extract_mesh(tsdf, weight, grid)
    assert len(v) == 970
    want = A.vertex_normals(v, f)
    got = dev_normals(dev, v, f)
    assert np.array_equal(bits(got), bits(want))
    radial = v.astype(np.float64) - centre
    assert ((got.astype(np.float64) * radial).sum(1) > 0).all()


def test_normals_equal_the_restatement_across_blocks(dev):
    tsdf, weight, grid, centre = M.sphere_field((65, 64, 64), 24.3)
    v, f = M.extract_mesh(tsdf, weight, grid)
    assert len(v) == 33266 and len(f) == 66528
    want = A.vertex_normals(v, f)
    got = dev_normals(dev, v, f)
    assert np.array_equal(bits(got), bits(want))
    assert dev_normals(dev, v, f).tobytes() == got.tobytes()                       # two launches: the same bytes
    length = np.linalg.norm(got.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() <= 2.0 ** -23


# ---------------------------------------------------------------- chain
def test_reconstruct_scan_with_mesh_colours_and_normals(dev, tmp_path, monkeypatch):
    """mesh={"resolution": 48, "colors": True, "normals": True} on the small synthetic scan: everything a run with mesh={"resolution": 48}
    gives is byte-equal; the attributes are those of the direct calls and of the restatement; result_mesh.ply holds all four arrays"""
    import test_reconstruct_gpu as TR
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    images, poses, intr, scales = TR._scan(128, 160)
    model = TR._model(dev)
    kw = dict(num_frames=TR.NF, streams=2)
    seen_args = {}
    inner = ME.mesh_of_scan

    def spy(xyz, est, masks, Ks, Es, refs, options, colors=None):
        seen_args.update(est=est, masks=masks, Ks=Ks, Es=Es, refs=list(refs), colors=colors)
        return inner(xyz, est, masks, Ks, Es, refs, options, colors=colors)
    monkeypatch.setattr(ME, "mesh_of_scan", spy)
    t_plain, t_attr = {}, {}
    plain = reconstruct_scan(model, images, poses, intr, TR.NAMES, TR.PAIRS, scales, tmp_path / "plain", mesh={"resolution": 48}, timings=t_plain, **kw)
    out = reconstruct_scan(model, images, poses, intr, TR.NAMES, TR.PAIRS, scales, tmp_path / "attr", mesh={"resolution": 48, "colors": True, "normals": True},
                           timings=t_attr, **kw)
    assert set(out) - set(plain) == {"mesh_colors", "mesh_normals"} and set(plain) <= set(out)
    assert set(out["mesh_info"]) - set(plain["mesh_info"]) == {"coloured"}
    for k in ("xyz", "rgb", "masks", "depth_est", "mesh_vertices", "mesh_faces"):
        assert out[k].dtype == plain[k].dtype and out[k].tobytes() == plain[k].tobytes(), k
    assert (tmp_path / "plain" / "result.ply").read_bytes() == (tmp_path / "attr" / "result.ply").read_bytes()
    v, f, col, nrm, info = out["mesh_vertices"], out["mesh_faces"], out["mesh_colors"], out["mesh_normals"], out["mesh_info"]
    nv = len(v)
    print(f"reconstruct_scan mesh attributes: {info}")
    assert nv > 0 and col.dtype == np.uint8 and col.shape == (nv, 3) and nrm.dtype == np.float32 and nrm.shape == (nv, 3)
    assert t_attr["d2h_bytes"] - t_plain["d2h_bytes"] == nv * 3 + nv * 12
    # the direct calls, on what the mesh step was given
    a = seen_args
    dv, df = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    rgb, seen = ME.vertex_colors(dv, a["est"], a["masks"], a["colors"], a["Ks"], a["Es"], info["trunc"], views=a["refs"])
    assert np.array_equal(rgb.cpu().numpy(), col) and info["coloured"] == int((seen > 0).sum()) and 0 < info["coloured"] <= nv
    assert np.array_equal(bits(ME.vertex_normals(dv, df).cpu().numpy()), bits(nrm))
    # and the restatement
    want = A.vertex_colors(v, a["est"].cpu().numpy(), a["masks"].cpu().numpy(), a["colors"].cpu().numpy(), a["Ks"].cpu().numpy(), a["Es"].cpu().numpy(),
                           info["trunc"], a["refs"])
    assert np.array_equal(want[0], col) and np.array_equal(want[1], seen.cpu().numpy())
    assert np.array_equal(bits(A.vertex_normals(v, f)), bits(nrm))
    pv, pf = ME.read_mesh_ply(tmp_path / "plain" / "result_mesh.ply")
    rv, rf, rn, rc = ME.read_mesh_ply(tmp_path / "attr" / "result_mesh.ply", attributes=True)
    assert np.array_equal(bits(rv), bits(v)) and np.array_equal(rf, f) and np.array_equal(bits(rn), bits(nrm)) and np.array_equal(rc, col)
    assert np.array_equal(bits(pv), bits(v)) and np.array_equal(pf, f)
    assert ME.read_mesh_ply(tmp_path / "plain" / "result_mesh.ply", attributes=True)[2:] == (None, None)
