"""Surface mesh on the MI355X (csrc/mesh.hip, cer-mvs_amd/mesh.py) against the numpy restatement of tests/mesh_reference.py.  Every
comparison is exact: tsdf as float32 bits, weight, vertices as bits, faces as indices.  The restatement itself is held to the properties of a
correct mesher in tests/test_mesh_cpu.py, where every case of the tetrahedron table is shown to occur in the random volume used here."""
import numpy as np
import pytest
import torch

import mesh_reference as M

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(bits(a), bits(b))


def dev_volume(dev, depths, masks, Ks, Es, grid, trunc, views=None):
    from cer_mvs_amd import mesh as ME
    t, w = ME.tsdf_volume(torch.from_numpy(depths).to(dev), None if masks is None else torch.from_numpy(masks).to(dev), torch.from_numpy(Ks),
                          torch.from_numpy(Es), grid, trunc, views)
    assert t.dtype == torch.float32 and w.dtype == torch.int32 and t.is_cuda and w.is_cuda
    return t.cpu().numpy(), w.cpu().numpy()


def dev_mesh(dev, tsdf, weight, grid, min_weight=1):
    from cer_mvs_amd import mesh as ME
    v, f = ME.extract_mesh(torch.from_numpy(tsdf).to(dev), torch.from_numpy(weight).to(dev), grid, min_weight)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    return v.cpu().numpy(), f.cpu().numpy()


def assert_same_mesh(got, want, what=""):
    (v, f), (rv, rf) = got, want
    assert v.shape == rv.shape and f.shape == rf.shape, f"{what}: {v.shape} / {f.shape} against {rv.shape} / {rf.shape}"
    assert np.array_equal(f, rf), what
    assert same_bits(v, rv), what


# ---------------------------------------------------------------- integration
def small_views():
    """three 5 x 7 views of the region around the origin: view 0 in front of it, view 1 looking away from it (every node behind the camera), view
    2 shifted so that part of the nodes leave the image; depths around the nodes' own, with NaN, inf, 0 and negative pixels; a mask with holes"""
    rng = np.random.default_rng(7)
    K = np.array([[4.0, 0.1, 3.0], [0.0, 4.2, 2.0], [0.0, 0.0, 1.0]], np.float32)
    E0 = np.eye(4, dtype=np.float32)
    E0[:3, 3] = (-0.9, -0.6, 4.0)
    E1 = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)                       # turned round: cz = -z - 4
    E1[:3, 3] = (0.0, 0.0, -4.0)
    c, s = np.cos(0.3), np.sin(0.3)
    E2 = np.array([[c, 0.0, s, -2.5], [0.0, 1.0, 0.0, -0.2], [-s, 0.0, c, 5.0], [0.0, 0.0, 0.0, 1.0]], np.float32)
    depths = rng.uniform(3.5, 6.5, (3, 5, 7)).astype(np.float32)
    for v in (0, 2):
        depths[v, 0, 1], depths[v, 1, 2], depths[v, 2, 3], depths[v, 3, 4], depths[v, 4, 0] = NAN, INF, 0.0, -4.5, -INF
    masks = (rng.uniform(size=(3, 5, 7)) > 0.25).astype(np.uint8)
    return depths, masks, np.stack([K, K, K]), np.stack([E0, E1, E2])


SMALL_GRIDS = [(1, 1, 1), (2, 2, 2), (7, 5, 3), (65, 3, 2)]


@pytest.mark.parametrize("dims", SMALL_GRIDS)
def test_integration_equals_the_restatement_on_small_grids(dev, dims):
    depths, masks, Ks, Es = small_views()
    grid = ((-0.31, -0.17, 0.05), 0.27, dims)
    seen = 0
    for mk in (masks, None):
        for views in ((0, 1, 2), (2, 0, 1), None, (2, 2, 0), (1,)):
            rt, rw = M.tsdf_volume(depths, mk, Ks, Es, grid, 0.8, views)
            t, w = dev_volume(dev, depths, mk, Ks, Es, grid, 0.8, views)
            assert np.array_equal(w, rw), (dims, views)
            assert same_bits(t, rt), (dims, views)
            if views == (1,):
                assert not w.any() and (t == 1.0).all()                          # entirely behind the grid
            seen = max(seen, int(rw.max()))
    assert seen >= 2 or dims == (1, 1, 1)
    if dims == (65, 3, 2):                                                        # part of the nodes outside the image, part inside
        for view in (0, 2):
            _, w0 = M.tsdf_volume(depths, None, Ks, Es, grid, 0.8, (view,))
            assert (w0 == 0).any() and (w0 == 1).any()


def test_integration_of_no_views_and_of_masked_and_bad_pixels(dev):
    depths, masks, Ks, Es = small_views()
    grid = ((-0.31, -0.17, 0.05), 0.27, (7, 5, 3))
    t, w = dev_volume(dev, depths, masks, Ks, Es, grid, 0.8, [])
    assert t.shape == (3, 5, 7) and not w.any() and (t == 1.0).all()
    # nothing but bad pixels: nothing contributes
    bad = np.tile(np.float32([NAN, INF, 0.0, -1.0, -INF, NAN, 0.0]), (3, 5, 1))
    t, w = dev_volume(dev, bad, None, Ks, Es, grid, 0.8)
    assert not w.any() and (t == 1.0).all()
    t, w = dev_volume(dev, depths, np.zeros_like(masks), Ks, Es, grid, 0.8)
    assert not w.any() and (t == 1.0).all()
    # the masks and the bad pixels of small_views() do remove contributions
    _, w_all = M.tsdf_volume(np.full_like(depths, 4.6), None, Ks, Es, grid, 0.8)
    _, w_bad = M.tsdf_volume(np.where(np.isfinite(depths) & (depths > 0), np.float32(4.6), depths), None, Ks, Es, grid, 0.8)
    _, w_msk = M.tsdf_volume(np.full_like(depths, 4.6), masks, Ks, Es, grid, 0.8)
    assert (w_bad < w_all).any() and (w_msk < w_all).any()


@pytest.fixture(scope="module")
def sphere():
    depths, masks, Ks, Es = M.sphere_views()
    return {"depths": depths, "masks": masks, "Ks": Ks, "Es": Es}


def test_integration_equals_the_restatement_on_the_sphere_views(dev, sphere):
    grid = M.sphere_grid(dims=(27, 29, 25), voxel=0.1)
    args = (sphere["depths"], sphere["masks"], sphere["Ks"], sphere["Es"], grid, 0.2)
    rt, rw = M.tsdf_volume(*args)
    t, w = dev_volume(dev, *args)
    assert rw.max() >= 4 and (rt < 0).any() and (rw == 0).any()
    assert np.array_equal(w, rw) and same_bits(t, rt)
    t2, w2 = dev_volume(dev, *args)                                               # two launches: the same bytes
    assert np.array_equal(w2, w) and same_bits(t2, t)


# ---------------------------------------------------------------- extraction
def test_extraction_equals_the_restatement_on_the_sphere_field(dev):
    tsdf, weight, grid, centre = M.sphere_field(12, 4.2)
    got = dev_mesh(dev, tsdf, weight, grid)
    assert got[0].shape == (970, 3) and got[1].shape == (1936, 3)
    assert_same_mesh(got, M.extract_mesh(tsdf, weight, grid), "12^3 sphere")
    moved = ((-3.7, 11.0, 0.25), 0.013, grid[2])                                  # another frame: the same faces, other coordinates
    assert_same_mesh(dev_mesh(dev, tsdf, weight, moved), M.extract_mesh(tsdf, weight, moved), "12^3 sphere, moved")


def test_single_cell_in_all_256_sign_patterns(dev):
    rng = np.random.default_rng(11)
    mag = rng.uniform(0.1, 1.0, 8).astype(np.float32)
    grid = ((0.5, -0.25, 2.0), 0.75, (2, 2, 2))
    weight = np.ones((2, 2, 2), np.int32)
    total = 0
    for pattern in range(256):
        sign = np.array([-1.0 if (pattern >> c) & 1 else 1.0 for c in range(8)], np.float32)
        tsdf = (sign * mag).reshape(2, 2, 2)                                      # corner c = node (c & 1, (c >> 1) & 1, c >> 2): [z, y, x] order
        want = M.extract_mesh(tsdf, weight, grid)
        assert_same_mesh(dev_mesh(dev, tsdf, weight, grid), want, f"pattern {pattern}")
        assert (len(want[1]) == 0) == (pattern in (0, 255))
        total += len(want[1])
    assert total > 256 * 4


@pytest.mark.parametrize("min_weight", [1, 2])
def test_extraction_equals_the_restatement_on_the_random_volume(dev, min_weight):
    tsdf, weight, grid = M.random_volume()
    want = M.extract_mesh(tsdf, weight, grid, min_weight)
    assert len(want[1]) > 100
    assert_same_mesh(dev_mesh(dev, tsdf, weight, grid, min_weight), want, f"random volume, min_weight {min_weight}")


def test_extraction_of_flat_and_all_positive_volumes_is_empty(dev):
    from cer_mvs_amd import mesh as ME
    rng = np.random.default_rng(2)
    for dims in ((9, 1, 7), (1, 8, 7), (9, 8, 1), (1, 1, 1)):                      # an axis of length 1: no cell
        nx, ny, nz = dims
        v, f = dev_mesh(dev, rng.normal(size=(nz, ny, nx)).astype(np.float32), np.ones((nz, ny, nx), np.int32), ((0.0, 0.0, 0.0), 1.0, dims))
        assert v.shape == (0, 3) and f.shape == (0, 3)
    tsdf = rng.uniform(0.0, 1.0, (7, 8, 9)).astype(np.float32)
    tsdf[3, 4, 5] = 0.0
    tsdf[2, 2, 2] = -0.0                                                          # zeros are outside
    weight, grid = np.ones((7, 8, 9), np.int32), ((0.0, 0.0, 0.0), 1.0, (9, 8, 7))
    v, f = dev_mesh(dev, tsdf, weight, grid)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    nv, nf, ws = ME.mesh_counts(torch.from_numpy(tsdf).to(dev), torch.from_numpy(weight).to(dev), grid)
    assert (nv, nf) == (0, 0) and ws is not None
    # an inside region that no valid cell touches: nothing either
    tsdf[3:5, 3:5, 3:5] = -1.0
    v, f = dev_mesh(dev, tsdf, np.zeros_like(weight), grid)
    assert v.shape == (0, 3) and f.shape == (0, 3)


@pytest.fixture(scope="module")
def big_field():
    """65 x 64 x 64 = 266 240 nodes: 1040 vertex partials and 1489 face partials - more than one compaction tile per pass, more than one
    1024-partial chunk of the scan"""
    tsdf, weight, grid, centre = M.sphere_field((65, 64, 64), 24.3)
    return tsdf, weight, grid, centre, M.extract_mesh(tsdf, weight, grid)


def test_extraction_equals_the_restatement_across_tiles_and_scan_chunks(dev, big_field):
    from cer_mvs_amd import _lib as L
    tsdf, weight, grid, centre, want = big_field
    assert tsdf.size == 266240 and L.load().cer_mesh_partials(65, 64, 64) == 1040 + 1489
    got = dev_mesh(dev, tsdf, weight, grid)
    print(f"65x64x64 sphere: {len(got[0])} vertices, {len(got[1])} faces")
    assert len(want[1]) > 20000
    assert_same_mesh(got, want, "65x64x64 sphere")
    again = dev_mesh(dev, tsdf, weight, grid)                                      # two launches: the same bytes
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
    once, closed, n_edges, boundary = M.edge_stats(got[1], len(got[0]))
    assert once and closed and len(got[0]) - n_edges + len(got[1]) == 2 and M.outward(got[0], got[1], centre)[0]


def test_emit_never_writes_past_the_capacity(dev, big_field):
    from cer_mvs_amd import mesh as ME
    tsdf, weight, grid, centre, (rv, rf) = big_field
    nv, nf, ws = ME.mesh_counts(torch.from_numpy(tsdf).to(dev), torch.from_numpy(weight).to(dev), grid)
    assert (nv, nf) == (len(rv), len(rf))                                          # the totals are reported whatever the capacity will be
    for vcap, fcap in ((nv - 1, nf - 1), (2049, 4097), (nv, 7), (0, 5), (3, 0)):
        vert = torch.full((nv + 8, 3), -7.5, device=dev)
        face = torch.full((nf + 8, 3), -9, device=dev, dtype=torch.int32)
        ME.mesh_emit(grid, nv, nf, ws, vertex_capacity=vcap, face_capacity=fcap, vertices=vert, faces=face)
        v, f = vert.cpu().numpy(), face.cpu().numpy()
        assert same_bits(v[:vcap], rv[:vcap]) and (v[vcap:] == -7.5).all(), (vcap, fcap)
        assert np.array_equal(f[:fcap], rf[:fcap]) and (f[fcap:] == -9).all(), (vcap, fcap)


# ---------------------------------------------------------------- chain and drivers
def test_integrated_sphere_chain_on_the_device(dev, sphere):
    """depth maps -> volume -> mesh without the restatement in between: the device's own output has the properties the CPU test asks of the
    restatement, and is the restatement's output"""
    from cer_mvs_amd import mesh as ME
    grid = M.sphere_grid()
    info = {}
    v, f = ME.mesh_from_depth_maps(torch.from_numpy(sphere["depths"]).to(dev), torch.from_numpy(sphere["masks"]).to(dev), torch.from_numpy(sphere["Ks"]),
                                   torch.from_numpy(sphere["Es"]), ME.Grid(*grid), trunc=2 * grid[1], info=info)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    once, closed, n_edges, boundary = M.edge_stats(f, len(v))
    out, flat = M.outward(v, f, M.SPHERE_CENTRE)
    dist = M.sphere_distance(v, M.SPHERE_CENTRE, 1.0) / grid[1]
    print(f"device chain: {len(v)} vertices, {len(f)} faces, {boundary} boundary edges, {flat} zero-area faces, within {dist:.3f} voxel; info {info}")
    assert len(f) > 10000 and once and out and dist <= 1.0
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    assert info["nv"] == len(v) and info["nf"] == len(f) and info["trunc"] == 2 * grid[1] and info["grid"] == ME.Grid(*grid) and info["observed"] > 0
    rt, rw = M.tsdf_volume(sphere["depths"], sphere["masks"], sphere["Ks"], sphere["Es"], grid, 2 * grid[1])
    assert info["observed"] == int((rw >= 1).sum())
    assert_same_mesh((v, f), M.extract_mesh(rt, rw, grid), "integrated sphere")


def test_mesh_from_synthetic_depth_maps_equals_the_restatement(dev):
    from cer_mvs_amd import fusion, mesh as ME
    from cer_mvs_amd.synthetic import synthetic_depth_maps, synthetic_scene
    H, W, V = 48, 64, 4
    _, poses, intr, _ = synthetic_scene(H, W, V, seed=1)
    Ks, Es = intr[0].float().numpy(), poses[0].float().numpy()
    depths = synthetic_depth_maps(H, W, V, seed=1).numpy().astype(np.float32)
    masks = (np.random.default_rng(4).uniform(size=depths.shape) > 0.1).astype(np.uint8)
    pts = fusion.backproject(depths[0].astype(np.float64), np.ones((H, W), bool), Ks[0].astype(np.float64), Es[0].astype(np.float64))
    grid = ME.grid_for(torch.from_numpy(pts).float(), resolution=24)
    assert max(grid.dims) <= 34 and min(grid.dims) >= 7
    for trunc, views, mw in ((None, None, 1), (2.5 * grid.voxel, [3, 0, 1], 2)):
        info = {}
        v, f = ME.mesh_from_depth_maps(torch.from_numpy(depths).to(dev), torch.from_numpy(masks).to(dev), torch.from_numpy(Ks), torch.from_numpy(Es),
                                       grid, trunc=trunc, views=views, min_weight=mw, info=info)
        tr = 3.0 * grid.voxel if trunc is None else trunc
        assert info["trunc"] == tr
        rt, rw = M.tsdf_volume(depths, masks, Ks, Es, grid, tr, views)
        want = M.extract_mesh(rt, rw, grid, mw)
        assert len(want[1]) > 100
        assert_same_mesh((v.cpu().numpy(), f.cpu().numpy()), want, f"synthetic depth maps, views {views}")


def test_reconstruct_scan_with_a_mesh(dev, tmp_path):
    """mesh={"resolution": 48} on a small synthetic scan: the cloud, the masks and the depths are the bytes of a run without it; the mesh is
    a mesh inside its grid, and result_mesh.ply holds it"""
    import test_reconstruct_gpu as TR
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    images, poses, intr, scales = TR._scan(128, 160)
    model = TR._model(dev)
    kw = dict(num_frames=TR.NF, streams=2)
    plain = reconstruct_scan(model, images, poses, intr, TR.NAMES, TR.PAIRS, scales, tmp_path / "plain", **kw)
    out = reconstruct_scan(model, images, poses, intr, TR.NAMES, TR.PAIRS, scales, tmp_path / "mesh", mesh={"resolution": 48}, **kw)
    assert set(out) - set(plain) == {"mesh_vertices", "mesh_faces", "mesh_info"} and set(plain) <= set(out)
    assert not (tmp_path / "plain" / "result_mesh.ply").exists()
    for k in ("xyz", "rgb", "masks", "depth_est"):
        assert out[k].dtype == plain[k].dtype and out[k].tobytes() == plain[k].tobytes(), k
    assert (tmp_path / "plain" / "result.ply").read_bytes() == (tmp_path / "mesh" / "result.ply").read_bytes()
    v, f, info = out["mesh_vertices"], out["mesh_faces"], out["mesh_info"]
    print(f"reconstruct_scan mesh: {info}")
    assert v.dtype == np.float32 and f.dtype == np.int32 and info["nv"] == len(v) and info["nf"] == len(f) > 0
    assert f.min() >= 0 and f.max() < len(v)
    assert M.edge_stats(f, len(v))[0]                                             # every directed edge at most once
    grid = info["grid"]
    lo = np.array(grid.origin)
    hi = lo + (np.array(grid.dims) - 1) * grid.voxel
    slack = np.spacing(np.abs(np.stack([lo, hi])).max().astype(np.float32)).astype(np.float64)   # one float32 rounding of a coordinate
    assert (v >= lo - slack).all() and (v <= hi + slack).all()
    assert abs(max(grid.dims) - 1 - 48 - 6) <= 2 and info["trunc"] == 3.0 * grid.voxel and 0 < info["observed"] <= int(np.prod(grid.dims))
    rv, rf = ME.read_mesh_ply(tmp_path / "mesh" / "result_mesh.ply")
    assert same_bits(rv, v) and np.array_equal(rf, f)
    with pytest.raises(ValueError, match="mesh"):
        reconstruct_scan(model, images, poses, intr, TR.NAMES, TR.PAIRS, scales, None, write=False, mesh={"colours": True}, **kw)
