"""Surface normals on the MI355X (csrc/cloud_eval.hip grid_normals_kernel, cer-mvs_amd/cloud_eval.py CloudIndex.normals / estimate_normals,
scan.reconstruct_scan(normals=...)) against the numpy fp64 restatement of tests/normals_reference.py.  The bars:

* ``count`` equal to ``knn``'s and ``mom`` bit-equal to the oracle's (the same additions in the same order, no contraction);
* validity equal to the oracle's - after asserting that no oracle l1 / l2 lies within a factor 10 of the degeneracy bar 1e-12;
* normals against ``numpy.linalg.eigh`` on the valid rows whose oracle gap g = (l1 - l0) / l2 is at least 1e-3 (at most 1 % of the valid rows
  may be left out): after sign alignment every component within 2^-23.  Two fp64 unit eigenvectors differ by an angle of at most
  64 * 2^-52 / g <= 1.5e-11 (the perturbation bound with a backward error of a few dozen eps |C| for Jacobi and LAPACK alike); each is then
  rounded once to float32, whose spacing below 1 is 2^-24; 2^-23 is that spacing with a factor 2;
* curvature at most one float32 step from the oracle's, or within 1e-13, on the same rows."""
import numpy as np
import pytest
import torch

import knn_reference as R
import normals_reference as NR

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, F32).reshape(-1, 3)).to(dev)


def make_index(dev, target, cell):
    from cer_mvs_amd.cloud_eval import CloudIndex
    return CloudIndex(on(dev, target), cell)


def device_normals(index, dev, queries, k, max_dist, viewpoints=None, **kw):
    """-> {"normal", "curvature", "count", "mom"} as numpy; the three-value form must return the four-value form's bytes"""
    q = on(dev, queries)
    vp = None if viewpoints is None else torch.from_numpy(np.ascontiguousarray(viewpoints, F32)).to(dev)
    normal, curv, count, mom = index.normals(q, k, max_dist, viewpoints=vp, moments=True, **kw)
    three = index.normals(q, k, max_dist, viewpoints=vp, **kw)
    m = len(q)
    assert normal.dtype == torch.float32 and curv.dtype == torch.float32 and count.dtype == torch.int32 and mom.dtype == torch.float64
    assert tuple(normal.shape) == (m, 3) and tuple(curv.shape) == (m,) and tuple(count.shape) == (m,) and tuple(mom.shape) == (m, 9)
    got = {"normal": normal.cpu().numpy(), "curvature": curv.cpu().numpy(), "count": count.cpu().numpy(), "mom": mom.cpu().numpy()}
    assert len(three) == 3 and all(t.cpu().numpy().tobytes() == got[key].tobytes() for t, key in zip(three, ("normal", "curvature", "count")))
    assert np.array_equal(count.cpu().numpy(), index.knn(q, k, max_dist, **kw)[2].cpu().numpy())
    return got


def same_bytes(a, b):
    return all(a[key].tobytes() == b[key].tobytes() for key in ("normal", "curvature", "count", "mom"))


def gap_of(want):
    lam = want["lam"]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (lam[:, 1] - lam[:, 0]) / lam[:, 2]


def compare(got, want, what, max_left_out=None):
    """the bars of the module docstring; -> the rows compared"""
    lam = want["lam"]
    with np.errstate(invalid="ignore", divide="ignore"):
        rows = (want["count"] >= 3) & (lam[:, 2] > 0) & (lam[:, 1] != 0)
        ratio = lam[:, 1] / lam[:, 2]
    near = rows & (ratio > 0.1 * NR.NORMAL_DEGENERATE) & (ratio < 10 * NR.NORMAL_DEGENERATE)
    valid = ~np.isnan(got["curvature"])
    mom_bits = int((got["mom"].view(np.uint64) != want["mom"].view(np.uint64)).sum())
    gap = gap_of(want)
    cmp_rows = want["valid"] & (gap >= 1e-3)
    left_out = int(want["valid"].sum() - cmp_rows.sum())
    gn, wn = got["normal"][cmp_rows].astype(np.float64), want["normal"][cmp_rows].astype(np.float64)
    sign = np.where((gn * wn).sum(1) < 0, -1.0, 1.0)[:, None]
    ndiff = np.abs(gn * sign - wn).max() if len(gn) else 0.0
    gc, wc = got["curvature"][cmp_rows], want["curvature"][cmp_rows]
    cdiff = np.abs(gc.astype(np.float64) - wc.astype(np.float64))
    step = np.spacing(np.maximum(np.abs(gc), np.abs(wc))).astype(np.float64)
    cbad = int(((cdiff > step) & (cdiff > 1e-13)).sum()) if len(gc) else 0
    print(f"cloud_normals {what}: rows = {len(valid)}, valid = {int(want['valid'].sum())}, count differing = {int((got['count'] != want['count']).sum())}, "
          f"mom bits differing = {mom_bits}, validity differing = {int((valid != want['valid']).sum())}, near the bar = {int(near.sum())}, "
          f"left out for a small gap = {left_out}, smallest gap compared = {gap[cmp_rows].min() if cmp_rows.any() else NAN:.3g}, "
          f"normal max diff = {ndiff / 2.0 ** -23:.3g} x 2^-23, curvature max diff = {cdiff.max() if len(cdiff) else 0.0:.3g}, beyond its bar = {cbad}")
    assert np.array_equal(got["count"], want["count"])
    assert mom_bits == 0
    assert not near.any()
    assert np.array_equal(valid, want["valid"])
    assert not got["normal"][~valid].any() and np.array_equal(valid, np.abs(np.linalg.norm(got["normal"].astype(np.float64), axis=1) - 1) < 1e-6)
    assert left_out <= (0.01 * want["valid"].sum() if max_left_out is None else max_left_out)
    assert ndiff <= 2.0 ** -23
    assert cbad == 0
    return cmp_rows


def leads_positive(normal, valid):
    """canonical sign, read off the float32 normal: a component within 2^-23 of the largest magnitude is positive (the fp64 leader is one of them)"""
    n = normal[valid].astype(np.float64)
    top = np.abs(n) >= np.abs(n).max(1, keepdims=True) - 2.0 ** -23
    return (np.where(top, n, -1.0).max(1) > 0).all()


@pytest.fixture(scope="module")
def surface():
    pts, planted = R.wavy_surface()
    return {"pts": pts, "planted": planted, "sorted": R.sorted_neighbours(pts, pts, 20)}


@pytest.fixture(scope="module")
def cube():
    t, q = R.random_pair()
    return {"t": t, "q": q, "self": R.sorted_neighbours(t, t, R.KNN_MAX), "pair": R.sorted_neighbours(t, q, 16)}


# ---------------------------------------------------------------- 1. count, moments, validity, normals and curvature against the oracle
@pytest.mark.parametrize("k", [8, 20])
def test_wavy_surface_on_itself(dev, surface, k):
    pts, planted = surface["pts"], surface["planted"]
    want = NR.normals(pts, pts, k, R.FILTER_MAX_DIST, sorted_pairs=surface["sorted"])
    index = make_index(dev, pts, R.FILTER_MAX_DIST / 4)
    got = device_normals(index, dev, pts, k, R.FILTER_MAX_DIST)
    compare(got, want, f"wavy surface k={k}", max_left_out=0)
    assert want["valid"].sum() == 4000
    assert (got["count"][planted] == 1).all() and not got["normal"][planted].any() and np.isnan(got["curvature"][planted]).all()
    assert leads_positive(got["normal"], want["valid"])      # no viewpoints: the canonical sign
    if k == 20:                                              # a guard against a transposed axis, not a precision bar (the oracle: 0.28 degrees)
        v = want["valid"]
        n = got["normal"][v].astype(np.float64)
        cos = np.abs((n * NR.wavy_normal(pts[v, :2].astype(np.float64))).sum(1))
        angle = np.degrees(np.median(np.arccos(np.clip(cos, -1, 1))))
        print(f"cloud_normals wavy surface k=20: median angle to the analytic normal = {angle:.3f} degrees")
        assert angle < 1.0


@pytest.mark.parametrize("k", [16, 5, 9, 17, 32])
def test_cube_targets_on_themselves(dev, cube, k):
    """both sides of the 8 / 16 / 32 dispatch, runtime k below the list's width; 1000 of the targets in one dense box"""
    t = cube["t"]
    want = NR.normals(t, t, k, 0.1, sorted_pairs=cube["self"])
    got = device_normals(make_index(dev, t, 0.05), dev, t, k, 0.1)
    compare(got, want, f"cube on itself k={k}")
    assert (want["count"] == k).any() and leads_positive(got["normal"], want["valid"])


def test_full_partly_filled_and_empty_rows(dev, cube):
    t, q = cube["t"], cube["q"]
    want = NR.normals(t, q, 16, 0.05, sorted_pairs=cube["pair"])
    assert (want["count"] == 16).any() and ((want["count"] >= 3) & (want["count"] < 16)).any() and (want["count"] == 0).any()
    assert ((want["count"] > 0) & (want["count"] < 3)).any() and want["valid"].any() and not want["valid"].all()
    index = make_index(dev, t, 0.05)
    got = device_normals(index, dev, q, 16, 0.05)
    compare(got, want, "5000 x 3000 at one ring, k=16")
    assert not got["mom"][want["count"] == 0].any()
    # two runs, permuted queries, unsorted walk: the same bytes
    assert same_bytes(got, device_normals(index, dev, q, 16, 0.05))
    assert same_bytes(got, device_normals(index, dev, q, 16, 0.05, sort_queries=False))
    perm = np.random.default_rng(3).permutation(len(q))
    moved = device_normals(index, dev, q[perm], 16, 0.05)
    assert all(got[key][perm].tobytes() == moved[key].tobytes() for key in got)


# ---------------------------------------------------------------- 2. exact cases
@pytest.mark.parametrize("k", [5, 9])
def test_lattice_normals_are_exactly_z(dev, k):
    """the planar lattice on itself: zz, xz and yz are exactly 0, so no rotation touches z; every valid normal is exactly (0, 0, 1)"""
    pts = R.lattice()
    want = NR.normals(pts, pts, k, 0.2)
    got = device_normals(make_index(dev, pts, 0.1), dev, pts, k, 0.2)
    assert np.array_equal(got["count"], want["count"]) and got["mom"].tobytes() == want["mom"].tobytes()
    valid = ~np.isnan(got["curvature"])
    assert np.array_equal(valid, want["valid"]) and valid.all()
    assert not got["mom"][:, [2, 5, 7, 8]].any()
    assert (got["normal"] == np.array([0, 0, 1], F32)).all() and (got["curvature"] == 0).all()
    down = device_normals(make_index(dev, pts, 0.1), dev, pts, k, 0.2, viewpoints=np.array([0.3, -0.2, -4.0], F32))
    assert (down["normal"] == np.array([0, 0, -1], F32)).all() and (down["curvature"] == 0).all()


@pytest.mark.parametrize("n", [1, 2])
def test_fewer_than_three_points(dev, n):
    pts = R.cube(n, 30 + n)
    got = device_normals(make_index(dev, pts, 0.5), dev, pts, 8, 4.0)
    want = NR.normals(pts, pts, 8, 4.0)
    assert (got["count"] == n).all() and not got["normal"].any() and np.isnan(got["curvature"]).all()
    assert got["mom"].tobytes() == want["mom"].tobytes()


def test_every_point_three_times(dev):
    """k = 4: the three copies and one more point - two distinct positions, a collinear neighbourhood: invalid, by l1 (a rounding error beside
    l2) far below the bar; k = 12 on the same cloud finds planes"""
    g = np.random.default_rng(7)
    base = R.cube(1500, 4)
    t = np.concatenate([base, base, base])[g.permutation(4500)]
    pairs = R.sorted_neighbours(t, t, 12)
    index = make_index(dev, t, 0.05)
    want = NR.normals(t, t, 4, 0.08, sorted_pairs=pairs)
    got = device_normals(index, dev, t, 4, 0.08)
    compare(got, want, "every point three times, k=4")
    assert (want["count"] >= 3).all() and not want["valid"].any() and not got["normal"].any()
    want = NR.normals(t, t, 12, 0.08, sorted_pairs=pairs)
    compare(device_normals(index, dev, t, 12, 0.08), want, "every point three times, k=12")
    assert want["valid"].sum() > 1000


def test_collinear_points_are_invalid(dev):
    on_axis = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F32)
    diagonal = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 5, 5]], F32)
    plane = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], F32)      # the fourth point off the line: valid, normal z
    for pts, k, valid in ((on_axis, 3, False), (on_axis, 8, False), (diagonal, 4, False), (plane, 4, True)):
        want = NR.normals(pts, pts, k, 20.0)
        got = device_normals(make_index(dev, pts, 1.0), dev, pts, k, 20.0)
        compare(got, want, f"collinear {len(pts)} points k={k}")
        assert (got["count"] == len(pts)).all() and want["valid"].all() == valid and want["valid"].any() == valid
    assert (got["normal"] == np.array([0, 0, 1], F32)).all() and (got["curvature"] == 0).all()


def test_non_finite_queries_targets_and_viewpoints(dev):
    t, q = R.cube(3000, 14), R.cube(600, 15)
    rows = ([NAN, 0.5, 0.5], [0.5, INF, 0.5], [0.5, 0.5, -INF], [NAN, NAN, NAN], [INF, -INF, NAN])
    for j, row in enumerate(rows):
        t[37 * j + 5] = row
        q[29 * j + 3] = row
    q[200] = t[5 + 37]
    vp = np.tile(np.array([[0.5, 0.5, 7.0]], F32), (len(q), 1))
    for j, row in enumerate(rows):
        vp[41 * j + 7] = row
    want = NR.normals(t, q, 10, 0.15, viewpoints=vp)
    index = make_index(dev, t, 0.05)
    assert index.n == 2995
    got = device_normals(index, dev, q, 10, 0.15, viewpoints=vp)
    rows_cmp = compare(got, want, "non-finite")
    bad = [29 * j + 3 for j in range(5)] + [200]
    assert not got["count"][bad].any() and not got["mom"][bad].any() and not got["normal"][bad].any() and np.isnan(got["curvature"][bad]).all()
    plain = device_normals(index, dev, q, 10, 0.15)
    odd = np.array([41 * j + 7 for j in range(5)])
    assert want["valid"][odd].all() and plain["normal"][odd].tobytes() == got["normal"][odd].tobytes()      # the canonical sign stays
    seen = want["valid"].copy()
    seen[odd] = False
    v = vp[seen].astype(np.float64) - q[seen].astype(np.float64)
    s = (got["normal"][seen].astype(np.float64) * v).sum(1)
    assert (s > -1e-6 * np.linalg.norm(v, axis=1)).all() and rows_cmp.sum() > 500
    assert plain["mom"].tobytes() == got["mom"].tobytes() and plain["curvature"].tobytes() == got["curvature"].tobytes()
    assert np.array_equal(np.abs(plain["normal"]), np.abs(got["normal"]))


# ---------------------------------------------------------------- 3. orientation
def test_orientation_towards_viewpoints(dev, surface):
    pts = surface["pts"]
    index = make_index(dev, pts, R.FILTER_MAX_DIST / 4)
    plain = device_normals(index, dev, pts, 20, R.FILTER_MAX_DIST)
    for what, vp, up in (("one viewpoint above", np.array([0.5, 0.5, 10.0], F32), True),
                         ("a viewpoint below every point", (pts.astype(np.float64) - np.array([0.0, 0.0, 1.0])).astype(F32), False)):
        want = NR.normals(pts, pts, 20, R.FILTER_MAX_DIST, viewpoints=vp, sorted_pairs=surface["sorted"])
        got = device_normals(index, dev, pts, 20, R.FILTER_MAX_DIST, viewpoints=vp)
        compare(got, want, f"wavy surface, {what}", max_left_out=0)
        v = want["valid"]
        assert v.sum() == 4000 and ((got["normal"][v, 2] > 0) if up else (got["normal"][v, 2] < 0)).all()
        with np.errstate(invalid="ignore"):
            clear = v & (np.abs(want["s"]) >= 1e-9 * want["vnorm"])
        assert clear.sum() == v.sum()                        # the oracle leaves none out on these inputs (at most 1 % may be)
        assert ((got["normal"][clear].astype(np.float64) * want["normal"][clear].astype(np.float64)).sum(1) > 0).all()
        # the viewpoint turns a normal or leaves it: everything else is the run without viewpoints
        assert np.array_equal(np.abs(got["normal"]), np.abs(plain["normal"])) and got["curvature"].tobytes() == plain["curvature"].tobytes()
        assert got["mom"].tobytes() == plain["mom"].tobytes() and got["count"].tobytes() == plain["count"].tobytes()
    one = torch.tensor([0.5, 0.5, 10.0], device=dev)         # a [3] viewpoint is expanded
    q = on(dev, pts)
    a = index.normals(q, 20, R.FILTER_MAX_DIST, viewpoints=one)
    b = index.normals(q, 20, R.FILTER_MAX_DIST, viewpoints=one[None].expand(len(pts), 3))
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    with pytest.raises(ValueError, match="viewpoints"):
        index.normals(q, 20, R.FILTER_MAX_DIST, viewpoints=torch.zeros(7, 3, device=dev))


# ---------------------------------------------------------------- 4. the Python layer
def test_empty_sides_and_reach(dev, surface):
    t = R.cube(100, 3)
    index = make_index(dev, t, 0.1)
    n, c, cnt, mom = index.normals(on(dev, np.zeros((0, 3), F32)), 5, 0.2, moments=True)
    assert tuple(n.shape) == (0, 3) and tuple(c.shape) == (0,) and tuple(cnt.shape) == (0,) and tuple(mom.shape) == (0, 9)
    empty = make_index(dev, np.zeros((0, 3), F32), 0.1)
    n, c, cnt, mom = empty.normals(on(dev, t), 5, 0.2, moments=True, viewpoints=torch.zeros(3, device=dev))
    assert n.dtype == torch.float32 and c.dtype == torch.float32 and cnt.dtype == torch.int32 and mom.dtype == torch.float64
    assert tuple(n.shape) == (100, 3) and not n.any() and bool(torch.isnan(c).all()) and not cnt.any() and not mom.any() and tuple(mom.shape) == (100, 9)
    with pytest.raises(ValueError, match="more than 4096 cells"):
        make_index(dev, surface["pts"], 1e-5).normals(on(dev, surface["pts"][:10]), 4, 0.06)


def test_estimate_normals_is_the_index_on_itself(dev, surface):
    from cer_mvs_amd.cloud_eval import CloudIndex, estimate_normals
    pts = on(dev, surface["pts"])
    vp = torch.tensor([0.5, 0.5, 10.0], device=dev)
    for kw, k, max_dist, cell in (({"k": 8, "max_dist": R.FILTER_MAX_DIST}, 8, float(F32(R.FILTER_MAX_DIST)), float(F32(R.FILTER_MAX_DIST)) / 4),
                                  ({"max_dist": R.FILTER_MAX_DIST, "cell": 0.05, "viewpoints": vp}, 20, float(F32(R.FILTER_MAX_DIST)), 0.05)):
        info = {}
        normal, curv = estimate_normals(pts, info=info, **kw)
        n2, c2, _ = CloudIndex(pts, cell).normals(pts, k, max_dist, viewpoints=kw.get("viewpoints"))
        assert normal.cpu().numpy().tobytes() == n2.cpu().numpy().tobytes() and curv.cpu().numpy().tobytes() == c2.cpu().numpy().tobytes()
        assert info == {"n_valid": 4000, "max_dist": max_dist, "cell": cell, "k": k}
    info = {}
    normal, curv = estimate_normals(pts, info=info)          # the defaults: k = 20, 1 % of the bounding-box diagonal, a quarter of it
    P = surface["pts"].astype(np.float64)
    want_dist = float(F32(0.01 * np.sqrt(((P.max(0) - P.min(0)) ** 2).sum())))
    assert set(info) == {"n_valid", "max_dist", "cell", "k"} and info["k"] == 20 and abs(info["max_dist"] - want_dist) <= 2e-7 * want_dist
    assert info["cell"] == info["max_dist"] / 4 and info["n_valid"] == int((~torch.isnan(curv)).sum()) and tuple(normal.shape) == (4040, 3)
    normal, curv = estimate_normals(torch.zeros(0, 3, device=dev), info=info)
    assert tuple(normal.shape) == (0, 3) and tuple(curv.shape) == (0,) and info["n_valid"] == 0


# ---------------------------------------------------------------- 5. end to end
def test_reconstruct_scan_with_and_without_normals(dev, tmp_path):
    """the small synthetic scan of the clean tests.  normals=None: today's keys, a second call's bytes.  With normals: estimate_normals on the
    cloud that leaves, every point turned towards the centre of the camera that produced it (the views read off the masks: the cloud is
    emitted view by view), result.ply carries them; with clean: the views go through the kept indices"""
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd.scan import reconstruct_scan
    from test_reconstruct_gpu import NAMES, NF, PAIRS, _model, _scan
    images, poses, intr, scales = _scan(128, 160)
    model = _model(dev)
    run = lambda **kw: reconstruct_scan(model, images, poses, intr, NAMES, PAIRS, scales, tmp_path, num_frames=NF, streams=2, **kw)
    plain, again = run(write=False), run(write=False, normals=None)
    assert set(plain) == set(again) == {"masks", "depth_est", "xyz", "rgb", "threshold", "history"}
    for key in ("masks", "depth_est", "xyz", "rgb"):
        assert plain[key].tobytes() == again[key].tobytes() and plain[key].dtype == again[key].dtype
    xyz = np.ascontiguousarray(plain["xyz"], F32)
    extent = float((xyz.max(0) - xyz.min(0)).max())
    reach = float(F32(0.05 * extent))                        # the cloud is sparse: a few points per 1 % of the extent
    centres = np.stack([np.linalg.inv(E)[:3, 3] for E in np.asarray(poses, F32)]).astype(F32)      # inv(E)[:3, 3] of the float32 pose
    view = np.repeat(np.arange(len(plain["masks"])), plain["masks"].reshape(len(plain["masks"]), -1).sum(1))
    assert len(view) == len(xyz) and len(np.unique(view)) > 1

    def check(out, pts, views, opts):
        info = {}
        vp = torch.from_numpy(centres[views]).to(dev)
        want, _ = CE.estimate_normals(torch.from_numpy(pts).to(dev), viewpoints=vp, info=info, **opts)
        assert out["normals"].dtype == F32 and out["normals"].shape == pts.shape and out["normals"].tobytes() == want.cpu().numpy().tobytes()
        assert out["normal_info"] == info and set(info) == {"n_valid", "max_dist", "cell", "k"}
        valid = np.abs(np.linalg.norm(out["normals"].astype(np.float64), axis=1) - 1) < 1e-6
        assert valid.sum() == info["n_valid"] and not out["normals"][~valid].any()
        s = (out["normals"][valid].astype(np.float64) * (centres[views][valid].astype(np.float64) - pts[valid].astype(np.float64))).sum(1)
        print(f"reconstruct_scan normals {opts}: {len(pts)} points, {int(valid.sum())} valid, min n . (c - p) = {s.min() if len(s) else NAN:.3g}")
        assert (s >= 0).all()
        return valid

    opts = {"k": 12, "max_dist": reach}
    out = run(write=True, normals=opts)
    assert set(out) == set(plain) | {"normals", "normal_info"}
    for key in ("masks", "depth_est", "xyz", "rgb"):
        assert out[key].tobytes() == plain[key].tobytes()
    assert check(out, xyz, view, opts).sum() > 100
    x, c, n = CE.read_ply(str(tmp_path / "result.ply"), normals=True)
    assert x.tobytes() == xyz.tobytes() and c.tobytes() == np.ascontiguousarray(plain["rgb"]).tobytes() and n.tobytes() == out["normals"].tobytes()
    # normals=True: the defaults (k = 20, 1 % of the bounding-box diagonal), after a radius filter: the views are selected through kept
    radius = float(F32(0.01 * extent))
    cloud = torch.from_numpy(xyz).to(dev)
    bar = int(np.median(CE.CloudIndex(cloud, radius / 4).count_within(cloud, radius).cpu().numpy()))
    clean = {"method": "radius", "radius": radius, "min_neighbours": bar}
    keep = CE.remove_radius_outliers(cloud, radius, bar).cpu().numpy()
    both = run(write=False, clean=clean, normals=True)
    assert set(both) == set(plain) | {"clean", "normals", "normal_info"} and 0 < len(keep) < len(xyz)
    assert both["xyz"].tobytes() == xyz[keep].tobytes() and both["normals"].shape == both["xyz"].shape
    check(both, xyz[keep], view[keep], {})
    with pytest.raises(ValueError, match="normals"):
        run(write=False, normals={"radius": 0.1})
