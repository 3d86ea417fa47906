"""k nearest neighbours, the count within a radius and the outlier filters on the MI355X (csrc/cloud_eval.hip grid_knn_kernel /
grid_count_within_kernel, cer-mvs_amd/cloud_eval.py) against the numpy fp64 brute force of tests/knn_reference.py.  The bars:
``idx`` and ``count`` equal, ``dist`` bit-equal (the kernel's fp64 square root is the correctly rounded one), ``mean`` bit-equal (the same
additions in the same order and one division), counts equal.  The one tolerance is 1e-12 relative on the filter's mu, sigma and threshold:
two fp64 summation orders over a few thousand terms."""
import numpy as np
import pytest
import torch

import knn_reference as R

pytestmark = pytest.mark.gpu

F32 = np.float32
WIDTHS = (1, 5, 8, 9, 16, 17, 20, 32)                        # both sides of the 8 / 16 / 32 dispatch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, F32).reshape(-1, 3)).to(dev)


def make_index(dev, target, cell):
    from cer_mvs_amd.cloud_eval import CloudIndex
    return CloudIndex(on(dev, target), cell)


def device_knn(index, dev, queries, k, max_dist, **kw):
    """-> (dist, idx, count, mean) as numpy; the mean comes from knn_mean_distance, whose count must be knn's"""
    q = on(dev, queries)
    dist, idx, count = index.knn(q, k, max_dist, **kw)
    mean, count2 = index.knn_mean_distance(q, k, max_dist, **kw)
    m = len(q)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and count.dtype == torch.int32 and mean.dtype == torch.float64
    assert tuple(dist.shape) == (m, k) and tuple(idx.shape) == (m, k) and tuple(count.shape) == (m,) and tuple(mean.shape) == (m,)
    assert torch.equal(count, count2)
    return dist.cpu().numpy(), idx.cpu().numpy(), count.cpu().numpy(), mean.cpu().numpy()


def same(got, want, what=""):
    (gd, gi, gc, gm), (wd, wi, wc, wm) = got, want
    print(f"cloud_knn {what}: rows = {len(wc)}, full = {int((wc == wd.shape[1]).sum())}, empty = {int((wc == 0).sum())}, "
          f"idx differing = {int((gi != wi).sum())}, dist bits differing = {int((gd.view(np.uint32) != wd.view(np.uint32)).sum())}, "
          f"count differing = {int((gc != wc).sum())}, mean bits differing = {int((gm.view(np.uint64) != wm.view(np.uint64)).sum())}")
    assert np.array_equal(gi, wi)
    assert np.array_equal(gc, wc)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))
    assert np.array_equal(gm.view(np.uint64), wm.view(np.uint64))


def check(dev, target, queries, cell, k, max_dist, what="", **kw):
    want = R.knn(target, queries, k, max_dist)
    index = make_index(dev, target, cell)
    same(device_knn(index, dev, queries, k, max_dist, **kw), want, what)
    return want, index


@pytest.fixture(scope="module")
def random_pair():
    """n = 5000 targets and m = 3000 queries in the unit cube with their 32 nearest of the whole target, sorted (computed once).  A fifth of
    the targets and a tenth of the queries lie in one box of edge 0.08: at a uniform density no query would have 16 targets within 0.05, and
    the full rows at the short cut-off would not occur"""
    t, q = R.random_pair()
    return {"t": t, "q": q, "sorted": R.sorted_neighbours(t, q, R.KNN_MAX)}


# ---------------------------------------------------------------- 1. every list width and its edges
@pytest.mark.parametrize("k", WIDTHS)
def test_every_list_width(dev, random_pair, k):
    t, q = random_pair["t"], random_pair["q"]
    want = R.knn_from_sorted(*random_pair["sorted"], k, 0.12)
    index = make_index(dev, t, 0.05)
    got = device_knn(index, dev, q, k, 0.12)
    same(got, want, f"k={k}")
    assert (want[2] == k).any()
    if k == 1:                                               # ... and nearest itself, bytes for bytes
        d1, i1 = index.nearest(on(dev, q), 0.12)
        assert d1.cpu().numpy().tobytes() == got[0].tobytes() and i1.cpu().numpy().tobytes() == got[1].tobytes()


def test_full_partly_filled_and_empty_rows(dev, random_pair):
    want = R.knn_from_sorted(*random_pair["sorted"], 16, 0.05)
    assert (want[2] == 16).any() and ((want[2] > 0) & (want[2] < 16)).any() and (want[2] == 0).any()
    index = make_index(dev, random_pair["t"], 0.05)
    same(device_knn(index, dev, random_pair["q"], 16, 0.05), want, "k=16 at one ring")


# ---------------------------------------------------------------- 2. sizes off the wave and block multiples
@pytest.mark.parametrize("n", [1, 63, 257, 4097])
@pytest.mark.parametrize("m", [1, 65, 1025])
def test_sizes_off_the_wave_and_block_multiples(dev, n, m):
    t, q = R.cube(n, 10 + n), R.cube(m, 20 + m)
    want, index = check(dev, t, q, 0.05, 8, 2.0, f"sizes n={n} m={m}")      # max_dist covers the cube: every target is a candidate
    if n < 8:
        assert (want[2] == n).all()
    assert np.array_equal(index.count_within(on(dev, q), 0.1).cpu().numpy(), R.count_within(t, q, 0.1))
    assert np.array_equal(index.count_within(on(dev, q), 2.0).cpu().numpy(), np.full(m, n))


def test_empty_sides(dev):
    t = R.cube(100, 3)
    index = make_index(dev, t, 0.1)
    d, i, c, mean = device_knn(index, dev, np.zeros((0, 3), F32), 5, 0.2)
    assert d.shape == (0, 5) and i.shape == (0, 5) and c.shape == (0,) and mean.shape == (0,)
    assert index.count_within(on(dev, np.zeros((0, 3), F32)), 0.2).shape == (0,)
    empty = make_index(dev, np.zeros((0, 3), F32), 0.1)
    d, i, c, mean = device_knn(empty, dev, t, 5, 0.2)
    assert np.isposinf(d).all() and (i == -1).all() and not c.any() and np.isposinf(mean).all() and d.shape == (100, 5)
    cw = empty.count_within(on(dev, t), 0.2)
    assert cw.dtype == torch.int32 and tuple(cw.shape) == (100,) and not cw.any()


# ---------------------------------------------------------------- 3. ties
def test_duplicates_give_the_lowest_indices(dev):
    g = np.random.default_rng(7)
    base = R.cube(1500, 4)
    t = np.concatenate([base, base, base])[g.permutation(4500)]
    q = np.concatenate([base[:700], R.cube(800, 5)])
    want, _ = check(dev, t, q, 0.05, 4, 0.08, "every point three times")
    assert (want[0][:700, :3] == 0).all() and (want[2][:700] >= 3).all()
    for k in (0, 1, 350, 699):                               # the three copies, ascending, then the next point
        copies = np.flatnonzero((t == base[k]).all(1))
        assert len(copies) == 3 and want[1][k, :3].tolist() == sorted(copies.tolist())


@pytest.mark.parametrize("k", [3, 5])
def test_lattice_cuts_through_equidistant_neighbours(dev, k):
    """the planar lattice on itself: every coordinate on (or an ulp beside) a cell face; around the origin (node 840 = 41 * 20 + 20) the four
    neighbours 799, 839, 841, 881 are exactly 0.1f away: k = 3 takes the two lowest indices of them"""
    pts = R.lattice()
    want, _ = check(dev, pts, pts, 0.1, k, 0.2, f"lattice on itself, k={k}")
    assert want[1][840].tolist() == [840, 799, 839, 841, 881][:k] and want[0][840, 1] == want[0][840, k - 1] == F32(0.1)


def test_cut_off_is_inclusive_in_fp64(dev):
    q = np.zeros((1, 3), F32)
    at = np.array([[0.5, 0, 0]], F32)
    beyond = np.array([[np.nextafter(F32(0.5), F32(1)), 0, 0]], F32)
    for cell in (0.5, 0.3, 0.125, 0.07):
        want, index = check(dev, np.concatenate([beyond, at]), q, cell, 2, 0.5, f"cut-off cell={cell}")
        assert want[1][0].tolist() == [1, -1] and want[0][0, 0] == F32(0.5) and want[2][0] == 1 and want[3][0] == 0.5
        assert index.count_within(on(dev, q), 0.5).tolist() == [1]
    d, i, c, mean = device_knn(make_index(dev, at, 0.125), dev, at, 3, 0.0)      # max_dist = 0: a coincident point is found
    assert i[0].tolist() == [0, -1, -1] and d[0, 0] == 0 and c[0] == 1 and mean[0] == 0.0


# ---------------------------------------------------------------- 4. geometry
def test_queries_outside_the_bounding_box(dev):
    t = R.cube(2000, 6)
    g = np.random.default_rng(8)
    q = []
    for axis in range(3):
        for side in (0, 1):
            for off in (0.03, 0.08, 0.25, 40.0, 3e6):        # less than and more than max_dist = 0.1; far beyond the key range
                p = g.random((40, 3)).astype(F32)
                p[:, axis] = -off if side == 0 else 1.0 + off
                q.append(p)
    q = np.concatenate(q).astype(F32)
    want, index = check(dev, t, q, 0.025, 6, 0.1, "outside the box")
    assert (want[2] > 0).any() and (want[2] == 0).sum() > 600
    assert np.array_equal(index.count_within(on(dev, q), 0.1).cpu().numpy(), R.count_within(t, q, 0.1))


def test_one_dense_cell(dev):
    g = np.random.default_rng(9)
    dense = (0.5001 + 0.0998 * g.random((3000, 3))).astype(F32)                 # all inside the cell [0.5, 0.6)^3 of the grid below
    sparse = R.cube(2000, 12)
    sparse[0] = 0.0                                                          # pins the grid's origin
    t = np.concatenate([sparse, dense])[g.permutation(5000)]
    q = np.concatenate([(0.5 + 0.1 * g.random((600, 3))), (0.35 + 0.4 * g.random((900, 3))), R.cube(500, 13)]).astype(F32)
    pairs = R.sorted_neighbours(t, q, 32)
    index = make_index(dev, t, 0.1)
    assert np.diff(index.cell_start.cpu().numpy()).max() >= 3000 and index.n == 5000
    for max_dist in (0.1, 0.25):                             # one ring and three
        same(device_knn(index, dev, q, 32, max_dist), R.knn_from_sorted(*pairs, 32, max_dist), f"dense cell, max_dist={max_dist}")
    assert np.array_equal(index.count_within(on(dev, q), 0.1).cpu().numpy(), R.count_within(t, q, 0.1))


def test_non_finite_points_and_queries(dev):
    t, q = R.cube(1000, 14), R.cube(600, 15)
    for k, row in enumerate(([np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.nan])):
        t[37 * k + 5] = row
        q[29 * k + 3] = row
    q[200] = t[5 + 37]                                       # a query equal to a non-finite target
    want, index = check(dev, t, q, 0.05, 10, 0.15, "non-finite")
    assert index.n == 995
    bad = [29 * k + 3 for k in range(5)] + [200]
    assert (want[2][bad] == 0).all() and not np.isin(want[1], [37 * k + 5 for k in range(5)]).any()
    got = index.count_within(on(dev, q), 0.15).cpu().numpy()
    assert np.array_equal(got, R.count_within(t, q, 0.15)) and (got[bad] == 0).all()


# ---------------------------------------------------------------- 5. determinism
def test_determinism_and_permutations(dev):
    g = np.random.default_rng(16)
    t, q = R.cube(4000, 17), R.cube(2500, 18)
    assert len(np.unique(t, axis=0)) == len(t)               # duplicate-free: idx maps through a permutation of the targets
    index = make_index(dev, t, 0.04)
    a = device_knn(index, dev, q, 12, 0.1)
    b = device_knn(index, dev, q, 12, 0.1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = device_knn(index, dev, q, 12, 0.1, sort_queries=False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))
    pq = g.permutation(len(q))
    d = device_knn(index, dev, q[pq], 12, 0.1)
    assert all(x[pq].tobytes() == y.tobytes() for x, y in zip(a, d))
    pt = g.permutation(len(t))                               # new position j holds old point pt[j]
    e = device_knn(make_index(dev, t[pt], 0.04), dev, q, 12, 0.1)
    assert e[0].tobytes() == a[0].tobytes() and e[2].tobytes() == a[2].tobytes() and e[3].tobytes() == a[3].tobytes()
    assert np.array_equal(np.where(e[1] >= 0, pt[np.maximum(e[1], 0)], -1), a[1])
    cw = index.count_within(on(dev, q), 0.1).cpu().numpy()
    assert cw.tobytes() == index.count_within(on(dev, q), 0.1, sort_queries=False).cpu().numpy().tobytes()
    assert cw[pq].tobytes() == index.count_within(on(dev, q[pq]), 0.1).cpu().numpy().tobytes()


# ---------------------------------------------------------------- 6. count_within
@pytest.mark.parametrize("radius", [0.05, 0.12])
def test_count_within_on_the_random_pair(dev, random_pair, radius):
    t, q = random_pair["t"], random_pair["q"]
    want = R.count_within(t, q, radius)
    d2 = random_pair["sorted"][0]
    if (d2[:, -1] > R.limit_of(radius)).all():               # fewer than 32 inside everywhere: the sorted lists know the count too
        assert np.array_equal(want, (d2 <= R.limit_of(radius)).sum(1))
    got = make_index(dev, t, 0.05).count_within(on(dev, q), radius)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert want.max() > 1 and (want.min() == 0 or radius > 0.1)


def test_count_within_on_the_lattice_and_at_radius_zero(dev):
    """radius 0.1 on the lattice: the spacing 0.1f * k - 0.1f * (k - 1) falls on both sides of it from node to node"""
    pts = R.lattice()
    want = R.count_within(pts, pts, 0.1)
    inner = want.reshape(41, 41)[1:-1, 1:-1]
    assert inner.max() == 5 and inner.min() < 5              # both sides occur
    index = make_index(dev, pts, 0.1)
    assert np.array_equal(index.count_within(on(dev, pts), 0.1).cpu().numpy(), want)
    twice = np.concatenate([pts, pts[::-1], R.cube(50, 19, -2.0, 2.0)])          # radius 0: coincident points only
    q = np.concatenate([pts[::3], R.cube(50, 19, -2.0, 2.0), R.cube(50, 20, -2.0, 2.0)])
    want = R.count_within(twice, q, 0.0)
    assert set(want.tolist()) == {0, 1, 2}
    assert np.array_equal(make_index(dev, twice, 0.1).count_within(on(dev, q), 0.0).cpu().numpy(), want)


# ---------------------------------------------------------------- 7. the filters
@pytest.fixture(scope="module")
def surface():
    pts, planted = R.wavy_surface()
    return {"pts": pts, "planted": planted, "sorted": R.sorted_neighbours(pts, pts, 20)}


@pytest.mark.parametrize("k", [8, 20])
def test_statistical_outliers_equal_the_oracle(dev, surface, k):
    from cer_mvs_amd.cloud_eval import remove_statistical_outliers
    pts, planted = surface["pts"], surface["planted"]
    pairs = (surface["sorted"][0][:, :k], surface["sorted"][1][:, :k])
    want, ref = R.statistical_outliers(pts, k, 2.0, R.FILTER_MAX_DIST, pairs)
    thr = ref["threshold"]
    assert np.abs(ref["mean"][ref["valid"]] - thr).min() > 1e-9 * thr      # no mean at the threshold: the sets are comparable
    assert not np.isin(planted, want).any() and (ref["valid"] & ~np.isin(np.arange(len(pts)), want)).any() and 0 < len(want) < len(pts) - 40
    info = {}
    got = remove_statistical_outliers(on(dev, pts), k=k, std_ratio=2.0, max_dist=R.FILTER_MAX_DIST, info=info)
    assert got.dtype == torch.int64 and got.is_cuda
    print(f"statistical k={k}: kept {len(want)} of {len(pts)}, valid {ref['n_valid']}, mu {info['mu']!r} / {ref['mu']!r}, "
          f"sigma {info['sigma']!r} / {ref['sigma']!r}, threshold {info['threshold']!r} / {thr!r}")
    for key in ("mu", "sigma", "threshold"):
        assert abs(info[key] - ref[key]) <= 1e-12 * abs(ref[key]), key
    assert info["n_valid"] == ref["n_valid"] and info["n_kept"] == len(want)
    assert info["max_dist"] == float(F32(R.FILTER_MAX_DIST)) and info["cell"] == info["max_dist"] / 4
    assert np.array_equal(got.cpu().numpy(), want)
    assert set(info) == {"mu", "sigma", "threshold", "n_valid", "n_kept", "max_dist", "cell"}


def test_statistical_outliers_default_scale_and_small_clouds(dev, surface):
    from cer_mvs_amd.cloud_eval import remove_statistical_outliers
    pts = surface["pts"]
    P = pts.astype(np.float64)
    info = {}
    got = remove_statistical_outliers(on(dev, pts), k=3, info=info)              # 1 % of the bounding-box diagonal, which the floaters widen
    want_dist = float(F32(0.01 * np.sqrt(((P.max(0) - P.min(0)) ** 2).sum())))
    assert abs(info["max_dist"] - want_dist) <= 2e-7 * want_dist                 # (the fp64 norm of a float32 extent, rounded once to float32)
    want, ref = R.statistical_outliers(pts, 3, 2.0, info["max_dist"])
    assert np.abs(ref["mean"][ref["valid"]] - ref["threshold"]).min() > 1e-9 * ref["threshold"] and 0 < len(want) < ref["n_valid"] < len(pts)
    assert np.array_equal(got.cpu().numpy(), want)
    one = np.array([[0.5, 0.5, 0.5], [np.nan, 0, 0]], F32)                       # fewer than 2 valid points: every valid point is kept
    assert remove_statistical_outliers(on(dev, one), k=1, max_dist=0.1).tolist() == [0]
    assert remove_statistical_outliers(on(dev, one), k=2, max_dist=0.1).tolist() == []
    assert remove_statistical_outliers(torch.zeros(0, 3, device=dev)).shape == (0,)


def test_radius_outliers_equal_the_oracle(dev, surface):
    from cer_mvs_amd.cloud_eval import remove_radius_outliers
    pts, planted = surface["pts"], surface["planted"]
    want = R.radius_outliers(pts, R.FILTER_RADIUS, R.FILTER_MIN_NEIGHBOURS)
    assert not np.isin(planted, want).any() and 0 < len(want) < len(pts) - 40    # kept and dropped surface points
    got = remove_radius_outliers(on(dev, pts), R.FILTER_RADIUS, R.FILTER_MIN_NEIGHBOURS)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(remove_radius_outliers(on(dev, pts), R.FILTER_RADIUS, R.FILTER_MIN_NEIGHBOURS, cell=0.05).cpu().numpy(), want)
    assert remove_radius_outliers(on(dev, pts), R.FILTER_RADIUS, 0).shape == (len(pts),)      # the point counts itself
    assert remove_radius_outliers(torch.zeros(0, 3, device=dev), 0.1, 2).shape == (0,)


def test_reach_beyond_the_rings_is_refused(dev, surface):
    index = make_index(dev, surface["pts"], 1e-5)
    q = on(dev, surface["pts"][:10])
    with pytest.raises(ValueError, match="more than 4096 cells"):
        index.knn(q, 4, 0.06)
    with pytest.raises(ValueError, match="more than 4096 cells"):
        index.count_within(q, 0.06)


# ---------------------------------------------------------------- 8. end to end
def test_reconstruct_scan_with_and_without_clean(dev):
    """the smallest scan tests/test_reconstruct_gpu.py builds.  clean=None: the dictionary of today, the bytes of a second plain call.
    clean by radius: xyz / rgb are the unfiltered arrays at remove_radius_outliers' indices; the radius is 1 % of the cloud's extent and the
    bar the median of the counts at that radius, so that points are kept and points are dropped"""
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd.scan import reconstruct_scan
    from test_reconstruct_gpu import NAMES, NF, PAIRS, _model, _scan
    images, poses, intr, scales = _scan(128, 160)
    model = _model(dev)
    run = lambda **kw: reconstruct_scan(model, images, poses, intr, NAMES, PAIRS, scales, None, num_frames=NF, streams=2, write=False, **kw)
    plain, again = run(), run(clean=None)
    assert set(plain) == set(again) == {"masks", "depth_est", "xyz", "rgb", "threshold", "history"}
    for key in ("masks", "depth_est", "xyz", "rgb"):
        assert plain[key].tobytes() == again[key].tobytes() and plain[key].dtype == again[key].dtype
    xyz = np.ascontiguousarray(plain["xyz"], F32)
    assert len(xyz) > 1000 and np.isfinite(xyz).all()
    extent = float((xyz.max(0) - xyz.min(0)).max())
    radius = float(F32(0.01 * extent))
    cloud = torch.from_numpy(xyz).to(dev)
    index = CE.CloudIndex(cloud, radius / 4)
    counts = index.count_within(cloud, radius).cpu().numpy()
    assert np.array_equal(counts[:4000], R.count_within(xyz, xyz[:4000], radius))      # the first 4000 points on the whole cloud
    bar = int(np.median(counts))
    keep = CE.remove_radius_outliers(cloud, radius, bar).cpu().numpy()
    assert np.array_equal(keep, np.flatnonzero(counts > bar))
    print(f"reconstructed cloud: {len(xyz)} points, extent {extent:.4f}, radius {radius:.5f}, counts {counts.min()} .. {counts.max()}, "
          f"bar {bar}, kept {len(keep)}")
    out = run(clean={"method": "radius", "radius": radius, "min_neighbours": bar})
    assert set(out) == set(plain) | {"clean"}
    assert out["xyz"].tobytes() == xyz[keep].tobytes() and out["rgb"].tobytes() == np.ascontiguousarray(plain["rgb"][keep]).tobytes()
    assert out["masks"].tobytes() == plain["masks"].tobytes() and out["depth_est"].tobytes() == plain["depth_est"].tobytes()
    c = out["clean"]
    assert c["method"] == "radius" and c["n_in"] == len(xyz) and c["n_kept"] == len(out["xyz"]) == len(keep) and 0 < c["n_kept"] < c["n_in"]
    assert c["radius"] == radius
    # ... and by the statistical filter: four neighbours within 5 % of the extent (the cloud is sparse: a few points per radius above)
    reach = float(F32(0.05 * extent))
    stat = run(clean={"method": "statistical", "k": 4, "max_dist": reach})
    c = stat["clean"]
    info = {}
    want = CE.remove_statistical_outliers(cloud, k=4, max_dist=reach, info=info).cpu().numpy()
    print(f"statistical: {c}")
    assert c["method"] == "statistical" and c["n_in"] == len(xyz) and c["n_kept"] == len(stat["xyz"]) == len(stat["rgb"]) == len(want)
    assert 2 <= c["n_valid"] and 0 < c["n_kept"] <= c["n_valid"] and c["max_dist"] == reach and c["threshold"] == c["mu"] + 2.0 * c["sigma"]
    assert stat["xyz"].tobytes() == xyz[want].tobytes() and stat["rgb"].tobytes() == np.ascontiguousarray(plain["rgb"][want]).tobytes()
    assert {k: c[k] for k in info} == info and set(c) == set(info) | {"method", "n_in"}
