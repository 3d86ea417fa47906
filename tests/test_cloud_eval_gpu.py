"""Cloud-to-cloud evaluation on the MI355X (csrc/cloud_eval.hip, cer-mvs_amd/cloud_eval.py) against a numpy fp64 brute force written here: the same
three operations for d2, the first minimum (the lowest index), the same <= test against double(max_dist)^2 and np.float32(np.sqrt(d2)).  The bar:
``idx`` equal everywhere, ``dist`` bit-equal (the kernel's fp64 square root is the correctly rounded one, so the two roundings - to fp64, then to
float32 - are the oracle's).

The issue's dense-cell case asks that 3000 points of one cell exceed the kernel's LDS chunk.  The search as built stages nothing in LDS (one thread
per query walks the sorted records of a row of cells directly: DESIGN.md 3u), so there is no chunk to exceed and no constant to assert against; the
case itself - 3000 points in one cell, 2000 sparse ones around it, queries in and beside the cell - is kept as stated."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


# ---------------------------------------------------------------- oracle
def oracle(target, queries, max_dist):
    """-> (dist float32 [m], idx int64 [m])"""
    T, Q = np.asarray(target, F32).astype(np.float64).reshape(-1, 3), np.asarray(queries, F32).astype(np.float64).reshape(-1, 3)
    m, limit = len(Q), np.float64(F32(max_dist)) * np.float64(F32(max_dist))
    dist, idx = np.full(m, np.inf, F32), np.full(m, -1, np.int64)
    if len(T) == 0:
        return dist, idx
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, m, 256):
            q = Q[s:s + 256]
            dx, dy, dz = T[None, :, 0] - q[:, None, 0], T[None, :, 1] - q[:, None, 1], T[None, :, 2] - q[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(np.isfinite(d2), d2, np.inf)               # a non-finite point or query: no neighbour
            j = np.argmin(d2, 1)                                     # the first minimum: the lowest index
            best = d2[np.arange(len(q)), j]
            ok = best <= limit
            dist[s:s + 256] = np.where(ok, np.sqrt(best).astype(F32), F32(np.inf))
            idx[s:s + 256] = np.where(ok, j, -1)
    return dist, idx


def device_nearest(dev, target, queries, cell, max_dist, **kw):
    from cer_mvs_amd.cloud_eval import CloudIndex
    index = CloudIndex(torch.from_numpy(np.ascontiguousarray(target, F32).reshape(-1, 3)).to(dev), cell)
    dist, idx = index.nearest(torch.from_numpy(np.ascontiguousarray(queries, F32).reshape(-1, 3)).to(dev), max_dist, **kw)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64
    return dist.cpu().numpy(), idx.cpu().numpy(), index


def check(dev, target, queries, cell, max_dist, what=""):
    want_d, want_i = oracle(target, queries, max_dist)
    got_d, got_i, index = device_nearest(dev, target, queries, cell, max_dist)
    found = int((want_i >= 0).sum())
    bad_d = int((got_d.view(np.uint32) != want_d.view(np.uint32)).sum())
    print(f"cloud_eval {what}: n = {len(target)}, m = {len(queries)}, found = {found}, idx differing = {int((got_i != want_i).sum())}, "
          f"dist bits differing = {bad_d}")
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    return want_d, want_i, index


def cube(n, seed, lo=0.0, hi=1.0):
    return (lo + (hi - lo) * np.random.default_rng(seed).random((n, 3))).astype(F32)


@pytest.fixture(scope="module")
def random_pair():
    """n = 5000 targets and m = 3000 queries in the unit cube, with the oracle's answers at both cut-offs (computed once)"""
    t, q = cube(5000, 1), cube(3000, 2)
    return {"t": t, "q": q, 0.05: oracle(t, q, 0.05), 0.12: oracle(t, q, 0.12)}


# ---------------------------------------------------------------- the search
@pytest.mark.parametrize("max_dist", [0.05, 0.12])
def test_random_cloud_one_and_three_rings(dev, random_pair, max_dist):
    want_d, want_i = random_pair[max_dist]
    got_d, got_i, index = device_nearest(dev, random_pair["t"], random_pair["q"], 0.05, max_dist)
    assert index.n == 5000 and 0 < index.cells <= 8000
    assert 0 < (want_i >= 0).sum() and ((want_i < 0).sum() > 0 or max_dist > 0.1)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    # the order in which the queries are walked changes nothing
    d2, i2, _ = device_nearest(dev, random_pair["t"], random_pair["q"], 0.05, max_dist, sort_queries=False)
    assert np.array_equal(i2, want_i) and np.array_equal(d2.view(np.uint32), want_d.view(np.uint32))


@pytest.mark.parametrize("n", [1, 63, 257, 4097])
@pytest.mark.parametrize("m", [1, 65, 1025])
def test_sizes_off_the_wave_and_block_multiples(dev, n, m):
    check(dev, cube(n, 10 + n), cube(m, 20 + m), 0.05, 0.1, f"sizes n={n} m={m}")


def test_empty_queries_and_empty_target(dev):
    from cer_mvs_amd.cloud_eval import CloudIndex, cloud_distances, voxel_downsample
    t = cube(100, 3)
    d, i, index = device_nearest(dev, t, np.zeros((0, 3), F32), 0.1, 0.2)
    assert d.shape == (0,) and i.shape == (0,) and index.n == 100
    d, i, index = device_nearest(dev, np.zeros((0, 3), F32), t, 0.1, 0.2)
    assert index.n == 0 and index.cells == 0 and (i == -1).all() and np.isposinf(d).all() and d.shape == (100,)
    assert voxel_downsample(torch.zeros(0, 3, device=dev), 0.1).shape == (0,)
    assert cloud_distances(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev), 0.1).shape == (0,)
    assert CloudIndex(torch.full((5, 3), float("nan"), device=dev), 0.1).n == 0


def test_duplicates_give_the_lowest_index(dev):
    g = np.random.default_rng(7)
    base = cube(1500, 4)
    t = np.concatenate([base, base, base])[g.permutation(4500)]
    q = np.concatenate([base[:700], cube(800, 5)])
    want_d, want_i, _ = check(dev, t, q, 0.05, 0.08, "duplicates")
    hit = want_i[:700]
    assert (want_d[:700] == 0).all()
    for k in (0, 1, 350, 699):                               # the lowest of the three copies
        copies = np.flatnonzero((t == base[k]).all(1))
        assert len(copies) == 3 and hit[k] == copies.min()


def lattice(plane):
    k = np.arange(-20, 21).astype(F32) * F32(0.1)            # k * np.float32(0.1), rounded to float32
    if not plane:
        return np.stack([k, np.zeros_like(k), np.zeros_like(k)], 1)
    x, y = np.meshgrid(k, k, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(x.size, F32)], 1).astype(F32)


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("max_dist", [0.1, 0.2])
def test_points_on_cell_boundaries(dev, plane, max_dist):
    """every coordinate sits on (or an ulp beside) a cell face; the oracle decides inclusion at d = max_dist"""
    pts = lattice(plane)
    check(dev, pts, pts, 0.1, max_dist, "lattice on itself")
    # the same lattice as queries against every other node: the neighbours are one spacing away, where 0.1f * k - 0.1f * (k - 1) is above or
    # below max_dist from node to node
    k = np.arange(len(pts))
    sub = pts[(k % 2) == 0]
    want_d, want_i, _ = check(dev, sub, pts, 0.1, max_dist, "lattice on every other node")
    if max_dist == 0.1:
        odd = want_i[(k % 2) == 1]
        assert (odd >= 0).any() and (odd < 0).any()          # both sides of the cut-off occur


def test_cut_off_is_inclusive_in_fp64(dev):
    q = np.zeros((1, 3), F32)
    at = np.array([[0.5, 0, 0]], F32)
    beyond = np.array([[np.nextafter(F32(0.5), F32(1)), 0, 0]], F32)
    d, i, _ = device_nearest(dev, at, q, 0.125, 0.5)
    assert i[0] == 0 and d[0] == F32(0.5)
    d, i, _ = device_nearest(dev, beyond, q, 0.125, 0.5)
    assert i[0] == -1 and np.isposinf(d[0])
    for cell in (0.5, 0.3, 0.07):
        check(dev, np.concatenate([beyond, at]), q, cell, 0.5, f"cut-off cell={cell}")
    d, i, _ = device_nearest(dev, at, at, 0.125, 0.0)        # max_dist = 0: a coincident point is found
    assert i[0] == 0 and d[0] == 0


def test_queries_outside_the_bounding_box(dev):
    t = cube(2000, 6)
    g = np.random.default_rng(8)
    q = []
    for axis in range(3):
        for side in (0, 1):
            for off in (0.03, 0.08, 0.25, 40.0, 3e6):        # less than and more than max_dist = 0.1; far beyond the key range
                p = g.random((40, 3)).astype(F32)
                p[:, axis] = -off if side == 0 else 1.0 + off
                q.append(p)
    q = np.concatenate(q).astype(F32)
    want_d, want_i, _ = check(dev, t, q, 0.025, 0.1, "outside the box")
    assert (want_i >= 0).any() and (want_i < 0).sum() > 600


def test_one_dense_cell(dev):
    g = np.random.default_rng(9)
    dense = (0.5001 + 0.0998 * g.random((3000, 3))).astype(F32)                 # all inside the cell [0.5, 0.6)^3 of the grid below
    sparse = cube(2000, 12)
    sparse[0] = 0.0                                                          # pins the grid's origin
    t = np.concatenate([sparse, dense])[g.permutation(5000)]
    q = np.concatenate([(0.5 + 0.1 * g.random((600, 3))), (0.35 + 0.4 * g.random((900, 3))), cube(500, 13)]).astype(F32)
    _, _, index = check(dev, t, q, 0.1, 0.1, "dense cell")
    counts = np.diff(index.cell_start.cpu().numpy())
    assert counts.max() >= 3000 and index.n == 5000
    check(dev, t, q, 0.1, 0.25, "dense cell, three rings")


def test_non_finite_points_and_queries(dev):
    t, q = cube(1000, 14), cube(600, 15)
    for k, row in enumerate(([np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.nan])):
        t[37 * k + 5] = row
        q[29 * k + 3] = row
    q[200] = t[5 + 37]                                       # a query equal to a non-finite target
    want_d, want_i, index = check(dev, t, q, 0.05, 0.15, "non-finite")
    assert index.n == 995
    bad = [29 * k + 3 for k in range(5)] + [200]
    assert (want_i[bad] == -1).all() and not np.isin(want_i, [37 * k + 5 for k in range(5)]).any()


def test_determinism_and_permutations(dev):
    g = np.random.default_rng(16)
    t, q = cube(4000, 17), cube(2500, 18)
    assert len(np.unique(t, axis=0)) == len(t)               # duplicate-free: idx maps through a permutation of the targets
    d0, i0, _ = device_nearest(dev, t, q, 0.04, 0.1)
    d1, i1, _ = device_nearest(dev, t, q, 0.04, 0.1)
    assert d0.tobytes() == d1.tobytes() and i0.tobytes() == i1.tobytes()
    pq = g.permutation(len(q))
    d2, i2, _ = device_nearest(dev, t, q[pq], 0.04, 0.1)
    assert d2.tobytes() == d0[pq].tobytes() and i2.tobytes() == i0[pq].tobytes()
    pt = g.permutation(len(t))                               # new position j holds old point pt[j]
    d3, i3, _ = device_nearest(dev, t[pt], q, 0.04, 0.1)
    assert d3.tobytes() == d0.tobytes()
    assert np.array_equal(np.where(i3 >= 0, pt[np.maximum(i3, 0)], -1), i0)


# ---------------------------------------------------------------- voxel thinning
def oracle_keys(points, cell):
    """(finite [n] bool, packed cell key of every finite point: int64, one dimension, ordered as the device's keys)"""
    P = np.asarray(points, F32).astype(np.float64)
    finite = np.isfinite(P).all(1)
    origin = P[finite].min(0)
    c = np.floor((P[finite] - origin) / np.float64(cell)).astype(np.int64)
    return finite, (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def oracle_voxels(points, cell):
    finite, keys = oracle_keys(points, cell)
    first = np.unique(keys, return_index=True)[1]            # the first occurrence: the lowest index
    return np.sort(np.flatnonzero(finite)[first])


@pytest.mark.parametrize("cloud", ["random", "line", "plane", "nan"])
def test_voxel_downsample_keeps_the_lowest_index_of_every_cell(dev, random_pair, cloud):
    from cer_mvs_amd.cloud_eval import voxel_downsample
    pts = {"random": random_pair["t"], "line": lattice(False), "plane": lattice(True), "nan": random_pair["q"].copy()}[cloud]
    cell = 0.1 if cloud in ("line", "plane") else 0.07
    if cloud == "nan":
        pts[::50, 1] = np.nan
    if cloud in ("line", "plane"):
        pts = np.concatenate([pts, pts[::-1]])               # every node twice: the first copy is kept
    got = voxel_downsample(torch.from_numpy(pts).to(dev), cell)
    assert got.dtype == torch.int64
    got = got.cpu().numpy()
    want = oracle_voxels(pts, cell)
    assert np.array_equal(got, want) and (np.diff(got) > 0).all() and 0 < len(got) < len(pts)
    again = voxel_downsample(torch.from_numpy(pts).to(dev), cell).cpu().numpy()
    assert again.tobytes() == got.tobytes()


def test_cell_table_across_the_scan_chunk_edge(dev):
    """1024 * 2048 + 1 points: 1025 partials, the smallest cloud at which the cell passes' scan carries a total from one 1024-partial chunk into
    the next.  2^21 points fill the 32^3 cells of the unit cube (every tile of sorted keys holds a few dozen heads); the last point, the
    highest index, lies alone in a far cell, so its key sorts last: the one key of tile 1024, a head, ranked by the carried total alone."""
    from cer_mvs_amd.cloud_eval import CloudIndex, voxel_downsample
    n, cell = 1024 * 2048 + 1, 1.0 / 32
    pts = np.random.default_rng(31).random((n, 3), dtype=F32)
    pts[0] = 0.0                                             # (the origin: cell edges at multiples of 2^-5, exact in every format)
    pts[-1] = 2.0
    finite, keys = oracle_keys(pts, cell)
    uniq, first, counts = np.unique(keys, return_index=True, return_counts=True)
    assert finite.all() and 20000 < len(uniq) <= 32 ** 3 + 1 and uniq[-1] == keys[-1] and counts[-1] == 1
    d = torch.from_numpy(pts).to(dev)
    index = CloudIndex(d, cell)
    assert index.cells == len(uniq) and index.n == n
    assert np.array_equal(index.cell_start.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
    assert np.array_equal(index.cell_keys.cpu().numpy() - index.cell_keys[0].item(), uniq - uniq[0])
    got = voxel_downsample(d, cell).cpu().numpy()
    assert np.array_equal(got, np.sort(first)) and got[-1] == n - 1


# ---------------------------------------------------------------- the protocols
def same_metrics(got, want, keys):
    for k in keys:
        g, w = got[k], want[k]
        if isinstance(w, int):
            assert g == w, (k, g, w)
        else:
            assert abs(g - w) <= 1e-12 * abs(w), (k, g, w)


DTU_KEYS = ("accuracy", "completeness", "overall", "n_pred", "n_gt", "n_pred_in", "n_gt_in")


def test_accuracy_completeness_and_fscore_equal_the_oracle(dev, random_pair):
    from cer_mvs_amd import cloud_eval as CE
    t, q = random_pair["t"], random_pair["q"]
    pred, gt = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    for max_dist in (0.05, 0.12):
        d_pred = random_pair[max_dist][0]
        d_gt = oracle(q, t, max_dist)[0]
        want = CE.metrics_from_distances(d_pred, d_gt, max_dist)
        got = CE.accuracy_completeness(pred, gt, max_dist=max_dist)
        assert set(got) == set(DTU_KEYS) and got["n_pred"] == 3000 and got["n_gt"] == 5000 and 0 < got["n_pred_in"] <= 3000
        assert (got["n_pred_in"] < 3000) == (max_dist < 0.1)     # at 0.05 some queries have no neighbour, at 0.12 all have one
        same_metrics(got, want, DTU_KEYS)
        same_metrics(CE.accuracy_completeness(pred, gt, max_dist=max_dist, cell=0.031), want, DTU_KEYS)      # the cell changes nothing
        dd = CE.cloud_distances(pred, gt, max_dist).cpu().numpy()
        assert dd.view(np.uint32).tobytes() == d_pred.view(np.uint32).tobytes()
    tau = 0.0625                                             # exact in float32: the cut-off of the search is tau itself
    want = CE.metrics_from_distances(oracle(t, q, tau)[0], oracle(q, t, tau)[0], tau, tau=tau)
    got = CE.fscore(pred, gt, tau)
    assert set(got) == {"precision", "recall", "fscore", "tau", "n_pred", "n_gt"} and 0 < got["precision"] < 1 and 0 < got["recall"] < 1
    same_metrics(got, want, ("precision", "recall", "fscore", "n_pred", "n_gt"))
    far = CE.fscore(pred, gt + 10.0, tau)
    assert far["precision"] == 0.0 and far["recall"] == 0.0 and far["fscore"] == 0.0


def test_thin_and_keep_masks_take_effect(dev, random_pair):
    from cer_mvs_amd import cloud_eval as CE
    t, q = random_pair["t"], random_pair["q"]
    pred, gt = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    sel = oracle_voxels(q, 0.09)
    assert 0 < len(sel) < len(q)
    got = CE.accuracy_completeness(pred, gt, max_dist=0.12, thin=0.09)
    want = CE.metrics_from_distances(oracle(t, q[sel], 0.12)[0], oracle(q[sel], t, 0.12)[0], 0.12)
    assert got["n_pred"] == len(sel)
    same_metrics(got, want, DTU_KEYS)
    kp, kg = q[:, 0] < 0.5, t[:, 2] > 0.25
    got = CE.accuracy_completeness(pred, gt, max_dist=0.12, keep_pred=torch.from_numpy(kp).to(dev), keep_gt=torch.from_numpy(kg))
    want = CE.metrics_from_distances(random_pair[0.12][0][kp], oracle(q, t, 0.12)[0][kg], 0.12)
    assert got["n_pred"] == int(kp.sum()) and got["n_gt"] == int(kg.sum())
    same_metrics(got, want, DTU_KEYS)
    # both: the mask is thinned with the points
    got = CE.accuracy_completeness(pred, gt, max_dist=0.12, thin=0.09, keep_pred=torch.from_numpy(kp).to(dev))
    want = CE.metrics_from_distances(oracle(t, q[sel], 0.12)[0][kp[sel]], oracle(q[sel], t, 0.12)[0], 0.12)
    assert got["n_pred"] == int(kp[sel].sum())
    same_metrics(got, want, DTU_KEYS)
    with pytest.raises(ValueError, match="keep_pred"):
        CE.accuracy_completeness(pred, gt, keep_pred=torch.ones(7, dtype=torch.bool))


# ---------------------------------------------------------------- end to end
def test_reconstructed_cloud_against_itself_and_the_oracle(dev):
    """the smallest scan tests/test_reconstruct_gpu.py builds, through reconstruct_scan(write=False)"""
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd.scan import reconstruct_scan
    from test_reconstruct_gpu import NAMES, NF, PAIRS, _model, _scan
    images, poses, intr, scales = _scan(128, 160)
    out = reconstruct_scan(_model(dev), images, poses, intr, NAMES, PAIRS, scales, None, num_frames=NF, streams=2, write=False)
    xyz = np.ascontiguousarray(out["xyz"], F32)
    assert len(xyz) > 1000 and np.isfinite(xyz).all()
    extent = float((xyz.max(0) - xyz.min(0)).max())
    max_dist = float(F32(0.05 * extent))
    cloud = torch.from_numpy(xyz).to(dev)
    m = CE.accuracy_completeness(cloud, cloud, max_dist=max_dist)
    assert m["accuracy"] == 0.0 and m["completeness"] == 0.0 and m["overall"] == 0.0 and m["n_pred_in"] == m["n_gt_in"] == len(xyz)
    f = CE.fscore(cloud, cloud, max_dist / 4)
    assert f["precision"] == 1.0 and f["recall"] == 1.0 and f["fscore"] == 1.0
    print(f"reconstructed cloud: {len(xyz)} points, extent {extent:.4f}, max_dist {max_dist:.5f}")
    check(dev, xyz, xyz[:4000], max_dist / 4, max_dist, "reconstructed cloud, first 4000 points on the whole")
    # ... and on a displaced copy, where the neighbour is not the point itself
    check(dev, xyz, xyz[:4000] + F32(0.3 * max_dist), max_dist / 4, max_dist, "reconstructed cloud, displaced")
