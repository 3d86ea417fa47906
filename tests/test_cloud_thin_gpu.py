"""Greedy radius thinning on the MI355X (cloud_eval.radius_thin, csrc/cloud_eval.hip grid_thin_round_kernel) against an oracle written
here: a numpy fp64 brute-force neighbour matrix with the contract's three operations for d2 and its inclusive test against
double(float32(radius))^2, and the sequential visiting loop of the DTU script over it.  The bar: the kept index set is EQUAL.

A second restatement, the synchronous-round form of the device's loop (every undecided point looks at the states of the round before), is run
beside it: it must reach the same set, and its round count bounds the device's, whose in-place updates can only decide a point earlier -
``info["rounds"]`` counts launches, which come in groups of THIN_ROUNDS_PER_COMPACTION, hence the rounding up."""
import numpy as np
import pytest
import torch

from test_cloud_eval_gpu import DTU_KEYS, cube, lattice, oracle as oracle_nearest, same_metrics

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


# ---------------------------------------------------------------- oracle
def neighbours(points, radius):
    """bool [n, n]: d2(i, j) <= double(float32(radius))^2, d2 = (dx*dx + dy*dy) + dz*dz in fp64; a non-finite point is nobody's neighbour"""
    P = np.asarray(points, F32).astype(np.float64).reshape(-1, 3)
    limit = np.float64(F32(radius)) * np.float64(F32(radius))
    nb = np.zeros((len(P), len(P)), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(P), 512):
            q = P[s:s + 512]
            dx, dy, dz = P[None, :, 0] - q[:, None, 0], P[None, :, 1] - q[:, None, 1], P[None, :, 2] - q[:, None, 2]
            nb[s:s + 512] = ((dx * dx + dy * dy) + dz * dz) <= limit             # (a NaN compares false)
    return nb


def visiting_order(n, order, seed=0):
    if isinstance(order, str) and order == "index":
        return np.arange(n)
    if isinstance(order, str):
        return torch.randperm(n, generator=torch.Generator("cpu").manual_seed(seed)).numpy()
    return np.asarray(order)


def sequential(nb, finite, visit):
    """the DTU script's loop: a point that is still in the set stays and removes every point within the radius -> kept indices, ascending"""
    alive, kept = finite.copy(), []
    for i in visit:
        if alive[i]:
            kept.append(i)
            alive &= ~nb[i]
    return np.sort(np.asarray(kept, np.int64))


def synchronous(nb, finite, visit):
    """the rounds of the device, every point reading the states of the round before -> (kept indices ascending, rounds)"""
    n = len(finite)
    rank = np.empty(n, np.int64)
    rank[visit] = np.arange(n)
    lower = nb & (rank[None, :] < rank[:, None])              # lower[i, j]: j is a neighbour of i visited before i
    kept, und, rounds = np.zeros(n, bool), finite.copy(), 0
    while und.any():
        near_kept, near_und = (lower & kept[None, :]).any(1), (lower & und[None, :]).any(1)
        removed, keep = und & near_kept, und & ~near_kept & ~near_und
        kept |= keep
        und &= ~(removed | keep)
        rounds += 1
    return np.flatnonzero(kept), rounds


def oracle_thin(points, radius, order="random", seed=0):
    """-> (kept indices, synchronous rounds, mean neighbours per finite point)"""
    P = np.asarray(points, F32).reshape(-1, 3)
    nb, finite = neighbours(P, radius), np.isfinite(P).all(1)
    visit = visiting_order(len(P), order, seed)
    kept = sequential(nb, finite, visit)
    kept_sync, rounds = synchronous(nb, finite, visit)
    assert np.array_equal(kept, kept_sync)                    # the fixed point of the rounds is the sequential loop's set
    k = kept[:, None]
    assert not (nb[k, kept[None, :]] & (k != kept[None, :])).any()                # independent
    assert nb[:, kept].any(1)[finite].all()                                       # maximal (a kept point is its own neighbour)
    return kept, rounds, (nb.sum() - finite.sum()) / max(int(finite.sum()), 1)


def launches(sync_rounds):
    """the bound on info["rounds"]: the synchronous count, rounded up to whole groups of launches"""
    from cer_mvs_amd.cloud_eval import THIN_ROUNDS_PER_COMPACTION as K
    return -(-sync_rounds // K) * K


def device_thin(dev, points, radius, **kw):
    from cer_mvs_amd.cloud_eval import radius_thin
    info = {}
    if isinstance(kw.get("order"), np.ndarray):
        kw["order"] = torch.from_numpy(kw["order"]).to(dev)
    got = radius_thin(torch.from_numpy(np.ascontiguousarray(points, F32).reshape(-1, 3)).to(dev), radius, info=info, **kw)
    assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 1
    got = got.cpu().numpy()
    assert (np.diff(got) > 0).all()
    return got, info


def check(dev, points, radius, what="", order="random", seed=0, **kw):
    want, sync_rounds, mean_nb = oracle_thin(points, radius, order, seed)
    got, info = device_thin(dev, points, radius, order=order, seed=seed, **kw)
    print(f"radius_thin {what}: n = {len(points)}, kept {len(got)} (oracle {len(want)}), {mean_nb:.2f} neighbours per point, rounds {info['rounds']} "
          f"(synchronous {sync_rounds}), compactions {info['compactions']}, differing = {len(np.setxor1d(got, want))}")
    assert np.array_equal(got, want)
    assert 1 <= info["rounds"] <= launches(sync_rounds) and 1 <= info["compactions"] <= info["rounds"]
    assert info["n_finite"] == int(np.isfinite(np.asarray(points, F32).reshape(-1, 3)).all(1).sum())
    return want, info


# ---------------------------------------------------------------- random cube
CUBES = {4097: 0.078, 2049: 0.15}


@pytest.fixture(scope="module")
def cubes():
    """the two clouds with their neighbour matrices (computed once)"""
    out = {}
    for n, radius in CUBES.items():
        P = cube(n, 40 + n)
        out[n] = (P, neighbours(P, radius), np.isfinite(P).all(1))
    return out


@pytest.mark.parametrize("n", sorted(CUBES))
@pytest.mark.parametrize("order", ["random0", "random1", "index", "tensor"])
def test_random_cube_equals_the_sequential_loop(dev, cubes, n, order):
    P, nb, finite = cubes[n]
    radius = CUBES[n]
    seed = 1 if order == "random1" else 0
    visit = visiting_order(n, "index" if order == "index" else "random", seed)
    want = sequential(nb, finite, visit)
    want_sync, sync_rounds = synchronous(nb, finite, visit)
    assert np.array_equal(want, want_sync)
    kw = {"order": visit} if order == "tensor" else {"order": "index"} if order == "index" else {"order": "random", "seed": seed}
    got, info = device_thin(dev, P, radius, **kw)
    print(f"radius_thin cube n = {n}, radius {radius}, {order}: kept {len(got)} (oracle {len(want)}), {(nb.sum() - n) / n:.2f} neighbours per point, "
          f"rounds {info['rounds']} (synchronous {sync_rounds}), compactions {info['compactions']}")
    assert 0 < len(want) < n and np.array_equal(got, want)
    assert info["rounds"] <= 64 and info["rounds"] <= launches(sync_rounds) and info["n_finite"] == n
    if order == "tensor":                                     # the explicit order is seed 0's permutation: the same set
        assert np.array_equal(got, device_thin(dev, P, radius, order="random", seed=0)[0])


@pytest.mark.parametrize("cell", [0.039, 0.2])
def test_the_cell_changes_nothing(dev, cubes, cell):
    """cell = radius / 2 (two rings plus one) and a cell of 2.5 radii"""
    P, nb, finite = cubes[4097]
    want = sequential(nb, finite, visiting_order(4097, "random", 0))
    got, _ = device_thin(dev, P, CUBES[4097], cell=cell)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [1, 2, 63, 257])
def test_sizes_off_the_wave_and_block_multiples(dev, n):
    check(dev, cube(n, 60 + n), 0.15, f"size {n}")
    check(dev, cube(n, 60 + n), 0.15, f"size {n}, index order", order="index")


def test_duplicates_keep_the_lowest_rank(dev):
    g = np.random.default_rng(7)
    P = cube(600, 8)
    copies = g.choice(600, 50, replace=False)
    P[copies] = P[copies[0]]
    for seed in (0, 3):
        want, _ = check(dev, P, 0.05, f"duplicates, seed {seed}", seed=seed)
        visit = visiting_order(600, "random", seed)
        rank = np.empty(600, np.int64)
        rank[visit] = np.arange(600)
        among = np.intersect1d(want, copies)
        # one copy at most, the lowest rank of them - unless an earlier kept point within the radius removed them all
        assert len(among) <= 1 and (len(among) == 0 or among[0] == copies[np.argmin(rank[copies])])
    want, _ = check(dev, np.repeat(P[:1], 50, 0), 0.05, "nothing but duplicates", order="index")
    assert list(want) == [0]
    want, _ = check(dev, np.repeat(P[:1], 50, 0), 0.05, "nothing but duplicates, random", seed=2)
    assert list(want) == [int(visiting_order(50, "random", 2)[0])]


# ---------------------------------------------------------------- the cut-off
@pytest.mark.parametrize("radius", [0.5, 0.1, 0.3])
def test_cut_off_is_inclusive_in_fp64(dev, radius):
    r = F32(radius)
    at = np.array([[0, 0, 0], [r, 0, 0]], F32)
    beyond = np.array([[0, 0, 0], [np.nextafter(r, F32(1)), 0, 0]], F32)
    for cell in (None, float(r) / 2, 0.07, 3.0):
        for axis in range(3):
            a, b = np.roll(at, axis, 1), np.roll(beyond, axis, 1)
            got, _ = device_thin(dev, a, radius, order="index", cell=cell)
            assert list(got) == [0]                           # exactly float32(radius) apart: the later one goes
            got, _ = device_thin(dev, a[::-1], radius, order="index", cell=cell)
            assert list(got) == [0]
            got, _ = device_thin(dev, b, radius, order="index", cell=cell)
            assert list(got) == [0, 1]                        # one ulp farther: both stay
    check(dev, at, radius, "cut-off, at", order="index")
    check(dev, beyond, radius, "cut-off, beyond", order="index")


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("cell", [None, 0.05])
def test_lattice_on_cell_faces(dev, plane, cell):
    """k * 0.1f with radius 0.1f: every coordinate sits on (or an ulp beside) a cell face, and the spacing 0.1f * k - 0.1f * (k - 1) is above or
    below the radius from node to node; cell = radius and cell = radius / 2"""
    pts = lattice(plane)
    nb = neighbours(pts, 0.1)
    step = np.diagonal(nb, 1) if not plane else nb[np.arange(len(pts) - 1), np.arange(1, len(pts))]
    assert step.any() and not step.all()                      # both sides of the cut-off occur
    for order, seed in (("index", 0), ("random", 0), ("random", 4)):
        check(dev, pts, 0.1, f"lattice plane={plane} cell={cell} {order} {seed}", order=order, seed=seed, cell=cell)


# ---------------------------------------------------------------- the long chain
def chain():
    k = np.arange(300).astype(F32) * F32(0.03)
    return np.stack([k, np.zeros_like(k), np.zeros_like(k)], 1)


def test_long_chain_in_index_order(dev):
    """points along a line, visited along it: two synchronous rounds per kept point"""
    from cer_mvs_amd.cloud_eval import radius_thin
    pts = chain()
    want, sync_rounds, _ = oracle_thin(pts, 0.1, "index")
    assert np.array_equal(want, np.arange(0, 300, 4)) and len(want) == 75 and sync_rounds == 150
    got, info = device_thin(dev, pts, 0.1, order="index")
    print(f"radius_thin chain, index order: rounds {info['rounds']} (synchronous 150), compactions {info['compactions']}")
    assert np.array_equal(got, want)
    assert info["rounds"] <= 150
    with pytest.raises(RuntimeError, match='order="random"'):
        radius_thin(torch.from_numpy(pts).to(dev), 0.1, order="index", max_rounds=8)


def test_long_chain_in_random_order(dev):
    pts = chain()
    want, sync_rounds, _ = oracle_thin(pts, 0.1, "random", 0)
    assert len(want) == 60 and sync_rounds == 6
    got, info = device_thin(dev, pts, 0.1, order="random", seed=0)
    print(f"radius_thin chain, random order: rounds {info['rounds']} (synchronous {sync_rounds})")
    assert np.array_equal(got, want) and info["rounds"] <= launches(sync_rounds)
    got8, _ = device_thin(dev, pts, 0.1, order="random", seed=0, max_rounds=launches(sync_rounds))
    assert np.array_equal(got8, want)


# ---------------------------------------------------------------- non-finite points, empty clouds, arguments
def test_non_finite_points_are_never_kept_and_remove_nobody(dev):
    P = cube(1000, 14)
    rows = ([np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.nan])
    bad = [0] + [37 * k + 5 for k in range(1, 5)]
    for b, row in zip(bad, rows):
        P[b] = row
    P[1] = [0.5, 0.5, 0.5]                                    # the first finite point visited: beside the non-finite one before it
    for order, seed in (("index", 0), ("random", 0), ("random", 6)):
        want, info = check(dev, P, 0.09, f"non-finite {order} {seed}", order=order, seed=seed)
        assert info["n_finite"] == 995 and not np.isin(want, bad).any()
        if order == "index":
            assert want[0] == 1
    # the same cloud without the non-finite rows keeps the same points
    fin = np.setdiff1d(np.arange(1000), bad)
    got, _ = device_thin(dev, P[fin], 0.09, order="index")
    assert np.array_equal(fin[got], check(dev, P, 0.09, "non-finite, again", order="index")[0])


def test_empty_and_all_non_finite_clouds(dev):
    from cer_mvs_amd.cloud_eval import radius_thin
    for pts in (torch.zeros(0, 3, device=dev), torch.full((7, 3), float("nan"), device=dev), torch.full((300, 3), float("inf"), device=dev)):
        for order in ("random", "index", torch.arange(len(pts), device=dev)):
            info = {"rounds": -1}
            got = radius_thin(pts, 0.1, order=order, info=info)
            assert got.shape == (0,) and got.dtype == torch.int64 and got.is_cuda
            assert info == {"rounds": 0, "compactions": 0, "n_finite": 0}


def test_bad_arguments_on_the_device(dev):
    from cer_mvs_amd.cloud_eval import radius_thin
    pts = torch.from_numpy(cube(16, 1)).to(dev)
    with pytest.raises(RuntimeError, match="float32"):
        radius_thin(pts.double(), 0.1)
    with pytest.raises(ValueError, match="n, 3"):
        radius_thin(pts[:, :2], 0.1)
    for order in (torch.arange(15), torch.arange(17), torch.arange(16) + 1, torch.zeros(16, dtype=torch.int64), -torch.arange(16),
                  torch.cat([torch.arange(15), torch.tensor([14])])):
        with pytest.raises(ValueError, match="permutation"):
            radius_thin(pts, 0.1, order=order)
    with pytest.raises(ValueError, match="cell"):
        radius_thin(pts, 0.1, cell=0.0)
    with pytest.raises(ValueError, match="larger cell"):
        radius_thin(pts, 0.5, cell=1e-4)                      # 5000 rings
    got = radius_thin(pts, 0.1, order=torch.arange(16).flip(0))                  # a CPU order tensor is taken
    assert got.is_cuda


# ---------------------------------------------------------------- invariants where a brute force is too big
def test_invariants_on_50000_points(dev):
    from cer_mvs_amd.cloud_eval import CloudIndex, radius_thin
    n, radius = 50_000, 0.034                                 # (4 / 3) pi r^3 n = 8.2 neighbours on average
    P = torch.from_numpy(cube(n, 77)).to(dev)
    P[::997] = float("nan")
    info = {}
    kept = radius_thin(P, radius, info=info)
    again = radius_thin(P, radius)
    assert torch.equal(kept, again) and kept.dtype == torch.int64
    finite = torch.isfinite(P).all(1)
    assert info["n_finite"] == int(finite.sum()) and info["rounds"] <= 64
    is_kept = torch.zeros(n, dtype=torch.bool, device=dev)
    is_kept[kept] = True
    assert bool(finite[kept].all())
    dropped = torch.nonzero(finite & ~is_kept).flatten()
    K = P.index_select(0, kept)
    print(f"radius_thin invariants: kept {len(kept)} of {int(finite.sum())}, rounds {info['rounds']}, compactions {info['compactions']}")
    assert 0 < len(kept) < n and len(dropped) > 0
    # maximal: every dropped finite point has a kept point within the radius
    idx = CloudIndex(K, radius).nearest(P.index_select(0, dropped), radius)[1]
    assert bool((idx >= 0).all())
    # independent: no two kept points within the radius (fp64, the contract's operations)
    K64, limit = K.double(), float(F32(radius)) ** 2
    closest = float("inf")
    for s in range(0, len(K64), 1024):
        q = K64[s:s + 1024]
        dx, dy, dz = K64[None, :, 0] - q[:, None, 0], K64[None, :, 1] - q[:, None, 1], K64[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[torch.arange(len(q), device=dev), torch.arange(s, s + len(q), device=dev)] = float("inf")
        closest = min(closest, float(d2.min()))
    assert closest > limit, (closest, limit)
    # another seed: another set of about the same size, with the same two properties by construction
    other = radius_thin(P, radius, seed=1)
    assert not torch.equal(other, kept) and abs(len(other) - len(kept)) < 0.05 * len(kept)


# ---------------------------------------------------------------- the protocol
@pytest.fixture(scope="module")
def pair():
    return cube(5000, 1), cube(3000, 2)                       # gt, pred


@pytest.mark.parametrize("seed", [0, 5])
def test_accuracy_completeness_with_greedy_thinning_equals_the_oracle(dev, pair, seed):
    from cer_mvs_amd import cloud_eval as CE
    t, q = pair
    pred, gt = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    sel = oracle_thin(q, 0.09, "random", seed)[0]
    assert 0 < len(sel) < len(q)
    d_pred, d_gt = oracle_nearest(t, q[sel], 0.12)[0], oracle_nearest(q[sel], t, 0.12)[0]
    want = CE.metrics_from_distances(d_pred, d_gt, 0.12)
    got = CE.accuracy_completeness(pred, gt, max_dist=0.12, thin=0.09, thin_method="greedy", thin_seed=seed)
    assert set(got) == set(DTU_KEYS) and got["n_pred"] == len(sel)
    same_metrics(got, want, DTU_KEYS)
    # the mask follows the selection
    kp = q[:, 0] < 0.5
    got = CE.accuracy_completeness(pred, gt, max_dist=0.12, thin=0.09, thin_method="greedy", thin_seed=seed, keep_pred=torch.from_numpy(kp).to(dev))
    want = CE.metrics_from_distances(d_pred[kp[sel]], d_gt, 0.12)
    assert got["n_pred"] == int(kp[sel].sum())
    same_metrics(got, want, DTU_KEYS)


def test_the_default_thinning_is_still_the_voxel_one(dev, pair):
    from cer_mvs_amd import cloud_eval as CE
    t, q = pair
    pred, gt = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    default = CE.accuracy_completeness(pred, gt, max_dist=0.12, thin=0.09)
    voxel = CE.accuracy_completeness(pred, gt, max_dist=0.12, thin=0.09, thin_method="voxel", thin_seed=3)
    greedy = CE.accuracy_completeness(pred, gt, max_dist=0.12, thin=0.09, thin_method="greedy")
    assert default == voxel and default["n_pred"] == len(CE.voxel_downsample(pred, 0.09))
    assert greedy["n_pred"] == len(CE.radius_thin(pred, 0.09)) != default["n_pred"]
    assert CE.accuracy_completeness(pred, gt, max_dist=0.12) == CE.accuracy_completeness(pred, gt, max_dist=0.12, thin_method="greedy")      # no thin: no thinning
