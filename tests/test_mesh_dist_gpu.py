"""Exact point-to-mesh distance on the MI355X (csrc/mesh_dist.hip, cer-mvs_amd/mesh.py MeshIndex / mesh_distances /
evaluate_mesh(method="exact")) against the numpy brute force of tests/mesh_dist_reference.py.  Every comparison is in bits:
distances, faces and closest points as bytes, pairs and counts as integers, ``info`` as dictionaries.  The restatement itself is held to
answers worked out by hand and to exact rational arithmetic in tests/test_mesh_dist_cpu.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_dist_reference as D
import mesh_sample_reference as R
import mesh_smooth_reference as S
from conftest import REPO

pytestmark = pytest.mark.gpu

CELLS = (0.3, 1.0, 2.5, None)
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sphere12():
    """the small analytic sphere mesh, computed once and left unchanged"""
    return S.field_mesh("sphere12")


def on(dev, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def same(a, b):
    """bit equality (NaNs included), shape and dtype"""
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def build(dev, v, f, cell=None, max_dist=None):
    from cer_mvs_amd import mesh as ME
    return ME.MeshIndex(on(dev, R.as_vertices(v)), on(dev, R.as_faces(f)), cell, max_dist)


def nearest(index, dev, q, max_dist, closest=True, sort_queries=True):
    out = index.nearest(on(dev, np.ascontiguousarray(q, np.float32).reshape(-1, 3)), max_dist, closest=closest, sort_queries=sort_queries)
    m = out[0].shape[0]
    assert len(out) == (3 if closest else 2) and all(t.is_cuda for t in out)
    assert out[0].dtype == torch.float32 and tuple(out[0].shape) == (m,) and out[1].dtype == torch.int32 and tuple(out[1].shape) == (m,)
    assert not closest or (out[2].dtype == torch.float32 and tuple(out[2].shape) == (m, 3))
    return tuple(t.cpu().numpy() for t in out)


def check(dev, v, f, q, max_dist, cells=(None,), what="", want=None):
    """the device at every cell of ``cells``, with the closest points and without, against the brute force -> the brute force's results"""
    want = D.brute(v, f, q, max_dist) if want is None else want
    for cell in cells:
        index = build(dev, v, f, cell, max_dist)
        got = nearest(index, dev, q, max_dist)
        for name, g, w in zip(("dist", "face", "closest"), got, want):
            assert same(g, w), (what, cell, name, np.flatnonzero((g != w).reshape(len(g), -1).any(1))[:5])
        plain = nearest(index, dev, q, max_dist, closest=False)
        assert same(plain[0], want[0]) and same(plain[1], want[1]), (what, cell)
    return want


def soup(nf, seed, size=0.6):
    """nf small triangles scattered in a box of edge 4, each with vertices of its own"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.0, 4.0, (nf, 1, 3))
    v = (centres + rng.uniform(-size, size, (nf, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)


def box_queries(v, m, seed, pad=0.5):
    rng = np.random.default_rng(seed)
    finite = v[np.isfinite(v).all(1)]
    return rng.uniform(finite.min(0) - pad, finite.max(0) + pad, (m, 3)).astype(np.float32)


# ---------------------------------------------------------------- shapes
def test_soups_of_every_size_and_every_query_count(dev):
    found = 0
    for nf in (1, 2, 3, 64, 65, 257):
        v, f = soup(nf, nf)
        for m in ((0, 1, 255, 256, 257) if nf == 65 else (257,)):
            want = check(dev, v, f, box_queries(v, m, 100 + m), 1.0, cells=(0.5, None), what=(nf, m))
            found += int((want[1] >= 0).sum())
    assert found >= 800
    q = box_queries(soup(3, 3)[0], 5, 1)
    for v, f in ((np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
                 (np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32))):               # nf = 0; nv = 0; nv = 0 with a face
        want = check(dev, v, f, q, 5.0, cells=(1.0, None))
        assert (want[1] == -1).all() and np.isinf(want[0]).all() and np.isnan(want[2]).all()
        index = build(dev, v, f, 1.0)
        assert index.info() == dict(cell=1.0, pairs=0, faces_indexed=0, cells=0)


# ---------------------------------------------------------------- ties and zero distance
def test_ties_go_to_the_lowest_face_and_surface_points_have_distance_zero(dev):
    """A fan of four faces around the apex, coordinates multiples of 6: an edge's midpoint has v = 1/2, exact, and a centroid v = w =
    fl(1/3), whose products with multiples of 3 below 2^50 round to the exact integers - so the closest point is the query itself and the
    distance an exact 0 (on a mesh at large that is not promised: v and w round)."""
    v = np.array([[0, 0, 6], [6, 0, 0], [0, 6, 0], [-6, 0, 0], [0, -6, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], np.int32)
    lowest = [min(i for i, face in enumerate(f) if k in face) for k in range(len(v))]
    mids = np.array([(v[a] + v[b]) / 2 for a, b in ((0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (4, 1))], np.float32)
    mid_face = [0, 0, 1, 2, 0, 1, 2, 3]
    cents = v[f].astype(np.float64).mean(1).astype(np.float32)
    q = np.concatenate([v, mids, cents])
    want = check(dev, v, f, q, 1.0, cells=(0.7, 2.0, None))
    assert (want[0] == 0.0).all() and want[1].tolist() == lowest + mid_face + [0, 1, 2, 3] and same(want[2], q)
    assert check(dev, v, f, q, 0.0, cells=(2.0,))[1].tolist() == want[1].tolist()              # max_dist = 0: the cut-off is inclusive
    # two coincident faces, and the same pair with opposite orientation: the lower index, from every side
    tri = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0]], np.float32)
    q = np.array([[1, 1, 0], [1, 1, 2], [1, 1, -2], [5, 5, 1], [-1, -1, 0], [1.5, -2, 0.5], [0, 0, 0], [1.5, 1.5, 0]], np.float32)
    for f2 in ([[0, 1, 2], [0, 1, 2]], [[0, 1, 2], [0, 2, 1]], [[0, 2, 1], [0, 1, 2]], [[1, 2, 0], [2, 1, 0]]):
        want = check(dev, tri, f2, q, 10.0, cells=(1.0, None))
        assert (want[1] == 0).all()
        one = D.brute(tri, [f2[1]], q, 10.0)
        assert same(want[0], one[0])                                                             # either orientation: the same distance


# ---------------------------------------------------------------- faces that must never win
BAD_VERTICES = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, 1]], np.float32)
BAD_FACES = [[0, 1, 1], [0, -1, 2], [0, 1, 7], [INT_MIN, 1, 2], [0, 1, INT_MAX], [0, 1, 4], [5, 1, 2], [0, 1, 3], [2, 2, 2]]


def test_faces_that_must_never_win(dev):
    q = np.concatenate([box_queries(BAD_VERTICES, 60, 2), BAD_VERTICES[:4], [[0.5, 0, 0], [1.5, 0, 0]]]).astype(np.float32)
    want = check(dev, BAD_VERTICES, BAD_FACES, q, 50.0, cells=(0.5, None))                      # a mesh of nothing but such faces
    assert (want[1] == -1).all() and np.isinf(want[0]).all() and np.isnan(want[2]).all()
    good = [[0, 1, 6], [0, 2, 6]]
    mixed = [BAD_FACES[i // 2] if i % 2 == 0 else good[(i // 2) % 2] for i in range(2 * len(BAD_FACES))]
    want = check(dev, BAD_VERTICES, mixed, q, 50.0, cells=(0.5, 1.0, None))
    assert set(want[1].tolist()) <= {i for i in range(len(mixed)) if i % 2 == 1} and (want[1] >= 0).all()
    index = build(dev, BAD_VERTICES, mixed, 1.0)
    assert index.info() == D.info_of(BAD_VERTICES, mixed, 1.0) and index.faces_indexed == len(BAD_FACES)


def test_a_sliver_and_queries_that_are_not_finite(dev):
    v = np.array([[0, 0, 0], [8, 0, 0], [4, 2.0 ** -20, 0], [4, 1e-30, 0], [0, 0, 1]], np.float32)
    f = [[0, 1, 2], [0, 1, 3], [0, 1, 4]]
    q = np.concatenate([box_queries(v, 100, 4), [[4, 0, 0], [4, 2.0 ** -21, 0], [4, -1, 0], [9, 0, 0]]]).astype(np.float32)
    want = check(dev, v, f, q, 3.0, cells=(0.5, 2.5, None))
    assert {0, 2} <= set(want[1].tolist()) and D.indexed_faces(v, f).tolist() == [True, True, True]
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [1, 0, 0]], np.float32)
    want = check(dev, v, f, bad, 3.0, cells=(0.5, None))
    assert want[1].tolist() == [-1, -1, -1, -1, 0]


# ---------------------------------------------------------------- the cut-off
def test_the_cut_off_is_inclusive(dev):
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    q = np.array([[1, 1, 0.5], [1, 1, -0.5], [1, 1, 0], [-0.5, 0, 0]], np.float32)
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert check(dev, v, [[0, 1, 2]], q, 0.5, cells=(0.3, 1.0, None))[1].tolist() == [0, 0, 0, 0]
    assert check(dev, v, [[0, 1, 2]], q, below, cells=(0.3, 1.0, None))[1].tolist() == [-1, -1, 0, -1]
    assert check(dev, v, [[0, 1, 2]], q, 0.0, cells=(0.3, 1.0))[1].tolist() == [-1, -1, 0, -1]


# ---------------------------------------------------------------- the cell does not matter
def fan(n=300):
    t = np.linspace(0.0, 2.0 * np.pi, n, endpoint=False)
    v = np.concatenate([[[0.0, 0.0, 1.0]], np.stack([3.0 * np.cos(t), 3.0 * np.sin(t), np.zeros(n)], 1)]).astype(np.float32)
    return v, np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)


def long_triangle(x):
    return np.array([[0, 0, 0], [x, 0, 0], [0, 0.25, 0]], np.float32), np.array([[0, 1, 2]], np.int32)


def test_the_cell_does_not_matter(dev, sphere12):
    meshes = {"sphere12": sphere12[:2], "open12": S.field_mesh("open12")[:2], "random": S.field_mesh("random")[:2], "fan": fan(),
              "long": long_triangle(1228.6)}                                                       # 4096 cells of 0.3: the cap itself
    assert D.cell_counts(*meshes["long"], 0.3)[0].tolist() == [4096]
    for name, (v, f) in meshes.items():
        if name == "long":
            rng = np.random.default_rng(6)
            q = np.stack([rng.uniform(-2, 1231, 300), rng.uniform(-1, 1, 300), rng.uniform(-1, 1, 300)], 1).astype(np.float32)
        else:
            q = np.concatenate([box_queries(v, 500 if name != "sphere12" else 2000, 7, pad=1.5), v[::5]])
        want = check(dev, v, f, q, 2.0, cells=CELLS, what=name)
        assert (want[1] >= 0).sum() >= len(q) // 3, name
    v, f = meshes["fan"]
    index = build(dev, v, f, 2.5)
    assert index.pairs >= 300 and index.cells <= 16                                               # many faces per cell


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_cell(dev, sphere12):
    v, f = long_triangle(1228.9)                                                                  # 4097 cells of 0.3
    assert D.cell_counts(v, f, 0.3)[0].tolist() == [0] and D.cell_counts(v, f, 0.3)[2]
    with pytest.raises(ValueError, match=r"more than 4096 cells of 0\.3; use a larger cell"):
        build(dev, v, f, 0.3)
    build(dev, v, f, 0.31)
    v, f = sphere12[:2]
    with pytest.raises(ValueError, match=r"more than 2\^20 cells of 1e-06 along an axis; use a larger cell"):
        build(dev, v, f, 1e-6)
    far = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3e6, 0, 0], [3e6 + 1, 0, 0], [3e6, 1, 0]], np.float32)
    assert D.cell_counts(far, [[0, 1, 2], [3, 4, 5]], 1.0)[1]
    with pytest.raises(ValueError, match=r"more than 2\^20 cells of 1\.0 along an axis; use a larger cell"):
        build(dev, far, [[0, 1, 2], [3, 4, 5]], 1.0)
    index = build(dev, v, f, 0.1)
    for reach in (500.0, math.inf):
        with pytest.raises(ValueError, match=r"max_dist %s is more than 4096 cells of 0\.1" % str(reach).replace(".", r"\.")):
            index.nearest(on(dev, v[:4]), reach)
    from cer_mvs_amd import mesh as ME
    vd, fd = on(dev, v), on(dev, f)
    with pytest.raises(ValueError, match="one device"):
        ME.mesh_distances(vd, fd, torch.zeros(4, 3), 1.0)
    for call in (lambda: ME.MeshIndex(vd.cpu(), fd.cpu(), 1.0), lambda: ME.mesh_distances(vd.cpu(), fd.cpu(), torch.zeros(4, 3), 1.0),
                 lambda: ME.MeshIndex(vd, fd, 1.0).nearest(torch.zeros(4, 3), 1.0)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()


# ---------------------------------------------------------------- pairs
def test_pairs_and_counts_equal_the_restatement(dev, sphere12):
    hand = (np.array([[0, 0, 0], [2.5, 0, 0], [0, 1.5, 0], [0, 0, 0.5], [-1, 0, 0]], np.float32), [[0, 1, 2], [0, 1, 1], [3, 1, 2], [0, 2, 4]])
    from cer_mvs_amd import mesh as ME
    for (v, f), cell in ((hand, 1.0), (sphere12[:2], 1.0), (sphere12[:2], 0.3), (fan(), 2.5), ((BAD_VERTICES, BAD_FACES + [[0, 1, 6]]), 0.5)):
        index = ME.MeshIndex(on(dev, R.as_vertices(v)), on(dev, R.as_faces(f)), cell, _keep_pairs=True)
        keys, ids = (t.cpu().numpy() for t in index._pairs_unsorted)
        wk, wi = D.pairs(v, f, cell)
        assert same(keys, wk) and same(ids, wi) and index.info() == D.info_of(v, f, cell)
        assert [float(x) for x in index.origin] == D.origin_of(v, f).tolist()
        order = np.argsort(wk, kind="stable")
        assert same(index.pair_face.cpu().numpy(), wi[order])                                     # faces ascending inside a cell
    v, f = sphere12[:2]
    info = {}
    d = ME.mesh_distances(on(dev, v), on(dev, f), on(dev, v[:50]), 1.0, info=info)
    assert tuple(info) == D.INFO_KEYS and info == D.info_of(v, f, D.default_cell(v, f, 1.0)) and same(d.cpu().numpy(), D.brute(v, f, v[:50], 1.0)[0])
    assert build(dev, v, f).cell == D.default_cell(v, f) and build(dev, v, f, None, 64.0).cell == 2.0


# ---------------------------------------------------------------- queries
def test_far_queries_orders_and_runs(dev, sphere12):
    v, f = sphere12[:2]
    far = np.array([[1e6, 0, 0], [0, -1e6, 0], [5, 5, 40], [1e30, 1e30, 1e30], [-3e38, 0, 0], [5.5, 5.5, 5.5]], np.float32)
    want = check(dev, v, f, far, 2.0, cells=(0.3, 1.0, None))
    assert want[1][:5].tolist() == [-1] * 5
    q = box_queries(v, 700, 9, pad=1.0)
    index = build(dev, v, f, 1.0)
    first = nearest(index, dev, q, 3.0)
    for again in (nearest(index, dev, q, 3.0), nearest(index, dev, q, 3.0, sort_queries=False), nearest(build(dev, v, f, 1.0), dev, q, 3.0)):
        assert all(same(a, b) for a, b in zip(first, again))
    assert all(same(a, b) for a, b in zip(first, D.brute(v, f, q, 3.0)))


def test_sphere_query_sets(dev, sphere12):
    from cer_mvs_amd import mesh as ME
    v, f = sphere12[:2]
    samples = ME.sample_mesh(on(dev, v), on(dev, f), n=2000, seed=3)[0].cpu().numpy()
    ties = 0
    for name, q in (("box", box_queries(v, 2000, 11, pad=1.5)), ("vertices", v), ("samples", samples)):
        want = check(dev, v, f, q, 20.0, cells=(None,), what=name)
        assert (want[1] >= 0).all()
        if name == "vertices":
            assert (want[0] == 0.0).all() and same(want[2], v)                                    # a corner region returns the corner itself
            ties = len(v)
        if name == "samples":                                                                      # on the surface to float32 rounding
            assert float(want[0].max()) <= 2 * 2.0 ** -24 * float(np.abs(v).max())
    assert ties == 970


# ---------------------------------------------------------------- evaluate_mesh
def sphere_points(centre, radius, n, seed=8):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (np.asarray(centre) + radius * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def test_evaluate_mesh_exact(dev, sphere12):
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd import mesh as ME
    v, f, centre = sphere12
    gt = sphere_points(centre, 4.2, 1000)
    vd, fd, gd = on(dev, v), on(dev, f), on(dev, gt)
    spacing, tau, max_dist = 0.75, 0.1, 2.0
    T = np.eye(4)
    T[:3, 3] = (0.25, -0.5, 0.125)
    for align in (None, T):
        samples = ME.sample_mesh_even(vd, fd, spacing, seed=4)[0]
        moved = v if align is None else CE.rigid_transform(vd, align).cpu().numpy()
        pred = samples if align is None else CE.rigid_transform(samples, align)
        cut = float(np.float32(tau))
        assert cut >= tau
        want = CE.metrics_from_distances(CE.cloud_distances(pred, gd, max_dist).cpu().numpy(), D.brute(moved, f, gt, max_dist)[0], max_dist)
        plain = ME.evaluate_mesh(vd, fd, gd, spacing, max_dist=max_dist, seed=4, align=align, method="exact")
        assert set(plain) == set(want) | {"samples", "spacing", "method"} and plain["method"] == "exact" and plain["samples"] == len(samples)
        assert all(np.float64(plain[k]).tobytes() == np.float64(want[k]).tobytes() for k in want), (plain, want)
        m = CE.metrics_from_distances(CE.cloud_distances(pred, gd, cut).cpu().numpy(), D.brute(moved, f, gt, cut)[0], cut, tau=tau)
        want.update({k: m[k] for k in ("precision", "recall", "fscore", "tau", "n_pred", "n_gt")})
        got = ME.evaluate_mesh(vd, fd, gd, spacing, max_dist=max_dist, tau=tau, seed=4, align=align, method="exact")
        assert set(got) == set(want) | {"samples", "spacing", "method"}
        assert all(np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes() for k in want), (got, want)
        assert got["recall"] <= 1.0 and (align is not None or got["recall"] > 0.5)
    # the default keeps every byte; the sampled route's completeness is never below the exact one's, point by point
    a = ME.evaluate_mesh(vd, fd, gd, spacing, max_dist=max_dist, tau=tau, seed=4)
    b = ME.evaluate_mesh(vd, fd, gd, spacing, max_dist=max_dist, tau=tau, seed=4, method="samples")
    assert a == b and "method" not in a and json.dumps(a) == json.dumps(b)
    samples = ME.sample_mesh_even(vd, fd, spacing, seed=4)[0]
    d_sampled = CE.cloud_distances(gd, samples, max_dist).double().cpu().numpy()
    d_exact = ME.mesh_distances(vd, fd, gd, max_dist).double().cpu().numpy()
    slack = 2 * 2.0 ** -24 * float(np.abs(v).max())                                              # a sample lies within this of its face's plane
    assert (d_exact <= d_sampled + slack).all() and np.isfinite(d_exact).all()
    exact = ME.evaluate_mesh(vd, fd, gd, spacing, max_dist=max_dist, tau=tau, seed=4, method="exact")
    assert exact["completeness"] < a["completeness"] and exact["recall"] >= a["recall"] and exact["accuracy"] == a["accuracy"]
    # the figures, recorded without a bar: the 24^3 sphere of 3zg's record, exact against both spacings
    v24, f24, c24 = S.field_mesh("sphere24")
    g24 = on(dev, sphere_points(c24, 9.3, 4000))
    figures = {}
    for s in (1.5, 0.75):
        kw = dict(max_dist=3.0, tau=0.5, seed=4, oversample=8.0 if s == 1.5 else 2.0)
        sampled = ME.evaluate_mesh(on(dev, v24), on(dev, f24), g24, s, **kw)
        ex = ME.evaluate_mesh(on(dev, v24), on(dev, f24), g24, s, method="exact", **kw)
        figures[f"spacing {s}"] = {k: {"samples": sampled[k], "exact": ex[k]} for k in ("completeness", "recall", "accuracy", "precision")}
        print(f"evaluate_mesh, 24^3 sphere against 4000 points on it, spacing {s}: {json.dumps(figures[f'spacing {s}'])}")
    assert figures["spacing 1.5"]["completeness"]["exact"] == figures["spacing 0.75"]["completeness"]["exact"]      # the spacing no longer matters
    path = os.path.join(REPO, "profiles", "mesh_dist_parity.json")
    if os.environ.get("CER_PARITY_RECORD"):
        record = json.load(open(path))
        record["evaluate24"] = figures
        json.dump(record, open(path, "w"), indent=1)
    assert json.load(open(path))["evaluate24"] == figures


# ---------------------------------------------------------------- tools
def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(REPO, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_mesh_distance_and_evaluate_tools(dev, sphere12, tmp_path, monkeypatch, capsys):
    """tools/mesh_distance.py and tools/evaluate_mesh.py --method exact, run in this process"""
    from cer_mvs_amd import fusion as FU
    from cer_mvs_amd import mesh as ME
    v, f, centre = sphere12
    src, cloud, out = tmp_path / "mesh.ply", tmp_path / "cloud.ply", tmp_path / "d.npy"
    ME.write_mesh_ply(src, v, f)
    pts = np.concatenate([sphere_points(centre, 4.2, 600), [[100, 100, 100]]]).astype(np.float32)
    FU.write_ply(str(cloud), pts, np.zeros((len(pts), 3), np.uint8))
    monkeypatch.setattr("sys.argv", ["mesh_distance.py", str(src), str(cloud), str(out), "--max-dist", "2.0"])
    _tool("mesh_distance").main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = D.brute(v, f, pts, 2.0)[0]
    assert same(np.load(out), want) and line["n"] == 601 and line["within"] == 600 and line["max_dist"] == 2.0
    assert {k: line[k] for k in D.INFO_KEYS} == D.info_of(v, f, D.default_cell(v, f, 2.0))
    assert line["mean"] == float(want[:600].astype(np.float64).mean())
    monkeypatch.setattr("sys.argv", ["mesh_distance.py", str(src), str(cloud), str(out), "--max-dist", "2.0", "--cell", "0.5"])
    _tool("mesh_distance").main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert same(np.load(out), want) and line["cell"] == 0.5
    FU.write_ply(str(cloud), pts[:600], np.zeros((600, 3), np.uint8))
    args = ["evaluate_mesh.py", str(src), str(cloud), "--spacing", "0.75", "--max-dist", "2.0", "--tau", "0.5", "--seed", "1"]
    monkeypatch.setattr("sys.argv", args + ["--method", "exact"])
    _tool("evaluate_mesh").main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = ME.evaluate_mesh(on(dev, v), on(dev, f), on(dev, pts[:600]), 0.75, max_dist=2.0, tau=0.5, seed=1, method="exact")
    assert {k: line[k] for k in want} == want and line["method"] == "exact"
    monkeypatch.setattr("sys.argv", args)
    _tool("evaluate_mesh").main()
    assert "method" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
