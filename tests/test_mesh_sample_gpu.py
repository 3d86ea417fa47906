"""Mesh surface sampling on the MI355X (csrc/mesh_sample.hip, cer-mvs_amd/mesh.py face_areas / sample_mesh / sample_mesh_even /
evaluate_mesh) against the numpy restatement of tests/mesh_sample_reference.py.  Every comparison is exact: integers as
integers, floats as bits, ``info`` as dictionaries.  The restatement itself is held to the published Philox vectors, to a sample worked out
by hand and to the statistics of the issue in tests/test_mesh_sample_cpu.py."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_sample_reference as R
import mesh_smooth_reference as S
from conftest import REPO

pytestmark = pytest.mark.gpu

MAXW = 0xffffffff


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sphere12():
    """the small analytic sphere mesh and colours for it, computed once and left unchanged"""
    v, f, centre = S.field_mesh("sphere12")
    return v, f, centre, R.random_colors(len(v))


def same(a, b):
    """bit equality (NaNs included), shape and dtype"""
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def on(dev, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def dev_sample(dev, v, f, colors=None, words=None, **kw):
    from cer_mvs_amd import mesh as ME
    info = {}
    out = ME.sample_mesh(on(dev, R.as_vertices(v)), on(dev, R.as_faces(f)), colors=on(dev, colors), words=on(dev, words, np.uint32), info=info, **kw)
    p, face, nrm, col, uv = out
    n = p.shape[0]
    assert p.dtype == torch.float32 and tuple(p.shape) == (n, 3) and face.dtype == torch.int32 and tuple(face.shape) == (n,)
    assert (nrm is None) == (not kw.get("normals", False)) and (nrm is None or (nrm.dtype == torch.float32 and tuple(nrm.shape) == (n, 3)))
    assert (col is None) == (colors is None) and (col is None or (col.dtype == torch.uint8 and tuple(col.shape) == (n, 3)))
    assert (uv is None) == (not kw.get("uv", False)) and (uv is None or (uv.dtype == torch.float64 and tuple(uv.shape) == (n, 2)))
    assert all(a is None or a.is_cuda for a in out) and tuple(info) == R.INFO_KEYS and type(info["n"]) is int and type(info["area"]) is float
    return tuple(None if a is None else a.cpu().numpy() for a in out), info


def check_sample(dev, v, f, what="", colors=None, words=None, n=None, seed=0, offset=0, normals=False, uv=False):
    """all five results of sample_mesh and its info on the device against the restatement -> the device's results"""
    kw = dict(normals=normals, uv=uv)
    if words is None:
        kw.update(n=n, seed=seed, offset=offset)
    got, ginfo = dev_sample(dev, v, f, colors=colors, words=words, **kw)
    want, winfo = R.sample(v, f, n=n, seed=seed, offset=offset, words=words, normals=normals, colors=colors, uv=uv)
    assert ginfo == winfo, (what, ginfo, winfo)
    for name, g, w in zip(("points", "face", "normals", "colors", "uv"), got, want):
        assert (g is None and w is None) or same(g, w), (what, name)
    return got


# ---------------------------------------------------------------- areas and weights
HAND_VERTICES = np.array([[0, 0, 0], [3, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [np.nan, 0, 0], [np.inf, 0, 0], [3, 2.0 ** -40, 0],
                          [0.1, 0.7, -0.3], [1e-20, 0, 0], [0, 1e-20, 0], [3e38, 0, 0], [0, -3e38, 0]], np.float32)
HAND_FACES = [[0, 1, 2], [0, 3, 4], [0, 1, 1], [0, -1, 2], [0, 1, 13], [0, 1, 5], [0, 6, 2], [0, 1, 7], [8, 1, 4], [2, 2, 2], [0, 9, 10], [0, 11, 12],
              [-2147483648, 0, 1], [0, 1, 2147483647]]


def dev_areas(dev, v, f):
    from cer_mvs_amd import mesh as ME
    a = ME.face_areas(on(dev, R.as_vertices(v)), on(dev, R.as_faces(f)))
    assert a.dtype == torch.float64 and a.is_cuda and tuple(a.shape) == (len(R.as_faces(f)),)
    return a


def dev_weights(dev, areas, shift):
    from cer_mvs_amd import _lib as L
    out = torch.full((areas.shape[0],), -7, device=dev, dtype=torch.int64)
    L.check(L.load().cer_mesh_face_weights_i64(L.dev_ptr(areas, "areas", torch.float64), areas.shape[0], shift, L.dev_ptr(out, "weights", torch.int64),
                                               L.cur_stream()), "mesh_face_weights")
    return out.cpu().numpy()


def test_areas_and_weights_equal_the_restatement(dev, sphere12):
    """the device's fp64 square root against numpy's correctly rounded one, bit for bit"""
    for what, v, f in (("hand-made", HAND_VERTICES, HAND_FACES), ("sphere12", sphere12[0], sphere12[1]),
                       ("random soup", *R.random_mesh(257, 4)), ("nv = 0", np.zeros((0, 3), np.float32), [[0, 1, 2]])):
        got, want = dev_areas(dev, v, f).cpu().numpy(), R.face_areas(v, f)
        differing = int((got.view(np.uint64) != want.view(np.uint64)).sum())
        print(f"face_areas {what}: {len(want)} faces, {differing} differ in their bits from numpy's")
        assert same(got, want), what
        if want.max() > 0:
            shift = R.shift_of(want.max())
            weights = dev_weights(dev, on(dev, want), shift)
            assert np.array_equal(weights, R.face_weights(want, shift)) and 1 << 31 <= weights.max() < 1 << 32, what
    got = dev_areas(dev, HAND_VERTICES, HAND_FACES).cpu().numpy()
    assert got[:10].tolist() == [1.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5 * 2.0 ** -40, got[8], 0.0] and got[8] > 0 and got[10] > 0 and got[12:].tolist() == [0.0, 0.0]
    assert np.isfinite(got).all() and got[11] == 0.5 * (float(np.float32(3e38)) ** 2)           # the largest coordinates: no overflow in fp64
    # weights of areas that are not a mesh's: a NaN, a negative one, infinity and 2^63 and beyond give 0; the extreme shifts
    odd = np.array([np.nan, -1.0, np.inf, 2.0 ** 40, 0.75, 0.0, 2.0 ** 32 - 2.0 ** -21, -0.0, 5e-324], np.float64)
    assert np.array_equal(dev_weights(dev, on(dev, odd), 31), R.face_weights(odd, 31))
    assert dev_weights(dev, on(dev, odd), 31).tolist() == [0, 0, 0, 0, 1610612736, 0, (1 << 63) - (1 << 10), 0, 0]
    for x, shift in ((5e-324, 1105), (2.0 ** -1073, 1104), (1.7e308, -992), (2.0 ** 1023, -992)):
        one = np.array([x], np.float64)
        assert shift == R.shift_of(x) and np.array_equal(dev_weights(dev, on(dev, one), shift), R.face_weights(one, shift)), x
    assert dev_areas(dev, sphere12[0], np.zeros((0, 3), np.int32)).shape == (0,)                # nf = 0


# ---------------------------------------------------------------- sampling against the restatement
@pytest.mark.parametrize("nf", (1, 2, 3, 5, 64, 65, 257))
def test_samples_equal_the_restatement_on_random_meshes(dev, nf):
    """random small soups with faces without weight at the start, at the end and in a run in the middle"""
    v, f = R.random_mesh(nf, seed=nf)
    col = R.random_colors(len(v), seed=nf)
    weights = np.diff(R.table(v, f)[0], prepend=0)
    if nf >= 5:
        assert weights[0] == 0 and weights[-1] == 0 and weights[nf // 2] == 0 and (weights > 0).sum() >= 2
    for n in (0, 1, 255, 256, 257, 4099):
        p, face, _, _, _ = check_sample(dev, v, f, f"nf = {nf}, n = {n}", colors=col, n=n, seed=nf, normals=True, uv=True)
        assert (weights[face] > 0).all() and np.isfinite(p).all()


@pytest.mark.parametrize("seed", (0, 1, (1 << 32) + 5))
def test_samples_equal_the_restatement_on_the_sphere(dev, sphere12, seed):
    v, f, _, col = sphere12
    n = 65537
    full = check_sample(dev, v, f, "sphere12, everything", colors=col, n=n, seed=seed, normals=True, uv=True)
    bare = check_sample(dev, v, f, "sphere12, points only", n=n, seed=seed)
    assert same(full[0], bare[0]) and same(full[1], bare[1])                                     # the attributes change nothing
    if seed == 0:
        check_sample(dev, v, f, "sphere12, normals", n=n, normals=True)
        check_sample(dev, v, f, "sphere12, colours", n=n, colors=col)
        check_sample(dev, v, f, "sphere12, uv", n=n, uv=True)
        again, _ = dev_sample(dev, v, f, colors=col, n=n, seed=seed, normals=True, uv=True)
        assert all(same(a, b) for a, b in zip(full, again))                                    # two runs: the same bytes
        assert np.isfinite(full[0]).all() and np.isfinite(full[2]).all() and len(np.unique(full[1])) > 0.9 * len(f)
    else:
        zero = dev_sample(dev, v, f, n=1000, seed=0)[0]
        assert not same(zero[0], bare[0][:1000])                                                 # the seed matters, both of its words


def test_offset_carries_into_the_high_counter_word(dev, sphere12):
    v, f, _, col = sphere12
    check_sample(dev, v, f, "offset 2^32 - 2", colors=col, n=5, seed=3, offset=(1 << 32) - 2, normals=True, uv=True)
    check_sample(dev, v, f, "offset 2^64 - 2", n=5, seed=(1 << 64) - 1, offset=(1 << 64) - 2)    # the index wraps


def test_prefix_property(dev, sphere12):
    v, f, _, col = sphere12
    kw = dict(colors=col, seed=7, normals=True, uv=True)
    long, _ = dev_sample(dev, v, f, n=1000, **kw)
    short, _ = dev_sample(dev, v, f, n=100, **kw)
    tail, info = dev_sample(dev, v, f, n=50, offset=50, **kw)
    assert all(same(s, a[:100]) for s, a in zip(short, long)) and all(same(t, a[50:100]) for t, a in zip(tail, long))
    assert info["n"] == 50
    by_density, dinfo = dev_sample(dev, v, f, density=1000 / info["area"] * 0.9995, **kw)       # ceil(area * density) = 1000
    assert dinfo["n"] == R.count_for(info["area"], 1000 / info["area"] * 0.9995) == 1000 and all(same(a, b) for a, b in zip(by_density, long))


# ---------------------------------------------------------------- planted words
def test_planted_words(dev):
    # faces 0 and 5 have no weight (a repeated index); face 3 is a sliver below 2^-32 of the largest
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 2], [1, 1, 1], [4, 2.0 ** -40, 0]], np.float32)
    f = [[0, 1, 1], [0, 1, 2], [0, 2, 3], [0, 1, 5], [1, 2, 4], [3, 3, 4]]
    cum, W, shift, areas = R.table(v, f)
    weights = np.diff(cum, prepend=0)
    assert (weights > 0).tolist() == [False, True, True, False, True, False] and areas[3] > 0
    col = R.random_colors(len(v))
    half = 1 << 31
    words = np.array([[0, 0, 5, 9],                                                             # r = 0: the first face with weight
                      [MAXW, MAXW, 5, 9],                                                       # r = 2^64 - 1: the last one
                      [1, 2, MAXW - 7, 7], [1, 2, half, half - 1],                              # a + b = 2^32 - 1: not folded
                      [1, 2, MAXW - 7, 8], [1, 2, half, half], [1, 2, MAXW, MAXW],              # a + b >= 2^32: folded
                      [1, 2, 0, 0], [1, 2, MAXW, 0], [1, 2, 0, MAXW]], np.uint32)               # the corner A; w = 0 on the edge B C
    p, face, nrm, c, uv = check_sample(dev, v, f, "planted", colors=col, words=words, normals=True, uv=True)
    assert face[0] == 1 and face[1] == 4 and (face[2:] == 1).all()
    two32 = 2.0 ** 32
    assert uv[2].tolist() == [(MAXW - 7 + 0.5) / two32, 7.5 / two32] and uv[3].tolist() == [(half + 0.5) / two32, (half - 0.5) / two32]
    assert uv[4].tolist() == [7.5 / two32, (MAXW - 8 + 0.5) / two32] and uv[5].tolist() == [(half - 0.5) / two32, (half - 0.5) / two32]
    assert uv[6].tolist() == [0.5 / two32, 0.5 / two32] and uv[7].tolist() == [0.5 / two32, 0.5 / two32] and same(p[6], p[7])
    assert uv[8].sum() == 1.0 and uv[9].sum() == 1.0 and p[8].tolist() == [4.0, 2.0 ** -31, 0.0] and p[9].tolist() == [2.0 ** -31, 4.0, 0.0]
    # every face boundary of the table from both sides: the last r of a face and the first of the next
    edges = []
    for t in (int(cum[1]), int(cum[2])):
        r = -((-t << 64) // W)                                                                  # the smallest r with floor(r W / 2^64) >= t
        edges += [[(r - 1) >> 32, (r - 1) & MAXW, 3, 4], [r >> 32, r & MAXW, 3, 4]]
    _, face, _, _, _ = check_sample(dev, v, f, "face boundaries", words=np.array(edges, np.uint32))
    assert face.tolist() == [1, 2, 2, 4]
    # the sliver is never drawn: a sweep of r, and random words
    sweep = np.zeros((4096, 4), np.uint32)
    sweep[:, 0] = np.arange(4096, dtype=np.uint64) << np.uint64(20)
    sweep[:, 2:] = np.random.default_rng(1).integers(0, 1 << 32, (4096, 2), dtype=np.uint64)
    _, face, _, _, _ = check_sample(dev, v, f, "sweep", words=sweep)
    assert set(face.tolist()) == {1, 2, 4} and (np.diff(face) >= 0).all()
    _, face, _, _, _ = check_sample(dev, v, f, "random", n=4099, seed=5)
    assert set(face.tolist()) == {1, 2, 4}
    assert dev_sample(dev, v, f, words=np.zeros((0, 4), np.uint32))[0][0].shape == (0, 3)


def test_a_table_that_is_not_the_meshs_own_stays_inside(dev):
    """the kernel under a prefix table its caller did not build: the search ends inside [0, nf - 1] and a face with bad indices gives NaN"""
    from cer_mvs_amd import _lib as L
    v = np.array([[1, 2, 3], [5, 2, 3], [1, 10, 3]], np.float32)
    f = np.array([[0, 1, 3], [0, 1, 1], [0, 1, 2], [-1, 0, 1]], np.int32)
    col = R.random_colors(3)
    words = R.philox_words(9, 0, 300)
    for cum in ([1, 2, 3, 4], [0, 0, 0, 0], [5, 5, 5, 5], [-3, -2, -1, -1], [9, 7, 3, 1], [1 << 62, 1 << 62, (1 << 63) - 1, (1 << 63) - 1]):
        cum = np.array(cum, np.int64)
        W = max(int(cum[-1]), 0)
        vd, fd, cd, wd, ud = on(dev, v), on(dev, f), on(dev, col), on(dev, words), on(dev, cum)
        p = torch.full((300, 3), 7.0, device=dev)
        face = torch.full((300,), -7, device=dev, dtype=torch.int32)
        nrm, oc = torch.full((300, 3), 7.0, device=dev), torch.full((300, 3), 7, device=dev, dtype=torch.uint8)
        L.check(L.load().cer_mesh_sample_f32(L.dev_ptr(vd, "v"), 3, L.dev_ptr(fd, "f", torch.int32), 4, L.dev_ptr(ud, "cum", torch.int64), 0, 0,
                                             L.dev_ptr(wd, "words", torch.uint32), 300, L.dev_ptr(cd, "c", torch.uint8), L.dev_ptr(p, "p"),
                                             L.dev_ptr(face, "face", torch.int32), None, L.dev_ptr(nrm, "n"), L.dev_ptr(oc, "oc", torch.uint8),
                                             L.cur_stream()), "mesh_sample")
        got_face = face.cpu().numpy()
        assert got_face.min() >= 0 and got_face.max() <= 3, cum
        if (np.diff(cum) >= 0).all():                                                          # a sorted table: the restatement's pick
            wp, wface, wn, wc, _ = R.sample_with(v, f, cum, W, words, normals=True, colors=col)
            assert np.array_equal(got_face, wface) and same(p.cpu().numpy(), wp) and same(nrm.cpu().numpy(), wn) and same(oc.cpu().numpy(), wc), cum
        bad = got_face != 2
        assert np.isnan(p.cpu().numpy()[bad]).all() and np.isfinite(p.cpu().numpy()[~bad]).all() and not oc.cpu().numpy()[bad].any()


# ---------------------------------------------------------------- even sampling
def brute_force_properties(drawn, kept_points, spacing):
    d = np.linalg.norm(drawn.astype(np.float64)[:, None] - kept_points.astype(np.float64)[None], axis=2)
    between = np.linalg.norm(kept_points.astype(np.float64)[:, None] - kept_points.astype(np.float64)[None], axis=2) + np.where(np.eye(len(kept_points), dtype=bool), np.inf, 0.0)
    return float(between.min()), float(d.min(1).max())


def test_even_sampling_equals_the_restatement(dev, sphere12):
    from cer_mvs_amd import mesh as ME
    v, f, _, col = sphere12
    vd, fd, cd = on(dev, v), on(dev, f), on(dev, col)
    for spacing, seed, oversample in ((0.75, 0, 8.0), (0.75, 2, 8.0), (1.5, 1, 8.0), (0.5, 3, 2.0)):
        (wp, wface, wn, wc), kept, n0 = R.sample_even(v, f, spacing, oversample=oversample, seed=seed, normals=True, colors=col)
        assert n0 <= 4096
        info = {}
        p, face, nrm, c = ME.sample_mesh_even(vd, fd, spacing, oversample=oversample, seed=seed, normals=True, colors=cd, info=info)
        assert info["drawn"] == n0 and info["kept"] == len(kept) and info["n_finite"] == n0 and info["rounds"] >= 1
        assert {k: info[k] for k in ("area", "faces_with_weight", "shift")} == {k: x for k, x in R.info_of(v, f, 0).items() if k != "n"}
        assert same(p.cpu().numpy(), wp) and same(face.cpu().numpy(), wface) and same(nrm.cpu().numpy(), wn) and same(c.cpu().numpy(), wc)
        (drawn, _, _, _, _), _ = dev_sample(dev, v, f, n=n0, seed=seed)
        assert same(drawn[kept], wp)                                                             # the kept indices are the restatement's
        apart, reach = brute_force_properties(drawn, p.cpu().numpy(), spacing)
        print(f"sample_mesh_even spacing {spacing}: drawn {n0}, kept {len(kept)}, closest kept pair {apart:.4f}, farthest drawn sample {reach:.4f}")
        assert apart > spacing and reach <= spacing
    p, face, nrm, c = ME.sample_mesh_even(vd, fd, 0.75)
    assert nrm is None and c is None and same(p.cpu().numpy(), R.sample_even(v, f, 0.75)[0][0])


# ---------------------------------------------------------------- evaluation
def sphere_points(centre, radius, n, seed=8):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (np.asarray(centre) + radius * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def test_evaluate_mesh_equals_the_cloud_protocols_on_the_restated_samples(dev):
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd import mesh as ME
    v, f, centre = S.field_mesh("sphere24")
    gt = sphere_points(centre, 9.3, 4000)
    vd, fd, gd = on(dev, v), on(dev, f), on(dev, gt)
    spacing, tau = 1.5, 0.5
    (wp, _, _, _), kept, n0 = R.sample_even(v, f, spacing, seed=4)
    assert n0 <= 4096
    samples = on(dev, wp)
    got = ME.evaluate_mesh(vd, fd, gd, spacing, max_dist=3.0, tau=tau, seed=4)
    want = CE.accuracy_completeness(samples, gd, 3.0)
    want.update(CE.fscore(samples, gd, tau))
    want.update(samples=len(kept), spacing=spacing)
    assert set(got) == set(want) and all(np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes() for k in want), (got, want)
    plain = ME.evaluate_mesh(vd, fd, gd, spacing, max_dist=3.0, seed=4)
    assert plain == {k: x for k, x in got.items() if k not in ("precision", "recall", "fscore", "tau")}
    T = np.eye(4)
    T[:3, 3] = (0.25, -0.5, 0.125)
    moved = ME.evaluate_mesh(vd, fd, gd, spacing, max_dist=3.0, tau=tau, seed=4, align=T)
    want = CE.accuracy_completeness(samples, gd, 3.0, align=T)
    want.update(CE.fscore(samples, gd, tau, align=T))
    assert all(np.float64(moved[k]).tobytes() == np.float64(want[k]).tobytes() for k in want) and moved["accuracy"] > got["accuracy"]
    # the figures, recorded without a bar: the 24^3 sphere against points on the analytic sphere at two spacings
    figures = {}
    for s in (1.5, 0.75):
        m = ME.evaluate_mesh(vd, fd, gd, s, max_dist=3.0, tau=tau, seed=4, oversample=8.0 if s == 1.5 else 2.0)
        figures[f"spacing {s}"] = m
        print(f"evaluate_mesh, 24^3 sphere (r = 9.3 voxels) against 4000 points on it, spacing {s}: {json.dumps(m)}")
    assert figures["spacing 1.5"] == got
    if os.environ.get("CER_PARITY_RECORD"):
        path = os.path.join(REPO, "profiles", "mesh_sample_parity.json")
        record = json.load(open(path))
        record["evaluate24"] = figures
        json.dump(record, open(path, "w"), indent=1)


# ---------------------------------------------------------------- the tools
def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(REPO, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_mesh_sample_and_evaluate_tools(dev, sphere12, tmp_path, monkeypatch, capsys):
    """tools/mesh_sample.py and tools/evaluate_mesh.py, run in this process"""
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd import fusion as FU
    from cer_mvs_amd import mesh as ME
    v, f, centre, col = sphere12
    src, dst, gtf = tmp_path / "in.ply", tmp_path / "out.ply", tmp_path / "gt.ply"
    ME.write_mesh_ply(src, v, f, colors=col)
    tool = _tool("mesh_sample")
    (wp, _, wn, wc, _), winfo = R.sample(v, f, n=777, seed=6, normals=True, colors=col)
    monkeypatch.setattr("sys.argv", ["mesh_sample.py", str(src), str(dst), "--n", "777", "--seed", "6", "--normals"])
    tool.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["samples"] == 777 and {k: line[k] for k in winfo} == winfo and line["normals"] and line["colors"]
    xyz, rgb, nrm = CE.read_ply(dst, normals=True)
    assert same(xyz, wp) and same(rgb, wc) and same(nrm, wn)
    ME.write_mesh_ply(src, v, f)
    (wp, _, _, _), kept, n0 = R.sample_even(v, f, 0.75, seed=1)
    monkeypatch.setattr("sys.argv", ["mesh_sample.py", str(src), str(dst), "--spacing", "0.75", "--seed", "1"])
    tool.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["samples"] == len(kept) and line["drawn"] == n0 and not line["colors"] and same(CE.read_ply(dst)[0], wp)
    gt = sphere_points(centre, 4.2, 1500)
    FU.write_ply(str(gtf), gt, np.zeros((len(gt), 3), np.uint8))
    monkeypatch.setattr("sys.argv", ["evaluate_mesh.py", str(src), str(gtf), "--spacing", "0.75", "--max-dist", "2.0", "--tau", "0.5", "--seed", "1"])
    _tool("evaluate_mesh").main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = ME.evaluate_mesh(on(dev, v), on(dev, f), on(dev, gt), 0.75, max_dist=2.0, tau=0.5, seed=1)
    assert {k: line[k] for k in want} == want and line["samples"] == len(kept)


# ---------------------------------------------------------------- chain
SAME_KEYS = ("xyz", "rgb", "masks", "depth_est", "mesh_vertices", "mesh_faces")
NEW_KEYS = {"mesh_samples", "mesh_sample_faces", "mesh_sample_colors"}


def test_reconstruct_scan_sample(dev, tmp_path):
    import test_reconstruct_gpu as TR
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd.scan import reconstruct_scan
    images, poses, intr, scales = TR._scan(128, 160)
    model = TR._model(dev)
    args = (model, images, poses, intr, TR.NAMES, TR.PAIRS, scales)
    kw = dict(num_frames=TR.NF, streams=2)
    plain_dir, sample_dir = tmp_path / "plain", tmp_path / "sample"
    plain_dir.mkdir()
    sample_dir.mkdir()
    plain = reconstruct_scan(*args, plain_dir, mesh={"resolution": 48}, **kw)
    assert not NEW_KEYS & set(plain) and set(plain["mesh_info"]) == {"grid", "trunc", "nv", "nf", "observed"}      # without the new key: no new key
    assert sorted(p.name for p in plain_dir.iterdir() if p.suffix == ".ply") == ["result.ply", "result_mesh.ply"]
    out = reconstruct_scan(*args, sample_dir, mesh={"resolution": 48, "sample": 1000}, **kw)
    assert set(out) - set(plain) == {"mesh_samples", "mesh_sample_faces"} and set(out["mesh_info"]) - set(plain["mesh_info"]) == {"sampled"}
    for key in SAME_KEYS:                                                                        # everything else: byte-equal to the plain run
        assert out[key].dtype == plain[key].dtype and out[key].tobytes() == plain[key].tobytes(), key
    for name in ("result.ply", "result_mesh.ply"):
        assert (sample_dir / name).read_bytes() == (plain_dir / name).read_bytes(), name
    v, f = out["mesh_vertices"], out["mesh_faces"]
    (p, face, _, _, _), info = dev_sample(dev, v, f, n=1000)
    (wp, wface, _, _, _), winfo = R.sample(v, f, n=1000)
    assert same(out["mesh_samples"], p) and same(out["mesh_sample_faces"], face) and out["mesh_info"]["sampled"] == info == winfo
    assert same(p, wp) and same(face, wface)
    xyz, rgb = CE.read_ply(sample_dir / "result_mesh_samples.ply")
    assert same(xyz, p) and not rgb.any()
    # a dictionary, a seed, colours: the samples carry the mixed vertex colours
    voxel = plain["mesh_info"]["grid"].voxel
    both = reconstruct_scan(*args, None, write=False, mesh={"resolution": 48, "colors": True, "sample": {"spacing": 2 * voxel, "seed": 3}}, **kw)
    assert NEW_KEYS <= set(both) and both["mesh_vertices"].tobytes() == v.tobytes()
    (wp, wface, _, wc), kept, n0 = R.sample_even(v, f, 2 * voxel, seed=3, colors=both["mesh_colors"], thin=lambda pts, r: device_thin(dev, pts, r))
    assert same(both["mesh_samples"], wp) and same(both["mesh_sample_faces"], wface) and same(both["mesh_sample_colors"], wc)
    sampled = both["mesh_info"]["sampled"]
    assert sampled["drawn"] == n0 and sampled["kept"] == len(kept)
    print(f"reconstruct_scan sample: 1000 samples on {len(f)} faces, area {info['area']:.4f}; spacing of two voxels: {sampled}")


def device_thin(dev, points, radius):
    """``radius_thin`` in index order (held to the sequential loop by tests/test_cloud_thin_gpu.py): the scan's mesh draws too many samples for
    the brute-force matrix"""
    from cer_mvs_amd.cloud_eval import radius_thin
    return radius_thin(on(dev, points), radius, order="index").cpu().numpy()


# ---------------------------------------------------------------- errors
def test_sample_refuses_bad_arguments_on_the_device(dev, sphere12):
    from cer_mvs_amd import mesh as ME
    v, f, _, col = sphere12
    vd, fd, cd = on(dev, v), on(dev, f), on(dev, col)
    flat = torch.zeros(4, 3, device=dev)
    for call in (lambda: ME.sample_mesh(flat, fd[:3] * 0, n=1), lambda: ME.sample_mesh(vd, fd[:0], n=1), lambda: ME.sample_mesh(vd[:0], fd[:0], n=5),
                 lambda: ME.sample_mesh(flat, torch.tensor([[0, 1, 2]], device=dev, dtype=torch.int32), n=3),
                 lambda: ME.sample_mesh(vd, fd[:0], words=torch.zeros(2, 4, device=dev, dtype=torch.uint32)),
                 lambda: ME.sample_mesh(vd[:3], fd[-4:], n=1)):                                  # every index out of range: no area
        with pytest.raises(ValueError, match="without area"):
            call()
    info = {}
    out = ME.sample_mesh(flat, fd[:0], n=0, normals=True, uv=True, info=info)                    # nothing asked of nothing: empties
    assert [tuple(a.shape) for a in out if a is not None] == [(0, 3), (0,), (0, 3), (0, 2)] and info == dict(n=0, area=0.0, faces_with_weight=0, shift=0)
    assert ME.sample_mesh(flat, fd[:0], density=5.0)[0].shape == (0, 3)                          # ceil(0 * density) = 0
    assert [tuple(a.shape) for a in ME.sample_mesh_even(flat, fd[:0], 0.5)[:2]] == [(0, 3), (0,)]
    with pytest.raises(ValueError, match="beyond 2\\^31 - 1"):
        ME.sample_mesh(vd, fd, density=1e9)
    with pytest.raises(ValueError, match="beyond 2\\^31 - 1"):
        ME.sample_mesh_even(vd, fd, 1e-4)
    with pytest.raises(ValueError, match="one device"):
        ME.sample_mesh(vd, fd.cpu(), n=4)
    with pytest.raises(ValueError, match="one device"):
        ME.sample_mesh(vd, fd, n=4, colors=cd.cpu())
    with pytest.raises(ValueError, match="one device"):
        ME.sample_mesh(vd, fd, words=torch.zeros(2, 4, dtype=torch.uint32))
    with pytest.raises(ValueError, match="one device"):
        ME.evaluate_mesh(vd, fd, torch.zeros(4, 3), 0.5)
    for call in (lambda: ME.face_areas(vd.cpu(), fd.cpu()), lambda: ME.sample_mesh(vd.cpu(), fd.cpu(), n=4),
                 lambda: ME.sample_mesh_even(vd.cpu(), fd.cpu(), 0.5), lambda: ME.evaluate_mesh(vd.cpu(), fd.cpu(), torch.zeros(4, 3), 0.5)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()
