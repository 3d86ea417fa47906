"""Mesh edges, the topology report and Taubin smoothing (csrc/mesh.hip, cer-mvs_amd/mesh.py mesh_edges / mesh_topology / smooth_mesh,
DESIGN.md 3ze), the parts that need no GPU: the seven entry points of ABI 1210 and their argument checks in the documented order, the
Python layer's ValueErrors and the forms of the "smooth" and "topology" options, and the numpy restatement of
tests/mesh_smooth_reference.py - which the GPU tests hold the device to, bit for bit - held to results written out by hand, to the figures
of the analytic meshes and to the quality bars of the issue (profiles/mesh_smooth_parity.json)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_smooth_reference as R
from conftest import REPO

BIG = 1 << 31
NAMES = ("cer_mesh_edge_keys_i64", "cer_mesh_edge_count", "cer_mesh_edge_emit_i32", "cer_mesh_smooth_prepare_f32", "cer_mesh_smooth_steps_f64",
         "cer_mesh_smooth_finish_f32")
KERNELS = ("mesh_edge_keys_kernel", "mesh_edge_count_kernel", "mesh_edge_emit_kernel", "mesh_smooth_prepare_kernel", "mesh_smooth_step_kernel",
           "mesh_smooth_finish_kernel")
INFO_KEYS = {"moved", "frozen_boundary", "steps", "edges"}


# ---------------------------------------------------------------- ABI
def test_smooth_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    names = L.exported_symbols()
    for n in NAMES:
        assert n in names and re.search(r"\bint %s\(" % n, hdr), n
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P                 # a stream: the last argument
    assert "cer_mesh_edge_partials" in names and re.search(r"\blong cer_mesh_edge_partials\(", hdr)
    assert L.ABI_VERSION >= 1210 and "Mesh edges and smoothing (ABI 1210" in hdr and len(names) >= 120
    lib = L.load()
    assert lib.cer_abi_version() == L.ABI_VERSION
    src = open(os.path.join(REPO, "cer-mvs_amd", "csrc", "mesh.hip")).read()
    for kernel in KERNELS:
        assert "void " + kernel in src, kernel                                                # in mesh.hip: mesh.o's flags
    section = src[src.index("// ---- mesh edges and smoothing"):]
    assert not re.search(r"atomic\w*\s*\(|\bfmaf?\s*\(", section)                               # no atomics, no fused multiply-add
    step = section[section.index("void mesh_smooth_step_kernel"):section.index("// ---- smoothing, finish")]
    assert not re.search(r"__shared__|__syncthreads", step)                                    # the step: registers only


def test_smooth_entry_points_refuse_bad_arguments_in_the_documented_order():
    """every check runs before any launch (the pointers are fake: a launch would fault).  The order: (1) a negative size CER_EINVAL (-1); (2)
    nv, 6 nf or nn >= 2^31 CER_ESHAPE (-2); (3) a non-finite weight CER_EINVAL; (4) nothing to do CER_OK; (5) null pointers CER_EINVAL - each
    case breaks one rule and every later one, and gets the earlier rule's answer."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, other, null = ctypes.c_void_p(4096), ctypes.c_void_p(8192), None
    sixth = (BIG + 5) // 6
    inf, nan = float("inf"), float("nan")

    assert lib.cer_mesh_edge_partials(-1) == -1 and lib.cer_mesh_edge_partials(sixth) == -2 and lib.cer_mesh_edge_partials(1 << 62) == -2
    assert [lib.cer_mesh_edge_partials(n) for n in (0, 1, 341, 342, 683)] == [0, 1, 1, 2, 3]    # ceil(6 nf / 2048)

    def keys(fac=fake, nf=4, nv=5, out=fake):
        return lib.cer_mesh_edge_keys_i64(fac, nf, nv, out, null)
    kn = dict(fac=null, out=null)
    for kw in (dict(nf=-1), dict(nv=-1), dict(nf=-1, nv=BIG), dict(nv=-1, nf=sixth)):                                                 # 1
        assert keys(**kw) == -1 and keys(**kw, **kn) == -1, kw
    for kw in (dict(nv=BIG), dict(nf=sixth), dict(nf=1 << 62), dict(nf=0, nv=BIG)):                                                   # 2
        assert keys(**kw) == -2 and keys(**kw, **kn) == -2, kw
    assert keys(nf=0) == 0 and keys(nf=0, **kn) == 0 and keys(nf=0, nv=0, **kn) == 0                                                  # 4
    for name in kn:                                                                                                                   # 5
        assert keys(**{name: null}) == -1, name

    def count(ks=fake, nf=4, partials=fake, offsets=fake, totals=fake):
        return lib.cer_mesh_edge_count(ks, nf, partials, offsets, totals, null)
    cn = dict(ks=null, partials=null, offsets=null, totals=null)
    assert count(nf=-1) == -1 and count(nf=-1, **cn) == -1                                                                            # 1
    assert count(nf=sixth) == -2 and count(nf=sixth, **cn) == -2                                                                      # 2
    assert count(nf=0) == 0 and count(nf=0, **cn) == 0                                                                                # 4
    for name in cn:                                                                                                                   # 5
        assert count(**{name: null}) == -1, name

    def emit(ks=fake, nf=4, offsets=fake, nn=6, owner=fake, nbrs=fake, along=fake, against=fake):
        return lib.cer_mesh_edge_emit_i32(ks, nf, offsets, nn, owner, nbrs, along, against, null)
    en = dict(ks=null, offsets=null, owner=null, nbrs=null, along=null, against=null)
    for kw in (dict(nf=-1), dict(nn=-1), dict(nn=-1, nf=sixth)):                                                                      # 1
        assert emit(**kw) == -1 and emit(**kw, **en) == -1, kw
    for kw in (dict(nf=sixth), dict(nn=BIG), dict(nf=0, nn=BIG)):                                                                     # 2
        assert emit(**kw) == -2 and emit(**kw, **en) == -2, kw
    assert emit(nf=0) == 0 and emit(nn=0) == 0 and emit(nf=0, **en) == 0 and emit(nn=0, **en) == 0                                     # 4
    for name in en:                                                                                                                   # 5
        assert emit(**{name: null}) == -1, name

    def prepare(ver=fake, nv=5, starts=fake, nbrs=fake, along=fake, against=fake, nn=6, fixed=1, walk=fake, flags=fake, state=fake):
        return lib.cer_mesh_smooth_prepare_f32(ver, nv, starts, nbrs, along, against, nn, fixed, walk, flags, state, null)
    pn = dict(ver=null, starts=null, nbrs=null, along=null, against=null, walk=null, flags=null, state=null)
    for kw in (dict(nv=-1), dict(nn=-1), dict(nv=-1, nn=BIG)):                                                                        # 1
        assert prepare(**kw) == -1 and prepare(**kw, **pn) == -1, kw
    for kw in (dict(nv=BIG), dict(nn=BIG), dict(nv=0, nn=BIG)):                                                                       # 2
        assert prepare(**kw) == -2 and prepare(**kw, **pn) == -2, kw
    assert prepare(nv=0) == 0 and prepare(nv=0, **pn) == 0 and prepare(nv=0, nn=0, **pn) == 0                                         # 4
    for name in pn:                                                                                                                   # 5
        assert prepare(**{name: null}) == -1, name
    assert prepare(nn=0, nbrs=null, along=null, against=null, walk=null, ver=null) == -1     # no edge: the lists may be null, the rest not

    def steps(a=fake, b=other, nv=5, starts=fake, walk=fake, nn=6, flags=fake, w0=0.5, w1=-0.53, n=2):
        return lib.cer_mesh_smooth_steps_f64(a, b, nv, starts, walk, nn, flags, w0, w1, n, null)
    sn = dict(a=null, b=null, starts=null, walk=null, flags=null)
    for kw in (dict(nv=-1), dict(nn=-1), dict(n=-1), dict(n=-1, nv=BIG), dict(nv=-1, w0=nan)):                                        # 1
        assert steps(**kw) == -1 and steps(**kw, **sn) == -1, kw
    for kw in (dict(nv=BIG), dict(nn=BIG), dict(nv=BIG, w0=nan), dict(nn=BIG, n=0)):                                                  # 2
        assert steps(**kw) == -2 and steps(**kw, **sn) == -2, kw
    for kw in (dict(w0=nan), dict(w0=inf), dict(w1=-inf), dict(w1=nan)):                                                              # 3
        assert steps(**kw) == -1 and steps(**kw, nv=0) == -1 and steps(**kw, n=0, **sn) == -1, kw
    assert steps(nv=0) == 0 and steps(n=0) == 0 and steps(nv=0, **sn) == 0 and steps(n=0, **sn) == 0                                  # 4
    for name in sn:                                                                                                                   # 5
        assert steps(**{name: null}) == -1, name
    assert steps(b=fake) == -1                                                               # one buffer twice: a step must not read what it writes
    assert steps(nn=0, walk=null, a=null) == -1

    def finish(state=fake, ver=fake, flags=fake, nv=5, out=fake):
        return lib.cer_mesh_smooth_finish_f32(state, ver, flags, nv, out, null)
    fn = dict(state=null, ver=null, flags=null, out=null)
    assert finish(nv=-1) == -1 and finish(nv=-1, **fn) == -1                                                                          # 1
    assert finish(nv=BIG) == -2 and finish(nv=BIG, **fn) == -2                                                                        # 2
    assert finish(nv=0) == 0 and finish(nv=0, **fn) == 0                                                                              # 4
    for name in fn:                                                                                                                   # 5
        assert finish(**{name: null}) == -1, name


# ---------------------------------------------------------------- the Python layer
def test_smooth_python_layer_refuses_bad_arguments_without_a_device():
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    ver = torch.zeros(5, 3)
    fac = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    out_of_range = (torch.tensor([[0, 1, 5]], dtype=torch.int32), torch.tensor([[0, -1, 2]], dtype=torch.int32))
    for fn in (ME.mesh_edges, ME.mesh_topology):
        for bad in (fac.long(), fac[:, :2], fac[0], fac.numpy(), None):
            with pytest.raises(ValueError, match="vertex_faces: faces"):                    # vertex_faces' rule, in its wording
                fn(bad, 5)
        for bad in out_of_range:
            with pytest.raises(ValueError, match="vertex_faces: faces must hold indices"):
                fn(bad, 5)
        for bad in (-1, 1 << 31):
            with pytest.raises(ValueError, match="vertex_faces: nv"):
                fn(fac, bad)
        with pytest.raises(ValueError, match="6 nf"):
            fn(torch.zeros(1, dtype=torch.int32).expand((BIG + 5) // 6, 3), 5)              # (an expanded view: no memory behind it, refused by its size)
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(fac, 5)
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(fac[:0], 0)
    sm = ME.smooth_mesh
    for bad in (ver.double(), ver[:, :2], ver[0], ver.numpy(), None):
        with pytest.raises(ValueError, match="vertices"):
            sm(bad, fac, 1)
    for bad in (fac.long(), fac[:, :2], fac[0], fac.numpy(), None):
        with pytest.raises(ValueError, match="faces"):
            sm(ver, bad, 1)
    for bad in out_of_range:
        with pytest.raises(ValueError, match="indices"):
            sm(ver, bad, 1)
    for bad in (0, -1, 1.0, 2.5, True, False, "3", None, [1]):
        with pytest.raises(ValueError, match="iterations"):
            sm(ver, fac, bad)
    for bad in ("Taubin", "humphrey", "", None, 1):
        with pytest.raises(ValueError, match="method"):
            sm(ver, fac, 1, method=bad)
    for bad in ("Fixed", "pinned", "", None, True):
        with pytest.raises(ValueError, match="boundary"):
            sm(ver, fac, 1, boundary=bad)
    for bad in (0, 0.0, -0.5, 1.5, float("inf"), float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match="lam"):
            sm(ver, fac, 1, lam=bad)
    for bad in (-0.5, -0.3, 0.0, 0.53, float("-inf"), float("nan"), True, "-0.53", None):
        with pytest.raises(ValueError, match="mu"):
            sm(ver, fac, 1, mu=bad)
        with pytest.raises(ValueError, match="mu"):
            sm(ver, fac, 1, method="laplacian", mu=bad)                                      # read for "taubin" only, checked always
    for call in (lambda: sm(ver, fac, 1), lambda: sm(ver, fac, 10, method="laplacian", lam=1, boundary="free", info={}),
                 lambda: sm(ver, fac, np.int64(2), lam=np.float32(0.25), mu=-0.26), lambda: sm(ver[:0], fac[:0], 3)):
        with pytest.raises(RuntimeError, match="CUDA"):      # good arguments: the host tensors are what is refused
            call()
    # the options of reconstruct_scan(mesh=...): refused before a model or a session is built
    bad_smooth = (0, -2, 1.0, 2.5, True, False, "3", None, [3], {}, {"method": "taubin"}, {"iterations": 0}, {"iterations": 2.0}, {"iterations": True},
                  {"iterations": 3, "method": "humphrey"}, {"iterations": 3, "lam": 0}, {"iterations": 3, "lam": 1.5}, {"iterations": 3, "mu": -0.4},
                  {"iterations": 3, "lam": 0.2, "mu": -0.2}, {"iterations": 3, "boundary": "pinned"}, {"iterations": 3, "steps": 2}, {"iterations": "3"})
    for bad in bad_smooth:
        with pytest.raises(ValueError, match="mesh: smooth"):
            ME.mesh_options({"smooth": bad})
        with pytest.raises(ValueError, match="mesh: smooth"):
            reconstruct_scan(None, [0], [0], [0], ["a"], [[0]], [1.0], None, write=False, mesh={"resolution": 48, "smooth": bad})
    for bad in (False, 1, "yes", None, {}):
        with pytest.raises(ValueError, match="mesh: topology"):
            ME.mesh_options({"topology": bad})
        with pytest.raises(ValueError, match="mesh: topology"):
            reconstruct_scan(None, [0], [0], [0], ["a"], [[0]], [1.0], None, write=False, mesh={"topology": bad})
    for bad in ({"smoothing": 2}, {"taubin": 2}, {"report": True}):
        with pytest.raises(ValueError, match="unknown"):
            ME.mesh_options(bad)
    for good in ({"smooth": 3}, {"smooth": {"iterations": 2}}, {"smooth": {"iterations": 5, "method": "laplacian", "lam": 1.0, "boundary": "free"}},
                 {"smooth": {"iterations": 1, "lam": 0.33, "mu": -0.34}}, {"topology": True},
                 {"resolution": 48, "min_component": 157, "smooth": 3, "simplify": 2, "colors": True, "normals": True, "topology": True}):
        assert ME.mesh_options(good) == good
    assert "smooth" in ME.MESH_OPTION_KEYS and "topology" in ME.MESH_OPTION_KEYS and ME.mesh_options({"resolution": 48}) == {"resolution": 48}
    assert ME._smooth_option(3) == (3, "taubin", 0.5, -0.53, "fixed")
    assert ME._smooth_option({"iterations": 2, "method": "laplacian", "boundary": "free"}) == (2, "laplacian", 0.5, -0.53, "free")
    assert ME.TOPOLOGY_KEYS == R.TOPOLOGY_KEYS and ME.SMOOTH_METHODS == R.METHODS and ME.SMOOTH_BOUNDARIES == R.BOUNDARIES


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(R.hand_made()))
def test_restated_report_on_hand_made_meshes(name):
    faces, nv, want = R.hand_made()[name]
    report = R.topology(faces, nv)
    assert tuple(report) == R.TOPOLOGY_KEYS and {k: report[k] for k in want} == want, (name, report)
    assert all(type(report[k]) is (bool if k in ("closed", "edge_manifold", "oriented") else int) for k in report)
    starts, nbrs, along, against = R.mesh_edges(faces, nv)
    lo, hi, fw, bw = R.edge_table(faces, nv)
    assert starts.dtype == nbrs.dtype == along.dtype == against.dtype == lo.dtype == np.int32
    assert len(starts) == nv + 1 and starts[0] == 0 and starts[-1] == len(nbrs) == 2 * len(lo) == 2 * report["edges"]
    pairs = {}
    for v in range(nv):
        run = nbrs[starts[v]:starts[v + 1]].tolist()
        assert run == sorted(set(run)) and v not in run                                     # distinct, ascending, never itself
        for e in range(starts[v], starts[v + 1]):
            pairs[(v, int(nbrs[e]))] = (int(along[e]), int(against[e]))
    assert all(pairs[(u, v)] == (b, a) for (v, u), (a, b) in pairs.items())                 # the mirror entry: the counts swapped
    assert [(int(a), int(b)) for a, b in zip(lo, hi)] == sorted(k for k in pairs if k[0] < k[1])
    assert [pairs[(int(a), int(b))] for a, b in zip(lo, hi)] == list(zip(fw.tolist(), bw.tolist()))
    f = R.as_faces(faces)
    assert int(along.sum()) == sum(int(f[q, c] != f[q, (c + 1) % 3]) for q in range(len(f)) for c in range(3))      # every directed edge once


def test_restated_edges_written_out_by_hand():
    starts, nbrs, along, against = R.mesh_edges([[0, 1, 2], [2, 1, 3]], 5)
    assert starts.tolist() == [0, 2, 5, 8, 10, 10] and nbrs.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2]
    assert along.tolist() == [1, 0, 0, 1, 1, 1, 1, 0, 0, 1] and against.tolist() == [0, 1, 1, 1, 0, 0, 1, 1, 1, 0]
    assert [a.tolist() for a in R.edge_table([[0, 1, 2], [2, 1, 3]], 5)] == [[0, 0, 1, 1, 2], [1, 2, 2, 3, 3], [1, 0, 1, 1, 0], [0, 1, 1, 0, 1]]
    # a degenerate face: (2, 2, 1) has the directed edges 2->1 and 1->2 only, which makes 1-2 an edge of three
    assert [a.tolist() for a in R.edge_table([[0, 1, 2], [2, 2, 1]], 3)] == [[0, 0, 1], [1, 2, 2], [1, 0, 2], [0, 1, 1]]
    assert [a.tolist() for a in R.mesh_edges([[1, 1, 1]], 2)] == [[0, 0, 0], [], [], []]


def test_restated_step_on_the_tetrahedron_is_the_mean_of_the_other_three():
    v = np.array(R.TETRAHEDRON_VERTICES, np.float32)
    _, _, state = R.smooth(v, R.TETRAHEDRON, 1, "laplacian", lam=1.0, states=True)
    p = v.astype(np.float64)
    for i in range(4):
        a, b, c = (p[j] for j in range(4) if j != i)                                        # ascending: the contract's order
        m = ((0.0 + a) + b + c) / 3.0
        want = p[i] + 1.0 * (m - p[i])
        assert state[i].tobytes() == want.tobytes(), i                                      # fp64 bits
    out, info = R.smooth(v, R.TETRAHEDRON, 1, "laplacian", lam=1.0)
    assert out.tobytes() == state.astype(np.float32).tobytes() and info == dict(moved=4, frozen_boundary=0, steps=1, edges=6)
    # one triangle: every vertex is on the boundary - frozen with "fixed", moving with "free"
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    out, info = R.smooth(tri, R.TRIANGLE, 3)
    assert out.tobytes() == tri.tobytes() and info == dict(moved=0, frozen_boundary=3, steps=6, edges=3)
    out, info = R.smooth(tri, R.TRIANGLE, 1, "laplacian", boundary="free")
    assert out.tolist() == [[0.25, 0.25, 0.0], [0.5, 0.25, 0.0], [0.25, 0.5, 0.0]] and info == dict(moved=3, frozen_boundary=0, steps=1, edges=3)
    # a non-finite vertex is frozen, keeps its bits and is left out of its neighbours' means; a vertex with no finite neighbour is frozen
    bad = tri.copy()
    bad[2, 1] = np.nan
    out, info = R.smooth(bad, R.TRIANGLE, 1, "laplacian", boundary="free")
    assert out[:2].tolist() == [[0.5, 0.0, 0.0], [0.5, 0.0, 0.0]] and out[2].tobytes() == bad[2].tobytes() and info["moved"] == 2
    bad[1, 0] = np.inf
    out, info = R.smooth(bad, R.TRIANGLE, 2, boundary="free")
    assert out.tobytes() == bad.tobytes() and info["moved"] == 0


FIGURES = {     # name: vertices, faces, edges, boundary edges, boundary vertices, non-manifold, inconsistent, euler, loops
    "sphere12": (970, 1936, 2904, 0, 0, 0, 0, 2, 0),
    "sphere24": (4848, 9692, 14538, 0, 0, 0, 0, 2, 0),
    "open12": (590, 1124, 1713, 54, 54, 0, 0, 1, 1),
}


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_restated_report_of_the_analytic_meshes(name):
    v, f, _ = R.field_mesh(name)
    report = R.topology(f, len(v))
    print(name, report)
    got = tuple(report[k] for k in ("vertices", "faces", "edges", "boundary_edges", "boundary_vertices", "nonmanifold_edges", "inconsistent_edges",
                                    "euler", "boundary_loops"))
    assert got == FIGURES[name]
    assert report["closed"] == (name != "open12") and report["oriented"] and report["unreferenced_vertices"] == 0 and report["degenerate_faces"] == 0
    starts, nbrs, _, _ = R.mesh_edges(f, len(v))
    degree = np.diff(starts)
    assert degree.sum() == 2 * report["edges"]
    if name == "sphere12":
        assert (degree.min(), degree.max(), int(degree.sum())) == (4, 8, 5808)


def test_restated_report_of_the_random_volume():
    v, f, _ = R.field_mesh("random")
    report = R.topology(f, len(v))
    print("random volume", report)
    assert (report["vertices"], report["faces"], report["edges"], report["boundary_edges"], report["nonmanifold_edges"]) == (1120, 1676, 2839, 650, 0)


@pytest.fixture(scope="module")
def noisy_sphere():
    """the 24^3 sphere with radial noise, computed once and left unchanged"""
    v, f, centre = R.field_mesh("sphere24")
    noisy = R.radial_noise(v, centre, 9.3)
    return noisy, f, centre


def test_restated_taubin_denoises_and_keeps_the_volume(noisy_sphere):
    """the bars: the mean distance to the sphere falls to <= 0.5 of the noisy mesh's (measured: 0.1190 -> 0.0471, a ratio of 0.396), the signed
    volume stays within 1 % of the noisy mesh's (3351.06 -> 3356.38)"""
    noisy, f, centre = noisy_sphere
    d0, vol0 = R.sphere_distance_mean(noisy, centre, 9.3), R.signed_volume(noisy, f)
    out, info = R.smooth(noisy, f, 10)
    d1, vol1 = R.sphere_distance_mean(out, centre, 9.3), R.signed_volume(out, f)
    print(f"taubin x 10: mean distance {d0:.4f} -> {d1:.4f} (ratio {d1 / d0:.3f}), signed volume {vol0:.2f} -> {vol1:.2f}; {info}")
    assert abs(d0 - 0.1190) < 5e-4 and abs(d1 - 0.0471) < 5e-4                              # what the prototype measured
    assert d1 <= 0.5 * d0 and abs(vol1 - vol0) <= 0.01 * vol0
    assert info == dict(moved=4848, frozen_boundary=0, steps=20, edges=14538)


def test_restated_laplacian_shrinks(noisy_sphere):
    """the shrinkage Taubin's second step exists to avoid: 20 Laplacian steps lose more than 4 % of the volume (measured: 3351.06 -> 3166.0)"""
    noisy, f, centre = noisy_sphere
    vol0 = R.signed_volume(noisy, f)
    out, info = R.smooth(noisy, f, 20, "laplacian")
    vol1 = R.signed_volume(out, f)
    print(f"laplacian x 20: signed volume {vol0:.2f} -> {vol1:.2f} ({vol1 / vol0:.4f})")
    assert abs(vol1 - 3166.0) < 1.0 and vol1 < 0.96 * vol0 and info["steps"] == 20


def test_restated_boundary_modes_on_the_open_mesh():
    v, f, _ = R.field_mesh("open12")
    on_boundary = R.boundary_vertices(f, len(v))
    assert on_boundary.sum() == 54
    fixed, info = R.smooth(v, f, 3)
    moved = (fixed.view(np.uint32) != v.view(np.uint32)).any(1)
    assert info == dict(moved=536, frozen_boundary=54, steps=6, edges=1713)
    assert not moved[on_boundary].any() and moved[~on_boundary].all()                        # all 54 keep their bits, the other 536 move
    free, info = R.smooth(v, f, 3, boundary="free")
    assert info == dict(moved=590, frozen_boundary=0, steps=6, edges=1713) and (free.view(np.uint32) != v.view(np.uint32)).any(1).all()
