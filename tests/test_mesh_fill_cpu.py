"""Mesh hole filling (csrc/mesh_fill.hip, cer-mvs_amd/mesh.py mesh_holes / fill_holes), the parts that need no GPU: the three
entry points of ABI 1220 and their argument checks in the documented order, the Python layer's ValueErrors and the forms of the
"fill_holes" option, and the numpy restatement of tests/mesh_fill_reference.py - which the GPU tests hold the device to, bit for bit -
held to results written out by hand, to the figures of the analytic meshes and to the quality bar of the issue
(profiles/mesh_fill_parity.json)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import mesh_fill_reference as R
import mesh_smooth_reference as S
from conftest import REPO

BIG = 1 << 31
NAMES = ("cer_mesh_hole_next_i32", "cer_mesh_hole_heads_i32", "cer_mesh_hole_fill_f32")
KERNELS = ("mesh_hole_next_kernel", "mesh_hole_heads_kernel", "mesh_hole_fill_kernel")


@pytest.fixture(scope="module")
def parity():
    return json.load(open(os.path.join(REPO, "profiles", "mesh_fill_parity.json")))


# ---------------------------------------------------------------- ABI
def test_fill_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    names = L.exported_symbols()
    for n in NAMES:
        assert n in names and re.search(r"\bint %s\(" % n, hdr), n
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P                 # a stream: the last argument
    assert L.ABI_VERSION >= 1220 and "Mesh hole filling (ABI 1220" in hdr and len(names) >= 123
    lib = L.load()
    assert lib.cer_abi_version() == L.ABI_VERSION
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(names)} entry points" in open(os.path.join(REPO, doc)).read(), doc
    csrc = os.path.join(REPO, "cer-mvs_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "mesh_fill.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert re.search(r"^mesh_fill\.o: CXXFLAGS \+= -fno-slp-vectorize$", mk, re.M) and "-ffast-math" not in mk
    src = open(os.path.join(csrc, "mesh_fill.hip")).read()
    for kernel in KERNELS:
        assert "void " + kernel in src, kernel
    assert not re.search(r"atomic\w*\s*\(|\bfmaf?\s*\(|__shared__|__syncthreads", src)        # registers only, in the whole file
    assert not re.search(r"^[ \t]*#[ \t]*ifndef", src, re.M)                                    # no overridable switch


def test_fill_entry_points_refuse_bad_arguments_in_the_documented_order():
    """every check runs before any launch (the pointers are fake: a launch would fault).  The order: (1) a negative size CER_EINVAL (-1); (2)
    nv, nn, nh, nv + added_vertices or 3 (nf + added_faces) >= 2^31, nh > nv, added_vertices > nh or max_edges < 3 CER_ESHAPE (-2); (3)
    nothing to do CER_OK; (4) null pointers CER_EINVAL - each case breaks one rule and every later one, and gets the earlier rule's answer."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    third = (BIG + 2) // 3

    def nxt(starts=fake, nbrs=fake, along=fake, against=fake, nv=5, nn=6, out=fake):
        return lib.cer_mesh_hole_next_i32(starts, nbrs, along, against, nv, nn, out, null)
    nn_ = dict(starts=null, nbrs=null, along=null, against=null, out=null)
    for kw in (dict(nv=-1), dict(nn=-1), dict(nv=-1, nn=BIG), dict(nn=-1, nv=BIG)):                                                   # 1
        assert nxt(**kw) == -1 and nxt(**kw, **nn_) == -1, kw
    for kw in (dict(nv=BIG), dict(nn=BIG), dict(nv=0, nn=BIG), dict(nv=1 << 62)):                                                     # 2
        assert nxt(**kw) == -2 and nxt(**kw, **nn_) == -2, kw
    assert nxt(nv=0) == 0 and nxt(nv=0, **nn_) == 0 and nxt(nv=0, nn=0, **nn_) == 0                                                   # 3
    for name in nn_:                                                                                                                  # 4
        assert nxt(**{name: null}) == -1, name
    assert nxt(nn=0, nbrs=null, along=null, against=null, starts=null) == -1                 # no edge: the lists may be null, the rest not
    assert nxt(nn=0, nbrs=null, along=null, against=null, out=null) == -1

    def heads(table=fake, ver=fake, nv=5, max_edges=8, length=fake):
        return lib.cer_mesh_hole_heads_i32(table, ver, nv, max_edges, length, null)
    hn = dict(table=null, ver=null, length=null)
    for kw in (dict(nv=-1), dict(nv=-1, max_edges=2), dict(nv=-1, max_edges=-5)):                                                     # 1
        assert heads(**kw) == -1 and heads(**kw, **hn) == -1, kw
    for kw in (dict(nv=BIG), dict(max_edges=2), dict(max_edges=0), dict(max_edges=-1), dict(nv=0, max_edges=2), dict(nv=BIG, max_edges=2)):   # 2
        assert heads(**kw) == -2 and heads(**kw, **hn) == -2, kw
    assert heads(nv=0) == 0 and heads(nv=0, **hn) == 0 and heads(nv=0, max_edges=3, **hn) == 0                                        # 3
    for name in ("table", "length"):                                                                                                  # 4
        assert heads(**{name: null}) == -1 and heads(**{name: null}, ver=null) == -1, name       # (vertices: null iff absent)

    def fill(table=fake, hd=fake, ln=fake, fo=fake, vo=fake, nh=2, ver=fake, col=fake, nv=5, nf=4, av=1, af=5, ov=fake, of=fake, hole=fake, oc=fake):
        return lib.cer_mesh_hole_fill_f32(table, hd, ln, fo, vo, nh, ver, col, nv, nf, av, af, ov, of, hole, oc, null)
    required = dict(table=null, hd=null, ln=null, fo=null, vo=null, of=null, hole=null)
    fn = dict(required, ver=null, col=null, ov=null, oc=null)
    for kw in (dict(nh=-1), dict(nv=-1), dict(nf=-1), dict(av=-1), dict(af=-1), dict(nh=-1, nv=BIG), dict(af=-1, nf=third), dict(av=-1, nh=9)):   # 1
        assert fill(**kw) == -1 and fill(**kw, **fn) == -1, kw
    for kw in (dict(nv=BIG), dict(nh=6), dict(nh=BIG, nv=BIG - 1), dict(av=3), dict(nv=BIG - 1, av=1), dict(nf=third), dict(af=third),
               dict(nf=third - 3, af=5), dict(nh=0, nv=BIG), dict(nh=0, av=1)):                                                       # 2
        assert fill(**kw) == -2 and fill(**kw, **fn) == -2, kw
    assert fill(nf=third - 6, af=5, nh=0, av=0) == 0                                         # 3 (nf + added_faces) = 2^31 - 2: the last that fits
    assert fill(nh=0, av=0) == 0 and fill(nh=0, av=0, **fn) == 0 and fill(nh=0, av=0, af=0, nv=0, nf=0, **fn) == 0                    # 3
    for name in required:                                                                                                             # 4
        assert fill(**{name: null}) == -1, name
    assert fill(ver=null) == -1 and fill(ov=null) == -1                                      # a centre to write: both needed
    assert fill(col=null) == -1 and fill(oc=null) == -1                                      # colours: both or neither
    assert fill(av=0, ver=null, ov=null, hd=null) == -1 and fill(col=null, oc=null, ln=null) == -1     # the optional ones absent, a required one too


# ---------------------------------------------------------------- the Python layer
def test_fill_python_layer_refuses_bad_arguments_without_a_device():
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    ver = torch.zeros(5, 3)
    col = torch.zeros(5, 3, dtype=torch.uint8)
    fac = torch.tensor(R.PAIR, dtype=torch.int32)
    out_of_range = (torch.tensor([[0, 1, 5]], dtype=torch.int32), torch.tensor([[0, -1, 2]], dtype=torch.int32))
    mh, fh = ME.mesh_holes, ME.fill_holes
    for bad in (fac.long(), fac[:, :2], fac[0], fac.numpy(), None):
        with pytest.raises(ValueError, match="vertex_faces: faces"):                        # mesh_edges' rule, in its wording
            mh(bad, 5, 8)
        with pytest.raises(ValueError, match="faces"):
            fh(ver, bad, 8)
    for bad in out_of_range:
        with pytest.raises(ValueError, match="vertex_faces: faces must hold indices"):
            mh(bad, 5, 8)
        with pytest.raises(ValueError, match="vertex_faces: faces must hold indices"):
            fh(ver, bad, 8)
    for bad in (-1, 1 << 31):
        with pytest.raises(ValueError, match="vertex_faces: nv"):
            mh(fac, bad, 8)
    big = torch.zeros(1, dtype=torch.int32).expand((BIG + 5) // 6, 3)                        # (an expanded view: no memory behind it, refused by its size)
    with pytest.raises(ValueError, match="6 nf"):
        mh(big, 5, 8)
    with pytest.raises(ValueError, match="6 nf"):
        fh(ver, big, 8)
    for bad in (2, 0, -1, 3.0, 8.5, True, False, "8", None, [8]):
        with pytest.raises(ValueError, match="max_edges must be an integer >= 3"):
            mh(fac, 5, bad)
        with pytest.raises(ValueError, match="max_edges must be an integer >= 3"):
            fh(ver, fac, bad)
    for bad in (ver.double(), ver[:, :2], ver[0], ver.numpy()):
        with pytest.raises(ValueError, match="vertices"):
            mh(fac, 5, 8, vertices=bad)
    with pytest.raises(ValueError, match="vertices float32 \\[5, 3\\]"):
        mh(fac, 5, 8, vertices=ver[:4])
    for bad in (ver.double(), ver[:, :2], ver[0], ver.numpy(), None):
        with pytest.raises(ValueError, match="vertices"):
            fh(bad, fac, 8)
    for bad in (col.float(), col[:4], col[:, :2], col.numpy()):
        with pytest.raises(ValueError, match="colors"):
            fh(ver, fac, 8, colors=bad)
    for call in (lambda: mh(fac, 5, 3), lambda: mh(fac, 5, np.int64(64), vertices=ver), lambda: mh(fac[:0], 0, 8), lambda: mh(fac, 5, 1 << 40),
                 lambda: fh(ver, fac, 3), lambda: fh(ver, fac, 1000, colors=col, info={}), lambda: fh(ver[:0], fac[:0], 8)):
        with pytest.raises(RuntimeError, match="CUDA"):      # good arguments: the host tensors are what is refused
            call()
    # the option of reconstruct_scan(mesh=...): refused before a model or a session is built
    for bad in (2, 0, -3, 3.0, 16.5, True, False, "16", None, [16], {}, {"max_edges": 16}):
        with pytest.raises(ValueError, match="mesh: fill_holes"):
            ME.mesh_options({"fill_holes": bad})
        with pytest.raises(ValueError, match="mesh: fill_holes"):
            reconstruct_scan(None, [0], [0], [0], ["a"], [[0]], [1.0], None, write=False, mesh={"resolution": 48, "fill_holes": bad})
    for bad in ({"fill": 16}, {"holes": 16}, {"max_edges": 16}):
        with pytest.raises(ValueError, match="unknown"):
            ME.mesh_options(bad)
    for good in ({"fill_holes": 3}, {"fill_holes": 32}, {"resolution": 48, "min_component": 157, "fill_holes": 32, "smooth": 3, "simplify": 2,
                                                          "colors": True, "normals": True, "topology": True}):
        assert ME.mesh_options(good) == good
    assert "fill_holes" in ME.MESH_OPTION_KEYS and ME.mesh_options({"resolution": 48}) == {"resolution": 48}
    assert ME.FILL_INFO_KEYS == R.INFO_KEYS
    for fn in (mh, fh):
        assert "remove_small_components" in fh.__doc__ and "Mesh hole filling" in fn.__doc__      # small pieces first: said where it is read


# ---------------------------------------------------------------- the restatement, by hand
def filled(vertices, faces, max_edges, colors=None):
    (v, f, hole, c), info = R.fill(vertices, faces, max_edges, colors)
    assert v.dtype == np.float32 and f.dtype == np.int32 and hole.dtype == np.int32 and tuple(info) == R.INFO_KEYS
    nv, nf = len(R.as_vertices(vertices)), len(R.as_faces(faces))
    assert v[:nv].tobytes() == R.as_vertices(vertices).tobytes() and f[:nf].tobytes() == R.as_faces(faces).tobytes()
    assert (hole[:nf] == -1).all() and len(hole) == len(f) and len(v) == nv + info["added_vertices"] and len(f) == nf + info["added_faces"]
    assert (c is None) == (colors is None) and (c is None or (c.dtype == np.uint8 and c[:nv].tobytes() == np.asarray(colors).tobytes()))
    return v, f, hole, c, info


def test_restated_fill_on_hand_made_meshes():
    none = np.zeros((0, 3), np.float32)
    v, f, hole, _, info = filled(none, [], 8)
    assert len(v) == 0 and len(f) == 0 and info == dict(holes=0, added_vertices=0, added_faces=0, pinched_vertices=0, boundary_edges_before=0)
    assert [a.tolist() for a in R.mesh_holes([], 0, 8)] == [[], []] and [a.tolist() for a in R.mesh_holes([], 4, 8)] == [[], []]
    # one triangle: the two-faced closed pillow
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    assert R.next_table(S.TRIANGLE, 3).tolist() == [1, 2, 0] and [a.tolist() for a in R.mesh_holes(S.TRIANGLE, 3, 3)] == [[0], [3]]
    v, f, hole, _, info = filled(tri, S.TRIANGLE, 3)
    assert f.tolist() == [[0, 1, 2], [0, 2, 1]] and hole.tolist() == [-1, 0] and len(v) == 3
    assert info == dict(holes=1, added_vertices=0, added_faces=1, pinched_vertices=0, boundary_edges_before=3)
    report = S.topology(f, 3)
    assert report["closed"] and report["oriented"] and report["euler"] == 2
    # two triangles on one edge: the hole 0, 1, 3, 2 and its fan around vertex 4
    pv = np.array(R.PAIR_VERTICES, np.float32)
    assert R.boundary_half_edges(R.PAIR) == [(0, 1), (1, 3), (2, 0), (3, 2)] and R.next_table(R.PAIR, 4).tolist() == [1, 3, 0, 2]
    assert R.cycles(R.next_table(R.PAIR, 4)) == [[0, 1, 3, 2]] and [a.tolist() for a in R.mesh_holes(R.PAIR, 4, 4)] == [[0], [4]]
    col = np.array([[10, 0, 255], [11, 1, 255], [12, 2, 254], [14, 0, 255]], np.uint8)
    v, f, hole, c, info = filled(pv, R.PAIR, 4, col)
    assert f[2:].tolist() == [[1, 0, 4], [3, 1, 4], [2, 3, 4], [0, 2, 4]] and hole.tolist() == [-1, -1, 0, 0, 0, 0] and len(v) == 5
    p = pv.astype(np.float64)
    want = ((((0.0 + p[0]) + p[1]) + p[3]) + p[2]) / 4.0                                       # cycle order, not index order
    assert v[4].tobytes() == want.astype(np.float32).tobytes() and c[4].tolist() == [47 // 4, 3 // 4, 1019 // 4]
    assert info == dict(holes=1, added_vertices=1, added_faces=4, pinched_vertices=0, boundary_edges_before=4)
    report = S.topology(f, 5)
    assert report["closed"] and report["oriented"] and report["euler"] == 2 and report["edges"] == 9
    assert filled(pv, R.PAIR, 3)[4]["holes"] == 0                                              # four edges are more than three
    # a sum whose order shows in the bits
    B = float(np.float32(1e17))
    odd = np.array([[B, 0, 0], [1.0, 0, 0], [-B, 0, 0], [0.25, 0, 0]], np.float32)
    v, _, _, _, _ = filled(odd, R.PAIR, 8)
    assert ((((0.0 + B) + 1.0) + -B) + 0.25) / 4.0 == 0.0625 and ((((0.0 + B) + 1.0) + 0.25) + -B) / 4.0 == 0.0       # index order, cycle order
    assert v[4, 0] == 0.0
    # pinched vertices: nothing is filled
    for faces, nv, pinched, table in ((R.PAIR_OPPOSITE, 4, 2, [1, -2, -2, 1]), (R.FAN_OF_THREE, 5, 2, [-2, -2, 0, 1, 0]), (R.BOW_TIE, 5, 1, [-2, 2, 0, 4, 0])):
        assert R.next_table(faces, nv).tolist() == table
        v, f, hole, _, info = filled(np.arange(3 * nv, dtype=np.float32).reshape(nv, 3), faces, 1000)
        assert len(v) == nv and f.tolist() == faces and info["holes"] == 0 and info["pinched_vertices"] == pinched and info["added_faces"] == 0
    # a tetrahedron: closed, unchanged
    tet = np.array(S.TETRAHEDRON_VERTICES, np.float32)
    v, f, hole, _, info = filled(tet, S.TETRAHEDRON, 64)
    assert (R.next_table(S.TETRAHEDRON, 4) == -1).all() and f.tolist() == S.TETRAHEDRON and len(v) == 4
    assert info == dict(holes=0, added_vertices=0, added_faces=0, pinched_vertices=0, boundary_edges_before=0)
    # an unreferenced vertex has no successor; two separate triangles are two holes in head order
    assert R.next_table(S.TRIANGLE, 5).tolist() == [1, 2, 0, -1, -1]
    v, f, hole, _, info = filled(np.zeros((6, 3), np.float32), [[3, 4, 5], [0, 1, 2]], 3)
    assert f[2:].tolist() == [[0, 2, 1], [3, 5, 4]] and hole.tolist() == [-1, -1, 0, 1] and info["holes"] == 2
    # a planted NaN on the loop: skipped with vertices given, seen without
    bad = pv.copy()
    bad[3, 1] = np.nan
    assert [a.tolist() for a in R.mesh_holes(R.PAIR, 4, 8, bad)] == [[], []] and [a.tolist() for a in R.mesh_holes(R.PAIR, 4, 8)] == [[0], [4]]
    v, f, _, _, info = filled(bad, R.PAIR, 8)
    assert len(v) == 4 and len(f) == 2 and info == dict(holes=0, added_vertices=0, added_faces=0, pinched_vertices=0, boundary_edges_before=4)


# ---------------------------------------------------------------- the restatement, on the analytic meshes
FIELD_FIGURES = {     # (name, max_edges): hole lengths in head order, (nv', nf'), boundary edges left, pinched
    ("open12", 3): ([], (590, 1124), 54, 0), ("open12", 8): ([], (590, 1124), 54, 0),
    ("open12", 64): ([54], (591, 1178), 0, 0), ("open12", 1000): ([54], (591, 1178), 0, 0),
    ("random", 3): ([], (1120, 1676), 650, 6), ("random", 8): ([4, 6, 6, 4], (1124, 1696), 630, 6),
    ("random", 64): ([56, 4, 10, 6, 6, 4, 14], (1127, 1776), 550, 6), ("random", 1000): ([136, 56, 70, 4, 10, 6, 6, 4, 14], (1129, 1982), 344, 6),
    ("sphere12", 3): ([], (970, 1936), 0, 0), ("sphere12", 8): ([], (970, 1936), 0, 0),
    ("sphere12", 64): ([], (970, 1936), 0, 0), ("sphere12", 1000): ([], (970, 1936), 0, 0),
}


@pytest.fixture(scope="module")
def fields():
    """the three small analytic meshes, computed once and left unchanged"""
    return {name: S.field_mesh(name) for name in ("open12", "random", "sphere12")}


@pytest.mark.parametrize("name", ("open12", "random", "sphere12"))
def test_restated_fill_of_the_analytic_meshes(fields, parity, name):
    v, f, _ = fields[name]
    before = S.topology(f, len(v))
    for max_edges in (3, 8, 64, 1000):
        lengths, sizes, left, pinched = FIELD_FIGURES[(name, max_edges)]
        heads, lens = R.mesh_holes(f, len(v), max_edges, v)
        ov, of, hole, oc, info = filled(v, f, max_edges, R.random_colors(len(v)))
        report = S.topology(of, len(ov))
        print(name, max_edges, lens.tolist(), info, report)
        assert lens.tolist() == lengths and (np.diff(heads) > 0).all() and (len(ov), len(of)) == sizes
        assert info == dict(holes=len(lengths), added_vertices=sum(n > 3 for n in lengths), added_faces=sum(1 if n == 3 else n for n in lengths),
                            pinched_vertices=pinched, boundary_edges_before=before["boundary_edges"])
        assert report["boundary_edges"] == left == before["boundary_edges"] - sum(lengths)          # every filled edge became interior
        assert report["oriented"] == before["oriented"] and report["nonmanifold_edges"] == before["nonmanifold_edges"] == 0
        assert report["euler"] == before["euler"] + len(lengths) and report["boundary_loops"] == before["boundary_loops"] - len(lengths)
        assert np.bincount(hole[len(f):], minlength=len(lengths)).tolist() == [1 if n == 3 else n for n in lengths]
        assert parity["fields"][f"{name}/{max_edges}"] == dict(lengths=lengths, vertices=sizes[0], faces=sizes[1], boundary_edges_left=left,
                                                                pinched_vertices=pinched)
    if name == "open12":
        report = S.topology(filled(v, f, 64)[1], 591)
        assert report["closed"] and report["euler"] == 2
    if name == "sphere12":
        assert filled(v, f, 1000)[1].tobytes() == f.tobytes()                                  # unchanged


@pytest.fixture(scope="module")
def punched24():
    """the punched 24^3 sphere and the unpunched one, computed once and left unchanged"""
    return R.punched_sphere(24, 9.3, 12)


def test_restated_fill_closes_the_punched_sphere(punched24, parity):
    (v, f), (wv, wf) = punched24
    before = S.topology(f, len(v))
    lengths = R.mesh_holes(f, len(v), 1000, v)[1].tolist()
    assert (len(v), len(f), before["boundary_loops"], before["euler"]) == (4713, 9252, 9, -7) and len(lengths) == 9
    assert (min(lengths), max(lengths)) == (14, 30) and sum(lengths) == before["boundary_edges"] == 188
    ov, of, _, _, info = filled(v, f, 16)
    assert info["holes"] == 4 and S.topology(of, len(ov))["boundary_loops"] == 5
    ov, of, _, _, info = filled(v, f, 64)
    report = S.topology(of, len(ov))
    assert info == dict(holes=9, added_vertices=9, added_faces=188, pinched_vertices=0, boundary_edges_before=188)
    assert report["closed"] and report["oriented"] and report["euler"] == 2 and report["nonmanifold_edges"] == 0 and (len(ov), len(of)) == (4722, 9440)
    # the quality bar: the caps face outward and none is missing - the signed volume within 0.5 % of the unpunched mesh's
    vol, whole = S.signed_volume(ov, of), S.signed_volume(wv, wf)
    print(f"punched 24^3 sphere, max_edges = 64: signed volume {vol:.2f} against {whole:.2f} unpunched ({abs(vol - whole) / whole:.4%})")
    assert abs(vol - whole) <= 0.005 * whole
    assert abs(vol - 3347.03) < 0.01 and abs(whole - 3349.79) < 0.01                           # what the prototype measured
    assert abs(parity["punched24"]["signed_volume"] - vol) < 1e-6 and abs(parity["punched24"]["signed_volume_unpunched"] - whole) < 1e-6
    assert parity["punched24"]["lengths"] == lengths
