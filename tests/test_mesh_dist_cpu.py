"""Exact point-to-mesh distance (csrc/mesh_dist.hip, csrc/grid_walk.hpp, cer-mvs_amd/mesh.py MeshIndex / mesh_distances /
evaluate_mesh(method="exact")), the parts that need no GPU: the four entry points of ABI 1240 and their argument checks in
the documented order, the Python layer's ValueErrors, and the numpy restatement of tests/mesh_dist_reference.py - which the GPU tests hold
the device to, bit for bit - held to answers worked out by hand, to exact rational arithmetic and to its own brute force through the
index's boxes (profiles/mesh_dist_parity.json)."""
import ctypes
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import mesh_dist_reference as D
import mesh_smooth_reference as S
from conftest import REPO

BIG = 1 << 31
NAMES = ("cer_mesh_tri_cells_i64", "cer_mesh_tri_pairs_i64", "cer_mesh_tri_pack_f32", "cer_mesh_tri_nearest_f32")
KERNELS = ("mesh_tri_cells_kernel", "mesh_tri_pairs_kernel", "mesh_tri_pack_kernel", "mesh_tri_nearest_kernel")
MOVED = ("struct GridView", "#define GRID_EPS", "double grid_gap(", "long grid_lower_bound(", "bool grid_row_span(", "GridHome grid_home(",
         "void grid_walk_rows(", "void grid_walk_home_first(", "long long grid_key(", "#define GRID_B ")
RIGHT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)


@pytest.fixture(scope="module")
def parity():
    return json.load(open(os.path.join(REPO, "profiles", "mesh_dist_parity.json")))


# ---------------------------------------------------------------- ABI
def test_dist_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    names = L.exported_symbols()
    for n in NAMES:
        assert n in names and re.search(r"\bint %s\(" % n, hdr), n
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P                 # a stream: the last argument
    assert L.ABI_VERSION >= 1240 and "Mesh distance (ABI 1240" in hdr and len(names) >= 130
    assert re.search(r"^#define CER_TRI_MAX_CELLS 4096$", hdr, re.M) and D.MAX_CELLS == 4096
    lib = L.load()
    assert lib.cer_abi_version() == L.ABI_VERSION
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(REPO, doc)).read()
        assert f"{len(names)} entry points" in text and "3zh" in text, doc
    csrc = os.path.join(REPO, "cer-mvs_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "mesh_dist.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert re.search(r"^mesh_dist\.o: CXXFLAGS \+= -fno-slp-vectorize$", mk, re.M) and "-ffast-math" not in mk
    assert re.search(r"^cloud_eval\.o mesh_dist\.o: grid_walk\.hpp$", mk, re.M)
    src = open(os.path.join(csrc, "mesh_dist.hip")).read()
    for kernel in KERNELS:
        assert "void " + kernel in src, kernel
    # registers only, in the whole file; no fused multiply-add; no overridable switch
    assert not re.search(r"atomic|__shared__|__syncthreads|\bfmaf?\s*\(", src)
    assert not re.search(r"^[ \t]*#[ \t]*ifndef", src, re.M)
    # the walk has one copy: in grid_walk.hpp, which both users include
    walk = open(os.path.join(csrc, "grid_walk.hpp")).read()
    cloud = open(os.path.join(csrc, "cloud_eval.hip")).read()
    for text in MOVED:
        assert text in walk and text not in cloud and text not in src, text
    assert '#include "grid_walk.hpp"' in cloud and '#include "grid_walk.hpp"' in src and "#pragma once" in walk
    same = open(os.path.join(REPO, "profiles", "mesh_dist_asm_identity.txt")).read()
    assert re.search(r"^cloud_eval\.o .* same$", same, re.M) and "DIFFERENT" not in same and re.search(r"^(\d+) of \1 objects same$", same, re.M)


def test_dist_entry_points_refuse_bad_arguments_in_the_documented_order():
    """every check runs before any launch (the pointers are fake: a launch would fault).  The order: (1) a negative size, a frame or a
    cut-off that is no number of its kind CER_EINVAL (-1); (2) nv, 3 nf, npairs or m >= 2^31, more cells than pairs, too many rings
    CER_ESHAPE (-2); (3) nothing to do CER_OK; (4) null pointers CER_EINVAL, then records off a 16-byte boundary CER_EALIGN (-3) - each
    case breaks one rule and every later one, and gets the earlier rule's answer."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, odd, null = ctypes.c_void_p(4096), ctypes.c_void_p(4104), None
    third = (BIG + 2) // 3                                                                     # the first nf with 3 nf >= 2^31
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    bad_org = (ctypes.c_double * 3)(0.0, math.nan, 0.0)
    inf = math.inf

    def cells(ver=fake, nv=5, fac=fake, nf=4, areas=fake, origin=org, cell=1.0, out=fake, flag=fake):
        return lib.cer_mesh_tri_cells_i64(ver, nv, fac, nf, areas, origin, cell, out, flag, null)
    cn = dict(ver=null, fac=null, areas=null, out=null, flag=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(cell=0.0), dict(cell=-1.0), dict(cell=inf), dict(cell=math.nan), dict(origin=bad_org),
               dict(origin=null), dict(nv=-1, nf=third), dict(cell=0.0, nv=BIG), dict(origin=null, nf=0)):                                # 1
        assert cells(**kw) == -1 and cells(**kw, **cn) == -1, kw
    for kw in (dict(nv=BIG), dict(nf=third), dict(nf=0, nv=BIG), dict(nf=1 << 62)):                                                       # 2
        assert cells(**kw) == -2 and cells(**kw, **cn) == -2, kw
    assert cells(nf=0) == 0 and cells(nf=0, **cn) == 0 and cells(nf=0, nv=0, **cn) == 0                                                   # 3
    for name in cn:                                                                                                                       # 4
        assert cells(**{name: null}) == -1, name
    assert cells(nv=0, ver=null, fac=null) == -1                                             # no vertex: vertices may be null, the rest not

    def pairs(ver=fake, nv=5, fac=fake, nf=4, areas=fake, origin=org, cell=1.0, cum=fake, npairs=9, keys=fake, ids=fake):
        return lib.cer_mesh_tri_pairs_i64(ver, nv, fac, nf, areas, origin, cell, cum, npairs, keys, ids, null)
    pn = dict(ver=null, fac=null, areas=null, cum=null, keys=null, ids=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(npairs=-1), dict(cell=0.0), dict(origin=bad_org), dict(origin=null), dict(npairs=-1, nf=third),
               dict(cell=math.nan, npairs=BIG)):                                                                                          # 1
        assert pairs(**kw) == -1 and pairs(**kw, **pn) == -1, kw
    for kw in (dict(nv=BIG), dict(nf=third), dict(npairs=BIG), dict(npairs=0, nv=BIG), dict(nf=0, npairs=BIG)):                          # 2
        assert pairs(**kw) == -2 and pairs(**kw, **pn) == -2, kw
    for kw in (dict(nf=0), dict(npairs=0), dict(nf=0, npairs=0, nv=0)):                                                                   # 3
        assert pairs(**kw) == 0 and pairs(**kw, **pn) == 0, kw
    for name in pn:                                                                                                                       # 4
        assert pairs(**{name: null}) == -1, name
    assert pairs(nv=0, ver=null, cum=null) == -1

    def pack(ver=fake, nv=5, fac=fake, nf=4, rec=fake):
        return lib.cer_mesh_tri_pack_f32(ver, nv, fac, nf, rec, null)
    kn = dict(ver=null, fac=null, rec=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nv=-1, nf=third)):                                                                          # 1
        assert pack(**kw) == -1 and pack(**kw, **kn) == -1, kw
    for kw in (dict(nv=BIG), dict(nf=third), dict(nf=0, nv=BIG)):                                                                         # 2
        assert pack(**kw) == -2 and pack(**kw, **kn) == -2 and pack(**kw, rec=odd) == -2, kw
    assert pack(nf=0) == 0 and pack(nf=0, **kn) == 0 and pack(nf=0, rec=odd) == 0                                                         # 3
    for name in kn:                                                                                                                       # 4
        assert pack(**{name: null}) == -1, name
    assert pack(rec=odd) == -3 and pack(rec=odd, fac=null) == -1 and pack(nv=0, ver=null, rec=odd) == -3

    def near(rec=fake, nf=4, pf=fake, npairs=9, ck=fake, cs=fake, ncells=3, origin=org, cell=1.0, qs=fake, qo=fake, m=7, reach=2.0, face=fake,
             dist=fake, closest=fake):
        return lib.cer_mesh_tri_nearest_f32(rec, nf, pf, npairs, ck, cs, ncells, origin, cell, qs, qo, m, reach, face, dist, closest, null)
    required = dict(rec=null, pf=null, ck=null, cs=null, qs=null, face=null, dist=null)
    nn = dict(required, qo=null, closest=null)
    for kw in (dict(nf=-1), dict(npairs=-1), dict(ncells=-1), dict(m=-1), dict(cell=0.0), dict(cell=inf), dict(origin=bad_org), dict(origin=null),
               dict(reach=-1.0), dict(reach=math.nan), dict(m=-1, nf=third), dict(reach=-1.0, ncells=10), dict(cell=0.0, reach=inf)):    # 1
        assert near(**kw) == -1 and near(**kw, **nn) == -1, kw
    for kw in (dict(nf=third), dict(npairs=BIG), dict(m=BIG), dict(ncells=10), dict(reach=4097.0), dict(reach=inf), dict(cell=1e-3, reach=4.2),
               dict(m=0, nf=third), dict(nf=0, ncells=1, npairs=0), dict(m=0, reach=inf)):                                               # 2
        assert near(**kw) == -2 and near(**kw, **nn) == -2 and near(**kw, rec=odd) == -2, kw
    for kw in (dict(m=0), dict(nf=0), dict(npairs=0, ncells=0), dict(ncells=0), dict(m=0, reach=4096.0), dict(m=0, reach=0.0)):           # 3
        assert near(**kw) == 0 and near(**kw, **nn) == 0 and near(**kw, rec=odd) == 0, kw
    for name in required:                                                                                                                 # 4
        assert near(**{name: null}) == -1, name
    assert near(rec=odd) == -3 and near(rec=odd, qs=null) == -1 and near(rec=odd, qo=null, closest=null) == -3


# ---------------------------------------------------------------- the Python layer
def test_dist_python_layer_refuses_bad_arguments_without_a_device():
    from cer_mvs_amd import mesh as ME
    ver = torch.zeros(5, 3)
    fac = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    qs = torch.zeros(4, 3)
    md, ev = ME.mesh_distances, ME.evaluate_mesh
    calls = (lambda v, f: ME.MeshIndex(v, f, 1.0), lambda v, f: md(v, f, qs, 1.0))
    for call in calls:
        for bad in (ver.double(), ver[:, :2], ver[0], ver.numpy(), None):
            with pytest.raises(ValueError, match="vertices"):
                call(bad, fac)
        for bad in (fac.long(), fac[:, :2], fac[0], fac.numpy(), None):
            with pytest.raises(ValueError, match="faces"):
                call(ver, bad)
        big = torch.zeros(1, dtype=torch.int32).expand((BIG + 2) // 3, 3)                    # (an expanded view: no memory behind it)
        with pytest.raises(ValueError, match="3 nf"):
            call(ver, big)
    for bad in (0, -1.0, math.inf, math.nan, True, "1", [1.0]):
        with pytest.raises(ValueError, match="cell must be a positive finite number"):
            ME.MeshIndex(ver, fac, bad)
        with pytest.raises(ValueError, match="cell must be a positive finite number"):
            md(ver, fac, qs, 1.0, cell=bad)
    for bad in (-1.0, math.nan, True, "1", None, [1.0], -1e-60 - 1e-30):
        with pytest.raises(ValueError, match="max_dist must be a number >= 0"):
            md(ver, fac, qs, bad)
    for bad in (-1.0, math.nan, True, "1"):
        with pytest.raises(ValueError, match="max_dist must be a number >= 0"):
            ME.MeshIndex(ver, fac, None, bad)
    for bad in (qs.double(), qs[:, :2], qs[0], qs.numpy(), None):
        with pytest.raises(ValueError, match="queries float32"):
            md(ver, fac, bad, 1.0)
    with pytest.raises(ValueError, match="info must be a dictionary"):
        md(ver, fac, qs, 1.0, info=[])
    # nearest's own checks, on an index that was never built
    index = ME.MeshIndex.__new__(ME.MeshIndex)
    index.cell, index.pairs, index.cells, index.nf = 0.001, 0, 0, 0
    for bad in (-1.0, math.nan, True, "1", None):
        with pytest.raises(ValueError, match="max_dist must be a number >= 0"):
            index.nearest(qs, bad)
    for name in ("closest", "sort_queries"):
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match=f"{name} must be True or False"):
                index.nearest(qs, 1.0, **{name: bad})
    for bad in (qs.double(), qs[:, :2], qs[0], qs.numpy(), None):
        with pytest.raises(ValueError, match="queries float32"):
            index.nearest(bad, 1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        index.nearest(qs, 1.0)
    # evaluate_mesh: the new argument is checked with the others, before the mesh is looked at
    gt = torch.zeros(4, 3)
    for bad in ("sample", "Exact", "", None, 1, True):
        with pytest.raises(ValueError, match="method must be one of"):
            ev(ver, fac, gt, 0.5, method=bad)
    with pytest.raises(ValueError, match="vertices"):
        ev(None, fac, gt, 0.5, method="exact")
    with pytest.raises(ValueError, match="spacing must be a positive finite"):
        ev(ver, fac, gt, 0, method="exact")
    for call in (lambda: ME.MeshIndex(ver, fac, 1.0), lambda: ME.MeshIndex(ver, fac), lambda: ME.MeshIndex(ver[:0], fac[:0], None, 2.0),
                 lambda: md(ver, fac, qs, 1.0), lambda: md(ver, fac, qs[:0], 0, cell=0.5, info={}), lambda: md(ver, fac, qs, math.inf),
                 lambda: ev(ver, fac, gt, 0.5, method="exact"), lambda: ev(ver, fac, gt, 0.5, tau=1.0, method="samples")):
        with pytest.raises(RuntimeError, match="CUDA"):      # good arguments: the host tensors are what is refused
            call()
    assert ME.DIST_INFO_KEYS == D.INFO_KEYS and ME.TRI_MAX_CELLS == D.MAX_CELLS and ME.EVALUATE_METHODS == ("samples", "exact")
    doc = ev.__doc__
    assert "upward bias" in doc and "future work" in doc and "hierarchy" in doc and "signed distance" in doc
    for fn in (ME.MeshIndex, ME.MeshIndex.nearest, md):
        assert '"Mesh distance"' in fn.__doc__


# ---------------------------------------------------------------- the restatement, by hand
HAND = (  # (x, y) of the query, its region, the closest point, dist2 less z^2
    ((-1.0, -1.0), 1, (0.0, 0.0), 2.0), ((2.0, 0.5), 2, (1.0, 0.0), 1.25), ((0.5, -1.0), 3, (0.5, 0.0), 1.0), ((0.5, 2.0), 4, (0.0, 1.0), 1.25),
    ((-1.0, 0.5), 5, (0.0, 0.5), 1.0), ((1.0, 1.0), 6, (0.5, 0.5), 0.5), ((0.25, 0.25), 7, (0.25, 0.25), 0.0))


def test_restated_distance_worked_out_by_hand():
    a, b, c = (RIGHT[i].astype(np.float64) for i in range(3))
    for z in (0.5, -0.5, 0.0):
        for (x, y), region, (qx, qy), flat in HAND:
            p = np.array([x, y, z])
            d2, q, r = D.closest_on_triangles(a, b, c, p)
            assert int(r) == region and float(d2) == flat + z * z and q.tolist() == [qx, qy, 0.0], (x, y, z)
            e2, eq, er = D.exact_dist2(a.tolist(), b.tolist(), c.tolist(), p.tolist())
            assert er == region and e2 == Fraction(flat + z * z) and [float(t) for t in eq] == [qx, qy, 0.0]
            # the other orientation of the same triangle: the same point and distance
            d2, q, _ = D.closest_on_triangles(a, c, b, p)
            assert float(d2) == flat + z * z and q.tolist() == [qx, qy, 0.0]
    queries = np.array([[x, y, z] for z in (0.5, -0.5) for (x, y), _, _, _ in HAND], np.float32)
    dist, face, near = D.brute(RIGHT, [[0, 1, 2]], queries, 1.5)
    want = [math.sqrt(flat + 0.25) for _ in range(2) for _, _, _, flat in HAND]
    assert dist.tolist() == [float(np.float32(w)) if w * w <= 2.25 else math.inf for w in want]
    assert face.tolist() == [0 if w * w <= 2.25 else -1 for w in want] and face.tolist().count(-1) == 0 and np.isfinite(near).all()
    # the cut-off is inclusive, and the float32 below it is not enough; a query that is not finite gets no face
    assert D.brute(RIGHT, [[0, 1, 2]], [[0.25, 0.25, 0.5]], 0.5)[1].tolist() == [0]
    assert D.brute(RIGHT, [[0, 1, 2]], [[0.25, 0.25, 0.5]], np.nextafter(np.float32(0.5), np.float32(0)))[1].tolist() == [-1]
    assert D.brute(RIGHT, [[0, 1, 2]], [[np.nan, 0, 0], [0, np.inf, 0], [0.25, 0.25, 0]], 0.0)[1].tolist() == [-1, -1, 0]
    # faces that are left out never win; two coincident faces: the lower index
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0]], np.float32)
    f = [[0, 1, 1], [0, 1, 5], [0, -1, 2], [0, 1, 3], [0, 1, 4], [0, 2, 1], [0, 1, 2]]
    dist, face, _ = D.brute(v, f, [[0.25, 0.25, 0.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.0]], 5.0)
    assert face.tolist() == [5, 5, 5] and dist.tolist() == [0.0, 0.0, 2.0] and D.indexed_faces(v, f).tolist() == [False] * 5 + [True] * 2
    assert D.brute(v, f[:5], [[0.25, 0.25, 0.0]], 5.0)[1].tolist() == [-1]


def test_restated_cells_and_pairs_by_hand():
    v = np.array([[0, 0, 0], [2.5, 0, 0], [0, 1.5, 0], [0, 0, 0.5], [-1, 0, 0]], np.float32)
    f = [[0, 1, 2], [0, 1, 1], [3, 1, 2], [0, 2, 4]]
    origin, lo, hi, rows = D.boxes(v, f, 1.0)
    assert origin.tolist() == [-1.0, 0.0, 0.0] and rows.tolist() == [True, False, True, True]
    assert lo.tolist() == [[1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]] and hi.tolist() == [[3, 1, 0], [0, 0, 0], [3, 1, 0], [1, 1, 0]]
    counts, beyond, large = D.cell_counts(v, f, 1.0)
    assert counts.tolist() == [6, 0, 6, 4] and not beyond and not large
    keys, ids = D.pairs(v, f, 1.0)
    assert ids.tolist() == [0] * 6 + [2] * 6 + [3] * 4
    assert keys[:6].tolist() == [D.key_of(x, y, 0) for y in (0, 1) for x in (1, 2, 3)]
    assert D.info_of(v, f, 1.0) == dict(cell=1.0, pairs=16, faces_indexed=3, cells=8)
    # the cap and the key range
    long_v = np.array([[0, 0, 0], [4095.5, 0, 0], [0, 0.5, 0]], np.float32)
    counts, beyond, large = D.cell_counts(long_v, [[0, 1, 2]], 1.0)
    assert counts.tolist() == [4096] and not beyond and not large
    long_v[1, 0] = 4096.5
    assert D.cell_counts(long_v, [[0, 1, 2]], 1.0)[1:] == (False, True)
    assert D.cell_counts(long_v, [[0, 1, 2]], 4096.5 / (1 << 20))[1:] == (True, False)
    assert D.origin_of(v, [[0, 1, 1]]) is None and D.default_cell(v, [[0, 1, 1]], 64.0) == 2.0 and D.default_cell(v, [[0, 1, 1]]) == 1.0


# ---------------------------------------------------------------- the restatement against exact arithmetic
def test_restated_distance_against_exact_rationals(parity):
    """Coordinates are integers in -8 .. 8, so every difference, dot product and va, vb, vc is an exact integer in fp64 and the regions
    are decided exactly.  What rounds, with u = 2^-53: v and w (one division each, region 6's v = 1 - w a second step: at most 2 u off, both
    in [0, 1]); v*ab and w*ac (|ab|, |ac| <= 16: 48 u and 32 u off); the two sums (values up to 24 and 40: 24 u and 40 u more): q is at
    most 144 u off per axis; r = q - p (up to 48: 48 u more): 192 u per axis.  dist2 = sum of three squares of values 192 u off, each
    product and the two sums rounded: |error| <= 2 * 192 u * (|rx| + |ry| + |rz|) + 3 u * dist2 + 3 * (192 u)^2 <= u * (666 * dist + 3 *
    dist2) + 2e-27.  The assertion takes 700 and 4.  On the 3000 random cases a zero of the exact distance must be an exact zero (a
    corner region returns the corner itself).  750 more cases plant the query in the triangle's plane, often on the triangle: there v
    and w round, q misses p by a few u and dist2 comes out as some 1e-31 instead of 0 - the bound holds, an exact zero is not promised;
    how many of the planted zeros come out exact is recorded."""
    rng = np.random.default_rng(12)
    u = 2.0 ** -53
    cases, worst, zeros, regions, planted_zeros, planted_exact, planted_worst = 0, 0.0, 0, [0] * 8, 0, 0, 0.0
    while cases < 3750:
        a, b, c, p = (rng.integers(-8, 9, 3) for _ in range(4))
        planted = cases >= 3000
        if planted:
            s, t = rng.integers(0, 5, 2)
            p = a + ((b - a) * s + (c - a) * t) // 4 if rng.integers(2) else a + (b - a) * s + (c - a) * t
        if not np.cross(b - a, c - a).any():
            continue
        cases += 1
        d2, q, region = D.closest_on_triangles(*(x.astype(np.float64) for x in (a, b, c, p)))
        e2, eq, er = D.exact_dist2(a.tolist(), b.tolist(), c.tolist(), p.tolist())
        assert int(region) == er
        regions[er] += 1
        err = abs(Fraction(float(d2)) - e2)
        dist = math.sqrt(float(e2))
        assert err <= Fraction(u * (700.0 * dist + 4.0 * float(e2)) + 2e-27), (a, b, c, p)
        if e2 == 0 and planted:
            planted_zeros += 1
            planted_exact += float(d2) == 0.0
        elif e2 == 0:
            zeros += 1
            assert float(d2) == 0.0, (a, b, c, p)
        elif planted:
            planted_worst = max(planted_worst, float(err / e2) / 2.0 ** -52)
        else:
            worst = max(worst, float(err / e2) / 2.0 ** -52)
    # the planted case that shows the limit: the query lies on the triangle, v and w round, and dist2 is 2.5e-31, not 0
    a, b, c, p = ([3, -8, -6], [7, -1, 5], [-2, -4, -4], [4, -2, 2])
    d2 = float(D.closest_on_triangles(*(np.array(x, np.float64) for x in (a, b, c, p)))[0])
    assert D.exact_dist2(a, b, c, p)[0] == 0 and 0.0 < d2 < 1e-30
    print(f"restatement against exact rationals, {cases} cases: worst relative error of dist2 {worst:.2f} x 2^-52, {zeros} exact zeros among "
          f"the 3000 random cases (planted cases: {planted_worst:.2f} x 2^-52), {planted_exact} of {planted_zeros} planted zeros exact, cases per region {regions[1:]}")
    assert min(regions[1:]) >= 30 and planted_zeros >= 100
    figures = {"cases": cases, "worst_relative_dist2_in_2^-52": round(worst, 4), "exact_zeros": zeros,
               "planted_worst_relative_dist2_in_2^-52": round(planted_worst, 4), "planted_zeros": planted_zeros,
               "planted_zeros_exact": int(planted_exact), "regions": regions[1:]}
    if os.environ.get("CER_PARITY_RECORD"):
        path = os.path.join(REPO, "profiles", "mesh_dist_parity.json")
        record = json.load(open(path)) if os.path.exists(path) else {}
        record["restatement"] = figures
        json.dump(record, open(path, "w"), indent=1)
    assert parity["restatement"] == figures


# ---------------------------------------------------------------- the restatement: the index loses nothing
def test_restated_index_search_equals_the_brute_force():
    v, f, centre = S.field_mesh("sphere12")
    rng = np.random.default_rng(3)
    lo, hi = v.min(0) - 1.5, v.max(0) + 1.5
    queries = np.concatenate([rng.uniform(lo, hi, (600, 3)).astype(np.float32), v[::7]])
    for max_dist in (1.0, 20.0):
        want = D.brute(v, f, queries, max_dist)
        assert (want[1] >= 0).sum() >= 300
        for cell in (0.3, 1.0, 2.5):
            got = D.index_search(v, f, queries, max_dist, cell)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes(), (max_dist, cell)
    ties = 0
    for i in range(0, len(queries), 128):
        q = queries[i:i + 128].astype(np.float64)
        p64 = v.astype(np.float64)
        d2, _, _ = D.closest_on_triangles(p64[f[:, 0]][None], p64[f[:, 1]][None], p64[f[:, 2]][None], q[:, None, :])
        ties += int(((d2 == d2.min(1, keepdims=True)).sum(1) > 1).sum())
    assert ties >= len(v[::7])                                                                 # every vertex query ties: the index rule is at work
