"""Mesh surface sampling (csrc/mesh_sample.hip, cer-mvs_amd/mesh.py face_areas / sample_mesh / sample_mesh_even / evaluate_mesh, DESIGN.md
3zg), the parts that need no GPU: the three entry points of ABI 1230 and their argument checks in the documented order, the Python layer's
ValueErrors and the forms of the "sample" option, and the numpy restatement of tests/mesh_sample_reference.py - which the GPU tests hold the
device to, bit for bit - held to the published Philox vectors, to a sample worked out by hand and to the statistics of the issue
(profiles/mesh_sample_parity.json)."""
import ctypes
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import mesh_sample_reference as R
import mesh_smooth_reference as S
from conftest import REPO

BIG = 1 << 31
NAMES = ("cer_mesh_face_areas_f64", "cer_mesh_face_weights_i64", "cer_mesh_sample_f32")
KERNELS = ("mesh_face_areas_kernel", "mesh_face_weights_kernel", "mesh_sample_kernel")
RIGHT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)


@pytest.fixture(scope="module")
def parity():
    return json.load(open(os.path.join(REPO, "profiles", "mesh_sample_parity.json")))


@pytest.fixture(scope="module")
def sphere12():
    """the small analytic sphere mesh, computed once and left unchanged"""
    return S.field_mesh("sphere12")


# ---------------------------------------------------------------- ABI
def test_sample_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    names = L.exported_symbols()
    for n in NAMES:
        assert n in names and re.search(r"\bint %s\(" % n, hdr), n
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P                 # a stream: the last argument
    assert L.ABI_VERSION >= 1230 and "Mesh surface sampling (ABI 1230" in hdr and len(names) >= 126
    lib = L.load()
    assert lib.cer_abi_version() == L.ABI_VERSION
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(REPO, doc)).read()
        assert "126 entry points" in text and f"{len(names)} entry points" in text, doc
    csrc = os.path.join(REPO, "cer-mvs_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "mesh_sample.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert re.search(r"^mesh_sample\.o: CXXFLAGS \+= -fno-slp-vectorize$", mk, re.M) and "-ffast-math" not in mk
    src = open(os.path.join(csrc, "mesh_sample.hip")).read()
    for kernel in KERNELS:
        assert "void " + kernel in src, kernel
    # registers only, in the whole file; no fused multiply-add: the device's fp64 square root needed no correction
    assert not re.search(r"atomic\w*\s*\(|\bfmaf?\s*\(|__shared__|__syncthreads", src)
    assert not re.search(r"^[ \t]*#[ \t]*ifndef", src, re.M)                                    # no overridable switch


def test_sample_entry_points_refuse_bad_arguments_in_the_documented_order():
    """every check runs before any launch (the pointers are fake: a launch would fault).  The order: (1) a negative size CER_EINVAL (-1); (2)
    nv, 3 nf or n >= 2^31, a shift out of range, samples from no face CER_ESHAPE (-2); (3) nothing to do CER_OK; (4) null pointers
    CER_EINVAL - each case breaks one rule and every later one, and gets the earlier rule's answer."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    third = (BIG + 2) // 3                                                                     # the first nf with 3 nf >= 2^31

    def areas(ver=fake, nv=5, fac=fake, nf=4, out=fake):
        return lib.cer_mesh_face_areas_f64(ver, nv, fac, nf, out, null)
    an = dict(ver=null, fac=null, out=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nv=-1, nf=third), dict(nf=-1, nv=BIG)):                                                 # 1
        assert areas(**kw) == -1 and areas(**kw, **an) == -1, kw
    for kw in (dict(nv=BIG), dict(nf=third), dict(nf=0, nv=BIG), dict(nf=1 << 62)):                                                   # 2
        assert areas(**kw) == -2 and areas(**kw, **an) == -2, kw
    assert areas(nf=0) == 0 and areas(nf=0, **an) == 0 and areas(nf=0, nv=0, **an) == 0                                               # 3
    for name in an:                                                                                                                   # 4
        assert areas(**{name: null}) == -1, name
    assert areas(nv=0, ver=null, fac=null) == -1 and areas(nv=0, ver=null, out=null) == -1   # no vertex: vertices may be null, the rest not

    def weights(src=fake, nf=4, shift=31, out=fake):
        return lib.cer_mesh_face_weights_i64(src, nf, shift, out, null)
    wn = dict(src=null, out=null)
    for kw in (dict(nf=-1), dict(nf=-1, shift=5000), dict(nf=-5, shift=-5000)):                                                       # 1
        assert weights(**kw) == -1 and weights(**kw, **wn) == -1, kw
    for kw in (dict(nf=third), dict(shift=1106), dict(shift=-993), dict(nf=0, shift=1 << 30), dict(nf=0, shift=-(1 << 30))):          # 2
        assert weights(**kw) == -2 and weights(**kw, **wn) == -2, kw
    assert weights(nf=0) == 0 and weights(nf=0, **wn) == 0 and weights(nf=0, shift=1105, **wn) == 0 and weights(nf=0, shift=-992, **wn) == 0   # 3
    for name in wn:                                                                                                                   # 4
        assert weights(**{name: null}) == -1 and weights(**{name: null}, shift=-992) == -1, name

    def sample(ver=fake, nv=5, fac=fake, nf=4, cum=fake, seed=0, offset=0, words=fake, n=7, col=fake, pts=fake, face=fake, uv=fake, nrm=fake,
               oc=fake):
        return lib.cer_mesh_sample_f32(ver, nv, fac, nf, cum, seed, offset, words, n, col, pts, face, uv, nrm, oc, null)
    required = dict(ver=null, fac=null, cum=null, pts=null, face=null)
    sn = dict(required, words=null, col=null, uv=null, nrm=null, oc=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(n=-1), dict(n=-1, nv=BIG), dict(nv=-1, nf=third), dict(nf=-1, n=BIG)):                  # 1
        assert sample(**kw) == -1 and sample(**kw, **sn) == -1, kw
    for kw in (dict(nv=BIG), dict(nf=third), dict(n=BIG), dict(nf=0), dict(n=0, nv=BIG), dict(n=0, nf=third), dict(nf=0, n=1)):       # 2
        assert sample(**kw) == -2 and sample(**kw, **sn) == -2, kw
    for kw in (dict(n=0), dict(n=0, nf=0), dict(n=0, nf=0, nv=0), dict(n=0, seed=(1 << 64) - 1, offset=(1 << 64) - 1)):               # 3
        assert sample(**kw) == 0 and sample(**kw, **sn) == 0, kw
    for name in required:                                                                                                             # 4
        assert sample(**{name: null}) == -1, name
    assert sample(col=null) == -1 and sample(oc=null) == -1                                  # colours: both or neither
    assert sample(nv=0, ver=null, cum=null) == -1 and sample(words=null, uv=null, nrm=null, col=null, oc=null, pts=null) == -1


# ---------------------------------------------------------------- the Python layer
def test_sample_python_layer_refuses_bad_arguments_without_a_device():
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    ver = torch.zeros(5, 3)
    col = torch.zeros(5, 3, dtype=torch.uint8)
    fac = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    gt = torch.zeros(4, 3)
    words = torch.zeros(3, 4, dtype=torch.uint32)
    fa, sm, se, ev = ME.face_areas, ME.sample_mesh, ME.sample_mesh_even, ME.evaluate_mesh
    calls = (lambda v, f: fa(v, f), lambda v, f: sm(v, f, n=4), lambda v, f: se(v, f, 0.5), lambda v, f: ev(v, f, gt, 0.5))
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
    for bad in (col.float(), col[:4], col[:, :2], col.numpy()):
        with pytest.raises(ValueError, match="colors"):
            sm(ver, fac, n=4, colors=bad)
        with pytest.raises(ValueError, match="colors"):
            se(ver, fac, 0.5, colors=bad)
    for kw in ({}, dict(n=4, density=2.0), dict(n=4, words=words), dict(density=1.0, words=words), dict(n=1, density=1.0, words=words)):
        with pytest.raises(ValueError, match="exactly one of n, density and words"):
            sm(ver, fac, **kw)
    for bad in (-1, BIG, 2.0, True, "4", [4]):
        with pytest.raises(ValueError, match="n must be an integer"):
            sm(ver, fac, n=bad)
    for bad in (0, -1.0, math.inf, math.nan, True, "1", [1.0]):
        with pytest.raises(ValueError, match="density must be a positive finite number"):
            sm(ver, fac, density=bad)
    for bad in (words.to(torch.int64), words.to(torch.int32), words[:, :3], words[0], words.numpy(), [[0, 0, 0, 0]]):
        with pytest.raises(ValueError, match="words uint32"):
            sm(ver, fac, words=bad)
    for name in ("seed", "offset"):
        for bad in (-1, 1 << 64, 1.0, True, "0", None):
            with pytest.raises(ValueError, match=f"{name} must be an integer"):
                sm(ver, fac, n=4, **{name: bad})
    for name in ("normals", "uv"):
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match=f"{name} must be True or False"):
                sm(ver, fac, n=4, **{name: bad})
    for bad in (0, -0.5, math.inf, math.nan, True, "1", None, 1e-60):                        # (1e-60 is zero as a float32 radius)
        with pytest.raises(ValueError, match="spacing must be a positive finite"):
            se(ver, fac, bad)
        with pytest.raises(ValueError, match="spacing must be a positive finite"):
            ev(ver, fac, gt, bad)
    for bad in (0, -8.0, math.inf, True, None):
        with pytest.raises(ValueError, match="oversample must be a positive finite number"):
            se(ver, fac, 0.5, oversample=bad)
    with pytest.raises(ValueError, match="seed must be an integer"):
        se(ver, fac, 0.5, seed=-1)
    for bad in (gt.double(), gt[:, :2], gt[0], gt.numpy(), None):
        with pytest.raises(ValueError, match="gt float32"):
            ev(ver, fac, bad, 0.5)
    for bad in (0, -1.0, math.inf, True, None):
        with pytest.raises(ValueError, match="max_dist must be a positive finite number"):
            ev(ver, fac, gt, 0.5, max_dist=bad)
    for bad in (0, -1.0, math.inf, True):
        with pytest.raises(ValueError, match="tau must be a positive finite number"):
            ev(ver, fac, gt, 0.5, tau=bad)
    for call in (lambda: fa(ver, fac), lambda: fa(ver[:0], fac[:0]), lambda: sm(ver, fac, n=0), lambda: sm(ver, fac, n=7, seed=(1 << 64) - 1),
                 lambda: sm(ver, fac, density=3.5, normals=True, colors=col, uv=True, info={}), lambda: sm(ver, fac, words=words),
                 lambda: sm(ver, fac, n=np.int64(4), offset=np.int64(9)), lambda: se(ver, fac, 0.5), lambda: se(ver, fac, 0.5, colors=col, info={}),
                 lambda: ev(ver, fac, gt, 0.5), lambda: ev(ver, fac, gt, 0.5, tau=1.0, max_dist=5)):
        with pytest.raises(RuntimeError, match="CUDA"):      # good arguments: the host tensors are what is refused
            call()
    # the option of reconstruct_scan(mesh=...): refused before a model or a session is built
    for bad in (0, -3, 3.0, True, False, "16", None, [16], BIG, {}, {"seed": 3}, {"n": 5, "density": 1.0}, {"n": 5, "spacing": 1.0},
                {"density": 1.0, "spacing": 1.0}, {"n": 0}, {"n": 2.0}, {"n": True}, {"density": 0}, {"density": math.inf}, {"density": "1"},
                {"spacing": -1.0}, {"spacing": math.nan}, {"n": 5, "seed": -1}, {"n": 5, "seed": 1.0}, {"n": 5, "seed": 1 << 64},
                {"n": 5, "offset": 3}, {"samples": 5}):
        with pytest.raises(ValueError, match="mesh: sample"):
            ME.mesh_options({"sample": bad})
        with pytest.raises(ValueError, match="mesh: sample"):
            reconstruct_scan(None, [0], [0], [0], ["a"], [[0]], [1.0], None, write=False, mesh={"resolution": 48, "sample": bad})
    for bad in ({"samples": 16}, {"n": 16}, {"spacing": 1.0}):
        with pytest.raises(ValueError, match="unknown"):
            ME.mesh_options(bad)
    for good in ({"sample": 1}, {"sample": 1000}, {"sample": {"n": 7}}, {"sample": {"density": 0.5, "seed": 3}}, {"sample": {"spacing": 2, "seed": (1 << 64) - 1}},
                 {"resolution": 48, "min_component": 157, "fill_holes": 32, "smooth": 3, "simplify": 2, "colors": True, "normals": True, "topology": True,
                  "sample": {"spacing": 0.25}}):
        assert ME.mesh_options(good) == good
    assert ME._sample_option(1000) == ("n", 1000, 0) and ME._sample_option({"spacing": 2, "seed": 9}) == ("spacing", 2.0, 9)
    assert "sample" in ME.MESH_OPTION_KEYS and ME.mesh_options({"resolution": 48}) == {"resolution": 48}
    assert ME.SAMPLE_INFO_KEYS == R.INFO_KEYS
    assert "2^-31 of the largest face" in sm.__doc__ and "never drawn" in sm.__doc__                              # the density's bound, where it is read
    assert "pairwise farther" in se.__doc__ and "every drawn sample has a kept one" in se.__doc__                 # radius_thin's two properties
    assert "upward bias" in ev.__doc__ and "future work" in ev.__doc__
    for fn in (fa, sm):
        assert "Mesh surface sampling" in fn.__doc__


# ---------------------------------------------------------------- the restatement: Philox
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),      # the digits of pi
)


def test_restated_philox_reproduces_the_published_vectors():
    for counter, key, want in KNOWN_ANSWERS:
        assert " ".join("%08x" % x for x in R.philox(counter, key)) == want
    # the vectorised form against the scalar one, across the carry into the high counter word and with a key of two words
    for seed, offset, n in ((0, 0, 5), (1, 7, 3), ((1 << 32) + 5, (1 << 32) - 2, 5), ((1 << 64) - 1, (1 << 64) - 2, 4)):
        words = R.philox_words(seed, offset, n)
        assert words.dtype == np.uint32 and words.shape == (n, 4)
        for i in range(n):
            k = (offset + i) % (1 << 64)
            assert tuple(words[i].tolist()) == R.philox((k & R.MASK32, k >> 32, 0, 0), (seed & R.MASK32, seed >> 32)), (seed, offset, i)
    assert R.philox_words(3, 0, 0).shape == (0, 4)
    assert tuple(R.philox_words(0, 0, 1)[0].tolist()) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)


# ---------------------------------------------------------------- the restatement, by hand
def test_restated_sample_worked_out_by_hand():
    v = np.array([[1, 2, 3], [5, 2, 3], [1, 10, 3]], np.float32)
    col = np.array([[0, 255, 10], [100, 255, 10], [0, 255, 11]], np.uint8)
    words = np.array([[0, 0, 1 << 30, 1 << 31],                                                # a + b < 2^32: as it is
                      [0xffffffff, 0xffffffff, 3 << 30, 1 << 31],                              # a + b = 5 * 2^30: folded
                      [7, 7, 0xffffffff, 0], [7, 7, 0, 0xffffffff],                            # a + b = 2^32 - 1: not folded, w = 0
                      [7, 7, 0xffffffff, 1], [7, 7, 0, 0]], np.uint32)                         # a + b = 2^32: folded to (0, 2^32 - 2); the corner A
    (p, face, nrm, c, uv), info = R.sample(v, [[0, 1, 2]], words=words, normals=True, colors=col, uv=True)
    assert info == dict(n=6, area=16.0, faces_with_weight=1, shift=27) and face.tolist() == [0] * 6
    half, two32 = Fraction(1, 2), Fraction(1 << 32)
    want_uv = [((1 << 30) + half, (1 << 31) + half), ((1 << 30) - 1 + half, (1 << 31) - 1 + half), ((1 << 32) - 1 + half, half),
               (half, (1 << 32) - 1 + half), (half, (1 << 32) - 2 + half), (half, half)]
    for i, (a, b) in enumerate(want_uv):
        fu, fv = a / two32, b / two32
        assert Fraction(float(uv[i, 0])) == fu and Fraction(float(uv[i, 1])) == fv, i        # exact in fp64
        fw = 1 - fu - fv
        assert fw >= 0
        exact = [fw * int(v[0, k]) + fu * int(v[1, k]) + fv * int(v[2, k]) for k in range(3)]
        assert p[i].tolist() == [float(np.float32(float(x))) for x in exact], i               # small integers: every fp64 step is exact here
    assert p[0].tolist() == [2.0, 6.0, 3.0] and p[1].tolist() == [2.0, 6.0, 3.0]
    assert p[2].tolist() == [5.0, 2.0, 3.0] and p[5].tolist() == [1.0, 2.0, 3.0]
    assert np.array_equal(nrm, np.tile(np.float32([0, 0, 1]), (6, 1)))
    assert c[0].tolist() == [25, 255, 11] and c[2].tolist() == [100, 255, 10] and c[5].tolist() == [0, 255, 10]    # 10.5 + 2^-33 rounds up
    # the fold is the point reflection of the square through its centre: it maps the far triangle onto the near one
    u, vv, w = R.barycentric(words)
    assert (w >= 0).all() and w[2] == 0.0 and w[3] == 0.0 and (u + vv <= 1.0).all()
    # r = 0 and r = 2^64 - 1 on a table with faces without weight at both ends
    cum = np.array([0, 0, 5, 5, 9, 9], np.int64)
    assert R.pick_faces(cum, 9, [[0, 0, 0, 0], [0xffffffff, 0xffffffff, 0, 0], [0x8e38e38e, 0x38e38e38, 0, 0], [0x8e38e38e, 0x38e38e39, 0, 0]]).tolist() \
        == [2, 4, 2, 4]                                                                        # t = 0, 8, 4, 5
    # a face with an index out of range or a repeated one: NaN, colour 0 (reached only through a table that is not the mesh's own)
    (p, face, nrm, c, _) = R.sample_with(v, [[0, 1, 3], [0, 1, 1]], np.array([1, 2], np.int64), 2, [[0, 0, 5, 5], [0x80000000, 0, 5, 5]],
                                         normals=True, colors=col)
    assert face.tolist() == [0, 1] and np.isnan(p).all() and np.isnan(nrm).all() and not c.any()


def test_restated_areas_and_weights():
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [np.nan, 0, 0], [np.inf, 0, 0], [3, 2.0 ** -40, 0]], np.float32)
    f = [[0, 1, 2], [0, 3, 4], [0, 1, 1], [0, -1, 2], [0, 1, 8], [0, 1, 5], [0, 6, 2], [0, 1, 7]]
    areas = R.face_areas(v, f)
    assert areas.tolist() == [1.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5 * 2.0 ** -40]            # the sliver: far below 2^-32 of the largest
    cum, W, shift, _ = R.table(v, f)
    assert shift == 31 and np.diff(cum, prepend=0).tolist() == [3221225472, 1073741824, 0, 0, 0, 0, 0, 0] and W == 1 << 32
    assert R.face_weights(np.array([np.nan, -1.0, np.inf, 2.0 ** 40, 0.75, 0.0]), 31).tolist() == [0, 0, 0, 0, 1610612736, 0]
    assert R.shift_of(1.5) == 31 and R.shift_of(1.0) == 31 and R.shift_of(0.99) == 32 and R.shift_of(2.0 ** -299) == 330
    assert R.table(v, [[0, 1, 1]])[1] == 0 and R.table(v, [])[1] == 0
    with pytest.raises(ValueError):
        R.sample(v, [[0, 1, 1]], n=1)
    assert R.sample(v, [[0, 1, 1]], n=0)[0][0].shape == (0, 3)


# ---------------------------------------------------------------- the restatement: statistics
def test_restated_sampling_statistics(sphere12, parity):
    figures = {}
    # two triangles of areas 1.5 and 0.5
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    f = [[0, 1, 2], [0, 3, 4]]
    cum, W, shift, _ = R.table(v, f)
    assert np.diff(cum, prepend=0).tolist() == [3221225472, 1073741824]
    (p, face, _, _, _), info = R.sample(v, f, n=4096, seed=0)
    count = int((face == 0).sum())
    sigma = math.sqrt(4096 * 0.75 * 0.25)
    print(f"two triangles, n = 4096: face 0 drawn {count} times (expected 3072, sigma {sigma:.1f})")
    assert abs(count - 3072) <= 139 and 5 * sigma < 139 < 5 * sigma + 1 and count == 3111
    assert info == dict(n=4096, area=2.0, faces_with_weight=2, shift=31)
    figures["two_triangles"] = {"n": 4096, "face0": count}
    # the unit right triangle: the mean against the centroid
    n = 65536
    (p, face, _, _, _), _ = R.sample(RIGHT, [[0, 1, 2]], n=n, seed=0)
    mean = p.astype(np.float64).mean(0)
    bound = 5 * math.sqrt(1 / 18 / n)
    print(f"unit right triangle, n = {n}: mean {mean.tolist()}, bound {bound:.6f} around 1/3")
    assert abs(mean[0] - 1 / 3) <= bound and abs(mean[1] - 1 / 3) <= bound and mean[2] == 0.0
    off, out = R.in_triangle(p, RIGHT, [[0, 1, 2]], face)
    assert off == 0.0 and out <= 2.0 ** -23
    figures["right_triangle"] = {"n": n, "mean": mean[:2].tolist()}
    # the small sphere: counts by the octant of the face's centroid
    sv, sf, centre = sphere12
    areas = R.face_areas(sv, sf)
    octant = ((sv.astype(np.float64)[sf].mean(1) > np.asarray(centre, np.float64)) * (1, 2, 4)).sum(1)
    (p, face, nrm, _, _), info = R.sample(sv, sf, n=n, seed=0, normals=True)
    got = np.bincount(octant[face], minlength=8)
    expected = n * np.bincount(octant, weights=areas, minlength=8) / areas.sum()
    chi2 = float((((got - expected) ** 2) / expected).sum())
    print(f"sphere12, n = {n}: octant counts {got.tolist()}, expected {np.round(expected, 1).tolist()}, chi-square {chi2:.2f} on 7 degrees of freedom")
    assert (expected > 0).all() and chi2 < 40.0
    assert info["faces_with_weight"] == len(sf) and abs(info["area"] - areas.sum()) <= len(sf) * 2.0 ** -info["shift"]
    figures["sphere12"] = {"n": n, "octants": got.tolist(), "chi2": round(chi2, 6), "area": info["area"], "shift": info["shift"]}
    # every sample in its triangle's plane and inside it, to float32 rounding; the normal is the face's
    off, out = R.in_triangle(p, sv, sf, face)
    print(f"sphere12: largest distance from the plane {off:.3e} and beyond an edge {out:.3e}, relative to the face's largest coordinate")
    # the exact point is inside; rounding moves each of its three coordinates by at most 2^-24 of itself: sqrt(3) * 2^-24 of the largest in all
    assert off <= 2 * 2.0 ** -24 and out <= 2 * 2.0 ** -24
    unit = np.cross(sv[sf[:, 1]].astype(np.float64) - sv[sf[:, 0]], sv[sf[:, 2]].astype(np.float64) - sv[sf[:, 0]])
    unit /= np.linalg.norm(unit, axis=1)[:, None]
    assert np.abs(nrm - unit[face]).max() <= 2.0 ** -23
    if os.environ.get("CER_PARITY_RECORD"):
        path = os.path.join(REPO, "profiles", "mesh_sample_parity.json")
        record = json.load(open(path)) if os.path.exists(path) else {}
        record["restatement"] = figures
        json.dump(record, open(path, "w"), indent=1)
    assert parity["restatement"] == figures


def test_restated_even_sampling(sphere12):
    sv, sf, _ = sphere12
    (p, face, nrm, col), kept, n0 = R.sample_even(sv, sf, 0.75, seed=2, normals=True, colors=R.random_colors(len(sv)))
    (q, qface, _, _, _), info = R.sample(sv, sf, n=n0, seed=2)
    assert n0 == R.drawn_for(info["area"], 0.75) and 64 <= len(kept) < n0 <= 4096 and (np.diff(kept) > 0).all()
    assert p.tobytes() == q[kept].tobytes() and np.array_equal(face, qface[kept]) and len(nrm) == len(col) == len(kept)
    d = np.linalg.norm(q.astype(np.float64)[:, None] - p.astype(np.float64)[None], axis=2)
    apart = d[kept] + np.where(np.eye(len(kept), dtype=bool), np.inf, 0.0)
    assert apart.min() > 0.75 and d.min(1).max() <= 0.75                                         # radius_thin's two properties
