"""Per-sample float64 parity of the two cost-volume builders on the HARD geometries (run on the GPU box: pytest -m gpu).

The epipolar-line tile kernel (csrc/cost_lines.hip, three-term and two-term) and the wave-per-pixel walk (csrc/cost_build.hip) project with
the same fp32 expressions, so the kernel-against-kernel maxima of test_cost_lines_matches_walk cannot see an error they share (NaN / inf /
clamp handling, the [-2, w2] texel clamp against the zero border, ``py + y0``, the origin shift), and the two geometries that drive the
direct path and the hand-over list sample almost nothing but the zero border (tests/cost_geometry_cases.py: census).  Here the coordinates
are restated bit for bit in numpy float32 (``parity_check.cost_coords32`` on an exact ``fma32``: a third implementation that shares no
code with either kernel), every sample's float64 value follows from its restated cell and fractions (``cost_samples_ref64``), and EVERY
element of every row is held to ``parity_check.cost_bound`` - the rounding of the 64-channel dot, the four weights and the view sum, derived
term by term from the kernel sources: c = 1.0e-6 (walk) / 1.28e-5 (tile kernel) of ``norm`` at V = 3, + 2^-31 * l1 where an f16 lo half
underflows.  ``norm`` is floored at the case's mean |ref|.  It is well defined where Z crosses 0 and at 0 / 0.

What runs: both builders (tile kernel in both forms; form 1 of ``cer_cost_lines_form`` too when the variant library is under test) on the
eight geometries of test_cost_lines_matches_walk and the four new ones that carry signal on the hard paths, at 7 x 13, 19 x 45, 33 x 65
(+ 70 x 150 for two), D = 64 / 44 / 20 (+ 37: pad columns untouched), V = 3 / 1, folded compact rows; the walk's per-view rows; full rows
from the fused epilogues and from the unfused build + ``ops.pyramid``; accumulate onto a hashed preset; row slabs (``y0`` / ``src_hw``),
also bit for bit against the same rows of the full build; the per-view launches ``cost_lines_views`` + ``cost_lines_reduce`` through a
permuted ``slots`` into a gathered buffer whose spare block is NaN, also bit for bit against the one-call build; and a ramp probe (the
source map's channels hold the texel's x and y, f1 selects one) that reads the device's own u and t back and holds them to the restated
ones within 8 * 2^-24 (|u| + 1) - which tells "the coordinates are off" from "the dots are off".  Every output is poisoned with NaN first
and must be covered; ``ops.check_overflow`` stays clear; ``cer_cost_build_algo`` is restored.

Measured on an MI355X (profiles/cost_geometry_parity.json, written only under CER_PARITY_RECORD=1 - another value: that path; a plain run
writes nothing), worst max |err| / bound over all cases, walk / three-term / two-term: folded rows 0.091 / 0.013 / 0.016 (99.9th percentile
0.062 / 0.007 / 0.009; max |err| / norm 8.1e-8 / 1.6e-7 / 2.1e-7), per-view rows 0.091, full rows 0.076 / 0.009 / 0.012 (fused and unfused alike),
accumulate 0.071 / 0.008 / 0.012, D = 37 0.065 / 0.008 / 0.007, slabs 0.074 / 0.009 / 0.009, per-view launches 0.009 / 0.012; the ramp probe 0.34 (walk)
and 0.44 (tile kernel) of 8 * 2^-24 (|u| + 1).  No ratio above 1: no kernel was changed and no constant replaced.  Bit identity: the per-view
launches equal the one-call build in both orders (asserted); the walk's slab rows equal the full build's (asserted), the tile kernel's in 53 of
108 slabs only - DESIGN.md section 4 says why.  The module takes 26 s; its slowest case (70 x 150, D = 64, both builders, V = 3 and 1) 4 s.
"""
import contextlib
import json
import os
import time

import numpy as np
import pytest
import torch

import cost_geometry_cases as G
import parity_check as pc
from conftest import REPO
from parity_check import assert_covered, poison_f16, poison_f32
from test_oracle_golden import hashed

pytestmark = pytest.mark.gpu


RECORD = {}
BUILDERS = [("walk", 1, False), ("three-term", 0, False), ("two-term", 0, True)]      # (form of cost_bound, cer_cost_build_algo, two_term)
KW = dict(tile=(1, 32), seam=32)
GEOM_D = [(g, D, s0) for g in G.GEOMS for D, s0 in G.DS]
GEOM_D_IDS = [f"{g}-D{D}" for g, D, s0 in GEOM_D]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _module_setup(dev):
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    t0 = time.time()
    yield
    torch.set_num_threads(n)
    target = os.environ.get("CER_PARITY_RECORD", "")
    if target:
        path = os.path.join(REPO, "profiles", "cost_geometry_parity.json") if target == "1" else target
        # per (section, builder, geometry-D): the worst figures over its sizes, view counts and slabs
        out = {"module_wall_s": round(time.time() - t0, 1), "cases": {}, "worst": {}}
        for key, d in RECORD.items():
            sec, form, case = key.split("/")[:3]
            for w in (out["cases"].setdefault(f"{sec}/{form}/{'-'.join(case.split('-')[:2])}", {}), out["worst"].setdefault(sec, {}).setdefault(form, {})):
                for k in ("max_ratio", "p999_ratio", "max_err_over_norm"):
                    w[k] = float(f"{max(w.get(k, 0.0), d[k]):.4g}")
                if "bit_identical_to_full_build" in d:
                    w["slabs"] = w.get("slabs", 0) + 1
                    w["slabs_bit_identical_to_full_build"] = w.get("slabs_bit_identical_to_full_build", 0) + int(d["bit_identical_to_full_build"])
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)


@contextlib.contextmanager
def algo(lib, a):
    prev = lib.cer_cost_build_algo(a)
    try:
        yield
    finally:
        lib.cer_cost_build_algo(prev)


def line_forms():
    """Forms of ``cer_cost_lines_form`` to run: the multi-line form only when the variant library is the one under test."""
    from cer_mvs_amd import _lib as L
    return (0, 1) if L.has_variant_forms() else (0,)


@contextlib.contextmanager
def line_form(lib, form):
    from cer_mvs_amd import _lib as L
    if not L.has_variant_forms():
        yield
        return
    prev = lib.cer_cost_lines_form(form)
    try:
        yield
    finally:
        lib.cer_cost_lines_form(prev)


def device_case(dev, geom, D, stage0, h, w):
    from cer_mvs_amd.corr import fmaps_to_nhwc
    fm, Pij, d0 = G.lines_geometry(geom, D, stage0, h, w)
    fm = fm.to(dev)
    return fmaps_to_nhwc(fm[0:1])[0], fmaps_to_nhwc(fm[1:], border=2), Pij.to(dev), d0.to(dev)


def judge(section, form, case, got, R, V, where, h, w, **kw):
    """Measure, print, record - then assert that every element is inside its bound."""
    rep = pc.check_cost_rows(got, R, V, form, where, h, w, **{k: v for k, v in kw.items() if k != "samples"})
    RECORD[f"{section}/{form}/{case}"] = {"max_ratio": rep.max_ratio, "p999_ratio": rep.p999_ratio, "max_err_over_norm": rep.max_rel}
    print(f"  {section:10s} {form:10s} {case:40s} max |err|/bound {rep.max_ratio:.3f}  p99.9 {rep.p999_ratio:.3f}  max |err|/norm {rep.max_rel:.2e}")
    assert rep.ok, rep.message() + corner_note(rep, kw.get("samples"), w)
    return rep


def corner_note(rep, S, w):
    """For the worst element of a failing check: the reference's four texel dots per view (CORNERS order), so that the message says which
    corner a wrong value could have come from."""
    y, x, c = rep.worst
    if S is None or "dots" not in S or c >= S["dots"].shape[2]:
        return ""
    d = S["dots"][:, y * w + x, c]
    return "\n  reference texel dots of the worst element, per view (corners 00 01 10 11): " + "; ".join(str([round(float(t), 6) for t in r]) for r in d)


def same_bits(a, b):
    return np.array_equal(a.detach().cpu().numpy().view(np.int32), b.detach().cpu().numpy().view(np.int32))


def sizes_of(geom):
    return G.SIZES + ([G.BIG] if geom in G.BIG_GEOMS else [])


def build(dev, f1, f2, Pij, d0, D, stage0, h, w, V, two_term=False, rows=None, y0=0, src_hw=None, compact=True, scale="mean", **kw):
    """``ops.cost_build`` (fold) into poisoned outputs -> (vol, origin)."""
    from cer_mvs_amd import ops
    _, _, rs = ops.row_layout(D, 3, compact)
    hh = h if rows is None else rows
    vol, org = poison_f32(torch.empty(hh * w, rs, device=dev)), poison_f32(torch.empty(hh * w, device=dev))
    extra = {} if scale is None else dict(pyramid_scale=(1.0 / V if scale == "mean" else scale))
    ops.cost_build(f1, f2[:V] if f2 is not None else None, Pij[:V], d0, D, G.incre_of(stage0), stage0, hh, w, 3, fold=True, vol=vol, origin=org,
                   compact=compact, two_term=two_term, y0=y0, src_hw=src_hw, **extra, **kw)
    return vol, org


# ------------------------------------------------------------------------------------------------ both builders against the reference
@pytest.mark.parametrize("geom,D,stage0", GEOM_D, ids=GEOM_D_IDS)
def test_builders_against_the_reference(dev, geom, D, stage0):
    """Folded compact rows (level 0, pyramid_scale = 1 / V), V = 3 and V = 1, every size of the geometry."""
    from cer_mvs_amd import _lib as L, ops
    lib = L.load()
    for h, w in sizes_of(geom):
        f1, f2, Pij, d0 = device_case(dev, geom, D, stage0, h, w)
        co = G.coords(geom, D, stage0, h, w)
        origin = torch.from_numpy(co["origin"])
        for form, a, two in BUILDERS:
            S = G.samples(geom, D, stage0, h, w, two)
            for V in (3, 1):
                R = pc.cost_rows_ref64(G.first_views(S, V), D, 3, 1.0 / V, True)
                for lf in (line_forms() if a == 0 else (0,)):
                    where = f"{form} {G.case_id(geom, D, stage0, h, w)} V={V}" + (" lines form 1" if lf else "")
                    with algo(lib, a), line_form(lib, lf):
                        vol, org = build(dev, f1, f2, Pij, d0, D, stage0, h, w, V, two_term=two)
                    assert_covered(vol[:, :D].cpu(), where, h=h, w=w, **KW)
                    assert_covered(org.cpu(), where + " origins", h=h, w=w, **KW)
                    assert same_bits(org, origin), where + ": origins"
                    judge("fold", form, f"{G.case_id(geom, D, stage0, h, w)}/V{V}" + ("/lf1" if lf else ""), vol, R, V, where, h, w,
                          samples=G.first_views(S, V))
    assert not ops.check_overflow(dev)


@pytest.mark.parametrize("geom", G.NEW_GEOMS + ["wild", "forward"])
def test_a_row_length_that_is_no_multiple_of_four(dev, geom):
    """D = 37: both builders accept it (the row is padded to 40 floats).  The pad columns stay as the wrapper left them: untouched in a
    volume the caller passed, zero in one the wrapper allocated."""
    from cer_mvs_amd import _lib as L, ops
    lib = L.load()
    D, stage0, (h, w), V = G.D_ODD, False, (19, 45), 3
    f1, f2, Pij, d0 = device_case(dev, geom, D, stage0, h, w)
    for form, a, two in BUILDERS:
        R = pc.cost_rows_ref64(G.samples(geom, D, stage0, h, w, two), D, 3, 1.0 / V, True)
        assert R["ref"].shape[1] == 40 and int((R["level"] >= 0).sum()) == D
        with algo(lib, a):
            vol, _ = build(dev, f1, f2, Pij, d0, D, stage0, h, w, V, two_term=two)
            own, _ = ops.cost_build(f1, f2, Pij, d0, D, G.incre_of(stage0), stage0, h, w, 3, fold=True, compact=True, pyramid_scale=1.0 / V, two_term=two)
        where = f"{form} {geom} D={D}"
        assert_covered(vol[:, :D].cpu(), where, h=h, w=w, **KW)
        assert bool(torch.isnan(vol[:, D:]).all()), where + ": a pad column was written"
        assert same_bits(own[:, :D], vol[:, :D]) and float(own[:, D:].abs().max()) == 0.0, where
        judge("odd_D", form, f"{geom}-D{D}-{h}x{w}", vol, R, V, where, h, w)
    assert not ops.check_overflow(dev)


# ------------------------------------------------------------------------------------------------ the walk, per view
@pytest.mark.parametrize("geom,D,stage0", GEOM_D, ids=GEOM_D_IDS)
def test_walk_per_view(dev, geom, D, stage0):
    """fold=False: [V, P, rs], level 0 of every view against that view's reference (the pooled levels of such rows are undefined until
    ``ops.pyramid`` runs: they must not have been written)."""
    from cer_mvs_amd import _lib as L, ops
    lib = L.load()
    V = G.V
    for h, w in G.SIZES:
        f1, f2, Pij, d0 = device_case(dev, geom, D, stage0, h, w)
        S = G.samples(geom, D, stage0, h, w)
        _, _, rs = ops.row_layout(D, 3)
        vol, org = poison_f32(torch.empty(V, h * w, rs, device=dev)), poison_f32(torch.empty(h * w, device=dev))
        with algo(lib, 1):
            ops.cost_build(f1, f2, Pij, d0, D, G.incre_of(stage0), stage0, h, w, 3, fold=False, vol=vol, origin=org)
        assert same_bits(org, torch.from_numpy(G.coords(geom, D, stage0, h, w)["origin"]))
        assert bool(torch.isnan(vol[..., D:]).all())
        for v in range(V):
            where = f"walk per view {G.case_id(geom, D, stage0, h, w)} view {v}"
            assert_covered(vol[v, :, :D].cpu(), where, h=h, w=w, **KW)
            R = pc.cost_rows_ref64({k: t[v:v + 1] for k, t in S.items()}, D, 3, None, True)
            judge("per_view", "walk", f"{G.case_id(geom, D, stage0, h, w)}/view{v}", vol[v, :, :R["ref"].shape[1]], R, 1, where, h, w)
    assert not ops.check_overflow(dev)


# ------------------------------------------------------------------------------------------------ row forms
@pytest.mark.parametrize("geom,D,stage0", GEOM_D, ids=GEOM_D_IDS)
def test_full_rows_fused_and_unfused(dev, geom, D, stage0):
    """compact=False, pyramid_scale = 1 / V: all pooled levels against ``cost_rows_ref64``; and the unfused build followed by
    ``ops.pyramid`` against the same reference.  Pad columns are left alone."""
    from cer_mvs_amd import _lib as L, ops
    lib = L.load()
    (h, w), V = (19, 45), G.V
    f1, f2, Pij, d0 = device_case(dev, geom, D, stage0, h, w)
    for form, a, two in BUILDERS:
        R = pc.cost_rows_ref64(G.samples(geom, D, stage0, h, w, two), D, 3, 1.0 / V, False)
        used = int((R["level"] >= 0).sum())
        assert used == D + D // 2 + D // 4
        with algo(lib, a):
            fused, _ = build(dev, f1, f2, Pij, d0, D, stage0, h, w, V, two_term=two, compact=False)
            plain, _ = build(dev, f1, f2, Pij, d0, D, stage0, h, w, V, two_term=two, compact=False, scale=None)
        assert bool(torch.isnan(plain[:, D:]).all())                     # level 0 only until the pyramid runs
        ops.pyramid(plain, D, 3, scale=1.0 / V)
        for name, vol in (("fused", fused), ("unfused", plain)):
            where = f"{form} {name} rows {G.case_id(geom, D, stage0, h, w)}"
            assert_covered(vol[:, :used].cpu(), where, h=h, w=w, **KW)
            assert bool(torch.isnan(vol[:, used:]).all()), where + ": a pad column was written"
            judge("rows_" + name, form, G.case_id(geom, D, stage0, h, w), vol, R, V, where, h, w)
    assert not ops.check_overflow(dev)


@pytest.mark.parametrize("geom,D,stage0", GEOM_D, ids=GEOM_D_IDS)
def test_accumulate_onto_a_preset(dev, geom, D, stage0):
    """accumulate=True onto a hashed volume: level 0 = preset + view sum; every other column of the row keeps its bits."""
    from cer_mvs_amd import _lib as L, ops
    lib = L.load()
    (h, w), V = (19, 45), G.V
    f1, f2, Pij, d0 = device_case(dev, geom, D, stage0, h, w)
    _, _, rs = ops.row_layout(D, 3)
    preset = hashed((h * w, rs), 5200 + D, -0.5, 0.5)
    for form, a, two in BUILDERS:
        R = pc.cost_rows_ref64(G.samples(geom, D, stage0, h, w, two), D, 3, None, False, preset=preset)
        vol, org = preset.to(dev), poison_f32(torch.empty(h * w, device=dev))
        with algo(lib, a):
            ops.cost_build(f1, f2, Pij, d0, D, G.incre_of(stage0), stage0, h, w, 3, fold=True, vol=vol, origin=org, accumulate=True, two_term=two)
        where = f"{form} accumulate {G.case_id(geom, D, stage0, h, w)}"
        assert_covered(vol.cpu(), where, h=h, w=w, **KW)
        assert_covered(org.cpu(), where + " origins", h=h, w=w, **KW)
        assert same_bits(vol[:, D:], preset[:, D:]), where + ": a column beyond level 0 changed"
        judge("accumulate", form, G.case_id(geom, D, stage0, h, w), vol, R, V, where, h, w, accumulate=True)
    assert not ops.check_overflow(dev)


# ------------------------------------------------------------------------------------------------ row slabs
@pytest.mark.parametrize("geom,D,stage0", GEOM_D, ids=GEOM_D_IDS)
def test_row_slabs(dev, geom, D, stage0):
    """A slab of image rows built on its own - f1 and d0 of its rows, ``src_hw`` the whole source map, ``y0`` its first row - against
    the reference with ``y0``; three slabs: rows 5 .. h - 1, the last three rows, and rows 2 .. 8 inside the image.  The walk's slab rows
    are also the full build's rows bit for bit (a wave per pixel: nothing depends on the grid); the tile kernel's are held to the reference
    alone (its tile partition is laid around the slab's own centre, so a sample may change between the band and the direct path)."""
    from cer_mvs_amd import _lib as L, ops
    lib = L.load()
    (h, w), V = (19, 45), G.V
    f1, f2, Pij, d0 = device_case(dev, geom, D, stage0, h, w)
    for form, a, two in BUILDERS:
        with algo(lib, a):
            full, _ = build(dev, f1, f2, Pij, d0, D, stage0, h, w, V, two_term=two)
        for y0, rows in ((5, h - 5), (h - 3, 3), (2, 7)):
            S = G.samples(geom, D, stage0, h, w, two, y0, rows)
            R = pc.cost_rows_ref64(S, D, 3, 1.0 / V, True)
            e = slice(y0 * w, (y0 + rows) * w)
            with algo(lib, a):
                vol, org = build(dev, f1[e], f2, Pij, d0[e], D, stage0, h, w, V, two_term=two, rows=rows, y0=y0, src_hw=(h, w))
            where = f"{form} slab rows {y0} .. {y0 + rows - 1} of {G.case_id(geom, D, stage0, h, w)}"
            assert_covered(vol[:, :D].cpu(), where, h=rows, w=w, **KW)
            assert same_bits(org, torch.from_numpy(G.coords(geom, D, stage0, h, w, y0, rows)["origin"])), where
            judge("slab", form, f"{G.case_id(geom, D, stage0, h, w)}/y{y0}+{rows}", vol, R, V, where, rows, w)
            bits = same_bits(vol[:, :D], full[e, :D])
            RECORD[f"slab/{form}/{G.case_id(geom, D, stage0, h, w)}/y{y0}+{rows}"]["bit_identical_to_full_build"] = bool(bits)
            if form == "walk":
                assert bits, where + ": not the full build's bits"
    assert not ops.check_overflow(dev)


# ------------------------------------------------------------------------------------------------ per-view launches through slots
@pytest.mark.parametrize("geom,D,stage0", GEOM_D, ids=GEOM_D_IDS)
def test_per_view_launches_through_permuted_slots(dev, geom, D, stage0):
    """``ops.cost_lines_views`` for views (0 .. 1) then (2), and (2) then (0 .. 1), followed by ``ops.cost_lines_reduce`` - fused, and
    accumulating onto a preset - with the source rows in a gathered buffer [4 blocks] addressed through slots = (2, 0, 3); block 1 holds
    the f16 NaN pattern and must never be read.  Against the reference, and bit for bit the one-call ``cost_build``."""
    from cer_mvs_amd import ops
    (h, w), V = (19, 45), G.V
    incre = G.incre_of(stage0)
    f1, f2, Pij, d0 = device_case(dev, geom, D, stage0, h, w)
    f1s, f2s = ops.feat_split(f1), ops.feat_split(f2)
    gathered = poison_f16(torch.empty((4,) + tuple(f2s.shape[1:]), device=dev, dtype=torch.float16))
    slots = torch.tensor([2, 0, 3], device=dev, dtype=torch.int32)
    for v in range(V):
        gathered[int(slots[v])] = f2s[v]
    _, _, rs = ops.row_layout(D, 3)
    preset = hashed((h * w, rs), 5300 + D, -0.5, 0.5)
    for form, two in (("three-term", False), ("two-term", True)):
        S = G.samples(geom, D, stage0, h, w, two)
        R = pc.cost_rows_ref64(S, D, 3, 1.0 / V, True)
        Ra = pc.cost_rows_ref64(S, D, 3, None, False, preset=preset)
        one, one_org = build(dev, f1, f2, Pij, d0, D, stage0, h, w, V, two_term=two)
        acc1 = preset.to(dev)
        ops.cost_build(f1, f2, Pij, d0, D, incre, stage0, h, w, 3, fold=True, vol=acc1, accumulate=True, two_term=two)
        # one call, through the slots (fmap2 = None: the split rows are all there is)
        via, via_org = build(dev, f1, None, Pij, d0, D, stage0, h, w, V, two_term=two, src_hw=(h, w), split=(f1s, gathered, slots))
        assert same_bits(via, one) and same_bits(via_org, one_org), f"{form} {geom} D={D}: one call through the slots"
        for order in (((0, 2), (2, 1)), ((2, 1), (0, 2))):
            tag = "+".join(f"{v0}..{v0 + nv - 1}" for v0, nv in order)
            for accumulate in (False, True):
                ws = ops.lines_workspace(V, h, w, D, dev)
                ws.fill_(0xFF)                                            # (every float of the partial volumes a NaN)
                for v0, nv in order:
                    ops.cost_lines_views(f1s, gathered, slots, Pij, d0, V, v0, nv, h, w, D, incre, stage0, two_term=two, ws=ws)
                if accumulate:
                    vol = preset.to(dev)
                    vol, org = ops.cost_lines_reduce(d0, V, h, w, D, incre, stage0, 3, vol=vol, accumulate=True, ws=ws)
                    want, ref, cols = acc1, Ra, rs
                else:
                    vol = poison_f32(torch.empty(h * w, ops.row_layout(D, 3, True)[2], device=dev))
                    vol, org = ops.cost_lines_reduce(d0, V, h, w, D, incre, stage0, 3, pyramid_scale=1.0 / V, vol=vol, ws=ws, compact=True)
                    want, ref, cols = one, R, D
                where = f"{form} views {tag}{' accumulate' if accumulate else ''} {G.case_id(geom, D, stage0, h, w)}"
                assert_covered(vol[:, :cols].cpu(), where, h=h, w=w, **KW)
                assert same_bits(org, one_org), where + ": origins"
                judge("views" + ("_acc" if accumulate else ""), form, f"{G.case_id(geom, D, stage0, h, w)}/{tag}", vol, ref, V, where, h, w, accumulate=accumulate)
                assert same_bits(vol[:, :cols], want[:, :cols]), where + ": not the one-call build's bits"
    assert not ops.check_overflow(dev)


# ------------------------------------------------------------------------------------------------ ramp probe
@pytest.mark.parametrize("geom,D,stage0", GEOM_D, ids=GEOM_D_IDS)
def test_ramp_probe_reads_the_device_coordinates(dev, geom, D, stage0):
    """f1 = one unit channel; channel 0 of the source map holds the texel's x, channel 1 its y (integers up to 64: exact as f16 operands
    x 64, far from the overflow flag).  Wherever all four corners of a sample are in the map the volume of ONE view at scale 1 is then the
    device's own u (or t): four weights, four products and three adds from the restated iu + du - within 8 * 2^-24 (|u| + 1)."""
    from cer_mvs_amd import _lib as L, ops
    lib = L.load()
    h, w = 33, 65
    _, Pij, d0 = G.lines_geometry(geom, D, stage0, h, w)
    co = G.coords(geom, D, stage0, h, w)
    Pd, dd = Pij.to(dev), d0.to(dev)
    ramp = torch.zeros(1, h + 4, w + 4, 64)
    ramp[0, 2:h + 2, 2:w + 2, 0] = torch.arange(w, dtype=torch.float32)[None, :]
    ramp[0, 2:h + 2, 2:w + 2, 1] = torch.arange(h, dtype=torch.float32)[:, None]
    f2 = ramp.reshape(1, -1, 64).to(dev)
    worst = {}
    for ch, cell, frac in ((0, "iu", "du"), (1, "iw", "dw")):
        f1 = torch.zeros(h * w, 64)
        f1[:, ch] = 1.0
        f1 = f1.to(dev)
        for v in range(G.V):
            inside = torch.from_numpy(co["ok"][v] & (co["iu"][v] >= 0) & (co["iu"][v] <= w - 2) & (co["iw"][v] >= 0) & (co["iw"][v] <= h - 2))
            want = torch.from_numpy(co[cell][v]).double() + torch.from_numpy(co[frac][v]).double()
            for form, a, two in BUILDERS[:2]:
                with algo(lib, a):
                    vol, _ = build(dev, f1, f2, Pd[v:v + 1], dd, D, stage0, h, w, 1, scale=1.0)
                got = vol[:, :D].cpu().double()
                where = f"ramp {'xy'[ch]} {form} {G.case_id(geom, D, stage0, h, w)} view {v}"
                assert_covered(got, where, h=h, w=w, **KW)
                mag = torch.where(inside, want.abs() + 1.0, torch.full_like(want, 1e300))      # (elsewhere a corner is the zero border: not a coordinate)
                rep = pc.check_elementwise(got, torch.where(inside, want, got), mag, 8 * pc.U24, 0.0, where, h=h, w=w, **KW)
                worst[form] = max(worst.get(form, 0.0), rep.max_ratio)
                assert rep.ok, rep.message()
    for form, r in worst.items():
        RECORD[f"ramp/{form}/{G.case_id(geom, D, stage0, h, w)}"] = {"max_ratio": r, "p999_ratio": 0.0, "max_err_over_norm": 0.0}
    print(f"  ramp {G.case_id(geom, D, stage0, h, w)}: worst |device coordinate - restated| / bound {worst}")
    assert not ops.check_overflow(dev)
