"""Bit-identity of the epipolar-line-tile cost volume (csrc/cost_lines.hip) with the library that recorded tests/golden/cost_lines_bits.npz.

The tile kernel's instruction stream may be reorganised; what it computes may not change by a bit: the per-view partial volumes (MFMA path,
direct path, zero samples), the reduced volume with its pooled levels and the hypothesis origins.  ``test_cost_lines_matches_walk`` holds the
kernel against the fp32 walk at 4e-6 max(|vol|, 1), which cannot tell a sample that went through the band products from one that went through
the per-sample direct path (they differ by 4e-8 relative); this file can.

Cases: the eight geometries of ``test_cost_lines_matches_walk`` (epipole inside the image, projections near Z = 0, a band wider than 29 texels,
a view with dir < 0, a source view mostly out of the frustum) x (40 x 56, 33 x 47: ragged 32-pixel tiles on both axes, more than one line
group) x D in (64, 44, 16) x both ``two_term`` values, V = 3.

The golden file holds no volume: 96 cases of [3, P, D] floats are 90 MB.  It holds, per case, a position-weighted digest of the BIT PATTERNS,
    digest[column] = sum over pixels p of int64(bits[p, column]) * w[p]   (mod 2^64),   w[p] odd, a different one per pixel,
one per (view, hypothesis) column of the partial volumes, one per column of the reduced rows, one for the origins.  A change of any single
element changes its column's digest (an odd weight times a non-zero 32-bit difference is non-zero mod 2^64); two pixels swapped change it
too; only several changed elements of one column whose weighted differences cancel mod 2^64 would pass.  ~150 KB.

What the recorded cases reach, counted on the device with a marking build of the recording library (every sample class of the tile kernel
writes its own marker value; the build is not part of the repository): see ``PATHS`` below.

Re-record (only when the arithmetic is changed on purpose):  python tests/test_cost_lines_bits_gpu.py --record [file]
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

GOLDEN = os.path.join(HERE, "golden", "cost_lines_bits.npz")
GEOMS = ["horizontal", "diagonal", "vertical", "wild", "rotation", "forward", "converging", "zoom"]
SHAPES = [(40, 56), (33, 47)]
DS = [(64, True), (44, False), (16, False)]                 # (D, stage0)
NUM_LEVELS = 3

# Samples per class over all recorded cases of a geometry (both shapes, the three D, three-term form), counted with the marking build:
# "band" through the MFMA band products, "zero" outside the source map, "direct" the per-sample direct path because the band analysis did
# not cover the sample, "behind" the direct path because the sample lies in a chunk the lane's cursor has already left.
# ("zero" counts values that are exactly 0.)  The direct path is reached by "wild" (its band analysis fails where Z crosses 0) and, for three
# samples, by "forward"; "behind" by "wild" and by "forward" (lines of every direction in one view: the pixels that travel against the
# tile's majority).  "zoom", whose lines lie six texels apart, samples almost only the zero border at these sizes and has no direct sample.
PATHS = {
    "horizontal": dict(band=1096831, zero=313421, direct=0, behind=0),
    "diagonal": dict(band=1349734, zero=60518, direct=0, behind=0),
    "vertical": dict(band=1073886, zero=336366, direct=0, behind=0),
    "wild": dict(band=56339, zero=1320490, direct=28648, behind=4775),
    "rotation": dict(band=1352096, zero=58156, direct=0, behind=0),
    "forward": dict(band=1396957, zero=0, direct=3, behind=13292),
    "converging": dict(band=1173156, zero=237096, direct=0, behind=0),
    "zoom": dict(band=43143, zero=1367109, direct=0, behind=0),
}


def key(geom, D, h, w, two_term):
    return f"{geom}-D{D}-{h}x{w}-{'x2' if two_term else 'x3'}"


def weights(P, dev):
    """Odd 64-bit weights, one per pixel (a multiplicative hash of the index; int64 arithmetic wraps)."""
    i = torch.arange(1, P + 1, dtype=torch.int64, device=dev)
    return (i * -7046029254386353131 + 0x7F4A7C15) | 1      # 0x9E3779B97F4A7C15 as a signed 64-bit number


def digest(x, wts):
    """x [..., P, n] fp32 -> int64 [..., n]: the weighted sum of the bit patterns over the pixel axis."""
    bits = x.contiguous().view(torch.int32).to(torch.int64)
    return (bits * wts.view(-1, 1)).sum(dim=-2)


def run_case(dev, geom, D, stage0, h, w, two_term):
    """-> {part [V, D], vol [rs], origin [1]} int64 digests (CPU) of one case."""
    from cer_mvs_amd import ops
    from cer_mvs_amd.corr import fmaps_to_nhwc
    from cost_geometry_cases import V, incre_of, lines_geometry
    fm, Pij, d0 = lines_geometry(geom, D, stage0, h, w)
    fm = fm.to(dev)
    f1 = fmaps_to_nhwc(fm[0:1])[0]
    f2 = fmaps_to_nhwc(fm[1:], border=2)
    P = h * w
    vol, origin = ops.cost_build(f1, f2, Pij.to(dev), d0.to(dev), D, incre_of(stage0), stage0, h, w, NUM_LEVELS, fold=True,
                                 pyramid_scale=1.0 / V, two_term=two_term)
    ws = ops.lines_workspace(V, h, w, D, f1.device)          # the launch's partial volumes lead its workspace: [V][P][D] fp32
    part = ws[:V * P * D * 4].view(torch.float32).view(V, P, D)
    wts = weights(P, dev)
    out = {"part": digest(part, wts), "vol": digest(vol, wts), "origin": digest(origin.view(P, 1), wts)}
    return {k: t.cpu() for k, t in out.items()}, part


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bits():
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("D,stage0", DS)
@pytest.mark.parametrize("geom", GEOMS)
def test_cost_lines_bits(dev, bits, geom, D, stage0):
    for h, w in SHAPES:
        for two_term in (False, True):
            got, _ = run_case(dev, geom, D, stage0, h, w, two_term)
            k = key(geom, D, h, w, two_term)
            for name, t in got.items():
                ref = bits[f"{k}/{name}"]
                if not torch.equal(t, ref):
                    bad = (t != ref).nonzero().tolist()
                    print(f"{k} {name}: {len(bad)} of {ref.numel()} column digests differ, first (view, hypothesis) / column: {bad[:8]}")
                assert torch.equal(t, ref), (k, name)


def record(path=GOLDEN):
    dev = torch.device("cuda")
    out = {}
    for geom in GEOMS:
        for D, stage0 in DS:
            for h, w in SHAPES:
                for two_term in (False, True):
                    got, _ = run_case(dev, geom, D, stage0, h, w, two_term)
                    again, _ = run_case(dev, geom, D, stage0, h, w, two_term)
                    for name, t in got.items():
                        assert torch.equal(t, again[name]), "the recording library is not deterministic"
                        out[f"{key(geom, D, h, w, two_term)}/{name}"] = t.numpy()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"recorded {len(out)} digests of {len(out) // 3} cases: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record(*sys.argv[sys.argv.index("--record") + 1:][:1])
