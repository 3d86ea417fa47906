"""Byte-exact parity of the layout, mover and glue kernels at ragged shapes, ONE LAUNCH PER ASSERTION (run on the GPU box: pytest -m gpu).

Every arithmetic kernel has a per-element float64 parity file; the small kernels that carry data between them had round trips at one shape,
aggregate rel_l1, or nothing.  All of them are pure data movement or a handful of separately rounded fp32 / fp64 operations (the library is
built with -ffp-contract=off), so their output is stated bit for bit in numpy (tests/glue_reference.py, written from the words of
include/cer_mvs.h and checked against itself by tests/test_glue_reference_cpu.py) and every byte is compared:

  cer_nchw_to_nhwc_f32, cer_nhwc_to_nchw_f32, cer_nchw_to_nhwc_border_f32, cer_copy_segments_f32 (alone and under slab.pack_strips /
  slab.unpack_halves), cer_s16_layout_f32 (three layouts, both directions, padding), cer_s16_rows_f32 (both directions, odd and even row
  boundaries), cer_split32_f32, cer_feat_split_f16 (multi-block, the clamp boundary), cer_feat_ref_rows_f16, cer_f16_scan_overflow (every
  position class, the grid-stride loop), cer_pyramid_f32 (odd D, row gaps), cer_plane_stats_f32 and cer_norm_act_f32 (scalar and chunked
  paths, in place).

Two rules hold throughout.  Every output lives inside a larger allocation (``Arena``) whose head and tail - 1024 words each - and whose
unwritten parts are pre-filled with a fixed NaN-payload word; guards and untouched bytes are compared as int32, so a stray write is found
without anything leaving its allocation.  Comparisons are ``torch.equal`` on int32 views, except for the two kernels that accumulate:

  * cer_plane_stats_f32: |mean - float32(mean64)| <= 1 ulp; rstd to 2^-23 + 0.5 * plane * 2^-52 * E[x^2] / (var + eps) relative - the final
    rounding plus the worst cancellation of the kernel's E[x^2] - mean^2 form in float64, computed per plane.  (For the constant plane and the
    mean-100 plane the second term is 1e-6 .. 2e-4 at the two-chunk sizes: it is the bound, not a remark about it, that the test applies.)
  * cer_norm_act_f32: |got - ref64| <= 2^-22 * (|t| + |u|) + 2^-149, t and u the two float64 branches as they enter the sum: three separately
    rounded fp32 operations per branch and one for the sum, doubled.  The statistics fed to kernel and reference are the kernel's own.  Where
    no statistics are given the result is a copy or a single fp32 sum and must be exact.

No test here is satisfied by a symmetric error.  Planted in the REFERENCE and run against the kernels on an MI355X: kg and li swapped in the
frag16 map turns test_s16_layouts (frag16), test_frag16_values and test_s16_rows red at every shape; the row parity dropped from the row
mover's map turns test_s16_rows red at every shape with more than one row; split32's 2^11 on the feature split's lo turns test_feat_split red
at every shape.  tests/test_glue_reference_cpu.py::test_symmetric_errors_are_rejected shows the first two without a GPU.

Measured figures go to profiles/glue_parity.json, only under CER_PARITY_RECORD (a plain run writes nothing): "1" writes the profile, any
other value is the path to write."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import glue_reference as G
from conftest import REPO
from test_oracle_golden import hashed

pytestmark = pytest.mark.gpu

GUARD = 1024
RECORD = {}
SHAPES = [(1, 1), (2, 16), (7, 17), (13, 37), (30, 64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    target = os.environ.get("CER_PARITY_RECORD", "")
    if target:
        path = os.path.join(REPO, "profiles", "glue_parity.json") if target == "1" else target
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
            f.write("\n")


def note(name, compared, ratio=None, unit="bytes_compared"):
    cur = RECORD.setdefault(name, {"cases": 0, unit: 0})
    cur["cases"] += 1
    cur[unit] += int(compared)
    if ratio is not None:
        cur["max_err_over_bound"] = max(cur.get("max_err_over_bound", 0.0), float(ratio))


class Arena:
    """``words`` int32 words between two guards of GUARD words, everything pre-filled with the sentinel."""

    def __init__(self, dev, words):
        self.n = int(words)
        self.all = torch.full((2 * GUARD + (self.n + 3) // 4 * 4,), G.SENTINEL, dtype=torch.int32, device=dev)

    @property
    def words(self):
        return self.all[GUARD:GUARD + self.n]

    def f32(self, *shape):
        v = self.words.view(torch.float32)
        return v.view(*shape) if shape else v

    def f16(self, *shape):
        v = self.words.view(torch.float16)
        return v.view(*shape) if shape else v

    def put(self, np_bytes, at=0):
        w = np.ascontiguousarray(np_bytes).view(np.int32).reshape(-1)
        self.words[at:at + w.size] = torch.from_numpy(w.copy()).to(self.all.device)

    def assert_is(self, want_words, where):
        """Body == want (numpy, any 4-byte-multiple dtype, compared as int32) and both guards untouched."""
        want = torch.from_numpy(np.ascontiguousarray(want_words).view(np.int32).reshape(-1).copy()).to(self.all.device)
        assert want.numel() == self.n, (where, want.numel(), self.n)
        if not torch.equal(self.words, want):
            bad = torch.nonzero(self.words != want).view(-1)
            raise AssertionError(f"{where}: {bad.numel()} of {self.n} words differ, first at word {int(bad[0])}: got "
                                 f"{int(self.words[bad[0]]) & 0xFFFFFFFF:#010x} want {int(want[bad[0]]) & 0xFFFFFFFF:#010x}")
        self.assert_guards(where)

    def assert_guards(self, where):
        assert bool((self.all[:GUARD] == G.SENTINEL).all()) and bool((self.all[GUARD + self.n:] == G.SENTINEL).all()), f"{where}: a guard was written"


def sentinel_words(n):
    return np.full(n, G.SENTINEL, np.int32)


def up(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _lib():
    from cer_mvs_amd import _lib as L
    return L, L.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------ transposes
def product_channel_counts():
    """The C values the product passes: the hidden state and the context (64 each, raft.py / update.py) and the concatenated GRU input ``cx``
    of ConvGRU.forward (update.py: inp | corr features | 7 x 7 disparity features)."""
    from cer_mvs_amd.update import UpdateBlock
    ub = UpdateBlock(dim_net=64, dim_inp=64, cascade=[(64, 64, 8), (-1, 320, 8)])       # RAFT's defaults (raft.py)
    cx = ub.gru.i_planes
    assert cx == ub.gru.convz.weight.shape[1] - ub.dim_net == ub.dim_inp + 64 + ub.size_disp_enc ** 2
    return sorted({ub.dim_net, ub.dim_inp, cx})


@pytest.mark.parametrize("direction", ["nchw_to_nhwc", "nhwc_to_nchw"])
def test_transposes(dev, direction):
    L, lib = _lib()
    counts = product_channel_counts()
    assert 177 in counts                                       # not a multiple of 4: the header's sentence says any C
    fn = getattr(lib, f"cer_{direction}_f32")
    for C in sorted({4, 64, 68, 132, 196} | set(counts)):
        for P in (1, 63, 64, 65, 193):
            x = hashed((C, P) if direction == "nchw_to_nhwc" else (P, C), 100 + C + P).numpy()
            xd = up(x, dev)
            for scale in (1.0, 0.125, 0.3):
                out = Arena(dev, C * P)
                L.check(fn(L.dev_ptr(xd, "src"), L.dev_ptr(out.f32(), "dst"), C, P, scale, L.cur_stream()), direction)
                want = (x * np.float32(scale)).T               # one rounding
                out.assert_is(bits(want), f"{direction} C={C} P={P} scale={scale}")
                note(f"cer_{direction}_f32", 4 * C * P)


@pytest.mark.parametrize("C,h,w,b", [(64, 5, 7, 2), (128, 9, 13, 0), (68, 3, 61, 3), (64, 1, 1, 2)])
def test_transpose_with_border(dev, C, h, w, b):
    L, lib = _lib()
    N, scale = 3, 0.125
    x = hashed((N, C, h, w), 200 + C + h).numpy()
    xd = up(x, dev)
    hp, wp = h + 2 * b, w + 2 * b
    out = Arena(dev, N * hp * wp * C)
    L.check(lib.cer_nchw_to_nhwc_border_f32(L.dev_ptr(xd, "src"), L.dev_ptr(out.f32(), "dst"), N, C, h, w, b, scale, L.cur_stream()), "border")
    want = np.zeros((N, hp, wp, C), np.float32)                # the border is +0.0
    want[:, b:b + h, b:b + w] = (x * np.float32(scale)).transpose(0, 2, 3, 1)
    out.assert_is(bits(want), f"border C={C} {h}x{w} b={b}")   # (the tail guard: nothing lands past N * Pp * C)
    note("cer_nchw_to_nhwc_border_f32", want.nbytes)


# ------------------------------------------------------------------------------------------------ segment copies
BIG = 4 * 256 * 1024 + 7                                       # more float4 than the 1024 x 256 threads of the capped grid: the loop wraps
SEG_LENGTHS = [(0, 1, 3, 4), (5, 1027, BIG, 3)]


@pytest.mark.parametrize("lengths", SEG_LENGTHS)
def test_copy_segments(dev, lengths):
    """Four segments per launch; source and destination offsets 0..3 floats mod 4 in all 16 combinations (both aligned: the 16-byte path with
    its scalar tail; otherwise the scalar path).  The whole destination allocation is compared: the segments byte-equal to their sources,
    every float between and around them untouched."""
    from cer_mvs_amd import ops
    total = sum(lengths) + 4 * 16 + 16
    src = (torch.arange(total, dtype=torch.int64, device=dev) * 2654435761 % 2147483629).to(torch.int32)     # any bit patterns: a mover moves bits
    for so in range(4):
        for do in range(4):
            dst = Arena(dev, total)
            want = sentinel_words(total)
            pairs, spos, dpos = [], 0, 0
            for n in lengths:
                s0 = (spos + 8 + 3) // 4 * 4 + so
                d0 = (dpos + 8 + 3) // 4 * 4 + do
                pairs.append((src[s0:s0 + n].view(torch.float32), dst.f32()[d0:d0 + n]))
                want[d0:d0 + n] = src[s0:s0 + n].cpu().numpy()
                spos, dpos = s0 + n, d0 + n
            assert dst.f32().data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
            ops.copy_segments(pairs)
            dst.assert_is(want, f"copy_segments lengths={lengths} src%4={so} dst%4={do}")
            note("cer_copy_segments_f32", 4 * total)


def _torch_copy(pairs):
    """The stand-in of tests/test_distributed_cpu.py for ops.copy_segments."""
    for src, dst in pairs:
        assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
        dst.view(-1).copy_(src.reshape(-1))


@pytest.mark.parametrize("w", [37, 48])
def test_strips_on_the_device(dev, w):
    """slab.pack_strips / slab.unpack_halves (plain path) with the kernel and with the torch stand-in: strips buffers and the refreshed
    (net, disp) byte-equal, guards included."""
    from cer_mvs_amd import slab
    h, C, Gr, halo = 45, 64, 3, 7
    assert slab.HALO == halo
    bounds = [slab.slab_bounds(h, Gr, g) for g in range(Gr)]
    full, fulld = hashed((h * w, C), 301).to(dev), hashed((h * w,), 302).to(dev)
    hb = slab.strip_half(w, C)
    bufs = {}
    for name, copy in (("kernel", slab._device_copy), ("torch", _torch_copy)):
        bufs[name] = []
        for r0, r1, e0, e1 in bounds:
            buf = Arena(dev, 2 * hb)
            slab.pack_strips(full[e0 * w:e1 * w].contiguous(), fulld[e0 * w:e1 * w].contiguous(), buf.f32(), w, r0, r1, e0, copy=copy)
            bufs[name].append(buf)
    for g in range(Gr):
        assert torch.equal(bufs["kernel"][g].all, bufs["torch"][g].all), f"pack_strips w={w} rank {g}"
        note("cer_copy_segments_f32", 8 * hb)
    for g, (r0, r1, e0, e1) in enumerate(bounds):
        got = {}
        for name, copy in (("kernel", slab._device_copy), ("torch", _torch_copy)):
            n = (e1 - e0) * w
            net, disp = Arena(dev, n * C), Arena(dev, n)
            # the owned rows hold data, the halo rows the sentinel: whatever the refresh does not write stays visible
            net.f32(n, C)[(r0 - e0) * w:(r1 - e0) * w] = full[r0 * w:r1 * w]
            disp.f32()[(r0 - e0) * w:(r1 - e0) * w] = fulld[r0 * w:r1 * w]
            prev_half = bufs["torch"][g - 1].f32()[hb:] if g > 0 else None
            next_half = bufs["torch"][g + 1].f32()[:hb] if g < Gr - 1 else None
            slab.unpack_halves(net.f32(n, C), disp.f32(), prev_half, next_half, w, g, Gr, r0, r1, e0, e1, copy=copy)
            got[name] = (net, disp)
        assert torch.equal(got["kernel"][0].all, got["torch"][0].all) and torch.equal(got["kernel"][1].all, got["torch"][1].all), (w, g)
        # and both are the full image's rows: the halo came from the right neighbour rows
        assert torch.equal(got["kernel"][0].f32((e1 - e0) * w, C), full[e0 * w:e1 * w]) and torch.equal(got["kernel"][1].f32(), fulld[e0 * w:e1 * w])
        note("cer_copy_segments_f32", 4 * (e1 - e0) * w * (C + 1))


# ------------------------------------------------------------------------------------------------ m-tile-major layouts
def _layout_reference(layout, x, h, w, C, log2s):
    if layout == G.FRAG16:
        return G.frag16_bytes(x, h, w, C, 2.0 ** log2s)
    return G.acc32_bytes(x, h, w, C) if layout == G.ACC32 else G.f32x8_bytes(x, h, w, C)


@pytest.mark.parametrize("layout", [G.FRAG16, G.ACC32, G.F32X8])
@pytest.mark.parametrize("h,w", SHAPES)
def test_s16_layouts(dev, layout, h, w):
    from cer_mvs_amd import _lib as L, ops
    assert (L.S16_FRAG16, L.S16_ACC32, L.S16_F32X8) == (G.FRAG16, G.ACC32, G.F32X8)
    name = ("frag16", "acc32", "f32x8")[layout]
    for C in (16, 32, 64, 128):
        if layout == G.ACC32 and C % 32:
            continue
        log2s = L.S16_RELU
        x = hashed((h * w, C), 400 + h + C).numpy() * 3.0
        PP = G.s16_pixels(h, w)
        assert PP == ops.s16_pixels(h, w)
        ref = _layout_reference(layout, x, h, w, C, log2s)
        covered = G.covered_bytes(layout, h, w, C)
        # forward: the reference's bytes where the layout writes, the sentinel where it must not (the padding pixels)
        out = Arena(dev, PP * C)
        ops.s16_layout(up(x, dev), h, w, layout, log2s, out=out.f32(PP, C))
        want = sentinel_words(PP * C).view(np.uint8)
        want[covered] = ref[covered]
        out.assert_is(want, f"s16_layout {name} forward {h}x{w} C={C}")
        # inverse of the reference tensor (padding zero)
        back = Arena(dev, h * w * C)
        ops.s16_layout(up(ref.view(np.float32).reshape(PP, C), dev), h, w, layout, log2s, inverse=True, out=back.f32(h * w, C))
        want_back = G.from_frag16(ref, h, w, C, 2.0 ** -log2s) if layout == G.FRAG16 else x
        back.assert_is(bits(want_back), f"s16_layout {name} inverse {h}x{w} C={C}")
        note(f"cer_s16_layout_f32/{name}", 4 * PP * C + 4 * h * w * C)


def test_frag16_values(dev):
    """Every hi / lo half equals split_f16, the inverse equals the join, for the four operand scales and the value classes a split must get
    right (signed zeros, far below the quantum, lo subnormal, hi subnormal, the clamp boundary itself, far beyond it)."""
    from cer_mvs_amd import _lib as L, ops
    h, w, C = 7, 17, 16
    PP = G.s16_pixels(h, w)
    for log2s in (L.S16_UNIT, L.S16_RELU, L.S16_DISP, 0):
        scale = 2.0 ** log2s
        x = hashed((h * w * C,), 500 + log2s).numpy() * np.float32(4000.0 / scale)
        cls = G.value_classes(scale)
        at = np.arange(0, x.size, 7)[:4 * cls.size]
        x[at] = np.tile(cls, 4)[:at.size]
        x = x.reshape(h * w, C)
        out = Arena(dev, PP * C)
        out.words.zero_()
        ops.s16_layout(up(x, dev), h, w, L.S16_FRAG16, log2s, out=out.f32(PP, C))
        got_hi, got_lo = G.frag16_halves(out.words.cpu().numpy().view(np.uint8), h, w, C)
        hi, lo = G.split_f16(x, scale)
        assert np.array_equal(got_hi.view(np.int16), hi.view(np.int16)), f"hi halves, log2s={log2s}"
        assert np.array_equal(got_lo.view(np.int16), lo.view(np.int16)), f"lo halves, log2s={log2s}"
        assert (lo.view(np.int16) & 0x7C00 == 0)[lo != 0].any() and (hi == np.float16(65504)).any() and (hi.view(np.int16) == -32768).any()
        out.assert_guards(f"frag16 values log2s={log2s}")
        back = Arena(dev, h * w * C)
        ops.s16_layout(out.f32(PP, C), h, w, L.S16_FRAG16, log2s, inverse=True, out=back.f32(h * w, C))
        back.assert_is(bits(G.join_frag16(hi, lo, 2.0 ** -log2s)), f"frag16 join log2s={log2s}")
        note("cer_s16_layout_f32/frag16_values", 4 * PP * C + 4 * h * w * C)


def _row_cases(h):
    cases = [(0, 1), (1, 1), (0, 7), (1, 7), (6, 7), (h - 7, 7), (3, 4)]
    return sorted({(y0, n) for y0, n in cases if y0 >= 0 and y0 + n <= h})


@pytest.mark.parametrize("h,w", SHAPES)
def test_s16_rows(dev, h, w):
    from cer_mvs_amd import ops
    for C in (16, 64):
        PP = G.s16_pixels(h, w)
        src_img, old_img = hashed((h * w, C), 600 + h + C).numpy(), hashed((h * w, C), 650 + h + C).numpy()
        src_t, old_t = G.frag16_bytes(src_img, h, w, C, 2.0 ** 14), G.frag16_bytes(old_img, h, w, C, 2.0 ** 14)
        covered = G.covered_bytes(G.FRAG16, h, w, C)
        old_sent = sentinel_words(PP * C).view(np.uint8)       # the old image with the SENTINEL in its padding pixels
        old_sent[covered] = old_t[covered]
        src_dev = up(src_t.view(np.float32).reshape(PP, C), dev)
        cases = _row_cases(h)
        assert cases and (h < 13 or {(1, 7), (6, 7), (0, 7)} <= set(cases))
        for y0, n in cases:
            where = f"s16_rows {h}x{w} C={C} y0={y0} n={n}"
            plain = G.rows_plain_bytes(src_t, h, w, C, y0, n)
            # out: tensor -> rows
            rows = Arena(dev, n * w * C)
            ops.s16_rows(src_dev, rows.f32(), h, w, y0, n, False)
            rows.assert_is(plain, where + " out")
            # in: rows -> a tensor that holds another image; only the pieces of those rows may change (not the other row of a shared m-tile,
            # not the padding)
            tensor = Arena(dev, PP * C)
            tensor.put(old_sent)
            ops.s16_rows(tensor.f32(PP, C), up(plain.view(np.float32), dev), h, w, y0, n, True)
            tensor.assert_is(G.rows_into_tensor_bytes(old_sent, plain, h, w, C, y0, n), where + " in")
            note("cer_s16_rows_f32", 4 * n * w * C + 4 * PP * C)


# ------------------------------------------------------------------------------------------------ split32
def test_split32(dev):
    from cer_mvs_amd import ops
    cls = G.value_classes(1.0)
    for P in (1, 7, 910):
        for C in (32, 64, 96, 128):
            x = hashed((P * C,), 700 + P + C).numpy() * np.float32(300.0)
            k = min(cls.size, x.size)
            x[:k] = cls[:k]
            x = x.reshape(P, C)
            ref = G.split32_bytes(x)
            out = Arena(dev, P * C)
            ops.split32(up(x, dev), out=out.f32(P, C))
            out.assert_is(ref, f"split32 forward P={P} C={C}")
            back = Arena(dev, P * C)
            ops.split32(up(ref.view(np.float32).reshape(P, C), dev), inverse=True, out=back.f32(P, C))
            back.assert_is(bits(G.from_split32(ref, P, C)), f"split32 inverse P={P} C={C}")
            note("cer_split32_f32", 8 * P * C)


# ------------------------------------------------------------------------------------------------ feature planes
def _feat_split(dev, x, blocks, bt, flag0=0):
    L, lib = _lib()
    out, flag = Arena(dev, blocks * bt * 64), Arena(dev, 1)
    flag.words.fill_(flag0)
    L.check(lib.cer_feat_split_f16(L.dev_ptr(up(x, dev), "x"), L.dev_ptr(out.f16(), "out", torch.float16), blocks, bt, 64,
                                   L.dev_ptr(flag.words, "flag", torch.int32), L.cur_stream()), "feat_split")
    flag.assert_guards("feat_split flag")
    return out, int(flag.words[0])


@pytest.mark.parametrize("blocks,bt", [(1, 1), (3, 37), (2, 256), (5, 129)])
def test_feat_split(dev, blocks, bt):
    x = hashed((blocks, bt, 64), 800 + bt).numpy() * np.float32(900.0)
    cls = G.value_classes(64.0)
    at = np.arange(0, x.size, 5)[:cls.size]
    x.reshape(-1)[at] = cls[:at.size]
    x[np.abs(x) > 1023.5] = 1000.0                             # (1e9 of the value classes belongs to the clamp cases below)
    out, flag = _feat_split(dev, x, blocks, bt)
    out.assert_is(G.feat_split_bytes(x, blocks, bt), f"feat_split blocks={blocks} bt={bt}")
    assert flag == 0
    note("cer_feat_split_f16", 256 * blocks * bt)
    # the clamp boundary: x * 64 = +-65504 exactly does not raise the flag ...
    edge = x.copy()
    edge[-1, -1, 63], edge[0, 0, 0] = 1023.5, -1023.5
    out, flag = _feat_split(dev, edge, blocks, bt)
    out.assert_is(G.feat_split_bytes(edge, blocks, bt), f"feat_split at the clamp blocks={blocks} bt={bt}")
    assert flag == 0 and not G.feat_saturates(edge).any()
    note("cer_feat_split_f16", 256 * blocks * bt)
    # ... the next float above, inf and NaN each raise bit 1; bytes are compared at the finite elements
    for bad in (np.nextafter(np.float32(1023.5), np.float32(2000.0)), np.float32(np.inf), np.float32(np.nan)):
        over = x.copy()
        over[-1, bt // 2, 37] = bad
        assert G.feat_saturates(over).sum() == 1
        out, flag = _feat_split(dev, over, blocks, bt, flag0=4)
        assert flag == 5, (bad, flag)
        finite = np.isfinite(over)
        got = out.words.cpu().numpy().view(np.float16).reshape(blocks, 8, bt, 16)
        got_hi = got[:, :4].transpose(0, 2, 1, 3).reshape(blocks, bt, 64)
        got_lo = got[:, 4:].transpose(0, 2, 1, 3).reshape(blocks, bt, 64)
        hi, lo = G.split_f16(over, 64.0)
        assert np.array_equal(got_hi.view(np.int16)[finite], hi.view(np.int16)[finite]) and np.array_equal(got_lo.view(np.int16)[finite], lo.view(np.int16)[finite])
        out.assert_guards("feat_split over the clamp")
        note("cer_feat_split_f16", 4 * int(finite.sum()))


@pytest.mark.parametrize("h,w,border", [(1, 1, 2), (5, 7, 2), (9, 13, 0), (6, 33, 3)])
def test_feat_ref_rows(dev, h, w, border):
    from cer_mvs_amd import ops
    Pb = (h + 2 * border) * (w + 2 * border)
    slot = (np.arange(8 * Pb * 16, dtype=np.int64) % 65521 - 32760).astype(np.int16)        # a counting pattern: every half says where it came from
    out = Arena(dev, h * w * 64)
    ops.feat_ref_rows(up(slot, dev).view(torch.float16).view(Pb, 128), h, w, border, out=out.f16(h * w, 128))
    out.assert_is(G.feat_ref_rows_bytes(slot, h, w, border), f"feat_ref_rows {h}x{w} b={border}")
    note("cer_feat_ref_rows_f16", 256 * h * w)


# ------------------------------------------------------------------------------------------------ saturation scan
def _scan(dev, halves, flag0=0):
    """cer_f16_scan_overflow with bit 4 on a test-owned flag; halves: numpy int16 (a multiple of 8)."""
    L, lib = _lib()
    flag = Arena(dev, 1)
    flag.words.fill_(flag0)
    data = up(halves, dev) if isinstance(halves, np.ndarray) else halves
    nbytes = data.numel() * data.element_size()
    L.check(lib.cer_f16_scan_overflow(ctypes.c_void_p(data.data_ptr()), nbytes, L.dev_ptr(flag.words, "flag", torch.int32), 4, L.cur_stream()), "scan")
    flag.assert_guards("scan flag")
    note("cer_f16_scan_overflow", nbytes)
    return int(flag.words[0])


def test_scan_overflow(dev):
    n = (3 * 256 + 5) * 8                                      # 773 pieces of 16 bytes: three full blocks and a ragged one
    as_i16 = lambda p: np.array(p, np.uint16).astype(np.int16)
    zero = np.zeros(n, np.int16)
    assert _scan(dev, zero) == 0 and _scan(dev, zero, 1) == 1
    # a single offending half: first piece / last piece x low / high half of a word
    for pattern in (0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00):   # +-65504, +-inf, NaN
        for pos in (0, 1, n - 8, n - 1, n // 2 + 3):
            buf = zero.copy()
            buf[pos] = as_i16(pattern)
            assert _scan(dev, buf) == 4, (hex(pattern), pos)
    for pattern in (0x7BFE, 0xFBFE):                           # the largest value below the clamp: clean, wherever it stands
        assert _scan(dev, np.full(n, as_i16(pattern), np.int16)) == 0, hex(pattern)
    hit = zero.copy()
    hit[n - 3] = as_i16(0x7BFF)
    assert _scan(dev, hit, 1) == 5                             # or-ed into a flag that is already set
    assert _scan(dev, np.full(n, as_i16(0x3C00), np.int16), 1) == 1


def test_scan_overflow_strides_past_the_grid_cap(dev):
    """2048 blocks x 256 threads x 16 bytes is one pass of the capped grid; the only hit sits in the piece behind it."""
    n = (2048 * 256 * 16 + 16) // 2
    buf = torch.zeros(n, dtype=torch.int16, device=dev)
    assert _scan(dev, buf) == 0
    buf[n - 8 + 5] = 0x7BFF
    assert _scan(dev, buf) == 4 and _scan(dev, buf, 1) == 5


# ------------------------------------------------------------------------------------------------ pyramid
@pytest.mark.parametrize("rows,D,L,stride", [(1, 64, 3, 112), (257, 44, 3, 80), (300, 5, 3, 16), (33, 3, 2, 4), (513, 64, 1, 64), (40, 40, 4, 96)])
def test_pyramid(dev, rows, D, L, stride):
    from cer_mvs_amd import ops
    need = G.pyramid_need(D, L)
    level0 = hashed((rows, D), 900 + rows).numpy() * np.float32(7.0)
    for scale in (1.0, 1.0 / 3):
        vol = Arena(dev, rows * stride)
        start = sentinel_words(rows * stride).reshape(rows, stride)
        start[:, :D] = bits(level0)                            # behind level 0 everything is the sentinel: the levels and the gap
        vol.put(start)
        ops.pyramid(vol.f32(rows, stride), D, L, scale=scale)
        want = start.copy()
        want[:, :need] = bits(G.pyramid_rows(start.view(np.float32), D, stride, L, scale))
        vol.assert_is(want, f"pyramid rows={rows} D={D} L={L} stride={stride} scale={scale}")
        note("cer_pyramid_f32", 4 * rows * stride)


# ------------------------------------------------------------------------------------------------ instance-norm glue
PLANES = [(12, 20), (5, 7), (1, 1), (128, 128), (128, 129), (129, 129), (2, 8194)]
EPS = 1e-5


def _plane_inputs(H, W, seed):
    """Six planes: constant 3.0; mean 100, std 0.01; the rest hashed."""
    plane = H * W
    x = hashed((6, plane), seed).numpy()
    x[0] = 3.0
    x[1] = np.float32(100.0) + hashed((plane,), seed + 1).numpy() * np.float32(0.01 * 3 ** 0.5)
    x[3] = x[3] * 50.0 - 20.0
    return x


@pytest.mark.parametrize("H,W", PLANES)
def test_plane_stats(dev, H, W):
    L, lib = _lib()
    plane = H * W
    x = _plane_inputs(H, W, 1000 + plane)
    stats = Arena(dev, 12)
    L.check(lib.cer_plane_stats_f32(L.dev_ptr(up(x, dev), "x"), L.dev_ptr(stats.f32(), "stats"), 6, plane, EPS, L.cur_stream()), "plane_stats")
    stats.assert_guards(f"plane_stats {H}x{W}")
    got = stats.f32(6, 2).cpu().numpy().astype(np.float64)
    mean, var, ex2, eps = G.plane_stats64(x, EPS)
    mean32 = mean.astype(np.float32)
    ulp = np.spacing(np.abs(mean32)).astype(np.float64)
    err_mean = np.abs(got[:, 0] - mean32.astype(np.float64))
    rstd = 1.0 / np.sqrt(var + eps)
    bound = 2.0 ** -23 + 0.5 * plane * 2.0 ** -52 * ex2 / (var + eps)
    err_rstd = np.abs(got[:, 1] - rstd) / rstd
    print(f"  plane_stats {H}x{W}: mean err / ulp {err_mean / ulp}, rstd err / bound {err_rstd / bound}")
    assert (err_mean <= ulp).all(), (H, W, err_mean / ulp)
    assert (err_rstd <= bound).all(), (H, W, err_rstd / bound)
    note("cer_plane_stats_f32", 12, ratio=max((err_mean / ulp).max(), (err_rstd / bound).max()), unit="elements_compared")


COMBOS = ["stats", "stats+res+rstats", "stats+res", "res", "plain"]       # which of x_stats / res / res_stats the launch gets


@pytest.mark.parametrize("H,W", PLANES)
def test_norm_act(dev, H, W):
    """6 planes in the middle of a 14-plane allocation; flags x combinations x (out=None | out=x)."""
    from cer_mvs_amd import ops
    plane = H * W
    lead = 4                                                   # planes in front: keeps the launch's first plane 16-byte aligned for any size
    x = _plane_inputs(H, W, 1100 + plane)
    r = hashed((6, plane), 1200 + plane).numpy() * np.float32(2.0) + np.float32(0.25)
    xd, rd = up(x, dev).view(1, 6, H, W), up(r, dev).view(1, 6, H, W)
    xs_d, rs_d = ops.plane_stats(xd, EPS), ops.plane_stats(rd, EPS)        # the kernel's OWN statistics feed kernel and reference
    xs, rs = xs_d.cpu().numpy(), rs_d.cpu().numpy()
    for flags in (0, 1, 5, 7):
        for combo in COMBOS:
            use_xs, use_res, use_rs = combo.startswith("stats"), "res" in combo, "rstats" in combo
            ref, t, u = G.norm_act64(x, xs if use_xs else None, r if use_res else None, rs if use_rs else None, flags)
            bound = 2.0 ** -22 * (np.abs(t) + np.abs(u)) + 2.0 ** -149
            exact = not use_xs and not use_rs                  # a copy or one fp32 sum (and ReLUs): no error allowed
            kw = dict(x_stats=xs_d if use_xs else None, res=rd if use_res else None, res_stats=rs_d if use_rs else None,
                      relu_a=bool(flags & 1), relu_b=bool(flags & 2), relu_out=bool(flags & 4))
            for in_place in (False, True):
                where = f"norm_act {H}x{W} flags={flags} {combo} {'out=x' if in_place else 'out=None'}"
                if in_place:
                    buf = Arena(dev, 14 * plane)
                    xin = buf.f32()[lead * plane:(lead + 6) * plane].view(1, 6, H, W)
                    xin.copy_(xd)
                    out = ops.norm_act(xin, out=xin, **kw)
                    assert out.data_ptr() == xin.data_ptr()
                    # the other planes of the allocation and the guards
                    assert bool((buf.words[:lead * plane] == G.SENTINEL).all()) and bool((buf.words[(lead + 6) * plane:] == G.SENTINEL).all()), where
                    buf.assert_guards(where)
                else:
                    out = ops.norm_act(xd, **kw)
                    assert torch.equal(xd.view(-1).view(torch.int32), up(bits(x).reshape(-1), dev)), where + ": x changed"
                got = out.view(6, plane).cpu().numpy()
                err = np.abs(got.astype(np.float64) - ref)
                if exact:
                    assert np.array_equal(got, ref.astype(np.float32)), where + ": must be exact"
                assert (err <= bound).all(), (where, float((err / bound).max()))
                note("cer_norm_act_f32", 6 * plane, ratio=float((err / bound).max()), unit="elements_compared")
