"""tests/glue_reference.py checks itself: no GPU, no library.

The GPU file compares kernels with these restatements byte by byte, so an error here that mirrors an error in a kernel would pass there.
What stands against that: every layout map is a bijection onto distinct byte ranges whose complement is exactly the padding pixels; the
vectorised form (an index table per (pixel, channel)) equals a second form that walks the storage in its own order; the row mover's plain
side equals rows cut from the whole image's tensor; the splits reconstruct to the header's 2^-22; the pyramid equals F.avg_pool2d.
The last test perturbs the maps the way a symmetric kernel error would (kg and li swapped, the row parity dropped) and shows that the
checks above reject each."""
import numpy as np
import pytest
import torch

import glue_reference as G
from test_oracle_golden import hashed

SHAPES = [(1, 1), (2, 16), (7, 17), (13, 37), (30, 64)]
LAYOUTS = [(G.FRAG16, (16, 32, 64, 128)), (G.ACC32, (32, 64, 128)), (G.F32X8, (16, 32, 64, 128))]


def _x(shape, seed):
    return hashed(shape, seed).numpy()


def _padding_bytes(h, w, C, unit):
    """Bool per byte: belongs to a padding pixel.  ``unit`` = bytes one (pixel, lane) piece spans in a 1 KiB plane (16), planes per m-tile
    follow from C: in every layout a 1 KiB plane is 64 pieces of 16 bytes = (kg, li), so byte b belongs to lane order li = (b / 16) % 32 of
    m-tile b / (C * 128)."""
    n = G.s16_pixels(h, w) * C * 4
    b = np.arange(n)
    tile, li = b // (C * 4 * G.MT_PIXELS), (b // unit) % G.MT_PIXELS
    tiles_across = -(-w // G.MT_COLS)
    y = tile // tiles_across * 2 + li // 16
    x = tile % tiles_across * 16 + li % 16
    return (y >= h) | (x >= w)


@pytest.mark.parametrize("layout,channels", LAYOUTS)
def test_layout_maps_are_bijections_onto_the_non_padding_bytes(layout, channels):
    for h, w in SHAPES:
        for C in channels:
            starts, width = G.layout_ranges(layout, h, w, C)
            n = G.s16_pixels(h, w) * C * 4
            flat = (starts.reshape(-1, 1) + np.arange(width)).reshape(-1)
            assert flat.min() >= 0 and flat.max() < n
            assert np.unique(flat).size == flat.size == h * w * C * 4, (layout, h, w, C)        # distinct ranges, every data byte once
            assert (starts % width == 0).all()
            hit = np.zeros(n, bool)
            hit[flat] = True
            assert np.array_equal(hit, G.covered_bytes(layout, h, w, C))
            assert np.array_equal(~hit, _padding_bytes(h, w, C, 16)), (layout, h, w, C)          # what is not hit is exactly the padding


@pytest.mark.parametrize("layout,channels", LAYOUTS)
def test_inverse_of_forward_is_the_identity(layout, channels):
    for h, w in SHAPES:
        for C in channels:
            x = _x((h * w, C), 11 + h + C)
            if layout == G.FRAG16:
                hi, lo = G.frag16_halves(G.frag16_bytes(x, h, w, C, 16.0), h, w, C)
                want_hi, want_lo = G.split_f16(x, 16.0)
                assert np.array_equal(hi.view(np.int16), want_hi.view(np.int16)) and np.array_equal(lo.view(np.int16), want_lo.view(np.int16))
            elif layout == G.ACC32:
                assert np.array_equal(G.from_acc32(G.acc32_bytes(x, h, w, C), h, w, C).view(np.int32), x.view(np.int32))
            else:
                assert np.array_equal(G.from_f32x8(G.f32x8_bytes(x, h, w, C), h, w, C).view(np.int32), x.view(np.int32))


def test_vectorised_forms_equal_the_storage_order_walks():
    h, w = 5, 19                                               # odd height, two tile columns, the second ragged
    x = _x((h * w, 32), 21)
    assert np.array_equal(G.frag16_bytes(x, h, w, 32, 64.0), G.frag16_bytes_scalar(x, h, w, 32, 64.0))
    assert np.array_equal(G.acc32_bytes(x, h, w, 32), G.acc32_bytes_scalar(x, h, w, 32))
    assert np.array_equal(G.f32x8_bytes(x, h, w, 32), G.f32x8_bytes_scalar(x, h, w, 32))
    x64 = _x((3 * 17, 64), 22)                                 # more than one 32-channel tile / 16-channel group
    assert np.array_equal(G.acc32_bytes(x64, 3, 17, 64), G.acc32_bytes_scalar(x64, 3, 17, 64))
    assert np.array_equal(G.frag16_bytes(x64, 3, 17, 64, 1.0), G.frag16_bytes_scalar(x64, 3, 17, 64, 1.0))
    xs = _x((7, 96), 23)
    assert np.array_equal(G.split32_bytes(xs), G.split32_bytes_scalar(xs))


def test_feat_split_bytes_equal_the_address_formula_of_the_header():
    """Header / kernel comment: halves of (block b, texel t, plane p, channel 16 ks + c) at ((b * 8 + p) * bt + t) * 16 + c."""
    blocks, bt = 3, 5
    x = _x((blocks, bt, 64), 31)
    got = G.feat_split_bytes(x, blocks, bt).view(np.float16)
    hi, lo = G.split_f16(x, 64.0)
    for b in range(blocks):
        for t in range(bt):
            for ch in range(64):
                ks, c = divmod(ch, 16)
                assert got[((b * 8 + ks) * bt + t) * 16 + c] == hi[b, t, ch]
                assert got[((b * 8 + 4 + ks) * bt + t) * 16 + c] == lo[b, t, ch]


@pytest.mark.parametrize("y0", [0, 1, 3, 6])
def test_rows_plain_equals_rows_cut_from_the_whole_image(y0):
    h, w, C, n = 13, 37, 32, 7
    x = _x((h * w, C), 41)
    whole = G.frag16_bytes(x, h, w, C, 2.0 ** 14)
    rows = G.rows_plain_bytes(whole, h, w, C, y0, n).reshape(n * w, C // 8, 2, 8, 2)
    hi, lo = G.split_f16(x[y0 * w:(y0 + n) * w], 2.0 ** 14)
    assert np.array_equal(rows[:, :, 0].reshape(n * w, C, 2), hi.view(np.uint8).reshape(n * w, C, 2))
    assert np.array_equal(rows[:, :, 1].reshape(n * w, C, 2), lo.view(np.uint8).reshape(n * w, C, 2))
    # and back: into a tensor of another image, only the pieces of those rows change
    other = G.frag16_bytes(_x((h * w, C), 42), h, w, C, 2.0 ** 14)
    xo =_x((h * w, C), 42)
    mixed = np.concatenate([xo[:y0 * w], x[y0 * w:(y0 + n) * w], xo[(y0 + n) * w:]])
    assert np.array_equal(G.rows_into_tensor_bytes(other, rows.reshape(-1), h, w, C, y0, n), G.frag16_bytes(mixed, h, w, C, 2.0 ** 14))


def test_splits_reconstruct_to_the_header_bounds():
    x = np.concatenate([_x((4096,), 51), _x((4096,), 52) * 1000.0, _x((4096,), 53) * 1e-3]).astype(np.float32)
    for scale in (1.0, 16.0, 64.0):
        keep = np.abs(x * np.float32(scale)) < 60000.0         # away from the clamp
        hi, lo = G.split_f16(x, scale)
        back = G.join_frag16(hi, lo, 1.0 / scale).astype(np.float64)
        # the residual's f16 rounding is 2^-11 of a residual that is 2^-11 of x: 2^-22; below the f16 normal range the quantum 2^-24 / scale rules
        tol = 2.0 ** -22 * np.abs(x[keep]) + 2.0 ** -25 / scale
        assert (np.abs(back[keep] - x[keep]) <= tol).all()
    keep = np.abs(x) < 60000.0
    hi, lo = G.split32_f16(x)
    back = G.join_split32(hi, lo).astype(np.float64)
    assert (np.abs(back[keep] - x[keep]) <= 2.0 ** -22 * np.abs(x[keep]) + 2.0 ** -36).all()
    # the clamp: +-65504 itself is kept, beyond it saturates
    hi, lo = G.split_f16(np.float32([1023.5, 1e9, -1e9, np.inf]), 64.0)
    assert hi.tolist() == [65504.0, 65504.0, -65504.0, 65504.0] and lo.tolist() == [0.0, 0.0, 0.0, 0.0]
    assert G.feat_saturates(np.float32([1023.5, np.nextafter(np.float32(1023.5), np.float32(2000)), np.inf, np.nan, -1023.5])).tolist() == \
        [False, True, True, True, False]


@pytest.mark.parametrize("D,L,scale", [(64, 3, 1.0), (44, 3, 1.0 / 3), (40, 4, 1.0), (8, 1, 0.5)])
def test_pyramid_rows_equal_avg_pool(D, L, scale):
    import torch.nn.functional as F
    stride = G.pyramid_need(D, L) + 5
    vol = _x((9, stride), 61)
    got = G.pyramid_rows(vol, D, stride, L, scale)
    level = torch.from_numpy(vol[:, :D].copy())
    if np.float32(scale) != 1.0:
        level = level * torch.tensor(np.float32(scale))
    want = []
    for _ in range(L):
        want.append(level)
        level = F.avg_pool2d(level[None, None], [1, 2], stride=[1, 2])[0, 0]
    assert np.array_equal(got.view(np.int32), torch.cat(want, 1).numpy().view(np.int32))


def test_pyramid_rows_floor_the_halved_length():
    got = G.pyramid_rows(np.arange(16, dtype=np.float32)[None], 5, 16, 3, 1.0)
    assert G.pyramid_need(5, 3) == 8 and got[0].tolist() == [0, 1, 2, 3, 4, 0.5, 2.5, 1.5]


def test_feat_ref_rows_slices_the_interior():
    h, w, b = 3, 4, 2
    slot = np.arange(8 * (h + 2 * b) * (w + 2 * b) * 16, dtype=np.int64).astype(np.int16)
    out = G.feat_ref_rows_bytes(slot, h, w, b).view(np.int16).reshape(8, h, w, 16)
    for p in range(8):
        for y in range(h):
            for x in range(w):
                at = ((p * (h + 2 * b) + y + b) * (w + 2 * b) + x + b) * 16
                assert np.array_equal(out[p, y, x], slot[at:at + 16])


def test_norm_act64_and_plane_stats64():
    x = _x((3, 35), 71) * 2 + 5
    mean, var, ex2, eps = G.plane_stats64(x, 1e-5)
    t = torch.from_numpy(x).double()
    assert np.allclose(mean, t.mean(1).numpy(), rtol=1e-15) and np.allclose(var, t.var(1, unbiased=False).numpy(), rtol=1e-12)
    assert np.allclose(ex2, var + mean ** 2, rtol=1e-12) and eps == np.float64(np.float32(1e-5)) != 1e-5
    xs = np.stack([mean, 1 / np.sqrt(var + eps)], 1).astype(np.float32)
    r = _x((3, 35), 72)
    out, tt, uu = G.norm_act64(x, xs, r, None, 7)
    ts = torch.from_numpy(xs).double()
    want = torch.relu(torch.relu((t - ts[:, 0:1]) * ts[:, 1:2]) + torch.relu(torch.from_numpy(r).double()))
    assert np.array_equal(out, want.numpy()) and np.array_equal(out, np.maximum(tt + uu, 0))
    out, tt, uu = G.norm_act64(x, None, None, None, 0)
    assert np.array_equal(out, x.astype(np.float64)) and not uu.any()


def test_symmetric_errors_are_rejected():
    """A kernel whose forward and inverse share a wrong index passes a round trip.  Against the reference it cannot: the same error put into
    the reference's maps breaks the properties above, so the maps the GPU file compares with are not satisfied by it."""
    h, w, C = 7, 17, 32
    good = G.frag16_map(h, w, C)
    mt, li = G._tile_lane(h, w)
    c = np.arange(C)
    # (a) kg and li swapped inside the plane: piece (li, kg) instead of (kg, li)
    swapped = (mt[:, None] * (C // 16) + c[None] // 16) * 2048 + (li[:, None] * 2 + (c[None] % 16) // 8) * 16 + c[None] % 8 * 2
    assert np.unique(swapped).size == swapped.size             # still a bijection: a round trip through it is the identity ...
    assert not np.array_equal(swapped, good)
    x = _x((h * w, C), 81)
    n = G.s16_pixels(h, w) * C * 4
    hi, lo = G.split_f16(x, 1.0)
    wrong = G._scatter(swapped, hi, n) | G._scatter(swapped + 1024, lo, n)
    assert not np.array_equal(wrong, G.frag16_bytes_scalar(x, h, w, C, 1.0))                     # ... but the storage-order walk rejects it,
    hit = np.zeros(n, bool)
    hit[(swapped.reshape(-1, 1) + np.arange(2)).reshape(-1)] = True
    hit[(swapped.reshape(-1, 1) + 1024 + np.arange(2)).reshape(-1)] = True
    assert not np.array_equal(~hit, _padding_bytes(h, w, C, 16))                                # and so does the padding test
    # (b) the row parity dropped from the lane order (li = x & 15): two image rows of an m-tile collide
    y, xx = np.divmod(np.arange(h * w), w)
    flat_li = xx % 16
    dropped = (mt[:, None] * (C // 16) + c[None] // 16) * 2048 + ((c[None] % 16) // 8 * 32 + flat_li[:, None]) * 16 + c[None] % 8 * 2
    assert np.unique(dropped).size < dropped.size
    # (c) the same in the row mover: rows cut with the parity dropped differ from the rows of the image for odd AND even y0
    whole = G.frag16_bytes(x, h, w, C, 1.0)
    for y0 in (0, 1):
        want = G.rows_plain_bytes(whole, h, w, C, y0, 3)
        span = np.arange(16)
        pieces = dropped[y0 * w:(y0 + 3) * w, ::8]
        got = np.stack([whole[pieces[..., None] + span], whole[pieces[..., None] + 1024 + span]], 2).reshape(-1)
        assert not np.array_equal(got, want)
