"""numpy restatements of the layout, mover and glue kernels, bit for bit (tests/test_glue_reference_cpu.py checks this file against
itself, tests/test_glue_parity_gpu.py compares the kernels with it byte by byte).

Everything here is written from the words of include/cer_mvs.h (and the comment block above ``s16_layout_kernel``), not from the kernels'
index expressions: every map is an index table built per (pixel, channel) from the sentence that describes the layout, and a second,
scalar form (``*_scalar``) walks the STORAGE in its own order - m-tile, channel group, plane, lane, element - and asks which element of the
image lives there.  The two forms share no expression; tests/test_glue_reference_cpu.py requires them to agree.

Arithmetic is stated in numpy's IEEE types: float32 products, sums and differences are single operations, each rounded once (the library
is built with -ffp-contract=off), ``astype(float16)`` rounds to nearest even with gradual underflow."""
import numpy as np

F16_MAX = np.float32(65504.0)
MT_ROWS, MT_COLS, MT_PIXELS = 2, 16, 32          # an m-tile: 2 rows x 16 columns of pixels
KIB = 1024
FRAG16, ACC32, F32X8 = 0, 1, 2                   # cer_s16_layout_f32 layouts
SENTINEL = 0x7FC5A5A5                            # a quiet NaN with a payload: what the GPU tests pre-fill outputs and guards with


# ------------------------------------------------------------------------------------------------ split arithmetic
def _clamped(x, scale):
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(x, np.float32) * np.float32(scale)
    return np.minimum(np.maximum(t, -F16_MAX), F16_MAX)


def split_f16(x, scale):
    """(hi, lo) of the s16 / feature split: t = clip(x * scale, +-65504), hi = f16(t), lo = f16(t - hi) (unscaled residual)."""
    t = _clamped(x, scale)
    hi = t.astype(np.float16)
    lo = (t - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split32_f16(x):
    """(hi, lo) of the split32 layout: scale 1, lo = f16((t - hi) * 2^11)."""
    t = _clamped(x, 1.0)
    hi = t.astype(np.float16)
    lo = ((t - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def join_frag16(hi, lo, inv):
    """(float32(hi) + float32(lo)) * inv, each step rounded to fp32."""
    return (hi.astype(np.float32) + lo.astype(np.float32)) * np.float32(inv)


def join_split32(hi, lo):
    """fma(lo, 2^-11, hi): one rounding.  lo * 2^-11 + hi is exact in float64 (two 11-bit significands at most 2^40 apart)."""
    return (lo.astype(np.float64) / 2048.0 + hi.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ m-tile-major layouts
def s16_pixels(h, w):
    """ceil(h/2) * ceil(w/16) m-tiles of 32 pixels."""
    return -(-h // MT_ROWS) * -(-w // MT_COLS) * MT_PIXELS


def _tile_lane(h, w):
    """Per pixel of the h x w image (row-major): its m-tile (m-tiles are numbered row by row of tiles) and its lane order li."""
    y, x = np.divmod(np.arange(h * w, dtype=np.int64), w)
    tiles_across = -(-w // MT_COLS)
    return (y // MT_ROWS) * tiles_across + x // MT_COLS, (y % MT_ROWS) * MT_COLS + x % MT_COLS


def frag16_map(h, w, C):
    """[h*w, C] byte offset of the HI half of every element; its LO half lies one KiB further.
    Header: per (m-tile, 16-channel group) 1 KiB of hi halves | 1 KiB of lo halves; inside a plane the 16-byte piece (kg, li) holds
    channels 8kg .. 8kg+7."""
    assert C % 16 == 0
    mt, li = _tile_lane(h, w)
    c = np.arange(C, dtype=np.int64)
    group, within = c // 16, c % 16
    kg, e = within // 8, within % 8
    block = (mt[:, None] * (C // 16) + group[None, :]) * (2 * KIB)               # hi plane | lo plane
    piece = kg[None, :] * MT_PIXELS + li[:, None]                                # 64 pieces of 16 bytes per plane
    return block + piece * 16 + e[None, :] * 2


def acc32_map(h, w, C):
    """[h*w, C] byte offset of every fp32 element.
    Header: per (m-tile, 32-channel tile, j < 4) 1 KiB, lane (kg, li) holds channels 8j + 4kg + 0..3."""
    assert C % 32 == 0
    mt, li = _tile_lane(h, w)
    c = np.arange(C, dtype=np.int64)
    tile, within = c // 32, c % 32
    j, kg, e = within // 8, (within % 8) // 4, within % 4
    block = ((mt[:, None] * (C // 32) + tile[None, :]) * 4 + j[None, :]) * KIB
    lane = kg[None, :] * MT_PIXELS + li[:, None]
    return block + lane * 16 + e[None, :] * 4


def f32x8_map(h, w, C):
    """[h*w, C] byte offset of every fp32 element.
    Header: per (m-tile, 16-channel group, q < 2) 1 KiB, lane (kg, li) holds channels 8kg + 4q + 0..3."""
    assert C % 16 == 0
    mt, li = _tile_lane(h, w)
    c = np.arange(C, dtype=np.int64)
    group, within = c // 16, c % 16
    kg, q, e = within // 8, (within % 8) // 4, within % 4
    block = ((mt[:, None] * (C // 16) + group[None, :]) * 2 + q[None, :]) * KIB
    lane = kg[None, :] * MT_PIXELS + li[:, None]
    return block + lane * 16 + e[None, :] * 4


def layout_ranges(layout, h, w, C):
    """The byte ranges of a layout as (starts [h*w, C, k], width): frag16 has two 2-byte ranges per element, the others one of 4."""
    if layout == FRAG16:
        m = frag16_map(h, w, C)
        return np.stack([m, m + KIB], -1), 2
    m = acc32_map(h, w, C) if layout == ACC32 else f32x8_map(h, w, C)
    return m[..., None], 4


def covered_bytes(layout, h, w, C):
    """Bool per byte of the [s16_pixels, C] tensor: written by the layout (the rest are the padding pixels)."""
    starts, width = layout_ranges(layout, h, w, C)
    mask = np.zeros(s16_pixels(h, w) * C * 4, bool)
    for k in range(width):
        mask[starts.reshape(-1) + k] = True
    return mask


def _scatter(starts, values, nbytes):
    """values (any 2- or 4-byte dtype, shape of starts) -> uint8 [nbytes], zero elsewhere."""
    out = np.zeros(nbytes, np.uint8)
    v = np.ascontiguousarray(values).view(np.uint8).reshape(-1, values.dtype.itemsize)
    for k in range(values.dtype.itemsize):
        out[starts.reshape(-1) + k] = v[:, k]
    return out


def frag16_bytes(x, h, w, C, scale):
    """Plain fp32 [h*w, C] -> the whole frag16 tensor [s16_pixels(h, w), C] as bytes, padding pixels zero."""
    x = np.asarray(x, np.float32).reshape(h * w, C)
    hi, lo = split_f16(x, scale)
    m = frag16_map(h, w, C)
    n = s16_pixels(h, w) * C * 4
    return _scatter(m, hi, n) | _scatter(m + KIB, lo, n)


def acc32_bytes(x, h, w, C):
    x = np.asarray(x, np.float32).reshape(h * w, C)
    return _scatter(acc32_map(h, w, C), x, s16_pixels(h, w) * C * 4)


def f32x8_bytes(x, h, w, C):
    x = np.asarray(x, np.float32).reshape(h * w, C)
    return _scatter(f32x8_map(h, w, C), x, s16_pixels(h, w) * C * 4)


def _gather(tensor_bytes, starts, dtype):
    width = np.dtype(dtype).itemsize
    idx = starts.reshape(-1, 1) + np.arange(width)
    return np.ascontiguousarray(np.asarray(tensor_bytes, np.uint8)[idx]).view(dtype).reshape(starts.shape)


def frag16_halves(tensor_bytes, h, w, C):
    """(hi, lo) float16 [h*w, C] read back out of a frag16 tensor."""
    m = frag16_map(h, w, C)
    return _gather(tensor_bytes, m, np.float16), _gather(tensor_bytes, m + KIB, np.float16)


def from_frag16(tensor_bytes, h, w, C, inv):
    hi, lo = frag16_halves(tensor_bytes, h, w, C)
    return join_frag16(hi, lo, inv)


def from_acc32(tensor_bytes, h, w, C):
    return _gather(tensor_bytes, acc32_map(h, w, C), np.float32)


def from_f32x8(tensor_bytes, h, w, C):
    return _gather(tensor_bytes, f32x8_map(h, w, C), np.float32)


# ---- the second form: walk the storage in its own order and ask which element lives there (plain loops; small cases only)
def _pixel_of(tile, li, h, w):
    """(pixel index or None) of lane-order position li of m-tile `tile`."""
    tiles_across = -(-w // MT_COLS)
    ty, tx = divmod(tile, tiles_across)
    y, x = ty * MT_ROWS + li // MT_COLS, tx * MT_COLS + li % MT_COLS
    return y * w + x if (y < h and x < w) else None


def frag16_bytes_scalar(x, h, w, C, scale):
    x = np.asarray(x, np.float32).reshape(h * w, C)
    hi, lo = split_f16(x, scale)
    out = np.zeros(s16_pixels(h, w) * C * 2, np.float16)       # the tensor as a sequence of halves
    pos = 0
    for tile in range(s16_pixels(h, w) // MT_PIXELS):
        for group in range(C // 16):
            for plane in (hi, lo):                             # 1 KiB of hi halves, then 1 KiB of lo halves
                for kg in range(2):
                    for li in range(MT_PIXELS):
                        p = _pixel_of(tile, li, h, w)
                        for e in range(8):                     # the piece holds channels 8kg .. 8kg+7 of the group
                            if p is not None:
                                out[pos] = plane[p, 16 * group + 8 * kg + e]
                            pos += 1
    return out.view(np.uint8)


def acc32_bytes_scalar(x, h, w, C):
    x = np.asarray(x, np.float32).reshape(h * w, C)
    out = np.zeros(s16_pixels(h, w) * C, np.float32)
    pos = 0
    for tile in range(s16_pixels(h, w) // MT_PIXELS):
        for ctile in range(C // 32):
            for j in range(4):
                for kg in range(2):
                    for li in range(MT_PIXELS):
                        p = _pixel_of(tile, li, h, w)
                        for e in range(4):                     # lane (kg, li) holds channels 8j + 4kg + 0..3 of the tile
                            if p is not None:
                                out[pos] = x[p, 32 * ctile + 8 * j + 4 * kg + e]
                            pos += 1
    return out.view(np.uint8)


def f32x8_bytes_scalar(x, h, w, C):
    x = np.asarray(x, np.float32).reshape(h * w, C)
    out = np.zeros(s16_pixels(h, w) * C, np.float32)
    pos = 0
    for tile in range(s16_pixels(h, w) // MT_PIXELS):
        for group in range(C // 16):
            for q in range(2):
                for kg in range(2):
                    for li in range(MT_PIXELS):
                        p = _pixel_of(tile, li, h, w)
                        for e in range(4):                     # lane (kg, li) holds channels 8kg + 4q + 0..3 of the group
                            if p is not None:
                                out[pos] = x[p, 16 * group + 8 * kg + 4 * q + e]
                            pos += 1
    return out.view(np.uint8)


# ------------------------------------------------------------------------------------------------ layout 3: the row mover
def _row_pieces(h, w, C, y0, n):
    """Byte offsets in the frag16 tensor of the hi pieces of image rows [y0, y0 + n): [n*w, C/8] (the lo piece lies one KiB further)."""
    m = frag16_map(h, w, C)
    return m[y0 * w:(y0 + n) * w, ::8]


def rows_plain_bytes(tensor_bytes, h, w, C, y0, n):
    """The plain side of the row mover for image rows [y0, y0 + n) of a frag16 tensor: per pixel and 8 channels, the 16 bytes of the hi
    piece, then the 16 bytes of the lo piece."""
    t = np.asarray(tensor_bytes, np.uint8)
    pieces = _row_pieces(h, w, C, y0, n)
    span = np.arange(16)
    out = np.empty((n * w, C // 8, 2, 16), np.uint8)
    out[:, :, 0] = t[pieces[..., None] + span]
    out[:, :, 1] = t[pieces[..., None] + KIB + span]
    return out.reshape(-1)


def rows_into_tensor_bytes(tensor_bytes, rows_bytes, h, w, C, y0, n):
    """The other direction: a copy of the tensor in which the pieces of rows [y0, y0 + n) are those of ``rows_bytes``."""
    t = np.array(tensor_bytes, np.uint8)
    r = np.asarray(rows_bytes, np.uint8).reshape(n * w, C // 8, 2, 16)
    pieces = _row_pieces(h, w, C, y0, n)
    span = np.arange(16)
    t[pieces[..., None] + span] = r[:, :, 0]
    t[pieces[..., None] + KIB + span] = r[:, :, 1]
    return t


# ------------------------------------------------------------------------------------------------ split32
def split32_map(P, C):
    """[P, C] byte offset of the hi half; the lo half lies 64 bytes further.  Header: per pixel and 32-channel chunk, 32 hi halves
    followed by 32 lo halves, in the bytes of the chunk's 32 fp32 slots."""
    assert C % 32 == 0
    p = np.arange(P, dtype=np.int64)[:, None]
    c = np.arange(C, dtype=np.int64)[None, :]
    return (p * C + c // 32 * 32) * 4 + c % 32 * 2


def split32_bytes(x):
    x = np.asarray(x, np.float32)
    P, C = x.shape
    hi, lo = split32_f16(x)
    m = split32_map(P, C)
    return _scatter(m, hi, P * C * 4) | _scatter(m + 64, lo, P * C * 4)


def split32_bytes_scalar(x):
    x = np.asarray(x, np.float32)
    P, C = x.shape
    hi, lo = split32_f16(x)
    out = np.zeros(P * C * 2, np.float16)
    pos = 0
    for p in range(P):
        for chunk in range(C // 32):
            for plane in (hi, lo):
                for e in range(32):
                    out[pos] = plane[p, 32 * chunk + e]
                    pos += 1
    return out.view(np.uint8)


def from_split32(tensor_bytes, P, C):
    m = split32_map(P, C)
    return join_split32(_gather(tensor_bytes, m, np.float16), _gather(tensor_bytes, m + 64, np.float16))


# ------------------------------------------------------------------------------------------------ feature planes
FEAT_SCALE = 64.0                                # 2^6: features saturate beyond +-1023


def feat_split_planes(x, blocks, bt):
    """fp32 [blocks, bt, 64] -> float16 [blocks, 8, bt, 16]: plane p = hl * 4 + ks (hl: hi / lo of x * 2^6 - NO 2^11 on lo; ks: 16-channel
    group)."""
    x = np.asarray(x, np.float32).reshape(blocks, bt, 64)
    hi, lo = split_f16(x, FEAT_SCALE)
    out = np.empty((blocks, 8, bt, 16), np.float16)
    for hl, half in enumerate((hi, lo)):
        for ks in range(4):
            out[:, hl * 4 + ks] = half[:, :, 16 * ks:16 * ks + 16]
    return out


def feat_split_bytes(x, blocks, bt):
    return feat_split_planes(x, blocks, bt).reshape(-1).view(np.uint8)


def feat_saturates(x):
    """Per element: the split clamps it (|x * 2^6| > 65504) or it is not finite - what raises overflow bit 1."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(x, np.float32) * np.float32(FEAT_SCALE)
    return ~(np.abs(t) <= F16_MAX)


def feat_ref_rows_bytes(slot, h, w, border):
    """One bordered block of operand planes, int16 [8, (h+2b)*(w+2b), 16] -> the bytes of its interior [8, h*w, 16]."""
    hb, wb = h + 2 * border, w + 2 * border
    s = np.asarray(slot, np.int16).reshape(8, hb, wb, 16)
    return np.ascontiguousarray(s[:, border:border + h, border:border + w]).reshape(-1).view(np.uint8)


# ------------------------------------------------------------------------------------------------ pyramid
def pyramid_need(D, L):
    need, n = 0, D
    for _ in range(L):
        need += n
        n //= 2
    return need


def pyramid_rows(vol, D, stride, L, scale):
    """Rows [level0 (D) | level1 (D // 2) | ...]: level0 *= scale where scale != 1, then every level = (a + b) * 0.5 of the previous,
    in float32.  Returns float32 [rows, need]; columns [need, stride) are not the pyramid's."""
    v = np.asarray(vol, np.float32).reshape(-1, stride)
    need = pyramid_need(D, L)
    assert stride >= need
    out = np.empty((v.shape[0], need), np.float32)
    level = v[:, :D].copy()
    if np.float32(scale) != np.float32(1.0):
        level = level * np.float32(scale)
    off = 0
    for l in range(L):
        n = level.shape[1]
        out[:, off:off + n] = level
        off += n
        m = n // 2
        level = (level[:, 0:2 * m:2] + level[:, 1:2 * m:2]) * np.float32(0.5)
    return out


# ------------------------------------------------------------------------------------------------ instance-norm glue
def plane_stats64(x, eps):
    """x [planes, plane] -> (mean, var, E[x^2]) in float64, two passes, biased variance; eps as the kernel receives it (a float32)."""
    x = np.asarray(x, np.float64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    ex2 = (x * x).mean(1)
    return mean, var, ex2, np.float64(np.float32(eps))


def norm_act64(x, xs, res, rs, flags):
    """out = relu4( relu1(norm(x)) + relu2(norm_r(res)) ) in float64 from the GIVEN fp32 statistics [planes, 2] = (mean, rstd).
    Returns (out, t, u): t, u the two branches as they enter the sum (u = 0 without a residual)."""
    x = np.asarray(x, np.float64)
    t = x if xs is None else (x - np.asarray(xs, np.float64)[:, 0:1]) * np.asarray(xs, np.float64)[:, 1:2]
    if flags & 1:
        t = np.maximum(t, 0.0)
    u = np.zeros_like(t)
    if res is not None:
        r = np.asarray(res, np.float64)
        u = r if rs is None else (r - np.asarray(rs, np.float64)[:, 0:1]) * np.asarray(rs, np.float64)[:, 1:2]
        if flags & 2:
            u = np.maximum(u, 0.0)
    out = t + u
    if flags & 4:
        out = np.maximum(out, 0.0)
    return out, t, u


# ------------------------------------------------------------------------------------------------ inputs
def value_classes(scale):
    """The values a split must get right for operand scale ``scale`` (a power of two): signed zeros, a value far below the f16 quantum, values
    whose lo half is an f16 subnormal, the clamp boundary itself and a value far beyond it."""
    s = np.float32(scale)
    v = [0.0, -0.0, 2.0 ** -30, -2.0 ** -30,
         (1.0 + 2.0 ** -20) / s, -(1.0 + 2.0 ** -18) / s, (3.0 + 2.0 ** -16) / s,          # hi normal, lo subnormal
         2.0 ** -15 / s, 2.0 ** -24 / s, 1.5 * 2.0 ** -24 / s,                              # hi itself subnormal; a tie at the smallest subnormal
         65504.0 / s, -65504.0 / s, 65503.99 / s, 1e9, -1e9, 1.0 / s, 1000.3 / s]
    return np.asarray(v, np.float32)
