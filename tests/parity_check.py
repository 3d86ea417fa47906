"""Element-wise parity checking at production shapes: helpers shared by tests/test_parity_check_cpu.py (which proves on planted
corruptions that the checker sees what a global mean cannot) and tests/test_fullsize_parity_gpu.py (which applies it to the HIP
kernels of one GRU iteration - through tests/s16_iteration_check.py, which tests/test_s16_ragged_parity_gpu.py runs at ragged sizes with
forced tile heights - and to the cost volume) and tests/test_encoder_parity_gpu.py (the encoder kernels, one launch at a time: the
float64 pieces and tile geometries further down), by tests/test_train_parity_{cpu,gpu}.py (the training-row kernels) and by
tests/test_postproc_parity_{cpu,gpu}.py (the last section: geometric consistency as a float64 chain that carries, next to every value, a
bound on what a correct fp32 evaluation may deviate by - ``geo_ref64`` / ``check_geo`` / ``GeoReport``: every element is inside its
bound, decided equal or provably undecidable; the image preparation from torch's fp32 taps - ``prep_ref64`` / ``check_prep``; the bit
comparison of the multires kernels - ``bits_equal``), and by tests/test_wide_parity_{cpu,gpu}.py (the wide-range loop: the float64 pieces
of one GRU iteration, which tests/test_fullsize_parity_gpu.py shares, the ``wide_*`` references and bounds, the split32 layout in numpy).
The last section - the cost volume from restated fp32 coordinates (``fma32``, ``cost_coords32``, ``cost_samples_ref64``, ``cost_rows_ref64``,
``cost_bound``) - serves tests/test_cost_geometry_{cpu,gpu}.py.  ``loop_ref64`` chains the update-loop pieces into T whole iterations
(hidden state and disparity after each): the float64 anchor of tests/test_update_run_gpu.py, which holds the three execution protocols
of ``UpdateBlock.run`` to identical bits; tests/test_update_run_cpu.py checks it against the oracle evaluated in float64.
Plain module, no fixtures.

Conventions: an image tensor is pixel-major, ``[h*w, C]`` or ``[h*w]``; a *tile* is a (rows, columns) block of pixels - 8 x 16 by
default, the smallest tile the s16 convolutions launch (16 x 16 for the tall ones); a *seam* is the border between two 32-pixel
segments of the epipolar-line kernel (csrc/cost_lines.hip: tiles of 32 pixels along the tile axis of a view)."""
import math

import torch
import torch.nn.functional as F

F16_NAN_BITS = 0x7E00        # a quiet f16 NaN: what the sentinel puts into every half of a frag16 / split32 plane


class ParityReport:
    """What ``check_elementwise`` found.  ``n_fail`` failing elements of ``n`` (a non-finite value fails), ``max_ratio`` = max |err| /
    bound, ``p999_ratio`` its 99.9th percentile, ``max_rel`` = max |err| / mag (the figure the profiles record); the failing elements by
    pixel (``pixels``: ids in the h x w image), by tile (``tiles``: {(tile_y, tile_x): count}), by image row and column (``rows``,
    ``cols``: {index: count}), and how many sit on the image rim, in a partial last tile, on a segment seam."""

    def __init__(self, where, h, w, tile, n, n_fail, max_ratio, p999_ratio, max_rel, worst, pixels, channels, seam):
        self.where, self.h, self.w, self.tile = where, h, w, tile
        self.n, self.n_fail, self.max_ratio, self.p999_ratio, self.max_rel, self.worst = n, n_fail, max_ratio, p999_ratio, max_rel, worst
        self.pixels, self.channels = pixels, channels
        ys, xs = pixels // w, pixels % w
        th, tw = tile
        count = lambda t: {tuple(k) if isinstance(k, list) else k: int(c) for k, c in zip(*[x.tolist() for x in torch.unique(t, dim=0, return_counts=True)])}
        self.tiles = count(torch.stack([ys // th, xs // tw], 1)) if n_fail else {}
        self.rows = count(ys) if n_fail else {}
        self.cols = count(xs) if n_fail else {}
        self.on_rim = int(rim_mask(h, w).reshape(-1)[pixels].sum()) if n_fail else 0
        self.in_partial_tile = int(partial_tile_mask(h, w, tile).reshape(-1)[pixels].sum()) if n_fail else 0
        self.on_seam = int(seam_mask(h, w, seam).reshape(-1)[pixels].sum()) if (n_fail and seam) else 0

    @property
    def ok(self):
        return self.n_fail == 0

    def only_tile(self):
        """(tile_y, tile_x) if every failing element lies in one tile, else None."""
        return next(iter(self.tiles)) if len(self.tiles) == 1 else None

    def only_row(self):
        return next(iter(self.rows)) if len(self.rows) == 1 else None

    def message(self):
        if self.ok:
            return f"{self.where}: all {self.n} elements within bound (max ratio {self.max_ratio:.3g})"
        top = lambda d, k=6: ", ".join(f"{key}: {c}" for key, c in sorted(d.items(), key=lambda kv: -kv[1])[:k]) + (" ..." if len(d) > k else "")
        y, x, c = self.worst
        th, tw = self.tile
        lines = [f"{self.where}: {self.n_fail} of {self.n} elements beyond their bound in a {self.h} x {self.w} image; worst |err| / bound = "
                 f"{self.max_ratio:.4g} at row {y}, column {x}, channel {c} ({th} x {tw} tile ({y // th}, {x // tw}))",
                 f"  {th} x {tw} tiles (tile_y, tile_x): failing elements - {len(self.tiles)} tile(s): {top(self.tiles)}",
                 f"  image rows - {len(self.rows)}: {top(self.rows)};  columns - {len(self.cols)}: {top(self.cols)}",
                 f"  channels - {top(self.channels)}",
                 f"  of the failing elements {self.on_rim} lie on the image rim, {self.in_partial_tile} in a partial last tile, "
                 f"{self.on_seam} on a segment seam"]
        if self.only_tile() is not None:
            lines.append(f"  => confined to tile {self.only_tile()}")
        if self.only_row() is not None:
            lines.append(f"  => confined to image row {self.only_row()}" + (" (the last row)" if self.only_row() == self.h - 1 else ""))
        return "\n".join(lines)


def rim_mask(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def partial_tile_mask(h, w, tile=(8, 16)):
    """Pixels of tiles that reach beyond the image (the last tile row / column when h / w is no multiple of the tile)."""
    th, tw = tile
    m = torch.zeros(h, w, dtype=torch.bool)
    if h % th:
        m[h // th * th:] = True
    if w % tw:
        m[:, w // tw * tw:] = True
    return m


def seam_mask(h, w, period=32):
    """Pixels on either side of a segment border, along both image axes (a view's tile axis is x or y)."""
    m = torch.zeros(h, w, dtype=torch.bool)
    if not period:
        return m
    y, x = torch.arange(h), torch.arange(w)
    sy = ((y % period == 0) & (y > 0)) | ((y % period == period - 1) & (y < h - 1))
    sx = ((x % period == 0) & (x > 0)) | ((x % period == period - 1) & (x < w - 1))
    m |= sy[:, None]
    m |= sx[None, :]
    return m


def check_elementwise(got, ref64, mag, c, abs_term=0.0, where="", h=None, w=None, tile=(8, 16), seam=None, pixels=None):
    """|got - ref64| <= c * mag + abs_term for every element -> ParityReport.  ``got``, ``ref64``, ``mag``: ``[N, C]`` or ``[N]``
    (``abs_term``: a number or a tensor that broadcasts); row i is pixel ``pixels[i]`` of the h x w image (default: N = h * w,
    all pixels in order)."""
    got = torch.as_tensor(got).detach().cpu().double()
    ref64 = torch.as_tensor(ref64).detach().cpu().double()
    if got.shape != ref64.shape:
        raise ValueError(f"{where}: shapes differ: {tuple(got.shape)} vs {tuple(ref64.shape)}")
    if got.dim() == 1:
        got, ref64 = got[:, None], ref64[:, None]
    mag = torch.as_tensor(mag, dtype=torch.float64)
    mag = mag[:, None] if mag.dim() == 1 else mag
    abs_term = torch.as_tensor(abs_term, dtype=torch.float64)
    abs_term = abs_term[:, None] if abs_term.dim() == 1 else abs_term
    N, C = got.shape
    pixels = torch.arange(N) if pixels is None else torch.as_tensor(pixels, dtype=torch.long)
    if pixels.numel() != N or (N and int(pixels.max()) >= h * w):
        raise ValueError(f"{where}: {N} rows do not match the pixel list of a {h} x {w} image")
    bound = (c * mag + abs_term).expand(N, C)
    err = (got - ref64).abs()
    ratio = err / bound.clamp_min(1e-300)
    bad = ~(err <= bound)                                  # (a NaN compares false: it fails)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    rel = err / mag.expand(N, C).clamp_min(1e-300)
    rel = torch.where(torch.isnan(rel), torch.full_like(rel, math.inf), rel)
    n_fail = int(bad.sum())
    flat = ratio.reshape(-1)
    k = max(1, int(math.ceil(0.999 * flat.numel())))
    p999 = float(torch.kthvalue(flat, k).values) if flat.numel() else 0.0
    wi = int(torch.argmax(flat)) if flat.numel() else 0
    wp = int(pixels[wi // C]) if N else 0
    idx = bad.nonzero()
    chans = {int(k_): int(c_) for k_, c_ in zip(*[x.tolist() for x in torch.unique(idx[:, 1], return_counts=True)])} if n_fail else {}
    return ParityReport(where, h, w, tile, N * C, n_fail, float(flat.max()) if flat.numel() else 0.0, p999, float(rel.max()) if N else 0.0,
                        (wp // w, wp % w, wi % C), pixels[idx[:, 0]], chans, seam)


def assert_elementwise(got, ref64, mag, c, abs_term=0.0, where="", **kw):
    """``check_elementwise`` that raises an AssertionError naming the failing tiles / rows; returns the report otherwise."""
    rep = check_elementwise(got, ref64, mag, c, abs_term, where, **kw)
    assert rep.ok, rep.message()
    return rep


# ------------------------------------------------------------------------------------------------ sentinel coverage
def poison_f32(t):
    """Fill an fp32-layout output buffer (acc32, f32x8, plain planes) with NaN before the launch under test."""
    t.fill_(float("nan"))
    return t


def poison_f16(t):
    """Fill a frag16 / split32 buffer (fp32 slots holding f16 halves) with the f16 NaN pattern in every half."""
    t.view(torch.int16).fill_(F16_NAN_BITS)
    return t


def assert_covered(plain, where, h, w, tile=(8, 16), seam=None, pixels=None):
    """After the launch: every data pixel of the output (read back to the plain layout) must hold a number - a NaN is a sentinel that
    no block overwrote (a skipped tile) or a sentinel that a kernel consumed from a padding slot.  No tolerance involved."""
    plain = torch.as_tensor(plain).detach().cpu().double()
    ones = torch.ones_like(plain)
    finite = torch.where(torch.isfinite(plain), torch.zeros_like(plain), torch.full_like(plain, float("nan")))
    rep = check_elementwise(finite, torch.zeros_like(plain), ones, 1.0, 0.0, where + " [sentinel coverage]", h=h, w=w, tile=tile, seam=seam, pixels=pixels)
    assert rep.ok, rep.message()
    return rep


# ------------------------------------------------------------------------------------------------ cost volume in float64
def cost_volume_ref64(fmaps, Pij, D, incre, disp_in, shift, pixels=None, chunk=2048):
    """Float64 restatement of oracle.cer_oracle.cost_volume (core/corr.py:46-91, utils/projective_ops.py:5-28, correlation_kernel.cu:59-116)
    on a subset of pixels: hypotheses d_k = fl32((k - D//2) * incre) + origin, x1 = Pij (x, y, 1, d), (x1 / x1_z)[:2] clamped to +-1e4,
    bilinear sample of the source map with zeros outside, 64-channel dot of the two maps (each / 8).
    fmaps [V+1,C,h,w]; Pij [V,4,4] (taken as given, in float64); disp_in [h,w]; pixels: ids (default all).
    -> (vol [V,N,D], norm [V,N,D], origin [N]) with norm = sum_c |f1_c| * (bilinear-weighted |f2_c|), the scale of a sample's rounding errors."""
    N1, C, h, w = fmaps.shape
    V = N1 - 1
    fm = fmaps.double() / 8.0
    pixels = torch.arange(h * w) if pixels is None else torch.as_tensor(pixels, dtype=torch.long)
    disp = disp_in.reshape(-1)[pixels].double()
    if shift:
        lim = float(torch.tensor((D // 2) * incre, dtype=torch.float32))
        origin = torch.where(disp < (D // 2) * incre, torch.full_like(disp, lim), disp)
    else:
        origin = disp.clone()
    steps = ((torch.arange(D) - D // 2) * incre).to(torch.float32).double()
    f1_all = fm[0].permute(1, 2, 0).reshape(h * w, C)
    px, py = (pixels % w).double(), (pixels // w).double()
    Pij = Pij.double()
    vol = torch.empty(V, pixels.numel(), D, dtype=torch.float64)
    norm = torch.empty_like(vol)
    for v in range(V):
        f2 = torch.cat([fm[v + 1].permute(1, 2, 0).reshape(h * w, C), torch.zeros(1, C, dtype=torch.float64)], 0)      # (row h*w: the zero texel)
        f2a = f2.abs()
        m = Pij[v]
        for s in range(0, pixels.numel(), chunk):
            e = slice(s, s + chunk)
            hyp = steps[None, :] + origin[e, None]                                                  # [n, D]
            x, y = px[e, None], py[e, None]
            X = m[0, 0] * x + m[0, 1] * y + m[0, 2] + m[0, 3] * hyp
            Y = m[1, 0] * x + m[1, 1] * y + m[1, 2] + m[1, 3] * hyp
            Z = m[2, 0] * x + m[2, 1] * y + m[2, 2] + m[2, 3] * hyp
            u, t = X / Z, Y / Z
            nan = torch.isnan(u) | torch.isnan(t)
            u = torch.where(nan, torch.full_like(u, -1e4), u).clamp(-1e4, 1e4)
            t = torch.where(nan, torch.full_like(t, -1e4), t).clamp(-1e4, 1e4)
            x0, y0 = torch.floor(u), torch.floor(t)
            fx, fy = u - x0, t - y0
            f1 = f1_all[pixels[e]]
            f1a = f1.abs()
            acc = torch.zeros_like(u)
            accn = torch.zeros_like(u)
            for dy, dx, wt in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
                xi, yi = (x0 + dx).long(), (y0 + dy).long()
                ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                idx = torch.where(ok, yi * w + xi, torch.full_like(xi, h * w))
                acc += wt * torch.einsum("ndc,nc->nd", f2[idx], f1)
                accn += wt * torch.einsum("ndc,nc->nd", f2a[idx], f1a)
            vol[v, e], norm[v, e] = acc, accn
    return vol, norm, origin


def cost_subset(h, w, period=32, tile=(8, 16), interior_fraction=0.05, seed=1):
    """The pixels on which the full-size cost volume is compared: the whole rim, the first and last tile row and column, both sides of
    every segment seam (along x and y: a view's tile axis is either), and a fixed pseudo-random ``interior_fraction`` of the rest.
    -> (sorted pixel ids, the mask of the pixels that MUST be in it)."""
    from cer_mvs_amd.synthetic import hash_uniform
    th, tw = tile
    must = rim_mask(h, w) | seam_mask(h, w, period)
    must[:th], must[-th:], must[:, :tw], must[:, -tw:] = True, True, True, True
    pick = torch.from_numpy(hash_uniform(h * w, seed) * 0.5 + 0.5).reshape(h, w) < interior_fraction
    return (must | pick).reshape(-1).nonzero().reshape(-1), must


# ------------------------------------------------------------------------------------------------ encoder launches in float64
# Tile geometries of the encoder kernels (rows, columns) - the ``tile=`` argument of the checks above: 8 x 32 everywhere except the
# stride-2 3 x 3 convolution (2 x 32; the tiled engine's stride-2 1 x 1 too) and the 128-channel context head of csrc/enc_pc.hip (4 x 32).
ENC_TILE = (8, 32)
ENC_TILE_S2 = (2, 32)
ENC_TILE_CTX = (4, 32)
U24 = 2.0 ** -24             # unit roundoff of fp32


def enc_pc_tile(cout, taps, stride):
    """Tile of cer_enc_pc_conv (csrc/enc_pc.hip: PcCfg::TH, pc_tile_rows)."""
    return ENC_TILE_S2 if (taps == 9 and stride == 2) else (ENC_TILE_CTX if cout >= 128 else ENC_TILE)


def enc_conv_tile(stride):
    """Tile of cer_enc_conv_f16x3 (csrc/enc_conv.hip: cer_enc_conv_tiles)."""
    return ENC_TILE_S2 if stride == 2 else ENC_TILE


def _enc_term64(X, s, relu):
    x = X.detach().cpu().double()
    N, C = x.shape[0], x.shape[-1]
    if s is not None:
        st = s.detach().cpu().double().view(N, *([1] * (x.dim() - 2)), C, 2)
        mean, rstd = st[..., 0], st[..., 1]
        y, mag = (x - mean) * rstd, (x.abs() + mean.abs()) * rstd
    else:
        y, mag = x, x.abs()
    return (torch.relu(y) if relu else y), mag


def enc_input_ref64(A, sA, rA, B=None, sB=None, rB=False, relu_sum=False):
    """The virtual input of an encoder convolution, relu_s(fa(A) + fb(B)) with f = the optional (x - mean) * rstd of the very stats
    tensor the kernel is given ([N * C, 2] = (mean, rstd)) followed by the optional ReLU; A, B: [N, ..., C] channels-last.
    -> (x64, mag_in) with mag_in = (|A| + |mean_A|) * rstd_A [+ the same of B]: the scale of the fp32 roundings in forming x."""
    y, mag = _enc_term64(A, sA, rA)
    if B is not None:
        yb, mb = _enc_term64(B, sB, rB)
        y, mag = y + yb, mag + mb
    return (torch.relu(y) if relu_sum else y), mag


def enc_conv_ref64(x64, w, b, taps, stride, mag_in=None):
    """x64 [N, h, w, Cin] channels-last float64, w [Cout, Cin, k, k], b [Cout] or None -> (conv, mag, mag_form), each
    [N, ho, wo, Cout] float64: the F.conv2d result (3 x 3 with padding 1, or 1 x 1), mag = conv(|x64|, |w|) + |b|, and mag_form =
    conv(mag_in, |w|) (None without ``mag_in``)."""
    import torch.nn.functional as F
    pad = 1 if taps == 9 else 0
    w64 = w.detach().cpu().double()
    assert w64.shape[2] * w64.shape[3] == taps
    b64 = None if b is None else b.detach().cpu().double()
    xc = x64.permute(0, 3, 1, 2)
    N = xc.shape[0]
    ref = F.conv2d(xc, w64, b64, stride=stride, padding=pad).permute(0, 2, 3, 1)
    mags = [xc.abs()] + ([mag_in.permute(0, 3, 1, 2)] if mag_in is not None else [])
    m = F.conv2d(torch.cat(mags, 0), w64.abs(), None, stride=stride, padding=pad).permute(0, 2, 3, 1)
    mag = m[:N] + (0.0 if b64 is None else b64.abs())
    return ref, mag, (m[N:] if mag_in is not None else None)


def enc_head_ref64(conv, epi, scale=1.0, border=0, fill=None):
    """Head epilogues of the encoder kernels in float64.  "fmap": ``scale * conv`` into a map with ``border`` texels on every side
    ([N, ho + 2b, wo + 2b, C]; the border keeps ``fill``, a tensor of that shape, or zeros); "ctx": (tanh of the first half of the
    channels, relu of the second half)."""
    if epi == "ctx":
        half = conv.shape[-1] // 2
        return torch.tanh(conv[..., :half]), torch.relu(conv[..., half:])
    assert epi == "fmap"
    N, ho, wo, C = conv.shape
    out = torch.zeros(N, ho + 2 * border, wo + 2 * border, C, dtype=torch.float64) if fill is None else fill.detach().cpu().double().clone()
    out[:, border:border + ho, border:border + wo] = scale * conv
    return out


def instance_stats64(y, eps=1e-5):
    """[N, ..., C] float64 -> [N * C, 2] float64 (mean, rstd) of InstanceNorm2d (biased variance, eps 1e-5)."""
    N, C = y.shape[0], y.shape[-1]
    f = y.reshape(N, -1, C)
    mean = f.mean(1)
    var = ((f - mean[:, None]) ** 2).mean(1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], -1).reshape(N * C, 2)


def check_batch(got, ref64, mag, c, abs_term=0.0, where="", h=None, w=None, tile=ENC_TILE):
    """``check_elementwise`` over a batch [N, h, w, C] (or [N, h * w, C]): every element of every image against c * mag + abs_term.
    Raises an AssertionError that names the first failing image and, inside it, the tile / row (``ParityReport.message``); otherwise
    -> {"max_ratio", "p999_ratio", "max_rel", "p999_rel"}: |err| / bound and |err| / mag over the whole batch."""
    got = torch.as_tensor(got).detach().cpu().double()
    N, C = got.shape[0], got.shape[-1]
    got = got.reshape(N, h * w, C)
    ref64 = ref64.reshape(N, h * w, C)
    mag = torch.as_tensor(mag, dtype=torch.float64).expand(N, *mag.shape[1:]).reshape(N, h * w, C)
    abs_term = torch.as_tensor(abs_term, dtype=torch.float64)
    abs_term = abs_term.reshape(N, h * w, C) if abs_term.dim() >= 3 else abs_term
    bound = c * mag + abs_term
    err = (got - ref64).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        n = int(bad.reshape(N, -1).any(1).nonzero()[0])
        rep = check_elementwise(got[n], ref64[n], mag[n], c, abs_term[n] if abs_term.dim() >= 3 else abs_term, f"{where}, image {n} of {N}",
                                h=h, w=w, tile=tile)
        raise AssertionError(f"{int(bad.reshape(N, -1).any(1).sum())} of {N} images fail; the first:\n" + rep.message())

    def top(t):
        flat = t.reshape(-1)
        k = max(1, int(math.ceil(0.999 * flat.numel())))
        return float(flat.max()), float(torch.kthvalue(flat, k).values)
    mr, pr = top(err / bound.clamp_min(1e-300))
    ml, pl = top(err / mag.clamp_min(1e-300))
    return {"max_ratio": mr, "p999_ratio": pr, "max_rel": ml, "p999_rel": pl}


def assert_covered_batch(out, where, h, w, tile=ENC_TILE):
    """``assert_covered`` over a batch [N, h * w, C] / [N, h, w, C]: no NaN sentinel may be left in any image."""
    out = torch.as_tensor(out).detach().cpu()
    N = out.shape[0]
    flat = out.reshape(N, h * w, -1)
    left = (~torch.isfinite(flat)).reshape(N, -1).any(1)
    if bool(left.any()):
        n = int(left.nonzero()[0])
        assert_covered(flat[n], f"{where}, image {n} of {N}", h, w, tile=tile)


def stats_records_ref64(out, tile):
    """out [N, ho, wo, C] (the kernel's own fp32 output) -> per tile, row-major tile id: (sum, sum of squares, sum of |.|), each
    [N, tiles, C] float64 - what a statistics record of that tile must hold."""
    o = torch.as_tensor(out).detach().cpu().double()
    N, ho, wo, C = o.shape
    th, tw = tile
    ty, tx = (ho + th - 1) // th, (wo + tw - 1) // tw
    p = torch.zeros(N, ty * th, tx * tw, C, dtype=torch.float64)
    p[:, :ho, :wo] = o
    p = p.view(N, ty, th, tx, tw, C)
    red = lambda t: t.sum((2, 4)).reshape(N, ty * tx, C)
    return red(p), red(p * p), red(p.abs())


def check_stats_records(part, out, tile, K, where=""):
    """Statistics partial records ``part`` [N, tiles, C, 2] against the float64 sums of ``out`` [N, ho, wo, C] over each tile's pixels:
    |sum - S| <= K 2^-24 sum|o|, |sumsq - Q| <= K 2^-24 sum o^2, every record finite.  -> (ok, message, max ratio); the message names
    the failing tiles as (image, tile_y, tile_x)."""
    part = torch.as_tensor(part).detach().cpu().double()
    S, Q, SA = stats_records_ref64(out, tile)
    N, nt, C = S.shape
    if tuple(part.shape) != (N, nt, C, 2):
        raise ValueError(f"{where}: records {tuple(part.shape)} for {(N, nt, C, 2)}")
    tiles_x = (out.shape[2] + tile[1] - 1) // tile[1]
    bs, bq = K * U24 * SA, K * U24 * Q
    es, eq = (part[..., 0] - S).abs(), (part[..., 1] - Q).abs()
    bad = ~(es <= bs) | ~(eq <= bq)                       # (a NaN record - the sentinel - compares false: it fails)
    ratio = torch.maximum(es / bs.clamp_min(1e-300), eq / bq.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    mx = float(ratio.max())
    if not bool(bad.any()):
        return True, f"{where}: all {N * nt} statistics records within bound (max ratio {mx:.3g})", mx
    tiles = sorted({(int(n), int(t) // tiles_x, int(t) % tiles_x) for n, t in bad.any(-1).nonzero().tolist()})
    msg = (f"{where}: {len(tiles)} of {N * nt} statistics records ({tile[0]} x {tile[1]} tiles) beyond K = {K} roundings of their tile's "
           f"sums, worst ratio {mx:.4g}; (image, tile_y, tile_x): " + ", ".join(str(t) for t in tiles[:8]) + (" ..." if len(tiles) > 8 else ""))
    return False, msg, mx


def assert_stats_records(part, out, tile, K, where=""):
    ok, msg, mx = check_stats_records(part, out, tile, K, where)
    assert ok, msg
    return mx


def enc_chain_ref64(x, sd, prefix, kind, outputs=None):
    """The whole "HR" encoder (oracle.cer_oracle.encoder) as a chain of ``enc_input_ref64`` and ``enc_conv_ref64`` with float64
    instance-norm statistics - the schedule of cer-mvs_amd/encoder_hip.py: raw convolution outputs plus statistics, the normalisation
    applied by the consumer, the residual merge as a two-tensor virtual input.  x [N, 3, H, W] -> [N, Cout, H/4, W/4] float64.
    ``outputs`` (a dict) receives every trunk convolution's raw output [N, ho, wo, C] by layer name."""
    import torch.nn.functional as F
    inorm = kind == "instance"
    st = lambda y: instance_stats64(y) if inorm else None
    wb = lambda name: (sd[prefix + name + ".weight"], sd[prefix + name + ".bias"])

    def conv(name, xin, taps, stride):
        y = enc_conv_ref64(xin, *wb(name), taps, stride)[0]
        if outputs is not None:
            outputs[name] = y
        return y, st(y)
    w0, b0 = wb("conv1")
    raw0 = F.conv2d(x.double(), w0.double(), b0.double(), stride=2, padding=3).permute(0, 2, 3, 1)
    if outputs is not None:
        outputs["conv1"] = raw0
    cur = (raw0, st(raw0), True, None, None, False)      # (A, sA, rA, B, sB, rB): relu_s only with a B
    for layer, stride in (("layer1.0", 1), ("layer1.1", 1), ("layer2.0", 2), ("layer2.1", 1)):
        A, sA, rA, B, sB, rB = cur
        xin = enc_input_ref64(A, sA, rA, B, sB, rB, relu_sum=B is not None)[0]
        r1, s1 = conv(layer + ".conv1", xin, 9, stride)
        r2, s2 = conv(layer + ".conv2", enc_input_ref64(r1, s1, True)[0], 9, 1)
        if stride == 2:
            rd, sd_ = conv(layer + ".downsample.0", xin, 1, 2)
            cur = (r2, s2, True, rd, sd_, False)
        else:
            cur = (r2, s2, True, xin, None, False)
    A, sA, rA, B, sB, rB = cur
    xin = enc_input_ref64(A, sA, rA, B, sB, rB, relu_sum=True)[0]
    return enc_conv_ref64(xin, *wb("conv2"), 1, 1)[0].permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ training row in float64
# References of the training-row kernels: csrc/alt_corr.hip (alt_cuda_corr/correlation_kernel.cu:18-119 forward, 122-256
# backward), csrc/train_ops.hip (core/corr.py:94-97,102-143 with test_mode=False, utils/bilinear_sampler.py:6-25; loss.py:18-19).  Plain
# torch on the CPU, no autograd.  Each takes the tensors the kernel reads, forms INDICES from the fp32 inputs with the kernel's own fp32
# steps (floorf and x - floorf(x), exact; the lookup's max((disp - origin) / incre + D//2, 0) chain; the upsample's fl32((in-1)/(out-1))
# and fl32(scale * dst)) and does everything else in float64.  ``mag`` = the sum of absolute products behind an output element;
# ``n`` = the number of terms added into it one after the other.  tests/test_train_parity_{cpu,gpu}.py.
K_COEF = 8                   # roundings of one tuple coefficient, see alt_corr_tuples_ref64
K_UP_FWD = 7                 # roundings of the upsample's two-by-two blend, see upsample_ac_ref64
C_CONV = 1e-6                # the project's per-element constant of an fp32 dot (tests/test_fullsize_parity_gpu.py: holds at 1593 terms)


def _corr_floor(coords):
    """coords [..., 2] fp32 -> (finite, floor x, floor y as fp32, fl32(x - floor x), fl32(y - floor y) as float64; 0 where the coordinate
    is not finite) - csrc/alt_corr.hip, the first lines of every sample loop.  The subtraction is an fp32 one, as in the kernel and in
    correlation_kernel.cu: exact for x >= 0 and x <= -1, one rounding for -1 < x < 0 (the fraction has more bits than x)."""
    c = coords.detach().cpu().float()
    x, y = c[..., 0], c[..., 1]
    finite = (x.abs() <= 3.0e38) & (y.abs() <= 3.0e38)                       # (a NaN compares false)
    fx, fy = torch.floor(x), torch.floor(y)
    zero = torch.zeros_like(x)
    dx = torch.where(finite, x - fx, zero).double()
    dy = torch.where(finite, y - fy, zero).double()
    return finite, fx, fy, dx, dy


def alt_corr_ref64(f1, f2, coords, r):
    """alt_corr_fwd_kernel (correlation_kernel.cu:18-119): f1 [B,H1,W1,C], f2 [B,H2,W2,C], coords [B,N,H1,W1,2] -> (corr, mag), each
    [B,N,(2r+1)^2,H1,W1] float64.  Channel ky + rd*kx is the bilinear sample of f2 at (x - r + kx, y - r + ky) dotted with f1; texels
    outside the map are zero; a sample whose coordinate is not finite is 0 (deliberate deviations)."""
    B, H1, W1, C = f1.shape
    _, H2, W2, _ = f2.shape
    N, rd, P1, T = coords.shape[1], 2 * r + 1, H1 * W1, H2 * W2
    finite, fx, fy, dx, dy = (t.reshape(B, N, P1) for t in _corr_floor(coords))
    a = f1.detach().cpu().double().reshape(B, 1, P1, C)
    t = torch.cat([f2.detach().cpu().double().reshape(B, T, C), torch.zeros(B, 1, C, dtype=torch.float64)], 1)       # (row T: the zero texel)
    aa, ta = a.abs(), t.abs()
    bidx = torch.arange(B).view(B, 1, 1)
    corr = torch.zeros(B, N, rd * rd, P1, dtype=torch.float64)
    mag = torch.zeros_like(corr)
    for kx in range(rd):
        for ky in range(rd):
            sx, sy = fx + float(kx - r), fy + float(ky - r)                  # fp32 adds, as cer_bilerp_dot receives them
            near = finite & (sx >= -1.0) & (sx <= float(W2)) & (sy >= -1.0) & (sy <= float(H2))
            ix, iy = torch.where(near, sx, torch.zeros_like(sx)).long(), torch.where(near, sy, torch.zeros_like(sy)).long()
            for oy, ox, wt in ((0, 0, (1 - dy) * (1 - dx)), (0, 1, (1 - dy) * dx), (1, 0, dy * (1 - dx)), (1, 1, dy * dx)):
                xi, yi = ix + ox, iy + oy
                ok = near & (xi >= 0) & (xi < W2) & (yi >= 0) & (yi < H2)
                idx = torch.where(ok, yi * W2 + xi, torch.full_like(xi, T))
                corr[:, :, ky + rd * kx] += wt * (t[bidx, idx] * a).sum(-1)
                mag[:, :, ky + rd * kx] += wt * (ta[bidx, idx] * aa).sum(-1)
    return corr.view(B, N, rd * rd, H1, W1), mag.view(B, N, rd * rd, H1, W1)


def alt_corr_tuples_ref64(coords, g, r, H2, W2):
    """alt_corr_bwd_tuples_kernel: one (key, coefficient, source pixel) per (sample, footprint texel), sample (b, n, p) major, footprint
    (iy, ix) in [0, rd]^2 row-major.  coords [B,N,H1,W1,2], g = corr_grad [B,N,rd^2,H1,W1] -> (keys int64, coef, coef_mag float64, src
    int32), each [S, (rd+1)^2].  Texel (iy0 + iy, ix0 + ix) with (ix0, iy0) = floor - r gathers the up to four outputs whose footprint
    holds it:  g[(iy-1) + rd (ix-1)] dy dx + g[(iy-1) + rd ix] dy (1-dx) + g[iy + rd (ix-1)] (1-dy) dx + g[iy + rd ix] (1-dy)(1-dx).
    key = (b H2 + h2) W2 + w2, or the sentinel B H2 W2 (coefficient 0) when the texel is outside the map, the coordinate is not finite
    or |floor| > 2e9.  In fp32 a term is (g * wy) * wx with wy or wx = 1 - d rounded: 4 roundings at most; three more for adding four
    terms; one for their second-order products: K_COEF = 8, relative to coef_mag = sum |g| wy wx."""
    B, N, H1, W1, _ = coords.shape
    rd, P1 = 2 * r + 1, H1 * W1
    S, fp = B * N * P1, (rd + 1) ** 2
    finite, fx, fy, dx, dy = (t.reshape(S) for t in _corr_floor(coords))
    ok = finite & (fx.abs() <= 2.0e9) & (fy.abs() <= 2.0e9)
    z = torch.zeros_like(fx)
    ix0, iy0 = torch.where(ok, fx, z).long() - r, torch.where(ok, fy, z).long() - r
    s = torch.arange(S)
    b, p = s // (N * P1), s % P1
    gs = g.detach().cpu().double().reshape(B, N, rd * rd, P1).permute(0, 1, 3, 2).reshape(S, rd * rd)
    keys = torch.empty(S, fp, dtype=torch.int64)
    coef = torch.zeros(S, fp, dtype=torch.float64)
    cmag = torch.zeros(S, fp, dtype=torch.float64)
    for iy in range(rd + 1):
        for ix in range(rd + 1):
            h2, w2 = iy0 + iy, ix0 + ix
            inb = ok & (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)
            c, m = torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
            for cy, cx, wy, wx in ((iy - 1, ix - 1, dy, dx), (iy - 1, ix, dy, 1 - dx), (iy, ix - 1, 1 - dy, dx), (iy, ix, 1 - dy, 1 - dx)):
                if 0 <= cy < rd and 0 <= cx < rd:
                    c += gs[:, cy + rd * cx] * wy * wx
                    m += gs[:, cy + rd * cx].abs() * wy * wx
            o = iy * (rd + 1) + ix
            keys[:, o] = torch.where(inb, (b * H2 + h2) * W2 + w2, torch.full_like(h2, B * H2 * W2))
            coef[:, o] = torch.where(inb, c, torch.zeros_like(c))
            cmag[:, o] = torch.where(inb, m, torch.zeros_like(m))
    src = (b * P1 + p).to(torch.int32)[:, None].expand(S, fp).contiguous()
    return keys, coef, cmag, src


def alt_corr_adjoint_ref64(f1, f2, coords, g, r):
    """alt_corr_bwd_kernel / the tuples + sorted reduction (correlation_kernel.cu:122-256) -> (g1, mag1, n1, g2, mag2, n2, keys, coef, src):
    g1 [B,H1,W1,C] = sum over the pixel's samples and their in-map footprint texels of coef * f2[texel] (n1 [B,H1,W1] terms, one fma
    each); g2 [B,H2,W2,C] = sum over the tuples of a texel of coef * f1[src] (n2 [B,H2,W2] = the texel's segment length); keys, coef, src
    flat in the order of cer_alt_corr_bwd_tuples_f32.  A sample with a non-finite coordinate or |floor| > 2e9 contributes nothing."""
    B, H1, W1, C = f1.shape
    _, H2, W2, _ = f2.shape
    P1, T = H1 * W1, H2 * W2
    keys, coef, cmag, src = alt_corr_tuples_ref64(coords, g, r, H2, W2)
    a = f1.detach().cpu().double().reshape(B * P1, C)
    t = torch.cat([f2.detach().cpu().double().reshape(B * T, C), torch.zeros(1, C, dtype=torch.float64)], 0)           # (row B*T: the sentinel)
    g1, mag1 = torch.zeros(B * P1, C, dtype=torch.float64), torch.zeros(B * P1, C, dtype=torch.float64)
    g2, mag2 = torch.zeros(B * T + 1, C, dtype=torch.float64), torch.zeros(B * T + 1, C, dtype=torch.float64)
    n1, n2 = torch.zeros(B * P1, dtype=torch.int64), torch.zeros(B * T + 1, dtype=torch.int64)
    sl = src[:, 0].long()
    for o in range(keys.shape[1]):
        k, c, m = keys[:, o], coef[:, o, None], cmag[:, o, None]
        inb = (k < B * T).long()
        g1.index_add_(0, sl, c * t[k])
        mag1.index_add_(0, sl, m * t[k].abs())
        n1.index_add_(0, sl, inb)
        g2.index_add_(0, k, c * a[sl])
        mag2.index_add_(0, k, m * a[sl].abs())
        n2.index_add_(0, k, inb)
    return (g1.view(B, H1, W1, C), mag1.view(B, H1, W1, C), n1.view(B, H1, W1), g2[:-1].view(B, H2, W2, C), mag2[:-1].view(B, H2, W2, C),
            n2[:-1].view(B, H2, W2), keys.reshape(-1), coef.reshape(-1), src.reshape(-1))


def tl_coord32(origin, disp, D, incre):
    """tl_coord (core/corr.py:107) in torch fp32: max((disp - origin) / incre + D//2, 0) - subtract, true division by fl32(incre), add,
    clamp, one fp32 rounding each, as __fsub_rn / __fdiv_rn / __fadd_rn."""
    inc = torch.tensor(float(incre), dtype=torch.float32)
    return torch.clamp_min((disp.detach().cpu().float() - origin.detach().cpu().float()) / inc + float(D // 2), 0.0)


def _tl_taps(c, D, L, r):
    """Every (level, tap) of the lookup: x = fl32((j - r) + c / 2^level) (the division is exact), i0 = floor x, w = x - i0 (exact) ->
    (level, j, length, i0 clamped into the level, mask of texel i0 in the level, i0 + 1 clamped, its mask, w as float64)."""
    for lv in range(L):
        n = D >> lv
        cl = c / float(1 << lv)
        for j in range(2 * r + 1):
            x = float(j - r) + cl
            fx = torch.floor(x)
            valid = (fx >= -1.0) & (fx <= float(n - 1))
            i0 = torch.where(valid, fx, torch.zeros_like(fx)).long()
            yield lv, j, n, i0.clamp(0, n - 1), valid & (i0 >= 0), (i0 + 1).clamp(0, n - 1), valid & (i0 + 1 < n), (x - fx).double()


def train_lookup_ref64(vol, origin, disp, D, incre, L, r):
    """train_lookup_fwd_kernel (core/corr.py:94-97,102-143; utils/bilinear_sampler.py:6-25): vol [V,D,P], origin, disp [P] ->
    (out, mag) [V, L (2r+1), P] float64.  Level l+1 = (a + b) * 0.5 of neighbouring pairs of level l, floor halving (the kernel's
    association; float64 here, so the kernel's level l carries l roundings); tap k = l (2r+1) + j is a (1 - w) + b w between texels i0
    and i0 + 1 of level l, zero outside it (1 - w, two products, one add: 4 roundings)."""
    V, _, P = vol.shape
    c = tl_coord32(origin, disp, D, incre)
    lev = [(vol.detach().cpu().double(), vol.detach().cpu().double().abs())]
    for _ in range(1, L):
        a, m = lev[-1]
        n = a.shape[1] // 2
        lev.append(((a[:, 0:2 * n:2] + a[:, 1:2 * n:2]) * 0.5, (m[:, 0:2 * n:2] + m[:, 1:2 * n:2]) * 0.5))
    taps = 2 * r + 1
    out = torch.zeros(V, L * taps, P, dtype=torch.float64)
    mag = torch.zeros_like(out)
    for lv, j, n, ia, oka, ib, okb, w in _tl_taps(c, D, L, r):
        for src, dst in zip(lev[lv], (out, mag)):
            a = src.gather(1, ia.view(1, 1, P).expand(V, 1, P))[:, 0] * oka
            b = src.gather(1, ib.view(1, 1, P).expand(V, 1, P))[:, 0] * okb
            dst[:, lv * taps + j] = a * (1 - w) + b * w
    return out, mag


def train_lookup_level_adjoints64(gout, origin, disp, D, incre, L, r):
    """The per-level accumulators of train_lookup_bwd_kernel before the fold -> [(acc, mag [V, D >> l, P], count [D >> l, P])]."""
    V, _, P = gout.shape
    c = tl_coord32(origin, disp, D, incre)
    g = gout.detach().cpu().double()
    taps = 2 * r + 1
    accs = [(torch.zeros(V, D >> lv, P, dtype=torch.float64), torch.zeros(V, D >> lv, P, dtype=torch.float64),
             torch.zeros(D >> lv, P, dtype=torch.int64)) for lv in range(L)]
    for lv, j, n, ia, oka, ib, okb, w in _tl_taps(c, D, L, r):
        acc, mag, cnt = accs[lv]
        gj = g[:, lv * taps + j]
        for idx, ok, wt in ((ia, oka, 1 - w), (ib, okb, w)):
            e = idx.view(1, 1, P).expand(V, 1, P)
            acc.scatter_add_(1, e, (gj * wt * ok)[:, None])
            mag.scatter_add_(1, e, (gj.abs() * wt * ok)[:, None])
            cnt.scatter_add_(0, idx.view(1, P), ok.long().view(1, P))
    return accs


def train_lookup_adjoint_ref64(gout, origin, disp, D, incre, L, r):
    """train_lookup_bwd_kernel: gout [V, L (2r+1), P] -> (grad, mag [V,D,P], n [D,P]): the taps of a level added into the level's row
    (g (1 - w) into i0, g w into i0 + 1, where inside), then level 0 gets  g0[d] + sum_l gl[d >> l] 2^-l  for d >> l < D >> l - an odd
    length leaves its last element without a partner.  n: the taps added into the element's cells plus the folded levels."""
    accs = train_lookup_level_adjoints64(gout, origin, disp, D, incre, L, r)
    grad, mag, n = accs[0][0].clone(), accs[0][1].clone(), accs[0][2].clone()
    d = torch.arange(D)
    for lv in range(1, L):
        i = d >> lv
        ok = i < (D >> lv)
        grad[:, d[ok]] += accs[lv][0][:, i[ok]] * 0.5 ** lv
        mag[:, d[ok]] += accs[lv][1][:, i[ok]] * 0.5 ** lv
        n[d[ok]] += accs[lv][2][i[ok]] + 1
    return grad, mag, n


def upsample_ac_taps(n_in, n_out):
    """up_tap of csrc/train_ops.hip (torch's upsample_bilinear2d, align_corners=True) for every output index: scale = fl32((in-1) /
    (out-1)) (0 for out = 1), s = fl32(scale * dst), i0 = min((int) s, in-1), i1 = i0 + 1 clamped, l1 = s - i0 (exact), l0 = 1 - l1
    (float64 here; one rounding in the kernel) -> (i0, i1 int64, l0, l1 float64)."""
    one = torch.tensor(1.0, dtype=torch.float32)
    scale = (one * float(n_in - 1)) / (one * float(n_out - 1)) if n_out > 1 else one * 0.0
    s = scale * torch.arange(n_out, dtype=torch.float32)
    i0 = s.long().clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = (s - i0.float()).double()
    return i0, i1, 1.0 - l1, l1


def upsample_ranges_brute(n_in, n_out):
    """{X : i0(X) == j or i1(X) == j} for every input texel j as [n_in, 2] int32 half-open ranges ((0, 0) for an empty set); the sets
    are checked to be contiguous."""
    i0, i1, _, _ = upsample_ac_taps(n_in, n_out)
    table = torch.zeros(n_in, 2, dtype=torch.int32)
    for j in range(n_in):
        X = ((i0 == j) | (i1 == j)).nonzero().reshape(-1)
        if X.numel():
            assert int(X[-1]) - int(X[0]) + 1 == X.numel(), (n_in, n_out, j)
            table[j, 0], table[j, 1] = int(X[0]), int(X[-1]) + 1
    return table


def upsample_ac_ref64(x, H, W):
    """upsample_ac_fwd_kernel (loss.py:18-19): x [n,h,w] -> (out, mag) [n,H,W] float64,  l0y (l0x a + l1x b) + l1y (l0x c + l1x d).  On the
    longest path: 1 - l1x, a product, the inner add, 1 - l1y, a product, the outer add = 6 roundings, one more for their second-order
    products: K_UP_FWD = 7."""
    n, h, w = x.shape
    y0, y1, ly0, ly1 = upsample_ac_taps(h, H)
    x0, x1, lx0, lx1 = upsample_ac_taps(w, W)
    res = []
    for v in (x.detach().cpu().double(), x.detach().cpu().double().abs()):
        top = v[:, y0][:, :, x0] * lx0 + v[:, y0][:, :, x1] * lx1
        bot = v[:, y1][:, :, x0] * lx0 + v[:, y1][:, :, x1] * lx1
        res.append(top * ly0[:, None] + bot * ly1[:, None])
    return res[0], res[1]


def upsample_ac_adjoint_pass64(g, n_in, dim):
    """One pass of the upsample adjoint (upsample_ac_bwd_{x,y}_kernel) along ``dim`` of g: out[j] = sum over the outputs X of range[j] of
    (l0(X) if i0(X) == j) + (l1(X) if i1(X) == j) times g[X] -> (out, mag, n [n_in], range table): n = the length of range[j], the
    trips of the kernel's loop.  Relative to mag, a term carries the rounding of l0 = 1 - l1 and of its product (2), and the n terms are
    joined by n - 1 adds: n + 1 roundings, and one to spare: (n + 2) u.  A trip adds two terms only where i0 == i1 == j, at the last
    texel: there l1 = s - (in-1) is 0 (an add of +-0, exact; on an axis with in = 1 every trip is of this kind and l0 = 1 makes the
    products exact too) or, where scale * dst rounds past in - 1, one ulp of it, and that one further add is the spare rounding."""
    g = g.detach().cpu().double()
    i0, i1, l0, l1 = upsample_ac_taps(n_in, g.shape[dim])
    shape = [1] * g.dim()
    shape[dim] = -1
    size = list(g.shape)
    size[dim] = n_in
    res = []
    for v in (g, g.abs()):
        o = torch.zeros(size, dtype=torch.float64)
        o.index_add_(dim, i0, v * l0.view(shape))
        o.index_add_(dim, i1, v * l1.view(shape))
        res.append(o)
    table = upsample_ranges_brute(n_in, g.shape[dim])
    return res[0], res[1], (table[:, 1] - table[:, 0]).long(), table


def upsample_ac_adjoint_ref64(g, h, w):
    """The whole adjoint, x pass then y pass: g [n,H,W] -> (grad, mag [n,h,w], n [h,w] = range lengths of both passes, (range_y, range_x))."""
    work, wmag, nx, rx = upsample_ac_adjoint_pass64(g, w, 2)
    grad, _, ny, ry = upsample_ac_adjoint_pass64(work, h, 1)
    mag = upsample_ac_adjoint_pass64(wmag, h, 1)[0]
    return grad, mag, ny[:, None] + nx[None, :], (ry, rx)


# ------------------------------------------------------------------------------------------------ post-processing kernels in float64
# csrc/fusion.hip (geometric consistency, multires merge / resize) and csrc/scan_ops.hip (image preparation); tests/test_postproc_parity_
# {cpu,gpu}.py.  numpy float64.  Every value of the geometric-consistency chain is a pair (v, e): v the float64 value, e a bound on
# |fp32 result - v| for ANY correct fp32 evaluation of the same expression (any order of the sums, products fused into the sums or not).
# With u = 2^-24 and gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1):
#   product of two pairs      |a| eb + |b| ea + ea eb + u (|a| + ea)(|b| + eb)          (the rounding acts on the perturbed operands)
#   matrix row, n terms       sum |m_i| e_i + gamma_n sum |m_i| (|v_i| + e_i) [+ |m_3|]   a term passes its product and at most n - 1 adds
#                             (n = 3: geo_mat3; n = 4: geo_mat34, the constant being the fourth term); an fma only removes roundings
#   quotient X / Z            needs low = |Z| - eZ > 0, else the element is UNDECIDABLE (e = inf):  ee = (eX + |X / Z| eZ) / low, e = ee + u (|X / Z| + ee)
#   sample at (xs, ys)        the kernel samples at ix = ((2 px / (w-1) - 1) + 1) / 2 * (w-1): four roundings (the doubling and the halving are
#                             exact), |ix - px| <= gamma_4 (|px| + (w-1) / 2) (the -1 / +1 pair rounds at the size of px - (w-1) / 2), so the
#                             coordinate is off by ec = e_px + gamma_4 (|px| + e_px + (w-1) / 2).  The zero-padded bilinear interpolant is
#                             continuous and, inside a cell, moves by at most |dx| Lx + |dy| Ly with Lx (Ly) the largest difference between
#                             horizontally (vertically) neighbouring taps of the cell's 2 x 2 footprint, zero padding counting as taps of
#                             value 0; the rectangle (xs +- ecx, ys +- ecy) meets at most the four cells of its corners (ec < 1/2 is
#                             required), so the move is bounded with the largest Lx, Ly of those.  The weights ix - floor(ix) and
#                             (floor(ix) + 1) - ix are exact except in the cells [-1, 0) and [0, 1), where one of each axis rounds by at
#                             most u / 2: < 2 u T with T the largest |tap| of the reachable cells.  A term tap * (wx * wy) passes 2 products and
#                             at most 3 adds, and sum |tap| w <= T:  e_ds = ecx Lx + ecy Ly + (gamma_5 + 2 u) T.  Where the reachable cells
#                             do not agree on holding a NaN tap the sample is undecidable; where all hold one it is NaN for sure.
#   difference xr - x         e_xr + u (|xr - x| + e_xr);  sum of two squares s: 2 |a| ea + ea^2 (both) + gamma_2 (sum of (|a| + ea)^2)
#   sqrt                      sqrt(s) - sqrt(max(s - es, 0)) (the larger side, the root being concave), then + u (dist + that)
#   |drep - d| / d            d is an input: e = (e_drep + u (|drep - d| + e_drep)) / |d|, then + u (|rel| + e);  d = 0 gives +inf where
#                             |drep| > e_drep (every mask false either way), d < 0 a negative rel as in the reference
#   (dsum + d) / (cnt + 1)    the S gated adds and the add of d: sum e_drep + gamma_(S+1) (sum (|drep| + e_drep) + |d|), divided by cnt + 1
#                             (exact), then + u (|v| + e)
# Nothing is tuned: no constant above comes from a measurement.
def _gam(k):
    return k * U24 / (1.0 - k * U24)


def _np():
    import numpy as np
    return np


def _san(e):
    np = _np()
    return np.where(np.isnan(e), np.inf, e)


def _prod(a, ea, b, eb):
    np = _np()
    return a * b, _san(np.abs(a) * eb + np.abs(b) * ea + ea * eb + U24 * (np.abs(a) + ea) * (np.abs(b) + eb))


def _rows(m, n, vals, errs):
    """Three rows of the row-major 3 x n matrix ``m`` (n = 4: the fourth column is the added constant) applied to three (value, bound) pairs."""
    np = _np()
    out = []
    for r in range(3):
        row = [float(t) for t in m[r * n:(r + 1) * n]]
        v = row[0] * vals[0] + row[1] * vals[1] + row[2] * vals[2]
        mag = sum(abs(row[i]) * (np.abs(vals[i]) + errs[i]) for i in range(3) if row[i] != 0.0)
        ein = sum(abs(row[i]) * errs[i] for i in range(3) if row[i] != 0.0)
        if n == 4:
            v, mag = v + row[3], mag + abs(row[3])
        out.append((v, _san(ein + _gam(n) * mag)))
    return out


def _quot(X, eX, Z, eZ):
    np = _np()
    low = np.abs(Z) - eZ
    ok = low > 0
    q = X / Z
    ee = (eX + np.abs(q) * eZ) / np.where(ok, low, 1.0)
    return q, np.where(ok, _san(ee + U24 * (np.abs(q) + ee)), np.inf)


def geo_cameras(N, h, w, seed=3):
    """The cameras of tests/test_cloud_gpu.py::_cameras: the ring of ``synthetic_scene`` with the focal length of an h x w image and a
    principal point off the centre -> (K [N,3,3], E [N,4,4]) fp32."""
    from cer_mvs_amd.synthetic import synthetic_scene
    _, poses, intr, _ = synthetic_scene(32, 32, N - 1, seed=seed)
    K, E = intr[0].clone().float(), poses[0].clone().float()
    K[:, 0, 0] = K[:, 1, 1] = 1.8 * w
    K[:, 0, 2], K[:, 1, 2] = w / 2.0 + 0.37, h / 2.0 - 0.21
    return K, E


def geo_thresholds(thre1, thre2):
    """The thresholds as the host forms them (csrc/fusion.hip:122-126): float32(i / thre1), float32(i / thre2), i = 2 .. 10 -> two float64 [9]."""
    np = _np()
    i = np.arange(2, 11, dtype=np.float64)
    return (i / float(thre1)).astype(np.float32).astype(np.float64), (i / float(thre2)).astype(np.float32).astype(np.float64)


def _geo_sample64(img, xs, ys, ex, ey):
    """Zero-padded bilinear sample of img [h, w] at the float64 coordinates (xs, ys) known to +- (ex, ey) -> (value, bound, NaN for sure,
    undecidable, outside-or-rim): see the table above."""
    np = _np()
    h, w = img.shape
    t = np.zeros((h + 4, w + 4))
    t[2:-2, 2:-2] = img                                                     # taps -2 .. w + 1; cells -2 .. w
    finite = np.isfinite(xs) & np.isfinite(ys)
    x, y = np.where(finite, xs, -9.0), np.where(finite, ys, -9.0)           # (the kernel returns 0 for a coordinate that is not finite)
    ecx = ex + _gam(4) * (np.abs(x) + ex + (w - 1) / 2.0)
    ecy = ey + _gam(4) * (np.abs(y) + ey + (h - 1) / 2.0)
    und = ~finite | ~(ecx < 0.5) | ~(ecy < 0.5)
    ecx, ecy = np.where(und, 0.0, ecx), np.where(und, 0.0, ecy)
    cell = lambda c, n: np.clip(np.floor(c), -2, n).astype(np.int64) + 2
    cx, cy = cell(x, w), cell(y, h)
    fx, fy = np.clip(x - np.floor(x), 0.0, 1.0), np.clip(y - np.floor(y), 0.0, 1.0)
    t00, t01, t10, t11 = t[cy, cx], t[cy, cx + 1], t[cy + 1, cx], t[cy + 1, cx + 1]
    val = (t00 * (1 - fx) + t01 * fx) * (1 - fy) + (t10 * (1 - fx) + t11 * fx) * fy
    with np.errstate(invalid="ignore"):
        Lx = np.maximum(np.abs(t[:-1, 1:] - t[:-1, :-1]), np.abs(t[1:, 1:] - t[1:, :-1]))      # per cell [h + 3, w + 3]
        Ly = np.maximum(np.abs(t[1:, :-1] - t[:-1, :-1]), np.abs(t[1:, 1:] - t[:-1, 1:]))
        T = np.maximum(np.maximum(np.abs(t[:-1, :-1]), np.abs(t[:-1, 1:])), np.maximum(np.abs(t[1:, :-1]), np.abs(t[1:, 1:])))
    nanc = np.isnan(t[:-1, :-1]) | np.isnan(t[:-1, 1:]) | np.isnan(t[1:, :-1]) | np.isnan(t[1:, 1:])
    lx = ly = tt = np.zeros_like(x)
    n_any, n_all = np.zeros(x.shape, bool), np.ones(x.shape, bool)
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            qx, qy = cell(x + sx * ecx, w), cell(y + sy * ecy, h)
            lx, ly, tt = np.fmax(lx, Lx[qy, qx]), np.fmax(ly, Ly[qy, qx]), np.fmax(tt, T[qy, qx])
            n_any, n_all = n_any | nanc[qy, qx], n_all & nanc[qy, qx]
    und = und | (n_any & ~n_all)
    nan = n_all & ~und
    err = ecx * lx + ecy * ly + (_gam(5) + 2 * U24) * tt
    zero = ~finite
    val = np.where(zero, 0.0, val)
    err = np.where(zero, 0.0, np.where(und | nan, np.inf, err))
    rim = ~finite | (np.floor(xs) < 0) | (np.floor(xs) >= w - 1) | (np.floor(ys) < 0) | (np.floor(ys) >= h - 1)
    return val, err, nan, und & finite, rim


def geo_ref64(depth_ref, depth_src, cams, thre1, thre2):
    """Float64 restatement of geo_consistency_kernel (csrc/fusion.hip:57-100; reference fusion.py:39-106, :226-236) with a carried
    bound.  depth_ref [H,W], depth_src [S,H,W], cams [S,60]: the fp32 tensors the kernel is given, promoted; the thresholds as the host
    rounds them.  Samples directly at (xs, ys).  -> dict:
      xs, ys, rel, drep, dist   (value, bound) [S,H,W]; bound = inf where undecidable; rel = +inf, bound 0 where d = 0 and drep is not 0 for sure
      nan_in, nan               [S,H,W] bool: NaN for sure - xs, ys (``nan_in``: d is NaN); drep, dist, rel (``nan``: also a NaN tap)
      m_lo, m_hi                [9,S,H,W] bool: the mask is true for sure / may be true (equal: decided)
      geo_lo, geo_hi            [H,W] bool: the vote from the lowest / highest possible counts
      est, est_ok               (value, bound) [H,W], and where every view's m10 is decided (elsewhere the pixel is undecidable)
      rim                       [S,H,W] bool: the sample's footprint reaches outside the source image (or the coordinate is not finite)
      cnt_lo, cnt_hi            [9,H,W] the lowest / highest possible counts"""
    np = _np()
    d = np.asarray(depth_ref, dtype=np.float64)
    src = np.asarray(depth_src, dtype=np.float64)
    cams = np.asarray(cams, dtype=np.float64)
    S, H, W = src.shape
    td, tr = geo_thresholds(thre1, thre2)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    zero = np.zeros_like(d)
    keys = ("xs", "ys", "rel", "drep", "dist")
    out = {k: (np.empty((S, H, W)), np.empty((S, H, W))) for k in keys}
    out.update(nan_in=np.zeros((S, H, W), bool), nan=np.zeros((S, H, W), bool), rim=np.zeros((S, H, W), bool),
               m_lo=np.zeros((9, S, H, W), bool), m_hi=np.zeros((9, S, H, W), bool))
    with np.errstate(all="ignore"):
        xd, yd = _prod(xx, zero, d, zero), _prod(yy, zero, d, zero)
        for s in range(S):
            c = cams[s]
            p = _rows(c[0:9], 3, [xd[0], yd[0], d], [xd[1], yd[1], zero])
            p = _rows(c[9:21], 4, [q[0] for q in p], [q[1] for q in p])
            p = _rows(c[21:30], 3, [q[0] for q in p], [q[1] for q in p])
            xs, exs = _quot(p[0][0], p[0][1], p[2][0], p[2][1])
            ys, eys = _quot(p[1][0], p[1][1], p[2][0], p[2][1])
            nan_in = np.isnan(d)
            exs, eys = np.where(nan_in, np.inf, exs), np.where(nan_in, np.inf, eys)
            ds, eds, nan_s, und_s, rim = _geo_sample64(src[s], xs, ys, exs, eys)
            und_s = und_s | (~nan_in & ~(np.isfinite(exs) & np.isfinite(eys)))    # (Z not bounded away from 0: whatever the kernel samples)
            nan = (nan_in | nan_s) & ~und_s
            a, b = _prod(xs, exs, ds, eds), _prod(ys, eys, ds, eds)
            p = _rows(c[30:39], 3, [a[0], b[0], ds], [a[1], b[1], eds])
            p = _rows(c[39:51], 4, [q[0] for q in p], [q[1] for q in p])
            drep, edrep = p[2]
            q = _rows(c[51:60], 3, [t[0] for t in p], [t[1] for t in p])
            xr, exr = _quot(q[0][0], q[0][1], q[2][0], q[2][1])
            yr, eyr = _quot(q[1][0], q[1][1], q[2][0], q[2][1])
            ex, ey = xr - xx, yr - yy
            eex, eey = exr + U24 * (np.abs(ex) + exr), eyr + U24 * (np.abs(ey) + eyr)
            sq = ex * ex + ey * ey
            esq = _san(2 * np.abs(ex) * eex + eex * eex + 2 * np.abs(ey) * eey + eey * eey + _gam(2) * ((np.abs(ex) + eex) ** 2 + (np.abs(ey) + eey) ** 2))
            dist = np.sqrt(sq)
            edist = dist - np.sqrt(np.maximum(sq - esq, 0.0))
            edist = _san(edist + U24 * (dist + edist))
            num = np.abs(drep - d)
            enum = edrep + U24 * (num + edrep)
            erel = enum / np.abs(d)
            rel = num / d
            erel = _san(erel + U24 * (np.abs(rel) + erel))
            d0 = d == 0
            rel = np.where(d0, np.inf, rel)
            erel = np.where(d0, np.where(np.abs(drep) > edrep, 0.0, np.inf), erel)
            bad = nan | und_s
            for k, (v, e) in (("xs", (xs, exs)), ("ys", (ys, eys)), ("rel", (rel, erel)), ("drep", (drep, edrep)), ("dist", (dist, edist))):
                out[k][0][s] = v
                out[k][1][s] = e if k in ("xs", "ys") else np.where(bad, np.inf, e)
            out["nan_in"][s], out["nan"][s], out["rim"][s] = nan_in, nan, rim
            for i in range(9):
                d_t, d_f = dist + edist < td[i], dist - edist > td[i]               # (an infinite bound decides neither)
                r_t = np.where(d0, False, rel + erel < tr[i])
                r_f = np.where(d0, True, rel - erel > tr[i])                       # (d = 0: rel is +inf or NaN, false either way)
                sure_t = d_t & r_t & ~bad
                sure_f = ((d_f | r_f) & ~und_s) | nan
                out["m_lo"][i, s] = sure_t
                out["m_hi"][i, s] = ~sure_f
        n = 1 + S
        cl, ch = out["m_lo"].sum(1), out["m_hi"].sum(1)
        vote = lambda cnt: np.logical_or.reduce([cnt[8] >= n] + [cnt[i - 2] >= i for i in range(2, min(n, 11))])
        out["cnt_lo"], out["cnt_hi"] = cl, ch
        out["geo_lo"], out["geo_hi"] = vote(cl), vote(ch)
        m10 = out["m_lo"][8]
        ok = (out["m_lo"][8] == out["m_hi"][8]).all(0)
        dr, edr = np.where(m10, out["drep"][0], 0.0), np.where(m10, out["drep"][1], 0.0)
        cnt = m10.sum(0) + 1.0
        v = (dr.sum(0) + d) / cnt
        e = (edr.sum(0) + _gam(S + 1) * ((np.abs(dr) + edr).sum(0) + np.abs(d))) / cnt
        out["est"] = (v, _san(e + U24 * (np.abs(v) + e)))
        out["est_ok"] = ok
    return out


class GeoReport:
    """What ``check_geo`` found: ``fails`` = {output: {"n", "views", "levels", "rows", "blocks" (256-pixel launch blocks), "pixels", "index", "worst"}}
    for every output with an element outside its bound / a decided element that differs; ``undecidable`` = {output: share} (per level for
    the masks: "masks9[i]"); ``max_ratio`` = {output: worst |err| / bound over the bounded elements}; ``checked`` = the outputs present."""

    def __init__(self, where, H, W):
        self.where, self.H, self.W = where, H, W
        self.fails, self.undecidable, self.max_ratio, self.checked = {}, {}, {}, []

    @property
    def ok(self):
        return not self.fails

    def add(self, name, bad, und, ratio=None, worst=None):
        """bad, und: bool [..., H, W] with leading (level, view) / (view) / no axes."""
        np = _np()
        self.checked.append(name)
        lead = bad.ndim - 2
        if name == "masks9":
            for i in range(und.shape[0]):
                self.undecidable[f"masks9[{i}]"] = float(und[i].mean())
        else:
            self.undecidable[name] = float(und.mean())
        if ratio is not None:
            self.max_ratio[name] = float(ratio)
        if not bad.any():
            return
        idx = np.argwhere(bad)
        pix = idx[:, -2] * self.W + idx[:, -1]
        cnt = lambda a: {int(k): int(c) for k, c in zip(*np.unique(a, return_counts=True))}
        self.fails[name] = {"n": int(bad.sum()), "views": cnt(idx[:, lead - 1]) if lead >= 1 else {}, "levels": cnt(idx[:, 0]) if lead == 2 else {},
                            "rows": cnt(idx[:, -2]), "blocks": cnt(pix // 256), "pixels": pix, "index": idx, "worst": worst}

    def only(self, name, key):
        """The single view / level / row / block that holds every failing element of an output, else None."""
        d = self.fails.get(name, {}).get(key, {})
        return next(iter(d)) if len(d) == 1 else None

    def message(self):
        if self.ok:
            return f"{self.where}: every decided element agrees ({', '.join(self.checked)})"
        top = lambda d, k=6: ", ".join(f"{key}: {c}" for key, c in sorted(d.items(), key=lambda kv: -kv[1])[:k]) + (" ..." if len(d) > k else "")
        lines = [f"{self.where}: {self.H} x {self.W}"]
        for name, f in self.fails.items():
            lines.append(f"  {name}: {f['n']} decided elements wrong" + (f"; worst |err| / bound = {f['worst']:.4g}" if f["worst"] is not None else ""))
            if f["levels"]:
                lines.append(f"    levels - {top(f['levels'])}")
            if f["views"]:
                lines.append(f"    views - {top(f['views'])}")
            lines.append(f"    image rows - {len(f['rows'])}: {top(f['rows'])};  256-pixel blocks - {len(f['blocks'])}: {top(f['blocks'])}")
            for key, what in (("rows", "image row"), ("blocks", "block"), ("views", "view"), ("levels", "level")):
                if len(f[key]) == 1:
                    k = next(iter(f[key]))
                    lines.append(f"    => confined to {what} {k}" + (" (the last row)" if key == "rows" and k == self.H - 1 else ""))
        return "\n".join(lines)


def _check_pair(got, val, err, nan_sure, zero_ok=None, measure=None):
    """-> (bad, undecidable, worst ratio): NaN for sure -> got must be NaN; value +-inf with bound 0 -> got must equal it; a finite bound ->
    |got - val| <= bound; an infinite bound: undecidable.  ``zero_ok``: elements where an exact 0 is accepted as well; ``measure``: the
    elements the worst ratio is taken over (default: all bounded ones)."""
    np = _np()
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        und = ~nan_sure & ~np.isfinite(err)
        diff = np.abs(got - val)
        inb = np.where(np.isinf(val), got == val, diff <= err)
        good = np.where(nan_sure, np.isnan(got), inb)
        if zero_ok is not None:
            good = good | (zero_ok & (got == 0))
        bad = ~good & ~und
        meas = ~nan_sure & ~und & np.isfinite(val) & (err > 0) & (True if measure is None else measure)
        ratio = np.where(meas, diff / np.where(err > 0, err, 1.0), 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return bad, und, float(ratio.max()) if ratio.size else 0.0


def check_geo(ref, where="", xs=None, ys=None, rel=None, drep=None, masks9=None, geo_mask=None, depth_est=None):
    """The outputs of a launch (whichever are given; numpy or CPU tensors) against ``geo_ref64``'s dict -> GeoReport.
    xs, ys, rel: inside the bound, NaN where the reference is NaN for sure.  drep (the kernel's ``m10 ? drep : 0``): the bound where m10 is
    true for sure, exactly 0 where it is false for sure, either where it is open.  masks9: every decided element equal (an element is decided
    false when dist OR rel is beyond its threshold by more than the bound, true when both are inside by more than it - no weaker than asking
    both to be decided), any byte other than 0 / 1 fails.  geo_mask: equal wherever the lowest and the highest possible counts give the same
    vote.  depth_est: inside the bound wherever every view's m10 is decided, NaN where d is."""
    np = _np()
    S, H, W = ref["nan"].shape
    rep = GeoReport(where, H, W)
    as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    for name, got, nan in (("xs", xs, ref["nan_in"]), ("ys", ys, ref["nan_in"]), ("rel", rel, ref["nan"])):
        if got is not None:
            bad, und, r = _check_pair(as_np(got), ref[name][0], ref[name][1], nan)
            rep.add(name, bad, und, r, r)
    if drep is not None:
        g = as_np(drep).astype(np.float64)
        lo, hi = ref["m_lo"][8], ref["m_hi"][8]
        bad, und, r = _check_pair(g, ref["drep"][0], ref["drep"][1], np.zeros_like(lo), zero_ok=~lo, measure=lo)
        bad = np.where(~hi, g != 0, bad)                      # (a NaN is != 0: a sentinel left behind fails)
        rep.add("drep", bad, (lo != hi) | (lo & und), r, r)
    if masks9 is not None:
        g = as_np(masks9)
        dec = ref["m_lo"] == ref["m_hi"]
        rep.add("masks9", (dec & (g != ref["m_lo"])) | (g > 1), ~dec)
    if geo_mask is not None:
        g = as_np(geo_mask)
        dec = ref["geo_lo"] == ref["geo_hi"]
        rep.add("geo_mask", (dec & (g != ref["geo_lo"])) | (g > 1), ~dec)
    if depth_est is not None:
        ok = ref["est_ok"]
        nan = np.isnan(ref["est"][0]) & ok & ref["nan_in"][0]
        bad, und, r = _check_pair(as_np(depth_est), ref["est"][0], np.where(ok, ref["est"][1], np.inf), nan)
        rep.add("depth_est", bad, und, r, r)
    return rep


def geo_census(ref):
    """The non-vacuity figures of a case, from the reference alone -> dict: per level the share of true / false among the decided mask
    elements (``true_share`` [9]), the share of samples outside the source image or on its zero-padded rim (``rim_share``), the number of
    decided pixels whose vote is lit by a lower level (cnt[i-2] >= i for some i < n) while cnt[8] < n (``lit_by_lower``)."""
    np = _np()
    dec = ref["m_lo"] == ref["m_hi"]
    n = 1 + ref["nan"].shape[0]
    true_share = [float((ref["m_lo"][i] & dec[i]).sum() / max(1, dec[i].sum())) for i in range(9)]
    decided = ref["geo_lo"] == ref["geo_hi"]
    lower = ref["geo_lo"] & decided & (ref["cnt_hi"][8] < n)
    return {"true_share": true_share, "rim_share": float(ref["rim"].mean()), "lit_by_lower": int(lower.sum())}


# ---- image preparation (csrc/scan_ops.hip: prep_tap, image_prep_kernel) in float64 from torch's fp32 taps
def prep_taps(n_in, n_out, first, count):
    """prep_tap for output indices first .. first + count - 1 of an axis resized from n_in to n_out: scale = fl32((in-1) / (out-1)) (0 for
    out = 1), s = fl32(scale * dst) - one fp32 product -, i0 = min(trunc(s), in-1), i1 = i0 + 1 clamped, l1 = fl32(s - i0), l0 = fl32(1 - l1)
    -> (i0, i1 int64, l0, l1 float64 holding fp32 values): torch's upsample_bilinear2d(align_corners=True) taps."""
    np = _np()
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    dst = np.arange(first, first + count).astype(np.float32)
    s = (scale * dst).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1.0) - l1).astype(np.float32)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


K_PREP = 4                   # tap product, inner sum, row product, outer sum: the roundings on the path of one term


def prep_ref64(img, H2, W2, y0, x0, H, W):
    """img [3,H0,W0] (the fp32 values the kernel reads, channels already in output order) resized to H2 x W2 (bilinear, align_corners=True),
    window rows y0 .. y0 + H - 1, columns x0 .. x0 + W - 1 -> (value, mag) float64 [3,H,W]: l0y (l0x a + l1x b) + l1y (l0x c + l1x d) from the
    fp32 weights of ``prep_taps``, and the same on absolute values.  Every term passes at most four fp32 roundings: gamma_4 * mag bounds a
    correct fp32 evaluation.  Equal sizes: the weights are (1, 0) and the value is the source texel."""
    np = _np()
    a = np.asarray(img, dtype=np.float64)
    ya, yb, ly0, ly1 = prep_taps(a.shape[1], H2, y0, H)
    xa, xb, lx0, lx1 = prep_taps(a.shape[2], W2, x0, W)
    res = []
    for v in (a, np.abs(a)):
        top = v[:, ya][:, :, xa] * lx0 + v[:, ya][:, :, xb] * lx1
        bot = v[:, yb][:, :, xa] * lx0 + v[:, yb][:, :, xb] * lx1
        res.append(top * ly0[None, :, None] + bot * ly1[None, :, None])
    return res[0], res[1]


def check_prep(got, ref, mag, where=""):
    """[3,H,W] against ``prep_ref64`` at gamma_4 * mag, element by element -> ParityReport over the H x W image (channels as channels)."""
    got = torch.as_tensor(got).detach().cpu()
    _, H, W = got.shape
    flat = lambda t: torch.as_tensor(t, dtype=torch.float64).reshape(3, H * W).t()
    return check_elementwise(flat(got), flat(ref), flat(mag), _gam(K_PREP), 0.0, where, h=H, w=W, tile=(1, 4))


def bits_equal(got, want):
    """float32 arrays compared through their int32 views -> bool array; a NaN equals a NaN (an invalid operation yields the default NaN
    with the sign bit set on x86 and clear on the GPU: the payload is not part of the documented sequence)."""
    np = _np()
    g, w = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return (g.view(np.int32) == w.view(np.int32)) | (np.isnan(g) & np.isnan(w))


# ------------------------------------------------------------------------------------------------ update-loop launches in float64
# The pure float64 pieces of one GRU iteration, shared by tests/test_fullsize_parity_gpu.py (the s16 loop) and
# tests/test_wide_parity_{cpu,gpu}.py (the wide-range loop): pixel-major [P, C] in and out.
def nchw(x, h, w):
    """[P, C] -> [1, C, h, w]"""
    return x.t().reshape(1, x.shape[1], h, w)


def plain(x):
    """[1, C, h, w] -> [P, C]"""
    return x[0].permute(1, 2, 0).reshape(-1, x.shape[1])


def conv64(x, wt, h, w):
    """3 x 3, padding 1, float64, pixel-major in and out."""
    return plain(F.conv2d(nchw(x, h, w), wt.double(), None, padding=1))


def conv_ref(x, xmag, wt, bias, h, w, record_as=None, yardstick=None):
    """-> (conv(x, w) + bias, conv(xmag, |w|) + |bias|) in float64.  When recording (``yardstick``: a dict, ``record_as``: the key): also
    the reference-only yardstick - the same convolution in float32 on the CPU against the float64 result, normalised like the kernels'
    errors."""
    ref = conv64(x, wt, h, w)
    mag = conv64(xmag, wt.abs(), h, w)
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if record_as and yardstick is not None:
        y32 = plain(F.conv2d(nchw(x, h, w).float(), wt.float(), None, padding=1)).double()
        if bias is not None:
            y32 = y32 + bias.double()
        yardstick[record_as] = float(((y32 - ref).abs() / mag.clamp_min(1e-300)).max())
    return ref, mag


def disp_feature_parts(disp, h, w):
    """disp [P] float64 -> (100 * (unfold7x7(d) - d) [P, 49], 100 * (unfold7x7|d| + |d|) [P, 49]): core/update.py:80-85,97 and the
    magnitude of the two parts the collapsed form sums separately."""
    d = disp.reshape(1, 1, h, w)
    u = F.unfold(d, [7, 7], padding=3).view(1, 49, h, w)
    ua = F.unfold(d.abs(), [7, 7], padding=3).view(1, 49, h, w)
    return plain(100 * (u - d)), plain(100 * (ua + d.abs()))


def wsum(wt):
    """sum |w| over a conv's taps and input channels, per output channel: [1, Cout]"""
    return wt.double().abs().sum((1, 2, 3))[None]


def delta_sum64(T, bias, disp, h, w):
    """T [nhalf, 9, P], disp [P] float64 -> (disp + 0.01 * (bias + sum of the taps at the neighbours, zero outside), its magnitude)."""
    nh = T.shape[0]
    img = F.pad(T.reshape(nh, 9, h, w), (1, 1, 1, 1))
    s = torch.zeros(h, w, dtype=torch.float64)
    sa = torch.zeros(h, w, dtype=torch.float64)
    for tap in range(9):
        dy, dx = tap // 3, tap % 3                     # (padded coordinates: y + dy - 1 + 1)
        s += img[:, tap, dy:dy + h, dx:dx + w].sum(0)
        sa += img[:, tap, dy:dy + h, dx:dx + w].abs().sum(0)
    return disp + 0.01 * (s.reshape(-1) + bias), 0.01 * (sa.reshape(-1) + abs(bias)) + disp.abs()


def lookup_ref(vol, origin, disp, w0t, b0, D, incre, L=3, r=5):
    """vol [P, >=D] level-0 rows, origin, disp [P], w0t [33, 64], b0 [64], all float64 (the fp32 values the kernel read) ->
    (relu(conv1x1(lookup)), c-scaled magnitude, absolute term of the fp32 index arithmetic): core/corr.py:94-143, core/update.py:61-64."""
    from oracle import cer_oracle as O
    P = vol.shape[0]
    levels = O.pyramid(vol[None, :, :D], L)
    feats = O.lookup(levels, origin.view(1, P), disp.view(1, P), D, incre, r).reshape(L * (2 * r + 1), P).t()      # [P, 33]
    ref = torch.relu(feats @ w0t + b0)
    mag = feats.abs() @ w0t.abs() + b0.abs()
    t = (disp - origin) / incre
    dt = 4 * 2.0 ** -24 * (t.abs() + D / 2)
    idx = torch.zeros(P, w0t.shape[1], dtype=torch.float64)
    for l, lv in enumerate(levels):
        row = F.pad(lv[0], (1, 1))
        step = (row[:, 1:] - row[:, :-1]).abs().max(1).values                     # largest |v[i+1] - v[i]| of the row, zero border included
        idx += (dt / 2 ** l * step)[:, None] * w0t[l * (2 * r + 1):(l + 1) * (2 * r + 1)].abs().sum(0)[None]
    return ref, mag, idx


def loop_ref64(iters, vol, origin, net, disp, inp, g, D, incre, h, w, L=3, r=5):
    """``iters`` iterations of the update step (``_S16Loop.step`` / ``_WideLoop.step`` with delta="now"; core/update.py:87-120, 17-25) in
    float64, from the values the device holds at the start: vol [P, >= D] level-0 rows, origin, disp [P], net, inp [P, 64] (the hidden state
    read back through its layout's inverse), all float64; ``g``: ``update._stage_weights(ub, stage, "cpu")``.  One iteration is
    ``lookup_ref`` -> relu(corr2) -> sigmoid(z | r) over net | inp | ``disp_feature_parts`` | corr -> tanh(q) over r*net | ... -> the GRU
    blend -> relu(delta1) projected per channel half and tap, summed by ``delta_sum64``.  -> [(net, disp) after iteration 0, 1, ...]."""
    d = lambda t: t.detach().cpu().double()
    w0t, b0 = d(g.w0t), d(g.b0)
    wc, bc = d(g.corr2.weight), d(g.corr2.bias)
    wzr, bzr, wq, bq = d(g.wzr), d(g.bzr), d(g.wq), d(g.bq)
    w1, b1 = d(g.delta1.weight), d(g.delta1.bias)
    proj = d(g.delta2.weight)[0].reshape(-1, 128, 9)                               # [half, channel, tap]
    net, disp, inp, vol, origin = net.double(), disp.double(), inp.double(), vol.double(), origin.double()
    out = []
    for _ in range(iters):
        c1 = lookup_ref(vol, origin, disp, w0t, b0, D, incre, L, r)[0]
        c2 = torch.relu(conv64(c1, wc, h, w) + bc)
        feat = disp_feature_parts(disp, h, w)[0]
        zr = torch.sigmoid(conv64(torch.cat([net, inp, feat, c2], 1), wzr, h, w) + bzr)
        z, rr = zr[:, :64], zr[:, 64:]
        q = torch.tanh(conv64(torch.cat([rr * net, inp, feat, c2], 1), wq, h, w) + bq)
        net = (1 - z) * net + z * q
        hid = torch.relu(conv64(net, w1, h, w) + b1)
        T = torch.stack([(hid[:, hf * 128:(hf + 1) * 128] @ proj[hf]).t() for hf in range(proj.shape[0])], 0)      # [nhalf, 9, P]
        disp = delta_sum64(T, g.d2b, disp, h, w)[0]
        out.append((net, disp))
    return out


# ------------------------------------------------------------------------------------------------ the wide-range loop (_WideLoop)
# References and bounds of the launches of ``_WideLoop.step`` (cer-mvs_amd/update.py: csrc/gru_f16x3.hip, csrc/gru.hip), shared by
# tests/test_wide_parity_gpu.py (the kernels) and tests/test_wide_parity_cpu.py (an fp32 emulation with planted corruptions).  Every
# ``wide_*`` function returns (ref, mag, abs_term) for ``check_elementwise(got, ref, mag, WIDE_C, abs_term)``: no constant is fitted.
WIDE_C = 2e-6                # per-element constant of an f16x3 / fp32-MFMA dot: tests/test_hip_parity.py::test_conv3x3_f16x3_dynamic_range
WIDE_ABS = 3e-11             # its absolute companion, per unit of sum|w| (the f16 subnormal step of the scaled lo half), same test
WIDE_ACT_ABS = 2.0 ** -20    # sigmoid / tanh / exp of the device library, as in the s16 loop's bounds
WIDE_TILE = (4, 32)          # pixel tile of cer_conv3x3_f16x3 (HX_TH x HX_TW)
WIDE_TILE_F32 = (8, 16)      # pixel tile of cer_conv3x3_f32 (CV_TH x CV_TW)
DT_STRIP = 16                # pixels of a cer_delta_tail_f32 strip (one wave); a block holds 4 strips
C_DSUM = 22 * 2.0 ** -24     # delta_sum: an 18-term fp32 sum, one product, two sums (tests/test_fullsize_parity_gpu.py)


def split32_np(x):
    """The split32 layout (include/cer_mvs.h; csrc/gru_f16x3.hip: hx_store_split8 / cer_split2) restated in numpy: fp32 [P, C], C % 32
    == 0 -> fp32 [P, C] whose bytes are, per pixel and 32-channel chunk, 32 f16 hi halves | 32 f16 lo halves with hi = f16(clamp(x,
    +-65504)) and lo = f16((clamp(x) - hi) * 2^11), both conversions round-to-nearest-even."""
    np = _np()
    x = np.clip(np.ascontiguousarray(x, dtype=np.float32), np.float32(-65504.0), np.float32(65504.0))
    P, C = x.shape
    assert C % 32 == 0
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    halves = np.concatenate([hi.reshape(P, C // 32, 32), lo.reshape(P, C // 32, 32)], 2)
    return np.ascontiguousarray(halves).reshape(P, 2 * C).view(np.float32)


def split32_inverse_np(s):
    """split32 [P, C] -> fp32 [P, C]: hi + 2^-11 lo (hx_load_split8; the product is exact, so the fused form rounds once like this one)."""
    np = _np()
    s = np.ascontiguousarray(s, dtype=np.float32)
    P, C = s.shape
    halves = s.view(np.float16).reshape(P, C // 32, 64).astype(np.float32)
    return (halves[:, :, 32:] * np.float32(1.0 / 2048.0) + halves[:, :, :32]).reshape(P, C)


def split32_quantum(ref):
    """What storing ``ref`` in the split32 layout may move it by: hi is f16(x), lo is f16 of the residual times 2^11 - the residual is
    below 2^-11 |x| and keeps 11 bits, so its last bit is 2^-22 |x|; below the f16 normal range the lo half steps by 2^-24, i.e. 2^-35 of x."""
    return 2.0 ** -22 * ref.abs() + 2.0 ** -35


def wide_interior_tiles(h, w, tile=WIDE_TILE):
    """[tiles_y, tiles_x] bool: the tiles of cer_conv3x3_f16x3 that evaluate a disparity source in the collapsed 81-tap form
    (conv3x3_f16x3_kernel: ``coll``) - every pixel of the tile has its 3 x 3 neighbourhood inside the image, which also excludes the
    first tile row and column."""
    th, tw = tile
    ty0 = torch.arange((h + th - 1) // th) * th
    tx0 = torch.arange((w + tw - 1) // tw) * tw
    return ((ty0 >= 1) & (ty0 + th <= h - 1))[:, None] & ((tx0 >= 1) & (tx0 + tw <= w - 1))[None, :]


def wide_conv_parts(x, xmag, wt, bias, h, w, init=None):
    """Pre-activation of one conv launch of the wide loop -> (pre, mag, abs) with |kernel - pre| <= WIDE_C * mag + abs: ``conv_ref`` on
    the sources (the disparity source enters ``xmag`` through ``disp_feature_parts``), the accumulator seed ``init`` [P, Cout] added with
    its own magnitude, abs = WIDE_ABS * sum|w| over the taps inside the image."""
    pre, mag = conv_ref(x, xmag, wt, bias, h, w)
    if init is not None:
        pre, mag = pre + init, mag + init.abs()
    return pre, mag, WIDE_ABS * conv64(torch.ones_like(x), wt.abs(), h, w)


def wide_relu_parts(pre, mag, abs_t, split):
    ref = torch.relu(pre)
    return ref, mag, abs_t + (split32_quantum(ref) if split else 0.0)


def wide_gates_parts(pre, mag, abs_t, hprev, split):
    """GATES epilogue -> ((z parts), (r*h parts)).  sigmoid is Lipschitz 1/4 (<= 1 is used), + WIDE_ACT_ABS for the device exp / rcp;
    r*h: that bound times |h| (``hprev``: the value the kernel read, exact), one rounding of the product, the split32 quantum."""
    half = pre.shape[1] // 2
    z = torch.sigmoid(pre[:, :half])
    rh = torch.sigmoid(pre[:, half:]) * hprev
    za = abs_t[:, :half] + WIDE_ACT_ABS
    ra = (abs_t[:, half:] + WIDE_ACT_ABS) * hprev.abs() + 2.0 ** -24 * rh.abs() + (split32_quantum(rh) if split else 0.0)
    return (z, mag[:, :half], za), (rh, mag[:, half:] * hprev.abs(), ra)


def wide_gru_parts(pre, mag, abs_t, z, hprev, split):
    """GRU epilogue: (1 - z) h + z tanh(pre) with the z and the PREVIOUS hidden state the kernel read.  tanh is Lipschitz 1: |z| *
    (pre-activation bound + WIDE_ACT_ABS); the blend's four roundings (1 - z, two products, one sum) at 2^-24 of |h| + |z|."""
    ref = (1 - z) * hprev + z * torch.tanh(pre)
    a = z.abs() * (abs_t + WIDE_ACT_ABS) + 4 * 2.0 ** -24 * (hprev.abs() + z.abs()) + (split32_quantum(ref) if split else 0.0)
    return ref, mag * z.abs(), a


def wide_delta_parts(pre, mag, abs_t, w2):
    """Fused delta head (EPI_DELTA): hid = relu(pre) is split to hi|lo f16 in LDS (hx_split: the split32 quantum) and projected with the
    256 -> 1 conv's weights per channel half and tap, ``w2`` [1, C, 3, 3] -> tap planes [P, nhalf * 9] (column = half * 9 + tap).  The
    hidden map's bound is projected with |w2|; the projection's own f16x3 products add WIDE_C * sum_c |w2| |hid|."""
    hid = torch.relu(pre)
    hb = WIDE_C * mag + abs_t + split32_quantum(hid)
    C = hid.shape[1]
    nhalf = C // 128
    proj = w2.double()[0].reshape(nhalf, 128, 9)                                  # [half, channel, tap]
    cols = lambda t, p: torch.cat([t[:, hf * 128:(hf + 1) * 128] @ p[hf] for hf in range(nhalf)], 1)
    return cols(hid, proj), cols(hid, proj.abs()), cols(hb, proj.abs())


def delta_tail_depth(C):
    """Roundings on the longest path of one cer_delta_tail_f32 output sum (csrc/gru.hip: delta_tail_kernel).  A lane owns 4 channels of
    every 256: per source column and kx it runs ONE fma chain over its C / 256 quads and the three ky taps - 12 * C / 256 fmas, one
    rounding each; the rolling accumulators add two of those chains' results (accA + c1, accB + c2): 2; cer_row16_sum is four DPP add
    levels (quad, quad, half-row mirror, row mirror): 4; the two cross-row shuffles: 2.  n = 12 * C / 256 + 8.  (The issue's count of
    + 12 took the 16-lane sum as eight levels; this one is tighter and is what the tests apply.)"""
    return 12 * (C // 256) + 8


def delta_tail_ref64(hid, w_tap_c, bias, disp, h, w):
    """cer_delta_tail_f32 in float64 from the values it read: hid [P, C], w_tap_c [9, C] (tap = ky * 3 + kx), disp [P] ->
    ((disp_out ref, mag, abs), (delta ref, mag, abs)) for a check at c = 3 * 2^-24 (disp_out) / 2 * 2^-24 (delta).  s = 3 x 3 conv (zero padding), S = the same on absolute values.  The kernel's sum
    deviates by at most gamma_n S with n = ``delta_tail_depth``; then fl(fl(0.01f * fl(s + bias)) + disp): three roundings, each of a
    value <= 0.01f (S + |bias|) + |disp| (two for the delta output, which has no last sum).  0.01f is the fp32 constant."""
    C = hid.shape[1]
    wt = w_tap_c.double().reshape(3, 3, C).permute(2, 0, 1)[None]                  # [1, C, 3, 3]
    s, S = conv64(hid, wt, h, w)[:, 0], conv64(hid.abs(), wt.abs(), h, w)[:, 0]
    c01 = float(torch.tensor(0.01, dtype=torch.float32))
    n = delta_tail_depth(C)
    gam = n * U24 / (1 - n * U24)
    dl = c01 * (s + bias)
    dmag = c01 * (S + abs(bias))
    return (disp + dl, dmag + disp.abs(), c01 * gam * S), (dl, dmag, c01 * gam * S)


# ------------------------------------------------------------------------------------------------ cost volume from restated fp32 coordinates
# The projection of both cost-volume builders (csrc/cost_build.hip:41-43, 69-79; ClLane::project / cl_lane_ray of csrc/cost_lines.hip) is
# written in fully specified fp32 operations - __fmul_rn, __fadd_rn, fmaf, two IEEE divisions, -ffp-contract=off - so it can be restated
# bit for bit in numpy float32 from the reference's definition (core/corr.py:56-65, utils/projective_ops.py:26-28) as a third
# implementation that shares no code with either kernel.  With the cell and the two fractions of every sample known exactly, what is left
# to a kernel is the rounding of the 64-channel dot, the four bilinear weights and the view sum: ``cost_bound``.
def fma32(a, b, c):
    """round_to_float32(a * b + c) with ONE rounding, on numpy arrays (this Python has no math.fma).  The product of two float32 is exact
    in float64 (48 significant bits); s = fl64(p + c) and TwoSum's residual e = (p + c) - s are exact.  s is the double nearest the true
    sum t, so t lies strictly on the same side of every double as s does - unless s IS that double: rounding s to float32 therefore equals
    rounding t, except where s sits exactly on a float32 tie (the midpoint of two neighbouring float32, a double) while t does not
    (e != 0); there the sign of e decides.  A double rounding is then impossible.  Proved against fractions.Fraction in
    tests/test_cost_geometry_cpu.py."""
    import numpy as np
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), np.asarray(c, dtype=np.float32))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        d = s - r64                                                           # exact: s and r agree in their leading bits
        other = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = (d != 0) & np.isfinite(s) & np.isfinite(other) & ((s - r64) == (other.astype(np.float64) - s))
        fix = tie & (e != 0)
        r = np.where(fix, np.where(e > 0, np.maximum(r, other), np.minimum(r, other)), r)
    return r.astype(np.float32)


def cost_coords32(Pij, D, incre, disp_in, shift, h, w, y0=0):
    """The source coordinates of every (view, pixel, hypothesis) of an h x w reference grid whose first image row is ``y0``, in numpy
    float32, operation for operation as the kernels and the reference form them:
      origin = disp_in, raised to lim = fl32((D // 2) * incre) under ``shift`` (core/corr.py:59-62) - equal to O.hypothesis_origin;
      hyp = fl(fl((k - D // 2) * fl32(incre)) + origin);
      a = fl(fma(m1, py, fl(m0 * px)) + m2), X = fma(m3, hyp, a), likewise Y (m4..m7) and Z (m8..m11), px = x, py = y + y0;
      u = X / Z, t = Y / Z (IEEE), ok = u == u and t == t, then both clamped to +-1e4 (fmaxf / fminf: a NaN becomes -1e4).
    Pij [V, 4, 4]; disp_in [h * w].  -> dict of numpy arrays: ok [V, P, D] bool; iu, iw int32 = floor(u), floor(t) (NOT clamped to the
    map: a texel outside the map is zero, which is what the kernels' clamp into the zero border computes; -2 where not ok); du, dw float32
    = u - floor(u), t - floor(t) (0 where not ok; the float32 difference, which can round to 1.0 just below an integer, as on the device);
    u, t (clamped), Z [V, P, D] float32; hyp [P, D]; origin [P]."""
    import numpy as np
    f32 = np.float32
    m = np.asarray(torch.as_tensor(Pij).detach().cpu().numpy(), dtype=f32).reshape(-1, 16)
    V, P = m.shape[0], h * w
    origin = np.asarray(torch.as_tensor(disp_in).detach().cpu().numpy(), dtype=f32).reshape(-1).copy()
    assert origin.size == P
    if shift:
        lim = f32((D // 2) * float(incre))
        origin = np.where(origin < lim, lim, origin).astype(f32)
    k = (np.arange(D) - D // 2).astype(f32)
    hyp = ((k * f32(incre)).astype(f32)[None, :] + origin[:, None]).astype(f32)
    px, py = (np.arange(P) % w).astype(f32), (np.arange(P) // w + y0).astype(f32)
    out = {key: np.empty((V, P, D), dtype=dt) for key, dt in (("ok", bool), ("iu", np.int32), ("iw", np.int32), ("du", f32), ("dw", f32),
                                                               ("u", f32), ("t", f32), ("Z", f32))}
    with np.errstate(all="ignore"):
        for v in range(V):
            def ray(r):
                a = (fma32(m[v, 4 * r + 1], py, (m[v, 4 * r] * px).astype(f32)) + m[v, 4 * r + 2]).astype(f32)
                return fma32(m[v, 4 * r + 3], hyp, a[:, None])
            X, Y, Z = ray(0), ray(1), ray(2)
            u, t = (X / Z).astype(f32), (Y / Z).astype(f32)
            ok = ~np.isnan(u) & ~np.isnan(t)
            u = np.fmin(np.fmax(u, f32(-1e4)), f32(1e4))
            t = np.fmin(np.fmax(t, f32(-1e4)), f32(1e4))
            fu, ft = np.floor(u), np.floor(t)
            out["ok"][v], out["u"][v], out["t"][v], out["Z"][v] = ok, u, t, Z
            out["du"][v], out["dw"][v] = np.where(ok, (u - fu).astype(f32), f32(0)), np.where(ok, (t - ft).astype(f32), f32(0))
            out["iu"][v], out["iw"][v] = np.where(ok, fu.astype(np.int32), -2), np.where(ok, ft.astype(np.int32), -2)
    out["hyp"], out["origin"] = hyp, origin
    return out


CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))                                    # (dy, dx) of a sample's four texels, in the order of ``dots``


def cost_f2_two_term(f2):
    """The two-term form's definition of a source row (tests/test_hip_parity.py::test_cost_lines_two_term_form): the kernel's operand is
    x * 2^6 split into f16 hi | lo, and the two-term form reads hi only."""
    return (f2.float() * 64.0).clamp(-65504.0, 65504.0).half().float() / 64.0


def cost_samples_ref64(f1, f2, coords, f2_round=None, views=None, chunk=1024):
    """The float64 value of every sample from the restated cells and fractions.  f1 [P, C]: the reference rows of the pixel grid of
    ``coords`` (as the kernels read them: fmaps / 8); f2 [V, h2, w2, C]: the source maps WITHOUT border (the size of the source map is
    theirs: a row slab's ``src_hw``); views: which source map each view of ``coords`` reads (default 0 .. V - 1: the ``slots``
    indirection is the caller's business - the reference is told what the kernel should have read).  The four weights are formed from the
    fp32 fractions in float64, (1 - du)(1 - dw) etc., exactly; a texel outside the source map is zero; a not-ok sample is zero.
    ``f2_round``: applied to the source maps first (``cost_f2_two_term``).
    -> dict of [V, P, D] float64 tensors: val; norm = sum_c |f1_c| * (bilinear-weighted |f2_c|), the convention of ``cost_volume_ref64``;
    l1 = sum_c |f1_c| + bilinear-weighted sum_c |f2_c| (what the absolute term of ``cost_bound`` scales with); and dots [V, P, D, 4], the
    texel dots of every sample in the order of CORNERS (zero outside the map), so that a failure can be attributed to a corner."""
    f1 = torch.as_tensor(f1).detach().cpu().double()
    f2 = torch.as_tensor(f2).detach().cpu()
    if f2_round is not None:
        f2 = f2_round(f2)
    f2 = f2.double()
    Vs, h2, w2, C = f2.shape
    V, P, D = coords["ok"].shape
    views = list(range(V)) if views is None else list(views)
    T = h2 * w2
    zero = torch.zeros(1, C, dtype=torch.float64)
    f1a, s1 = f1.abs(), f1.abs().sum(1)
    out = {k: torch.zeros(V, P, D, dtype=torch.float64) for k in ("val", "norm", "l1")}
    out["dots"] = torch.zeros(V, P, D, 4, dtype=torch.float64)
    tt = lambda a: torch.from_numpy(a)
    for v in range(V):
        f2z = torch.cat([f2[views[v]].reshape(T, C), zero], 0)
        f2za, s2 = f2z.abs(), f2z.abs().sum(1)
        for s in range(0, P, chunk):
            e = slice(s, s + chunk)
            ok, iu, iw = tt(coords["ok"][v, e]), tt(coords["iu"][v, e]).long(), tt(coords["iw"][v, e]).long()
            du, dw = tt(coords["du"][v, e]).double(), tt(coords["dw"][v, e]).double()
            for q, (dy, dx) in enumerate(CORNERS):
                wt = (du if dx else 1.0 - du) * (dw if dy else 1.0 - dw)
                xi, yi = iu + dx, iw + dy
                inside = ok & (xi >= 0) & (xi < w2) & (yi >= 0) & (yi < h2)
                idx = torch.where(inside, yi * w2 + xi, torch.full_like(xi, T))
                dots = torch.einsum("ndc,nc->nd", f2z[idx], f1[e])
                out["dots"][v, e, :, q] = dots
                out["val"][v, e] += wt * dots
                out["norm"][v, e] += wt * torch.einsum("ndc,nc->nd", f2za[idx], f1a[e])
                out["l1"][v, e] += wt * s2[idx]
            out["l1"][v, e] += s1[e, None] * ok
    return out


def cost_rows_ref64(per_view, D, num_levels, scale, compact, preset=None):
    """Volume rows from per-view samples (``cost_samples_ref64``): the view sum in view order, times ``scale`` (None: the plain sum), the
    pooled levels of O.pyramid ((a + b) / 2 pairwise, floor) unless ``compact`` or ``preset``; ``preset`` [P, rs]: accumulate - level 0 is
    preset + sum, every other column of the row stays what it was.  Laid out by ``ops.row_layout``.
    -> dict of [P, rs] float64: ref, norm, l1 (pad columns and, under ``preset``, the columns beyond level 0: ref = preset or 0, norm = l1
    = 0), and level [rs] (long): the pyramid level of a column, -1 for a column the builder does not write."""
    from cer_mvs_amd import ops
    offs, lens, rs = ops.row_layout(D, num_levels, compact)
    P = per_view["val"].shape[1]
    sc = 1.0 if scale is None else float(torch.tensor(float(scale), dtype=torch.float32))       # (the kernels take the scale as a C float)
    out = {k: torch.zeros(P, rs, dtype=torch.float64) for k in ("ref", "norm", "l1")}
    level = torch.full((rs,), -1, dtype=torch.long)
    if preset is not None:
        pre = torch.as_tensor(preset).detach().cpu().double()
        out["ref"] = pre.clone()
        out["norm"][:, :D] = pre[:, :D].abs()
    for k, src in (("ref", "val"), ("norm", "norm"), ("l1", "l1")):
        cur = per_view[src].sum(0) * sc
        out[k][:, :D] += cur
        if preset is not None:
            continue
        for l in range(1, 1 if compact else num_levels):
            n = cur.shape[1] // 2
            cur = (cur[:, 0:2 * n:2] + cur[:, 1:2 * n:2]) * 0.5
            out[k][:, offs[l]:offs[l] + lens[l]] = cur
    level[:D] = 0
    if preset is None and not compact:
        for l in range(1, num_levels):
            level[offs[l]:offs[l] + lens[l]] = l
    out["level"] = level
    return out


def _gamma(n):
    return n * U24 / (1.0 - n * U24)


COST_FORMS = ("walk", "three-term", "two-term")


def cost_bound(norm, V, form, level=0, accumulate=False, l1=None):
    """-> (c, abs_term): |kernel - reference| <= c * norm + abs_term for an element of a cost-volume row whose cell and fractions are the
    restated ones; u = 2^-24, gamma_n = n u / (1 - n u).  Every term is read off the kernel source; nothing is fitted to an output.

    walk (csrc/cost_build.hip, C = 64): a lane owns 4 channels of one corner: ``cer_dot4``, a chain of 4 fmaf from 0: 4 roundings.  Its
    corner weight: 1 - du and 1 - dw round once each (a single fp32 subtraction: relative u of its result), their product once: 3.
    ``acc = fmaf(sdot, wgt, acc)`` once per view: V.  The butterfly sums the 64 lanes in 6 levels of one add each: 6.  ``acc * scale``: 1.
    Every partial sum is bounded by the sum of the absolute terms, which is V * norm / scale: n = 14 + V.

    three-term (csrc/cost_lines.hip): the operand of both maps is x' = 64 x = hi + lo + d, hi = f16(x'), lo = f16(x' - hi):
    |d| <= 2^-11 |x' - hi| <= 2^-22 |x'| while lo is a normal f16, else |d| <= 2^-25 (half an f16 subnormal step; the same when hi itself
    is subnormal).  The kernel sums hi hi + hi lo + lo hi: it drops lo1 lo2 (<= 2^-22 |x1' x2'|) and inherits d1 x2' + d2 x1'
    (<= 2 * 2^-22 |x1' x2'| + 2^-25 (|x1'| + |x2'|)): relative 3 * 2^-22, absolute 2^-25 * 64 / 4096 = 2^-31 per unit of |x1| + |x2|,
    i.e. 2^-31 * l1.  The 12 MFMAs (v_mfma_f32_32x32x16_f16: f16 products are exact in fp32) add 192 products into one fp32 accumulator;
    the order inside an instruction is the hardware's, so each of the 192 additions is charged one rounding of a partial sum that is at
    most the whole sum of absolute terms: 192.  (The direct path - ``cl_direct`` - is a chain of 64 fmaf on (hi + lo) rounded once per
    operand: 66, inside the same figure, and drops nothing.)  Gather: the weight as above, 3; dot * weight, 1; three adds, 3.  View sum
    (cost_lines_reduce_kernel: s = 0 + part_0 + ...): V - 1; ``s * scale`` (a power of two folded in): 1.  n = 199 + V.

    two-term: judged against the reference on f16-rounded source rows (``cost_f2_two_term``: its definition, pinned bit for bit by
    test_cost_lines_two_term_form) with the three-term figure: its lo planes are exactly zero there, its 8 MFMAs a subset of the 12.

    Pooled level l (both epilogues and cer_pyramid_f32: (a + b) * 0.5f, level by level): the children's errors average into c * (pooled
    norm); the add rounds once and the halving is exact short of underflow - charged two per level.  Accumulate: one more rounding of
    preset + sum, relative to |preset| + norm - the caller adds |preset| to ``norm``.
    The factor 1 + 2^-10 covers the products of two error terms.  (The issue's own estimate, (C + 12 + V) u + 3 * 2^-22 ~ 5e-6, charges
    the MFMA chain one rounding per CHANNEL; per product, which is what the instruction's unspecified inner order allows, it is 1.3e-5.)"""
    if form not in COST_FORMS:
        raise ValueError(form)
    n = (14 + V if form == "walk" else 199 + V) + 2 * int(level) + int(bool(accumulate))
    split = 0.0 if form == "walk" else 3.0 * 2.0 ** -22
    c = (_gamma(n) + split) * (1.0 + 2.0 ** -10)
    a = 0.0 if (form == "walk" or l1 is None) else 2.0 ** -31 * (1.0 + 2.0 ** -10) * torch.as_tensor(l1, dtype=torch.float64)
    return c, a


def check_cost_rows(got, R, V, form, where, h, w, accumulate=False, floor=None):
    """``check_elementwise`` of volume rows ``got`` [P, rs] against ``R`` (``cost_rows_ref64``) on every column a builder writes: the
    norm floored at the case's mean |ref| (``floor``: that figure, when ``got`` is part of a larger case), c and the absolute term from
    ``cost_bound`` column by column (a pooled column has its level's c), 1 x 32 tiles and 32-pixel seams -> ParityReport (its
    ``channels`` are the row's columns)."""
    cols = (R["level"] >= 0).nonzero().reshape(-1)
    ref = R["ref"][:, cols]
    floor = float(ref.abs().mean()) if floor is None else floor
    c0, a = cost_bound(None, V, form, 0, accumulate, l1=R["l1"][:, cols])
    cl = torch.tensor([cost_bound(None, V, form, int(l), accumulate)[0] for l in R["level"][cols]], dtype=torch.float64)
    mag = R["norm"][:, cols].clamp_min(floor) * (cl / c0)[None, :]
    return check_elementwise(torch.as_tensor(got).detach().cpu().double()[:, cols], ref, mag, c0, a, where, h=h, w=w, tile=(1, 32), seam=32)


def assert_cost_rows(got, R, V, form, where, h, w, **kw):
    rep = check_cost_rows(got, R, V, form, where, h, w, **kw)
    assert rep.ok, rep.message()
    return rep
