"""Element-wise parity checking at production shapes: helpers shared by tests/test_parity_check_cpu.py (which proves on planted
corruptions that the checker sees what a global mean cannot) and tests/test_fullsize_parity_gpu.py (which applies it to the HIP
kernels of one GRU iteration and to the cost volume).  Plain module, no fixtures.

Conventions: an image tensor is pixel-major, ``[h*w, C]`` or ``[h*w]``; a *tile* is a (rows, columns) block of pixels - 8 x 16 by
default, the smallest tile the s16 convolutions launch (16 x 16 for the tall ones); a *seam* is the border between two 32-pixel
segments of the epipolar-line kernel (csrc/cost_lines.hip: tiles of 32 pixels along the tile axis of a view)."""
import math

import torch

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
