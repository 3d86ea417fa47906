"""The float64 references of the training-row kernels (tests/parity_check.py: csrc/alt_corr.hip, csrc/train_ops.hip) and the inputs of
tests/test_train_parity_gpu.py, checked without a GPU:
  * every reference against float64 torch autograd at every shape the GPU module runs - grid_sample for the correlation, grid_sample +
    avg_pool2d for the lookup, grid_sample again for the upsample (all fed the fp32-formed coordinates, so the two sides choose their
    texels from the same numbers and agree to 1e-12; a coordinate that is not finite or beyond +-2e9 samples nothing on either side),
    and F.interpolate(align_corners=True) for the upsample (its source index is formed in float64 there and in fp32 here: bilinear
    weights are continuous in the source coordinate, so the two differ by at most |ds| times the local slope);
  * planted corruptions of a COPY of a reference output, each under the old global bar (rel_l1 < 1e-5) and each caught by
    check_elementwise under the bound the GPU module uses: the transposed tap index, a sample dropped from a 200-sample segment, the
    level fold without its odd-length guard, a range entry off by one;
  * cer_upsample_ac_ranges (host code) against the brute-force table, the lookup's argument checks, and the edge census of every GPU
    case.  CPU only."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import parity_check as pc
import train_parity_cases as tc
from conftest import rel_l1
from parity_check import U24, check_elementwise
from test_oracle_golden import hashed

TIGHT = 1e-12            # float64 against float64 on the same indices: |a - b| <= TIGHT * (mag + 1)


def close64(a, b, mag, what):
    bad = ~((a - b).abs() <= TIGHT * (mag + 1.0))
    assert not bool(bad.any()), (what, int(bad.sum()), float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ references against autograd
def _corr_autograd(f1, f2, coords, g, r):
    """corr, d/df1, d/df2 of the grid_sample form (oracle.cer_oracle.alt_corr_forward, one shifted sample per channel) in float64."""
    B, H1, W1, C = f1.shape
    _, H2, W2, _ = f2.shape
    N, rd = coords.shape[1], 2 * r + 1
    a = f1.double().requires_grad_(True)
    b = f2.double().requires_grad_(True)
    finite, fx, fy, dx, dy = pc._corr_floor(coords)
    # floor + fl32(x - floor): the fraction the kernel (and the reference's CUDA) forms in fp32 - exact except for -1 < x < 0, where the
    # difference needs more bits than x has and rounds once
    xy = torch.stack([fx.double() + dx, fy.double() + dy], -1)
    dead = ~finite | (xy.abs() > 2.0e9).any(-1)
    xy = torch.where(dead[..., None], torch.full_like(xy, -100.0), xy)        # far outside the map: samples nothing
    img = b.permute(0, 3, 1, 2)
    chans = [None] * (rd * rd)
    for kx in range(rd):
        for ky in range(rd):
            gx = 2 * (xy[..., 0] + (kx - r)) / (W2 - 1) - 1
            gy = 2 * (xy[..., 1] + (ky - r)) / (H2 - 1) - 1
            s = F.grid_sample(img, torch.stack([gx, gy], -1).view(B, N * H1, W1, 2), align_corners=True)       # [B,C,N*H1,W1]
            chans[ky + rd * kx] = (s.view(B, C, N, H1, W1) * a.permute(0, 3, 1, 2)[:, :, None]).sum(1)
    corr = torch.stack(chans, 2)
    (corr * g.double()).sum().backward()
    return corr.detach(), a.grad, b.grad


@pytest.mark.parametrize("C,r", tc.CORR_CASES)
def test_correlation_references_match_autograd(C, r):
    f1, f2, coords, g = tc.corr_case(C, r)
    corr, g1, g2 = _corr_autograd(f1, f2, coords, g, r)
    ref, mag = pc.alt_corr_ref64(f1, f2, coords, r)
    close64(ref, corr, mag, "corr")
    r1, m1, n1, r2, m2, n2, keys, coef, src = pc.alt_corr_adjoint_ref64(f1, f2, coords, g, r)
    close64(r1, g1, m1, "fmap1 gradient")
    close64(r2, g2, m2, "fmap2 gradient")
    B, N, P1, T, fp = 2, 3, 117, 77, (2 * r + 2) ** 2
    assert keys.shape == coef.shape == src.shape == (B * N * P1 * fp,) and keys.dtype == torch.int64 and src.dtype == torch.int32
    assert int(keys.max()) == B * T and int((keys == B * T).sum()) > 0 and bool((coef[keys == B * T] == 0).all())
    assert int(n2.sum()) == int((keys < B * T).sum()) == int(n1.sum()) and int(n1.max()) <= N * fp
    assert bool((r2[n2 == 0] == 0).all()) and bool((m2[n2 == 0] == 0).all())


def _lookup_autograd(vol, origin, disp, gout, D, L, r):
    V, _, P = vol.shape
    v = vol.double().requires_grad_(True)
    c = pc.tl_coord32(origin, disp, D, tc.LOOKUP_INCRE)
    lvl = v.permute(0, 2, 1).reshape(V * P, 1, 1, D)
    outs = []
    for lv in range(L):
        if lv:
            lvl = F.avg_pool2d(lvl, [1, 2], stride=[1, 2])
        n = lvl.shape[-1]
        x = torch.stack([float(j - r) + c / float(1 << lv) for j in range(2 * r + 1)], -1)                # [P, taps], formed in fp32
        x = torch.floor(x).double() + (x - torch.floor(x)).double()            # floor + fl32(x - floor): one rounding for -1 < x < 0
        grid = torch.stack([2 * x / (n - 1) - 1, torch.zeros_like(x)], -1).repeat(V, 1, 1).view(V * P, 1, 2 * r + 1, 2)
        outs.append(F.grid_sample(lvl, grid, align_corners=True).view(V, P, 2 * r + 1))
    out = torch.cat(outs, -1).permute(0, 2, 1)
    (out * gout.double()).sum().backward()
    return out.detach(), v.grad


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("D,L,r,P", tc.LOOKUP_CASES)
def test_lookup_references_match_autograd(D, L, r, P, shift):
    vol, origin, disp, gout = tc.lookup_case(D, L, r, P, shift)
    out, grad = _lookup_autograd(vol, origin, disp, gout, D, L, r)
    ref, mag = pc.train_lookup_ref64(vol, origin, disp, D, tc.LOOKUP_INCRE, L, r)
    close64(ref, out, mag, "lookup")
    gref, gmag, n = pc.train_lookup_adjoint_ref64(gout, origin, disp, D, tc.LOOKUP_INCRE, L, r)
    close64(gref, grad, gmag, "lookup adjoint")
    assert n.shape == (D, P) and int(n.max()) <= 2 * L + (L - 1)              # two taps per cell and level, one fold per level


def _upsample_source32(n_in, n_out):
    """The source coordinate the kernel forms, fl32(fl32((in-1) / (out-1)) * dst), as float64, and its grid_sample coordinate."""
    i0, _, _, l1 = pc.upsample_ac_taps(n_in, n_out)
    s = i0.double() + l1                                                           # (int) s + (s - (int) s): exact
    return s, (2 * s / (n_in - 1) - 1 if n_in > 1 else torch.zeros_like(s))


@pytest.mark.parametrize("n,h,w,H,W", tc.UPSAMPLE_CASES)
def test_upsample_references_match_interpolate(n, h, w, H, W):
    """Two float64 autograd forms.  grid_sample fed the fp32-formed source coordinates (padding_mode="border": a coordinate an ulp past
    the last texel reads the last texel, as the kernel's clamped i1 does) picks its texels and weights from the same numbers as the
    reference: every element of the forward and of the adjoint to 1e-12.  F.interpolate(align_corners=True) forms its source index in
    float64: where the two indices pick different texels, and everywhere else too, it can only be compared up to the continuity of the
    bilinear weights in the source coordinate."""
    x, g = tc.upsample_case(n, h, w, H, W)
    ref, mag = pc.upsample_ac_ref64(x, H, W)
    grad, gmag, cnt, (ry, rx) = pc.upsample_ac_adjoint_ref64(g, h, w)
    xt = x.double().requires_grad_(True)
    (sy, gy), (sx, gx) = _upsample_source32(h, H), _upsample_source32(w, W)
    grid = torch.stack([gx.view(1, W).expand(H, W), gy.view(H, 1).expand(H, W)], -1)[None].expand(n, H, W, 2)
    same = F.grid_sample(xt[:, None], grid, mode="bilinear", padding_mode="border", align_corners=True)[:, 0]
    (same * g.double()).sum().backward()
    close64(ref, same.detach(), mag, "upsample")
    close64(grad, xt.grad, gmag, "upsample adjoint")
    xt = x.double().requires_grad_(True)
    want = F.interpolate(xt[:, None], [H, W], mode="bilinear", align_corners=True)[:, 0]
    (want * g.double()).sum().backward()
    # |s32 - s64| <= 2 u s (the scale's rounding and the product's) <= 2 u (in - 1) per axis; a bilinear weight has slope 1 in s, so a
    # value moves by at most that times the two texel magnitudes it blends: sum over both axes, times 2 max|x| (max|g| for the adjoint)
    ds = 2 * U24 * (max(h - 1, 0) + max(w - 1, 0))
    assert float((ref - want.detach()).abs().max()) <= ds * 2 * float(x.abs().max()) + TIGHT
    ny, nx = (ry[:, 1] - ry[:, 0]).double() + 2, (rx[:, 1] - rx[:, 0]).double() + 2          # outputs that may hold the texel, either index form
    assert bool(((grad - xt.grad).abs() <= ds * float(g.abs().max()) * ny[:, None] * nx[None, :] + TIGHT).all())
    assert bool((grad[:, (ry[:, 0] == ry[:, 1])] == 0).all()) and bool((grad[:, :, (rx[:, 0] == rx[:, 1])] == 0).all())
    if (h, w) == (H, W):
        assert torch.equal(ref, x.double()) and torch.equal(grad, g.double())


# ------------------------------------------------------------------------------------------------ planted corruptions
BIG = dict(B=1, N=8, H1=160, W1=160, H2=128, W2=128, C=8, r=1)


@pytest.fixture(scope="module")
def big_corr():
    """A correlation adjoint in which ONE wrong sample stays under rel_l1 = 1e-5: 204 800 samples with positive features and gradients
    (no cancellation: a sample is 1 / 204 800 of a gradient's mass), spread over 128 x 128 texels so that a texel's segment has about
    200 samples (204 800 x 16 / 16 384).  C = 8: the reference takes any width."""
    B, N, H1, W1, H2, W2, C, r = (BIG[k] for k in ("B", "N", "H1", "W1", "H2", "W2", "C", "r"))
    f1, f2 = hashed((B, H1, W1, C), 7701, 0.1, 1.0), hashed((B, H2, W2, C), 7702, 0.1, 1.0)
    g = hashed((B, N, 9, H1, W1), 7703, 0.1, 1.0)
    xy = torch.stack([hashed((B, N, H1, W1), 7704, -3.0, W2 + 2.0), hashed((B, N, H1, W1), 7705, -3.0, H2 + 2.0)], -1).contiguous()
    return f1, f2, xy, g, pc.alt_corr_adjoint_ref64(f1, f2, xy, g, r)


def _one_sample(f1, f2, xy, g, n, y, x, transposed=False):
    """The adjoint of the gradient of ONE sample (the operator is linear in g): what that sample adds to g1 and g2.  ``transposed``:
    the sample's gradient channels permuted ky + rd kx <-> kx + rd ky before the (unmodified) reference gathers them, which is what a
    kernel reading gp[(ix-1) + rd (iy-1)] in place of gp[(iy-1) + rd (ix-1)] computes."""
    rd = 2 * BIG["r"] + 1
    gs = torch.zeros_like(g[:, n:n + 1])
    gv = g[0, n, :, y, x]
    gs[0, 0, :, y, x] = gv.view(rd, rd).t().reshape(-1) if transposed else gv
    out = pc.alt_corr_adjoint_ref64(f1, f2, xy[:, n:n + 1], gs, BIG["r"])
    return out[0], out[3]


def test_transposed_tap_index_is_invisible_to_rel_l1_and_caught_elementwise(big_corr):
    """One sample gathers with (ix-1) + rd (iy-1) instead of (iy-1) + rd (ix-1): both gradients stay under rel_l1 = 1e-5 and both fail
    element-wise, at the sample's pixel (fmap1) and inside its footprint (fmap2)."""
    f1, f2, xy, g, (g1, m1, n1, g2, m2, n2, _, _, _) = big_corr
    B, N, H1, W1, H2, W2, C, r = (BIG[k] for k in ("B", "N", "H1", "W1", "H2", "W2", "C", "r"))
    n, y, x = 2, 77, 31
    fx, fy = int(torch.floor(xy[0, n, y, x, 0])), int(torch.floor(xy[0, n, y, x, 1]))
    assert 2 <= fx < W2 - 3 and 2 <= fy < H2 - 3                             # the whole footprint lies inside the map
    good, bad = _one_sample(f1, f2, xy, g, n, y, x), _one_sample(f1, f2, xy, g, n, y, x, transposed=True)
    got1, got2 = g1 - good[0] + bad[0], g2 - good[1] + bad[1]
    assert 0 < rel_l1(got1, g1) < 1e-5 and 0 < rel_l1(got2, g2) < 1e-5
    rep = check_elementwise(got1[0].reshape(-1, C), g1[0].reshape(-1, C), m1[0].reshape(-1, C), (N * 16 + pc.K_COEF) * U24, where="g1", h=H1, w=W1)
    assert not rep.ok and set(rep.pixels.tolist()) == {y * W1 + x}
    bound2 = (n2[0].reshape(-1, 1).double() + pc.K_COEF) * U24 * m2[0].reshape(-1, C)
    rep = check_elementwise(got2[0].reshape(-1, C), g2[0].reshape(-1, C), bound2, 1.0, where="g2", h=H2, w=W2)
    assert not rep.ok and set(rep.rows) <= set(range(fy - 1, fy + 3)) and set(rep.cols) <= set(range(fx - 1, fx + 3))
    assert check_elementwise(g2[0].reshape(-1, C).float(), g2[0].reshape(-1, C), bound2, 1.0, where="clean", h=H2, w=W2).ok


def test_dropped_sample_of_a_long_segment_is_invisible_to_rel_l1_and_caught_elementwise(big_corr):
    """One sample of a texel whose segment has 200 or more is left out of the fmap2 gradient: 1 / 200 of that texel, 5e-6 of the whole."""
    f1, f2, xy, g, (g1, m1, n1, g2, m2, n2, keys, coef, _) = big_corr
    N, H1, W1, H2, W2, C = (BIG[k] for k in ("N", "H1", "W1", "H2", "W2", "C"))
    seg = n2[0].reshape(-1)
    t = int(((seg >= 200) & (seg <= 230)).nonzero()[0])                           # a texel with a segment of 200 .. 230 samples
    tup = int(((keys == t) & (coef > 0.05)).nonzero()[0])                         # a sample that gives it more than a sliver
    s = tup // 16
    n, y, x = s // (H1 * W1), (s % (H1 * W1)) // W1, s % W1
    got2 = g2 - _one_sample(f1, f2, xy, g, n, y, x)[1]
    assert 0 < rel_l1(got2, g2) < 1e-5
    bound2 = (seg.reshape(-1, 1).double() + pc.K_COEF) * U24 * m2[0].reshape(-1, C)
    rep = check_elementwise(got2[0].reshape(-1, C), g2[0].reshape(-1, C), bound2, 1.0, where="g2", h=H2, w=W2)
    assert not rep.ok and t in set(rep.pixels.tolist()) and len(set(rep.pixels.tolist())) <= 16
    assert set(rep.rows) <= set(range(t // W2 - 3, t // W2 + 4)) and set(rep.cols) <= set(range(t % W2 - 3, t % W2 + 4))


def test_level_fold_without_its_guard_is_invisible_to_rel_l1_and_caught_elementwise():
    """D = 45, three levels (45 | 22 | 11): element 44 of level 0 has no partner in level 1 (44 >> 1 = 22 = its length); without the
    guard `i < len` the fold reads the next slot of the row, which is element 0 of level 2.  That slot is non-zero only for a pixel
    whose taps reach the start of level 2 (c / 4 - r < 1): one pixel of 8192 here."""
    V, D, L, r, P = 1, 45, 3, 5, 8192
    origin = hashed((P,), 8801, 0.001, 0.002)
    disp = origin + hashed((P,), 8802, 6.0, 30.0) * tc.LOOKUP_INCRE          # c in [28, 52]: no tap near the start of level 2
    disp[4097] = origin[4097] - 12.5 * tc.LOOKUP_INCRE                            # c = 9.5
    gout = hashed((V, L * (2 * r + 1), P), 8803)
    ref, mag, n = pc.train_lookup_adjoint_ref64(gout, origin, disp, D, tc.LOOKUP_INCRE, L, r)
    accs = pc.train_lookup_level_adjoints64(gout, origin, disp, D, tc.LOOKUP_INCRE, L, r)
    got = ref.clone()
    got[:, D - 1] += accs[2][0][:, 0] * 0.5                                        # what row[off[1] + 22] * 0.5 adds
    assert int((accs[2][0][0, 0] != 0).sum()) == 1
    assert 0 < rel_l1(got, ref) < 1e-5
    rep = check_elementwise(got[0].T, ref[0].T, mag[0].T, (2 * r + 1 + L + 3) * U24, where="lookup adjoint", h=1, w=P, tile=(1, 64))
    assert not rep.ok and rep.pixels.tolist() == [4097] and rep.channels == {D - 1: 1}


def test_range_entry_off_by_one_is_invisible_to_rel_l1_and_caught_elementwise():
    """The x pass of the upsample adjoint at 400 -> 1600 with the range of ONE texel one output short: the texel loses its last and
    lightest term in every row.  The texel is the one whose lost weight is smallest (not zero): the hardest entry to see."""
    w, W, rows = 400, 1600, 64
    g = hashed((1, rows, W), 9901)
    ref, mag, n, table = pc.upsample_ac_adjoint_pass64(g, w, 2)
    assert torch.equal(n, (table[:, 1] - table[:, 0]).long())                     # the bound's n is the range length
    i0, i1, l0, l1 = pc.upsample_ac_taps(w, W)
    last = (table[:, 1] - 1).long()                                               # the last output of every texel's range
    lost = torch.where(i0[last] == torch.arange(w), l0[last], l1[last])
    lost = torch.where(lost > 0, lost, torch.full_like(lost, 2.0))
    j = int(torch.argmin(lost))
    assert 0 < float(lost[j]) < 2e-3
    got = ref.clone()
    got[:, :, j] -= float(lost[j]) * g[:, :, int(last[j])].double()
    assert 0 < rel_l1(got, ref) < 1e-5
    bound = (n.double() + 2).view(1, w) * U24 * mag[0]
    rep = check_elementwise(got[0].reshape(-1, 1), ref[0].reshape(-1, 1), bound.reshape(-1, 1), 1.0, where="x pass", h=rows, w=w)
    assert not rep.ok and set(rep.cols) == {j} and rep.n_fail > rows // 2
    assert check_elementwise(ref[0].reshape(-1, 1).float(), ref[0].reshape(-1, 1), bound.reshape(-1, 1), 1.0, where="clean", h=rows, w=w).ok


# ------------------------------------------------------------------------------------------------ host code
def _lib_ranges(lib, n_in, n_out):
    buf = (ctypes.c_int * (2 * n_in))()
    assert lib.cer_upsample_ac_ranges(n_in, n_out, buf) == 0
    return torch.tensor(list(buf), dtype=torch.int32).view(n_in, 2)


def test_upsample_range_table_matches_brute_force():
    from cer_mvs_amd import _lib
    lib = _lib.load()
    sizes = [(i, o) for i in range(1, 41) for o in range(1, 41)] + [(296, 1184), (400, 1600), (128, 512), (160, 640)]
    for n_in, n_out in sizes:
        assert torch.equal(_lib_ranges(lib, n_in, n_out), pc.upsample_ranges_brute(n_in, n_out)), (n_in, n_out)
    assert lib.cer_upsample_ac_ranges(0, 4, (ctypes.c_int * 2)()) == -1 and lib.cer_upsample_ac_ranges(4, 4, None) == -1


def test_lookup_argument_checks_without_device():
    from cer_mvs_amd import _lib
    lib = _lib.load()
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(0x1000)
    inc = tc.LOOKUP_INCRE
    for fn in (lib.cer_train_lookup_fwd_f32, lib.cer_train_lookup_bwd_f32):
        assert fn(fake, fake, fake, fake, 3, 273, 129, inc, 3, 5, null) == -2         # D > 128
        assert fn(fake, fake, fake, fake, 3, 273, 64, inc, 5, 1, null) == -2          # L > 4
        assert fn(fake, fake, fake, fake, 3, 273, 7, inc, 3, 1, null) == -2           # 7 >> 2 = 1: a level of one element
        assert fn(fake, fake, fake, fake, 3, 273, 64, inc, 1, 32, null) == -2         # L (2r + 1) = 65 taps
        assert fn(fake, fake, fake, fake, 3, 273, 64, 0.0, 3, 5, null) == -1          # incre = 0
        assert fn(null, fake, fake, fake, 3, 273, 64, inc, 3, 5, null) == -1
    assert b"CER_ESHAPE" in lib.cer_error_string(-2) and b"CER_EINVAL" in lib.cer_error_string(-1)


# ------------------------------------------------------------------------------------------------ edge census of the GPU cases
@pytest.mark.parametrize("C,r", tc.CORR_CASES)
def test_correlation_case_census(C, r):
    f1, f2, coords, g = tc.corr_case(C, r)
    n2 = pc.alt_corr_adjoint_ref64(f1[..., :1], f2[..., :1], coords, g, r)[5]
    tc.assert_corr_census(tc.corr_census(coords, r, n2))
    assert int(n2[0, 0, 0]) == 0 and int(n2[1, 0, 0]) == 0 and int(n2[:, 5, 3].min()) >= 100
    assert (9 * 13) % 16 and (11 * 7) % 16                                         # partial 16-lane groups in both kernels


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("D,L,r,P", tc.LOOKUP_CASES)
def test_lookup_case_census(D, L, r, P, shift):
    vol, origin, disp, gout = tc.lookup_case(D, L, r, P, shift)
    tc.assert_lookup_census(tc.lookup_census(origin, disp, D, L, r), D, L, P)


def test_upsample_case_census():
    cens = {case: tc.upsample_census(*case[1:]) for case in tc.UPSAMPLE_CASES}
    assert cens == tc.UPSAMPLE_CENSUS
    assert cens[(1, 40, 50, 7, 9)]["empty_rows"] > 0 and cens[(1, 40, 50, 7, 9)]["empty_cols"] > 0
    assert cens[(2, 1, 7, 5, 30)]["one_texel_axis"] == (True, False) and cens[(2, 6, 1, 9, 1)]["one_texel_axis"] == (False, True)
    assert cens[(2, 6, 1, 9, 1)]["one_output_axis"] == (False, True)
    assert cens[(2, 9, 11, 9, 11)]["identity"] and sum(c["identity"] for c in cens.values()) == 1
    # the largest legal lookup launch: 64 rows of 241 floats of LDS, just under 64 KiB
    pitch = sum(128 >> lv for lv in range(4)) | 1
    assert pitch == 241 and 64 * pitch * 4 == 61696 < 65536
