"""Element-wise float64 parity of the training-row kernels, one launch at a time: csrc/alt_corr.hip (forward, atomic
backward, tuples, sorted reduction, and ops.alt_corr_backward end to end in both forms) and csrc/train_ops.hip (train lookup and its
adjoint, the loss's upsample, its x pass into `work` and its y pass).  Every launch goes through the C ABI into buffers this module
owns, filled with NaN sentinels first (assert_covered: no sentinel may be left), and every output element is compared with the float64
reference of that one kernel (tests/parity_check.py) under |err| <= c * mag, u = 2^-24, none of the constants fitted to an output:
  correlation forward   c = 1e-6 (C_CONV, the project's fp32-dot constant);
  tuple coefficient     c = 8 u (K_COEF: (g * wy) * wx with a rounded 1 - d is 4 roundings, adding four terms 3, second order 1);
  fmap1 gradient        c = (N (rd+1)^2 + K_COEF) u: one fma per (sample, footprint texel);
  fmap2 gradient        c = (n_t + K_COEF) u, n_t the texel's segment length (sorted form: n_t fmas; atomic form: a product and n_t - 1 adds);
  lookup forward        c = (4 + level) u: 1 - w, two products, one add; a pooled level carries one rounding per level;
  lookup adjoint        c = (taps + L + 3) u;
  upsample forward      c = 7 u (K_UP_FWD: six roundings on the longest path of the blend, second order 1);
  upsample x / y pass   c = (n + 2) u, n the length of the texel's range (per term 1 - l1 and a product, n - 1 adds, one to spare); the
                        y pass against the kernel's own `work`, read back.
The shapes are the smallest that reach each branch (partial 16-lane groups, C = 64 .. 256, H2 x W2 != H1 x W1, B = 2, empty and
100-sample segments, non-finite and huge coordinates; odd level lengths, the 61.7 KB launch, P of one partial block; empty ranges,
w = 1, W = 1, the identity size); tests/test_train_parity_cpu.py checks the references and the edge census of these inputs without a GPU.

Measured on an MI355X (profiles/train_parity.json, written only under CER_PARITY_RECORD=1 and only by a run of the whole module), max /
99.9th-percentile |err| / bound - the maximum over all cases, the percentile the largest among the cases of at least 1000 elements (a
smaller case has none apart from its maximum):
correlation forward 0.05 / 0.04; tuple coefficient 0.40 / 0.26; fmap1 gradient 0.23 / 0.14; fmap2 gradient, atomic 0.28 / 0.20;
fmap2 gradient, sorted 0.21 / 0.18; lookup forward 0.50 / 0.36; lookup adjoint 0.19 / 0.14; upsample forward 0.39 / 0.31; x pass
0.33 / 0.23; y pass 0.27 / 0.22 (ops.alt_corr_backward end to end: the same figures)."""
import json
import os
import warnings

import pytest
import torch

import parity_check as pc
import train_parity_cases as tc
from conftest import REPO
from parity_check import U24, assert_covered_batch, check_batch, poison_f32

pytestmark = pytest.mark.gpu
RECORD = {}                                            # figures for profiles/train_parity.json (written only with CER_PARITY_RECORD)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _expected_cases():
    """How many cases feed each figure when the whole module runs."""
    nc, nl, nu = len(tc.CORR_CASES), 2 * len(tc.LOOKUP_CASES), len(tc.UPSAMPLE_CASES)
    corr = ["alt_corr forward", "alt_corr tuples coef", "alt_corr reduce fmap2_grad"]
    corr += [k + g for k in ("alt_corr backward (atomic)", "ops.alt_corr_backward (sorted)", "ops.alt_corr_backward (atomic)")
             for g in (" fmap1_grad", " fmap2_grad")]
    up = ["upsample forward", "upsample adjoint x pass", "upsample adjoint y pass"]
    return {**{k: nc for k in corr}, "train_lookup forward": nl, "train_lookup adjoint": nl, **{k: nu for k in up}}


@pytest.fixture(scope="module", autouse=True)
def _record(dev):
    """The measured figures are written out only when CER_PARITY_RECORD asks for it, and only by a run of the whole module: a partial run
    (-k, one parametrisation, a failure on the way) would replace the profile with the figures of the cases that happened to run."""
    yield
    target = os.environ.get("CER_PARITY_RECORD", "")
    if not target:
        return
    if {k: v["cases"] for k, v in RECORD.items()} != _expected_cases():
        warnings.warn("CER_PARITY_RECORD: not every case of the module ran; the profile is left as it was")
        return
    path = os.path.join(REPO, "profiles", "train_parity.json") if target == "1" else target
    with open(path, "w") as f:
        json.dump(RECORD, f, indent=1, sort_keys=True)
        f.write("\n")


P999_MIN = 1000                                        # a case with fewer elements has no 99.9th percentile apart from its maximum


def compare(name, got, ref, bound, h, w, tile):
    """No sentinel left, every element of ``got`` [N, h*w, C] within ``bound`` of ``ref``.  RECORD[name]: ``max_ratio`` the largest
    |err| / bound over all cases, ``p999_ratio`` the largest per-case 99.9th percentile among the cases of at least P999_MIN elements."""
    assert_covered_batch(got, name, h, w, tile=tile)
    res = check_batch(got, ref, bound, 1.0, where=name, h=h, w=w, tile=tile)
    cur = RECORD.setdefault(name, {"max_ratio": 0.0, "p999_ratio": 0.0, "cases": 0})
    cur["max_ratio"], cur["cases"] = max(cur["max_ratio"], res["max_ratio"]), cur["cases"] + 1
    if got.numel() >= P999_MIN:
        cur["p999_ratio"] = max(cur["p999_ratio"], res["p999_ratio"])


def _lib():
    from cer_mvs_amd import _lib as L
    return L, L.load()


def nan_buf(dev, *shape):
    return poison_f32(torch.empty(*shape, device=dev, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ correlation
_CORR = {}


def corr_reference(C, r):
    """The case's inputs and float64 references, computed once and shared by the tests of the case (never modified)."""
    if (C, r) not in _CORR:
        f1, f2, coords, g = tc.corr_case(C, r)
        H2, W2 = f2.shape[1:3]
        fwd = pc.alt_corr_ref64(f1, f2, coords, r)
        adj = pc.alt_corr_adjoint_ref64(f1, f2, coords, g, r)
        cmag = pc.alt_corr_tuples_ref64(coords, g, r, H2, W2)[2].reshape(-1)
        tc.assert_corr_census(tc.corr_census(coords, r, adj[5]))
        _CORR[(C, r)] = ((f1, f2, coords, g), fwd, adj, cmag)
    return _CORR[(C, r)]


def corr_gradient_checks(name, g1, g2, gc, adj, N, r):
    r1, m1, n1, r2, m2, n2 = adj[:6]
    B, H1, W1, C = r1.shape
    _, H2, W2, _ = r2.shape
    c1 = (N * (2 * r + 2) ** 2 + pc.K_COEF) * U24
    compare(name + " fmap1_grad", g1.view(B, H1 * W1, C), r1.view(B, H1 * W1, C), c1 * m1.view(B, H1 * W1, C), H1, W1, (1, 16))
    b2 = (n2.double().view(B, H2 * W2, 1) + pc.K_COEF) * U24 * m2.view(B, H2 * W2, C)
    compare(name + " fmap2_grad", g2.view(B, H2 * W2, C), r2.view(B, H2 * W2, C), b2, H2, W2, (1, 16))
    assert bool((g2.cpu()[n2 == 0] == 0).all())                               # a texel nobody samples receives zeros
    if gc is not None:
        assert float(gc.abs().max()) == 0.0                                   # the reference never writes coords_grad


@pytest.mark.parametrize("C,r", tc.CORR_CASES)
def test_correlation_forward_and_atomic_backward(dev, C, r):
    L, lib = _lib()
    (f1, f2, coords, g), (ref, mag), adj, _ = corr_reference(C, r)
    B, H1, W1, _ = f1.shape
    _, H2, W2, _ = f2.shape
    N, K, P1 = coords.shape[1], (2 * r + 1) ** 2, H1 * W1
    a, b, xy, gd = f1.to(dev), f2.to(dev), coords.to(dev), g.to(dev)
    out = nan_buf(dev, B, N, K, H1, W1)
    L.check(lib.cer_alt_corr_forward_f32(L.dev_ptr(a, "f1"), L.dev_ptr(b, "f2"), L.dev_ptr(xy, "xy"), L.dev_ptr(out, "out"), B, N, H1, W1, H2, W2,
                                         C, r, L.cur_stream()), "forward")
    pm = lambda t: t.reshape(B, N * K, P1).permute(0, 2, 1)
    compare("alt_corr forward", pm(out.cpu()), pm(ref), pc.C_CONV * pm(mag), H1, W1, (1, 16))
    g1, g2, gc = nan_buf(dev, B, H1, W1, C), nan_buf(dev, B, H2, W2, C), nan_buf(dev, B, N, H1, W1, 2)
    L.check(lib.cer_alt_corr_backward_f32(L.dev_ptr(a, "f1"), L.dev_ptr(b, "f2"), L.dev_ptr(xy, "xy"), L.dev_ptr(gd, "g"), L.dev_ptr(g1, "g1"),
                                          L.dev_ptr(g2, "g2"), L.dev_ptr(gc, "gc"), B, N, H1, W1, H2, W2, C, r, L.cur_stream()), "backward")
    corr_gradient_checks("alt_corr backward (atomic)", g1.cpu(), g2.cpu(), gc.cpu(), adj, N, r)


@pytest.mark.parametrize("C,r", tc.CORR_CASES)
def test_correlation_tuples_and_sorted_reduction(dev, C, r):
    L, lib = _lib()
    (f1, f2, coords, g), _, adj, cmag = corr_reference(C, r)
    r2, m2, n2, keys_ref, coef_ref, src_ref = adj[3:]
    B, H1, W1, _ = f1.shape
    _, H2, W2, _ = f2.shape
    N, T = coords.shape[1], B * H2 * W2
    n = keys_ref.numel()
    a, xy, gd = f1.to(dev), coords.to(dev), g.to(dev)
    keys = torch.full((n,), -7, device=dev, dtype=torch.int64)
    src = torch.full((n,), -7, device=dev, dtype=torch.int32)
    coef = nan_buf(dev, n)
    L.check(lib.cer_alt_corr_bwd_tuples_f32(L.dev_ptr(xy, "xy"), L.dev_ptr(gd, "g"), L.dev_ptr(keys, "keys", torch.int64), L.dev_ptr(coef, "coef"),
                                            L.dev_ptr(src, "src", torch.int32), B, N, H1, W1, H2, W2, r, L.cur_stream()), "tuples")
    assert torch.equal(keys.cpu(), keys_ref) and torch.equal(src.cpu(), src_ref)
    fp = (2 * r + 2) ** 2
    S = n // fp
    compare("alt_corr tuples coef", coef.cpu().view(1, S, fp), coef_ref.view(1, S, fp), pc.K_COEF * U24 * cmag.view(1, S, fp), 1, S, (1, 256))
    skeys, order = torch.sort(keys, stable=True)
    seg = torch.searchsorted(skeys, torch.arange(T + 1, device=dev, dtype=torch.int64)).contiguous()
    assert torch.equal((seg[1:] - seg[:-1]).cpu(), n2.reshape(-1))
    runs = []
    for _ in range(3):
        g2 = nan_buf(dev, B, H2, W2, C)
        L.check(lib.cer_alt_corr_bwd_reduce_f32(L.dev_ptr(a, "f1"), L.dev_ptr(order.contiguous(), "order", torch.int64), L.dev_ptr(coef, "coef"),
                                                L.dev_ptr(src, "src", torch.int32), L.dev_ptr(seg, "seg", torch.int64), L.dev_ptr(g2, "g2"), T, C,
                                                L.cur_stream()), "reduce")
        runs.append(g2.cpu())
    b2 = (n2.double().view(B, H2 * W2, 1) + pc.K_COEF) * U24 * m2.view(B, H2 * W2, C)
    compare("alt_corr reduce fmap2_grad", runs[0].view(B, H2 * W2, C), r2.view(B, H2 * W2, C), b2, H2, W2, (1, 16))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert bool((runs[0][n2 == 0] == 0).all())


@pytest.mark.parametrize("C,r", tc.CORR_CASES)
def test_alt_corr_backward_end_to_end_in_both_forms(dev, C, r):
    """ops.alt_corr_backward: the per-view slicing of the deterministic path (B = 2 views) and the one-call atomic form."""
    from cer_mvs_amd import ops
    (f1, f2, coords, g), _, adj, _ = corr_reference(C, r)
    N = coords.shape[1]
    a, b, xy, gd = f1.to(dev), f2.to(dev), coords.to(dev), g.to(dev)
    runs = [ops.alt_corr_backward(a, b, xy, gd, r, deterministic=True) for _ in range(3)]
    corr_gradient_checks("ops.alt_corr_backward (sorted)", runs[0][0].cpu(), runs[0][1].cpu(), runs[0][2].cpu(), adj, N, r)
    assert all(torch.equal(runs[0][0], x[0]) and torch.equal(runs[0][1], x[1]) for x in runs[1:])
    g1, g2, gc = ops.alt_corr_backward(a, b, xy, gd, r, deterministic=False)
    corr_gradient_checks("ops.alt_corr_backward (atomic)", g1.cpu(), g2.cpu(), gc.cpu(), adj, N, r)


# ------------------------------------------------------------------------------------------------ lookup
@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("D,L,r,P", tc.LOOKUP_CASES)
def test_train_lookup_forward_and_adjoint(dev, D, L, r, P, shift):
    Lb, lib = _lib()
    V, incre, taps = tc.LOOKUP_V, tc.LOOKUP_INCRE, 2 * r + 1
    vol, origin, disp, gout = tc.lookup_case(D, L, r, P, shift)
    tc.assert_lookup_census(tc.lookup_census(origin, disp, D, L, r), D, L, P)
    ref, mag = pc.train_lookup_ref64(vol, origin, disp, D, incre, L, r)
    gref, gmag, _ = pc.train_lookup_adjoint_ref64(gout, origin, disp, D, incre, L, r)
    v, o, z, gd = vol.to(dev), origin.to(dev), disp.to(dev), gout.to(dev)
    out = nan_buf(dev, V, L * taps, P)
    Lb.check(lib.cer_train_lookup_fwd_f32(Lb.dev_ptr(v, "vol"), Lb.dev_ptr(o, "origin"), Lb.dev_ptr(z, "disp"), Lb.dev_ptr(out, "out"), V, P, D,
                                          float(incre), L, r, Lb.cur_stream()), "lookup")
    level = torch.arange(L * taps) // taps
    bound = ((4 + level).double() * U24).view(1, 1, -1) * mag.permute(0, 2, 1)
    compare("train_lookup forward", out.cpu().permute(0, 2, 1), ref.permute(0, 2, 1), bound, 1, P, (1, 64))
    runs = []
    for _ in range(3):
        grad = nan_buf(dev, V, D, P)
        Lb.check(lib.cer_train_lookup_bwd_f32(Lb.dev_ptr(gd, "gout"), Lb.dev_ptr(o, "origin"), Lb.dev_ptr(z, "disp"), Lb.dev_ptr(grad, "grad"), V, P,
                                              D, float(incre), L, r, Lb.cur_stream()), "lookup adjoint")
        runs.append(grad.cpu())
    compare("train_lookup adjoint", runs[0].permute(0, 2, 1), gref.permute(0, 2, 1), (taps + L + 3) * U24 * gmag.permute(0, 2, 1), 1, P, (1, 64))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


# ------------------------------------------------------------------------------------------------ upsample
@pytest.mark.parametrize("n,h,w,H,W", tc.UPSAMPLE_CASES)
def test_upsample_forward_and_both_adjoint_passes(dev, n, h, w, H, W):
    from cer_mvs_amd import ops
    Lb, lib = _lib()
    x, g = tc.upsample_case(n, h, w, H, W)
    ref, mag = pc.upsample_ac_ref64(x, H, W)
    xd, gd = x.to(dev), g.to(dev)
    out = nan_buf(dev, n, H, W)
    Lb.check(lib.cer_upsample_bilinear_ac_f32(Lb.dev_ptr(xd, "x"), Lb.dev_ptr(out, "out"), n, h, w, H, W, Lb.cur_stream()), "upsample")
    compare("upsample forward", out.cpu().view(n, H * W, 1), ref.view(n, H * W, 1), pc.K_UP_FWD * U24 * mag.view(n, H * W, 1), H, W, (1, 256))
    ry, rx = ops.upsample_ac_ranges(h, H), ops.upsample_ac_ranges(w, W)
    gin, work = nan_buf(dev, n, h, w), nan_buf(dev, n, H, w)
    ryd, rxd = ry.to(dev), rx.to(dev)
    Lb.check(lib.cer_upsample_bilinear_ac_bwd_f32(Lb.dev_ptr(gd, "g"), Lb.dev_ptr(gin, "gin"), Lb.dev_ptr(work, "work"), Lb.dev_ptr(ryd, "ry", torch.int32),
                                                  Lb.dev_ptr(rxd, "rx", torch.int32), n, h, w, H, W, Lb.cur_stream()), "upsample adjoint")
    wk, gi = work.cpu(), gin.cpu()
    wref, wmag, nx, bx = pc.upsample_ac_adjoint_pass64(g, w, 2)
    assert torch.equal(rx, bx)
    compare("upsample adjoint x pass", wk.view(n, H * w, 1), wref.view(n, H * w, 1), ((nx.double() + 2) * U24 * wmag).view(n, H * w, 1), H, w, (1, 256))
    yref, ymag, ny, by = pc.upsample_ac_adjoint_pass64(wk, h, 1)              # against the kernel's own work
    assert torch.equal(ry, by)
    compare("upsample adjoint y pass", gi.view(n, h * w, 1), yref.view(n, h * w, 1), ((ny.double() + 2).view(1, h, 1) * U24 * ymag).view(n, h * w, 1),
            h, w, (1, 256))
    cen = tc.upsample_census(h, w, H, W)
    assert cen == tc.UPSAMPLE_CENSUS[(n, h, w, H, W)]                         # the case still reaches its edge (empty ranges, w = 1, W = 1, ...)
    empty_y, empty_x = ry[:, 0] == ry[:, 1], rx[:, 0] == rx[:, 1]
    assert int(empty_y.sum()) == cen["empty_rows"] and int(empty_x.sum()) == cen["empty_cols"]
    assert bool((wk[:, :, empty_x] == 0).all()) and bool((gi[:, empty_y] == 0).all()) and bool((gi[:, :, empty_x] == 0).all())
    if (n, h, w, H, W) == (1, 40, 50, 7, 9):
        assert cen["empty_rows"] > 0 and cen["empty_cols"] > 0                # the downsampling case has texels in no footprint
    if (h, w) == (H, W):
        assert cen["identity"] and torch.equal(out.cpu(), x) and torch.equal(gi, g)
