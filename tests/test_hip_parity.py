"""Parity of the HIP path (through the C ABI) against the oracle and the golden fixtures.
Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import cached_scene, rel_l1
from test_oracle_golden import blank_state_dict, hashed

pytestmark = pytest.mark.gpu

TOL = 1e-4          # BASELINE.md §3 parity bar (relative L1); kernels typically land at 1e-6..1e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def test_library_sees_gpu():
    from cer_mvs_amd import _lib
    assert _lib.load().cer_device_count() >= 1


# ------------------------------------------------------------------------------------ alt_cuda_corr
@pytest.mark.parametrize("shape", [(1, 5, 12, 20, 12, 20, 64), (2, 3, 9, 13, 11, 7, 128)])
def test_alt_corr_forward_radius0(dev, shape):
    from cer_mvs_amd import alt_cuda_corr
    from oracle import cer_oracle as O
    B, N, H1, W1, H2, W2, C = shape
    f1 = hashed((B, H1, W1, C), 51)
    f2 = hashed((B, H2, W2, C), 52)
    xy = torch.stack([hashed((B, N, H1, W1), 53, -3.0, W2 + 2.0), hashed((B, N, H1, W1), 54, -3.0, H2 + 2.0)], -1).contiguous()
    xy[0, 0, 0, 0] = torch.tensor([1e4, -1e4])       # clamped extremes
    xy[0, 0, 0, 1] = torch.tensor([2.0, 3.0])         # exactly on a texel
    ref = O.alt_corr_forward(f1, f2, xy)
    out, = alt_cuda_corr.forward(f1.to(dev), f2.to(dev), xy.to(dev), 0)
    assert out.shape == ref.shape
    assert rel_l1(out.cpu(), ref) < 1e-5


def test_alt_corr_forward_radius1(dev):
    """General radius: channel ky + rd*kx samples at (x - r + kx, y - r + ky) (correlation_kernel.cu:92-114)."""
    from cer_mvs_amd import alt_cuda_corr
    from oracle import cer_oracle as O
    B, N, H, W, C, r = 1, 2, 10, 14, 64, 1
    f1, f2 = hashed((B, H, W, C), 61), hashed((B, H, W, C), 62)
    xy = torch.stack([hashed((B, N, H, W), 63, -2.0, W + 1.0), hashed((B, N, H, W), 64, -2.0, H + 1.0)], -1).contiguous()
    out, = alt_cuda_corr.forward(f1.to(dev), f2.to(dev), xy.to(dev), r)
    rd = 2 * r + 1
    assert out.shape == (B, N, rd * rd, H, W)
    for kx in range(rd):
        for ky in range(rd):
            # integer offsets keep floor/frac unchanged, so shifting the coordinates is the same sample
            ref = O.alt_corr_forward(f1, f2, xy + torch.tensor([kx - r, ky - r], dtype=torch.float32))[:, :, 0]
            assert rel_l1(out[:, :, ky + rd * kx].cpu(), ref) < 1e-5


def test_alt_corr_backward(dev):
    """Gradients of the radius-0 op wrt fmap1/fmap2 equal autograd through the oracle's grid_sample form."""
    from cer_mvs_amd import alt_cuda_corr
    from oracle import cer_oracle as O
    B, N, H, W, C = 1, 3, 8, 12, 64
    f1, f2 = hashed((B, H, W, C), 71), hashed((B, H, W, C), 72)
    xy = torch.stack([hashed((B, N, H, W), 73, -1.0, W + 0.5), hashed((B, N, H, W), 74, -1.0, H + 0.5)], -1).contiguous()
    g = hashed((B, N, 1, H, W), 75)
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    (O.alt_corr_forward(a, b, xy) * g).sum().backward()
    g1, g2, gc = alt_cuda_corr.backward(f1.to(dev), f2.to(dev), xy.to(dev), g.to(dev), 0)
    assert rel_l1(g1.cpu(), a.grad) < 1e-5
    assert rel_l1(g2.cpu(), b.grad) < 1e-5
    assert float(gc.abs().max()) == 0.0               # the reference never writes coords_grad (correlation_kernel.cu:307)


def test_alt_corr_rejects_bad_inputs(dev):
    from cer_mvs_amd import alt_cuda_corr
    f = torch.zeros(1, 4, 4, 64)
    xy = torch.zeros(1, 1, 4, 4, 2)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        alt_cuda_corr.forward(f, f.to(dev), xy.to(dev), 0)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        alt_cuda_corr.forward(f.to(dev).permute(0, 2, 1, 3), f.to(dev), xy.to(dev), 0)


# ------------------------------------------------------------------------------------ CorrBlock
def _corrblock_inputs(golden):
    g = golden("corrblock")
    h1, w1, V = int(g["h1"]), int(g["w1"]), int(g["V"])
    fmaps = hashed((1, V + 1, 64, h1, w1), 11, -2.0, 2.0)
    return g, h1, w1, V, fmaps, torch.from_numpy(g["poses"]), torch.from_numpy(g["intrinsics"])


@pytest.mark.parametrize("stage", [0, 1])
def test_corrblock_matches_reference_capture(dev, golden, stage):
    from cer_mvs_amd import CorrBlock
    g, h1, w1, V, fmaps, poses, intr = _corrblock_inputs(golden)
    D, N, shift = ((64, 64, True), (44, 320, False))[stage]
    incre = 0.0025 / N
    disp_in = torch.from_numpy(g[f"disp_in{stage}"])
    cb = CorrBlock(fmaps.to(dev), poses.to(dev), intr.to(dev), torch.zeros(V, dtype=torch.long), torch.arange(1, V + 1),
                   nIncre=D, incre=incre, disps_input=disp_in.to(dev), shift=shift, num_levels=3, radius=5)
    assert torch.equal(cb.disps_origin.cpu().reshape(h1, w1), torch.from_numpy(g[f"origin{stage}"]))
    for lv in range(3):
        ref = torch.from_numpy(g[f"pyr{stage}_{lv}"])
        got = cb.corr_pyramid[lv].cpu().reshape(V, h1 * w1, -1)
        assert got.shape == ref.shape
        assert rel_l1(got, ref) < 1e-5, (stage, lv)
    zinv = torch.from_numpy(g[f"zinv{stage}"])
    feats = cb(zinv[:, [0] * V].to(dev))
    ref = torch.from_numpy(g[f"feats{stage}"])
    assert feats.shape == ref.shape and feats.is_contiguous()
    assert rel_l1(feats.cpu(), ref) < 1e-5


@pytest.mark.parametrize("stage", [0, 1])
def test_view_mean_fold_is_exact(dev, golden, stage):
    """lookup(mean_v volume) == mean_v lookup(volume_v) (first reduction)."""
    from cer_mvs_amd import CorrBlock
    g, h1, w1, V, fmaps, poses, intr = _corrblock_inputs(golden)
    D, N, shift = ((64, 64, True), (44, 320, False))[stage]
    args = (fmaps.to(dev), poses.to(dev), intr.to(dev), torch.zeros(V, dtype=torch.long), torch.arange(1, V + 1))
    kw = dict(nIncre=D, incre=0.0025 / N, disps_input=torch.from_numpy(g[f"disp_in{stage}"]).to(dev), shift=shift, num_levels=3, radius=5)
    zinv = torch.from_numpy(g[f"zinv{stage}"])[:, [0] * V].to(dev)
    per_view = CorrBlock(*args, **kw)(zinv).mean(1)
    folded = CorrBlock(*args, fold_views=True, **kw)(zinv)[:, 0]
    assert rel_l1(folded.cpu(), per_view.cpu()) < 1e-5
    ref = torch.from_numpy(g[f"feats{stage}"]).mean(1)
    assert rel_l1(folded.cpu(), ref) < 1e-5


def test_cost_build_edge_cases(dev):
    """Ragged sizes (P not a multiple of 16, D not a multiple of 16), a single view, views that project
    entirely out of bounds and a degenerate Pij (Z = 0 -> non-finite coordinates)."""
    from cer_mvs_amd import ops
    from oracle import cer_oracle as O
    h1, w1, V, C, D, incre = 7, 13, 2, 64, 20, 0.0025 / 64
    fm = hashed((V + 1, C, h1, w1), 81, -2, 2)
    poses = torch.eye(4).repeat(V + 1, 1, 1)
    poses[1, 0, 3] = 40.0
    poses[2, 0, 3] = 1e7                              # projects far outside: all zeros
    intr = torch.tensor([[90.0, 0, 6.5], [0, 90.0, 3.5], [0, 0, 1]]).repeat(V + 1, 1, 1)
    disp_in = hashed((h1, w1), 82, 0.0, 0.002)
    vol_ref, origin_ref = O.cost_volume(fm, poses, intr, D, incre, disp_in, True)
    from cer_mvs_amd.corr import fmaps_to_nhwc
    f1, f2 = fmaps_to_nhwc(fm[:1].to(dev))[0], fmaps_to_nhwc(fm[1:].to(dev), border=2)
    Pij = O.pij_matrices(poses, intr, [0] * V, [1, 2]).contiguous()
    vol, origin = ops.cost_build(f1, f2, Pij.to(dev), disp_in.reshape(-1).to(dev), D, incre, True, h1, w1, 3, fold=False)
    assert torch.equal(origin.cpu().view(h1, w1), origin_ref)
    assert rel_l1(vol[..., :D].cpu(), vol_ref) < 1e-5
    assert float(vol[1, :, 1:D].abs().max()) == 0.0      # hypothesis 0 can be exactly d = 0, which projects onto itself
    bad = Pij.clone()
    bad[0, 2] = 0.0                                    # Z == 0 everywhere
    vol2, _ = ops.cost_build(f1, f2, bad.to(dev), disp_in.reshape(-1).to(dev), D, incre, True, h1, w1, 3, fold=False)
    # (level 0 only: the pooled levels of a row are undefined until cer_pyramid_f32 has run)
    assert torch.isfinite(vol2[..., :D]).all() and float(vol2[0, :, :D].abs().max()) == 0.0


def test_lookup_edge_cases(dev):
    """Index below 0 (clamped), far beyond the row (all taps zero), exactly integral, and a ragged P."""
    from cer_mvs_amd import ops
    from oracle import cer_oracle as O
    P, D, incre, L, r = 37, 44, 0.0025 / 320, 3, 5
    offs, lens, rs = ops.row_layout(D, L)
    vol0 = hashed((1, P, D), 91)
    levels = O.pyramid(vol0, L)
    packed = torch.zeros(1, P, rs)
    for o, n, lv in zip(offs, lens, levels):
        packed[..., o:o + n] = lv
    origin = hashed((P,), 92, 0.001, 0.002)
    steps = hashed((P,), 93, -40.0, 60.0)
    steps[0], steps[1], steps[2], steps[3] = -100.0, 1e6, 3.0, -22.0
    disp = origin + steps * incre
    ref = O.lookup(levels, origin.view(1, P), disp.view(1, P), D, incre, r)
    out = ops.corr_lookup(packed.to(dev), origin.to(dev), disp.to(dev), D, incre, L, r)
    assert rel_l1(out.cpu().view(1, -1, 1, P), ref) < 1e-5


@pytest.mark.parametrize("D,L", [(64, 3), (44, 3), (20, 2), (40, 4), (64, 1), (5, 3), (3, 2)])
def test_lookup_on_level0_rows_is_bit_identical(dev, D, L):
    """Round 5: rows that hold level 0 only (row_stride < the whole pyramid) - both lookup kernels form the pooled levels on the fly, in
    cer_pyramid_f32's association: bit for bit what they read from rows that store the levels (core/corr.py:94-97,102-143), incl. the
    indices of test_lookup_edge_cases (below 0, beyond the row, integral) and a ragged P."""
    from cer_mvs_amd import _lib as Lb, ops
    h, w, r = 9, 21, 5
    P, incre = h * w, 0.0025 / 320
    _, _, rs = ops.row_layout(D, L)
    _, _, rs0 = ops.row_layout(D, L, compact=True)
    assert rs0 == (D + 3) // 4 * 4 and (rs0 < rs or L == 1 or D <= 5)      # (D <= 5: both forms fit one stride - the flag is explicit)
    full = torch.zeros(P, rs, device=dev)
    full[:, :D] = hashed((P, D), 191, -30.0, 30.0).to(dev)
    ops.pyramid(full, D, L, scale=0.1)
    lvl0 = torch.zeros(P, rs0, device=dev)
    lvl0[:, :D] = full[:, :D]
    origin = hashed((P,), 192, 0.001, 0.002)
    steps = hashed((P,), 193, -40.0, 90.0)
    steps[0], steps[1], steps[2], steps[3] = -100.0, 1e6, 3.0, -22.0
    disp = (origin + steps * incre).to(dev)
    origin = origin.to(dev)
    a = ops.corr_lookup(full, origin, disp, D, incre, L, r, level0_only=False)
    b = ops.corr_lookup(lvl0, origin, disp, D, incre, L, r, level0_only=True)
    assert torch.equal(a, b) and float(a.abs().sum()) > 0
    K = L * (2 * r + 1)
    w0t, b0 = hashed((K, 64), 194, -0.2, 0.2).to(dev), hashed((64,), 195, -0.1, 0.1).to(dev)
    for kw in ({}, {"out_split": 2, "log2s": Lb.S16_RELU, "img_w": w}):
        assert torch.equal(ops.lookup_encode(full, origin, disp, w0t, b0, D, incre, L, r, level0_only=False, **kw),
                           ops.lookup_encode(lvl0, origin, disp, w0t, b0, D, incre, L, r, level0_only=True, **kw))
    if rs0 < rs:       # unmarked tensors: the stride decides where it can ...
        assert torch.equal(ops.corr_lookup(lvl0, origin, disp, D, incre, L, r), a)
    elif L > 1:        # ... and a stride that fits both forms is refused, not guessed
        with pytest.raises(ValueError):
            ops.corr_lookup(lvl0, origin, disp, D, incre, L, r)


def test_lookup_row_form_is_explicit(dev):
    """ABI 1060: the row form is an argument of both lookup entry points.  Level-0-only rows form at most 4 levels (lk_elem);
    whole-pyramid rows must hold the whole pyramid."""
    from cer_mvs_amd import ops
    P, D, r, incre = 40, 64, 1, 0.0025 / 64
    origin, disp = torch.zeros(P, device=dev), torch.full((P,), 10 * incre, device=dev)
    vol = hashed((P, 64), 196, -1.0, 1.0).to(dev)
    ops.corr_lookup(vol, origin, disp, D, incre, 4, r, level0_only=True)
    with pytest.raises(RuntimeError):
        ops.corr_lookup(vol, origin, disp, D, incre, 5, r, level0_only=True)        # five levels cannot be pooled on the fly
    with pytest.raises(RuntimeError):
        ops.corr_lookup(vol, origin, disp, D, incre, 3, r, level0_only=False)       # 64 floats do not hold 64 + 32 + 16


def test_lookup_flags_a_saturated_output_itself(dev):
    """Round 5: the lookup's frag16 output (c1, ReLU class: 65504 / 2^4 = 4094) shares its buffer with r * h later in the iteration, so
    it cannot be scanned after the fact any more - the kernel checks what it clamps: a clean launch leaves the flag alone, one output
    beyond the limit raises bit 4 (saturation is never silent)."""
    from cer_mvs_amd import _lib as Lb, ops
    h, w, D, L, r = 9, 21, 64, 3, 5
    P, incre = h * w, 0.0025 / 64
    vol = hashed((P, 64), 211, -30.0, 30.0).to(dev)
    origin = torch.full((P,), 0.00125, device=dev)
    disp = hashed((P,), 212, 0.0, 60 * incre).to(dev)
    w0t, b0 = hashed((33, 64), 213, -0.2, 0.2).to(dev), hashed((64,), 214, -0.1, 0.1).to(dev)
    ops.check_overflow(dev)
    ops.lookup_encode(vol, origin, disp, w0t, b0, D, incre, L, r, out_split=2, log2s=Lb.S16_RELU, img_w=w)
    assert ops.check_overflow(dev) == 0
    b_hot = b0.clone()
    b_hot[17] = 5000.0                                         # one output channel beyond 4094 at every pixel
    ops.lookup_encode(vol, origin, disp, w0t, b_hot, D, incre, L, r, out_split=2, log2s=Lb.S16_RELU, img_w=w)
    assert ops.check_overflow(dev) & 4
    assert ops.check_overflow(dev) == 0                         # (reading clears it)


@pytest.mark.parametrize("h,w,nhalf", [(9, 21, 2), (40, 150, 2), (7, 64, 1)])
def test_lookup_applies_the_pending_disparity_update(dev, h, w, nhalf):
    """Round 5: cer_lookup_encode_f32 with delta_taps = the previous iteration's cer_delta_sum_f32 (core/update.py:114, core/raft.py:101)
    riding on the lookup launch: the disparity it leaves in place and the features it writes are bit for bit those of the two launches."""
    from cer_mvs_amd import _lib as Lb, ops
    P, D, L, r, incre = h * w, 64, 3, 5, 0.0025 / 64
    _, _, rs0 = ops.row_layout(D, L, compact=True)
    vol = hashed((P, rs0), 201, -30.0, 30.0).to(dev)
    origin = hashed((P,), 202, 0.001, 0.002).to(dev)
    disp0 = (origin.cpu() + hashed((P,), 203, -30.0, 40.0) * incre).to(dev)
    T = hashed((nhalf, 9, P), 204, -0.02, 0.02).to(dev)
    bias = 0.0123
    w0t, b0 = hashed((L * (2 * r + 1), 64), 205, -0.2, 0.2).to(dev), hashed((64,), 206, -0.1, 0.1).to(dev)
    d_ref, _ = ops.delta_sum(T, bias, disp0, h, w)
    f_ref = ops.lookup_encode(vol, origin, d_ref, w0t, b0, D, incre, L, r, out_split=2, log2s=Lb.S16_RELU, img_w=w)
    assert not torch.equal(d_ref, disp0)
    for _ in range(3):
        d = disp0.clone()
        f = ops.lookup_encode(vol, origin, d, w0t, b0, D, incre, L, r, out_split=2, log2s=Lb.S16_RELU, img_w=w, delta=(T, bias))
        assert torch.equal(d, d_ref) and torch.equal(f, f_ref)


# ------------------------------------------------------------------------------------ conv kernels
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
@pytest.mark.parametrize("h,w,cout", [(8, 16, 64), (11, 21, 64), (9, 17, 128), (16, 32, 256), (5, 70, 128)])
def test_conv3x3_matches_torch(dev, h, w, cout, mode):
    from cer_mvs_amd import _lib as L, ops
    cin = 64
    x = hashed((1, cin, h, w), 101)
    wt = hashed((cout, cin, 3, 3), 102, -0.1, 0.1)
    b = hashed((cout,), 103)
    ref = F.conv2d(x, wt, b, padding=1)[0].permute(1, 2, 0).reshape(h * w, cout)
    pc = ops.PackedConv3x3(wt, b, [(cin, 0)], dev)
    xl = x[0].permute(1, 2, 0).reshape(h * w, cin).contiguous().to(dev)
    out = ops.conv3x3(pc, [xl], h, w, L.EPI_LINEAR, mode=mode)
    assert rel_l1(out.cpu(), ref) < 2e-6
    out = ops.conv3x3(pc, [xl], h, w, L.EPI_RELU, mode=mode)
    assert rel_l1(out.cpu(), F.relu(ref)) < 2e-6


def test_conv3x3_f16x3_dynamic_range(dev):
    """The split keeps fp32-class accuracy for tiny and large activations (fp16 subnormal / near-overflow ranges)
    and saturates beyond +-65504 instead of producing inf."""
    from cer_mvs_amd import _lib as L, ops
    h, w, cin, cout = 8, 32, 32, 64
    x = hashed((1, cin, h, w), 121)
    scale = torch.logspace(-4, 4, h * w).view(1, 1, h, w)           # 1e-4 .. 1e4 per pixel
    x = x * scale
    wt = hashed((cout, cin, 3, 3), 122, -0.2, 0.2)
    ref = F.conv2d(x.double(), wt.double(), None, padding=1)[0].permute(1, 2, 0).reshape(h * w, cout)
    pc = ops.PackedConv3x3(wt, None, [(cin, 0)], dev)
    xl = x[0].permute(1, 2, 0).reshape(h * w, cin).contiguous().to(dev)
    got = ops.conv3x3(pc, [xl], h, w, L.EPI_LINEAR, mode="f16x3").cpu().double()
    exact = ops.conv3x3(pc, [xl], h, w, L.EPI_LINEAR, mode="fp32").cpu().double()
    mag = F.conv2d(x.abs().double(), wt.abs().double(), None, padding=1)[0].permute(1, 2, 0).reshape(h * w, cout)
    assert float(((got - ref).abs() / mag).max()) < 2e-6            # error relative to sum |x||w| per output
    assert float(((exact - ref).abs() / mag).max()) < 2e-6
    # below the f16 normal range the split has an ABSOLUTE resolution of 2^-25 * 2^-11 ~ 1.5e-11 per operand
    # (f16 subnormal step on the scaled lo half): error <= 2e-6 * sum|x||w| + 3e-11 * sum|w|
    tiny = (hashed((h * w, cin), 123) * torch.logspace(-8, -5, h * w).view(-1, 1)).contiguous()
    tref = F.conv2d(tiny.t().reshape(1, cin, h, w).double(), wt.double(), None, padding=1)[0].permute(1, 2, 0).reshape(h * w, cout)
    tmag = F.conv2d(tiny.t().reshape(1, cin, h, w).abs().double(), wt.abs().double(), None, padding=1)[0].permute(1, 2, 0).reshape(h * w, cout)
    tgot = ops.conv3x3(pc, [tiny.to(dev)], h, w, L.EPI_LINEAR, mode="f16x3").cpu().double()
    wsum = F.conv2d(torch.ones(1, cin, h, w).double(), wt.abs().double(), None, padding=1)[0].permute(1, 2, 0).reshape(h * w, cout)
    assert bool(((tgot - tref).abs() <= 2e-6 * tmag + 3e-11 * wsum).all())
    big = torch.full((h * w, cin), 1e6, device=dev)
    out = ops.conv3x3(pc, [big], h, w, L.EPI_LINEAR, mode="f16x3")
    assert torch.isfinite(out).all()


def test_conv3x3_disp_encoder_source(dev):
    """Source kind 1 generates 100*(unfold7x7(disp) - disp) on the fly (core/update.py:80-85,97)."""
    from cer_mvs_amd import _lib as L, ops
    from oracle import cer_oracle as O
    h, w, cout = 13, 19, 64
    disp = hashed((1, 1, h, w), 111, 0.0, 0.0025)
    a = hashed((1, 32, h, w), 112)
    feat = 100 * O.disp_features(disp)
    wt = hashed((cout, 32 + 49, 3, 3), 113, -0.1, 0.1)
    ref = F.conv2d(torch.cat([a, feat], 1), wt, None, padding=1)[0].permute(1, 2, 0).reshape(h * w, cout)
    pc = ops.PackedConv3x3(wt, None, [(32, 0), (49, 1)], dev)
    al = a[0].permute(1, 2, 0).reshape(h * w, 32).contiguous().to(dev)
    for mode in ("fp32", "f16x3"):
        out = ops.conv3x3(pc, [al, disp.reshape(-1).to(dev)], h, w, L.EPI_LINEAR, mode=mode)
        assert rel_l1(out.cpu(), ref) < 2e-6, mode


def _lines_case(dev, D, stage0, geom, h1, w1):
    """The geometries live in tests/cost_geometry_cases.py (which tests/test_cost_geometry_gpu.py holds against a float64 reference)."""
    from cer_mvs_amd.corr import fmaps_to_nhwc
    from cost_geometry_cases import V, lines_geometry
    fm, Pij, d0 = lines_geometry(geom, D, stage0, h1, w1)
    fm = fm.to(dev)
    f1 = fmaps_to_nhwc(fm[0:1])[0]
    f2 = fmaps_to_nhwc(fm[1:], border=2)
    return f1, f2, Pij.to(dev), d0.to(dev), V


@pytest.mark.parametrize("geom", ["horizontal", "diagonal", "vertical", "wild", "rotation", "forward", "converging", "zoom"])
@pytest.mark.parametrize("D,stage0", [(64, True), (44, False), (20, False)])
@pytest.mark.parametrize("form", [0, 1])
def test_cost_lines_matches_walk(dev, D, stage0, geom, form):
    """The round-3 fold kernel (epipolar-line tiles: MFMA band products + 4-tap gather, csrc/cost_lines.hip) against the
    wave-per-pixel walk on the same inputs: epipolar lines of every direction (both tile axes, both band axes, both travel
    directions), a view whose projection blows up (Z crosses 0 inside the hypothesis range: direct per-sample path), no
    baseline, an epipole inside the image, image sizes with partial tiles and several segments, a row-slab offset,
    accumulate mode and the fused pyramid.  form 0: one line per block (the default); form 1: several lines per block sharing one band
    (round 4 experiment; the "zoom" geometry spreads the lines of a block too far apart for its window and goes through its hand-over list)."""
    from cer_mvs_amd import _lib as L, ops
    lib = L.load()
    if form == 0 and not L.has_variant_forms():
        return _cost_lines_matches_walk(dev, D, stage0, geom, lib)
    if not L.has_variant_forms():
        pytest.skip("the multi-line form is not in the product library: run with CER_MVS_LIB=.../variants/libcermvs_optin.so (tools/archive/r05/test_variants.sh)")
    prev_form = lib.cer_cost_lines_form(form)
    try:
        _cost_lines_matches_walk(dev, D, stage0, geom, lib)
    finally:
        lib.cer_cost_lines_form(prev_form)


@pytest.mark.parametrize("geom", ["horizontal", "diagonal", "forward", "converging"])
@pytest.mark.parametrize("D,stage0", [(64, True), (44, False)])
def test_cost_lines_two_term_form(dev, D, stage0, geom):
    """Round 6 (ABI 1070, ``two_term``): the tile kernel WITHOUT the source texels' lo planes - the source features enter the 64-channel dots as
    f16, the reference rows keep both halves.  Against the three-term form on the same inputs: origins identical, the volume a source-f16
    rounding away (each texel 2^-12 relative: 1.2e-5 relative L1 on the volume at the bench workload, ~2e-4 on this test's hashed features whose
    dots cancel; a wrong plane is 1e-1), and exactly what the THREE-term kernel returns for source features rounded to
    f16 beforehand - which pins the form to its definition instead of to a tolerance.  Deterministic; the fused epilogue and the
    level-0-only rows as in the three-term form."""
    from cer_mvs_amd import ops
    for h1, w1 in ((19, 45), (70, 150)):
        f1, f2, Pij, d0, V = _lines_case(dev, D, stage0, geom, h1, w1)
        incre = 0.0025 / (64 if stage0 else 320)
        a3, o3 = ops.cost_build(f1, f2, Pij, d0, D, incre, stage0, h1, w1, 3, fold=True, pyramid_scale=1.0 / V)
        a2, o2 = ops.cost_build(f1, f2, Pij, d0, D, incre, stage0, h1, w1, 3, fold=True, pyramid_scale=1.0 / V, two_term=True)
        again, _ = ops.cost_build(f1, f2, Pij, d0, D, incre, stage0, h1, w1, 3, fold=True, pyramid_scale=1.0 / V, two_term=True)
        c2, _ = ops.cost_build(f1, f2, Pij, d0, D, incre, stage0, h1, w1, 3, fold=True, pyramid_scale=1.0 / V, compact=True, two_term=True)
        assert torch.equal(o3, o2) and torch.equal(a2, again) and torch.equal(c2[:, :D], a2[:, :D])
        e = rel_l1(a2.cpu(), a3.cpu())
        # the kernel's operand is x * 2^6 split into f16 hi | lo: the two-term form sees hi only
        f2r = ((f2 * 64.0).clamp(-65504.0, 65504.0).half().float() / 64.0)
        r3, _ = ops.cost_build(f1, f2r, Pij, d0, D, incre, stage0, h1, w1, 3, fold=True, pyramid_scale=1.0 / V)
        print(f"{geom} D={D} {h1}x{w1}: two-term vs three-term {e:.2e}; vs three-term on f16-rounded source rows {rel_l1(a2.cpu(), r3.cpu()):.2e}")
        assert 1e-6 < e < 1e-3            # (hashed features: dots of random signs cancel, the relative figure is 10 x the bench scene's 1.2e-5)
        assert torch.equal(a2, r3)


def _cost_lines_matches_walk(dev, D, stage0, geom, lib):
    from cer_mvs_amd import ops
    for h1, w1 in ((19, 45), (70, 150)):
        f1, f2, Pij, d0, V = _lines_case(dev, D, stage0, geom, h1, w1)
        incre = 0.0025 / (64 if stage0 else 320)
        res = {}
        for algo in (1, 0):
            prev = lib.cer_cost_build_algo(algo)
            try:
                a, oa = ops.cost_build(f1, f2, Pij, d0, D, incre, stage0, h1, w1, 3, fold=True)
                b, ob = ops.cost_build(f1, f2, Pij, d0, D, incre, stage0, h1, w1, 3, fold=True, pyramid_scale=1.0 / V)
                c, _ = ops.cost_build(f1, f2, Pij, d0, D, incre, stage0, h1, w1, 3, fold=True, vol=a.clone(), accumulate=True)
                s_, _ = ops.cost_build(f1[5 * w1:], f2, Pij, d0[5 * w1:], D, incre, stage0, h1 - 5, w1, 3, fold=True, src_hw=(h1, w1), y0=5)
                # level-0-only rows, scaled (fuse_levels = 1 means "scale only" in BOTH builders since ABI 1060): level 0 of b, bit for bit
                e, _ = ops.cost_build(f1, f2, Pij, d0, D, incre, stage0, h1, w1, 3, fold=True, pyramid_scale=1.0 / V, compact=True)
                assert e.shape[1] == (D + 3) // 4 * 4 and e.level0_only and not b.level0_only and torch.equal(e[:, :D], b[:, :D])
                res[algo] = (a, oa, b, ob, c, s_)
            finally:
                lib.cer_cost_build_algo(prev)
        ref, new = res[1], res[0]
        n = D + D // 2 + D // 4
        assert torch.equal(ref[1], new[1]) and torch.equal(ref[3], new[3])                    # origins
        mag = max(float(ref[0][:, :D].abs().max()), 1.0)
        for i, cols in ((0, D), (2, n), (4, D), (5, D)):
            err = float((ref[i][:, :cols] - new[i][:, :cols]).abs().max())
            assert err <= 4e-6 * mag * (2 if i == 4 else 1), (geom, h1, w1, i, err, mag)
        assert float((new[5][:, :D] - new[0][5 * w1:, :D]).abs().max()) <= 4e-6 * mag         # the slab sees the same samples
        assert new[0][:, :D].abs().sum() > 0
    assert not ops.check_overflow(dev)


def test_depth_map_pipeline_two_streams(dev, golden):
    """pipeline.DepthMapPipeline: two independent depth maps in flight on two HIP streams (a model replica each) give, in order,
    exactly the disparities of one-at-a-time forwards - alternating between two different scenes."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.pipeline import DepthMapPipeline
    from cer_mvs_amd.synthetic import fill_state_dict
    g = golden("e2e_cfg1")
    cascade = [tuple(int(x) for x in c) for c in g["cascade"]]
    model = RAFT(cascade=cascade, test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(g["weight_seed"])))
    model = model.to(dev).eval()
    scenes = []
    for seed in (int(g["scene_seed"]), 17):
        images, poses, intr, scale = cached_scene(int(g["H"]), int(g["W"]), int(g["V"]), seed)
        scenes.append((images.to(dev), poses.to(dev), intr.to(dev), scale))
    with torch.no_grad():
        want = [model(*s_[:3], scale=s_[3]).clone() for s_ in scenes]
    assert rel_l1(want[0].cpu(), torch.from_numpy(g["disp"])) < TOL and not torch.equal(want[0], want[1])
    pipe = DepthMapPipeline(model, streams=2)
    got = list(pipe.map([scenes[i % 2] for i in range(7)]))
    assert len(got) == 7 and all(torch.equal(o, want[i % 2]) for i, o in enumerate(got))
    assert pipe.check_overflow() == 0
    # new weights on the original reach the replica through refresh_weights()
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=99))
    pipe.refresh_weights()
    with torch.no_grad():
        want2 = model(*scenes[0][:3], scale=scenes[0][3]).clone()
    got2 = list(pipe.map([scenes[0]] * 2))
    assert not torch.equal(want2, want[0]) and all(torch.equal(o, want2) for o in got2)


def test_encoder_type_lr_matches_reference_capture(dev, golden):
    """encoder_type="LR" (core/extractor.py:87-90,151: a third residual stage, features at 1/8 resolution, core/raft.py:38) end to
    end against the reference's own output (tests/golden/e2e_lr.npz) - fast path and literal path."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    g = golden("e2e_lr")
    cascade = [tuple(int(x) for x in c) for c in g["cascade"]]
    model = RAFT(cascade=cascade, encoder_type="LR", test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(g["weight_seed"])))
    model = model.to(dev).eval()
    images, poses, intr, scale = cached_scene(int(g["H"]), int(g["W"]), int(g["V"]), int(g["scene_seed"]))
    args = (images.to(dev), poses.to(dev), intr.to(dev))
    ref = torch.from_numpy(g["disp"])
    with torch.no_grad():
        fast = model(*args, scale=scale)
        lit = model._forward_literal(*args, scale, False)
    assert fast.shape == ref.shape
    assert rel_l1(fast.cpu(), ref) < TOL and rel_l1(lit.cpu(), ref) < TOL


def test_s16_saturation_raises_the_overflow_flag(dev):
    """The s16 layouts clamp ReLU-class activations beyond 4094 = 65504 / 2^4 (silent saturation).  An activation of
    5000 in a frag16 tensor is found by the scan, a hidden activation beyond the limit inside the fused delta head by the kernel's
    own check, and RAFT.check_overflow turns the flag into an error."""
    from cer_mvs_amd import RAFT, _lib as L, ops
    h, w = 16, 32
    ops.check_overflow(dev)
    x = torch.relu(hashed((h * w, 64), 901, -1.0, 3000.0)).to(dev)
    fr = ops.to_frag16(x, h, w, L.S16_RELU)
    ops.scan_overflow(fr)
    assert ops.check_overflow(dev) == 0                     # 3000 * 16 = 48000 < 65504: clean
    x[5, 7] = 5000.0
    fr = ops.to_frag16(x, h, w, L.S16_RELU)
    ops.scan_overflow(fr)
    assert ops.check_overflow(dev) == 4 and ops.check_overflow(dev) == 0
    assert float(ops.from_frag16(fr, h, w, L.S16_RELU)[5, 7]) < 4095.0          # ... and it WAS clamped
    # fused delta head: hidden = relu(conv(net)) with weights large enough to push one channel beyond 4094
    wt = hashed((256, 64, 3, 3), 902, -0.02, 0.02)
    wt[3] = 12.0
    pc = ops.PackedConvS16(wt, torch.zeros(256), [(64, 2, L.S16_UNIT)], dev)
    proj = ops.delta_proj_pack_s16(hashed((1, 256, 3, 3), 903, -0.1, 0.1), dev)
    net = ops.to_frag16(torch.full((h * w, 64), 0.9, device=dev), h, w, L.S16_UNIT)
    T = torch.empty(2, 9, h * w, device=dev)
    ops.conv3x3_s16(pc, [net], h, w, L.EPI_DELTA, out=T, aux=proj)
    assert ops.check_overflow(dev) & 2
    model = RAFT(test_mode=True)
    ops.overflow_flag(dev).fill_(4)
    with pytest.raises(RuntimeError, match="saturated"):
        model.to(dev).check_overflow(dev)
    assert ops.check_overflow(dev) == 0


def test_feat_split_roundtrip_and_overflow_flag(dev):
    """cer_feat_split_f16 (plane-major operand layout, cer_mvs.h): hi + lo reconstructs x * 64 to 2^-22 relative; a value beyond +-1023 saturates and raises the
    sticky overflow flag (saturation must not be silent)."""
    from cer_mvs_amd import ops
    x = hashed((500, 64), 881, -900.0, 900.0).to(dev)
    x[3, 5] = 1e-4
    s = ops.feat_split(x).float().reshape(8, 500, 16)            # planes hl * 4 + ks, each [texel][16 channels of group ks]
    rec = (s[:4] + s[4:]).permute(1, 0, 2).reshape(500, 64) / 64.0
    assert float(((rec - x).abs() / x.abs().clamp_min(1e-3)).max()) < 3e-7
    assert not ops.check_overflow(dev)
    x[7, 9] = 1500.0
    ops.feat_split(x)
    assert ops.check_overflow(dev) and not ops.check_overflow(dev)            # reported once, then cleared


@pytest.mark.parametrize("D", [64, 44, 20])
def test_cost_build_fused_pyramid_equals_two_pass(dev, D):
    """cer_cost_build_f32 with fuse_levels: level 0 * 1/V and the avg-pooled levels written by the build's epilogue are
    bit-identical to cer_cost_build_f32 + cer_pyramid_f32 (core/corr.py:94-97)."""
    from cer_mvs_amd import ops
    from cer_mvs_amd.corr import fmaps_to_nhwc
    h1, w1, V, C = 11, 17, 3, 64
    fm = hashed((1, V + 1, C, h1, w1), 301, -2, 2).to(dev)
    f1 = fmaps_to_nhwc(fm[0, 0:1])[0]
    f2 = fmaps_to_nhwc(fm[0, 1:], border=2)
    Pij = torch.eye(4).repeat(V, 1, 1)
    for v in range(V):
        Pij[v, 0, 3] = 900.0 * (v + 1)
        Pij[v, 1, 3] = -300.0 * v
    d0 = hashed((h1 * w1,), 302, 0.0005, 0.002).to(dev)
    incre = 0.0025 / 64
    a, oa = ops.cost_build(f1, f2, Pij.to(dev), d0, D, incre, False, h1, w1, 3, fold=True)
    ops.pyramid(a, D, 3, scale=1.0 / V)
    b, ob = ops.cost_build(f1, f2, Pij.to(dev), d0, D, incre, False, h1, w1, 3, fold=True, pyramid_scale=1.0 / V)
    n = D + D // 2 + D // 4
    assert torch.equal(a[:, :n], b[:, :n]) and torch.equal(oa, ob)
    assert a[:, :D].abs().sum() > 0


def test_conv3x3_split32_layout(dev):
    """Activations in the split32 layout (hi|lo f16 pairs in the fp32 slots, cer_mvs.h): a conv fed by pre-split sources
    (kind 3) is BIT-identical to the same conv splitting fp32 sources in its staging loop; CER_EPI_OUT_SPLIT writes exactly
    split32(fp32 result); the GRU / GATES epilogues reading the hidden state from the split layout differ from the fp32
    read only by the 2^-22 reconstruction."""
    from cer_mvs_amd import _lib as L, ops
    h, w = 13, 70
    P = h * w
    net = torch.tanh(hashed((P, 64), 501, -2, 2)).to(dev)
    c2 = torch.relu(hashed((P, 64), 502, -1, 2)).to(dev)
    disp = hashed((P,), 503, 0.0005, 0.0025).to(dev)
    init = hashed((P, 128), 504, -0.3, 0.3).to(dev)
    rt = ops.split32(ops.split32(net), inverse=True)
    assert (rt - net).abs().max() <= net.abs().max() * 2.0 ** -21
    pc = ops.PackedConv3x3(hashed((128, 177, 3, 3), 505, -0.05, 0.05), None, [(64, 0), (49, 1), (64, 0)], dev)
    z0, rh0 = ops.conv3x3(pc, [net, disp, c2], h, w, L.EPI_GATES, aux=net, init=init)
    z1, rh1 = ops.conv3x3(pc, [ops.split32(net), disp, ops.split32(c2)], h, w, L.EPI_GATES, aux=net, init=init, kinds=[3, 1, 3])
    assert torch.equal(z0, z1) and torch.equal(rh0, rh1)
    z2, rh2 = ops.conv3x3(pc, [net, disp, c2], h, w, L.EPI_GATES, aux=net, init=init, out_split=True)
    assert torch.equal(z2, z0) and torch.equal(rh2, ops.split32(rh0))
    z3, rh3 = ops.conv3x3(pc, [net, disp, c2], h, w, L.EPI_GATES, aux=ops.split32(net), init=init, aux_split=True)
    assert torch.equal(z3, z0) and rel_l1(rh3.cpu(), rh0.cpu()) < 1e-6
    pq = ops.PackedConv3x3(hashed((64, 177, 3, 3), 506, -0.05, 0.05), None, [(64, 0), (49, 1), (64, 0)], dev)
    initq = hashed((P, 64), 507, -0.3, 0.3).to(dev)
    n0 = ops.conv3x3(pq, [rh0, disp, c2], h, w, L.EPI_GRU, aux=net, aux2=z0, init=initq)
    n1 = ops.conv3x3(pq, [ops.split32(rh0), disp, ops.split32(c2)], h, w, L.EPI_GRU, aux=ops.split32(net), aux2=z0, init=initq,
                     kinds=[3, 1, 3], out_split=True, aux_split=True)
    assert rel_l1(ops.split32(n1, inverse=True).cpu(), n0.cpu()) < 1e-6
    pr = ops.PackedConv3x3(hashed((64, 64, 3, 3), 508, -0.1, 0.1), hashed((64,), 509, -0.1, 0.1), [(64, 0)], dev)
    r0 = ops.conv3x3(pr, [c2], h, w, L.EPI_RELU)
    r1 = ops.conv3x3(pr, [ops.split32(c2)], h, w, L.EPI_RELU, kinds=[3], out_split=True)
    assert torch.equal(r1, ops.split32(r0))


@pytest.mark.parametrize("h,w,cout", [(20, 140, 128), (13, 101, 64), (24, 96, 64)])
def test_conv3x3_collapsed_disparity_tiles(dev, h, w, cout):
    """Interior tiles evaluate the disparity source as one 81-tap filter on the raw disparity (cer_mvs.h,
    cer_conv3x3_f16x3_pack_collapsed); border tiles keep the literal 49-feature form.  Both must match the literal
    convolution, including where the 9x9 window leaves the image (unfold zero padding, core/update.py:80-83)."""
    from cer_mvs_amd import _lib as L, ops
    from oracle import cer_oracle as O
    disp = hashed((1, 1, h, w), 211, 0.0005, 0.0025)
    a = hashed((1, 32, h, w), 212)
    feat = 100 * O.disp_features(disp)
    wt = hashed((cout, 32 + 49, 3, 3), 213, -0.1, 0.1)
    ref = F.conv2d(torch.cat([a, feat], 1).double(), wt.double(), None, padding=1)[0].permute(1, 2, 0).reshape(h * w, cout)
    pc = ops.PackedConv3x3(wt, None, [(32, 0), (49, 1)], dev)
    assert pc.packed_c is not None
    al = a[0].permute(1, 2, 0).reshape(h * w, 32).contiguous().to(dev)
    outs = {}
    for flag in (True, False):
        ops.COLLAPSE_DISP = flag
        try:
            outs[flag] = ops.conv3x3(pc, [al, disp.reshape(-1).to(dev)], h, w, L.EPI_LINEAR, mode="f16x3").cpu().double()
        finally:
            ops.COLLAPSE_DISP = True
        assert rel_l1(outs[flag], ref) < 2e-6, flag
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    interior = ((ys // 4 >= 1) & (ys // 4 * 4 + 4 <= h - 1) & (xs // 32 >= 1) & (xs // 32 * 32 + 32 <= w - 1)).reshape(-1)
    assert interior.any() and not interior.all()
    assert torch.equal(outs[True][~interior], outs[False][~interior])        # border tiles run the literal form
    assert not torch.equal(outs[True][interior], outs[False][interior])      # interior tiles really took the other path
    assert (outs[True] - ref).abs().max() < 5e-6 * ref.abs().max()


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
@pytest.mark.parametrize("stage", [0, 1])
def test_update_block_matches_reference_capture(dev, golden, stage, mode):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    g = golden("update")
    h1, w1, V = int(g["h1"]), int(g["w1"]), int(g["V"])
    model = RAFT(cascade=[(64, 64, 1), (-1, 320, 1)], test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(g["weight_seed"])))
    ub = model.update_block.to(dev)
    ub.conv_mode = mode
    net = torch.tanh(hashed((1, 1, 64, h1, w1), 31, -2, 2))
    inp = torch.relu(hashed((1, 1, 64, h1, w1), 32, -1, 2))
    disp = hashed((1, 1, h1, w1), 33, 0.0, 0.0025)
    corr = hashed((1, V, 33, h1, w1), 34, -1.5, 3.0)
    n2, delta = ub(net.to(dev), inp.to(dev), disp.to(dev), corr.to(dev), stage)
    assert n2.shape == (1, 1, 64, h1, w1) and delta.shape == (1, 1, h1, w1)
    assert rel_l1(n2.cpu(), torch.from_numpy(g[f"net{stage}"])) < 1e-5
    assert rel_l1(delta.cpu(), torch.from_numpy(g[f"delta{stage}"])) < 1e-5


# ------------------------------------------------------------------------------------ encoders
@pytest.mark.parametrize("which", ["fnet", "cnet"])
def test_encoder_fused_passes_match_oracle(dev, which):
    """MIOpen convolutions + fused stats/normalise/ReLU/residual kernels vs the oracle's torch-CPU encoder."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from oracle import cer_oracle as O
    images, _, _, _ = synthetic_scene(72, 104, 1, seed=8)
    model = RAFT(test_mode=True)
    sd = fill_state_dict(model.state_dict(), seed=13)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    x = images[0].float() * (2 / 255.0) - 1
    with torch.no_grad():
        got = getattr(model, which)(x.to(dev)).cpu()
        ref = O.encoder(x, sd, which + ".", "instance" if which == "fnet" else "none")
    assert got.shape == ref.shape
    assert rel_l1(got, ref) < 1e-5


@pytest.mark.parametrize("size", [(72, 104), (128, 160), (64, 96)])
@pytest.mark.parametrize("which", ["fnet", "cnet"])
def test_hip_encoder_engine_matches_oracle(dev, which, size):
    """The channels-last encoder engine (stem + split-f16 MFMA convs + on-the-fly instance norm) vs the oracle."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.encoder_hip import HipEncoder
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from oracle import cer_oracle as O
    images, _, _, _ = synthetic_scene(size[0], size[1], 2, seed=8)
    model = RAFT(test_mode=True)
    sd = fill_state_dict(model.state_dict(), seed=13)
    model.load_state_dict(sd)
    x = images[0].float() * (2 / 255.0) - 1
    eng = HipEncoder(getattr(model, which), dev)
    with torch.no_grad():
        got = eng.forward_nchw(x.to(dev)).cpu()
        ref = O.encoder(x, sd, which + ".", "instance" if which == "fnet" else "none")
    assert got.shape == ref.shape
    assert rel_l1(got, ref) < 1e-5


@pytest.mark.parametrize("size", [(72, 104), (128, 160), (70, 132), (296, 400)])
@pytest.mark.parametrize("which", ["fnet", "cnet"])
def test_hip_encoder_fp6_correction_form(dev, which, size):
    """Round 6: the producer / consumer convolutions with both correction terms of a tap on ONE e2m3 (FP6) MFMA with a power-of-two scale
    per (pixel | output channel, 16-channel block) - csrc/enc_pc.hip, flags & 8, cer_enc_conv_pack_f6.  Costed on the oracle before it was built
    (tools/experiments/encoder_corr_numerics.py: features 4.4e-5 / context 2.3e-5 relative L1 from fp32); the kernels must land THERE - a lost
    term or a wrong scale byte is 1e-3 (the f16-only product) or worse - be a different arithmetic from the three-term form (the flag took effect)
    and reproduce bit for bit.  Sizes with partial tiles in both directions; (296, 400) has interior AND border units."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.encoder_hip import HipEncoder
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from oracle import cer_oracle as O
    images, _, _, _ = synthetic_scene(size[0], size[1], 2, seed=8)
    model = RAFT(test_mode=True)
    sd = fill_state_dict(model.state_dict(), seed=13)
    model.load_state_dict(sd)
    x = images[0].float() * (2 / 255.0) - 1
    eng = HipEncoder(getattr(model, which), dev)
    with torch.no_grad():
        g3 = eng.forward_nchw(x.to(dev)).cpu()
        eng.f6 = True
        g6 = eng.forward_nchw(x.to(dev)).cpu()
        again = eng.forward_nchw(x.to(dev)).cpu()
        ref = O.encoder(x, sd, which + ".", "instance" if which == "fnet" else "none")
    e3, e6, d = rel_l1(g3, ref), rel_l1(g6, ref), rel_l1(g6, g3)
    print(f"{which} {size}: three-term form {e3:.2e}, FP6-correction form {e6:.2e} from the oracle; {d:.2e} apart")
    assert torch.isfinite(g6).all() and torch.equal(g6, again)
    assert e3 < 1e-5 and 2e-6 < d and e6 < (7e-5 if which == "fnet" else 4e-5)
    assert float((g6 - g3).abs().max() / g3.abs().max()) < 3e-4


@pytest.mark.parametrize("size", [(64, 96), (70, 130), (37, 51), (70, 132), (37, 52), (150, 260)])
@pytest.mark.parametrize("raw", [False, True])
def test_stem_on_matrix_cores(dev, size, raw):
    """7x7 stride-2 stem (core/extractor.py:81,145; raw: with the x * 2/255 - 1 of core/raft.py:40-41 folded in): the MFMA kernel
    (csrc/enc_stem.hip: K padded to 7 x 32, split-f16 single accumulator) and the direct fp32 kernel against an fp64 conv, incl.
    ragged sizes (partial tiles, odd widths) and the per-tile (sum, sum of squares) records of the following instance norm.
    Widths that are multiples of 4 run the round-4 producer / consumer form (16-byte image loads), the others the round-2 kernel."""
    import ctypes
    from cer_mvs_amd import _lib as L
    H, W = size
    N = 3
    lib = L.load()
    w = hashed((32, 3, 7, 7), 401, -0.4, 0.4)
    b = hashed((32,), 402, -0.2, 0.2)
    x = hashed((N, 3, H, W), 403, 0.0, 255.0) if raw else hashed((N, 3, H, W), 403, -1.0, 1.0)
    xn = (x.double() * (2.0 / 255.0) - 1.0) if raw else x.double()
    ref = torch.nn.functional.conv2d(xn, w.double(), b.double(), stride=2, padding=3)               # [N,32,ho,wo]
    ho, wo = ref.shape[2], ref.shape[3]
    ref_cl = ref.permute(0, 2, 3, 1).reshape(N, ho * wo, 32)
    mag = torch.nn.functional.conv2d(xn.abs(), w.double().abs(), b.double().abs(), stride=2, padding=3).permute(0, 2, 3, 1).reshape(N, ho * wo, 32)
    packed = torch.empty(lib.cer_enc_stem_s16_packed_size(), dtype=torch.float16)
    k = ctypes.c_int(0)
    L.check(lib.cer_enc_stem_s16_pack(ctypes.c_void_p(w.contiguous().data_ptr()), ctypes.c_void_p(packed.data_ptr()), ctypes.byref(k)), "pack")
    xd, bd = x.to(dev).contiguous(), b.to(dev)
    outs = {}
    # MFMA
    nt = lib.cer_enc_stem_s16_tiles(ho, wo)
    out = torch.full((N, ho * wo, 32), float("nan"), device=dev)
    part = torch.full((N, nt, 32, 2), float("nan"), device=dev)
    L.check(lib.cer_enc_stem_s16(L.dev_ptr(xd, "x"), L.dev_ptr(packed.to(dev), "w", torch.float16), L.dev_ptr(bd, "b"), L.dev_ptr(out, "out"),
                                 L.dev_ptr(part, "part"), N, H, W, int(raw), int(k.value), L.cur_stream()), "stem_s16")
    outs["mfma"] = (out.cpu(), part.cpu())
    # direct fp32
    nt2 = lib.cer_enc_stem_tiles(ho, wo)
    out2 = torch.full((N, ho * wo, 32), float("nan"), device=dev)
    part2 = torch.full((N, nt2, 32, 2), float("nan"), device=dev)
    wk = w.permute(1, 2, 3, 0).reshape(147, 32).contiguous().to(dev)
    L.check(lib.cer_enc_stem_f32(L.dev_ptr(xd, "x"), L.dev_ptr(wk, "w"), L.dev_ptr(bd, "b"), L.dev_ptr(out2, "out"), L.dev_ptr(part2, "part"),
                                 N, H, W, int(raw), L.cur_stream()), "stem_f32")
    outs["fp32"] = (out2.cpu(), part2.cpu())
    for name, (o, p_) in outs.items():
        assert torch.isfinite(o).all() and torch.isfinite(p_).all(), name
        err = ((o.double() - ref_cl).abs() / mag).max().item()
        assert err < 2e-6, (name, err)                                       # fp32-class: relative to sum |x||w|
        tot = p_.double().sum(1)                                             # [N,32,2]
        assert torch.allclose(tot[..., 0], o.double().sum(1), rtol=1e-5, atol=1e-3), name
        assert torch.allclose(tot[..., 1], (o.double() ** 2).sum(1), rtol=1e-5, atol=1e-3), name
    assert rel_l1(outs["mfma"][0], outs["fp32"][0]) < 1e-6


@pytest.mark.parametrize("size", [(72, 104), (128, 160), (100, 132)])
def test_encoder_head_writes_split_planes_directly(dev, size):
    """features_split (the fnet head's FSPLIT epilogue, csrc/enc_pc.hip) == feat_split(features(...)): the split-f16 operand planes of the
    cost volume bit for bit - reference map and bordered source maps, partial tiles included - and the overflow flag stays clear."""
    from cer_mvs_amd import RAFT, ops
    from cer_mvs_amd.encoder_hip import HipEncoder
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    images, _, _, _ = synthetic_scene(size[0], size[1], 3, seed=8)
    model = RAFT(test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=13))
    eng = HipEncoder(model.fnet, dev)
    x = images[0].float().to(dev)
    N = x.shape[0]
    with torch.no_grad():
        ref, src, h, w = eng.features(x, n_ref=1, raw=True)
        want_ref, want_src = ops.feat_split(ref[0]), ops.feat_split(src)
        f1s = torch.full((h * w, 128), float("nan"), device=dev, dtype=torch.float16)
        f2s = torch.zeros(N - 1, (h + 4) * (w + 4), 128, device=dev, dtype=torch.float16)
        assert eng.features_split(x, f1s, f2s, n_ref=1, raw=True, flag=ops.overflow_flag(dev)) == (h, w)
    assert torch.equal(f1s.view(torch.int16), want_ref.view(torch.int16))
    assert torch.equal(f2s.view(torch.int16), want_src.view(torch.int16))
    assert not ops.check_overflow(dev)


@pytest.mark.parametrize("f6", [False, True])
def test_encoder_engine_batch_invariance_at_tnt_size(dev, f6):
    """BASELINE.json configs[2] size (3840x2160, 16 images per fnet launch): layer-1 activations are 16 x 1080 x 1920 x 32
    floats = 4.2 GB, i.e. element offsets beyond 2^31 bytes.  Instance norm is per image, so the batched launch must
    reproduce, bit for bit, what the LAST image gives alone (an offset overflow would corrupt exactly the late images)."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.encoder_hip import HipEncoder
    from cer_mvs_amd.synthetic import fill_state_dict
    model = RAFT(test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=13))
    eng = HipEncoder(model.fnet, dev)
    eng.f6 = f6
    N, H, W = 16, 2160, 3840
    g = torch.Generator(device="cpu").manual_seed(7)
    small = torch.rand(N, 3, H // 8, W // 8, generator=g) * 2 - 1
    x = torch.nn.functional.interpolate(small, size=(H, W), mode="bilinear", align_corners=False).to(dev)
    x += 0.05 * torch.sin(torch.arange(W, device=dev) * 0.37)[None, None, None, :]
    with torch.no_grad():
        ref_all, src_all, h, w = eng.features(x, n_ref=1)
        _, src_last, _, _ = eng.features(x[[0, N - 1]], n_ref=1)
        _, src_mid, _, _ = eng.features(x[[0, 9]], n_ref=1)
    assert (h, w) == (H // 4, W // 4) and torch.isfinite(src_all).all()
    assert torch.equal(src_all[N - 2], src_last[0])
    assert torch.equal(src_all[8], src_mid[0])
    assert src_all[N - 2].abs().sum() > 0


def test_norm_act_kernels(dev):
    from cer_mvs_amd import ops
    x = hashed((3, 5, 12, 20), 131, -3, 5)
    r = hashed((3, 5, 12, 20), 132, -2, 2)
    xs, rs = ops.plane_stats(x.to(dev)), ops.plane_stats(r.to(dev))
    mean, var = x.mean((2, 3)), x.var((2, 3), unbiased=False)
    assert rel_l1(xs.cpu()[:, 0].view(3, 5), mean) < 1e-6
    assert rel_l1(xs.cpu()[:, 1].view(3, 5), 1 / torch.sqrt(var + 1e-5)) < 1e-6
    inorm = lambda t: F.instance_norm(t, eps=1e-5)
    got = ops.norm_act(x.to(dev), xs, res=r.to(dev), res_stats=rs, relu_a=True, relu_out=True).cpu()
    assert rel_l1(got, F.relu(F.relu(inorm(x)) + inorm(r))) < 1e-6
    got = ops.norm_act(x.to(dev), None, res=r.to(dev), relu_a=True, relu_b=True).cpu()
    assert rel_l1(got, F.relu(x) + F.relu(r)) < 1e-7


def test_update_block_other_aggregations(dev):
    """aggregation = ["mean", "max", "std"] (core/update.py:101-110): the literal UpdateBlock API against the oracle."""
    from cer_mvs_amd.update import UpdateBlock
    from oracle import cer_oracle as O
    h1, w1, V = 12, 20, 4
    agg = ["mean", "max", "std"]
    torch.manual_seed(3)
    ub = UpdateBlock(cascade=[(64, 64, 1), (-1, 320, 1)], dim_net=64, dim_inp=64, aggregation=agg)
    sd = {"update_block." + k: v.detach().clone() for k, v in ub.state_dict().items()}
    net = torch.tanh(hashed((1, 1, 64, h1, w1), 141, -2, 2))
    inp = torch.relu(hashed((1, 1, 64, h1, w1), 142, -1, 2))
    disp = hashed((1, 1, h1, w1), 143, 0.0, 0.0025)
    corr = hashed((1, V, 33, h1, w1), 144, -1.5, 3.0)
    ub = ub.to(dev)
    with torch.no_grad():
        n2, delta = ub(net.to(dev), inp.to(dev), disp.to(dev), corr.to(dev), 1)
        rn, rd = O.update_block(sd, net[0], inp[0], disp, corr[0], 1, aggregation=agg)
    assert rel_l1(n2.cpu()[0], rn) < 1e-5 and rel_l1(delta.cpu(), rd) < 1e-5


def test_inference_driver_writes_reference_format(dev, tmp_path):
    """The caller-side counterpart of inference.py:41-66 end to end: loader tuple -> model -> depth -> PFM file."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd import inference as I
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    images, poses, intr, scale = synthetic_scene(64, 96, 2, seed=5)
    model = RAFT(cascade=[(64, 64, 1), (-1, 320, 1)], test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=2))
    model = model.to(dev)
    loader = [(images, poses, intr, [["rect_001"]], scale)]
    files = I.inference(loader, None, tmp_path, rescale=1, model=model, num_frames=3)
    assert files == [str(tmp_path / "depths" / "rect_001_scale1_nf3.pfm")]
    raw = open(files[0], "rb").read()
    assert raw.startswith(b"Pf\n24 16\n-1.000000\n")
    depth = np.frombuffer(raw[len(b"Pf\n24 16\n-1.000000\n"):], dtype="<f4").reshape(16, 24)[::-1]
    with torch.no_grad():
        disp = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale).cpu().numpy()[0, 0]
    assert np.array_equal(depth, I.disp_to_depth(disp))
    # rescale + crop path (utils/data_utils.py:58-78) keeps running and changes the output size accordingly
    files = I.inference(loader, None, tmp_path, rescale=2, crop=(64, 128), model=model, num_frames=3)
    assert open(files[0], "rb").read().startswith(b"Pf\n32 16\n")


def test_large_configs_run(dev):
    """BASELINE.json configs[4] size (2048x1536, 7 views) with a short cascade: finite output of the right shape, bitwise repeatable."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    images, poses, intr, scale = synthetic_scene(1536, 2048, 7, seed=1)
    model = RAFT(cascade=[(64, 64, 1), (-1, 320, 1)], test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
    model = model.to(dev).eval()
    with torch.no_grad():
        a = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale)
        b = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale)
    assert a.shape == (1, 1, 384, 512) and torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------------------------ end to end
def _run_e2e(dev, golden, name, literal=False, gru_precision="s16f8", enc_precision="auto", cost_precision="auto", info=None):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene, tensor_checksum
    g = golden(name)
    H, W, V = int(g["H"]), int(g["W"]), int(g["V"])
    cascade = [tuple(int(x) for x in c) for c in g["cascade"]]
    images, poses, intr, scale = cached_scene(H, W, V, int(g["scene_seed"]))
    assert tensor_checksum(images) == int(g["images_checksum"])
    model = RAFT(cascade=cascade, test_mode=True, gru_precision=gru_precision, enc_precision=enc_precision, cost_precision=cost_precision)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(g["weight_seed"])))
    model = model.to(dev).eval()
    if info is not None:
        info["model"] = model
    before = images.clone()
    with torch.no_grad():
        if literal:
            disp = model._forward_literal(images.to(dev), poses.to(dev), intr.to(dev), scale, False)
        else:
            disp = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale)
    assert torch.equal(images, before)
    ref = torch.from_numpy(g["disp"])
    assert disp.shape == ref.shape
    d = disp.cpu()
    depth, depth_ref = torch.where(d == 0, d, 1 / d), torch.where(ref == 0, ref, 1 / ref)
    return rel_l1(d, ref), rel_l1(depth, depth_ref)


def test_end_to_end_tiny(dev, golden):
    e_disp, e_depth = _run_e2e(dev, golden, "e2e_tiny")
    print(f"e2e_tiny rel-L1 disp {e_disp:.3e} depth {e_depth:.3e}")
    assert e_disp < TOL and e_depth < TOL


def test_end_to_end_tiny_literal_api(dev, golden):
    e_disp, e_depth = _run_e2e(dev, golden, "e2e_tiny", literal=True)
    print(f"e2e_tiny (literal) rel-L1 disp {e_disp:.3e} depth {e_depth:.3e}")
    assert e_disp < TOL and e_depth < TOL


@pytest.mark.parametrize("gru_precision", ["s16f6", "s16f8", "s16", "f16x3", "fp32"])
def test_end_to_end_cfg1(dev, golden, gru_precision):
    """BASELINE.json configs[0] shape: 640x480, 1 ref + 2 src views, 4 GRU iterations."""
    e_disp, e_depth = _run_e2e(dev, golden, "e2e_cfg1", gru_precision=gru_precision)
    print(f"e2e_cfg1[{gru_precision}] rel-L1 disp {e_disp:.3e} depth {e_depth:.3e}")
    assert e_disp < TOL and e_depth < TOL
    # tighter than the bar, per arithmetic: a wrong scale or a lost correction term in one of the forms must not hide under 1e-4
    # (measured: s16f8 3.9e-6 / 4.1e-6 - the e4m3 correction terms; s16f6, round 6: e2m3 with block scales, costed at 5.5e-6 by
    # tools/experiments/fp8_correction_numerics.py and gated at 1.5e-5 by VERDICT r5; the all-f16 and fp32 forms 1.9e-7 ... 2.2e-7)
    assert max(e_disp, e_depth) < {"s16f8": 2e-5, "s16f6": 1.5e-5}.get(gru_precision, 2e-6)


@pytest.mark.parametrize("gru_precision", ["s16f8", "s16"])
def test_end_to_end_cfg1_encoders_in_fp6_form(dev, golden, gru_precision):
    """enc_precision="f6" against the reference's own output at configs[0]: with the update block fp32-class ("s16") the figure is the encoders'
    contribution alone (costed at 7e-6 by tools/experiments/encoder_corr_numerics.py), with "s16f8" it is what the default "auto" form runs."""
    e_disp, e_depth = _run_e2e(dev, golden, "e2e_cfg1", gru_precision=gru_precision, enc_precision="f6")
    print(f"e2e_cfg1[{gru_precision} + encoders f6] rel-L1 disp {e_disp:.3e} depth {e_depth:.3e}")
    assert 1e-6 < max(e_disp, e_depth) < 2.5e-5


def test_end_to_end_cfg1_two_term_cost_volume(dev, golden):
    """cost_precision="x2" alone (update block and encoders fp32-class) against the reference's own output at configs[0]: the contribution of the
    source features' f16 rounding in the cost volume (costed on the oracle at 5-6e-6 before it was built)."""
    e_disp, e_depth = _run_e2e(dev, golden, "e2e_cfg1", gru_precision="s16", enc_precision="f16x3", cost_precision="x2")
    print(f"e2e_cfg1[s16, two-term cost volume] rel-L1 disp {e_disp:.3e} depth {e_depth:.3e}")
    assert 5e-7 < max(e_disp, e_depth) < 2e-5


def test_end_to_end_cfg2_default_auto_form(dev, golden):
    """The bench workload in the DEFAULT arithmetic: gru_precision="auto" calibrates on this input (reference form, then candidates) and returns
    the kept form's result - whatever it keeps must sit inside a quarter of the bar from the reference's own output."""
    info = {}
    e_disp, e_depth = _run_e2e(dev, golden, "e2e_cfg2", gru_precision="auto", info=info)
    m = info["model"]
    print(f"e2e_cfg2[auto -> {m.auto_choice}, calibration {m.auto_error:.2e}] rel-L1 disp {e_disp:.3e} depth {e_depth:.3e}")
    assert m.auto_choice in m._auto_forms() and max(e_disp, e_depth) < 2.5e-5


def test_end_to_end_cfg2_bench_workload(dev, golden):
    """BASELINE.json configs[1] - the bench workload itself: 1600x1184, 10 source views, cascade (64,64,16),(-1,320,16) =
    32 GRU iterations, same scene / weight seeds as bench.py - against the reference's own output on it
    (tools/gen_golden.py --only e2e_cfg2: 2.5 minutes of the reference on 8 CPU cores)."""
    e_disp, e_depth = _run_e2e(dev, golden, "e2e_cfg2")
    print(f"e2e_cfg2 rel-L1 disp {e_disp:.3e} depth {e_depth:.3e}")
    assert e_disp < TOL and e_depth < TOL


@pytest.mark.parametrize("size,V", [((100, 132), 2), ((68, 148), 3), ((52, 76), 1), ((32, 48), 2), ((36, 20), 1), ((20, 260), 2)])
def test_end_to_end_ragged_sizes_match_oracle(dev, size, V):
    """Whole forward at image sizes whose feature maps (25 x 33, 17 x 37, 13 x 19) are multiples of none of the kernels' tiles
    (2 x 16 m-tiles, 8 / 16-row conv tiles, 64-pixel lookup tiles, 8 x 32 stem tiles) - down to feature maps smaller than one
    tile (8 x 12, 9 x 5, 5 x 65): every kernel's partial-tile path in one run, against the CPU oracle (which is pinned to the reference captures at the regular sizes)."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from oracle import cer_oracle as O
    H, W = size
    cascade = [(64, 64, 2), (-1, 320, 2)]
    images, poses, intr, scale = synthetic_scene(H, W, V, seed=21)
    model = RAFT(cascade=cascade, test_mode=True)
    sd = fill_state_dict(model.state_dict(), seed=9)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    with torch.no_grad():
        got = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale).cpu()
        ref = O.raft_forward({k: v.cpu() for k, v in sd.items()}, images, poses, intr, scale, cascade=cascade)
    assert got.shape == ref.shape == (1, 1, H // 4, W // 4)
    assert rel_l1(got, ref) < TOL


def test_non_default_feature_width_runs_on_the_general_kernels(dev):
    """`dim_fmap` is a constructor argument of the reference's RAFT (core/raft.py:14-30).  The producer / consumer encoder
    engine has a 64 -> 64 feature head only and the epipolar-line cost volume 64-channel operands only: a model with dim_fmap = 128 must
    take the tiled engine's head (cer_enc_pc_supported is consulted) and the wave-per-pixel walk, and still match the oracle."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.encoder_hip import HipEncoder
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from oracle import cer_oracle as O
    H, W, V = 72, 104, 2
    cascade = [(64, 64, 2), (-1, 320, 2)]
    images, poses, intr, scale = synthetic_scene(H, W, V, seed=27)
    model = RAFT(cascade=cascade, dim_fmap=128, test_mode=True)
    sd = fill_state_dict(model.state_dict(), seed=11)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    eng = HipEncoder(model.fnet, dev)
    assert eng.pc_trunk and not eng.pc_head[1] and not eng.supports_split_head()
    x = images[0].float() * (2 / 255.0) - 1
    with torch.no_grad():
        f = eng.forward_nchw(x.to(dev)).cpu()
        assert rel_l1(f, O.encoder(x, sd, "fnet.", "instance")) < 1e-5
        got = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale).cpu()
        ref = O.raft_forward({k: v.cpu() for k, v in sd.items()}, images, poses, intr, scale, cascade=cascade)
    assert rel_l1(got, ref) < TOL


@pytest.mark.parametrize("size,V,G", [((100, 132), 2, 2), ((132, 100), 3, 3), ((68, 148), 1, 2)])
def test_slab_sharded_forward_at_ragged_sizes(dev, size, V, G):
    """Row slabs whose heights (25 / 3 ranks, 33 / 3, 17 / 2) and widths fit no tile size: the sharded forward must reproduce the
    single-GPU forward (uneven slabs, halo rows inside partial m-tile rows, more ranks than views)."""
    from cer_mvs_amd import RAFT, slab
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    H, W = size
    images, poses, intr, scale = synthetic_scene(H, W, V, seed=23)
    model = RAFT(cascade=[(64, 64, 2), (-1, 320, 2)], test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=10))
    model = model.to(dev).eval()
    assert slab.can_shard(H // 4, G)
    with torch.no_grad():
        single = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale)
        sharded = slab.sharded_forward(model, images.to(dev), poses.to(dev), intr.to(dev), scale, slab.LocalExchange(G))
    assert sharded.shape == single.shape
    assert rel_l1(sharded.cpu(), single.cpu()) < 1e-5


@pytest.mark.parametrize("name", ["e2e_blended", "e2e_tnt"])
def test_end_to_end_other_baseline_configs(dev, golden, name):
    """BASELINE.json configs[4] (BlendedMVS 2048x1536, 7 source views) and configs[2] (Tanks&Temples 3840x2160, 15 source
    views), 16 GRU iterations each, against the reference's own output (tools/gen_golden.py --only e2e_blended | e2e_tnt:
    4 and 26 minutes of the reference on 8 CPU cores)."""
    e_disp, e_depth = _run_e2e(dev, golden, name)
    print(f"{name} rel-L1 disp {e_disp:.3e} depth {e_depth:.3e}")
    assert e_disp < TOL and e_depth < TOL


@pytest.mark.parametrize("name,G", [("e2e_tiny", 2), ("e2e_cfg1", 2), ("e2e_cfg1", 3), ("e2e_cfg1", 8), ("e2e_cfg2", 8), ("e2e_cfg2", 4),
                                    ("e2e_blended", 8), ("e2e_tnt", 8)])
def test_slab_sharded_forward_matches_reference_capture(dev, golden, name, G):
    """The multi-GPU row-slab algorithm (slab.py) with G ranks simulated in one process: same kernels, same halo
    bookkeeping, only the collective is replaced by list passing.  Must equal the captures like the 1-GPU path."""
    from cer_mvs_amd import RAFT, slab
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    g = golden(name)
    H, W, V = int(g["H"]), int(g["W"]), int(g["V"])
    cascade = [tuple(int(x) for x in c) for c in g["cascade"]]
    images, poses, intr, scale = cached_scene(H, W, V, int(g["scene_seed"]))
    model = RAFT(cascade=cascade, test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(g["weight_seed"])))
    model = model.to(dev).eval()
    assert slab.can_shard(H // 4, G)
    with torch.no_grad():
        single = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale)
        sharded = slab.sharded_forward(model, images.to(dev), poses.to(dev), intr.to(dev), scale, slab.LocalExchange(G))
    ref = torch.from_numpy(g["disp"])
    assert sharded.shape == ref.shape
    assert rel_l1(sharded.cpu(), ref) < TOL
    assert rel_l1(sharded.cpu(), single.cpu()) < 1e-5


def test_slab_forward_over_rccl_single_rank(dev, golden):
    """The torch.distributed (nccl = RCCL) exchange layer with a 1-rank group on the GPU: every collective of the sharded
    forward runs through RCCL with real device tensors (the box has one GPU; multi-rank logic is covered by the simulated
    ranks above and the gloo tests)."""
    import os
    import torch.distributed as dist
    from cer_mvs_amd import RAFT, slab
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    g = golden("e2e_tiny")
    H, W, V = int(g["H"]), int(g["W"]), int(g["V"])
    cascade = [tuple(int(x) for x in c) for c in g["cascade"]]
    images, poses, intr, scale = synthetic_scene(H, W, V, seed=int(g["scene_seed"]))
    model = RAFT(cascade=cascade, test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(g["weight_seed"])))
    model = model.to(dev).eval()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    import socket
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))                              # a free port: the suite may run beside other jobs
    port = sock.getsockname()[1]
    sock.close()
    os.environ["MASTER_PORT"] = str(port)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        with torch.no_grad():
            out = slab.sharded_forward(model, images.to(dev), poses.to(dev), intr.to(dev), scale, slab.DistExchange(dist.group.WORLD))
    finally:
        if created:
            dist.destroy_process_group()
    assert rel_l1(out.cpu(), torch.from_numpy(g["disp"])) < TOL


@pytest.mark.parametrize("gru_precision", ["s16f6", "s16f8", "s16", "f16x3", "fp32"])
def test_odd_image_size_vs_oracle(dev, gru_precision):
    """h1, w1 not multiples of the 8x16 conv tile, V = 1; every arithmetic mode of the update block."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from oracle import cer_oracle as O
    cascade = [(64, 64, 2), (-1, 320, 1)]
    images, poses, intr, scale = synthetic_scene(76, 108, 1, seed=6)
    model = RAFT(cascade=cascade, test_mode=True, gru_precision=gru_precision)
    sd = fill_state_dict(model.state_dict(), seed=12)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    with torch.no_grad():
        disp = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale).cpu()
        ref = O.raft_forward(sd, images, poses, intr, scale, cascade=cascade)
    assert rel_l1(disp, ref) < TOL


def test_full_size_properties(dev):
    """BASELINE.json configs[1] size (1600x1184, 10 source views) is too slow for the CPU oracle inside the test
    budget, so check size-independent properties at full size: finiteness, determinism (bitwise), invariance to
    a permutation of the source views (view-mean is symmetric; fp32 sum order changes -> tolerance), and
    linearity of the folded volume in fmap2."""
    from cer_mvs_amd import RAFT, ops
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    H, W, V = 1184, 1600, 10
    cascade = [(64, 64, 2), (-1, 320, 2)]
    images, poses, intr, scale = synthetic_scene(H, W, V, seed=3)
    model = RAFT(cascade=cascade, test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
    model = model.to(dev).eval()
    with torch.no_grad():
        a = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale)
        b = model(images.to(dev), poses.to(dev), intr.to(dev), scale=scale)
        perm = [0] + list(range(V, 0, -1))
        c = model(images[:, perm].to(dev), poses[:, perm].to(dev), intr[:, perm].to(dev), scale=scale)
    assert a.shape == (1, 1, H // 4, W // 4)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert rel_l1(c.cpu(), a.cpu()) < TOL
    # linearity: build(f2a + f2b) == build(f2a) + build(f2b)
    h1, w1, P, C, D = 296, 400, 296 * 400, 64, 64
    f1 = torch.randn(P, C, device=dev) * 0.1
    from cer_mvs_amd.corr import fmaps_to_nhwc
    f2a = fmaps_to_nhwc(torch.randn(2, C, h1, w1, device=dev) * 0.8, border=2)
    f2b = fmaps_to_nhwc(torch.randn(2, C, h1, w1, device=dev) * 0.8, border=2)
    Pij = torch.eye(4).repeat(2, 1, 1)
    Pij[0, 0, 3], Pij[1, 0, 3] = 9000.0, -14000.0
    Pij = Pij.to(dev)
    d0 = torch.zeros(P, device=dev)
    va, _ = ops.cost_build(f1, f2a, Pij, d0, D, 0.0025 / 64, True, h1, w1, 3, fold=True)
    vb, _ = ops.cost_build(f1, f2b, Pij, d0, D, 0.0025 / 64, True, h1, w1, 3, fold=True)
    vab, _ = ops.cost_build(f1, f2a + f2b, Pij, d0, D, 0.0025 / 64, True, h1, w1, 3, fold=True)
    assert rel_l1((va + vb).cpu(), vab.cpu()) < 1e-5


# ------------------------------------------------------------------------------------ arithmetic form of the update block's loop
_FORM_CASCADE = [(64, 64, 2), (-1, 320, 2)]


def _form_model(dev, gru_precision, sd):
    from cer_mvs_amd import RAFT
    model = RAFT(cascade=_FORM_CASCADE, test_mode=True, gru_precision=gru_precision)
    model.load_state_dict(sd)
    return model.to(dev).eval()


def _form_weights(edit=None):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    sd = fill_state_dict(RAFT(cascade=_FORM_CASCADE, test_mode=True).state_dict(), seed=9)
    if edit is not None:
        edit(sd)
    return sd


def _form_scene(dev):
    images, poses, intr, scale = cached_scene(64, 96, 3, 4)
    return images.to(dev), poses.to(dev), intr.to(dev), scale


def test_unscalable_update_weights_switch_to_f16x3(dev):
    """Update-block weights without a shared split-f16 scale (cer_conv3x3_s16_scale refuses them): the s16 forward warns, leaves the
    update block on the f16x3 kernels and computes exactly what a gru_precision="f16x3" model with the same weights computes."""
    import ctypes
    from cer_mvs_amd import _lib as L, ops

    def shrink(sd):          # the hidden-state source of the z|r conv (net | inp | disp49 | corr), both gates
        for k in ("update_block.gru.convz.weight", "update_block.gru.convr.weight"):
            sd[k][:, :64] *= 2.0 ** -30
    sd = _form_weights(shrink)
    wzr = torch.cat([sd["update_block.gru.convz.weight"], sd["update_block.gru.convr.weight"]], 0)
    loop_srcs = wzr[:, list(range(64)) + list(range(128, 241))].contiguous()
    I3 = ctypes.c_int * 3
    assert L.load().cer_conv3x3_s16_scale(ctypes.c_void_p(loop_srcs.data_ptr()), 128, 177, I3(64, 49, 64), I3(2, 1, 2),
                                          I3(L.S16_UNIT, L.S16_DISP, L.S16_RELU), 3) < -1000
    s16, f16 = _form_model(dev, "s16", sd), _form_model(dev, "f16x3", sd)
    scene = _form_scene(dev)
    ops.check_overflow(dev)
    with torch.no_grad():
        with pytest.warns(UserWarning, match="gru_precision='f16x3'"):
            out = s16(*scene[:3], scale=scene[3]).clone()
        assert s16.update_block.conv_mode == "f16x3"
        want = f16(*scene[:3], scale=scene[3])
    assert torch.isfinite(out).all() and torch.equal(out, want)


def test_overflow_fallback_repeats_the_forward_in_f16x3(dev):
    """overflow_policy="fallback": a ReLU-class activation beyond 4094 (one channel of the corr encoder's output at 5000) sets flag bit 4
    on the s16 kernels; the forward then repeats on the f16x3 kernels, returns exactly what a gru_precision="f16x3" model returns,
    and leaves the update block on "s16" and the flag clear."""
    from cer_mvs_amd import ops

    def hot(sd):
        sd["update_block.corr_encoder.0.bias"][0] = 5000.0
    sd = _form_weights(hot)
    s16, f16 = _form_model(dev, "s16", sd), _form_model(dev, "f16x3", sd)
    scene = _form_scene(dev)
    ops.check_overflow(dev)
    with torch.no_grad():
        s16.overflow_policy = "ignore"
        s16(*scene[:3], scale=scene[3])
        assert ops.check_overflow(dev) & 4
        s16.overflow_policy = "fallback"
        out = s16(*scene[:3], scale=scene[3]).clone()
        assert s16.update_block.conv_mode == "s16" and ops.check_overflow(dev) == 0
        want = f16(*scene[:3], scale=scene[3])
    assert torch.isfinite(out).all() and torch.equal(out, want)


@pytest.mark.parametrize("gru_precision", ["s16", "f16x3", "fp32"])
def test_update_loop_packs_only_its_own_form(dev, monkeypatch, gru_precision):
    """A fast-path forward packs the update block's weights for its own arithmetic form only: no PackedConv3x3 (the general kernels'
    packs) on the default s16 path, no PackedConvS16 in the "f16x3" and "fp32" forms - six convs per cascade stage either way."""
    from cer_mvs_amd import ops
    built = {"PackedConv3x3": 0, "PackedConvS16": 0}
    for name in built:
        def counted(self, *a, _init=getattr(ops, name).__init__, _name=name, **k):
            built[_name] += 1
            _init(self, *a, **k)
        monkeypatch.setattr(getattr(ops, name), "__init__", counted)
    model = _form_model(dev, gru_precision, _form_weights())
    scene = _form_scene(dev)
    with torch.no_grad():
        out = model(*scene[:3], scale=scene[3])
    assert torch.isfinite(out).all()
    if gru_precision == "s16":
        assert built == {"PackedConv3x3": 0, "PackedConvS16": 6 * len(_FORM_CASCADE)}
    else:
        assert built == {"PackedConv3x3": 6 * len(_FORM_CASCADE), "PackedConvS16": 0}
