"""GPU tests of the training step's HIP backend (csrc/train_ops.hip, cer_mvs_amd/train.py): the train-mode lookup and its adjoint
against the grid_sample / avg_pool2d form, the loss's upsample and its adjoint against F.interpolate, the training row and two
optimiser steps against captures of the reference itself, and a whole step under torch.use_deterministic_algorithms(True)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, REPO, cached_scene, rel_l1
from test_oracle_golden import hashed

pytestmark = pytest.mark.gpu

TRAIN_GRADS = ("fnet.conv1.weight", "fnet.conv2.weight", "cnet.conv2.weight", "update_block.gru.convz.weight",
               "update_block.corr_encoder.0.weight", "update_block.delta0.0.weight", "update_block.delta1.2.weight")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _blocks(dev, D, shift, L, r, h=13, w=21, V=3):
    """Two TrainCorrBlocks (torch / hip) over the same DirectCorr volume: P = 273 pixels (not a multiple of the 64-pixel block)."""
    from cer_mvs_amd.projective import pij_matrices
    from cer_mvs_amd.train import TrainCorrBlock
    _, poses, intr, _ = cached_scene(4 * h, 4 * w, V, 2)
    intr = intr.clone()
    intr[:, :, :2] /= 4
    Pij = pij_matrices(poses[0], intr[0], [0] * V, list(range(1, V + 1))).to(dev)
    fmaps = hashed((1, V + 1, 64, h, w), 501 + D).to(dev)
    incre = 0.0025 / 64
    d_in = hashed((1, 1, h, w), 502, 0.0, 0.0025).to(dev)
    blk_t = TrainCorrBlock(fmaps, Pij, D, incre, d_in, shift, L, r, backend="torch")
    blk_h = TrainCorrBlock(fmaps, Pij, D, incre, d_in, shift, L, r, backend="hip")
    # disparities around the origin: c = (disp - origin)/incre + D//2 from -0.75 D (clamped at 0) to 1.6 D (taps partly and wholly past
    # the end of every level)
    disp = (blk_t.origin.view(1, 1, h, w) + hashed((1, 1, h, w), 503, -1.25 * D, 1.1 * D).to(dev) * incre).contiguous()
    return blk_t, blk_h, disp, incre


LOOKUP_CASES = [(64, True, 3, 5), (44, False, 3, 5), (64, True, 4, 7), (44, False, 2, 3)]


@pytest.mark.parametrize("D,shift,L,r", LOOKUP_CASES)
def test_train_lookup_forward_matches_grid_sample(dev, D, shift, L, r):
    blk_t, blk_h, disp, _ = _blocks(dev, D, shift, L, r)
    with torch.no_grad():
        a = blk_t(disp)
        b = blk_h(disp)
    assert a.shape == b.shape == (1, 3, L * (2 * r + 1), 13, 21)
    c = ((disp.view(-1) - blk_t.origin.view(-1)) / blk_t.incre + D // 2)
    assert float(c.min()) < 0 and float(c.max()) > D + r                   # the clamp and the taps past the end are exercised
    assert float(a.abs().sum()) > 0 and bool((a == 0).any())
    assert rel_l1(b.cpu(), a.cpu()) <= 1e-6


def _torch_form(vol, blk_t, disp, L):
    """The grid_sample + avg_pool2d form (TrainCorrBlock, backend="torch") on a [V,D,P] volume that autograd can differentiate."""
    V, D, P = vol.shape
    c = vol.view(V, D, blk_t.h1, blk_t.w1).permute(0, 2, 3, 1).reshape(V * P, 1, 1, D)
    pyr = [c]
    for _ in range(L - 1):
        c = F.avg_pool2d(c, [1, 2], stride=[1, 2])
        pyr.append(c)
    blk_t.corr_pyramid = pyr
    return blk_t(disp)


@pytest.mark.parametrize("D,shift,L,r", LOOKUP_CASES)
def test_train_lookup_backward_matches_autograd(dev, D, shift, L, r):
    from cer_mvs_amd.train import TrainLookup
    blk_t, blk_h, disp, incre = _blocks(dev, D, shift, L, r)
    vol0 = blk_h.volume.detach().clone()
    g = hashed((1, 3, L * (2 * r + 1), 13, 21), 504).to(dev)
    vt = vol0.clone().requires_grad_(True)
    (_torch_form(vt, blk_t, disp, L) * g).sum().backward()
    z = disp.reshape(-1).contiguous()
    grads = []
    for _ in range(3):
        vh = vol0.clone().requires_grad_(True)
        out = TrainLookup.apply(vh, blk_h.origin_flat, z, D, incre, L, r)
        (out.view_as(g) * g).sum().backward()
        grads.append(vh.grad)
    assert rel_l1(grads[0].cpu(), vt.grad.cpu()) <= 1e-5
    assert all(torch.equal(grads[0], x) for x in grads[1:])
    with pytest.raises(RuntimeError, match="must not require grad"):
        TrainLookup.apply(vol0, blk_h.origin_flat, z.clone().requires_grad_(True), D, incre, L, r)


@pytest.mark.parametrize("n,h,w,H,W", [(16, 16, 24, 64, 96), (1, 8, 12, 64, 96), (3, 13, 21, 50, 77), (2, 1, 7, 5, 30),
                                       (2, 6, 7, 1, 30), (16, 33, 45, 132, 180)])
def test_upsample_ac_matches_interpolate(dev, n, h, w, H, W):
    from cer_mvs_amd.train import UpsampleAC
    x = hashed((n, h, w), 505 + h, 0.0, 0.003).to(dev)
    g = hashed((n, H, W), 506 + H).to(dev)
    xt = x.clone().requires_grad_(True)
    ref = F.interpolate(xt[:, None], [H, W], mode="bilinear", align_corners=True)[:, 0]
    (ref * g).sum().backward()
    outs, grads = [], []
    for _ in range(3):
        xh = x.clone().requires_grad_(True)
        out = UpsampleAC.apply(xh, H, W)
        (out * g).sum().backward()
        outs.append(out.detach())
        grads.append(xh.grad)
    assert rel_l1(outs[0].cpu(), ref.detach().cpu()) <= 1e-6
    assert rel_l1(grads[0].cpu(), xt.grad.cpu()) <= 1e-5
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and all(torch.equal(grads[0], x_) for x_ in grads[1:])


def _train_model(dev, g, **kw):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    cascade = [tuple(int(x) for x in c) for c in g["cascade"]]
    model = RAFT(cascade=cascade, test_mode=False, **kw)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(g["weight_seed"])))
    images, poses, intr, scale = cached_scene(int(g["H"]), int(g["W"]), int(g["V"]), int(g["scene_seed"]))
    return model.to(dev).train(), (images.to(dev), poses.to(dev), intr.to(dev)), scale


def test_training_row_hip_backend_matches_reference_capture(dev, golden):
    """The training row with train_backend="hip" (HIP lookup + its adjoint, HIP upsample + its adjoint) against the reference's own
    capture (tests/golden/train_tiny.npz), at the bars of test_train_gpu.py::test_training_row_matches_reference_capture."""
    from cer_mvs_amd.train import sequence_loss
    g = golden("train_tiny")
    model, inputs, scale = _train_model(dev, g, train_backend="hip")
    preds = model(*inputs, scale=scale)
    want = torch.from_numpy(g["predictions"])
    assert len(preds) == want.shape[0]
    for i, p_ in enumerate(preds):
        assert rel_l1(p_.detach().cpu(), want[i]) < 1e-4, i
    gt = torch.from_numpy(g["gt"]).to(dev)
    loss, metrics = sequence_loss(list(preds), gt, gradual_weight=float(g["gradual_weight"]), backend="hip")
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    loss.backward()
    params = dict(model.named_parameters())
    errs = {}
    for name in TRAIN_GRADS:
        grad = params[name].grad.detach().reshape(-1).cpu()
        ref = torch.from_numpy(g["grad_" + name])
        sub = grad if grad.numel() == ref.numel() else grad[::7]
        errs[name] = rel_l1(sub, ref)
        assert errs[name] < 1e-3, (name, errs[name])
    print("gradient rel-L1 vs the reference capture:", {k: f"{v:.2e}" for k, v in errs.items()})


def test_train_step_matches_reference_capture(dev, golden):
    """Two train_steps (backend="hip") against two iterations of the reference's own loop body (tests/golden/train_step_tiny.npz:
    the reference's fetch_optimizer, GradScaler, clip_grad_norm_(1.0); captured on a CPU torch, where GradScaler disables itself).
    On the GPU the scaler is live: scaling the loss by a power of two and unscaling the gradients is exact barring overflow (which
    would skip the step: the learning-rate and update checks would fail), so the two runs compute the same step.

    Bars.  Learning rates: equal (the same OneCycleLR arithmetic).  Pre-clip norms and losses: 1e-4 relative.  Parameter updates
    (after - before) over the two steps: AdamW's first steps are close to -lr * sign(g) whatever |g| is, so the update of an element does
    not scale with its gradient: a relative gradient error d becomes an update error of about d * |g| / |m| (m: Adam's first moment),
    which is large where |g| is near eps = 1e-8 and where the second step's moment nearly cancels (0.9 * 0.1 * g1 ~ -0.1 * g2), and an
    element whose gradient is within its error of zero can take the opposite sign (up to ~2 lr).  Measured: the training row's
    gradients agree with the reference to <= 1.4e-6 relative L1 on these parameters (fnet.conv1.weight, the worst; the others
    <= 3e-7: test_training_row_hip_backend_matches_reference_capture prints them), and the two-step update of fnet.conv1.weight
    to 1.5e-3 with no element of opposite sign - an amplification of ~1e3 by the normalised steps (the other six tensors' updates agree
    to <= 7e-7).  The bar is that amplification of
    the worst gradient agreement with a margin of ~3: 5e-3 relative L1 per tensor, and at most 0.5 % of the elements of opposite
    sign.  A skipped step, a wrong learning rate or a wrong step count give >= 5e-3 on every tensor (and fail the lr check)."""
    from cer_mvs_amd.train import fetch_optimizer, train_step
    g = golden("train_step_tiny")
    assert not bool(g["scaler_enabled"])
    model, (images, poses, intr), _ = _train_model(dev, g, train_backend="hip")
    params = dict(model.named_parameters())
    before = {n: params[n].detach().clone() for n in TRAIN_GRADS}
    optimizer, scheduler = fetch_optimizer(model, num_steps=int(g["num_steps"]))
    scaler = torch.amp.GradScaler("cuda", enabled=True)
    depths = torch.from_numpy(g["depths"]).to(dev)
    lrs, norms, losses = [], [], []
    for _ in range(2):
        loss, metrics = train_step(model, optimizer, scheduler, scaler, images, depths, poses, intr, float(g["gradual_weight"]))
        lrs.append(scheduler.get_last_lr()[0])
        norms.append(metrics["grad_norm"])
        losses.append(float(loss))
    assert scaler.get_scale() == 65536.0 * 1.0                      # no overflow skipped a step (the growth interval is 2000 steps)
    assert lrs == [float(x) for x in g["lr"]]
    for a, b in zip(norms, g["grad_norm"]):
        assert abs(a - float(b)) <= 1e-4 * float(b), (norms, g["grad_norm"])
    for a, b in zip(losses, g["loss"]):
        assert abs(a - float(b)) <= 1e-4 * abs(float(b)), (losses, g["loss"])
    report = {}
    for name in TRAIN_GRADS:
        upd = (params[name].detach() - before[name]).reshape(-1)[::int(g["stride_" + name])].cpu()
        ref = torch.from_numpy(g["upd_" + name])
        assert upd.numel() == ref.numel(), name
        err = rel_l1(upd, ref)
        flips = float(((upd * ref) < 0).float().mean())
        report[name] = (err, flips)
    print("update rel-L1 / opposite-sign share:", {k: (f"{e:.2e}", f"{f:.2e}") for k, (e, f) in report.items()})
    for name, (err, flips) in report.items():
        assert err <= 5e-3 and flips <= 5e-3, (name, err, flips)


_CHILD = r"""
import json, sys
sys.path.insert(0, REPO)
import numpy as np
import torch
torch.use_deterministic_algorithms(True)
from cer_mvs_amd import RAFT
from cer_mvs_amd.projective import pij_matrices
from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
from cer_mvs_amd.train import TrainCorrBlock, fetch_optimizer, sequence_loss, train_step

dev = torch.device("cuda:0")
g = np.load(GOLDEN + "/train_step_tiny.npz")
cascade = [tuple(int(x) for x in c) for c in g["cascade"]]
H, W, V = int(g["H"]), int(g["W"]), int(g["V"])
images, poses, intr, _ = synthetic_scene(H, W, V, seed=int(g["scene_seed"]))
depths = torch.from_numpy(g["depths"]).to(dev)


def steps():
    model = RAFT(cascade=cascade, test_mode=False, train_backend="hip")
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(g["weight_seed"])))
    model = model.to(dev).train()
    opt, sch = fetch_optimizer(model, num_steps=int(g["num_steps"]))
    scaler = torch.amp.GradScaler("cuda", enabled=True)
    losses = []
    for _ in range(2):
        loss, _m = train_step(model, opt, sch, scaler, images.to(dev), depths, poses.to(dev), intr.to(dev), float(g["gradual_weight"]))
        losses.append(float(loss))
    return losses, {n: p.detach().clone() for n, p in model.named_parameters()}


def corr_grad():
    h, w = H // 4, W // 4
    gen = torch.Generator().manual_seed(7)
    fmaps = torch.randn(1, V + 1, 64, h, w, generator=gen).to(dev).requires_grad_(True)
    head = torch.randn(3 * 11, generator=gen).to(dev).view(1, 1, 33, 1, 1)
    k = intr.clone()
    k[:, :, :2] /= 4
    Pij = pij_matrices(poses[0], k[0], [0] * V, list(range(1, V + 1))).to(dev)
    disp = torch.full((1, 1, h, w), 0.0015, device=dev)
    blk = TrainCorrBlock(fmaps, Pij, 64, 0.0025 / 64, disp, True, 3, 5, backend="hip")
    preds = []
    for _ in range(3):
        frames = blk(disp.detach())
        disp = disp.detach() + 1e-5 * (frames * head).sum(dim=(1, 2)).view(1, 1, h, w)
        preds.append(disp)
    gt = torch.full((1, 1, H, W), 0.0016, device=dev)
    loss, _m = sequence_loss(preds, gt, gradual_weight=0.3, backend="hip")
    loss.backward()
    return fmaps.grad.detach().clone()


l1, p1 = steps()
l2, p2 = steps()
c1, c2 = corr_grad(), corr_grad()
differ = sorted(n for n in p1 if not torch.equal(p1[n], p2[n]))
print(json.dumps({"losses": [l1, l2], "finite": all(bool(torch.isfinite(t).all()) for t in p1.values()),
                  "params_differ": differ, "corr_grad_identical": bool(torch.equal(c1, c2)),
                  "corr_grad_nonzero": float(c1.abs().sum()) > 0}))
"""


def test_train_step_runs_in_deterministic_mode():
    """Two train_steps under torch.use_deterministic_algorithms(True), in a fresh child process (the flag must not leak into other
    tests).  The grid_sample and upsample backwards of the torch backend raise there; the HIP backend's do not.  The correlation
    subgraph (DirectCorr -> TrainLookup -> a fixed linear head -> sequence_loss, HIP backend) gives bit-identical feature gradients
    over two runs, and so do the whole steps' parameters (MIOpen's convolutions included: DESIGN.md 3d)."""
    env = dict(os.environ)
    env["CUBLAS_WORKSPACE_CONFIG"] = ":4096:8"
    code = "REPO = %r\nGOLDEN = %r\n" % (REPO, GOLDEN) + _CHILD
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-4000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print(out)
    assert out["finite"] and out["corr_grad_nonzero"]
    assert out["corr_grad_identical"]
    assert out["losses"][0] == out["losses"][1]
    assert out["params_differ"] == [], out["params_differ"]
