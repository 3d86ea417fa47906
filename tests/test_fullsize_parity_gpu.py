"""Element-wise parity of one GRU iteration's kernels and of the cost volume AT PRODUCTION SHAPES (run on the GPU box: pytest -m gpu).

The kernel tests of tests/test_conv_s16_gpu.py and tests/test_hip_parity.py stop at 70 x 150 pixels and mostly force a tile height; at
the sizes the project is benchmarked at the only comparison was a global mean (rel_l1 < 1e-4) against a capture, which a wrong 8 x 16
tile, a wrong last row or a wrong segment seam passes (tests/test_parity_check_cpu.py shows it).  Here every launch of
``_S16Loop.step`` (update.py), the two hoisted convolutions and the epipolar-line cost volume run at 296 x 400 (the bench workload),
384 x 512, 540 x 960 and the 37 / 51 x 400 row slabs with ``ops.TILE_MT = 0`` - the production tile choice, the rim-first block order,
the XCD order at 925 .. 2040 blocks and the stagger branch (> 768 blocks) are what is under test - and EVERY output element is compared
with a float64 reference of that one kernel, computed from the tensors the kernel actually read (read back from the device layouts), so
that rounding does not compound from launch to launch.  A failure names the tile, row or seam (tests/parity_check.py).

Sentinel coverage: every output buffer is filled with NaN (fp32 layouts) or the f16 NaN pattern (frag16 planes) before its launch, the
padding slots of the inputs too; afterwards every data pixel must hold a number.  ``net_l`` and ``disp`` are updated in place: the copy read
back before the launch is the reference's input, and a pixel that no block wrote fails the bound.

Bounds (none is fitted to a kernel's output):
  * convolutions: |err| <= c * sum|x||w| + abs, c = 1e-6 x {1, 30, 45} for the f16x3-terms / fp8 / FP6 forms
    (test_conv_s16_two_sources_and_error_bound, the ``f8`` fixture of test_conv_s16_gpu.py), abs = 2^-(24 + log2s) * sum|w| per frag16
    operand (test_conv_s16_dynamic_range) + the frag16 quantum of the output.  The generated disparity source is evaluated by the kernel
    as 100 * (sum_taps w * d(neighbour) - (sum_taps w) * d): its magnitude enters as 100 * (unfold|d| + |d|), not as |feature|.
  * sigmoid / tanh / GRU blend: the pre-activation bound carries over (Lipschitz <= 1, |h| <= 1), + ACT_ABS = 2^-20 for the hardware
    exp2 / rcp (1 ulp each, conv_s16_shared.hpp) and the blend: <= 8 roundings of values <= 1 at 2^-23.
  * delta head: hid = relu(conv) carries the conv bound, projected with |w2|; hid is kept at 2^-(24 + 4) absolute.
  * delta_sum (and the disparity the lookup leaves in place): an 18-term fp32 sum, one product, two sums: (18 + 4) * 2^-24 of
    0.01 * (sum|T| + |bias|) + |disp|.
  * lookup + 1x1 conv: c = 1e-6 of sum|feature||w| + |b|, plus what fp32 index arithmetic costs: the index t = (disp - origin) / incre
    + D/2 is formed in fp32 from an fp32 ``incre`` (four roundings: <= 4 * 2^-24 * (|t| + D/2)), a sample moves by at most the largest
    step between neighbouring entries of its level's row (the zero border included) per unit of index, and level l sees t / 2^l.
  * cost volume: coordinates are formed in fp32, so the yardstick is the oracle's own fp32 arithmetic - oracle.cer_oracle.cost_volume in
    float32 against the float64 restatement on the same pixels, both normalised by sum_c |f1_c| * (bilinear-weighted |f2_c|) floored at the
    volume's mean magnitude; the kernel's maximum and 99.9th-percentile ratio may be at most 4 x the yardstick's.

Measured on an MI355X (profiles/fullsize_parity.json, written only under CER_PARITY_RECORD=1; a plain run writes nothing): max |err| /
sum|x||w| over all shapes - f16x3 terms: corr2 3.8e-7, hoisted 2.7e-7, q 1.1e-7, z|r 3.8e-8, delta head 7e-9; fp8: corr2 2.5e-5 (0.82 of its
bound at 51 x 400), hoisted 4.5e-6, q 2.3e-6, z|r 7.0e-7, delta head 2.3e-7; FP6: corr2 9.3e-6, hoisted 4.2e-6, q 2.5e-6; the fp32 CPU
convolution against float64 on the same inputs: 2.1e-7 - the project's constants hold at 1593-term dots, none was replaced.  delta_sum 1.1e-7,
lookup <= 0.17 of its bound.  Cost volume, |err| / norm, stage 0 / 1: kernel max 4.4e-5 / 3.6e-5, p99.9 8.2e-6 / 7.7e-6; fp32 oracle max
3.9e-5 / 4.0e-5, p99.9 7.9e-6 / 7.4e-6.  540 x 960 runs the default fp8 form only (48 s of the module's 157 s, nearly all float64 references)."""
import functools
import json
import math
import os
import time

import pytest
import torch

from conftest import REPO, cached_scene
import parity_check
from parity_check import (assert_covered, assert_elementwise, check_elementwise, cost_subset, cost_volume_ref64, delta_sum64,
                          disp_feature_parts, lookup_ref, poison_f16, poison_f32, wsum)
from test_oracle_golden import hashed

pytestmark = pytest.mark.gpu

FORMS = {"f16x3terms": ("s16", 1.0), "fp8corr": ("s16f8", 30.0), "fp6corr": ("s16f6", 45.0)}
C_CONV = 1e-6
ACT_ABS = 2.0 ** -20
C_DSUM = 22 * 2.0 ** -24
CASES = [(296, 400, "f16x3terms"), (296, 400, "fp8corr"), (296, 400, "fp6corr"), (384, 512, "fp8corr"), (540, 960, "fp8corr"),
         (37, 400, "fp8corr"), (51, 400, "fp8corr")]
STAGES = ((64, 0.0025 / 64), (44, 0.0025 / 320))       # (D, incre) of the bench cascade (64, 64, T), (-1, 320, T)
CASCADE = [(64, 64, 16), (-1, 320, 16)]
RECORD = {}                                            # figures for profiles/fullsize_parity.json (written only with CER_PARITY_RECORD)
# the float64 convolution of tests/parity_check.py; when recording it also leaves the fp32-CPU yardstick of every call in RECORD
conv_ref = functools.partial(parity_check.conv_ref, yardstick=RECORD.setdefault("yardstick_conv_fp32_cpu", {})
                             if os.environ.get("CER_PARITY_RECORD") else None)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _module_setup(dev):
    """References run on at most 16 CPU threads; the measured figures are written out only when CER_PARITY_RECORD asks for it."""
    from cer_mvs_amd import ops
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    t0 = time.time()
    yield
    torch.set_num_threads(n)
    ops.check_overflow(dev)                            # (NaN sentinels in padding slots may have raised the sticky saturation flag)
    target = os.environ.get("CER_PARITY_RECORD", "")
    if target:
        path = os.path.join(REPO, "profiles", "fullsize_parity.json") if target == "1" else target
        RECORD["module_wall_s"] = round(time.time() - t0, 1)
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


_MODELS = {}


def update_block(dev, form):
    """The update block of a RAFT with the bench's closed-form weights in arithmetic form ``form``: its loops pack the shipped layers."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    if form not in _MODELS:
        model = RAFT(cascade=CASCADE, test_mode=True, gru_precision=FORMS[form][0])
        model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
        _MODELS[form] = model.to(dev).eval()
    ub = _MODELS[form].update_block
    assert ub.conv_mode == "s16" and ub.corr_fp8 == {"f16x3terms": False, "fp8corr": True, "fp6corr": 6}[form]
    return ub


# ------------------------------------------------------------------------------------------------ layouts and float64 pieces
def unfrag(t, h, w, log2s):
    from cer_mvs_amd import ops
    return ops.from_frag16(t, h, w, log2s).cpu().double()


def unacc(t, h, w, layout):
    from cer_mvs_amd import ops
    return ops.s16_layout(t, h, w, layout, inverse=True).cpu().double()


def frag_poisoned_padding(x, h, w, log2s):
    """[P, C] device fp32 -> frag16 whose padding slots (pixels beyond the image in the last m-tile row / column) hold the f16 NaN
    sentinel instead of zeros: a kernel that consumed one would spread NaN over its output."""
    from cer_mvs_amd import ops
    buf = poison_f16(torch.empty(ops.s16_pixels(h, w), x.shape[1], device=x.device, dtype=torch.float32))
    return ops.to_frag16(x, h, w, log2s, out=buf)


# ------------------------------------------------------------------------------------------------ the production tile choice, restated
def s16_grid(h, w, cout, form, ncu):
    """Blocks of a cer_conv3x3_s16 launch with tile_mt = 0 (csrc/conv_s16.hip: ``pick`` and ``sx_launch``), restated to assert that the
    shapes of this module reach the code that only large images reach."""
    tx = (w + 15) // 16
    slots = 2 * ncu

    def pick(rows_per_mt, lo, hi, ny):
        best_mt, best = hi, -1.0
        for c in range(hi, lo - 1, -1):
            nblk = (h + rows_per_mt * c - 1) // (rows_per_mt * c) * tx * ny
            cost = ((nblk + slots - 1) // slots) * (c + 1.1)
            if best < 0 or cost < best - 1e-9:
                best, best_mt = cost, c
        return best_mt
    if cout % 128 == 0:
        mt = 2 if pick(2, 2, 4, cout // 128) == 2 else 4
        th, ny = 2 * mt, cout // 128
    else:
        mt = pick(4, 2, 3 if form != "f16x3terms" else 4, cout // 64)
        th, ny = 4 * mt, cout // 64
    return (h + th - 1) // th * tx * ny, th


def record(h, w, form, kernel, rep):
    RECORD.setdefault("kernels", {})[f"{h}x{w}/{form}/{kernel}"] = {"max_err_over_mag": rep.max_rel, "max_ratio_to_bound": rep.max_ratio,
                                                                   "p999_ratio_to_bound": rep.p999_ratio}
    print(f"  {h}x{w} {form:11s} {kernel:22s} max |err|/mag {rep.max_rel:.3e}   max |err|/bound {rep.max_ratio:.3f}   p99.9 {rep.p999_ratio:.3f}")


# ------------------------------------------------------------------------------------------------ one GRU iteration
@pytest.mark.parametrize("h,w,form", CASES, ids=[f"{h}x{w}-{f}" for h, w, f in CASES])
def test_gru_iteration_kernel_by_kernel(dev, h, w, form):
    """hoist, then the launches of ``_S16Loop.step`` in order - lookup_encode (plain, with edge-case indices, D = 64 and D = 44; then the
    ``delta=(T, bias)`` form the loop's iterations 2.. run), corr2 (RELU), z|r (GATES, disparity source in the collapsed form with the rim
    correction), q (GRU, in place, r*h in c1's buffer), the delta head (DELTA, both stages' weights) and delta_sum - each against the
    float64 reference of that launch on the inputs it read."""
    from cer_mvs_amd import _lib as L, ops, update
    assert ops.TILE_MT == 0
    widen = FORMS[form][1]
    c = C_CONV * widen
    ub = update_block(dev, form)
    loop = ub.loop(0, dev)
    loop1 = ub.loop(1, dev)
    assert isinstance(loop, update._S16Loop) and loop.zr.corr_fp8 == {"f16x3terms": 0, "fp8corr": 1, "fp6corr": 6}[form]
    g = update._stage_weights(ub, 0, "cpu")
    g1 = update._stage_weights(ub, 1, "cpu")
    P, PP = h * w, ops.s16_pixels(h, w)
    U, R = L.S16_UNIT, L.S16_RELU
    kw = dict(h=h, w=w, tile=(8, 16))
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    if (h, w) == (296, 400):                           # the stagger branch (gridDim.x > 3 * 256) and the rim-first order really run
        for cout in (64, 128, 256):                    # (the 64-channel launches of the f16x3-terms form take 16-row tiles: 475 blocks)
            assert s16_grid(h, w, cout, form, ncu)[0] > 768 or (form, cout) == ("f16x3terms", 64), (cout, s16_grid(h, w, cout, form, ncu))
    if (h, w) in ((37, 400), (51, 400)):               # the row slabs take the half-height tiles
        assert s16_grid(h, w, 128, form, ncu)[1] == 4 and s16_grid(h, w, 64, form, ncu)[1] == 8
    RECORD.setdefault("grids", {})[f"{h}x{w}/{form}"] = {str(co): s16_grid(h, w, co, form, ncu)[0] for co in (64, 128, 256)}
    seed = 5000 + 7 * h + w

    # ---- hoisted convolutions (EPI_LINEAR, acc32 out)
    inp = torch.relu(hashed((P, 64), seed + 1, -1.0, 2.0)).to(dev)
    inp_s = frag_poisoned_padding(inp, h, w, R)
    inp_rb = unfrag(inp_s, h, w, R)
    hoisted = []
    for name, pack, wt, b in (("hoist_zr", loop.zr_inp, g.wzr[:, g.inp], g.bzr), ("hoist_q", loop.q_inp, g.wq[:, g.inp], g.bq)):
        out = poison_f32(torch.empty(PP, pack.cout, device=dev))
        ops.conv3x3_s16(pack, [inp_s], h, w, L.EPI_LINEAR, out=out)
        got = unacc(out, h, w, L.S16_ACC32)
        assert_covered(got, f"{name} {h}x{w} {form}", **kw)
        ref, mag = conv_ref(inp_rb, inp_rb.abs(), wt.cpu(), b.cpu(), h, w, record_as=f"{h}x{w}/{name}")
        record(h, w, form, name, assert_elementwise(got, ref, mag, c, 2.0 ** (-24 - R) * wsum(wt.cpu()), f"{name} {h}x{w} {form}", **kw))
        hoisted.append(out)
    hzr_rb, hq_rb = unacc(hoisted[0], h, w, L.S16_ACC32), unacc(hoisted[1], h, w, L.S16_ACC32)

    # ---- lookup_encode, plain form, indices below 0 / beyond the row / integral (test_lookup_edge_cases), both stages' row lengths
    ws = {"c1": torch.empty(PP, 64, device=dev), "c2": torch.empty(PP, 64, device=dev), "z": torch.empty(PP, 64, device=dev),
          "T": torch.empty(2, 9, P, device=dev)}
    ws["rn"] = ws["c1"]                                # as shipped (update.ALIAS_RN_C1)
    w0t64, b064 = g.w0t.cpu().double(), g.b0.cpu().double()
    vols = {}
    for stage, (D, incre) in enumerate(STAGES):
        if stage == 1 and form != "fp8corr":           # (the lookup kernel does not depend on the convs' arithmetic form)
            continue
        _, _, rs = ops.row_layout(D, 3, compact=True)
        vol = hashed((P, rs), seed + 10 + stage, -4.0, 4.0).to(dev)      # (a 64-channel dot of fnet features / 8: a few units)
        vol.level0_only = True
        origin = hashed((P,), seed + 12 + stage, 0.001, 0.0015).to(dev)
        steps = hashed((P,), seed + 14 + stage, -40.0, 60.0)
        steps[::97] = torch.round(steps[::97])
        steps[0], steps[1], steps[2], steps[3], steps[P - 1], steps[P - 2] = -100.0, 1e6, 3.0, -22.0, 1e6, -100.0
        disp = (origin.cpu() + steps * incre).to(dev)
        vols[stage] = (vol, origin)
        poison_f16(ws["c1"])
        ops.lookup_encode(vol, origin, disp, loop.w0t, loop.b0, D, incre, 3, 5, out=ws["c1"], out_split=2, log2s=R, img_w=w)
        got = unfrag(ws["c1"], h, w, R)
        assert_covered(got, f"lookup D={D} {h}x{w}", **kw)
        ref, mag, idx = lookup_ref(vol.cpu().double(), origin.cpu().double(), disp.cpu().double(), w0t64, b064, D, incre)
        record(h, w, form, f"lookup_D{D}", assert_elementwise(got, ref, mag, C_CONV, idx + 2.0 ** (-24 - R), f"lookup D={D} {h}x{w}", **kw))

    # ---- the loop's own lookup: the pending disparity update rides on it (delta=(T, bias)); disparity in place, then the features
    D, incre = STAGES[0]
    vol, origin = vols[0]
    disp = (origin.cpu() + hashed((P,), seed + 20, -40.0, 60.0) * incre).to(dev)
    T0 = hashed((2, 9, P), seed + 21, -0.02, 0.02).to(dev)
    disp_before = disp.cpu().double()
    poison_f16(ws["c1"])
    ops.lookup_encode(vol, origin, disp, loop.w0t, loop.b0, D, incre, 3, 5, out=ws["c1"], out_split=2, log2s=R, img_w=w,
                      delta=(T0, loop.d2b))
    disp_rb = disp.cpu().double()
    ref, mag = delta_sum64(T0.cpu().double(), loop.d2b, disp_before, h, w)
    record(h, w, form, "lookup_delta_disp", assert_elementwise(disp_rb, ref, mag, C_DSUM, 0.0, f"lookup delta form: disparity {h}x{w}", **kw))
    c1_rb = unfrag(ws["c1"], h, w, R)
    assert_covered(c1_rb, f"lookup delta form {h}x{w}", **kw)
    ref, mag, idx = lookup_ref(vol.cpu().double(), origin.cpu().double(), disp_rb, w0t64, b064, D, incre)
    record(h, w, form, "lookup_delta_feat", assert_elementwise(c1_rb, ref, mag, C_CONV, idx + 2.0 ** (-24 - R), f"lookup delta form: features {h}x{w}", **kw))

    # ---- corr2 (EPI_RELU)
    poison_f16(ws["c2"])
    ops.conv3x3_s16(loop.corr2, [ws["c1"]], h, w, L.EPI_RELU, out=ws["c2"], out_split=True, log2s_out=R)
    c2_rb = unfrag(ws["c2"], h, w, R)
    assert_covered(c2_rb, f"corr2 {h}x{w} {form}", **kw)
    wt, b = g.corr2.weight.detach().cpu(), g.corr2.bias.detach().cpu()
    ref, mag = conv_ref(c1_rb, c1_rb.abs(), wt, b, h, w, record_as=f"{h}x{w}/corr2")
    record(h, w, form, "corr2", assert_elementwise(c2_rb, torch.relu(ref), mag, c, 2.0 ** (-24 - R) * (wsum(wt) + 1), f"corr2 {h}x{w} {form}", **kw))

    # ---- z|r (EPI_GATES): sources h | disparity (collapsed + rim correction) | c2, accumulators seeded with the hoisted term
    net = torch.tanh(hashed((P, 64), seed + 30, -2.0, 2.0)).to(dev)
    net_l = frag_poisoned_padding(net, h, w, U)
    net_rb = unfrag(net_l, h, w, U)
    feat, feat_mag = disp_feature_parts(disp_rb, h, w)
    poison_f32(ws["z"])
    poison_f16(ws["rn"])                               # (c1's buffer: its only reader, the corr2 launch, has run)
    assert ws["rn"] is ws["c1"] and ops.COLLAPSE_DISP and ops.EDGE_CORRECT
    ops.conv3x3_s16(loop.zr, [net_l, disp, ws["c2"]], h, w, L.EPI_GATES, out=ws["z"], out2=ws["rn"], aux=net_l, init=hoisted[0],
                    log2s_out=U, log2s_aux=U)
    z_rb, rh_rb = unacc(ws["z"], h, w, L.S16_F32X8), unfrag(ws["rn"], h, w, U)
    assert_covered(z_rb, f"z {h}x{w} {form}", **kw)
    assert_covered(rh_rb, f"r*h {h}x{w} {form}", **kw)
    wt = g.wzr[:, g.rest].cpu()
    pre, mag = conv_ref(torch.cat([net_rb, feat, c2_rb], 1), torch.cat([net_rb.abs(), feat_mag, c2_rb.abs()], 1), wt, None, h, w,
                        record_as=f"{h}x{w}/zr")
    pre, mag = pre + hzr_rb, mag + hzr_rb.abs()
    abs_t = 2.0 ** (-24 - R) * wsum(wt) + ACT_ABS
    record(h, w, form, "zr_z", assert_elementwise(z_rb, torch.sigmoid(pre[:, :64]), mag[:, :64], c, abs_t[:, :64], f"z|r: z {h}x{w} {form}", **kw))
    record(h, w, form, "zr_rh", assert_elementwise(rh_rb, torch.sigmoid(pre[:, 64:]) * net_rb, mag[:, 64:], c, abs_t[:, 64:],
                                                   f"z|r: r*h {h}x{w} {form}", **kw))

    # ---- q (EPI_GRU), in place on the hidden state
    ops.conv3x3_s16(loop.q, [ws["rn"], disp, ws["c2"]], h, w, L.EPI_GRU, out=net_l, aux=net_l, aux2=ws["z"], init=hoisted[1],
                    log2s_out=U, log2s_aux=U)
    new_rb = unfrag(net_l, h, w, U)
    assert_covered(new_rb, f"q {h}x{w} {form}", **kw)
    wt = g.wq[:, g.rest].cpu()
    pre, mag = conv_ref(torch.cat([rh_rb, feat, c2_rb], 1), torch.cat([rh_rb.abs(), feat_mag, c2_rb.abs()], 1), wt, None, h, w,
                        record_as=f"{h}x{w}/q")
    pre, mag = pre + hq_rb, mag + hq_rb.abs()
    new_ref = (1 - z_rb) * net_rb + z_rb * torch.tanh(pre)
    record(h, w, form, "q_gru", assert_elementwise(new_rb, new_ref, mag, c, 2.0 ** (-24 - R) * wsum(wt) + ACT_ABS, f"q / GRU blend {h}x{w} {form}", **kw))

    # ---- delta head (EPI_DELTA) + delta_sum, both stages' weights
    for stage, lp, gs in ((0, loop, g), (1, loop1, g1)):
        poison_f32(ws["T"])
        ops.conv3x3_s16(lp.d1, [net_l], h, w, L.EPI_DELTA, out=ws["T"], aux=lp.d2proj)
        T_rb = ws["T"].cpu().double()
        got = T_rb.permute(2, 0, 1).reshape(P, 18)
        assert_covered(got, f"delta head stage {stage} {h}x{w} {form}", **kw)
        w1, b1, w2 = gs.delta1.weight.detach().cpu(), gs.delta1.bias.detach().cpu(), gs.delta2.weight.detach().cpu().double()
        hid, hmag = conv_ref(new_rb, new_rb.abs(), w1, b1, h, w, record_as=f"{h}x{w}/d1_stage{stage}")
        hid = torch.relu(hid)
        proj = w2[0].reshape(2, 128, 9)                                              # [half, channel, tap]
        ref = torch.cat([hid[:, hf * 128:(hf + 1) * 128] @ proj[hf] for hf in range(2)], 1)
        mag = torch.cat([hmag[:, hf * 128:(hf + 1) * 128] @ proj[hf].abs() for hf in range(2)], 1)
        abs_t = 2.0 ** (-24 - 4) * proj.abs().sum(1).reshape(1, 18)
        record(h, w, form, f"d1_stage{stage}", assert_elementwise(got, ref, mag, c, abs_t, f"delta head stage {stage} {h}x{w} {form}", **kw))
        d_before = disp.cpu().double()
        ops.delta_sum(ws["T"], lp.d2b, disp, h, w, disp_out=disp, want_delta=False)
        ref, mag = delta_sum64(T_rb, lp.d2b, d_before, h, w)
        record(h, w, form, f"delta_sum_stage{stage}", assert_elementwise(disp.cpu().double(), ref, mag, C_DSUM, 0.0,
                                                                        f"delta_sum stage {stage} {h}x{w} {form}", **kw))


# ------------------------------------------------------------------------------------------------ the cost volume at the bench geometry
@pytest.mark.parametrize("stage", [0, 1])
def test_cost_volume_at_bench_geometry(dev, stage):
    """ops.cost_build(fold, compact, pyramid_scale = 1 / V) on the epipolar-line kernel (three-term form) at 296 x 400, V = 10, with the
    poses and intrinsics of the bench scene, against the float64 restatement of the oracle on: the whole rim, the first and last tile row
    and column, both sides of every 32-pixel segment seam, and 5 % of the interior (>= 8 % of all pixels).  Then the two-term form: bit for
    bit the three-term kernel on f16-rounded source rows (test_cost_lines_two_term_form), at this size."""
    from cer_mvs_amd import _lib as L, ops
    from cer_mvs_amd.corr import fmaps_to_nhwc
    from cer_mvs_amd.projective import pij_matrices
    from oracle import cer_oracle as O
    h, w, V = 296, 400, 10
    P = h * w
    D, incre = STAGES[stage]
    shift = stage == 0
    _, poses, intr, _ = cached_scene(1184, 1600, V, 0)                     # (bench.py: synthetic_scene(H, W, V, seed=0), scale 1)
    poses, intr = poses[0], intr[0].clone()
    intr[:, :2] /= 4
    Pij = pij_matrices(poses, intr, [0] * V, list(range(1, V + 1)))
    assert torch.equal(Pij, O.pij_matrices(poses, intr, [0] * V, list(range(1, V + 1))))      # the yardstick projects with the same bits
    fmaps = hashed((V + 1, 64, h, w), 6100, -2.0, 2.0)
    disp_in = torch.zeros(h, w) if shift else hashed((h, w), 6101, 0.0012, 0.0022)
    idx, must = cost_subset(h, w)
    assert idx.numel() >= 0.08 * P and bool(torch.isin(must.reshape(-1).nonzero().reshape(-1), idx).all())
    kw = dict(h=h, w=w, tile=(8, 16), seam=32, pixels=idx)

    fm = fmaps.to(dev)
    f1, f2 = fmaps_to_nhwc(fm[:1])[0], fmaps_to_nhwc(fm[1:], border=2)
    d0 = disp_in.reshape(-1).to(dev)
    lib = L.load()
    prev = lib.cer_cost_build_algo(0)
    try:
        _, _, rs = ops.row_layout(D, 3, compact=True)
        assert rs == D
        vol = poison_f32(torch.empty(P, rs, device=dev))
        org = poison_f32(torch.empty(P, device=dev))
        build = lambda src, **k: ops.cost_build(f1, src, Pij.to(dev), d0, D, incre, shift, h, w, 3, fold=True, compact=True, pyramid_scale=1.0 / V, **k)
        build(f2, vol=vol, origin=org)
        a2, o2 = build(f2, two_term=True)
        f2r = (f2 * 64.0).clamp(-65504.0, 65504.0).half().float() / 64.0
        r3, _ = build(f2r)
    finally:
        lib.cer_cost_build_algo(prev)
    assert not ops.check_overflow(dev)
    got_all = vol.cpu()
    assert_covered(got_all, f"cost volume stage {stage}", h=h, w=w, seam=32)
    assert_covered(org.cpu(), f"origins stage {stage}", h=h, w=w, seam=32)
    assert torch.equal(org.cpu().view(h, w), O.hypothesis_origin(disp_in, D, incre, shift))
    assert torch.equal(o2, org) and torch.equal(a2, r3) and not torch.equal(a2, vol)          # the two-term form, pinned to its definition

    ref, norm, _ = cost_volume_ref64(fmaps, Pij, D, incre, disp_in, shift, pixels=idx)
    ref, norm = ref.mean(0), norm.mean(0)
    norm = norm.clamp_min(float(ref.abs().mean()))
    yard = O.cost_volume(fmaps, poses, intr, D, incre, disp_in, shift)[0].mean(0)[idx]
    y = check_elementwise(yard, ref, norm, 1.0, where="fp32 oracle", **kw)
    figures = {"yardstick_max": y.max_ratio, "yardstick_p999": y.p999_ratio}
    k = check_elementwise(got_all[idx].double(), ref, norm, 1.0, where="kernel", **kw)
    figures.update(kernel_max=k.max_ratio, kernel_p999=k.p999_ratio, subset_fraction=idx.numel() / P)
    RECORD.setdefault("cost_volume", {})[f"stage{stage}_D{D}"] = figures
    print(f"  cost volume stage {stage} D={D}: |err| / norm  fp32 oracle max {y.max_ratio:.3e} p99.9 {y.p999_ratio:.3e};  kernel max {k.max_ratio:.3e} "
          f"p99.9 {k.p999_ratio:.3e}  ({idx.numel()} pixels, {100.0 * idx.numel() / P:.1f} %)")
    assert math.isfinite(y.max_ratio) and y.max_ratio > 0
    assert_elementwise(got_all[idx].double(), ref, norm, 4 * y.max_ratio, 0.0, f"cost volume stage {stage} (bound: 4 x the fp32 oracle's maximum)", **kw)
    assert k.p999_ratio <= 4 * y.p999_ratio, (k.p999_ratio, y.p999_ratio)
