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
import json
import math
import os
import time

import pytest
import torch

from conftest import REPO, cached_scene
from parity_check import assert_covered, assert_elementwise, check_elementwise, cost_subset, cost_volume_ref64, poison_f32
from s16_iteration_check import CASES, STAGES, check_iteration
from test_oracle_golden import hashed

pytestmark = pytest.mark.gpu

RECORD = {}                                            # figures for profiles/fullsize_parity.json (written only with CER_PARITY_RECORD)


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


# ------------------------------------------------------------------------------------------------ one GRU iteration
@pytest.mark.parametrize("h,w,form", CASES, ids=[f"{h}x{w}-{f}" for h, w, f in CASES])
def test_gru_iteration_kernel_by_kernel(dev, h, w, form):
    """hoist, then the launches of ``_S16Loop.step`` in order - lookup_encode (plain, with edge-case indices, D = 64 and D = 44; then the
    ``delta=(T, bias)`` form the loop's iterations 2.. run), corr2 (RELU), z|r (GATES, disparity source in the collapsed form with the rim
    correction), q (GRU, in place, r*h in c1's buffer), the delta head (DELTA, both stages' weights) and delta_sum - each against the
    float64 reference of that launch on the inputs it read: ``check_iteration`` of tests/s16_iteration_check.py, which
    tests/test_s16_ragged_parity_gpu.py runs at ragged sizes with forced tile heights."""
    check_iteration(dev, h, w, form, tile_mt=0, record=RECORD)


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
