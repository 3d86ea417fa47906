"""Element-wise float64 parity of the WIDE-RANGE path, one launch at a time (run on the GPU box: pytest -m gpu).

The wide-range path is what a forward runs when the fast s16 path was not trusted - an s16 kernel clamped, the update weights do not fit a
shared split-f16 scale, or the caller pinned ``gru_precision="f16x3"`` / ``"fp32"``: ``_WideLoop`` (cer-mvs_amd/update.py) on
csrc/gru_f16x3.hip and csrc/gru.hip, and the wave-per-pixel cost-volume walk (``cer_cost_build_algo(1)``, csrc/cost_build.hip).  Until this
module only means (rel_l1 on a capture) and one kernel-against-kernel maximum judged it; tests/test_wide_parity_cpu.py shows what those let
through.  Here every launch of ``_WideLoop.step`` and the two hoisted convolutions run with the model's own packed weights, in both modes and
both cascade stages, for two consecutive iterations (the second reads the layouts the first wrote), and EVERY output element is compared with
a float64 reference computed from the tensors that launch read, read back from the device (split32 tensors through ``ops.split32(...,
inverse=True)``; the hidden state is copied before the in-place GRU launch), so that rounding does not compound.  The launches are restated
here; the end of the test runs ``step`` itself from the same start and requires the same bits.

Shapes (wide_parity_cases.SHAPES): 1 x 1, 3 x 70, 4 x 32, 5 x 33, 13 x 101, 24 x 96 - the f16x3 kernel tiles 4 x 32 pixels, the fp32 kernel
8 x 16; ``parity_check.wide_interior_tiles`` restates which tiles take the collapsed 81-tap disparity form, and the test asserts that the
last two shapes have both kinds of tile and the others only literal ones.

Sentinel coverage: every output buffer is filled with NaN (the f16 NaN pattern for split32 buffers) before its launch; afterwards every
element must be a number.  ``net_l`` and ``disp`` are updated in place: their coverage is the bound itself.

Bounds (parity_check.wide_*; none is fitted to a kernel's output):
  * convolutions: |err| <= 2e-6 * sum|x||w| + 3e-11 * sum|w| (test_conv3x3_f16x3_dynamic_range's pair, both modes); the accumulator seed
    enters the magnitude with |init|, the generated disparity source as 100 * (unfold|d| + |d|); a split32 output adds 2^-22 |ref| + 2^-35
    and is also compared BIT FOR BIT with the numpy restatement of split32 applied to the same launch without ``out_split``.
  * z: the pre-activation bound + 2^-20; r*h: that times |h|, + 2^-24 |ref|, + the split32 quantum.
  * q / GRU blend: |z| * (pre-activation bound + 2^-20) + 4 * 2^-24 * (|h| + |z|) + the split32 quantum, against the hidden state copied
    BEFORE the launch (out aliases aux).
  * delta head, f16x3: the hidden map's bound (with hx_split's quantum) projected with |w2|, + 2e-6 * sum_c |w2||hid|; then delta_sum at
    22 * 2^-24 of its magnitude.
  * delta head, fp32: the conv as above; cer_delta_tail_f32 at gamma_n * 0.01 * sum|w||hid| + 3 * 2^-24 * (0.01 (sum|w||hid| + |bias|) +
    |disp|) with n = 12 * C / 256 + 8, derived in ``parity_check.delta_tail_depth`` / ``delta_tail_ref64`` (the issue's first count, + 12,
    took the 16-lane sum as eight add levels; it is four).  ``test_delta_tail_alone`` runs it on its own at C = 256 / 512, widths around the
    16-pixel strip, heights 1 and 5, ``disp_out`` aliasing ``disp_in`` or not, with and without a (poisoned) ``delta``.
  * lookup: 1e-6 * mag + the fp32 index term of ``lookup_ref`` (+ the split32 quantum), the full-size module's rule.
  * the cost-volume walk: all pixels against ``cost_volume_ref64``; the yardstick is oracle.cer_oracle.cost_volume in float32 against the
    same restatement, both normalised by ``norm`` floored at the volume's mean magnitude; the kernel's maximum and 99.9th-percentile ratio
    may be at most 4 x the yardstick's.  fold=False (per-view rows) and fold=True (compact rows, pyramid_scale = 1 / V); 7 x 13 and 19 x 45;
    D = 64 / 44 / 20; V = 1 / 3; both stages; lateral, vertical, diagonal (+ in-plane rotation) and converging geometries given as poses
    and intrinsics.  Origins bit-equal to the oracle's.

Measured on an MI355X (profiles/wide_parity.json, written only under CER_WIDE_PARITY_RECORD=1; a plain run writes nothing), worst max |err| /
bound over all shapes, stages and both iterations, f16x3 / fp32 mode: lookup 0.15 / 0.15, corr2 0.10 / 0.09, hoisted 0.06 / 0.14, z 0.02 /
0.02, r*h 0.16 / 0.02, q with the in-place blend 0.53 / 0.56 (where z is near 0 the bound is the blend's four roundings and the split32
quantum alone), delta head 0.004 (tap planes) and delta_sum 0.07 / hidden map 0.14 and delta_tail 0.26; delta_tail on its own 0.014 (C = 256)
and 0.005 (C = 512) of its worst-case bound.  Convolutions, max |err| / sum|x||w|: f16x3 kernel 2.1e-7 (corr2), fp32 kernel 2.8e-7 (delta
hidden map).  The walk, |err| / norm over the 192 runs: kernel max 2.7e-5 and p99.9 5.0e-6 against the fp32 oracle's 4.9e-5 and 5.0e-6; the
worst kernel / oracle ratio of one run is 1.9 (maximum) and 1.5 (p99.9) of the 4 allowed.  No ratio above 1: no kernel was changed and no
constant replaced.  The module takes 6 s.
"""
import json
import os
import time

import numpy as np
import pytest
import torch

import parity_check as pc
import wide_parity_cases as cases
from conftest import REPO
from parity_check import assert_covered, assert_elementwise, check_elementwise, poison_f16, poison_f32

pytestmark = pytest.mark.gpu

RECORD_ENV = "CER_WIDE_PARITY_RECORD"                  # "1": write profiles/wide_parity.json; another value: that path; unset: nothing
RECORD = {}
C_LOOKUP = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _module_setup(dev):
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    t0 = time.time()
    yield
    torch.set_num_threads(n)
    target = os.environ.get(RECORD_ENV, "")
    if target:
        path = os.path.join(REPO, "profiles", "wide_parity.json") if target == "1" else target
        RECORD["module_wall_s"] = round(time.time() - t0, 1)
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


_MODELS = {}


def update_block(dev, mode):
    """The update block of a RAFT pinned to ``mode`` with the closed-form weights: its loops pack the shipped layers."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    if mode not in _MODELS:
        model = RAFT(cascade=cases.CASCADE, test_mode=True, gru_precision=mode)
        model.load_state_dict(fill_state_dict(model.state_dict(), seed=cases.WEIGHT_SEED))
        _MODELS[mode] = model.to(dev).eval()
    ub = _MODELS[mode].update_block
    assert ub.conv_mode == mode
    return ub


def record(section, key, rep):
    """Keep the worst figures seen under ``key`` (the two iterations of a stage share one)."""
    d = RECORD.setdefault(section, {}).setdefault(key, {"max_err_over_mag": 0.0, "max_ratio_to_bound": 0.0})
    d["max_err_over_mag"] = max(d["max_err_over_mag"], rep.max_rel)
    d["max_ratio_to_bound"] = max(d["max_ratio_to_bound"], rep.max_ratio)
    print(f"  {section} {key:44s} max |err|/mag {rep.max_rel:.3e}   max |err|/bound {rep.max_ratio:.3f}")


def same_bits(dev_tensor, want_np):
    return np.array_equal(dev_tensor.cpu().numpy().view(np.int32), np.ascontiguousarray(want_np, dtype=np.float32).view(np.int32))


# ------------------------------------------------------------------------------------------------ the loop, launch by launch
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("h,w", cases.SHAPES, ids=[f"{h}x{w}" for h, w in cases.SHAPES])
def test_wide_loop_launch_by_launch(dev, h, w, mode):
    from cer_mvs_amd import _lib as L, ops, update
    assert ops.COLLAPSE_DISP
    interior = pc.wide_interior_tiles(h, w)
    if (h, w) in cases.WITH_INTERIOR:
        assert bool(interior.any()) and not bool(interior.all())
    else:
        assert not bool(interior.any())
    ub = update_block(dev, mode)
    split = mode == "f16x3"
    P = h * w
    X3, F32 = dict(h=h, w=w, tile=pc.WIDE_TILE), dict(h=h, w=w, tile=pc.WIDE_TILE_F32)
    HO = F32 if mode == "fp32" else X3                                   # the kernel of the hoisted convolutions and of d1
    rb = lambda t, s=split: (ops.split32(t, inverse=True) if s else t).cpu().double()
    poison = lambda t: poison_f16(t) if split else poison_f32(t)
    sp = lambda **k: k if split else {}

    for stage in (0, 1):
        loop = ub.loop(stage, dev)
        assert isinstance(loop, update._WideLoop) and loop.mode == mode
        g = update._stage_weights(ub, stage, "cpu")
        cw = lambda t: t.detach().cpu()
        ci = cases.loop_inputs(h, w, stage)
        D, incre = ci["D"], ci["incre"]
        tag = lambda k: f"{h}x{w}/{mode}/stage{stage}/{k}"
        where = lambda k, it: f"{k} {h}x{w} {mode} stage {stage} iteration {it}"
        vol = ci["vol"].to(dev)
        vol.level0_only = True
        origin, disp, inp = ci["origin"].to(dev), ci["disp"].to(dev), ci["inp"].to(dev)
        net_l = loop.prepare_net(ci["net"].to(dev), h, w)
        start = (net_l.clone(), disp.clone())
        vol64, origin64, inp64 = vol.cpu().double(), origin.cpu().double(), inp.cpu().double()
        w0t64, b064 = g.w0t.double(), g.b0.double()

        # ---- 7. the two hoisted convolutions (loop.hoist): EPI_LINEAR in the loop's mode
        hoisted, hoisted_rb = [], []
        for name, pack, wt, b in (("hoist_zr", loop.zr_inp, cw(g.wzr[:, g.inp]), cw(g.bzr)), ("hoist_q", loop.q_inp, cw(g.wq[:, g.inp]), cw(g.bq))):
            out = poison_f32(torch.empty(P, pack.cout, device=dev))
            ops.conv3x3(pack, [inp], h, w, L.EPI_LINEAR, mode=mode, out=out)
            got = out.cpu().double()
            assert_covered(got, where(name, 0), **HO)
            ref, mag, a = pc.wide_conv_parts(inp64, inp64.abs(), wt, b, h, w)
            record("loop", tag(name), assert_elementwise(got, ref, mag, pc.WIDE_C, a, where(name, 0), **HO))
            hoisted.append(out)
            hoisted_rb.append(got)
        ref_h = loop.hoist(inp, h, w)
        assert torch.equal(ref_h[0], hoisted[0]) and torch.equal(ref_h[1], hoisted[1])

        ws = loop.workspace(h, w, dev)
        for it in (0, 1):
            # ---- 1. lookup_encode
            poison(ws["c1"])
            disp64 = disp.cpu().double()
            ops.lookup_encode(vol, origin, disp, loop.w0t, loop.b0, D, incre, loop.num_levels, loop.radius, out=ws["c1"], **sp(out_split=True))
            c1 = rb(ws["c1"])
            assert_covered(c1, where("lookup", it), **X3)
            ref, mag, idx = pc.lookup_ref(vol64, origin64, disp64, w0t64, b064, D, incre)
            record("loop", tag("lookup"), assert_elementwise(c1, ref, mag, C_LOOKUP, idx + (pc.split32_quantum(ref) if split else 0.0),
                                                             where("lookup", it), **X3))

            # ---- 2. corr2 (RELU)
            poison(ws["c2"])
            ops.conv3x3(loop.corr2, [ws["c1"]], h, w, L.EPI_RELU, mode="f16x3", out=ws["c2"], **sp(kinds=[3], out_split=True))
            c2 = rb(ws["c2"])
            assert_covered(c2, where("corr2", it), **X3)
            pre, mag, a = pc.wide_conv_parts(c1, c1.abs(), cw(g.corr2.weight), cw(g.corr2.bias), h, w)
            ref, mag, a = pc.wide_relu_parts(pre, mag, a, split)
            record("loop", tag("corr2"), assert_elementwise(c2, ref, mag, pc.WIDE_C, a, where("corr2", it), **X3))
            if split:
                flat = ops.conv3x3(loop.corr2, [ws["c1"]], h, w, L.EPI_RELU, mode="f16x3", kinds=[3])
                assert same_bits(ws["c2"], pc.split32_np(flat.cpu().numpy())), where("corr2: out_split is split32 of the plain output", it)

            # ---- 3. z|r (GATES): sources h | disparity | c2, accumulators seeded with the hoisted term, aux = h
            h_prev = rb(net_l)
            feat, feat_mag = pc.disp_feature_parts(disp64, h, w)
            poison_f32(ws["z"])
            poison(ws["rn"])
            ops.conv3x3(loop.zr, [net_l, disp, ws["c2"]], h, w, L.EPI_GATES, mode="f16x3", out=ws["z"], out2=ws["rn"], aux=net_l, init=hoisted[0],
                        **sp(kinds=[3, 1, 3], out_split=True, aux_split=True))
            z, rh = ws["z"].cpu().double(), rb(ws["rn"])
            assert_covered(z, where("z", it), **X3)
            assert_covered(rh, where("r*h", it), **X3)
            pre, mag, a = pc.wide_conv_parts(torch.cat([h_prev, feat, c2], 1), torch.cat([h_prev.abs(), feat_mag, c2.abs()], 1),
                                             cw(g.wzr[:, g.rest]), None, h, w, init=hoisted_rb[0])
            zp, rp = pc.wide_gates_parts(pre, mag, a, h_prev, split)
            record("loop", tag("zr_z"), assert_elementwise(z, zp[0], zp[1], pc.WIDE_C, zp[2], where("z|r: z", it), **X3))
            record("loop", tag("zr_rh"), assert_elementwise(rh, rp[0], rp[1], pc.WIDE_C, rp[2], where("z|r: r*h", it), **X3))
            if split:
                z2, flat = ops.conv3x3(loop.zr, [net_l, disp, ws["c2"]], h, w, L.EPI_GATES, mode="f16x3", aux=net_l, init=hoisted[0],
                                       kinds=[3, 1, 3], aux_split=True)
                assert torch.equal(z2, ws["z"]) and same_bits(ws["rn"], pc.split32_np(flat.cpu().numpy())), where("z|r: out_split", it)

            # ---- 4. q (GRU), in place on the hidden state: the reference blends with the copy taken before the launch
            flat = None
            if split:
                flat = ops.conv3x3(loop.q, [ws["rn"], disp, ws["c2"]], h, w, L.EPI_GRU, mode="f16x3", aux=net_l, aux2=ws["z"], init=hoisted[1],
                                   kinds=[3, 1, 3], aux_split=True)
            ops.conv3x3(loop.q, [ws["rn"], disp, ws["c2"]], h, w, L.EPI_GRU, mode="f16x3", out=net_l, aux=net_l, aux2=ws["z"], init=hoisted[1],
                        **sp(kinds=[3, 1, 3], out_split=True, aux_split=True))
            new = rb(net_l)
            pre, mag, a = pc.wide_conv_parts(torch.cat([rh, feat, c2], 1), torch.cat([rh.abs(), feat_mag, c2.abs()], 1),
                                             cw(g.wq[:, g.rest]), None, h, w, init=hoisted_rb[1])
            ref, gmag, ga = pc.wide_gru_parts(pre, mag, a, z, h_prev, split)
            record("loop", tag("q_gru"), assert_elementwise(new, ref, gmag, pc.WIDE_C, ga, where("q / GRU blend (in place)", it), **X3))
            if split:
                assert same_bits(net_l, pc.split32_np(flat.cpu().numpy())), where("q: in place + out_split is split32 of the out-of-place output", it)

            # ---- 5. / 6. the delta head and the disparity update
            w1, b1 = cw(g.delta1.weight), cw(g.delta1.bias)
            pre, mag, a = pc.wide_conv_parts(new, new.abs(), w1, b1, h, w)
            d_before = disp.cpu().double()
            if split:
                poison_f32(ws["T"])
                ops.conv3x3(loop.d1, [net_l], h, w, L.EPI_DELTA, mode="f16x3", out=ws["T"], aux=loop.d2proj, kinds=[3])
                T = ws["T"].cpu().double()
                got = T.permute(2, 0, 1).reshape(P, 18)
                assert_covered(got, where("delta head", it), **X3)
                ref, pmag, pabs = pc.wide_delta_parts(pre, mag, a, cw(g.delta2.weight))
                record("loop", tag("delta_head"), assert_elementwise(got, ref, pmag, pc.WIDE_C, pabs, where("delta head (tap planes)", it), **X3))
                ops.delta_sum(ws["T"], loop.d2b, disp, h, w, disp_out=disp, want_delta=False)
                ref, dmag = pc.delta_sum64(T, loop.d2b, d_before, h, w)
                record("loop", tag("delta_sum"), assert_elementwise(disp.cpu().double(), ref, dmag, pc.C_DSUM, 0.0, where("delta_sum", it), **X3))
            else:
                poison_f32(ws["hid"])
                ops.conv3x3(loop.d1, [net_l], h, w, L.EPI_RELU, mode="fp32", out=ws["hid"])
                hid = ws["hid"].cpu().double()
                assert_covered(hid, where("delta hidden map", it), **F32)
                ref, hmag, ha = pc.wide_relu_parts(pre, mag, a, False)
                record("loop", tag("delta_hid"), assert_elementwise(hid, ref, hmag, pc.WIDE_C, ha, where("delta hidden map (fp32 kernel)", it), **F32))
                ops.delta_tail(ws["hid"], loop.d2w, loop.d2b, disp, h, w, disp_out=disp, want_delta=False)
                (ref, dmag, dabs), _ = pc.delta_tail_ref64(hid, loop.d2w.cpu(), loop.d2b, d_before, h, w)
                record("loop", tag("delta_tail"), assert_elementwise(disp.cpu().double(), ref, dmag, 3 * pc.U24, dabs, where("delta_tail", it),
                                                                     h=h, w=w, tile=(1, pc.DT_STRIP)))

        # ---- the launches above are the ones ``step`` issues: two steps from the same start leave the same bits
        net2, disp2 = start
        ws2 = loop.workspace(h, w, dev)
        for it in (0, 1):
            loop.step(vol, origin, net2, disp2, tuple(hoisted), h, w, D, incre, ws2)
        assert torch.equal(net2, net_l) and torch.equal(disp2, disp), f"step() and its restatement diverge: {h}x{w} {mode} stage {stage}"


# ------------------------------------------------------------------------------------------------ cer_delta_tail_f32 on its own
@pytest.mark.parametrize("C,h,w", cases.DT_CASES, ids=[f"C{C}-{h}x{w}" for C, h, w in cases.DT_CASES])
def test_delta_tail_alone(dev, C, h, w):
    """Against a float64 3 x 3 conv at the bound derived in ``parity_check.delta_tail_ref64``; ``disp_out`` aliasing ``disp_in`` and not,
    ``delta`` absent and given (poisoned first: every element must be written)."""
    from cer_mvs_amd import ops
    hid, wt, bias, disp = cases.delta_tail_inputs(C, h, w)
    (ref, dmag, dabs), (dref, lmag, labs) = pc.delta_tail_ref64(hid.double(), wt, bias, disp.double(), h, w)
    kw = dict(h=h, w=w, tile=(1, pc.DT_STRIP))
    hid_d, wt_d = hid.to(dev), wt.to(dev)
    outs = []
    for alias in (False, True):
        for want_delta in (False, True):
            d_in = disp.to(dev).clone()
            d_out = d_in if alias else poison_f32(torch.empty(h * w, device=dev))
            where = f"delta_tail C={C} {h}x{w} alias={alias} delta={want_delta}"
            if want_delta:                                   # (ops.delta_tail allocates the delta plane itself: poison through the C entry)
                from cer_mvs_amd import _lib as L
                delta = poison_f32(torch.empty(h * w, device=dev))
                L.check(L.load().cer_delta_tail_f32(L.dev_ptr(hid_d, "hid"), L.dev_ptr(wt_d, "w"), float(bias), L.dev_ptr(d_in, "disp_in"),
                                                    L.dev_ptr(d_out, "disp_out"), L.dev_ptr(delta, "delta"), h, w, C, L.cur_stream()), "delta_tail")
                assert_covered(delta.cpu(), where + " [delta]", **kw)
                record("delta_tail", f"C{C}/{h}x{w}/delta", assert_elementwise(delta.cpu().double(), dref, lmag, 2 * pc.U24, labs, where + " [delta]", **kw))
            else:
                ops.delta_tail(hid_d, wt_d, bias, d_in, h, w, disp_out=d_out, want_delta=False)
            assert_covered(d_out.cpu(), where, **kw)
            record("delta_tail", f"C{C}/{h}x{w}/disp", assert_elementwise(d_out.cpu().double(), ref, dmag, 3 * pc.U24, dabs, where, **kw))
            if not alias:
                assert torch.equal(d_in.cpu(), disp)           # the input is left alone
            outs.append(d_out.cpu())
    assert all(torch.equal(o, outs[0]) for o in outs[1:])      # the same bits whatever the aliasing and the delta output


# ------------------------------------------------------------------------------------------------ the cost-volume walk
@pytest.mark.parametrize("h,w", cases.WALK_SHAPES, ids=[f"{h}x{w}" for h, w in cases.WALK_SHAPES])
@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("geom", cases.WALK_GEOMS)
def test_cost_walk_all_pixels(dev, geom, stage, h, w):
    """``ops.cost_build`` under ``cer_cost_build_algo(1)``: V = 1 / 3, D = 64 / 44 / 20, per-view rows (fold=False) and the folded compact
    rows the forward builds (fold=True, pyramid_scale = 1 / V), every pixel against the float64 restatement, judged by 4 x the fp32 oracle."""
    from cer_mvs_amd import _lib as L, ops
    from cer_mvs_amd.corr import fmaps_to_nhwc
    from cer_mvs_amd.projective import pij_matrices
    P = h * w
    kw = dict(h=h, w=w, tile=(1, 4))
    lib = L.load()
    prev = lib.cer_cost_build_algo(1)
    try:
        for V in cases.WALK_VS:
            c = cases.walk_case(geom, stage, h, w, V)
            assert torch.equal(pij_matrices(c["poses"], c["intr"], [0] * V, list(range(1, V + 1))), c["Pij"])
            fm = c["fmaps"].to(dev)
            f1, f2 = fmaps_to_nhwc(fm[:1])[0], fmaps_to_nhwc(fm[1:], border=2)
            d0, Pij = c["disp_in"].reshape(-1).to(dev), c["Pij"].to(dev)
            for D in cases.WALK_DS:
                R = cases.walk_reference(geom, stage, h, w, V, D)
                for fold in (False, True):
                    key = "fold" if fold else "views"
                    _, _, rs = ops.row_layout(D, 3, compact=fold)
                    vol = poison_f32(torch.empty((P, rs) if fold else (V, P, rs), device=dev))
                    org = poison_f32(torch.empty(P, device=dev))
                    extra = dict(compact=True, pyramid_scale=1.0 / V) if fold else {}
                    ops.cost_build(f1, f2, Pij, d0, D, c["incre"], c["shift"], h, w, 3, fold=fold, vol=vol, origin=org, **extra)
                    where = f"cost walk {geom} stage {stage} {h}x{w} V={V} D={D} {key}"
                    got = cases.walk_rows(vol[..., :D].cpu().double())     # (columns beyond D of the row stride are not compared)
                    assert_covered(got, where, **kw)
                    assert_covered(org.cpu(), where + " origins", **kw)
                    assert torch.equal(org.cpu(), R["origin"]), where
                    ref, norm = R[key]
                    ymax, yp = R["yardstick"][key]
                    assert np.isfinite(ymax) and ymax > 0
                    k = check_elementwise(got, ref, norm, 1.0, where=where, **kw)
                    RECORD.setdefault("cost_walk", {})[f"{geom}/stage{stage}/{h}x{w}/V{V}/D{D}/{key}"] = {
                        "yardstick_max": ymax, "yardstick_p999": yp, "kernel_max": k.max_ratio, "kernel_p999": k.p999_ratio}
                    print(f"  {where}: |err| / norm  fp32 oracle max {ymax:.3e} p99.9 {yp:.3e};  kernel max {k.max_ratio:.3e} p99.9 {k.p999_ratio:.3e}")
                    assert_elementwise(got, ref, norm, 4 * ymax, 0.0, where + " (bound: 4 x the fp32 oracle's maximum)", **kw)
                    assert k.p999_ratio <= 4 * yp, (where, k.p999_ratio, yp)
    finally:
        lib.cer_cost_build_algo(prev)
