"""One GRU iteration of the s16 update loop, launch by launch, against float64: the check shared by tests/test_fullsize_parity_gpu.py
(production shapes, ``ops.TILE_MT = 0``), tests/test_s16_ragged_parity_gpu.py (the smallest shapes at which every tiling edge exists, with
a forced tile height) and tests/test_s16_ragged_cpu.py (the restated dispatch and the census of what the ragged cases reach, no GPU).
Plain module, no fixtures.  The bounds and their derivation: the docstring of tests/test_fullsize_parity_gpu.py.

``check_iteration`` runs the two hoisted convolutions and the launches of ``_S16Loop.step`` (update.py) in order; every output buffer
holds NaN sentinels before its launch, the padding slots of the inputs too, and every output element is compared with the float64
reference of that one launch on the tensors the kernel read.  ``s16_grid`` restates the whole dispatch of ``cer_conv3x3_s16``
(csrc/conv_s16.hip: the forced tile height where it is valid, ``pick`` otherwise, ``sx_launch``), so that a failure names the tile the
launch really used and so that a module can prove which kernel family ran at which edge (``launch_edges``, ``census``)."""
import functools
import os

import torch

import parity_check
from parity_check import (assert_covered, assert_elementwise, delta_sum64, disp_feature_parts, lookup_ref, poison_f16, poison_f32, wsum)
from test_oracle_golden import hashed

FORMS = {"f16x3terms": ("s16", 1.0), "fp8corr": ("s16f8", 30.0), "fp6corr": ("s16f6", 45.0)}
C_CONV = 1e-6
ACT_ABS = 2.0 ** -20
C_DSUM = 22 * 2.0 ** -24
CASES = [(296, 400, "f16x3terms"), (296, 400, "fp8corr"), (296, 400, "fp6corr"), (384, 512, "fp8corr"), (540, 960, "fp8corr"),
         (37, 400, "fp8corr"), (51, 400, "fp8corr")]
STAGES = ((64, 0.0025 / 64), (44, 0.0025 / 320))       # (D, incre) of the bench cascade (64, 64, T), (-1, 320, T)
CASCADE = [(64, 64, 16), (-1, 320, 16)]

# The ragged module's cases: the smallest shapes at which each tiling edge of the 4 / 8 / 12 / 16-row tiles exists (what each reaches:
# the docstring of tests/test_s16_ragged_parity_gpu.py), every arithmetic form, every value ``ops.TILE_MT`` can force.
RAGGED_SHAPES = [(37, 33), (33, 37), (17, 48), (13, 37), (9, 21), (5, 70), (1, 40), (40, 2), (2, 3)]
RAGGED_TILE_MT = (2, 3, 4)
RAGGED_CASES = [(h, w, form, mt) for h, w in RAGGED_SHAPES for form in FORMS for mt in RAGGED_TILE_MT]

SX_TW = 16                                             # tile width of every s16 convolution (csrc/conv_s16.hip)
# The convolution launches of one iteration: (name, output channels, epilogue, reads the disparity source).  The delta head runs twice
# (both stages' weights).
LAUNCHES = (("hoist_zr", 128, "LINEAR", False), ("hoist_q", 64, "LINEAR", False), ("corr2", 64, "RELU", False),
            ("zr", 128, "GATES", True), ("q", 64, "GRU", True), ("d1_stage0", 256, "DELTA", False), ("d1_stage1", 256, "DELTA", False))
EPILOGUES = {64: ("LINEAR", "RELU", "GRU"), 128: ("LINEAR", "GATES"), 256: ("DELTA",)}
EDGES = ("partial_x", "partial_y", "one_row", "short")
EDGES_DISP = ("interior", "border")                    # asked of the launches with a disparity source (z|r, q) on top of EDGES


# ------------------------------------------------------------------------------------------------ the model under test
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


def planted_indices(P):
    """Where the plain lookup's edge-case indices go in an image of P pixels: ([pixels whose step is rounded to an integer], [(pixel,
    step)] in the order they are written).  Every position is taken modulo P, so that images with fewer than 6 pixels work; with P >= 6
    they are 0, 97, 194, ... and 0, 1, 2, 3, P - 1, P - 2."""
    integral = [k % P for k in range(0, P, 97)]
    planted = [(0 % P, -100.0), (1 % P, 1e6), (2 % P, 3.0), (3 % P, -22.0), ((P - 1) % P, 1e6), ((P - 2) % P, -100.0)]
    return integral, planted


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def s16_grid(h, w, cout, form, ncu, tile_mt=0):
    """(blocks, tile height) of a cer_conv3x3_s16 launch (csrc/conv_s16.hip: the dispatch at the end of ``cer_conv3x3_s16``, ``pick`` and
    ``sx_launch``), restated.  ``tile_mt`` (``ops.TILE_MT``) is honoured only where the library honours it - 2 / 4 for outputs of a
    multiple of 128 channels (2 m-tile rows per unit: 4 / 8 rows), 2 .. 3 for 64 channels in the fp8 / FP6 forms, 2 .. 4 in the
    f16x3-terms form (4 rows per unit: 8 / 12 / 16) - otherwise the picker decides."""
    tx = (w + SX_TW - 1) // SX_TW
    slots = 2 * ncu

    def pick(rows_per_mt, lo, hi, ny):
        best_mt, best = hi, -1.0
        for c in range(hi, lo - 1, -1):
            nblk = (h + rows_per_mt * c - 1) // (rows_per_mt * c) * tx * ny
            cost = ((nblk + slots - 1) // slots) * (c + 1.1)
            if best < 0 or cost < best - 1e-9:
                best, best_mt = cost, c
        return best_mt
    mt = tile_mt
    if cout % 128 == 0:
        if mt not in (2, 4):
            mt = 2 if pick(2, 2, 4, cout // 128) == 2 else 4
        th, ny = 2 * mt, cout // 128
    else:
        hi = 3 if form != "f16x3terms" else 4
        if mt < 2 or mt > hi:
            mt = pick(4, 2, hi, cout // 64)
        th, ny = 4 * mt, cout // 64
    return (h + th - 1) // th * tx * ny, th


def family(cout, form, th):
    """The kernel template ``<WM, WN, MT, F8>`` (conv3x3_s16_kernel) that a launch with this tile height instantiates."""
    f8 = {"f16x3terms": 0, "fp8corr": 1, "fp6corr": 2}[form]
    return (1, 4, th // 2, f8) if cout % 128 == 0 else (2, 2, th // 4, f8)


FAMILIES = ([(1, 4, mt, f8) for mt in (2, 4) for f8 in (0, 1, 2)] + [(2, 2, mt, f8) for mt in (2, 3) for f8 in (1, 2)]
            + [(2, 2, mt, 0) for mt in (2, 3, 4)])


def family_epilogues(fam):
    """The epilogues a family is launched with by the update loop: {64: LINEAR, RELU, GRU; 128: LINEAR, GATES; 256: DELTA}."""
    return EPILOGUES[64] if fam[0] == 2 else EPILOGUES[128] + EPILOGUES[256]


def launch_edges(h, w, th, disp_source):
    """Which tiling edges a launch with ``th``-row tiles meets in an h x w image: a partial last tile column, a partial last tile row
    below at least one whole one, such a row of exactly one image row, an image shorter than the tile; with a disparity source also
    whether interior tiles (all 3 x 3 neighbourhoods inside the image: the kernel's ``interior``) and border tiles exist, and whether the
    rim tiles are launched first (``border_first`` of ``sx_launch``)."""
    tiles_y, tiles_x = (h + th - 1) // th, (w + SX_TW - 1) // SX_TW
    e = set()
    if w % SX_TW:
        e.add("partial_x")
    if h > th and h % th:
        e.add("partial_y")
    if h > th and h % th == 1:
        e.add("one_row")
    if h < th:
        e.add("short")
    if disp_source:
        inner = sum(1 for ty in range(tiles_y) for tx in range(tiles_x)
                    if ty * th >= 1 and ty * th + th <= h - 1 and tx * SX_TW >= 1 and tx * SX_TW + SX_TW <= w - 1)
        if inner:
            e.add("interior")
        if inner < tiles_y * tiles_x:
            e.add("border")
        if tiles_x >= 3 and tiles_y >= 3:
            e.add("rim_first")
    return e


def iteration_launches(h, w, form, ncu, tile_mt=0):
    """The convolution launches of ``check_iteration`` as the restated dispatch sees them: [(name, cout, epilogue, disparity source, tile
    height, blocks)]."""
    out = []
    for name, cout, epi, dsrc in LAUNCHES:
        blocks, th = s16_grid(h, w, cout, form, ncu, tile_mt)
        out.append((name, cout, epi, dsrc, th, blocks))
    return out


def expected_tile_height(cout, form, tile_mt):
    """The tile height of a launch on an image so small that the picker, unforced, returns MT = 2 - stated without the picker: a forced
    value where the family exists, the two-unit tile otherwise."""
    if cout % 128 == 0:
        return 2 * (tile_mt if tile_mt in (2, 4) else 2)
    return 4 * (tile_mt if 2 <= tile_mt <= (4 if form == "f16x3terms" else 3) else 2)


def census(runs):
    """runs: iterable of (h, w, form, launches) with launches as ``iteration_launches`` returns them -> {(family, epilogue): set of edges
    met over all runs}."""
    seen = {}
    for h, w, form, launches in runs:
        for _, cout, epi, dsrc, th, _ in launches:
            seen.setdefault((family(cout, form, th), epi), set()).update(launch_edges(h, w, th, dsrc))
    return seen


def census_gaps(seen):
    """What is missing from a census for all 13 families x their epilogues x the edges: [] when complete."""
    gaps = []
    for fam in FAMILIES:
        for epi in family_epilogues(fam):
            want = EDGES + (EDGES_DISP if epi in ("GATES", "GRU") else ())
            miss = [e for e in want if e not in seen.get((fam, epi), ())]
            if miss:
                gaps.append((fam, epi, miss))
    return gaps


# ------------------------------------------------------------------------------------------------ one GRU iteration
def _note(record, h, w, form, kernel, rep):
    if record is not None:
        record.setdefault("kernels", {})[f"{h}x{w}/{form}/{kernel}"] = {"max_err_over_mag": rep.max_rel, "max_ratio_to_bound": rep.max_ratio,
                                                                       "p999_ratio_to_bound": rep.p999_ratio}
    print(f"  {h}x{w} {form:11s} {kernel:22s} max |err|/mag {rep.max_rel:.3e}   max |err|/bound {rep.max_ratio:.3f}   p99.9 {rep.p999_ratio:.3f}")


def check_iteration(dev, h, w, form, tile_mt=0, record=None):
    """hoist, then the launches of ``_S16Loop.step`` in order - lookup_encode (plain, with edge-case indices, D = 64 and D = 44; then the
    ``delta=(T, bias)`` form the loop's iterations 2.. run), corr2 (RELU), z|r (GATES, disparity source in the collapsed form with the rim
    correction), q (GRU, in place, r*h in c1's buffer), the delta head (DELTA, both stages' weights) and delta_sum - each against the
    float64 reference of that launch on the inputs it read.  ``ops.TILE_MT`` must be ``tile_mt`` (the caller sets and restores it).
    ``record`` (a dict): receives the figures under "kernels", the launch grids under "grids" and, when CER_PARITY_RECORD is set, the
    fp32-CPU yardstick of every reference convolution.  -> the convolution launches, as ``iteration_launches``."""
    from cer_mvs_amd import _lib as L, ops, update
    assert ops.TILE_MT == tile_mt
    yard = record.setdefault("yardstick_conv_fp32_cpu", {}) if record is not None and os.environ.get("CER_PARITY_RECORD") else None
    conv_ref = functools.partial(parity_check.conv_ref, yardstick=yard)
    note = functools.partial(_note, record, h, w, form)
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
    kw = dict(h=h, w=w, tile=(8, SX_TW))               # the launches that are no s16 convolution: reported by the smallest conv tile
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    grid = lambda cout: s16_grid(h, w, cout, form, ncu, tile_mt)
    launches = iteration_launches(h, w, form, ncu, tile_mt)
    kt = {name: dict(h=h, w=w, tile=(th, SX_TW)) for name, _, _, _, th, _ in launches}     # each conv launch's own tile
    if (h, w) == (296, 400):                           # the stagger branch (gridDim.x > 3 * 256) and the rim-first order really run
        for cout in (64, 128, 256):                    # (the 64-channel launches of the f16x3-terms form take 16-row tiles: 475 blocks)
            assert grid(cout)[0] > 768 or (form, cout) == ("f16x3terms", 64), (cout, grid(cout))
    if (h, w) in ((37, 400), (51, 400)):               # the row slabs take the half-height tiles
        assert grid(128)[1] == 4 and grid(64)[1] == 8
    if record is not None:
        record.setdefault("grids", {})[f"{h}x{w}/{form}"] = {str(co): grid(co)[0] for co in (64, 128, 256)}
    seed = 5000 + 7 * h + w

    # ---- hoisted convolutions (EPI_LINEAR, acc32 out)
    inp = torch.relu(hashed((P, 64), seed + 1, -1.0, 2.0)).to(dev)
    inp_s = frag_poisoned_padding(inp, h, w, R)
    inp_rb = unfrag(inp_s, h, w, R)
    hoisted = []
    for name, pack, wt, b in (("hoist_zr", loop.zr_inp, g.wzr[:, g.inp], g.bzr), ("hoist_q", loop.q_inp, g.wq[:, g.inp], g.bq)):
        assert pack.cout == {"hoist_zr": 128, "hoist_q": 64}[name]
        out = poison_f32(torch.empty(PP, pack.cout, device=dev))
        ops.conv3x3_s16(pack, [inp_s], h, w, L.EPI_LINEAR, out=out)
        got = unacc(out, h, w, L.S16_ACC32)
        assert_covered(got, f"{name} {h}x{w} {form}", **kt[name])
        ref, mag = conv_ref(inp_rb, inp_rb.abs(), wt.cpu(), b.cpu(), h, w, record_as=f"{h}x{w}/{name}")
        note(name, assert_elementwise(got, ref, mag, c, 2.0 ** (-24 - R) * wsum(wt.cpu()), f"{name} {h}x{w} {form}", **kt[name]))
        hoisted.append(out)
    hzr_rb, hq_rb = unacc(hoisted[0], h, w, L.S16_ACC32), unacc(hoisted[1], h, w, L.S16_ACC32)

    # ---- lookup_encode, plain form, indices below 0 / beyond the row / integral (test_lookup_edge_cases), both stages' row lengths
    ws = {"c1": torch.empty(PP, 64, device=dev), "c2": torch.empty(PP, 64, device=dev), "z": torch.empty(PP, 64, device=dev),
          "T": torch.empty(2, 9, P, device=dev)}
    ws["rn"] = ws["c1"]                                # as shipped (update.ALIAS_RN_C1)
    w0t64, b064 = g.w0t.cpu().double(), g.b0.cpu().double()
    integral, planted = planted_indices(P)
    vols = {}
    for stage, (D, incre) in enumerate(STAGES):
        if stage == 1 and form != "fp8corr":           # (the lookup kernel does not depend on the convs' arithmetic form)
            continue
        _, _, rs = ops.row_layout(D, 3, compact=True)
        vol = hashed((P, rs), seed + 10 + stage, -4.0, 4.0).to(dev)      # (a 64-channel dot of fnet features / 8: a few units)
        vol.level0_only = True
        origin = hashed((P,), seed + 12 + stage, 0.001, 0.0015).to(dev)
        steps = hashed((P,), seed + 14 + stage, -40.0, 60.0)
        steps[integral] = torch.round(steps[integral])
        for k, v in planted:
            steps[k] = v
        disp = (origin.cpu() + steps * incre).to(dev)
        vols[stage] = (vol, origin)
        poison_f16(ws["c1"])
        ops.lookup_encode(vol, origin, disp, loop.w0t, loop.b0, D, incre, 3, 5, out=ws["c1"], out_split=2, log2s=R, img_w=w)
        got = unfrag(ws["c1"], h, w, R)
        assert_covered(got, f"lookup D={D} {h}x{w}", **kw)
        ref, mag, idx = lookup_ref(vol.cpu().double(), origin.cpu().double(), disp.cpu().double(), w0t64, b064, D, incre)
        note(f"lookup_D{D}", assert_elementwise(got, ref, mag, C_CONV, idx + 2.0 ** (-24 - R), f"lookup D={D} {h}x{w}", **kw))

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
    note("lookup_delta_disp", assert_elementwise(disp_rb, ref, mag, C_DSUM, 0.0, f"lookup delta form: disparity {h}x{w}", **kw))
    c1_rb = unfrag(ws["c1"], h, w, R)
    assert_covered(c1_rb, f"lookup delta form {h}x{w}", **kw)
    ref, mag, idx = lookup_ref(vol.cpu().double(), origin.cpu().double(), disp_rb, w0t64, b064, D, incre)
    note("lookup_delta_feat", assert_elementwise(c1_rb, ref, mag, C_CONV, idx + 2.0 ** (-24 - R), f"lookup delta form: features {h}x{w}", **kw))

    # ---- corr2 (EPI_RELU)
    poison_f16(ws["c2"])
    ops.conv3x3_s16(loop.corr2, [ws["c1"]], h, w, L.EPI_RELU, out=ws["c2"], out_split=True, log2s_out=R)
    c2_rb = unfrag(ws["c2"], h, w, R)
    assert_covered(c2_rb, f"corr2 {h}x{w} {form}", **kt["corr2"])
    wt, b = g.corr2.weight.detach().cpu(), g.corr2.bias.detach().cpu()
    assert wt.shape[0] == 64
    ref, mag = conv_ref(c1_rb, c1_rb.abs(), wt, b, h, w, record_as=f"{h}x{w}/corr2")
    note("corr2", assert_elementwise(c2_rb, torch.relu(ref), mag, c, 2.0 ** (-24 - R) * (wsum(wt) + 1), f"corr2 {h}x{w} {form}", **kt["corr2"]))

    # ---- z|r (EPI_GATES): sources h | disparity (collapsed + rim correction) | c2, accumulators seeded with the hoisted term
    net = torch.tanh(hashed((P, 64), seed + 30, -2.0, 2.0)).to(dev)
    net_l = frag_poisoned_padding(net, h, w, U)
    net_rb = unfrag(net_l, h, w, U)
    feat, feat_mag = disp_feature_parts(disp_rb, h, w)
    poison_f32(ws["z"])
    poison_f16(ws["rn"])                               # (c1's buffer: its only reader, the corr2 launch, has run)
    assert ws["rn"] is ws["c1"] and ops.COLLAPSE_DISP and ops.EDGE_CORRECT
    assert loop.zr.cout == 128
    ops.conv3x3_s16(loop.zr, [net_l, disp, ws["c2"]], h, w, L.EPI_GATES, out=ws["z"], out2=ws["rn"], aux=net_l, init=hoisted[0],
                    log2s_out=U, log2s_aux=U)
    z_rb, rh_rb = unacc(ws["z"], h, w, L.S16_F32X8), unfrag(ws["rn"], h, w, U)
    assert_covered(z_rb, f"z {h}x{w} {form}", **kt["zr"])
    assert_covered(rh_rb, f"r*h {h}x{w} {form}", **kt["zr"])
    wt = g.wzr[:, g.rest].cpu()
    pre, mag = conv_ref(torch.cat([net_rb, feat, c2_rb], 1), torch.cat([net_rb.abs(), feat_mag, c2_rb.abs()], 1), wt, None, h, w,
                        record_as=f"{h}x{w}/zr")
    pre, mag = pre + hzr_rb, mag + hzr_rb.abs()
    abs_t = 2.0 ** (-24 - R) * wsum(wt) + ACT_ABS
    note("zr_z", assert_elementwise(z_rb, torch.sigmoid(pre[:, :64]), mag[:, :64], c, abs_t[:, :64], f"z|r: z {h}x{w} {form}", **kt["zr"]))
    note("zr_rh", assert_elementwise(rh_rb, torch.sigmoid(pre[:, 64:]) * net_rb, mag[:, 64:], c, abs_t[:, 64:],
                                     f"z|r: r*h {h}x{w} {form}", **kt["zr"]))

    # ---- q (EPI_GRU), in place on the hidden state
    assert loop.q.cout == 64
    ops.conv3x3_s16(loop.q, [ws["rn"], disp, ws["c2"]], h, w, L.EPI_GRU, out=net_l, aux=net_l, aux2=ws["z"], init=hoisted[1],
                    log2s_out=U, log2s_aux=U)
    new_rb = unfrag(net_l, h, w, U)
    assert_covered(new_rb, f"q {h}x{w} {form}", **kt["q"])
    wt = g.wq[:, g.rest].cpu()
    pre, mag = conv_ref(torch.cat([rh_rb, feat, c2_rb], 1), torch.cat([rh_rb.abs(), feat_mag, c2_rb.abs()], 1), wt, None, h, w,
                        record_as=f"{h}x{w}/q")
    pre, mag = pre + hq_rb, mag + hq_rb.abs()
    new_ref = (1 - z_rb) * net_rb + z_rb * torch.tanh(pre)
    note("q_gru", assert_elementwise(new_rb, new_ref, mag, c, 2.0 ** (-24 - R) * wsum(wt) + ACT_ABS, f"q / GRU blend {h}x{w} {form}", **kt["q"]))

    # ---- delta head (EPI_DELTA) + delta_sum, both stages' weights
    for stage, lp, gs in ((0, loop, g), (1, loop1, g1)):
        kd = kt[f"d1_stage{stage}"]
        assert lp.d1.cout == 256
        poison_f32(ws["T"])
        ops.conv3x3_s16(lp.d1, [net_l], h, w, L.EPI_DELTA, out=ws["T"], aux=lp.d2proj)
        T_rb = ws["T"].cpu().double()
        got = T_rb.permute(2, 0, 1).reshape(P, 18)
        assert_covered(got, f"delta head stage {stage} {h}x{w} {form}", **kd)
        w1, b1, w2 = gs.delta1.weight.detach().cpu(), gs.delta1.bias.detach().cpu(), gs.delta2.weight.detach().cpu().double()
        hid, hmag = conv_ref(new_rb, new_rb.abs(), w1, b1, h, w, record_as=f"{h}x{w}/d1_stage{stage}")
        hid = torch.relu(hid)
        proj = w2[0].reshape(2, 128, 9)                                              # [half, channel, tap]
        ref = torch.cat([hid[:, hf * 128:(hf + 1) * 128] @ proj[hf] for hf in range(2)], 1)
        mag = torch.cat([hmag[:, hf * 128:(hf + 1) * 128] @ proj[hf].abs() for hf in range(2)], 1)
        abs_t = 2.0 ** (-24 - 4) * proj.abs().sum(1).reshape(1, 18)
        note(f"d1_stage{stage}", assert_elementwise(got, ref, mag, c, abs_t, f"delta head stage {stage} {h}x{w} {form}", **kd))
        d_before = disp.cpu().double()
        ops.delta_sum(ws["T"], lp.d2b, disp, h, w, disp_out=disp, want_delta=False)
        ref, mag = delta_sum64(T_rb, lp.d2b, d_before, h, w)
        note(f"delta_sum_stage{stage}", assert_elementwise(disp.cpu().double(), ref, mag, C_DSUM, 0.0,
                                                           f"delta_sum stage {stage} {h}x{w} {form}", **kw))
    return launches
