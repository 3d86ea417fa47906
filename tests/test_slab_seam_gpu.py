"""The halo seam of the row-slab forward (cer-mvs_amd/slab.py) on the device, per pixel and bit for bit (on the GPU box: pytest -m gpu).

slab.py promises that the sharded forward's "results equal the single-GPU forward" and derives HALO = 7 in a comment.  Every kernel of
the path has an element-wise reference somewhere; the path itself was held to one figure per map (rel-L1 < 1e-5), which a stale, shifted
or one-row-short halo - confined to the rows next to a seam - passes.  Here, in ONE process on ``slab.LocalExchange``, at the shapes of
tests/slab_seam_cases.py (ranks that own exactly HALO rows, overlapping strips, interior ranks, odd widths; tests/test_slab_seam_cpu.py
asserts the census and proves the harness and its planted faults on the CPU), all five arithmetic forms:

  A  test_reach_of_one_iteration        one ``loop.step`` on the full image (23 x 21, 23 x 50, both stages), again with every input
                                        replaced from row 15 on / on rows 0..7: the disparity beyond 7 rows and the hidden state beyond 5
                                        keep their bits, and the rows at exactly 7 / 5 change
  B  test_slab_loop_equals_full_loop    ``slab_seam_cases.slab_loop`` (step, ``pack_strips``, ``neighbor_exchange``, ``unpack_halves``; s16
                                        forms through ``ops.s16_rows``) for T = 3: every rank's whole EXTENDED state after every iteration
                                        against the full-image loop's rows, from the same start and the same volume rows
  C  test_gather_form_*                 ``all_gather_flat`` + ``unpack_halo`` against the p2p form, and ``slab.P2P_HALO = False`` in
                                        ``sharded_forward`` at 88 x 84, G = 3: same bits
  D  test_planted_faults_are_caught     each of the five faults fails B's comparison, in a report whose first rows lie within 7 of a seam
  E  test_sharded_forward_per_pixel     ``sharded_forward`` against ``model(...)`` on the fp32 walk, 56 x 84 .. 148 x 132, G = 2, 3, 4
  F  test_sharded_cost_volume_rows      the line-tile builder's slab arguments (``y0``, ``src_hw``, ``split`` + ``slots`` into the gathered
                                        buffer with an empty view slot): origins bit-equal, volume rows within 4e-6 of the full build's
  G  test_persistent_buffers_do_not_leak   ``_slab_pads`` / ``_slab_own`` / the exchange objects' buffers across sizes, G and V

The slabs start from the stored pieces of the full image's hidden state, moved row by row (``ops.s16_rows``; plain rows in the wide forms),
not from its plain values through ``prepare_net`` again: the layouts' inverse followed by ``prepare_net`` keeps every VALUE but may split
one differently into hi | lo, and the convolutions' products then round
differently - 37 of 18 816 hidden-state elements after one s16 iteration at 14 x 21, where both slabs ARE the whole image.  The product
splits the encoder's plain output once per pixel on either path, so it is not affected.

Bits or bound, decided on an MI355X and hard-coded in ``BITS`` (profiles/slab_seam_parity.json, written only with CER_PARITY_RECORD set; a
plain run writes nothing): class "loop" (B, C, D) is BIT-IDENTICAL in all five forms - s16, s16f8, s16f6, f16x3, fp32 - in every shape,
stage, rank and iteration, hidden state (values and stored hi | lo pieces) and disparity; class "forward" (E) is bit-identical in both
forms run, s16f8 and fp32, at all four sizes.  So ``torch.equal`` is asserted everywhere and no launch had to be singled out; the per-pixel
bound (MARGIN x WIDEN[form] x the fp32 oracle's distance from ``loop_ref64``, ``yardstick``) stays in the module for a pair that a
later kernel change makes inexact - it must then be switched on here by hand, with the launch that differs named.  A: the outermost row
changes in every form - hidden-state row k - 5 at 1339 or more of its 1344 / 3200 elements, disparity row k - 7 at 16 or more of its 21 / 50 pixels (fp32 form: by 1e-9 .. 2e-8;
the row carries little signal, as the float64 experiment said, but it carries some) - so HALO = 7 is exact on the device, not generous.
D: all 30 (form, shape, fault) cases are caught, 10 to 18 failing reports each.  F: the line-tile builder's slab rows had the full build's
BITS at all four sizes (0 of the 4e-6 allowed), and the stage-1 origins with them.  The module's 137 cases take 17 s (19 s of pytest; tests/
test_update_run_gpu.py quotes 4 s for its 148 on the same kind of machine); the slowest case takes 0.8 s."""
import json
import os
import time
from types import SimpleNamespace

import pytest
import torch

import slab_seam_cases as SC
from conftest import REPO
from parity_check import check_elementwise, loop_ref64
from test_oracle_golden import hashed
from test_update_run_gpu import MARGIN, S16, WIDEN, model_of, oracle_loop32, setup, unlayout

pytestmark = pytest.mark.gpu

FORMS = tuple(WIDEN)
# What is asserted per (case class, form): True - identical bits (torch.equal), False - the per-pixel bound of ``yardstick``.  Decided by
# the device run quoted in the docstring, never at run time.
BITS = {(cls, form): True for cls in ("loop", "forward") for form in FORMS}
FWD_CASCADE = [(64, 64, 2), (-1, 320, 2)]
FWD_SIZES = ((56, 84, 2, 1), (88, 84, 3, 2), (92, 200, 2, 3), (148, 132, 4, 3))          # (H, W, G, V): 14 x 21, 22 x 21, 23 x 50, 37 x 33 features
FWD_FORMS = ("s16f8", "fp32")
RECORD = {"bit_identical": {}, "worst_ratio_to_bound": {}, "reach": {}, "faults_caught": {}}
shape_id = lambda s: f"{s[0]}x{s[1]}-G{s[2]}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _module_setup(dev):
    from cer_mvs_amd import ops
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    ops.check_overflow(dev)
    t0 = time.time()
    yield
    torch.set_num_threads(n)
    torch.cuda.synchronize()
    ops.check_overflow(dev)                            # (the planted faults may have raised the sticky saturation flag: later modules start clean)
    if os.environ.get("CER_PARITY_RECORD"):
        RECORD["module_wall_s"] = round(time.time() - t0, 1)
        with open(os.path.join(REPO, "profiles", "slab_seam_parity.json"), "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


def note(table, key, value, worse=max):
    RECORD[table][key] = value if key not in RECORD[table] else worse(RECORD[table][key], value)


# ------------------------------------------------------------------------------------------------ full image and slabs from one start
_FULL, _START, _YARD = {}, {}, {}


def take_rows(S, net_l, y0, y1, hs=None):
    """Image rows [y0, y1) of a hidden state in the loop's layout, as the layout holds them (the hi | lo pieces bit for bit: the layout's
    inverse followed by ``prepare_net`` may split a value differently) -> [(y1 - y0) * w, 64]."""
    h, w = (S.h if hs is None else hs), S.w
    if S.form not in S16:
        return net_l[y0 * w:y1 * w].clone()
    flat = torch.empty((y1 - y0) * w * 64, device=net_l.device, dtype=torch.float32)
    S.ub.loop(0, net_l.device).rows(h, w)(net_l, flat, y0, y1 - y0, False)
    return flat.view(-1, 64)


def put_rows(S, net_l, rows, y0, hs=None):
    """``take_rows``' inverse: write [n * w, 64] layout rows into image rows y0 .. of ``net_l``."""
    h, w = (S.h if hs is None else hs), S.w
    n = rows.shape[0] // w
    if S.form not in S16:
        net_l[y0 * w:(y0 + n) * w] = rows
    else:
        S.ub.loop(0, net_l.device).rows(h, w)(net_l, rows.reshape(-1).contiguous(), y0, n, True)
    return net_l


def slab_net(S, e0, e1):
    """The extended rows of the start's hidden state as a slab in the loop's layout, every stored piece unchanged."""
    from cer_mvs_amd import ops
    rows = take_rows(S, S.net0, e0, e1)
    if S.form not in S16:
        return rows
    return put_rows(S, torch.zeros(ops.s16_pixels(e1 - e0, S.w), 64, device=rows.device, dtype=torch.float32), rows, 0, hs=e1 - e0)


def ints(t):
    return t.contiguous().view(torch.int32)


def full_loop(dev, form, h, w, stage):
    """T iterations of ``loop.step(delta="now")`` on ``setup``'s tensors -> [(hidden state [P, 64] plain, disp [P], hidden state as the
    layout holds it [P, 64])] after each."""
    key = (form, h, w, stage)
    if key not in _FULL:
        S = setup(dev, form, h, w)
        st, loop = S.stages[stage], S.ub.loop(stage, dev)
        net, disp = S.net0.clone(), st.disp0.clone()
        out = []
        for _ in range(SC.T):
            loop.step(st.vol, st.origin, net, disp, S.hoisted[stage], h, w, st.D, st.incre, S.ws, delta="now")
            out.append((unlayout(S, "net", net), disp.clone(), take_rows(S, net, 0, h)))
        _FULL[key] = out
    return _FULL[key]


def slab_inputs(S, stage, d, vol, origin, inp, dev):
    """What ``sharded_forward`` gives a rank: its extended rows of the volume, origins and context, its own hoisted terms and workspace,
    (its hidden state is ``slab_net``'s)."""
    w, ub = S.w, S.ub
    rows = slice(d.e0 * w, d.e1 * w)
    d.vol = vol[rows].clone()
    d.vol.level0_only = True
    d.origin, d.inp = origin[rows].clone(), inp[rows].clone()
    d.hoist = ub.hoist_all(d.inp, d.hs, w, 2)
    d.ws = ub.workspace(d.hs, w, dev)
    d.view = SimpleNamespace(form=S.form, h=d.hs, w=w)


def slab_start(dev, form, h, w, G, stage):
    key = (form, h, w, G, stage)
    if key not in _START:
        S = setup(dev, form, h, w)
        st = S.stages[stage]
        start = SC.slab_start(h, w, G, lambda e0, e1: slab_net(S, e0, e1), st.disp0)
        for d in start.slabs:
            slab_inputs(S, stage, d, st.vol, st.origin, S.inp, dev)
        _START[key] = start
    return _START[key]


def device_step(S, stage, dev):
    st, loop = S.stages[stage], S.ub.loop(stage, dev)

    def step(d, stage_):
        loop.step(d.vol, d.origin, d.net, d.disp, d.hoist[stage_], d.hs, S.w, st.D, st.incre, d.ws, delta="now")
    return step


def run_slabs(dev, form, h, w, G, stage, exchange="p2p", fault=None):
    """``slab_loop`` on the HIP loop -> (start, [per iteration, per rank (hidden state plain, disp, hidden state as the layout holds it)])."""
    from cer_mvs_amd import slab
    S = setup(dev, form, h, w)
    loop = S.ub.loop(stage, dev)
    start = slab_start(dev, form, h, w, G, stage)
    got = SC.slab_loop(start, stage, G, SC.T, exchange, device_step(S, stage, dev), slab._device_copy, loop.rows, fault=fault)
    torch.cuda.synchronize()
    return start, [[(unlayout(d.view, "net", net), disp, take_rows(S, net, 0, d.hs, hs=d.hs)) for d, (net, disp) in zip(start.slabs, per_rank)] for per_rank in got]


def yardstick(dev, form, h, w, stage):
    """Per iteration (max |net - net64|, max |disp - disp64|) of the fp32 CPU oracle against ``loop_ref64``, both from the device's start on
    the full image: the figures of test_update_run_gpu.py::test_anchor_float64 at this size and stage."""
    from cer_mvs_amd import _lib as L, ops, update
    key = (form, h, w, stage)
    if key not in _YARD:
        S = setup(dev, form, h, w)
        st = S.stages[stage]
        net0 = unlayout(S, "net", S.net0).cpu().double()
        inp0 = (ops.from_frag16(ops.to_frag16(S.inp, h, w, L.S16_RELU), h, w, L.S16_RELU) if form in S16 else S.inp).cpu().double()
        vol, origin, disp0 = st.vol.cpu().double(), st.origin.cpu().double(), st.disp0.cpu().double()
        ref = loop_ref64(SC.T, vol, origin, net0, disp0, inp0, update._stage_weights(S.ub, stage, "cpu"), st.D, st.incre, h, w)
        sd = {k: v.detach().cpu().float() for k, v in model_of(dev, form).state_dict().items() if k.startswith("update_block.")}
        yard = oracle_loop32(sd, SC.T, vol, origin, net0, disp0, inp0, stage, st.D, st.incre, h, w)
        _YARD[key] = [(float((y[0] - r[0]).abs().max()), float((y[1] - r[1]).abs().max())) for y, r in zip(yard, ref)]
        assert all(a > 0 and b > 0 for a, b in _YARD[key])
    return _YARD[key]


def compare(cls, form, got, ref, bound, where, h, w, pixels=None, record=True, stored=None):
    """Per pixel: identical bits where ``BITS`` says so, else |got - ref| <= bound -> ParityReport (rows and columns are the full image's).
    ``stored``: the same pair as the layout holds it - where bits are asserted, the hi | lo pieces must be the same too."""
    bits = BITS[(cls, form)]
    same = torch.equal(got, ref)
    if same and bits and stored is not None and not torch.equal(ints(stored[0]), ints(stored[1])):
        got, ref, same, where = ints(stored[0]).double(), ints(stored[1]).double(), False, where + " [same values, other hi | lo pieces]"
    diff = float((got.double() - ref.double()).abs().max())
    if record:
        note("bit_identical", f"{cls}/{form}", same, worse=min)
    if bound and record:
        note("worst_ratio_to_bound", f"{cls}/{form}", diff / bound)
    if bits and same:
        return None
    if not same:
        print(f"  {where}: {int((got != ref).sum())} of {got.numel()} elements differ, max |diff| {diff:.3e}" + (f" = {diff / bound:.3g} of the bound" if bound else ""))
    return check_elementwise(got, ref, torch.ones_like(ref, dtype=torch.float64).cpu(), 0.0 if bits else bound, 0.0, where, h=h, w=w, pixels=pixels)


def loop_reports(dev, form, shape, stage, exchange="p2p", fault=None):
    """B's comparison: every rank's extended (hidden state, disp) after every iteration against the full image's rows -> failing reports."""
    h, w, G = shape
    full = full_loop(dev, form, h, w, stage)
    start, got = run_slabs(dev, form, h, w, G, stage, exchange, fault)
    yard = None if BITS[("loop", form)] else yardstick(dev, form, h, w, stage)
    bad = []
    for it in range(SC.T):
        for d, (net, disp, raw) in zip(start.slabs, got[it]):
            rows = slice(d.e0 * w, d.e1 * w)
            px = torch.arange(d.e0 * w, d.e1 * w)
            for name, x, r, k, stored in (("hidden state", net, full[it][0][rows], 0, (raw, full[it][2][rows])), ("disp", disp, full[it][1][rows], 1, None)):
                bound = MARGIN * WIDEN[form] * yard[it][k] if yard else 0.0
                rep = compare("loop", form, x, r, bound, f"{form} {shape_id(shape)} stage {stage} {exchange} iteration {it} rank {d.g} "
                              f"(rows {d.e0}..{d.e1}, owns {d.r0}..{d.r1}): {name}" + (f" [{fault}]" if fault else ""), h, w, px, record=fault is None, stored=stored)
                if rep is not None and not rep.ok:
                    bad.append(rep)
    return bad


# ------------------------------------------------------------------------------------------------ A: the reach of one iteration
def _replaced(dev, S, stage, rows):
    """The start of ``setup`` with every input replaced on image rows ``rows`` (a slice) by other values of the same ranges."""
    h, w, P, ub = S.h, S.w, S.P, S.ub
    st = S.stages[stage]
    px = slice(rows.start * w, rows.stop * w)
    seed = 9100 + 7 * h + w + stage

    def put(x, other):
        y = x.clone()
        y[px] = other.to(dev)[px]
        return y
    other = ub.prepare_net(torch.tanh(hashed((P, 64), seed + 30, -2.0, 2.0)).to(dev), h, w)
    net = put_rows(S, S.net0.clone(), take_rows(S, other, rows.start, rows.stop), rows.start)      # (the kept rows keep their stored pieces)
    inp = put(S.inp, torch.relu(hashed((P, 64), seed + 1, -1.0, 2.0)))
    vol = put(st.vol, hashed(tuple(st.vol.shape), seed + 10, -4.0, 4.0))
    vol.level0_only = True
    origin = put(st.origin, hashed((P,), seed + 12, 0.001, 0.0015))
    steps = hashed((P,), seed + 14, -40.0, 60.0)                                   # (tens of steps of ``incre`` away from the start's)
    disp = put(st.disp0, origin.cpu() + steps * st.incre)
    return SimpleNamespace(net=net, inp=inp, vol=vol, origin=origin, disp=disp, hoisted=ub.hoist_all(inp, h, w, 2))


@pytest.mark.parametrize("stage", (0, 1))
@pytest.mark.parametrize("size", ((23, 21), (23, 50)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", FORMS)
def test_reach_of_one_iteration(dev, form, size, stage):
    """One ``loop.step`` on the full image, twice from the same start; the second time every input is replaced from row k = 15 on (then: on
    rows 0 .. k' = 7).  Same size, same tiling: rows of the disparity further than 7 and rows of the hidden state further than 5 from the
    replaced rows keep their BITS, and the rows at exactly 7 / 5 change - HALO = 7 is neither too small nor generous."""
    h, w = size
    S = setup(dev, form, h, w)
    st, loop = S.stages[stage], S.ub.loop(stage, dev)

    def one(x):
        net, disp = x.net.clone(), x.disp.clone()
        loop.step(x.vol, x.origin, net, disp, x.hoisted[stage], h, w, st.D, st.incre, S.ws, delta="now")
        return unlayout(S, "net", net).view(h, w, 64), disp.view(h, w).clone(), ints(take_rows(S, net, 0, h)).view(h, w, 64)
    base = one(SimpleNamespace(net=S.net0, disp=st.disp0, vol=st.vol, origin=st.origin, hoisted=S.hoisted))
    k, k2 = 15, 7
    for what, rows, keep_net, keep_disp, edge_net, edge_disp in (
            (f"rows {k}.. replaced", slice(k, h), slice(0, k - 5), slice(0, k - 7), k - 5, k - 7),
            (f"rows 0..{k2} replaced", slice(0, k2 + 1), slice(k2 + 6, h), slice(k2 + 8, h), k2 + 5, k2 + 7)):
        net, disp, raw = one(_replaced(dev, S, stage, rows))
        assert torch.equal(raw[keep_net], base[2][keep_net]), f"{form} {h}x{w} stage {stage}, {what}: stored pieces of the hidden state changed beyond its reach"
        assert torch.isfinite(net).all() and torch.isfinite(disp).all()
        for name, x, b, keep, edge in (("hidden state", net, base[0], keep_net, edge_net), ("disp", disp, base[1], keep_disp, edge_disp)):
            ne = (x != b).reshape(h, -1).any(1).nonzero().flatten().tolist()
            assert torch.equal(x[keep], b[keep]), f"{form} {h}x{w} stage {stage}, {what}: {name} changed on rows {ne}, beyond its reach"
            moved = int((x[edge] != b[edge]).sum())
            print(f"  {form} {h}x{w} stage {stage}, {what}: {name} row {edge} changed at {moved} of {x[edge].numel()} elements, "
                  f"max {float((x[edge] - b[edge]).abs().max()):.3e}")
            note("reach", f"{form}/{name}/moved_elements_in_the_outermost_row", moved, worse=min)
            assert moved > 0, f"{form} {h}x{w} stage {stage}, {what}: {name} row {edge} did not change: the reach is shorter than stated"


# ------------------------------------------------------------------------------------------------ B: slab loop = full loop
@pytest.mark.parametrize("stage", (0, 1))
@pytest.mark.parametrize("shape", SC.SHAPES, ids=shape_id)
@pytest.mark.parametrize("form", FORMS)
def test_slab_loop_equals_full_loop(dev, form, shape, stage):
    from cer_mvs_amd import ops
    h, w, G = shape
    ops.check_overflow(dev)
    full = full_loop(dev, form, h, w, stage)
    S = setup(dev, form, h, w)
    assert not torch.equal(full[0][1], S.stages[stage].disp0) and not torch.equal(full[-1][0], full[0][0])     # (a loop that did nothing cannot pass)
    bad = loop_reports(dev, form, shape, stage)
    assert not bad, "\n".join(r.message() for r in bad[:4])
    assert ops.check_overflow(dev) == 0


# ------------------------------------------------------------------------------------------------ C: the all-gather form
@pytest.mark.parametrize("stage", (0, 1))
@pytest.mark.parametrize("shape", SC.ONE_PER_G, ids=shape_id)
@pytest.mark.parametrize("form", FWD_FORMS)
def test_gather_form_equals_p2p_form(dev, form, shape, stage):
    """``all_gather_flat`` + ``unpack_halo`` deliver what ``neighbor_exchange`` + ``unpack_halves`` deliver: same bits on every rank."""
    h, w, G = shape
    _, a = run_slabs(dev, form, h, w, G, stage, "p2p")
    _, b = run_slabs(dev, form, h, w, G, stage, "gather")
    for it in range(SC.T):
        for g in range(G):
            assert torch.equal(ints(a[it][g][2]), ints(b[it][g][2])) and torch.equal(a[it][g][1], b[it][g][1]), (form, shape, stage, it, g)
    bad = loop_reports(dev, form, shape, stage, "gather")
    assert not bad, "\n".join(r.message() for r in bad[:4])


_FWD, _SCENES = {}, {}


def fwd_model(dev, form, fresh=False):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    if fresh or form not in _FWD:
        model = RAFT(cascade=FWD_CASCADE, test_mode=True, gru_precision=form)
        model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
        model = model.to(dev).eval()
        if fresh:
            return model
        _FWD[form] = model
    return _FWD[form]


def scene(dev, H, W, V):
    from cer_mvs_amd.synthetic import synthetic_scene
    if (H, W, V) not in _SCENES:
        images, poses, intr, scale = synthetic_scene(H, W, V, seed=23)
        _SCENES[(H, W, V)] = (images.to(dev), poses.to(dev), intr.to(dev), scale)
    return _SCENES[(H, W, V)]


def sharded(model, sc, ex):
    from cer_mvs_amd import slab
    with torch.no_grad():
        return slab.sharded_forward(model, sc[0], sc[1], sc[2], sc[3], ex).clone()


@pytest.mark.parametrize("form", FWD_FORMS)
def test_gather_form_of_the_sharded_forward(dev, monkeypatch, form):
    """``slab.P2P_HALO = False`` at 88 x 84 (22 x 21 features, G = 3: the interior rank owns HALO rows), against the default, bit for bit."""
    from cer_mvs_amd import slab
    model, sc = fwd_model(dev, form), scene(dev, 88, 84, 2)
    assert slab.P2P_HALO is True
    a = sharded(model, sc, slab.LocalExchange(3))
    ex = slab.LocalExchange(3)
    monkeypatch.setattr(slab, "P2P_HALO", False)
    b = sharded(model, sc, ex)
    assert hasattr(ex, "_flat") and not hasattr(ex, "_nb")                          # (the collective that ran)
    assert torch.isfinite(a).all() and float(a.abs().sum()) > 0
    assert torch.equal(a, b), f"{int((a != b).sum())} pixels differ between the two forms of the exchange"


# ------------------------------------------------------------------------------------------------ D: planted faults
@pytest.mark.parametrize("fault", SC.FAULTS)
@pytest.mark.parametrize("shape", SC.FAULT_SHAPES, ids=shape_id)
@pytest.mark.parametrize("form", ("s16", "s16f8", "fp32"))
def test_planted_faults_are_caught(dev, form, shape, fault):
    """Each planted error must fail B's comparison, in a ``check_elementwise`` report that names rows near a seam."""
    h, w, G = shape
    bad = loop_reports(dev, form, shape, 0, "p2p", fault)
    note("faults_caught", f"{form}/{shape_id(shape)}/{fault}", len(bad))
    assert bad and not bad[0].ok, f"{fault} passed the comparison of {form} at {shape_id(shape)}: the comparison is too loose for this form"
    rows = sorted({r for rep in bad for r in rep.rows})
    print(f"  {form} {shape_id(shape)} {fault}: {len(bad)} failing reports, rows {rows}, worst ratio {max(r.max_ratio for r in bad):.3g}")
    assert max(SC.rows_from_seam(sorted(bad[0].rows), h, G)) <= 7                    # (the first report in time: the halo rows themselves)


# ------------------------------------------------------------------------------------------------ E: the sharded forward per pixel
def forward_yardstick(dev, form, h, w):
    """No float64 whole forward exists: the loop's yardstick at this feature size, in steps of ``incre`` times ``incre``, summed over the
    iterations the forward runs (2 per stage) -> a bound on |disp| differences before the final scale."""
    return sum(yardstick(dev, form, h, w, stage)[it][1] for stage in (0, 1) for it in range(2))


@pytest.mark.parametrize("size", FWD_SIZES, ids=lambda s: f"{s[0]}x{s[1]}-G{s[2]}-V{s[3]}")
@pytest.mark.parametrize("form", FWD_FORMS)
def test_sharded_forward_per_pixel(dev, form, size):
    """``slab.sharded_forward`` against ``model(...)`` with the cost volume on the fp32 walk, whose slab rows carry the full build's bits
    (tests/test_cost_geometry_gpu.py): every pixel, not one figure for the map."""
    from cer_mvs_amd import _lib as L, ops, slab
    H, W, G, V = size
    h, w = H // 4, W // 4
    assert slab.can_shard(h, G) and (h, w, G) in SC.SHAPES
    model, sc = fwd_model(dev, form), scene(dev, H, W, V)
    lib = L.load()
    prev = lib.cer_cost_build_algo(1)
    try:
        assert not ops.on_line_tiles(64, 64)
        with torch.no_grad():
            single = model(sc[0], sc[1], sc[2], scale=sc[3]).clone()
        got = sharded(model, sc, slab.LocalExchange(G))
    finally:
        lib.cer_cost_build_algo(prev)
    assert got.shape == single.shape == (1, 1, h, w) and torch.isfinite(single).all() and float(single.abs().sum()) > 0
    bound = 0.0 if BITS[("forward", form)] else MARGIN * WIDEN[form] * forward_yardstick(dev, form, h, w) * float(sc[3])
    rep = compare("forward", form, got.reshape(-1), single.reshape(-1), bound, f"{form} {H}x{W} G={G} V={V}: sharded forward", h, w)
    assert rep is None or rep.ok, rep.message()
    assert ops.check_overflow(dev) == 0


# ------------------------------------------------------------------------------------------------ F: the cost volume's slab arguments
@pytest.mark.parametrize("size", FWD_SIZES, ids=lambda s: f"{s[0]}x{s[1]}-G{s[2]}-V{s[3]}")
def test_sharded_cost_volume_rows(dev, monkeypatch, size):
    """The line-tile builder as the sharded forward calls it (``y0``, ``src_hw``, ``split`` with ``slots`` into the gathered
    [G, vmax, Pb, 128] buffer - an empty view slot at V = 1 and V = 3 with G = 2) against the single forward's build, row by row."""
    from cer_mvs_amd import ops, slab
    H, W, G, V = size
    h, w = H // 4, W // 4
    model, sc = fwd_model(dev, "s16f8"), scene(dev, H, W, V)
    calls = []
    plain = ops.cost_build

    def recorder(f1, f2, Pij, disp_in, D, *a, **k):
        before = disp_in.clone()
        vol, origin = plain(f1, f2, Pij, disp_in, D, *a, **k)
        calls.append(SimpleNamespace(D=D, vol=vol.clone(), origin=origin.clone(), disp_in=before, y0=k.get("y0", 0), src_hw=k.get("src_hw"),
                                     split=k.get("split"), h1=a[2], lines=ops.on_line_tiles(64, D)))
        return vol, origin
    monkeypatch.setattr(ops, "cost_build", recorder)
    with torch.no_grad():
        model(sc[0], sc[1], sc[2], scale=sc[3])
    full, calls[:] = list(calls), []
    sharded(model, sc, slab.LocalExchange(G))
    assert len(full) == 2 and len(calls) == 2 * G and all(c.lines for c in full + calls)
    vmax = (V + G - 1) // G
    for stage in (0, 1):
        f = full[stage]
        mag = max(float(f.vol[:, :f.D].abs().max()), 1.0)
        for g in range(G):
            c = calls[stage * G + g]
            r0, r1, e0, e1 = slab.slab_bounds(h, G, g)
            assert (c.y0, c.src_hw, c.h1, c.D) == (e0, (h, w), e1 - e0, f.D) and c.split[1].shape[:2] == (G, vmax) and len(c.split[2]) == V
            where = f"{H}x{W} G={G} V={V} stage {stage} rank {g}"
            same_in = torch.equal(c.disp_in, f.disp_in[e0 * w:e1 * w])
            ne = int((c.origin != f.origin[e0 * w:e1 * w]).sum())
            err = float((c.vol[:, :f.D] - f.vol[e0 * w:e1 * w, :f.D]).abs().max())
            print(f"  {where}: disparity in {'same bits' if same_in else 'differs'}, origin differs at {ne} pixels, |vol - full| max {err:.3e} = "
                  f"{err / (4e-6 * mag):.3g} of the bound")
            assert ne == 0, f"{where}: origin differs from the single forward's rows at {ne} pixels"
            rep = check_elementwise(c.vol[:, :f.D], f.vol[e0 * w:e1 * w, :f.D], torch.ones(1, 1, dtype=torch.float64), 4e-6 * mag, 0.0,
                                    f"{where}: volume rows", h=h, w=w, pixels=torch.arange(e0 * w, e1 * w))
            assert rep.ok, rep.message()
    assert (V % G != 0) == (G * vmax > V)                                            # (an empty view slot)


# ------------------------------------------------------------------------------------------------ G: persistent buffers
def test_persistent_buffers_do_not_leak(dev):
    """``model._slab_pads`` / ``_slab_own`` and the exchange objects' buffers across forwards of another size, G and V: the first forward
    again, bit for bit, and what a fresh model gives."""
    from cer_mvs_amd import slab
    model = fwd_model(dev, "s16f8", fresh=True)
    ex = {2: slab.LocalExchange(2), 3: slab.LocalExchange(3)}
    size1, size2 = (56, 84), (88, 84)
    first = sharded(model, scene(dev, *size1, 1), ex[2])
    other = sharded(model, scene(dev, *size2, 2), ex[3])
    v4 = sharded(model, scene(dev, *size2, 4), ex[2])
    v3 = sharded(model, scene(dev, *size2, 3), ex[2])                                # (equal vmax = 2: rank 1's second slot keeps view 4's rows)
    last = sharded(model, scene(dev, *size1, 1), ex[2])
    assert len(model._slab_pads) >= 4 and len(model._slab_own) >= 4
    assert torch.isfinite(first).all() and float(first.abs().sum()) > 0 and not torch.equal(v4, v3) and other.shape == v3.shape
    assert torch.equal(last, first), f"{int((last != first).sum())} pixels of the first forward changed after forwards of other sizes"
    fresh = fwd_model(dev, "s16f8", fresh=True)
    assert torch.equal(sharded(fresh, scene(dev, *size1, 1), slab.LocalExchange(2)), first)
    fresh = fwd_model(dev, "s16f8", fresh=True)
    assert torch.equal(sharded(fresh, scene(dev, *size2, 3), slab.LocalExchange(2)), v3), "V = 3 after V = 4 read the stale view slot"
