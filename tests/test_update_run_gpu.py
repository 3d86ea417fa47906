"""Protocol parity of ``UpdateBlock.run`` (cer-mvs_amd/update.py): the update loop AS IT RUNS (on the GPU box: pytest -m gpu).

Every kernel of a GRU iteration is checked element by element one launch at a time (tests/test_fullsize_parity_gpu.py,
tests/test_conv_s16_gpu.py, tests/test_wide_parity_gpu.py).  What turns those launches into a forward is ``run``, which executes the same
arithmetic in one of three ways:

  A  "now"       every iteration through the checked wrappers, the disparity update a launch of its own (``after=`` given, or nothing else on)
  B  fused       ``_S16Loop.FUSE_DELTA``: iteration 0 "defer", 1.. "apply+defer" (the update of iteration i rides on the lookup of i + 1),
                 one stand-alone ``delta_sum`` after the last; only for iters >= 2
  C  replayed    ``update.USE_PLANS``: the first non-"defer" step is recorded as raw C-ABI calls, every later iteration is ``plan.replay()``

A forward runs B + C.  The pieces are bit-exact where they must be (test_lookup_applies_the_pending_disparity_update), so the three must
give IDENTICAL BITS: no tolerance below except in the float64 anchor.  ``run`` is driven directly, on ``hashed`` inputs in the ranges of
the full-size module, at the smallest sizes at which the loop can go wrong - 9 x 21 (5 x 2 m-tiles, 131 of 320 slots padding, less than a
conv tile), 23 x 50 (several conv tile rows, a partial last one), 7 x 64 (one full 64-pixel lookup tile per row) - both cascade stages
(D = 64 / 44), 0, 1, 2, 3, 5 iterations (2: the recorded step runs, nothing replays; 3: the first replay; 5: one plan three times) and the
five arithmetic forms (f16x3 / fp32 never fuse: wrappers against replay).  All protocols start from clones of one hidden state and
disparity and share the block's cached workspace on purpose.

  a  test_three_protocols_same_bits   disp, hidden state (raw layout and its inverse), data pixels of c2 / z / r*h / tap planes
  b  test_stale_workspace             protocol C on a workspace filled with NaN sentinels = protocol A on a zeroed one; all data finite
  c  test_two_stages_one_workspace    stage 0 then stage 1 (its own volume, origins, delta head) on one workspace, A against C
  d  test_replay_is_what_ran          counts of ``LaunchPlan.replay`` and of the delta tails at the wrapper level: the equalities of (a)
                                      compared different paths (the counts are asserted inside (a) - (c) too)
  e  test_anchor_float64              protocol A, observed through ``after(i)``, against ``parity_check.loop_ref64``; the yardstick is
                                      the fp32 oracle (oracle.cer_oracle: pyramid / lookup / update_block on the CPU) from the same start:
                                      max and 99.9th percentile of |net - net64| and |disp - disp64| / incre after every iteration may be
                                      at most 4 x the oracle's (the margin of test_cost_volume_at_bench_geometry: both round in fp32, at
                                      different places), times the project's widening factors 30 / 45 for the fp8 / FP6 correction forms
  f  test_whole_forward_*             the public entries: RAFT.forward and slab.sharded_forward with plans on / off, fusion on / off, and a
                                      second forward on the cached workspace

Measured on an MI355X (profiles/update_run_parity.json, written only with CER_PARITY_RECORD set; a plain run writes nothing): the three
protocols gave identical bits in every case - nothing to fix.  Anchor, device figure / fp32 oracle's figure, worst over the five
iterations and both sizes, hidden state max / p99.9, disparity max / p99.9: s16 1.25 / 1.05, 0.95 / 0.99; f16x3 1.19 / 1.27, 1.21 / 1.00;
fp32 1.09 / 1.12, 1.37 / 1.37 (of 4 allowed); s16f8 11.8 / 10.9, 7.8 / 7.9 (of 120); s16f6 12.6 / 12.1, 9.4 / 10.2 (of 180).  In absolute
terms after five iterations at 23 x 50: the oracle is 1.5e-5 (hidden state) and 1.7e-5 steps of ``incre`` (disparity) from float64, the
f16x3-terms and wide forms the same.  The module's 148 cases take 4 s."""
import json
import math
import os
import time
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from parity_check import assert_covered, check_elementwise, loop_ref64, poison_f16, poison_f32
from test_oracle_golden import hashed

pytestmark = pytest.mark.gpu

WIDEN = {"s16": 1.0, "s16f8": 30.0, "s16f6": 45.0, "f16x3": 1.0, "fp32": 1.0}    # the ``f8`` fixture of test_conv_s16_gpu.py / FORMS of the full-size module
S16 = ("s16", "s16f8", "s16f6")
MARGIN = 4.0
SIZES = ((9, 21), (23, 50), (7, 64))
STAGES = ((64, 0.0025 / 64), (44, 0.0025 / 320))
CASCADE = [(64, 64, 16), (-1, 320, 16)]
ITERS = (0, 1, 2, 3, 5)
OTHER_SIZE = {"s16": (23, 50), "s16f6": (7, 64), "f16x3": (23, 50), "fp32": (7, 64)}
RECORD = {}


def _cases():
    out = [("s16f8", h, w, st, it) for h, w in SIZES for st in (0, 1) for it in ITERS]
    for form, other in OTHER_SIZE.items():
        out += [(form, 9, 21, st, it) for st in (0, 1) for it in ITERS]
        out += [(form, *other, st, it) for st in (0, 1) for it in (2, 3, 5)]
    return out


CASES = _cases()
case_id = lambda c: f"{c[0]}-{c[1]}x{c[2]}-stage{c[3]}-T{c[4]}"


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
    ops.check_overflow(dev)                            # (NaN sentinels may have raised the sticky saturation flag: later modules start clean)
    if os.environ.get("CER_PARITY_RECORD"):
        RECORD["module_wall_s"] = round(time.time() - t0, 1)
        with open(os.path.join(REPO, "profiles", "update_run_parity.json"), "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


_MODELS, _SETUPS = {}, {}


def model_of(dev, form):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    if form not in _MODELS:
        model = RAFT(cascade=CASCADE, test_mode=True, gru_precision=form)
        model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
        _MODELS[form] = model.to(dev).eval()
    ub = _MODELS[form].update_block
    assert ub.conv_mode == ("s16" if form in S16 else form) and ub.corr_fp8 == {"s16f8": True, "s16f6": 6}.get(form, False)
    return _MODELS[form]


def setup(dev, form, h, w):
    """Inputs of ``run`` for both stages at one size, built once and never written: every protocol starts from clones of ``net0`` / ``disp0``
    and runs on ``ws``, the block's cached workspace."""
    from cer_mvs_amd import ops, update
    key = (form, h, w)
    if key in _SETUPS:
        return _SETUPS[key]
    ub = model_of(dev, form).update_block
    loop = ub.loop(0, dev)
    assert isinstance(loop, update._S16Loop if form in S16 else update._WideLoop) and loop.FUSE_DELTA == (form in S16)
    P = h * w
    seed = 7000 + 7 * h + w
    inp = torch.relu(hashed((P, 64), seed + 1, -1.0, 2.0)).to(dev)
    net = torch.tanh(hashed((P, 64), seed + 30, -2.0, 2.0)).to(dev)
    S = SimpleNamespace(form=form, h=h, w=w, P=P, ub=ub, inp=inp, net0=ub.prepare_net(net, h, w), hoisted=ub.hoist_all(inp, h, w, 2),
                        ws=ub.workspace(h, w, dev), stages=[])
    if form in S16:
        assert S.ws is ub.workspace(h, w, dev) and S.ws["rn"] is S.ws["c1"] and S.ws["c1"].shape[0] == ops.s16_pixels(h, w)
    for stage, (D, incre) in enumerate(STAGES):
        _, _, rs = ops.row_layout(D, 3, compact=True)
        vol = hashed((P, rs), seed + 10 + stage, -4.0, 4.0).to(dev)
        vol.level0_only = True
        origin = hashed((P,), seed + 12 + stage, 0.001, 0.0015).to(dev)
        steps = hashed((P,), seed + 14 + stage, -40.0, 60.0)
        steps[::17] = torch.round(steps[::17])
        disp0 = (origin.cpu() + steps * incre).to(dev)
        S.stages.append(SimpleNamespace(stage=stage, D=D, incre=incre, vol=vol, origin=origin, disp0=disp0))
    _SETUPS[key] = S
    return S


def unlayout(S, name, t):
    """Data pixels of a loop tensor in the plain [P, C] layout (bit-preserving for what the layouts hold)."""
    from cer_mvs_amd import _lib as L, ops
    h, w = S.h, S.w
    if name in ("T", "hid"):
        return t.clone()
    if S.form in S16:
        if name == "z":
            return ops.s16_layout(t, h, w, L.S16_F32X8, inverse=True)
        return ops.from_frag16(t, h, w, L.S16_RELU if name == "c2" else L.S16_UNIT)
    return ops.split32(t, inverse=True) if (S.form == "f16x3" and name != "z") else t.clone()      # (z stays plain fp32 in the wide forms)


def ws_names(S):
    return ("c2", "z", "rn", "hid" if S.form == "fp32" else "T")


def fill_ws(S, how):
    """``how``: "zero", or "poison" - the sentinels of parity_check in every tensor (f16 NaN halves in the frag16 / split32 ones, fp32 NaN
    in the rest), and the tap planes NaN."""
    seen = set()
    for name, t in S.ws.items():
        if t.data_ptr() in seen:
            continue
        seen.add(t.data_ptr())
        if how == "zero":
            t.zero_()
        elif name in ("T", "hid", "z") or S.form == "fp32":
            poison_f32(t)
        else:
            poison_f16(t)
    if how == "poison" and "T" in S.ws:
        S.ws["T"].fill_(float("nan"))


def run_protocol(monkeypatch, S, proto, stage, iters, start=None, observe=None, origin=None):
    """One ``run`` under protocol ``proto`` from clones of the start -> SimpleNamespace(disp, net_raw, net, ws = {name: data pixels},
    after = [i, ...], replays, dsum, dtail, switches)."""
    from cer_mvs_amd import _lib as L, ops, update
    st = S.stages[stage]
    net_l, disp = (S.net0.clone(), st.disp0.clone()) if start is None else (start[0].clone(), start[1].clone())
    counts = {"replay": 0, "delta_sum": 0, "delta_tail": 0}
    seen = []
    with monkeypatch.context() as m:
        m.setattr(update, "USE_PLANS", proto == "C")
        replay, dsum, dtail = L.LaunchPlan.replay, ops.delta_sum, ops.delta_tail

        def counted(name, fn):
            def call(*a, **k):
                counts[name] += 1
                return fn(*a, **k)
            return call
        m.setattr(L.LaunchPlan, "replay", counted("replay", replay))
        m.setattr(ops, "delta_sum", counted("delta_sum", dsum))
        m.setattr(ops, "delta_tail", counted("delta_tail", dtail))

        def after(i):
            seen.append(i)
            if observe is not None:
                observe(i, net_l, disp)
        switches = (update.USE_PLANS, S.ub.loop(stage, disp.device).FUSE_DELTA, proto == "A")
        S.ub.run(iters, st.vol, st.origin if origin is None else origin, net_l, disp, S.hoisted[stage], stage, S.h, S.w, st.D, st.incre, S.ws,
                 after=after if proto == "A" else None)
    torch.cuda.synchronize()
    res = SimpleNamespace(disp=disp, net_raw=net_l, net=unlayout(S, "net", net_l),
                          ws={n: unlayout(S, n, S.ws[n]) for n in ws_names(S)} if iters else {}, after=seen, switches=switches,
                          replays=counts["replay"], dsum=counts["delta_sum"], dtail=counts["delta_tail"], proto=proto, iters=iters)
    check_counts(S, res)
    return res


def check_counts(S, r):
    """(d): what ran.  Replays: iters - 2 on the s16 forms (iteration 0 is "defer", iteration 1 the recorded one), iters - 1 on the wide
    forms, none without plans.  Delta tails at the wrapper level: protocol A one per iteration; fused, the single trailing delta_sum;
    replayed wide forms, the recorded iteration's only."""
    s16, T = S.form in S16, r.iters
    fused = s16 and r.proto != "A" and T >= 2
    assert r.switches == (r.proto == "C", s16, r.proto == "A")
    assert r.after == (list(range(T)) if r.proto == "A" else [])
    assert r.replays == (max(T - (2 if s16 else 1), 0) if r.proto == "C" else 0), f"protocol {r.proto}, {T} iterations: {r.replays} replays"
    tails = 1 if fused else (min(T, 1) if r.proto == "C" else T)
    assert (r.dtail, r.dsum) == ((tails, 0) if S.form == "fp32" else (0, tails)), \
        f"protocol {r.proto}, {T} iterations ({S.form}): {r.dsum} delta_sum and {r.dtail} delta_tail calls at the wrapper level, {tails} expected"


def assert_same_bits(S, a, b, what, raw=True):
    """disp, hidden state (raw layout tensor, and its inverse) and the workspace's data pixels; the first differing pixel is named."""
    pairs = [("disp", a.disp, b.disp), ("hidden state", a.net, b.net)] + [(f"ws[{n}]", a.ws[n], b.ws[n]) for n in a.ws]
    if raw:
        pairs.append(("hidden state, raw layout", a.net_raw, b.net_raw))
    for name, x, y in pairs:
        if not torch.equal(x, y):
            ne = (x.view(torch.int32) != y.view(torch.int32))
            if name.startswith("ws[T") and ne.dim() == 3:
                ne = ne.permute(2, 0, 1)
            ne = ne.reshape(ne.shape[0], -1)
            first = int(ne.any(1).nonzero()[0])
            where = f"pixel {first} (row {first // S.w}, column {first % S.w})" if ne.shape[0] == S.P else f"slot {first}"
            raise AssertionError(f"{what}: {name} differs between protocols {a.proto} and {b.proto} at {int(ne.sum())} elements of {ne.numel()}, "
                                 f"first at {where}, channel {int(ne[first].nonzero()[0])} ({S.form}, {S.h} x {S.w}, {a.iters} iterations)")


def assert_finite(S, r, what):
    kw = dict(h=S.h, w=S.w)
    assert_covered(r.disp, f"{what}: disp", **kw)
    assert_covered(r.net, f"{what}: hidden state", **kw)
    for n, t in r.ws.items():
        assert_covered(t.permute(2, 0, 1).reshape(S.P, -1) if t.dim() == 3 else t, f"{what}: ws[{n}]", **kw)


# ------------------------------------------------------------------------------------------------ (a) three protocols, same bits
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_three_protocols_same_bits(dev, monkeypatch, case):
    from cer_mvs_amd import ops
    form, h, w, stage, iters = case
    S = setup(dev, form, h, w)
    st = S.stages[stage]
    ops.check_overflow(dev)
    a = run_protocol(monkeypatch, S, "A", stage, iters)
    b = run_protocol(monkeypatch, S, "B", stage, iters)
    c = run_protocol(monkeypatch, S, "C", stage, iters)
    what = f"{case_id(case)}"
    if iters == 0:
        for r in (a, b, c):
            assert torch.equal(r.disp, st.disp0) and torch.equal(r.net_raw, S.net0)
        assert ops.check_overflow(dev) == 0
        return
    assert_finite(S, a, what)
    assert not torch.equal(a.disp, st.disp0) and not torch.equal(a.net_raw, S.net0)            # (a loop that did nothing cannot pass)
    assert_same_bits(S, a, b, what)
    assert_same_bits(S, a, c, what)
    assert ops.check_overflow(dev) == 0


# ------------------------------------------------------------------------------------------------ (b) stale workspace
STALE = [("s16f8", h, w, st) for h, w in SIZES for st in (0, 1)] + [(f, 9, 21, 0) for f in ("s16", "s16f6", "f16x3", "fp32")]


@pytest.mark.parametrize("form,h,w,stage", STALE, ids=[f"{f}-{h}x{w}-stage{s}" for f, h, w, s in STALE])
def test_stale_workspace(dev, monkeypatch, form, h, w, stage):
    """Nothing of a previous run may reach a result: "defer" must not read the tap planes, no consumer may read a padding slot.  (The
    padding slots of the hidden state's raw layout do inherit what the workspace's padding held - the epilogues store whole m-tiles -
    so the raw tensor is compared on a zeroed workspace only, in (a).)"""
    from cer_mvs_amd import ops
    S = setup(dev, form, h, w)
    try:
        fill_ws(S, "zero")
        a = run_protocol(monkeypatch, S, "A", stage, 3)
        fill_ws(S, "poison")
        c = run_protocol(monkeypatch, S, "C", stage, 3)
        assert_finite(S, c, f"poisoned workspace {form} {h}x{w}")
        assert_same_bits(S, a, c, f"poisoned workspace {form} {h}x{w} stage {stage}", raw=False)
        assert c.replays == (1 if form in S16 else 2)
    finally:
        torch.cuda.synchronize()
        ops.check_overflow(dev)
        fill_ws(S, "zero")


# ------------------------------------------------------------------------------------------------ (c) two stages on one workspace
TWO = [("s16f8", h, w) for h, w in SIZES] + [(f, 9, 21) for f in ("s16", "s16f6", "f16x3", "fp32")]


@pytest.mark.parametrize("form,h,w", TWO, ids=[f"{f}-{h}x{w}" for f, h, w in TWO])
def test_two_stages_one_workspace(dev, monkeypatch, form, h, w):
    """run(3, stage 0) then run(3, stage 1) on the state stage 0 left, with stage 1's volume and its own delta head (the cascade shares the
    GRU and the correlation encoder: RAFT's constructor offers no other sharing), origins = the disparity stage 0 ended on, as the cost
    volume of a refinement stage sets them.  The first step of stage 1 is a "defer" step over stage 0's tap planes."""
    from cer_mvs_amd import update
    S = setup(dev, form, h, w)
    g0, g1 = (update._stage_weights(S.ub, s, "cpu") for s in (0, 1))
    assert not torch.equal(g0.delta1.weight, g1.delta1.weight) and S.ub.loop(0, dev) is not S.ub.loop(1, dev)
    res = {}
    for proto in ("A", "C"):
        r0 = run_protocol(monkeypatch, S, proto, 0, 3)
        origin1 = r0.disp.clone()
        r1 = run_protocol(monkeypatch, S, proto, 1, 3, start=(r0.net_raw, r0.disp), origin=origin1)
        res[proto] = (r0, r1)
    for k in (0, 1):
        assert_finite(S, res["A"][k], f"stage {k}")
        assert_same_bits(S, res["A"][k], res["C"][k], f"two stages, after stage {k}")
    assert not torch.equal(res["A"][1].disp, res["A"][0].disp) and not torch.equal(res["A"][1].net_raw, res["A"][0].net_raw)


# ------------------------------------------------------------------------------------------------ (d) replay is really what ran
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("form", list(WIDEN))
def test_replay_is_what_ran(dev, monkeypatch, form, iters):
    S = setup(dev, form, 9, 21)
    s16 = form in S16
    got = {p: run_protocol(monkeypatch, S, p, 0, iters) for p in "ABC"}
    assert [got[p].replays for p in "ABC"] == [0, 0, max(iters - (2 if s16 else 1), 0)]
    tails = lambda r: r.dtail if form == "fp32" else r.dsum
    assert tails(got["A"]) == iters
    if s16 and iters >= 2:
        assert tails(got["B"]) == tails(got["C"]) == 1
    if not s16:
        assert tails(got["B"]) == iters and tails(got["C"]) == min(iters, 1)


# ------------------------------------------------------------------------------------------------ (e) anchor to float64
def oracle_loop32(sd, iters, vol, origin, net, disp, inp, stage, D, incre, h, w):
    """The yardstick: ``iters`` iterations of the oracle (pyramid, lookup, update_block) in float32 on the CPU -> [(net [P,64], disp [P])]."""
    from oracle import cer_oracle as O
    P = h * w
    levels = O.pyramid(vol[None, :, :D].float(), 3)
    nchw = lambda x: x.float().t().reshape(1, -1, h, w).contiguous()
    net, inp, disp, origin = nchw(net), nchw(inp), disp.float().reshape(1, 1, h, w), origin.float().reshape(h, w)
    out = []
    for _ in range(iters):
        feats = O.lookup(levels, origin, disp[0, 0], D, incre, 5)
        net, delta = O.update_block(sd, net, inp, disp, feats, stage)
        disp = disp + delta
        out.append((net[0].permute(1, 2, 0).reshape(P, -1).double(), disp.reshape(P).double()))
    return out


def figures(x, ref):
    err = (x.double() - ref).abs().reshape(-1)
    k = max(1, int(math.ceil(0.999 * err.numel())))
    return float(err.max()), float(torch.kthvalue(err, k).values)


ANCHOR = [(f, h, w) for f in WIDEN for h, w in ((9, 21), (23, 50))]


@pytest.mark.parametrize("form,h,w", ANCHOR, ids=[f"{f}-{h}x{w}" for f, h, w in ANCHOR])
def test_anchor_float64(dev, monkeypatch, form, h, w):
    """Measured on an MI355X: profiles/update_run_parity.json (``ratios``)."""
    from cer_mvs_amd import _lib as L, ops, update
    S = setup(dev, form, h, w)
    st = S.stages[0]
    T, P = 5, S.P
    seen = []
    a = run_protocol(monkeypatch, S, "A", 0, T, observe=lambda i, net_l, disp: seen.append((unlayout(S, "net", net_l).cpu(), disp.cpu().clone())))
    assert len(seen) == T and torch.equal(seen[-1][0], a.net.cpu()) and torch.equal(seen[-1][1], a.disp.cpu())
    # the start, as the device holds it
    net0 = unlayout(S, "net", S.net0).cpu().double()
    inp0 = (ops.from_frag16(ops.to_frag16(S.inp, h, w, L.S16_RELU), h, w, L.S16_RELU) if form in S16 else S.inp).cpu().double()
    vol, origin, disp0 = st.vol.cpu().double(), st.origin.cpu().double(), st.disp0.cpu().double()
    g = update._stage_weights(S.ub, 0, "cpu")
    ref = loop_ref64(T, vol, origin, net0, disp0, inp0, g, st.D, st.incre, h, w)
    sd = {k: v.detach().cpu().float() for k, v in model_of(dev, form).state_dict().items() if k.startswith("update_block.")}
    yard = oracle_loop32(sd, T, vol, origin, net0, disp0, inp0, 0, st.D, st.incre, h, w)
    allowed = MARGIN * WIDEN[form]
    failures, ratios = [], {}
    for i in range(T):
        for name, got, y, r64, scale in (("net", seen[i][0], yard[i][0], ref[i][0], 1.0), ("disp", seen[i][1], yard[i][1], ref[i][1], st.incre)):
            dmax, dp = (v / scale for v in figures(got, r64))
            ymax, yp = (v / scale for v in figures(y, r64))
            assert ymax > 0 and yp > 0 and torch.isfinite(got).all()
            ratios[f"iter{i}/{name}"] = {"device_max": dmax, "device_p999": dp, "oracle_max": ymax, "oracle_p999": yp,
                                         "ratio_max": dmax / ymax, "ratio_p999": dp / yp}
            print(f"  {form:6s} {h}x{w} iteration {i} {name:4s}: device max {dmax:.3e} p99.9 {dp:.3e};  fp32 oracle max {ymax:.3e} p99.9 {yp:.3e};  "
                  f"ratio {dmax / ymax:.2f} / {dp / yp:.2f} of {allowed:g} allowed")
            rep = check_elementwise(got, r64, torch.ones_like(r64), allowed * ymax * scale, 0.0, f"{form} iteration {i}: {name}", h=h, w=w)
            if not rep.ok:
                failures.append(rep.message())
            if dp > allowed * yp:
                failures.append(f"{form} {h}x{w} iteration {i}: {name} p99.9 {dp:.3e} > {allowed:g} x the fp32 oracle's {yp:.3e}")
    RECORD.setdefault("ratios", {})[f"{form}/{h}x{w}"] = ratios
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ (f) whole forward
FWD_CASCADE = [(64, 64, 3), (-1, 320, 3)]


@pytest.fixture(scope="module")
def fwd_model(dev):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    model = RAFT(cascade=FWD_CASCADE, test_mode=True, gru_precision="s16f8")
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
    return model.to(dev).eval()


def test_whole_forward_protocols(dev, monkeypatch, fwd_model):
    """RAFT.forward at 36 x 84 (9 x 21 features, T = 3 per stage): plans on / off and fusion on / off give the same bits, and so does a
    second forward, which finds the first one's planes in the cached workspace."""
    from cer_mvs_amd import _lib as L, update
    from cer_mvs_amd.synthetic import synthetic_scene
    images, poses, intr, scale = synthetic_scene(36, 84, 3, seed=2)
    images, poses, intr = images.to(dev), poses.to(dev), intr.to(dev)
    counts = {"replay": 0}
    plain = L.LaunchPlan.replay

    def replay(self):
        counts["replay"] += 1
        return plain(self)
    monkeypatch.setattr(L.LaunchPlan, "replay", replay)
    outs = {}
    for plans, fuse in ((True, True), (False, True), (True, False), (False, False), (True, True)):
        monkeypatch.setattr(update, "USE_PLANS", plans)
        monkeypatch.setattr(update._S16Loop, "FUSE_DELTA", fuse)
        counts["replay"] = 0
        with torch.no_grad():
            out = fwd_model(images, poses, intr, scale=scale).clone()
        assert counts["replay"] == ((2 * (1 if fuse else 2)) if plans else 0)                  # (per stage: T - 2 fused, T - 1 not)
        outs.setdefault((plans, fuse), []).append(out)
    first = outs[(True, True)][0]
    assert torch.isfinite(first).all() and float(first.abs().sum()) > 0
    for key, got in outs.items():
        for k, out in enumerate(got):
            assert torch.equal(out, first), f"USE_PLANS={key[0]} FUSE_DELTA={key[1]} forward {k}: {int((out != first).sum())} pixels differ"


def test_whole_forward_sharded(dev, monkeypatch, fwd_model):
    """slab.sharded_forward over two simulated ranks at 100 x 132 (T = 3): its plan_step / plan_halo replay is the same mechanism."""
    from cer_mvs_amd import _lib as L, slab, update
    from cer_mvs_amd.synthetic import synthetic_scene
    images, poses, intr, scale = synthetic_scene(100, 132, 2, seed=23)
    images, poses, intr = images.to(dev), poses.to(dev), intr.to(dev)
    assert slab.can_shard(100 // 4, 2)
    counts = {"replay": 0}
    plain = L.LaunchPlan.replay

    def replay(self):
        counts["replay"] += 1
        return plain(self)
    monkeypatch.setattr(L.LaunchPlan, "replay", replay)
    outs = {}
    for plans in (True, False):
        monkeypatch.setattr(update, "USE_PLANS", plans)
        counts["replay"] = 0
        with torch.no_grad():
            outs[plans] = slab.sharded_forward(fwd_model, images, poses, intr, scale, slab.LocalExchange(2)).clone()
        assert (counts["replay"] > 0) == plans
    assert torch.isfinite(outs[True]).all() and float(outs[True].abs().sum()) > 0
    assert torch.equal(outs[True], outs[False]), f"{int((outs[True] != outs[False]).sum())} pixels differ between USE_PLANS on and off"
