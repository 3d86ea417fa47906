"""The control flow of ``UpdateBlock.run`` (cer-mvs_amd/update.py) without a GPU and without the library: a fake loop object logs its
``step(..., delta=mode)`` and ``finish(ws)`` calls, ``ops.delta_sum``, ``_lib.LaunchPlan`` and ``_lib.recording`` are recording stand-ins
(the pattern of tests/test_drivers_cpu.py).  What is pinned, for 0 .. 4 iterations and every combination of ``FUSE_DELTA``, ``USE_PLANS``
and ``after``: the order of the modes, which iteration is recorded and which are replays, one trailing ``delta_sum`` exactly when the loop
fused, ``finish`` iff anything ran, ``after(i)`` behind every iteration (replayed ones too), and that the plan keeps the buffers whose
pointers it captured.  tests/test_update_run_gpu.py holds the same protocols to identical bits on the device.

Event tokens: ``S:<mode>`` a step through the wrappers, ``[`` / ``]`` a recording opens / closes (the step between them is the recorded
one), ``P`` a replay, ``A<i>`` the callback, ``D`` the stand-alone delta_sum, ``F`` finish."""
import itertools
from types import SimpleNamespace

import pytest

ITERS = (0, 1, 2, 3, 4)
D2B = 0.375
H, W, D, INCRE = 9, 21, 64, 0.0025 / 64


class FakeLoop:
    def __init__(self, log, fuse):
        self.log, self.FUSE_DELTA, self.d2b, self.step_args = log, fuse, D2B, []

    def step(self, *args, delta="now"):
        self.step_args.append(args)
        self.log.append(f"S:{delta}")

    def finish(self, ws):
        self.finish_ws = ws
        self.log.append("F")


class FakeBlock:
    """What ``run`` touches of an UpdateBlock: ``loop(stage, device)``."""

    def __init__(self, loop, log):
        self._loop, self.log, self.asked = loop, log, []

    def loop(self, stage, device):
        self.asked.append((stage, device, len(self.log)))
        return self._loop


@pytest.fixture
def rig(monkeypatch):
    """-> run(iters, fuse, plans, after) -> SimpleNamespace(log, plans, loop, block, bufs, dsum)."""
    from cer_mvs_amd import _lib as L, ops, update

    def run(iters, fuse, plans, after):
        log, made, dsum = [], [], []

        class Plan:
            def __init__(self, keep=()):
                self.keep = list(keep)
                made.append(self)

            def replay(self):
                log.append("P")

        class Recording:
            def __init__(self, plan):
                self.plan = plan

            def __enter__(self):
                assert self.plan is made[-1]
                log.append("[")
                return self.plan

            def __exit__(self, *exc):
                log.append("]")
                return False

        def delta_sum(T, bias, disp_in, h, w, disp_out=None, want_delta=True):
            dsum.append((T, bias, disp_in, h, w, disp_out, want_delta))
            log.append("D")
            return disp_out, None
        monkeypatch.setattr(update, "USE_PLANS", plans)
        monkeypatch.setattr(L, "LaunchPlan", Plan)
        monkeypatch.setattr(L, "recording", Recording)
        monkeypatch.setattr(ops, "delta_sum", delta_sum)
        loop = FakeLoop(log, fuse)
        block = FakeBlock(loop, log)
        b = SimpleNamespace(vol=object(), origin=object(), net_l=SimpleNamespace(device="dev0"), disp=object(), hoisted=(object(), object()),
                            ws={"T": object(), "c2": object()})
        cb = (lambda i: log.append(f"A{i}")) if after else None
        update.UpdateBlock.run(block, iters, b.vol, b.origin, b.net_l, b.disp, b.hoisted, 1, H, W, D, INCRE, b.ws, after=cb)
        return SimpleNamespace(log=log, plans=made, loop=loop, block=block, bufs=b, dsum=dsum)
    return run


def expected(iters, fuse, plans, after):
    """The issue's description of the three protocols, spelled as an event list."""
    fused = fuse and not after and iters >= 2
    ev = []
    recorded = False
    for i in range(iters):
        mode = ("defer" if i == 0 else "apply+defer") if fused else "now"
        if not plans or mode == "defer":
            ev.append(f"S:{mode}")
        elif not recorded:
            ev += ["[", f"S:{mode}", "]"]
            recorded = True
        else:
            ev.append("P")
        if after:
            ev.append(f"A{i}")
    return ev + (["D"] if fused else []) + (["F"] if iters else [])


# the shipped protocols written out by hand, so that ``expected`` is itself pinned: (iters, FUSE_DELTA, USE_PLANS, after) -> events
LITERAL = {
    (4, True, True, False): "S:defer [ S:apply+defer ] P P D F",                    # fused + replayed: what a forward runs
    (4, True, False, False): "S:defer S:apply+defer S:apply+defer S:apply+defer D F",
    (4, True, True, True): "[ S:now ] A0 P A1 P A2 P A3 F",                         # the slab exchange: never fused, iteration 0 recorded
    (4, True, False, True): "S:now A0 S:now A1 S:now A2 S:now A3 F",
    (4, False, True, False): "[ S:now ] P P P F",                                   # the wide forms
    (4, False, False, False): "S:now S:now S:now S:now F",
    (3, True, True, False): "S:defer [ S:apply+defer ] P D F",                      # the first replay
    (2, True, True, False): "S:defer [ S:apply+defer ] D F",                        # recorded, never replayed
    (1, True, True, False): "[ S:now ] F",                                          # one iteration does not fuse
    (1, True, False, False): "S:now F",
    (0, True, True, False): "",
    (0, True, True, True): "",
}


@pytest.mark.parametrize("key", sorted(LITERAL), ids=lambda k: "-".join(str(int(x)) for x in k))
def test_shipped_sequences_by_hand(rig, key):
    got = rig(*key)
    assert got.log == LITERAL[key].split()
    assert expected(*key) == LITERAL[key].split()


@pytest.mark.parametrize("fuse,plans,after", list(itertools.product((True, False), repeat=3)),
                         ids=lambda v: str(int(v)))
@pytest.mark.parametrize("iters", ITERS)
def test_event_sequence(rig, iters, fuse, plans, after):
    r = rig(iters, fuse, plans, after)
    b = r.bufs
    assert r.log == expected(iters, fuse, plans, after)
    fused = fuse and not after and iters >= 2
    # modes in order
    modes = [e[2:] for e in r.log if e.startswith("S:")]
    n_replay = r.log.count("P")
    if fused:
        assert modes[0] == "defer" and set(modes[1:]) == {"apply+defer"}
    else:
        assert set(modes) <= {"now"}
    assert len(modes) + n_replay == iters
    # which iteration is recorded, which replay: nothing pending may be recorded ("defer" is never inside a recording), one plan at most,
    # and every replay comes after the recording closed
    assert len(r.plans) == (1 if plans and iters >= (2 if fused else 1) else 0)
    if r.plans:
        o, c = r.log.index("["), r.log.index("]")
        assert c == o + 2 and r.log[o + 1] == ("S:apply+defer" if fused else "S:now") and r.log.count("[") == 1
        assert all(i > c for i, e in enumerate(r.log) if e == "P")
        assert n_replay == iters - (2 if fused else 1)
        keep = r.plans[0].keep
        for t in (b.vol, b.origin, b.net_l, b.disp, b.hoisted, b.ws):
            assert any(k is t for k in keep)
    else:
        assert n_replay == 0 and "[" not in r.log
    # exactly one trailing delta_sum when fused, on the loop's tap planes and bias, in place on the disparity
    assert len(r.dsum) == (1 if fused else 0)
    if fused:
        assert r.log[-2:] == ["D", "F"]
        T, bias, disp_in, h, w, disp_out, want = r.dsum[0]
        assert T is b.ws["T"] and bias == D2B and disp_in is b.disp and disp_out is b.disp and (h, w) == (H, W) and want is False
    # finish iff anything ran, last, on the workspace
    assert r.log.count("F") == (1 if iters else 0)
    if iters:
        assert r.log[-1] == "F" and r.loop.finish_ws is b.ws
    # after(i) behind every iteration, in order, replayed ones included
    calls = [e for e in r.log if e.startswith("A")]
    assert calls == ([f"A{i}" for i in range(iters)] if after else [])
    if after:
        work = [i for i, e in enumerate(r.log) if e in ("P", "]") or (e.startswith("S:") and (i == 0 or r.log[i - 1] != "["))]
        assert [r.log[i + 1] for i in work] == calls
    # every step got the caller's buffers, in the order of ``step``'s signature
    for args in r.loop.step_args:
        assert len(args) == 10 and all(x is y for x, y in zip(args, (b.vol, b.origin, b.net_l, b.disp, b.hoisted)))
        assert args[5:9] == (H, W, D, INCRE) and args[9] is b.ws
    # the loop object (weight packing is host work) is fetched once, before anything is recorded, for the stage asked
    assert r.block.asked == [(1, "dev0", 0)]


@pytest.mark.parametrize("stage", [0, 1])
def test_loop_ref64_is_the_oracle_in_float64(stage):
    """``parity_check.loop_ref64`` - the anchor of tests/test_update_run_gpu.py - restates T iterations from the per-launch pieces (hoisting
    nothing, tap planes and ``delta_sum64`` for the delta head).  The oracle's own iteration (pyramid, lookup, update_block, disp + delta)
    evaluated in float64 must agree with it to float64 rounding, at a ragged size, for both stages' delta heads."""
    import torch
    from cer_mvs_amd import RAFT, update
    from cer_mvs_amd.synthetic import fill_state_dict
    from oracle import cer_oracle as O
    from parity_check import loop_ref64
    from test_oracle_golden import hashed
    h, w, T = 9, 21, 3
    P = h * w
    D, incre = ((64, 0.0025 / 64), (44, 0.0025 / 320))[stage]
    model = RAFT(cascade=[(64, 64, T), (-1, 320, T)], test_mode=True, gru_precision="s16")
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
    sd = {k: v.detach().double() for k, v in model.state_dict().items() if k.startswith("update_block.")}
    g = update._stage_weights(model.update_block, stage, "cpu")
    vol = hashed((P, D), 11, -4.0, 4.0).double()
    origin = hashed((P,), 12, 0.001, 0.0015).double()
    disp = origin + hashed((P,), 13, -40.0, 60.0).double() * incre
    net = torch.tanh(hashed((P, 64), 14, -2.0, 2.0)).double()
    inp = torch.relu(hashed((P, 64), 15, -1.0, 2.0)).double()
    got = loop_ref64(T, vol, origin, net, disp, inp, g, D, incre, h, w)
    nchw = lambda x: x.t().reshape(1, -1, h, w).contiguous()
    levels = O.pyramid(vol[None], 3)
    n, i, d = nchw(net), nchw(inp), disp.reshape(1, 1, h, w)
    for it in range(T):
        feats = O.lookup(levels, origin.reshape(h, w), d[0, 0], D, incre, 5)
        n, delta = O.update_block(sd, n, i, d, feats, stage)
        d = d + delta
        assert n.dtype == torch.float64 and d.dtype == torch.float64
        assert float((got[it][0] - n[0].permute(1, 2, 0).reshape(P, 64)).abs().max()) < 1e-12, it
        assert float((got[it][1] - d.reshape(P)).abs().max()) < 1e-12 * incre * 1e3, it
        assert float((got[it][1] - disp).abs().max()) > incre / 100             # (the iterations moved the disparity)
