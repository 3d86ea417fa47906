"""The halo seam of the row-slab forward without a GPU: the census of tests/slab_seam_cases.py's shapes, and its harness and planted faults
on the 15-tap stand-in for the update iteration (``test_distributed_cpu._fake_step``: a receptive field of exactly HALO = 7 rows, zero
padded at the edge of whatever it is given, like the conv kernels on a slab).  What passes here is what tests/test_slab_seam_gpu.py
relies on: without a fault the harness reproduces the full image on every rank's EXTENDED rows after every iteration, in both forms of
the exchange; every fault moves an owned row near a seam by more than 1e-3 - or, where ``INERT`` says why it cannot, moves nothing."""
import pytest
import torch

import slab_seam_cases as SC
from parity_check import check_elementwise
from s16_iteration_check import launch_edges
from test_distributed_cpu import _fake_step, _torch_copy
from test_oracle_golden import hashed

C = 5
shape_id = lambda s: f"{s[0]}x{s[1]}-G{s[2]}"


def test_census():
    """What the shapes are there for, from the product's own bookkeeping: a later edit of the list cannot quietly lose an edge."""
    from cer_mvs_amd import slab
    H = slab.HALO
    assert H == 7 and set(SC.OWNED) == set(SC.SHAPES) and set(SC.FAULT_SHAPES) <= set(SC.SHAPES)
    assert sorted(s[2] for s in SC.ONE_PER_G) == sorted({s[2] for s in SC.SHAPES}) and set(SC.ONE_PER_G) <= set(SC.SHAPES)
    seen = set()
    for h, w, G in SC.SHAPES:
        b = SC.bounds(h, G)
        assert slab.can_shard(h, G) and tuple(r1 - r0 for r0, r1, _, _ in b) == SC.OWNED[(h, w, G)]
        owned = [r1 - r0 for r0, r1, _, _ in b]
        if min(owned) == H:
            seen.add("top strip is bottom strip")
        if min(owned) < 2 * H:
            seen.add("strips overlap")
        if len(set(owned)) > 1:
            seen.add("uneven split")
        if h % G:
            seen.add("ragged final gather")
        for g, (r0, r1, e0, e1) in enumerate(b):
            assert e0 == max(r0 - H, 0) and e1 == min(r1 + H, h)
            if 0 < g < G - 1:
                seen.add("interior rank")
                if r1 - r0 == H:
                    seen.add("interior rank owns HALO rows")
            assert (r0 - e0 == H or g == 0) and (e1 - r1 == H or g == G - 1)       # (a halo towards a neighbour is never clipped)
            if (e0, e1) == (0, h):
                seen.add("slab is the whole image")
        if sum(1 for g in range(1, G - 1)) >= 2:
            seen.add("two interior ranks")
        if w % 2 and (H * w * 65) % 4:
            seen.add("padded strip half")
            assert slab.strip_half(w, 64) > H * w * 65 and slab.strip_half(w, 64) % 4 == 0
        # conv tiles of 16 columns (8 rows: the smallest the s16 convolutions launch): interior ones need 33 columns
        edges = [launch_edges(h, w, 8, True)] + [launch_edges(e1 - e0, w, 8, True) for _, _, e0, e1 in b]
        if w < 33:
            assert all("interior" not in e for e in edges)
        else:
            assert "interior" in edges[0]
            seen.add("interior conv tiles")
        assert all("border" in e for e in edges)
        if any("partial_x" in e for e in edges) and any("partial_y" in e for e in edges):
            seen.add("partial tiles")
    assert SC.bounds(14, 2) == [(0, 7, 0, 14), (7, 14, 0, 14)]
    assert SC.bounds(22, 3)[1] == (8, 15, 1, 22)
    assert seen == {"top strip is bottom strip", "strips overlap", "uneven split", "ragged final gather", "interior rank",
                    "interior rank owns HALO rows", "slab is the whole image", "two interior ranks",
                    "padded strip half", "interior conv tiles", "partial tiles"}, seen
    # the faults that cannot show: only where every slab is the whole image and every rank owns HALO rows
    for (h, w, G), faults in SC.INERT.items():
        assert all((e0, e1) == (0, h) and r1 - r0 == H for r0, r1, e0, e1 in SC.bounds(h, G)) and set(faults) == {"no_disp", "short", "swapped"}
    assert not set(SC.INERT) & set(SC.FAULT_SHAPES)


_FULL = {}


def full_and_start(h, w, G):
    """The full image's state after each of T stand-in iterations, and the slabs' start; computed once, never written."""
    key = (h, w, G)
    if key not in _FULL:
        net, disp = hashed((h * w, C), 77 + h), hashed((h * w,), 79 + h)
        ref, x, xd = [], net, disp
        for _ in range(SC.T):
            x, xd = _fake_step(x, h, w), _fake_step(xd[:, None], h, w)[:, 0].contiguous()
            ref.append((x, xd))
        _FULL[key] = (ref, SC.slab_start(h, w, G, lambda e0, e1: net[e0 * w:e1 * w].clone(), disp))
    return _FULL[key]


def fake_step(w):
    def step(d, stage):
        d.net = _fake_step(d.net, d.hs, w)
        d.disp = _fake_step(d.disp[:, None], d.hs, w)[:, 0].contiguous()
    return step


def run(shape, exchange, fault=None):
    h, w, G = shape
    ref, start = full_and_start(h, w, G)
    got = SC.slab_loop(start, 0, G, SC.T, exchange, fake_step(w), _torch_copy, lambda hs, w_: None, fault=fault)
    return ref, start, got


@pytest.mark.parametrize("exchange", ["p2p", "gather"])
@pytest.mark.parametrize("shape", SC.SHAPES, ids=shape_id)
def test_harness_reproduces_the_full_image(shape, exchange):
    h, w, G = shape
    ref, start, got = run(shape, exchange)
    assert len(got) == SC.T
    for it in range(SC.T):
        for d, (net, disp) in zip(start.slabs, got[it]):
            px = torch.arange(d.e0 * w, d.e1 * w)
            for name, x, r in (("net", net, ref[it][0]), ("disp", disp, ref[it][1])):
                rep = check_elementwise(x, r[d.e0 * w:d.e1 * w], torch.ones_like(x, dtype=torch.float64), 1e-6, 0.0,
                                        f"{shape_id(shape)} {exchange} iteration {it} rank {d.g}: {name}", h=h, w=w, pixels=px)
                assert rep.ok, rep.message()
    # the start is left as it was, and a second run gives the same bits
    again = SC.slab_loop(start, 0, G, SC.T, exchange, fake_step(w), _torch_copy, lambda hs, w_: None)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for x, y in zip(got, again) for a, b in zip(x, y))


@pytest.mark.parametrize("fault", SC.FAULTS)
@pytest.mark.parametrize("exchange", ["p2p", "gather"])
@pytest.mark.parametrize("shape", SC.SHAPES, ids=shape_id)
def test_planted_faults_move_owned_rows(shape, exchange, fault):
    """After T iterations: more than 1e-3 on an owned row, every failing row within 7 * T rows of a seam and the worst one named by the
    report - or, for the faults of ``INERT``, not one bit anywhere."""
    h, w, G = shape
    ref, start, got = run(shape, exchange, fault)
    clean = SC.slab_loop(start, 0, G, SC.T, exchange, fake_step(w), _torch_copy, lambda hs, w_: None)
    if fault in SC.INERT.get(shape, ()):
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for x, y in zip(got, clean) for a, b in zip(x, y))
        return
    worst, bad_rows, named = 0.0, set(), []
    for d, (net, disp) in zip(start.slabs, got[-1]):
        o0, o1 = (d.r0 - d.e0) * w, (d.r1 - d.e0) * w
        px = torch.arange(d.r0 * w, d.r1 * w)
        for name, x, r in (("net", net, ref[-1][0]), ("disp", disp, ref[-1][1])):
            rep = check_elementwise(x[o0:o1], r[d.r0 * w:d.r1 * w], torch.ones_like(x[o0:o1], dtype=torch.float64), 1e-6, 0.0,
                                    f"{fault} rank {d.g}: {name}", h=h, w=w, pixels=px)
            worst = max(worst, float((x[o0:o1] - r[d.r0 * w:d.r1 * w]).abs().max()))
            bad_rows |= set(rep.rows)
            if not rep.ok:
                named.append(rep.worst[0])
                assert f"row {rep.worst[0]}," in rep.message()
    assert worst > 1e-3, f"{fault} at {shape_id(shape)} ({exchange}): the owned rows moved by {worst:.3e} only"
    assert named and max(SC.rows_from_seam(sorted(bad_rows), h, G)) <= 7 * SC.T
    assert min(SC.rows_from_seam(named, h, G)) <= 7 * SC.T


def test_both_exchange_forms_see_the_same_fault():
    """The faults are planted on the strips themselves, so "p2p" and "gather" deliver the same wrong rows."""
    for fault in SC.FAULTS:
        a, b = run((22, 21, 3), "p2p", fault)[2], run((22, 21, 3), "gather", fault)[2]
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for p, q in zip(a, b) for x, y in zip(p, q))
