"""Saturation is never silent: flag-or-parity at every clamp site that has a reporter (run on the GPU box: pytest -m gpu).

The parity modules prove the kernels right INSIDE the f16 range of their split operands.  DESIGN.md 3f and include/cer_mvs.h promise that
a value which leaves it raises a bit of the sticky device flag.  tests/saturation_cases.py lists every clamp site and who reports it;
here each reporter is made to fire, one planted value at a time:

  (a) threshold pins      the same launch three times - the clean side of the threshold (flag 0), the flag side (exactly the site's bit), NaN
                          (the bit too).  In-kernel checks are exact: 4094.0 / 1023.5 / 5.1175 clean, the next float flagged.
  (b) coverage            one hot (pixel, channel) per launch, everything else below a quarter of the threshold by the float64 reference of
                          that launch; the plant walks the position classes of the site's tiling (first / last pixel, partial last tile
                          column and row, the one-row last m-tile, an interior and a rim pixel; the first and last channel of every
                          16-group) in every arithmetic form and with every tile height the family exists for.  Each plant must raise
                          the bit.  The opposite direction: clean inputs with NaN-poisoned padding slots into a garbage-filled
                          destination must leave the flag alone, and a scan of the whole c2 buffer must be clean.
  (c) flag-or-parity      the hot value runs over ``saturation_cases.SWEEP``: either the bit is raised or every output element is within
                          the bound of tests/s16_iteration_check.py against the float64 reference WITHOUT any clamp.
  protocol level          ``UpdateBlock.run`` with T = 3: the volume scaled up for exactly one iteration k, on the wrappers (``after=``) and
                          on the fused, plan-replaying protocol - bit 4 for every k; a stage-0-only saturation through RAFT.forward and
                          slab.sharded_forward; the overflow policies on real forwards.
  unreported clamps       the f16x3 loop's split (conv3x3 RELU with ``out_split``, the lookup's split32 output): 60000 within parity,
                          1e5 comes back as exactly 65504, finite, no flag - pinned so that the limit stays on paper.

  reported upstream       the disparity features that the s16 convs generate clamp beyond a difference of 10.235 with no check in the conv:
                          the writers of the disparity raise bit 8 (pinned at 5.1175), and one z|r launch with a planted disparity of 10.2
                          (within parity) and 10.3 (finite, clamped) shows the site itself.

Measured on an MI355X (profiles/saturation_parity.json, written only under CER_PARITY_RECORD=1 by a whole-module run; a plain run writes
nothing): 66 cases in 2.6 s of module wall time (4.4 s with start-up), the slowest 0.29 s (the pipeline of three replicas).  Worst |err| / bound
on the parity side of the sweep, f16x3 terms / fp8 / FP6: corr2 0.87 / 0.18 / 0.14, delta head 0.27 / 0.18 / 0.11, lookup 0.49, the generated
disparity features at 10.2 <= 0.016.  What was red on the parent commit: DESIGN.md 3f."""
import copy
import json
import os
import time
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
import saturation_cases as S
from parity_check import check_elementwise, conv_ref, disp_feature_parts, lookup_ref, poison_f16, poison_f32, wsum
from s16_iteration_check import ACT_ABS, C_CONV, FORMS, update_block, expected_tile_height, frag_poisoned_padding, s16_grid, unfrag
from test_oracle_golden import hashed

pytestmark = pytest.mark.gpu

SHAPES = ((37, 33), (33, 37))
CORR2_MT = {"f16x3terms": (2, 3, 4), "fp8corr": (2, 3), "fp6corr": (2, 3)}
DELTA_MT = (2, 4)
F8 = {"f16x3terms": False, "fp8corr": True, "fp6corr": 6}
NAN_HALF = 0x7E00
RAN = {}                 # {(site, form, tile height or 0): set of position classes at which a single plant raised the bit}
SWEPT = {}               # {(site, form): [planted cases, worst ratio to bound on the parity side]}
TIMES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def drain(dev):
    """Leave both the sticky flag and the lazy policy's snapshot clear."""
    from cer_mvs_amd import ops
    torch.cuda.synchronize()
    ops.overflow_poll(dev)
    return ops.check_overflow(dev)


@pytest.fixture(scope="module", autouse=True)
def _module_setup(dev):
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    drain(dev)
    t0 = time.time()
    yield
    torch.set_num_threads(n)
    drain(dev)
    if os.environ.get("CER_PARITY_RECORD") and "census" in TIMES:      # a whole-module run only
        slow = max(TIMES, key=TIMES.get)
        out = {"sweep": {f"{k[0]}/{k[1]}": {"planted": v[0], "worst_ratio_to_bound": v[1]} for k, v in sorted(SWEPT.items())},
               "fired": {f"{k[0]}/{k[1]}/th{k[2]}": sorted(v) for k, v in sorted(RAN.items())},
               "module_wall_s": round(time.time() - t0, 1), "slowest_case": [slow, round(TIMES[slow], 2)]}
        with open(os.path.join(REPO, "profiles", "saturation_parity.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _hygiene(dev, request):
    """The flag is process-sticky: every test starts and ends with it (and the lazy snapshot) clear; ``ops.TILE_MT`` goes back to 0."""
    from cer_mvs_amd import ops
    drain(dev)
    t0 = time.time()
    try:
        yield
    finally:
        ops.TILE_MT = 0
        drain(dev)
        TIMES[request.node.name] = time.time() - t0


def flag(dev):
    from cer_mvs_amd import ops
    return ops.check_overflow(dev)


def pixel_classes(h, w):
    """The position classes of the 16-column tiles and 2-row m-tiles at an odd-height ragged shape -> {class: pixel index}."""
    assert h % 2 == 1 and w % 16 and h > 32 and w > 32
    yx = {"first": (0, 0), "last": (h - 1, w - 1), "partial_col": (1, w - 1), "partial_row": (h - 1, 3), "one_row_odd": (h - 1, 17),
          "interior": (17, 17), "rim": (0, 17)}
    return {k: y * w + x for k, (y, x) in yx.items()}


def plant_half(fr, h, w, log2s, p, ch, bits=NAN_HALF):
    """Overwrite the hi half of (pixel p, channel ch) of a frag16 tensor with ``bits`` (NaN): found through the layout kernel itself."""
    from cer_mvs_amd import ops
    mark = torch.zeros(h * w, fr.shape[1], device=fr.device)
    mark[p, ch] = 1.0
    at = ops.to_frag16(mark, h, w, log2s).view(torch.int16).reshape(-1).nonzero()
    assert at.numel() == 1
    fr.view(torch.int16).reshape(-1)[int(at)] = bits
    return fr


def note_sweep(site, form, rep):
    s = SWEPT.setdefault((site, form), [0, 0.0])
    s[0] += 1
    if rep is not None:
        s[1] = max(s[1], float(rep.max_ratio))


# ================================================================================================ feature rows (bit 1)
def test_feat_split_pins_and_coverage(dev):
    """cer_feat_split_f16 at (3, 37) blocks x texels: +-1023.5 clean, the next float flagged, NaN and inf flagged; every block's first and
    last texel, both 8-channel halves of every 16-group, both signs."""
    from cer_mvs_amd import ops
    base = hashed((3, 37, 64), 4101, -1.0, 1.0).to(dev)

    def run(b, t, c, v):
        x = base.clone()
        x[b, t, c] = float(v)
        ops.feat_split(x)
        return flag(dev)
    assert run(1, 5, 7, 0.5) == 0
    for sign in (1.0, -1.0):
        assert run(1, 5, 7, sign * S.FEAT_CLEAN) == 0, "1023.5 * 64 = 65504 is not clamped"
        assert run(1, 5, 7, sign * S.FEAT_FLAG) == S.BIT_FEAT
        assert run(1, 5, 7, sign * float("inf")) == S.BIT_FEAT
    assert run(1, 5, 7, float("nan")) == S.BIT_FEAT and flag(dev) == 0                       # (reading clears it)
    fired = set()
    for b, t, cls in ((0, 0, "first"), (2, 36, "last"), (0, 36, "block_seam"), (1, 0, "block_seam")):
        for c in (0, 7, 8, 15, 16, 31, 32, 47, 48, 63):
            for sign in (1.0, -1.0):
                assert run(b, t, c, sign * 1500.0) == S.BIT_FEAT, (b, t, c, sign)
        fired.update((cls, "sign", "channels"))
    RAN[("feat_split", "-", 0)] = fired


def test_fsplit_head_fires(dev):
    """The encoder head's own check (PC_EPI_FSPLIT, bit 1) seen to fire: clean on the parity module's inputs, raised by one hot bias channel
    (first and last of the 64) and by one hot input pixel."""
    import test_encoder_parity_gpu as EP
    from cer_mvs_amd import ops
    _, cin, cout, taps, stride, _ = EP.INST["fsplit"]
    (form,) = EP.FORMS["none"]["fsplit"]
    N, h, w = 3, 9, 67
    A, sA, B, sB = EP.make_inputs(dev, form, N, h, w, cin, 8501)
    fl = ops.overflow_flag(dev)
    planes = lambda: torch.full((N, h * w, 128), float("nan"), device=dev, dtype=torch.float16)
    conv, wt, b = EP.packed_conv(dev, "fsplit")
    for f6 in (False, True):
        EP.pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, 3, f6=f6, out=planes(), scale=0.125, flag=fl)
        assert flag(dev) == 0
    fired = set()
    for ch in (0, cout - 1):
        hot = b.clone()
        hot[ch] = 9000.0                                           # * 1/8 = 1125 > 1023.5 at every pixel of one channel
        conv_h, _, _ = EP.packed_conv(dev, "fsplit", bias=hot)
        for f6 in (False, True):
            EP.pc_conv(dev, conv_h, A, sA, B, sB, form, N, h, w, 3, f6=f6, out=planes(), scale=0.125, flag=fl)
            assert flag(dev) == S.BIT_FEAT, (ch, f6)
        fired.add("bias_channel")
    for n, p in ((0, 0), (N - 1, h * w - 1), (1, 4 * w + 40)):
        A2 = A.clone()
        A2[n, p] = 3.0e5 * torch.sign(wt[5, :, 0, 0]).to(dev)      # output channel 5 of that pixel: 3e5 * sum |w| / 8, far beyond 1023.5
        assert float(3.0e5 * wt[5].abs().sum() / 8) > 4 * 1023.5
        EP.pc_conv(dev, conv, A2, sA, B, sB, form, N, h, w, 3, out=planes(), scale=0.125, flag=fl)
        assert flag(dev) == S.BIT_FEAT, (n, p)
        fired.add("input_pixel")
    RAN[("fsplit_head", "-", 0)] = fired


# ================================================================================================ lookup -> c1 (bit 4, in the kernel)
LK = SimpleNamespace(h=9, w=21, D=64, incre=0.0025 / 64)


def lookup_case(dev, p, ch, v, nan=False, split=2):
    """A constant cost row of 1.0 for pixel ``p`` with its disparity mid-range (every tap of every level reads 1.0), all other rows tiny;
    column ``ch`` of the 1x1 weight is zero but for tap 0 = ``v``: out[p, ch] = v exactly.  -> (features, float64 reference, mag, idx)."""
    from cer_mvs_amd import _lib as L, ops
    P = LK.h * LK.w
    _, _, rs = ops.row_layout(LK.D, 3, compact=True)
    vol = hashed((P, rs), 4201, -0.01, 0.01)
    vol[p] = 1.0
    if nan:
        vol[p, LK.D // 2] = float("nan")
    origin = hashed((P,), 4202, 0.001, 0.0015)
    disp = origin + hashed((P,), 4203, -20.0, 20.0) * LK.incre
    disp[p] = origin[p]
    w0t, b0 = hashed((33, 64), 4204, -0.02, 0.02), hashed((64,), 4205, -0.1, 0.1)
    w0t[:, ch] = 0.0
    w0t[0, ch] = float(v)
    b0[ch] = 0.0
    vol_d = vol.to(dev)
    vol_d.level0_only = True
    kw = dict(out_split=2, log2s=L.S16_RELU, img_w=LK.w) if split == 2 else dict(out_split=True)
    out = poison_f16(torch.empty(ops.s16_pixels(LK.h, LK.w) if split == 2 else P, 64, device=dev))
    ops.lookup_encode(vol_d, origin.to(dev), disp.to(dev), w0t.to(dev), b0.to(dev), LK.D, LK.incre, 3, 5, out=out, **kw)
    ref = None if nan else lookup_ref(vol.double(), origin.double(), disp.double(), w0t.double(), b0.double(), LK.D, LK.incre)
    return out, ref


def test_lookup_pins(dev):
    p, ch = 4 * LK.w + 10, 17
    _, (ref, _, _) = lookup_case(dev, p, ch, S.ACT_CLEAN)
    assert float(ref[p, ch]) == 4094.0 and flag(dev) == 0, "4094.0 * 16 = 65504 is not clamped"
    lookup_case(dev, p, ch, S.ACT_FLAG)
    assert flag(dev) == S.BIT_ACT and flag(dev) == 0
    lookup_case(dev, p, ch, 1.0, nan=True)
    assert flag(dev) == S.BIT_ACT, "a NaN in the cost row of one pixel must be reported, not turned into 0 by the ReLU"
    lookup_case(dev, p, ch, float("inf"))
    assert flag(dev) == S.BIT_ACT


def test_lookup_coverage(dev):
    """9 x 21 (131 of 320 padding slots, three 64-pixel tiles, the last one partial): one hot output at a time."""
    P = LK.h * LK.w
    px = {"first": 0, "last": P - 1, "partial_col": 1 * LK.w + 20, "partial_row": 8 * LK.w + 3, "one_row_odd": 8 * LK.w + 17, "interior": 4 * LK.w + 10,
          "rim": 10, "tile_seam": 63, "tile_seam2": 64}
    fired = set()
    for cls, p in px.items():
        for ch in (S.CH64 if cls == "interior" else (0, 63)):
            _, (ref, _, _) = lookup_case(dev, p, ch, 5000.0)
            rest = ref.clone()
            rest[p, ch] = 0.0
            assert float(ref[p, ch]) == 5000.0 and float(rest.max()) < S.ACT_LIMIT / 4
            assert flag(dev) == S.BIT_ACT, (cls, p, ch)
        fired.add(cls.rstrip("2"))
    fired.add("channels64")
    RAN[("lookup", "-", 0)] = fired


def test_lookup_sweep(dev):
    from cer_mvs_amd import _lib as L
    p, ch = 4 * LK.w + 10, 33
    for v in S.SWEEP:
        out, (ref, mag, idx) = lookup_case(dev, p, ch, v)
        bits = flag(dev)
        assert bits in (0, S.BIT_ACT)
        rep = None
        if not bits:
            rep = check_elementwise(unfrag(out, LK.h, LK.w, L.S16_RELU), ref, mag, C_CONV, idx + 2.0 ** (-24 - L.S16_RELU), f"lookup, planted {v}",
                                    h=LK.h, w=LK.w)
            assert rep.ok, f"planted {v}: no flag and not within parity of the unclamped reference\n{rep.message()}"
        assert bits or v <= S.ACT_SCAN_CLEAN
        note_sweep("lookup", "-", rep)


def test_lookup_split32_clamp_is_unreported(dev):
    """The f16x3 loop's c1 (split32 output, cer_split8): 60000 comes back within parity, 1e5 as exactly 65504 - finite, and NO flag."""
    from cer_mvs_amd import ops
    p, ch = 4 * LK.w + 10, 33
    out, (ref, mag, idx) = lookup_case(dev, p, ch, 60000.0, split=1)
    got = ops.split32(out, inverse=True).cpu().double()
    rep = check_elementwise(got, ref, mag, C_CONV, idx + 2.0 ** -24, "lookup split32, planted 60000", h=LK.h, w=LK.w)
    assert rep.ok and flag(dev) == 0, rep.message()
    out, _ = lookup_case(dev, p, ch, 1.0e5, split=1)
    got = ops.split32(out, inverse=True)
    assert float(got[p, ch]) == S.F16_MAX and bool(torch.isfinite(got).all()) and flag(dev) == 0


# ================================================================================================ corr2 -> c2 (bit 4, in the kernel)
_PACKS = {}


def corr2_pack(dev, form, gain=2.0):
    """64 -> 64 conv, small weights; the centre tap of (co, ci = co) is ``gain`` and of (co, ci = co + 1) 2^-8: a hot c1[p, co] lands on
    c2[p, co] alone, and c1[p, co + 1] = 2^-4 adds exactly 2^-12 to it."""
    from cer_mvs_amd import _lib as L, ops
    key = ("corr2", form, gain)
    if key not in _PACKS:
        wt = hashed((64, 64, 3, 3), 4301, -0.02, 0.02)
        for co in range(64):
            wt[co, co, 1, 1] = gain
            wt[co, (co + 1) % 64, 1, 1] = 2.0 ** -8
        _PACKS[key] = (ops.PackedConvS16(wt, torch.zeros(64), [(64, 2, L.S16_RELU)], dev, corr_fp8=F8[form]), wt)
    return _PACKS[key]


def corr2_row_pack(dev, form, co, gain):
    """The sweep's conv: the WHOLE centre tap of output channel ``co`` is ``gain`` (64 input channels - the correction terms of the fp8 / FP6
    forms are block-scaled along the input channels, so a lone large weight inside a block is not what they are built for), the rest small."""
    from cer_mvs_amd import _lib as L, ops
    key = ("corr2_row", form, co, gain)
    if key not in _PACKS:
        wt = hashed((64, 64, 3, 3), 4301, -0.02, 0.02)
        wt[co, :, 1, 1] = gain
        _PACKS[key] = (ops.PackedConvS16(wt, torch.zeros(64), [(64, 2, L.S16_RELU)], dev, corr_fp8=F8[form]), wt)
    return _PACKS[key]


def corr2_launch(dev, form, mt, h, w, plants, gain=2.0, nan_at=None, base=None, pack=None):
    """c1 = ``base`` (default zeros) with ``plants`` {(pixel, channel): value}, NaN-poisoned padding slots, into a NaN-filled c2 ->
    (c2 frag16, c1 read back as float64)."""
    from cer_mvs_amd import _lib as L, ops
    ops.TILE_MT = mt
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert s16_grid(h, w, 64, form, ncu, mt)[1] == expected_tile_height(64, form, mt) == 4 * (mt or 2)
    pc = corr2_pack(dev, form, gain)[0] if pack is None else pack
    x = torch.zeros(h * w, 64) if base is None else base.clone()
    for (p, c), v in plants.items():
        x[p, c] = v
    c1 = frag_poisoned_padding(x.to(dev), h, w, L.S16_RELU)
    if nan_at is not None:
        plant_half(c1, h, w, L.S16_RELU, *nan_at)
    c2 = poison_f16(torch.empty(ops.s16_pixels(h, w), 64, device=dev))
    ops.conv3x3_s16(pc, [c1], h, w, L.EPI_RELU, out=c2, out_split=True, log2s_out=L.S16_RELU)
    return c2, (None if nan_at is not None else unfrag(c1, h, w, L.S16_RELU))


CORR2_CASES = [(h, w, form, mt) for h, w in SHAPES for form in FORMS for mt in CORR2_MT[form]]


@pytest.mark.parametrize("h,w,form,mt", CORR2_CASES, ids=[f"{h}x{w}-{f}-mt{m}" for h, w, f, m in CORR2_CASES])
def test_corr2_pins_and_coverage(dev, h, w, form, mt):
    """The RELU epilogue checks what it clamps.  Pins: 2047 * 2 = 4094.0 clean, + 2^-4 * 2^-8 flagged (all operands exact in f16, so every
    arithmetic form computes them exactly), a NaN half in c1 flagged.  Coverage: c2[p, co] = 2500 * 2 at one position at a time."""
    from cer_mvs_amd import _lib as L, ops
    cls = pixel_classes(h, w)
    p, co = cls["interior"], 17
    c2, _ = corr2_launch(dev, form, mt, h, w, {(p, co): 2047.0})
    assert flag(dev) == 0 and float(unfrag(c2, h, w, L.S16_RELU)[p, co]) == 4094.0, "4094.0 is not clamped and must not be reported"
    corr2_launch(dev, form, mt, h, w, {(p, co): 2047.0, (p, co + 1): 2.0 ** -4})
    assert flag(dev) == S.BIT_ACT, "4094 + 2^-12 is clamped: bit 4"
    assert flag(dev) == 0
    corr2_launch(dev, form, mt, h, w, {}, nan_at=(p, co))
    assert flag(dev) == S.BIT_ACT, "a NaN half in c1 must be reported, not turned into 0 by the ReLU"
    _, wt = corr2_pack(dev, form)
    fired = set()
    for name, px in cls.items():
        for ch in (S.CH64 if name == "interior" else (0, 63)):
            c2, c1_rb = corr2_launch(dev, form, mt, h, w, {(px, ch): 2500.0})
            ref, _ = conv_ref(c1_rb, c1_rb.abs(), wt, None, h, w)
            ref = torch.relu(ref)
            assert float(ref[px, ch]) == 5000.0
            ref[px, ch] = 0.0
            assert float(ref.max()) < S.ACT_LIMIT / 4
            assert flag(dev) == S.BIT_ACT, f"one hot c2 at the {name} pixel {px}, channel {ch}: no flag ({form}, {4 * mt}-row tiles)"
        fired.add(name)
    fired.add("channels64")
    RAN[("corr2", form, 4 * mt)] = RAN.get(("corr2", form, 4 * mt), set()) | fired


@pytest.mark.parametrize("form,mt", [(f, m) for f in FORMS for m in CORR2_MT[f]])
def test_corr2_clean_launch_is_silent(dev, form, mt):
    """The opposite direction: c1 in the full-size module's range with NaN in its padding slots, c2's buffer full of NaN halves - no flag
    from the kernel, and a scan of the WHOLE c2 buffer (the epilogue stores whole m-tiles) is clean too."""
    from cer_mvs_amd import ops
    h, w = 37, 33
    base = torch.relu(hashed((h * w, 64), 4310, -1.0, 3.0))
    c2, _ = corr2_launch(dev, form, mt, h, w, {}, base=base)
    assert flag(dev) == 0
    ops.scan_overflow(c2)
    assert flag(dev) == 0, "a padding slot of c2 still holds a sentinel or a saturated half after one clean launch"


@pytest.mark.parametrize("form", list(FORMS))
def test_corr2_sweep(dev, form):
    from cer_mvs_amd import _lib as L
    h, w = 37, 33
    p, co, R = pixel_classes(h, w)["interior"], 33, L.S16_RELU
    base = torch.relu(hashed((h * w, 64), 4311, -1.0, 2.0))      # (c1 in the full-size module's range: the bounds are derived for it)
    for v in S.SWEEP:
        # one pixel of c1 at 16 in all 64 channels; the centre tap of channel ``co`` has the gain: c2[p, co] = v, c2[q, co] < v / 16 elsewhere.
        # (Measured while building this: a lone c1 of 2000, a lone weight of 60 among weights of 0.02, or a c1 of order 0.01 miss the
        # per-element bound of the fp8 / FP6 forms by ~4 x away from the hot output - their correction terms are block-scaled along the
        # input channels and have an absolute floor.  Not a saturation matter; the sweep keeps operands where the bound is derived.)
        pack, wt = corr2_row_pack(dev, form, co, v / 1024.0)
        c2, c1_rb = corr2_launch(dev, form, 0, h, w, {(p, c): 16.0 for c in range(64)}, base=base, pack=pack)
        bits = flag(dev)
        assert bits in (0, S.BIT_ACT)
        rep = None
        if not bits:
            ref, mag = conv_ref(c1_rb, c1_rb.abs(), wt, None, h, w)
            assert abs(float(ref[p, co]) - v) < 1e-3 * v
            rep = check_elementwise(unfrag(c2, h, w, R), torch.relu(ref), mag, C_CONV * FORMS[form][1], 2.0 ** (-24 - R) * (wsum(wt) + 1),
                                    f"corr2 {form}, planted {v}", h=h, w=w)
            assert rep.ok, f"planted {v}: no flag and not within parity of the unclamped reference\n{rep.message()}"
        assert bits or v <= S.ACT_SCAN_CLEAN, f"planted {v}: clamped without a flag"
        note_sweep("corr2", form, rep)


# ================================================================================================ delta head (bit 2, in the kernel)
def delta_pack(dev, form, co, gain, exact=False):
    """64 -> 256 conv, small weights.  ``exact``: the centre tap of (co, ci = 5) is ``gain`` and of (co, ci = 6) 2^-6 (pins); else the whole
    centre tap of ``co`` is ``gain``: a hidden state of 0.9 in all channels of one pixel gives hid[p, co] = 57.6 * gain."""
    from cer_mvs_amd import _lib as L, ops
    key = ("delta", form, co, gain, exact)
    if key not in _PACKS:
        wt = hashed((256, 64, 3, 3), 4401, -0.02, 0.02)
        if exact:
            wt[co, 5, 1, 1], wt[co, 6, 1, 1] = gain, 2.0 ** -6
        else:
            wt[co, :, 1, 1] = gain
        if "proj" not in _PACKS:
            w2 = hashed((1, 256, 3, 3), 4402, -0.1, 0.1)
            _PACKS["proj"] = (ops.delta_proj_pack_s16(w2, dev), w2)
        _PACKS[key] = (ops.PackedConvS16(wt, torch.zeros(256), [(64, 2, L.S16_UNIT)], dev, corr_fp8=F8[form]), wt)
    return _PACKS[key]


def delta_launch(dev, form, mt, h, w, pack, plants, nan_at=None, base=None):
    from cer_mvs_amd import _lib as L, ops
    ops.TILE_MT = mt
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert s16_grid(h, w, 256, form, ncu, mt)[1] == expected_tile_height(256, form, mt) == (2 * mt if mt else 4)
    x = torch.zeros(h * w, 64) if base is None else base.clone()
    for (p, c), v in plants.items():
        x[p, c] = v
    net = frag_poisoned_padding(x.to(dev), h, w, L.S16_UNIT)
    if nan_at is not None:
        plant_half(net, h, w, L.S16_UNIT, *nan_at)
    T = poison_f32(torch.empty(2, 9, h * w, device=dev))
    ops.conv3x3_s16(pack, [net], h, w, L.EPI_DELTA, out=T, aux=_PACKS["proj"][0])
    return T, (None if nan_at is not None else unfrag(net, h, w, L.S16_UNIT))


DELTA_CASES = [(h, w, form, mt) for h, w in SHAPES for form in FORMS for mt in DELTA_MT]


@pytest.mark.parametrize("h,w,form,mt", DELTA_CASES, ids=[f"{h}x{w}-{f}-mt{m}" for h, w, f, m in DELTA_CASES])
def test_delta_head_pins_and_coverage(dev, h, w, form, mt):
    """The hidden map never reaches memory: the DELTA epilogue checks it in registers.  Pins: 0.5 * 8188 = 4094.0 clean, + 2^-6 * 2^-6
    flagged, a NaN half in the hidden state flagged.  Coverage: hid[p, co] = 5000 at one (pixel, channel) at a time."""
    cls = pixel_classes(h, w)
    p, co = cls["interior"], 100
    pack, _ = delta_pack(dev, form, co, 8188.0, exact=True)
    delta_launch(dev, form, mt, h, w, pack, {(p, 5): 0.5})
    assert flag(dev) == 0, "4094.0 is not clamped and must not be reported"
    delta_launch(dev, form, mt, h, w, pack, {(p, 5): 0.5, (p, 6): 2.0 ** -6})
    assert flag(dev) == S.BIT_HIDDEN, "4094 + 2^-12 is clamped: bit 2"
    assert flag(dev) == 0
    delta_launch(dev, form, mt, h, w, pack, {}, nan_at=(p, 5))
    assert flag(dev) == S.BIT_HIDDEN, "a NaN half in the hidden state must be reported, not turned into 0 by the ReLU"
    fired = set()
    gain = 5000.0 / (0.9 * 64)
    for name, px in cls.items():
        for ch in (S.CH256 if name == "interior" else (0, 255)):
            pack, wt = delta_pack(dev, form, ch, gain)
            _, net_rb = delta_launch(dev, form, mt, h, w, pack, {(px, c): 0.9 for c in range(64)})
            key = ("delta_ref", h, w, px, ch)
            if key not in _PACKS:
                hid = torch.relu(conv_ref(net_rb, net_rb.abs(), wt, None, h, w)[0])
                hot = float(hid[px, ch])
                hid[px, ch] = 0.0
                _PACKS[key] = (hot, float(hid.max()))
            hot, rest = _PACKS[key]
            assert abs(hot - 5000.0) < 1.0 and rest < S.ACT_LIMIT / 4
            assert flag(dev) == S.BIT_HIDDEN, f"one hot hidden activation at the {name} pixel {px}, channel {ch}: no flag ({form}, {2 * mt}-row tiles)"
        fired.add(name)
    fired.add("channels256")
    RAN[("delta", form, 2 * mt)] = RAN.get(("delta", form, 2 * mt), set()) | fired


@pytest.mark.parametrize("form,mt", [(f, m) for f in FORMS for m in DELTA_MT])
def test_delta_head_clean_launch_is_silent(dev, form, mt):
    h, w = 37, 33
    base = torch.tanh(hashed((h * w, 64), 4410, -2.0, 2.0))
    pack, _ = delta_pack(dev, form, 0, 0.01)
    T, _ = delta_launch(dev, form, mt, h, w, pack, {}, base=base)
    assert flag(dev) == 0 and bool(torch.isfinite(T).all())


@pytest.mark.parametrize("form", list(FORMS))
def test_delta_head_sweep(dev, form):
    h, w = 37, 33
    p, co = pixel_classes(h, w)["interior"], 129
    base = torch.tanh(hashed((h * w, 64), 4411, -2.0, 2.0)) * 0.01
    for v in S.SWEEP:
        pack, wt = delta_pack(dev, form, co, v / (0.9 * 64))
        T, net_rb = delta_launch(dev, form, 0, h, w, pack, {(p, c): 0.9 for c in range(64)}, base=base)
        bits = flag(dev)
        assert bits in (0, S.BIT_HIDDEN)
        rep = None
        if not bits:
            w2 = _PACKS["proj"][1].double()
            hid, hmag = conv_ref(net_rb, net_rb.abs(), wt, None, h, w)
            hid = torch.relu(hid)
            proj = w2[0].reshape(2, 128, 9)
            ref = torch.cat([hid[:, hf * 128:(hf + 1) * 128] @ proj[hf] for hf in range(2)], 1)
            mag = torch.cat([hmag[:, hf * 128:(hf + 1) * 128] @ proj[hf].abs() for hf in range(2)], 1)
            got = T.cpu().double().permute(2, 0, 1).reshape(h * w, 18)
            rep = check_elementwise(got, ref, mag, C_CONV * FORMS[form][1], 2.0 ** (-24 - 4) * proj.abs().sum(1).reshape(1, 18),
                                    f"delta head {form}, planted {v}", h=h, w=w)
            assert rep.ok, f"planted {v}: no flag and not within parity of the unclamped reference\n{rep.message()}"
        assert bits or v <= S.ACT_SCAN_CLEAN, f"planted {v}: clamped without a flag"
        note_sweep("delta", form, rep)


# ================================================================================================ disparity writers (bit 8)
@pytest.mark.parametrize("h,w", [(9, 21), (37, 33)])
def test_disparity_writers_report_the_generators_limit(dev, h, w):
    """The s16 convs clamp 100 * (d[q] - d[p]) * 2^6 without a check of their own; cer_delta_sum_f32 and the delta prologue of the lookup
    bound |d| instead: 5.1175 clean, the next float, NaN and inf raise bit 8 - at the first, the last and an interior pixel, both signs -
    and the disparity's bytes are what they were."""
    from cer_mvs_amd import _lib as L, ops
    P = h * w
    T = torch.zeros(2, 9, P, device=dev)
    _, _, rs = ops.row_layout(64, 3, compact=True)
    vol = hashed((P, rs), 4501, -1.0, 1.0).to(dev)
    vol.level0_only = True
    origin = torch.full((P,), 0.00125, device=dev)
    w0t, b0 = hashed((33, 64), 4502, -0.02, 0.02).to(dev), hashed((64,), 4503, -0.1, 0.1).to(dev)
    base = torch.full((P,), 0.0013)

    def writers(p, v):
        d = base.clone()
        d[p] = float(v)
        out, _ = ops.delta_sum(T, 0.0, d.to(dev), h, w)
        bits = [flag(dev)]
        assert torch.equal(out.cpu().view(torch.int32), d.view(torch.int32))
        dd = d.to(dev)
        ops.lookup_encode(vol, origin, dd, w0t, b0, 64, 0.0025 / 64, 3, 5, out_split=2, log2s=L.S16_RELU, img_w=w, delta=(T, 0.0))
        bits.append(flag(dev))
        assert torch.equal(dd.cpu().view(torch.int32), d.view(torch.int32))
        return bits
    fired = set()
    for cls, p in (("first", 0), ("last", P - 1), ("interior", (h // 2) * w + w // 2)):
        for sign in (1.0, -1.0):
            assert writers(p, sign * S.DISP_CLEAN) == [0, 0]
            assert writers(p, sign * S.DISP_FLAG) == [S.BIT_DISP, S.BIT_DISP]
            assert [b & ~S.BIT_ACT for b in writers(p, sign * float("inf"))] == [S.BIT_DISP, S.BIT_DISP]     # (+inf: the lookup's own features are NaN too)
        assert writers(p, float("nan")) == [S.BIT_DISP, S.BIT_DISP]
        fired.add(cls)
    RAN[("disparity", "-", 0)] = RAN.get(("disparity", "-", 0), set()) | fired


@pytest.mark.parametrize("form", list(FORMS))
def test_generated_disparity_features_flag_or_parity(dev, form):
    """The site behind bit 8, itself: the z|r conv of the shipped weights at 9 x 21 with ONE disparity planted among values of 0.0013.
    At 10.2 every difference inside a window stays below the generators' clamp (10.235): z and r*h are within the full-size module's bound
    of the float64 reference.  At 10.3 the features clamp: the output stays finite and leaves that bound near the planted pixel - the
    clamp is real and silent in the conv, which is why the disparity's writers report |d| > 5.1175 (both values are far beyond it:
    test_disparity_writers_report_the_generators_limit)."""
    from cer_mvs_amd import _lib as L, ops, update
    h, w = 9, 21
    P, PP, U, R = h * w, ops.s16_pixels(h, w), L.S16_UNIT, L.S16_RELU
    ub = update_block(dev, form)
    loop, g = ub.loop(0, dev), update._stage_weights(ub, 0, "cpu")
    net_l = frag_poisoned_padding(torch.tanh(hashed((P, 64), 4701, -2.0, 2.0)).to(dev), h, w, U)
    c2_l = frag_poisoned_padding(torch.relu(hashed((P, 64), 4702, -1.0, 2.0)).to(dev), h, w, R)
    net_rb, c2_rb = unfrag(net_l, h, w, U), unfrag(c2_l, h, w, R)
    wt = g.wzr[:, g.rest].cpu()
    q = 4 * w + 10
    reps = {}
    for v in (10.2, 10.3):
        disp = torch.full((P,), 0.0013)
        disp[q] = v
        z, rn = poison_f32(torch.empty(PP, 64, device=dev)), poison_f16(torch.empty(PP, 64, device=dev))
        ops.conv3x3_s16(loop.zr, [net_l, disp.to(dev), c2_l], h, w, L.EPI_GATES, out=z, out2=rn, aux=net_l, log2s_out=U, log2s_aux=U)
        assert flag(dev) == 0                                          # (the conv has no check of its own: the census row says "writer")
        z_rb = ops.s16_layout(z, h, w, L.S16_F32X8, inverse=True).cpu().double()
        rh_rb = unfrag(rn, h, w, U)
        assert bool(torch.isfinite(z_rb).all()) and bool(torch.isfinite(rh_rb).all())
        feat, feat_mag = disp_feature_parts(disp.double(), h, w)
        assert float(feat.abs().max()) == pytest.approx(100 * (v - 0.0013), rel=1e-6)
        pre, mag = conv_ref(torch.cat([net_rb, feat, c2_rb], 1), torch.cat([net_rb.abs(), feat_mag, c2_rb.abs()], 1), wt, None, h, w)
        abs_t = 2.0 ** (-24 - R) * wsum(wt) + ACT_ABS
        c = C_CONV * FORMS[form][1]
        reps[v] = (check_elementwise(z_rb, torch.sigmoid(pre[:, :64]), mag[:, :64], c, abs_t[:, :64], f"z, planted {v}", h=h, w=w),
                   check_elementwise(rh_rb, torch.sigmoid(pre[:, 64:]) * net_rb, mag[:, 64:], c, abs_t[:, 64:], f"r*h, planted {v}", h=h, w=w))
    assert reps[10.2][0].ok and reps[10.2][1].ok, reps[10.2][0].message() + reps[10.2][1].message()
    assert not (reps[10.3][0].ok and reps[10.3][1].ok), "a difference of 10.3 is beyond 65504 / 2^6 / 100 = 10.235: the features clamp"
    note_sweep("disp_features", form, reps[10.2][0])
    RAN[("disp_features", form, 0)] = {"below", "beyond"}


# ================================================================================================ unreported: the f16x3 loop's split
def test_f16x3_conv_clamp_is_unreported(dev):
    """conv3x3(mode="f16x3") RELU with ``out_split`` at 9 x 21 (cer_split8, clamp at the f16 maximum in the tensor's own units, 16 x beyond
    the s16 path): 60000 within parity, 1e5 comes back as exactly 65504 - finite, NO flag.  The remedy the saturation error names is
    wider, not unlimited."""
    from cer_mvs_amd import _lib as L, ops
    h, w = 9, 21
    p, co = 4 * w + 10, 33
    x = torch.relu(hashed((h * w, 64), 4601, -1.0, 2.0))
    x[p] = 0.0
    x[p, co] = 1000.0
    for v, exact in ((60000.0, False), (1.0e5, True)):
        wt = hashed((64, 64, 3, 3), 4602, -0.02, 0.02)
        wt[co, co, 1, 1] = v / 1000.0
        pc = ops.PackedConv3x3(wt, torch.zeros(64), [(64, 0)], dev)
        out = poison_f16(torch.empty(h * w, 64, device=dev))
        ops.conv3x3(pc, [ops.split32(x.to(dev))], h, w, L.EPI_RELU, mode="f16x3", out=out, kinds=[3], out_split=True)
        got = ops.split32(out, inverse=True).cpu().double()
        assert flag(dev) == 0 and bool(torch.isfinite(got).all())
        if exact:
            assert float(got[p, co]) == S.F16_MAX
        else:
            xr = ops.split32(ops.split32(x.to(dev)), inverse=True).cpu().double()
            ref, mag = conv_ref(xr, xr.abs(), wt, None, h, w)
            rep = check_elementwise(got, torch.relu(ref), mag, C_CONV, 2.0 ** -24 * (wsum(wt) + 1), "f16x3 conv, planted 60000", h=h, w=w)
            assert rep.ok, rep.message()


# ================================================================================================ protocol level: any iteration counts
SCALE_UP = 64.0


@pytest.mark.parametrize("form", ["s16", "s16f8", "s16f6"])
def test_any_iteration_counts(dev, monkeypatch, form):
    """``UpdateBlock.run`` with T = 3 at 9 x 21: the volume's contents are scaled by 64 for exactly one iteration k and restored.  The corr2
    conv has a gain (output channel 3 sums its whole 3 x 3 x 64 window) chosen from the float64 reference so that c1 stays below 4093 and
    c2 goes beyond 4094 when and only when the volume is scaled.  Bit 4 must be set after ``run`` for every k, on the wrappers (protocol A,
    ``after=``) and on the fused, plan-replaying production protocol (C): a check of what the LAST iteration left is not enough."""
    import test_update_run_gpu as UR
    from cer_mvs_amd import _lib as L, ops, update
    h, w, stage, T = 9, 21, 0, 3
    S0 = UR.setup(dev, form, h, w)
    st = S0.stages[stage]
    g = update._stage_weights(S0.ub, stage, "cpu")
    w0t, b0 = g.w0t.double(), g.b0.double()

    def c1_ref(scale, disp):
        return lookup_ref(st.vol.cpu().double() * scale, st.origin.cpu().double(), disp.cpu().double(), w0t, b0, st.D, st.incre)[0]
    window = lambda c1: torch.nn.functional.avg_pool2d(c1.t().reshape(1, 64, h, w), 3, 1, 1, divisor_override=1).sum(1).max()
    gain = 8000.0 / float(window(c1_ref(SCALE_UP, st.disp0)))
    ub = copy.deepcopy(S0.ub)
    with torch.no_grad():
        ub.corr_encoder[2].weight[3] = gain
        ub.corr_encoder[2].bias[3] = 0.0
    ub.refresh_weights()
    hot = SimpleNamespace(**{**vars(S0), "ub": ub, "hoisted": ub.hoist_all(S0.inp, h, w, 2), "ws": ub.workspace(h, w, dev)})
    assert flag(dev) == 0
    wt, bias = ub.corr_encoder[2].weight.detach().cpu(), ub.corr_encoder[2].bias.detach().cpu()

    # the unscaled run is clean (c2 beyond 4094 ONLY when the test wants it), and gives the disparity each iteration starts from
    disps = [st.disp0.clone()]
    UR.run_protocol(monkeypatch, hot, "A", stage, T, observe=lambda i, net_l, disp: disps.append(disp.clone()))
    assert flag(dev) == 0 and len(disps) == T + 1
    for k in range(T):
        c1 = c1_ref(SCALE_UP, disps[k])
        c2 = torch.relu(conv_ref(c1, c1.abs(), wt, bias, h, w)[0])
        c2_plain = torch.relu(conv_ref(c1_ref(1.0, disps[k]), c1.abs(), wt, bias, h, w)[0])
        assert float(c1.max()) < S.ACT_SCAN_CLEAN and float(c2.max()) > 1.2 * S.ACT_LIMIT and float(c2_plain.max()) < S.ACT_LIMIT / 4, \
            (k, float(c1.max()), float(c2.max()), float(c2_plain.max()))

    def scaled(k):
        """Patches that scale the volume around call number k of (step | replay): the fused protocol's iterations."""
        n = {"i": 0}

        def around(fn):
            def call(*a, **kw):
                i = n["i"]
                n["i"] += 1
                if i == k:
                    st.vol.mul_(SCALE_UP)
                try:
                    return fn(*a, **kw)
                finally:
                    if i == k:
                        st.vol.div_(SCALE_UP)
            return call
        return around
    vol0 = st.vol.clone()
    try:
        for k in range(T):
            # protocol A: scale through after=
            def observe(i, net_l, disp, k=k):
                if i == k - 1:
                    st.vol.mul_(SCALE_UP)
                if i == k:
                    st.vol.div_(SCALE_UP)
            if k == 0:
                st.vol.mul_(SCALE_UP)
            UR.run_protocol(monkeypatch, hot, "A", stage, T, observe=observe)
            bits = flag(dev)
            assert torch.equal(st.vol, vol0)
            assert bits & S.BIT_ACT, f"{form}, wrappers: c2 beyond 4094 in iteration {k} of {T} only - flag {bits}"
            # protocol C: fused delta + replayed plan, scaled through a counting wrapper around _S16Loop.step and LaunchPlan.replay
            with monkeypatch.context() as m:
                around = scaled(k)
                m.setattr(update._S16Loop, "step", around(update._S16Loop.step))
                m.setattr(L.LaunchPlan, "replay", around(L.LaunchPlan.replay))
                r = UR.run_protocol(monkeypatch, hot, "C", stage, T)
            bits = flag(dev)
            assert r.replays == 1 and torch.equal(st.vol, vol0)
            assert bits & S.BIT_ACT, f"{form}, fused + replayed: c2 beyond 4094 in iteration {k} of {T} only - flag {bits}"
    finally:
        st.vol.copy_(vol0)
    RAN[("run_any_iteration", form, 0)] = {"k0", "k1", "k2"}


# ================================================================================================ protocol level: any stage, both paths
def _stage0_hot_model(dev, policy):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    from cer_mvs_amd.update import UpdateBlock
    model = RAFT(cascade=[(64, 64, 3), (-1, 320, 3)], test_mode=True, gru_precision="s16f8")
    model.update_block = UpdateBlock(cascade=model.cascade, dim_net=64, dim_inp=64, share_corr=False)
    model.update_block.corr_fp8 = True
    sd = fill_state_dict(model.state_dict(), seed=5)
    sd["update_block.corr_encoder0.2.bias"][3] = 5000.0          # c2 channel 3 of STAGE 0 beyond 4094 in every iteration; stage 1 is clean
    model.load_state_dict(sd)
    model.overflow_policy = policy
    return model.to(dev).eval()


def test_any_stage_counts_on_both_paths(dev):
    """A saturation in stage 0 only (its own corr encoder, share_corr=False) at 100 x 132: RAFT.forward and slab.sharded_forward over two
    simulated ranks must both leave bit 4 - the stage-1 iterations overwrite stage 0's c2."""
    from cer_mvs_amd import slab
    from cer_mvs_amd.synthetic import synthetic_scene
    images, poses, intr, scale = synthetic_scene(100, 132, 2, seed=23)
    images, poses, intr = images.to(dev), poses.to(dev), intr.to(dev)
    model = _stage0_hot_model(dev, "ignore")
    assert model.update_block.loop(0, dev) is not model.update_block.loop(1, dev)
    with torch.no_grad():
        model(images, poses, intr, scale=scale)
        bits = flag(dev)
        assert bits & S.BIT_ACT, f"RAFT.forward: stage 0 saturated, flag {bits}"
        slab.sharded_forward(model, images, poses, intr, scale, slab.LocalExchange(2))
        bits = flag(dev)
        assert bits & S.BIT_ACT, f"slab.sharded_forward: stage 0 saturated, flag {bits}"
    RAN[("any_stage", "s16f8", 0)] = {"forward", "sharded"}


def test_any_stage_control_only_stage_0_saturates(dev, monkeypatch):
    """The control of the test above: the same two forwards with the flag read (and cleared) behind every step, plans off so that every
    iteration is a step.  Every stage-0 step raises bit 4 and nothing else; every stage-1 step leaves the flag at 0 - c1 (checked exactly by
    the lookup in every iteration), stage 1's c2 and the hidden maps are clean, so what the test above sees is stage 0's c2.  The same
    model without the hot bias is clean throughout."""
    from cer_mvs_amd import ops, slab, update
    from cer_mvs_amd.synthetic import synthetic_scene
    images, poses, intr, scale = synthetic_scene(100, 132, 2, seed=23)
    images, poses, intr = images.to(dev), poses.to(dev), intr.to(dev)
    model = _stage0_hot_model(dev, "ignore")
    loops, seen = [], {0: [], 1: []}
    plain = update._S16Loop.step

    def step(self, *a, **kw):
        plain(self, *a, **kw)
        if not any(self is lp for lp in loops):
            loops.append(self)                                         # (a forward runs its stages in order: the first loop seen is stage 0's)
        seen[[self is lp for lp in loops].index(True)].append(ops.check_overflow(dev))
    monkeypatch.setattr(update, "USE_PLANS", False)
    monkeypatch.setattr(update._S16Loop, "step", step)
    with torch.no_grad():
        for run in (lambda: model(images, poses, intr, scale=scale), lambda: slab.sharded_forward(model, images, poses, intr, scale, slab.LocalExchange(2))):
            seen[0].clear(), seen[1].clear(), loops.clear()
            run()
            assert len(loops) == 2 and len(seen[0]) >= 3 and len(seen[1]) >= 3
            assert all(b == S.BIT_ACT for b in seen[0]), seen
            assert all(b == 0 for b in seen[1]), seen
            assert flag(dev) == 0
        with torch.no_grad():
            model.update_block.corr_encoder0[2].bias[3] = 0.0
        model.update_block.refresh_weights()
        seen[0].clear(), seen[1].clear(), loops.clear()
        model(images, poses, intr, scale=scale)
        assert flag(dev) == 0 and len(seen[0]) >= 3 and all(b == 0 for b in seen[0] + seen[1])


def test_pipeline_checked_never_yields_a_saturated_result(dev):
    """``pipeline.checked`` over a real DepthMapPipeline of 3 streams and 5 entries under the default "lazy" policy.  Entries go to the
    replicas round robin, so the third runs on replica 2, whose corr encoder has the hot bias: its forward, and only its, saturates.
    ``checked`` must raise SaturationError and must not yield entries 3 - 5.  Entries 1 and 2 may already have been yielded - when their
    results were taken, entry 3 need not have finished, and nothing of theirs saturated - and nothing else: the yielded list is a prefix
    of [1, 2]."""
    import test_hip_parity as HP
    from cer_mvs_amd import pipeline
    from cer_mvs_amd.raft import SaturationError

    def hot(sd):
        sd["update_block.corr_encoder.0.bias"][0] = 5000.0
    core = HP._form_model(dev, "s16", HP._form_weights())
    pipe = pipeline.DepthMapPipeline(core, streams=3)
    pipe.models[2].load_state_dict(HP._form_weights(hot))
    scene = HP._form_scene(dev)
    assert len(pipe) == 3 and all(m.overflow_policy == "lazy" for m in pipe.models)
    yielded = []
    try:
        with pytest.raises(SaturationError, match="beyond 4094"):
            for (k, _), out in pipeline.checked(pipe, core, ((k, pipe.submit(*scene[:3], scene[3])) for k in range(1, 6)), lambda e: pipe.result(e[1])):
                assert bool(torch.isfinite(out).all())
                yielded.append(k)
        assert yielded in ([], [1], [1, 2]), f"yielded {yielded}: entry 3 saturated, and a result from 3 on was handed out before its flag was read"
    finally:
        pipe.synchronize()
        pipe.close()
    RAN[("pipeline_checked", "s16", 0)] = {"raised"}


# ================================================================================================ protocol level: the policies on real forwards
def test_policies_on_a_real_forward(dev):
    """One hot corr-encoder bias (c1 channel 0 at 5000, as test_overflow_fallback_repeats_the_forward_in_f16x3): "raise" raises from the
    forward itself and leaves the flag clear; "lazy" returns, the NEXT forward raises, the one after runs; "ignore" leaves the bits."""
    import test_hip_parity as HP
    from cer_mvs_amd import ops
    from cer_mvs_amd.raft import SaturationError

    def hot(sd):
        sd["update_block.corr_encoder.0.bias"][0] = 5000.0
    hot_model, clean = HP._form_model(dev, "s16", HP._form_weights(hot)), HP._form_model(dev, "s16", HP._form_weights())
    scene = HP._form_scene(dev)
    run = lambda m: m(*scene[:3], scale=scene[3])
    with torch.no_grad():
        assert hot_model.overflow_policy == "lazy" and clean.overflow_policy == "lazy"      # the default
        hot_model.overflow_policy = "raise"
        with pytest.raises(SaturationError, match="beyond 4094"):
            run(hot_model)
        assert flag(dev) == 0
        hot_model.overflow_policy = "lazy"
        out = run(hot_model)                                       # returns: nothing has been read yet
        assert bool(torch.isfinite(out).all())
        torch.cuda.synchronize()                                   # (the snapshot has landed)
        with pytest.raises(SaturationError, match="beyond 4094"):
            run(clean)                                             # the NEXT forward raises, whichever model runs it
        out = run(clean)                                           # the one after that runs clean
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and ops.overflow_poll(dev) == 0 and flag(dev) == 0
        hot_model.overflow_policy = "ignore"
        run(hot_model)
        run(hot_model)
        assert flag(dev) & S.BIT_ACT


def test_policies_on_the_sharded_forward(dev):
    from cer_mvs_amd import slab
    from cer_mvs_amd.raft import SaturationError
    from cer_mvs_amd.synthetic import synthetic_scene
    images, poses, intr, scale = synthetic_scene(100, 132, 2, seed=23)
    images, poses, intr = images.to(dev), poses.to(dev), intr.to(dev)
    model = _stage0_hot_model(dev, "raise")
    with torch.no_grad():
        with pytest.raises(SaturationError, match="beyond 4094"):
            slab.sharded_forward(model, images, poses, intr, scale, slab.LocalExchange(2))      # (through LocalExchange.max_int)
        assert flag(dev) == 0
        model.overflow_policy = "fallback"
        with pytest.raises(NotImplementedError):
            slab.sharded_forward(model, images, poses, intr, scale, slab.LocalExchange(2))
        assert flag(dev) == 0                                      # refused up front: nothing ran


# ================================================================================================ what ran
def test_census_of_what_ran():
    """Every in-kernel reporter of the census fired at every position class of its site, in every arithmetic form and with every tile
    height the family exists for; counts only cases that passed, so it needs the whole module (it runs last)."""
    want = {("feat_split", "-", 0): {"first", "last", "block_seam", "sign", "channels"}, ("fsplit_head", "-", 0): {"bias_channel", "input_pixel"},
            ("lookup", "-", 0): set(S.PIXEL_CLASSES) | {"channels64", "tile_seam"}, ("disparity", "-", 0): {"first", "last", "interior"}}
    for form in FORMS:
        for mt in CORR2_MT[form]:
            want[("corr2", form, 4 * mt)] = set(S.PIXEL_CLASSES) | {"channels64"}
        for mt in DELTA_MT:
            want[("delta", form, 2 * mt)] = set(S.PIXEL_CLASSES) | {"channels256"}
    for form in ("s16", "s16f8", "s16f6"):
        want[("run_any_iteration", form, 0)] = {"k0", "k1", "k2"}
    want[("any_stage", "s16f8", 0)] = {"forward", "sharded"}
    want[("pipeline_checked", "s16", 0)] = {"raised"}
    for form in FORMS:
        want[("disp_features", form, 0)] = {"below", "beyond"}
    missing = {k: sorted(v - RAN.get(k, set())) for k, v in want.items() if v - RAN.get(k, set())}
    assert not missing, f"reporters that did not fire (or whose case did not pass): {missing}"
    sites = {r["site"] for r in S.KERNEL_REPORTERS}
    assert len(sites) == 5                                           # feat_split, FSPLIT head, lookup, RELU epilogue, DELTA epilogue
    for site in ("lookup", "corr2", "delta"):
        forms = ["-"] if site == "lookup" else list(FORMS)
        assert all(SWEPT.get((site, f), [0])[0] == len(S.SWEEP) for f in forms), (site, SWEPT)
    assert all(v[1] <= 1.0 for v in SWEPT.values())
    TIMES["census"] = 0.0
