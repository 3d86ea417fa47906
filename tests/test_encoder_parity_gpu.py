"""Element-wise parity of the encoder kernels, ONE LAUNCH AT A TIME (run on the GPU box: pytest -m gpu).

The encoders were compared only as wholes (rel_l1 < 1e-5 against the oracle: a global mean that one wrong 2 x 32 tile, a wrong last row or
two swapped statistics records pass - tests/test_parity_check_cpu.py shows it), at sizes where a persistent block of csrc/enc_pc.hip owns
one tile, and never on the tiled engine's trunk (csrc/enc_conv.hip).  Here every launch kind runs alone: cer_enc_pc_conv in all seven
instantiations x every producer form ``HipEncoder._trunk_pc`` / ``_head`` issue (enumerated by tracing them: the module asserts that the set
it tests is the set the trace shows) x both norm kinds, cer_enc_conv_f16x3 (RAW with partials - the streaming 32 -> 32 kernel included - and
its FMAP / CTX heads), cer_enc_merge_f32 and cer_enc_stats_reduce_f32.  EVERY output element is compared with a float64 reference of that one
launch, computed from the tensors the kernel was given (tests/parity_check.py: enc_input_ref64, enc_conv_ref64, enc_head_ref64); a failure
names the image and the tile or row.

Shapes - the smallest at which each path exists (the CU count is read from the device, the tile-count preconditions are asserted):
  * "multi": more than 2 x CUs tiles, so that a persistent block walks several tiles (LDS buffer parity across tile changes, the
    double-buffered statistics patch, finalize(u - 1) behind the next barrier, prepare() past the last unit, interior units next to border
    units) in the XCD column order (grid = CUs, a multiple of 8): 19 x 134 inputs (10 x 67 for the heads), 40 .. 90 images; every geometry
    has interior units, border units and partial last tiles in both directions (the 2-row tiles of the stride-2 3 x 3: along x);
  * "few": fewer tiles than CUs and a grid that is no multiple of 8 (plain order): 18 x 133 (odd width: the even / odd column planes of
    the stride-2 halo), 9 x 67 for the heads, 3 images;
  * "tiny" 3 x 5 (smaller than a tile and than the halo: everything is clamped) and "row" 1 x 40 (a single row).

Sentinel coverage: ``out``, ``out2``, ``merged_out`` and the partial records are NaN before every launch (f16 NaN for the split planes); a
bordered output's border holds a fixed finite pattern that must come back bit for bit; afterwards ``assert_covered_batch`` with the
launch's own tile (8 x 32; 2 x 32 for the stride-2 3 x 3 - on the tiled engine for the stride-2 1 x 1 too; 4 x 32 for the 128-channel head).

Bounds (none is fitted to a kernel's output):
  * three-term convolution: |err| <= 2e-6 * mag + 4 * 2^-24 * mag_form, mag = conv(|x|, |w|) + |b|, mag_form = conv(mag_in, |w|), mag_in =
    (|A| + |mean_A|) * rstd_A [+ the same of B].  2e-6 is the constant of test_stem_on_matrix_cores for this arithmetic; the second term is
    the fp32 forming of the input - a subtraction, a product, the sum of the two terms, at most four roundings - carried through |w|.
    Heads: FMAP scales both sides by ``scale`` (a power of two); CTX adds ACT_ABS = 2^-20 for tanhf (tanh and relu are 1-Lipschitz), the
    constant of tests/test_fullsize_parity_gpu.py; FSPLIT is compared BIT FOR BIT with ops.feat_split of the FMAP output of the same
    launch configuration (the idiom of test_encoder_head_writes_split_planes_directly).
  * merged_out and cer_enc_merge_f32: |err| <= 4 * 2^-24 * mag_in.
  * statistics partial records: (sum, sum of squares) of a tile against the float64 sums of the kernel's OWN output over that tile's pixels:
    K * 2^-24 * sum|o| and K * 2^-24 * sum o^2 with K = 67, the longest chain of fp32 additions a record passes through, read from the
    kernels: a lane adds its own pixels one by one (csrc/enc_pc.hip consumer epilogue: RPW rows x 16 accumulator registers, RPW = TH / WM <= 4
    -> 64; the squares by fmaf, one rounding per step), one addition joins the two half-waves (__shfl_xor 32), and ``finalize`` adds the WM
    row groups (2 where RPW = 4; the 32 -> 32 kernel: 32 + 1 + 4 = 37).  csrc/enc_conv.hip: 16 + 1 + 8 = 25 (tiled), 2 x 16 + 1 + 4 = 37
    (streaming).  Every record of every tile must be finite (they are NaN before the launch).
  * cer_enc_stats_reduce_f32 accumulates in fp64: against a float64 reduction of the same records mean and rstd agree to 2^-23 relative
    (the fp32 rounding of the result, 2^-24, and as much again for the order of the fp64 sums); |mean| is floored at 2^-24 * sqrt(Q / n).
  * rstd of a badly conditioned channel (conv + reduce against the float64 rstd of the float64 convolution): var = Q / n - mean^2 is formed
    from records that carry K roundings each, relative to Q / n = sigma^2 + mean^2: d var / var <= K 2^-24 (1 + mean^2 / sigma^2), and
    d rstd / rstd = d var / (2 var); + 2^-23 for the reduce; + the convolution's own bound: moving every output by at most e moves sigma by at
    most e, so its share is max_pixels(2e-6 mag + 4 * 2^-24 mag_form) / sigma.
  * FP6-correction form (flags & 8): no per-element constant is known.  The yardstick is the CPU emulation the form was costed with
    (tools/experiments/encoder_corr_numerics.py, ``conv_emul`` in its "fp6blk" mode, imported) on the same input and weights, against the same
    float64 reference, normalised by mag: the kernel's maximum and 99.9th percentile of |err| / mag may be at most 2 x the emulation's (the
    factor covers the different accumulation order and nothing else).  The output must differ from the three-term output (the flag took
    effect) and reproduce bit for bit on a second launch.
  * csrc/enc_pc.hip claims the arithmetic of csrc/enc_conv.hip "bit for bit": for every RAW case in the three-term form cer_enc_conv_f16x3 on
    the same input (single forms: the same tensor, statistics and ReLU; two-tensor forms: the input formed on the host in fp32 with the
    kernel's own operation order) must give identical bits.

Measured figures go to profiles/encoder_parity.json, only under CER_PARITY_RECORD=1 (a plain run writes nothing)."""
import functools
import json
import math
import os
import sys
import time

import pytest
import torch

from conftest import REPO, rel_l1
from parity_check import (ENC_TILE, U24, assert_covered_batch, assert_stats_records, check_batch, enc_chain_ref64, enc_conv_ref64, enc_conv_tile,
                          enc_head_ref64, enc_input_ref64, enc_pc_tile, instance_stats64)
from test_oracle_golden import blank_state_dict, hashed

pytestmark = pytest.mark.gpu

C3 = 2e-6                    # three f16 terms per product: tests/test_hip_parity.py::test_stem_on_matrix_cores
C_FORM = 4 * U24             # forming the virtual input in fp32: at most four roundings
ACT_ABS = 2.0 ** -20         # tanhf: tests/test_fullsize_parity_gpu.py
K_STATS = 67                 # longest chain of fp32 additions behind a statistics record (module docstring)
RECORD = {}

# instantiation -> (layer of fill_state_dict, Cin, Cout, taps, stride, epilogue of cer_enc_pc_conv)
INST = {"c32": ("fnet.layer1.0.conv1", 32, 32, 9, 1, 0), "c32_64s2": ("fnet.layer2.0.conv1", 32, 64, 9, 2, 0),
        "d32_64s2": ("fnet.layer2.0.downsample.0", 32, 64, 1, 2, 0), "c64": ("fnet.layer2.1.conv1", 64, 64, 9, 1, 0),
        "fmap": ("fnet.conv2", 64, 64, 1, 1, 1), "fsplit": ("fnet.conv2", 64, 64, 1, 1, 3), "ctx": ("cnet.conv2", 64, 128, 1, 1, 2)}
RAW = ("c32", "c32_64s2", "d32_64s2", "c64")
HEADS = ("fmap", "fsplit", "ctx")
# producer forms: (flags & 7, statistics of A, second tensor, statistics of B, merged_out).  flags: 1 ReLU on A, 2 ReLU on B, 4 on the sum.
_T, _F = True, False
SINGLE, DUAL_MERGED, DUAL_NORMB_MERGED, DUAL_PLAIN = (1, _T, _F, _F, _F), (7, _T, _T, _T, _T), (5, _T, _T, _T, _T), (5, _T, _T, _F, _F)


def _none(form):
    """The same launch as the norm kind "none" issues it: no statistics tensor."""
    return (form[0], _F, form[2], _F, form[4])


FORMS = {"instance": {"c32": {SINGLE, DUAL_MERGED}, "c32_64s2": {DUAL_PLAIN}, "d32_64s2": {DUAL_PLAIN}, "c64": {SINGLE, DUAL_NORMB_MERGED},
                      "fmap": {DUAL_PLAIN}, "fsplit": {DUAL_PLAIN}, "ctx": {DUAL_PLAIN}}}
FORMS["none"] = {k: {_none(f) for f in v} for k, v in FORMS["instance"].items()}
GEOMS = ("multi", "few", "tiny", "row")


def form_name(form):
    fl, sa, dual, sb, merged = form
    return (f"dual{fl}" if dual else f"single{fl}") + ("_sA" if sa else "") + ("_sB" if sb else ("_plainB" if dual and not fl & 2 else "")) + \
        ("_merged" if merged else "")


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
    assert not ops.check_overflow(dev)
    target = os.environ.get("CER_PARITY_RECORD", "")
    if target:
        path = os.path.join(REPO, "profiles", "encoder_parity.json") if target == "1" else target
        RECORD["module_wall_s"] = round(time.time() - t0, 1)
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


def ncus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@functools.lru_cache(maxsize=None)
def weights():
    from cer_mvs_amd.synthetic import fill_state_dict
    return fill_state_dict(blank_state_dict(), seed=5)


_CONVS = {}


def packed_conv(dev, inst, bias=None):
    """``encoder_hip._Conv`` (packed three-term and FP6 weights, bias) of the layer behind ``inst``, + its fp32 weight and bias."""
    from cer_mvs_amd.encoder_hip import _Conv
    layer, cin, cout, taps, stride, _ = INST[inst]
    key = (layer, bias is None)
    if key not in _CONVS or bias is not None:
        k = 3 if taps == 9 else 1
        m = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2)
        with torch.no_grad():
            m.weight.copy_(weights()[layer + ".weight"])
            m.bias.copy_(weights()[layer + ".bias"] if bias is None else bias)
        c = (_Conv(m, dev), m.weight.detach().clone(), m.bias.detach().clone())
        if bias is not None:
            return c
        _CONVS[key] = c
    return _CONVS[key]


def out_size(h, w, taps, stride):
    pad, ks = (1, 3) if taps == 9 else (0, 1)
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def geometry(dev, inst, geom):
    """-> (N, h, w) of the input; asserts what the geometry is for."""
    from cer_mvs_amd import _lib as L
    _, _, cout, taps, stride, epi = INST[inst]
    head = epi != 0
    if geom == "multi":
        h, w = (10, 67) if head else (19, 134)
        N = {"d32_64s2": 90, "fmap": 90, "fsplit": 90, "ctx": 60}.get(inst, 40)
    elif geom == "few":
        h, w = (9, 67) if head else (18, 133)
        N = 3
    else:
        (h, w), N = ((3, 5) if geom == "tiny" else (1, 40)), 2
    ho, wo = out_size(h, w, taps, stride)
    per = L.load().cer_enc_pc_tiles(ho, wo, cout, taps, stride)
    th, tw = enc_pc_tile(cout, taps, stride)
    assert per == ((ho + th - 1) // th) * ((wo + tw - 1) // tw)
    cus = ncus(dev)
    if geom == "multi":
        assert per * N > 2 * cus and cus % 8 == 0, (inst, per * N, cus)        # several tiles per block, XCD order
        assert wo % tw and wo > tw and ho > th and (ho % th or th == 2)         # partial last tiles (the 2-row tiles: along x), more than one tile
    elif geom == "few":
        while per * N % 8 == 0:
            N += 1
        assert per * N < cus and per * N % 8, (inst, per * N, cus)             # one tile per block, plain order
    else:
        assert per <= 2
    return N, h, w


def make_inputs(dev, form, N, h, w, C, seed):
    """Hashed tensors of the producer form -> device (A, sA, B, sB): statistics are the instance-norm statistics of the tensor, computed on
    the host and rounded to fp32 - the reference uses the very tensor the kernel gets."""
    fl, sa, dual, sb, _ = form
    stats = lambda t: instance_stats64(t.double().view(N, h, w, C)).float().contiguous().to(dev)
    A = hashed((N, h * w, C), seed, -1.0, 2.0)
    A += 0.5 * hashed((C,), seed + 1)                      # (per-channel offsets: the means differ)
    B = sB = None
    if dual:
        B = hashed((N, h * w, C), seed + 2, -1.5, 1.5) + 0.3 * hashed((C,), seed + 3)
        if not sb and not fl & 2:
            B = torch.relu(B)                              # a merged activation enters as it is
        sB = stats(B) if sb else None
        B = B.to(dev)
    return A.to(dev), (stats(A) if sa else None), B, sB


def reference_input(A, sA, B, sB, form, N, h, w):
    fl = form[0]
    x, mag_in = enc_input_ref64(A, sA, bool(fl & 1), B, sB, bool(fl & 2), relu_sum=bool(fl & 4) and B is not None)
    return x.view(N, h, w, -1), mag_in.view(N, h, w, -1)


def host_input_fp32(A, sA, B, sB, form):
    """The virtual input in fp32 with the kernel's own operation order (csrc/enc_pc.hip ``commit_items``; the kernel works on 2048 x the
    values: exact) - the materialised input of the bit-for-bit comparison."""
    fl = form[0]

    def term(X, s, relu):
        x = X.cpu()
        if s is not None:
            st = s.cpu().view(x.shape[0], 1, x.shape[2], 2)
            x = (x - st[..., 0]) * st[..., 1]
        return torch.relu(x) if relu else x
    y = term(A, sA, fl & 1)
    if B is not None:
        y = y + term(B, sB, fl & 2)
        if fl & 4:
            y = torch.relu(y)
    return y.clamp(-65504.0, 65504.0).contiguous()


def pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, epi, f6=False, out=None, out2=None, border=0, scale=1.0, want_part=False, flag=None):
    """One cer_enc_pc_conv launch with NaN in every output it owns -> (out, out2, part, merged_out)."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    ho, wo = out_size(h, w, conv.taps, conv.stride)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    part = None
    if epi == 0:
        out = nan(N, ho * wo, conv.cout)
        if want_part:
            part = nan(N, lib.cer_enc_pc_tiles(ho, wo, conv.cout, conv.taps, conv.stride), conv.cout, 2)
    m = nan(N, h * w, conv.cin) if form[4] else None
    flags = form[0] | (8 if f6 else 0)
    assert bool(flags & 4) == (B is not None)
    o2 = L.dev_ptr(flag, "flag", torch.int32) if epi == 3 else L.dev_ptr(out2, "out2")
    L.check(lib.cer_enc_pc_conv(L.dev_ptr(A, "srcA"), L.dev_ptr(sA, "statsA"), L.dev_ptr(B, "srcB"), L.dev_ptr(sB, "statsB"), flags, L.dev_ptr(m, "merged"),
                                L.dev_ptr(conv.packed_f6 if f6 else conv.packed, "w", torch.float16), L.dev_ptr(conv.bias, "bias"),
                                L.dev_ptr(out, "out", torch.float16 if epi == 3 else torch.float32), o2, L.dev_ptr(part, "part"), N, h, w, conv.cin,
                                conv.cout, conv.taps, conv.stride, epi, border, float(scale), L.cur_stream()), "enc_pc_conv")
    return out, out2, part, m


def tiled_conv(dev, conv, x, tf, relu, N, h, w, epi=0, out=None, out2=None, border=0, scale=1.0, want_part=False):
    """One cer_enc_conv_f16x3 launch, outputs NaN before it -> (out, out2, part)."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    ho, wo = out_size(h, w, conv.taps, conv.stride)
    part = None
    if epi == 0:
        out = torch.full((N, ho * wo, conv.cout), float("nan"), device=dev)
        if want_part:
            part = torch.full((N, lib.cer_enc_conv_tiles(ho, wo, conv.stride, conv.taps, conv.cout), conv.cout, 2), float("nan"), device=dev)
    L.check(lib.cer_enc_conv_f16x3(L.dev_ptr(x, "src"), L.dev_ptr(tf, "tf"), int(relu), L.dev_ptr(conv.packed, "w", torch.float16), L.dev_ptr(conv.bias, "bias"),
                                   L.dev_ptr(out, "out"), L.dev_ptr(out2, "out2"), L.dev_ptr(part, "part"), N, h, w, conv.cin, conv.cout, conv.taps,
                                   conv.stride, epi, border, float(scale), L.cur_stream()), "enc_conv")
    return out, out2, part


def stats_reduce(dev, part, pixels):
    from cer_mvs_amd import _lib as L
    N, nblk, C, _ = part.shape
    st = torch.full((N * C, 2), float("nan"), device=dev)
    L.check(L.load().cer_enc_stats_reduce_f32(L.dev_ptr(part, "part"), L.dev_ptr(st, "stats"), N, nblk, C, pixels, 1e-5, L.cur_stream()), "enc_stats_reduce")
    return st


def record(key, figs):
    RECORD.setdefault("kernels", {})[key] = {k: figs[k] for k in ("max_rel", "p999_rel", "max_ratio")}
    print(f"  {key:58s} max |err|/mag {figs['max_rel']:.3e}  p99.9 {figs['p999_rel']:.3e}  max |err|/bound {figs['max_ratio']:.3f}")


def emulate_fp6(x64, wt, b, taps, stride):
    """``conv_emul`` of tools/experiments/encoder_corr_numerics.py in its FP6 mode ("fp6blk": e2m3 correction terms, one power-of-two scale
    per pixel / output channel and 16-channel block) on the fp32 input -> [N, ho, wo, Cout] float64."""
    exp_dir = os.path.join(REPO, "tools", "experiments")
    if exp_dir not in sys.path:
        sys.path.insert(0, exp_dir)
    import encoder_corr_numerics as E
    prev, E.MODE = E.MODE, "fp6blk"
    try:
        y = E.conv_emul(x64.float().permute(0, 3, 1, 2).contiguous(), wt, b, stride=stride, padding=1 if taps == 9 else 0)
    finally:
        E.MODE = prev
    return y.double().permute(0, 2, 3, 1)


def rel_figures(got, ref, mag):
    r = ((got.double() - ref).abs() / mag.clamp_min(1e-300)).reshape(-1)
    assert bool(torch.isfinite(r).all())
    k = max(1, int(math.ceil(0.999 * r.numel())))
    return float(r.max()), float(torch.kthvalue(r, k).values)


def assert_fp6_within_emulation(key, got6, emu, ref, mag, got3):
    """The FP6 form against its yardstick: max and p99.9 of |err| / mag at most 2 x the emulation's; different from the three-term output."""
    km, kp = rel_figures(got6, ref, mag)
    em, ep = rel_figures(emu, ref, mag)
    RECORD.setdefault("fp6", {})[key] = {"kernel_max_rel": km, "kernel_p999_rel": kp, "emulation_max_rel": em, "emulation_p999_rel": ep,
                                         "three_term_max_rel": rel_figures(got3, ref, mag)[0]}
    print(f"  {key:58s} FP6 |err|/mag: kernel max {km:.3e} p99.9 {kp:.3e};  emulation max {em:.3e} p99.9 {ep:.3e}")
    assert em > 0 and km <= 2 * em and kp <= 2 * ep, (key, km, em, kp, ep)
    assert not torch.equal(got6, got3), f"{key}: the FP6 form returned the three-term bits (flags & 8 did nothing)"


# ------------------------------------------------------------------------------------------------ the forms, traced
def test_tested_forms_are_the_forms_the_encoder_issues(dev, monkeypatch):
    """``HipEncoder._trunk_pc`` and the heads, run once per norm kind and head with a spy on cer_enc_pc_conv: the (instantiation, producer form)
    pairs they launch are exactly the ones FORMS lists - single + ReLU, dual 1|2|4, dual 1|4 with a normalised B, dual with a plain B,
    with and without merged_out."""
    from cer_mvs_amd import _lib as L, ops
    from cer_mvs_amd.encoder_hip import HipEncoder
    from cer_mvs_amd.extractor import BasicEncoder
    lib = L.load()
    real = lib.cer_enc_pc_conv
    by_shape = {v[1:]: k for k, v in INST.items()}
    seen = set()

    def spy(*a):
        seen.add((by_shape[tuple(a[14:19])], (a[4] & 7, a[1] is not None, a[2] is not None, a[3] is not None, a[5] is not None)))
        assert not a[4] & 8
        return real(*a)
    monkeypatch.setattr(lib, "cer_enc_pc_conv", spy)
    x = hashed((3, 3, 32, 48), 7001).to(dev)
    for kind in ("instance", "none"):
        seen.clear()
        torch.manual_seed(1)
        for dim in (64, 128):
            eng = HipEncoder(BasicEncoder(output_dim=dim, norm_fn=kind), dev)
            assert eng.pc_trunk
            with torch.no_grad():
                if dim == 64:
                    _, _, h, w = eng.features(x, n_ref=1)
                    f1 = torch.zeros(h * w, 128, device=dev, dtype=torch.float16)
                    f2 = torch.zeros(2, (h + 4) * (w + 4), 128, device=dev, dtype=torch.float16)
                    eng.features_split(x, f1, f2, n_ref=1, flag=ops.overflow_flag(dev))
                else:
                    eng.context(x[:1])
        ops.check_overflow(dev)                           # (random weights: a clamped feature is no concern of this test)
        want = {(inst, f) for inst, forms in FORMS[kind].items() for f in forms}
        assert seen == want, (kind, sorted(seen - want), sorted(want - seen))


# ------------------------------------------------------------------------------------------------ RAW convolutions, both engines
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("kind", ["instance", "none"])
@pytest.mark.parametrize("inst", RAW)
def test_raw_convolution_launch_by_launch(dev, inst, kind, geom):
    """Every producer form of one RAW instantiation: cer_enc_pc_conv (three-term: out, merged_out, statistics records; then the FP6 form
    against its emulation), cer_enc_conv_f16x3 on the same input (element-wise, its own records at its own tiles; 32 -> 32 is the
    persistent streaming kernel: 600 tiles > 2 x CUs in "multi", 45 < 2 x CUs in "few"), and the two engines' outputs bit for bit."""
    layer, cin, cout, taps, stride, _ = INST[inst]
    conv, wt, b = packed_conv(dev, inst)
    N, h, w = geometry(dev, inst, geom)
    ho, wo = out_size(h, w, taps, stride)
    tile = enc_pc_tile(cout, taps, stride)
    for i, form in enumerate(sorted(FORMS[kind][inst])):
        key = f"{inst}/{kind}/{form_name(form)}/{geom}"
        A, sA, B, sB = make_inputs(dev, form, N, h, w, cin, 8000 + 100 * RAW.index(inst) + 10 * GEOMS.index(geom) + i)
        x64, mag_in = reference_input(A, sA, B, sB, form, N, h, w)
        ref, mag, mag_form = enc_conv_ref64(x64, wt, b, taps, stride, mag_in)
        form_abs = C_FORM * mag_form

        # ---- producer / consumer engine, three-term form
        out, _, part, m = pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, 0, want_part=kind == "instance")
        got = out.cpu()
        assert_covered_batch(got, key + " pc out", ho, wo, tile)
        record(key + "/pc", check_batch(got, ref, mag, C3, form_abs, key + " pc out", h=ho, w=wo, tile=tile))
        if m is not None:
            assert_covered_batch(m.cpu(), key + " merged_out", h, w, ENC_TILE)
            record(key + "/merged_out", check_batch(m.cpu(), x64, mag_in, C_FORM, 0.0, key + " merged_out", h=h, w=w, tile=ENC_TILE))
        if part is not None:
            mx = assert_stats_records(part.cpu(), got.view(N, ho, wo, cout), tile, K_STATS, key + " pc records")
            RECORD.setdefault("stats_records_max_ratio", {})[key + "/pc"] = mx

        # ---- tiled engine on the same input
        if form[2]:
            xt, tf, relu = host_input_fp32(A, sA, B, sB, form).to(dev), None, False
        else:
            xt, tf, relu = A, sA, True
        ttile = enc_conv_tile(stride)
        tout, _, tpart = tiled_conv(dev, conv, xt, tf, relu, N, h, w, want_part=kind == "instance")
        tgot = tout.cpu()
        assert_covered_batch(tgot, key + " tiled out", ho, wo, ttile)
        record(key + "/tiled", check_batch(tgot, ref, mag, C3, form_abs, key + " tiled out", h=ho, w=wo, tile=ttile))
        if tpart is not None:
            mx = assert_stats_records(tpart.cpu(), tgot.view(N, ho, wo, cout), ttile, K_STATS, key + " tiled records")
            RECORD.setdefault("stats_records_max_ratio", {})[key + "/tiled"] = mx
        # ---- "the arithmetic of enc_conv.hip, bit for bit" (both are within their bounds at this point)
        same = torch.equal(got, tgot)
        RECORD.setdefault("pc_equals_tiled_bit_for_bit", {})[key] = same
        assert same, f"{key}: {int((got != tgot).sum())} of {got.numel()} elements differ between enc_pc.hip and enc_conv.hip (max {float((got - tgot).abs().max()):.3e})"

        # ---- FP6-correction form
        out6, _, part6, m6 = pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, 0, f6=True, want_part=kind == "instance")
        got6 = out6.cpu()
        assert_covered_batch(got6, key + " FP6 out", ho, wo, tile)
        again, _, part6b, _ = pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, 0, f6=True, want_part=kind == "instance")
        assert torch.equal(again.cpu(), got6), key + ": the FP6 form does not reproduce"
        if m6 is not None:                                # (the write-back does not depend on the arithmetic form)
            assert torch.equal(m6.cpu(), m.cpu())
        if part6 is not None:
            assert torch.equal(part6.cpu(), part6b.cpu())
            assert_stats_records(part6.cpu(), got6.view(N, ho, wo, cout), tile, K_STATS, key + " FP6 records")
        emu = emulate_fp6(x64, wt, b, taps, stride)
        assert_fp6_within_emulation(key, got6.view(N, ho, wo, cout), emu, ref, mag, got.view(N, ho, wo, cout))


# ------------------------------------------------------------------------------------------------ heads of the producer / consumer engine
def bordered(dev, N, ho, wo, C, border, seed):
    """A bordered fp32 output: NaN inside, a fixed finite pattern on the border texels -> (device buffer, the pattern on the host)."""
    hb, wb = ho + 2 * border, wo + 2 * border
    pat = hashed((N, hb, wb, C), seed, -3.0, 3.0)
    buf = pat.clone()
    buf[:, border:border + ho, border:border + wo] = float("nan")
    return buf.view(N, hb * wb, C).to(dev), pat


def split_interior(planes, N, ho, wo, border):
    """View of the data texels of ops.feat_split's layout (per block 8 planes [texels][16] halves)."""
    hb, wb = ho + 2 * border, wo + 2 * border
    return planes.view(N, 8, hb, wb, 16)[:, :, border:border + ho, border:border + wo]


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("kind", ["instance", "none"])
def test_feature_heads_launch_by_launch(dev, kind, geom):
    """FMAP (plain with scale 1 and 1/8, bordered with 1/8) element-wise, border texels back bit for bit; FSPLIT (plain and bordered, 1/8) =
    ops.feat_split of the FMAP output of the same configuration, bit for bit, NaN halves inside and the split of the pattern on the border
    before the launch; both in the three-term and the FP6 form."""
    from cer_mvs_amd import ops
    _, cin, cout, taps, stride, _ = INST["fmap"]
    conv, wt, b = packed_conv(dev, "fmap")
    N, h, w = geometry(dev, "fmap", geom)
    assert (N, h, w) == geometry(dev, "fsplit", geom)
    (form,) = FORMS[kind]["fmap"]
    assert FORMS[kind]["fsplit"] == {form}
    key = f"fmap/{kind}/{form_name(form)}/{geom}"
    A, sA, B, sB = make_inputs(dev, form, N, h, w, cin, 8500 + GEOMS.index(geom))
    x64, mag_in = reference_input(A, sA, B, sB, form, N, h, w)
    ref, mag, mag_form = enc_conv_ref64(x64, wt, b, taps, stride, mag_in)
    emu = emulate_fp6(x64, wt, b, taps, stride)
    flag = ops.overflow_flag(dev)
    for border, scale in ((0, 1.0), (0, 0.125), (2, 0.125)):
        outs = {}
        for f6 in (False, True):
            buf, pat = bordered(dev, N, h, w, cout, border, 8600 + border)
            pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, 1, f6=f6, out=buf, border=border, scale=scale)
            got = buf.cpu().view(N, h + 2 * border, w + 2 * border, cout)
            inner = got[:, border:border + h, border:border + w]
            where = f"{key} border {border} scale {scale}" + (" FP6" if f6 else "")
            assert_covered_batch(inner, where, h, w, ENC_TILE)
            rim = got.clone()
            rim[:, border:border + h, border:border + w] = pat[:, border:border + h, border:border + w]
            assert torch.equal(rim, pat), where + ": the kernel wrote border texels"
            outs[f6] = (buf, inner)
            if not f6:
                want = enc_head_ref64(ref, "fmap", scale, border)[:, border:border + h, border:border + w]
                record(f"{key}/b{border}_s{scale}", check_batch(inner, want, scale * mag, C3, scale * C_FORM * mag_form, where, h=h, w=w, tile=ENC_TILE))
            else:
                buf2, _ = bordered(dev, N, h, w, cout, border, 8600 + border)
                pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, 1, f6=True, out=buf2, border=border, scale=scale)
                assert torch.equal(buf2.cpu(), buf.cpu()), where + ": does not reproduce"
                assert_fp6_within_emulation(f"{key}/b{border}_s{scale}", inner, scale * emu, scale * ref, scale * mag, outs[False][1])
            if scale != 0.125:
                continue
            # FSPLIT of the same configuration: the planes feat_split makes of this very map (border pattern included)
            want_planes = ops.feat_split(buf)
            planes = want_planes.clone()
            split_interior(planes, N, h, w, border).fill_(float("nan"))
            assert bool(torch.isnan(split_interior(planes, N, h, w, border)).all())
            pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, 3, f6=f6, out=planes, border=border, scale=scale, flag=flag)
            assert bool(torch.isfinite(planes).all()), where + " FSPLIT: a NaN half is left (a tile nobody wrote)"
            assert torch.equal(planes.view(torch.int16), want_planes.view(torch.int16)), where + " FSPLIT differs from feat_split(FMAP)"
    assert not ops.check_overflow(dev)


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("kind", ["instance", "none"])
def test_context_head_launch_by_launch(dev, kind, geom):
    """CTX: tanh of the first 64 channels into ``out``, relu of the others into ``out2``; 4 x 32 tiles; three-term and FP6 form."""
    _, cin, cout, taps, stride, _ = INST["ctx"]
    conv, wt, b = packed_conv(dev, "ctx")
    N, h, w = geometry(dev, "ctx", geom)
    (form,) = FORMS[kind]["ctx"]
    key = f"ctx/{kind}/{form_name(form)}/{geom}"
    tile = enc_pc_tile(cout, taps, stride)
    A, sA, B, sB = make_inputs(dev, form, N, h, w, cin, 8700 + GEOMS.index(geom))
    x64, mag_in = reference_input(A, sA, B, sB, form, N, h, w)
    ref, mag, mag_form = enc_conv_ref64(x64, wt, b, taps, stride, mag_in)
    want = torch.cat(enc_head_ref64(ref, "ctx"), -1)
    act = torch.cat([torch.full((64,), ACT_ABS, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)])
    got = {}
    for f6 in (False, True):
        nan = lambda: torch.full((N, h * w, 64), float("nan"), device=dev)
        net, inp, _, _ = pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, 2, f6=f6, out=nan(), out2=nan())
        got[f6] = torch.cat([net.cpu(), inp.cpu()], -1).view(N, h, w, cout)
        assert_covered_batch(got[f6], key + (" FP6" if f6 else ""), h, w, tile)
    record(key, check_batch(got[False], want, mag, C3, C_FORM * mag_form + act, key, h=h, w=w, tile=tile))
    net, inp, _, _ = pc_conv(dev, conv, A, sA, B, sB, form, N, h, w, 2, f6=True, out=torch.empty(N, h * w, 64, device=dev), out2=torch.empty(N, h * w, 64, device=dev))
    assert torch.equal(torch.cat([net.cpu(), inp.cpu()], -1).view(N, h, w, cout), got[True]), key + ": the FP6 form does not reproduce"
    emu = torch.cat(enc_head_ref64(emulate_fp6(x64, wt, b, taps, stride), "ctx"), -1)
    assert_fp6_within_emulation(key, got[True], emu, want, mag, got[False])


# ------------------------------------------------------------------------------------------------ tiled engine: heads, merge, whole encoder
@pytest.mark.parametrize("geom", ["few", "tiny", "row"])
@pytest.mark.parametrize("head", ["fmap64", "fmap128", "ctx128", "ctx64"])
def test_tiled_engine_heads(dev, head, geom):
    """cer_enc_conv_f16x3 with the FMAP (plain and bordered) and CTX epilogues at 64 -> 64 and 64 -> 128, on a plain input as ``_head`` gives
    it (no statistics, no ReLU)."""
    inst = "fmap" if head.endswith("64") else "ctx"
    _, cin, cout, taps, stride, _ = INST[inst]
    conv, wt, b = packed_conv(dev, inst)
    N, h, w = geometry(dev, "fmap", geom)
    x = hashed((N, h * w, cin), 8800 + GEOMS.index(geom), -1.0, 2.0).to(dev)
    x64 = x.cpu().double().view(N, h, w, cin)
    ref, mag, _ = enc_conv_ref64(x64, wt, b, taps, stride)
    key = f"tiled_{head}/{geom}"
    if head.startswith("fmap"):
        for border, scale in ((0, 1.0), (2, 0.125)):
            buf, pat = bordered(dev, N, h, w, cout, border, 8900 + border)
            tiled_conv(dev, conv, x, None, False, N, h, w, epi=1, out=buf, border=border, scale=scale)
            got = buf.cpu().view(N, h + 2 * border, w + 2 * border, cout)
            inner = got[:, border:border + h, border:border + w]
            assert_covered_batch(inner, key, h, w, ENC_TILE)
            rim = got.clone()
            rim[:, border:border + h, border:border + w] = pat[:, border:border + h, border:border + w]
            assert torch.equal(rim, pat), key + ": the kernel wrote border texels"
            record(f"{key}/b{border}", check_batch(inner, scale * ref, scale * mag, C3, 0.0, key, h=h, w=w, tile=ENC_TILE))
    else:
        half = cout // 2
        nan = lambda: torch.full((N, h * w, half), float("nan"), device=dev)
        net, inp, _ = tiled_conv(dev, conv, x, None, False, N, h, w, epi=2, out=nan(), out2=nan())
        got = torch.cat([net.cpu(), inp.cpu()], -1).view(N, h, w, cout)
        assert_covered_batch(got, key, h, w, ENC_TILE)
        act = torch.cat([torch.full((half,), ACT_ABS, dtype=torch.float64), torch.zeros(half, dtype=torch.float64)]).view(1, cout)
        record(key, check_batch(got, torch.cat(enc_head_ref64(ref, "ctx"), -1), mag, C3, act, key, h=h, w=w, tile=ENC_TILE))


MERGE_SHAPES = [(3, 19 * 134, 32), (3, 10 * 67, 64), (3, 3 * 5, 32), (52, 19 * 134, 64)]


@pytest.mark.parametrize("N,P,C", MERGE_SHAPES, ids=[f"{n}x{p}x{c}" for n, p, c in MERGE_SHAPES])
def test_merge_kernel(dev, N, P, C):
    """cer_enc_merge_f32 with the flag combinations ``HipEncoder.trunk`` and ``_head`` use (1|4, 1|2|4), with and without each statistics
    tensor: |err| <= 4 * 2^-24 * mag_in.  3 x 15 x 32 / 4 = 360 float4 is no multiple of the block; 52 x 2546 x 64 / 4 is more than the grid's
    8192 x 256 threads (the stride loop)."""
    from cer_mvs_amd import _lib as L
    assert (3 * 15 * 32 // 4) % 256 and 52 * 2546 * 64 // 4 > 8192 * 256
    a = (hashed((N, P, C), 9001, -1.0, 2.0) + 0.5 * hashed((C,), 9002)).to(dev)
    b = (hashed((N, P, C), 9003, -1.5, 1.5) + 0.3 * hashed((C,), 9004)).to(dev)
    stats = lambda t: instance_stats64(t.cpu().double()).float().contiguous().to(dev)
    sa, sb = stats(a), stats(b)
    combos = [(fl, ua, ub) for fl in (5, 7) for ua in (True, False) for ub in (True, False)]
    if N > 3:
        combos = [(5, True, True), (7, False, False)]
    for fl, ua, ub in combos:
        out = torch.full((N, P, C), float("nan"), device=dev)
        L.check(L.load().cer_enc_merge_f32(L.dev_ptr(a, "a"), L.dev_ptr(sa if ua else None, "sa"), L.dev_ptr(b, "b"), L.dev_ptr(sb if ub else None, "sb"),
                                           L.dev_ptr(out, "out"), N, P, C, fl, L.cur_stream()), "enc_merge")
        want, mag_in = enc_input_ref64(a, sa if ua else None, True, b, sb if ub else None, bool(fl & 2), relu_sum=True)
        got = out.cpu().double()
        bad = ~((got - want).abs() <= C_FORM * mag_in)
        assert not bool(bad.any()), (f"merge flags {fl} sa {ua} sb {ub}: {int(bad.sum())} elements beyond 4 * 2^-24 * mag_in, first (image, pixel, channel) "
                                     f"{tuple(bad.nonzero()[0].tolist())}")
        RECORD.setdefault("merge_max_ratio", {})[f"{N}x{P}x{C}/flags{fl}_sa{int(ua)}_sb{int(ub)}"] = float(((got - want).abs() / (C_FORM * mag_in).clamp_min(1e-300)).max())


@pytest.mark.parametrize("which", ["fnet", "cnet"])
def test_tiled_engine_whole_encoder_matches_oracle(dev, which, monkeypatch):
    """``encoder_hip.ENGINE = "tiled"``: the trunk of csrc/enc_conv.hip (RAW convolutions, the streaming kernel, four merge passes) and its
    head against the oracle at 72 x 104, to the bar of the default engine."""
    from cer_mvs_amd import RAFT, encoder_hip
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from oracle import cer_oracle as O
    monkeypatch.setattr(encoder_hip, "ENGINE", "tiled")
    images, _, _, _ = synthetic_scene(72, 104, 2, seed=8)
    model = RAFT(test_mode=True)
    sd = fill_state_dict(model.state_dict(), seed=13)
    model.load_state_dict(sd)
    x = images[0].float() * (2 / 255.0) - 1
    eng = encoder_hip.HipEncoder(getattr(model, which), dev)
    calls = []
    real = eng._merge
    monkeypatch.setattr(eng, "_merge", lambda *a: (calls.append(a[-1]), real(*a))[1])
    with torch.no_grad():
        got = eng.forward_nchw(x.to(dev)).cpu()
        ref = O.encoder(x, sd, which + ".", "instance" if which == "fnet" else "none")
    assert calls == [7, 5, 5, 5]                          # the tiled trunk really ran: its four merge passes
    assert got.shape == ref.shape and rel_l1(got, ref) < 1e-5


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("nblk", [1, 63, 256, 257, 600])
def test_stats_reduce_alone(dev, nblk):
    """cer_enc_stats_reduce_f32 on synthetic records (N = 2, C = 64; 257 and 600 take the ``b += 256`` loop) against a float64 reduction of
    the same records.  Channel 5 holds all-equal values: the variance clamps at 0 and rstd = 1 / sqrt(eps)."""
    N, C, p = 2, 64, 256                                   # p pixels per tile
    m = hashed((N, nblk, C), 9100 + nblk, -1.0, 1.0).double() + 3.0 * hashed((1, 1, C), 9101).double()
    v = hashed((N, nblk, C), 9102 + nblk, 0.05, 2.0).double()
    m[:, :, 5], v[:, :, 5] = 0.5, 0.0
    part = torch.stack([p * m, p * (v + m * m)], -1).float().contiguous()
    pixels = nblk * p
    got = stats_reduce(dev, part.to(dev), pixels).cpu().double().view(N, C, 2)
    S, Q = part.double().sum(1)[..., 0], part.double().sum(1)[..., 1]
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    mean = S / pixels
    var = (Q / pixels - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    assert bool((var[:, 5] == 0).all()) and bool((got[:, 5, 1] == float(torch.tensor(1.0 / math.sqrt(eps), dtype=torch.float32))).all())
    em = (got[..., 0] - mean).abs() / mean.abs().clamp_min(U24 * torch.sqrt(Q / pixels))
    er = (got[..., 1] - rstd).abs() / rstd
    RECORD.setdefault("stats_reduce_max_ratio", {})[str(nblk)] = {"mean": float(em.max() / 2.0 ** -23), "rstd": float(er.max() / 2.0 ** -23)}
    assert float(em.max()) <= 2.0 ** -23 and float(er.max()) <= 2.0 ** -23, (float(em.max()), float(er.max()))


def test_statistics_of_a_badly_conditioned_channel(dev):
    """The 32 -> 32 convolution at 19 x 134, N = 2, with biases that put the output channels at |mean| / sigma of about 1, 10 and 30: the rstd
    that conv + reduce deliver against the float64 rstd of the float64 convolution (bound: module docstring).  Variance from Q / n - mean^2
    multiplies the rounding of the fp32 records by 1 + mean^2 / sigma^2."""
    inst, form, N = "c32", SINGLE, 2
    _, cin, cout, taps, stride, _ = INST[inst]
    h, w = 19, 134
    A, sA, _, _ = make_inputs(dev, form, N, h, w, cin, 9200)
    x64, mag_in = reference_input(A, sA, None, None, form, N, h, w)
    wt = weights()[INST[inst][0] + ".weight"]
    y0 = enc_conv_ref64(x64, wt, None, taps, stride)[0]
    st0 = instance_stats64(y0, eps=0.0).view(N, cout, 2)
    target = torch.tensor([1.0, 10.0, 30.0], dtype=torch.float64).repeat(cout)[:cout]
    bias = (target / st0[0, :, 1] - st0[0, :, 0]).float()                      # image 0: mean = target * sigma
    conv, wt, b = packed_conv(dev, inst, bias=bias)
    ref, mag, mag_form = enc_conv_ref64(x64, wt, b, taps, stride, mag_in)
    f = ref.reshape(N, h * w, cout)
    mean = f.mean(1)
    var = ((f - mean[:, None]) ** 2).mean(1)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    rstd = 1.0 / torch.sqrt(var + eps)
    cond = mean.abs() / torch.sqrt(var)
    assert float(cond.max()) > 25 and float(cond.min()) < 2 and bool(((cond > 8) & (cond < 12)).any()), cond
    share = (C3 * mag + C_FORM * mag_form).reshape(N, h * w, cout).amax(1) / torch.sqrt(var)
    bound = 0.5 * K_STATS * U24 * (1 + cond ** 2) + 2.0 ** -23 + share
    figures = {}
    for engine in ("pc", "tiled"):
        if engine == "pc":
            out, _, part, _ = pc_conv(dev, conv, A, sA, None, None, form, N, h, w, 0, want_part=True)
        else:
            out, _, part = tiled_conv(dev, conv, A, sA, True, N, h, w, want_part=True)
        check_batch(out.cpu(), ref, mag, C3, C_FORM * mag_form, f"conditioned {engine}", h=h, w=w, tile=ENC_TILE)
        got = stats_reduce(dev, part, h * w).cpu().double().view(N, cout, 2)
        err = (got[..., 1] - rstd).abs() / rstd
        ratio = err / bound
        worst = int(ratio.reshape(-1).argmax())
        figures[engine] = {"max_rel_err_rstd": float(err.max()), "max_ratio_to_bound": float(ratio.max()), "cond_at_worst": float(cond.reshape(-1)[worst]),
                           "max_rel_err_by_cond": {str(t): float(err[(cond > 0.7 * t) & (cond < 1.4 * t)].max()) for t in (1, 10, 30)}}
        print(f"  rstd of conditioned channels, {engine}: {figures[engine]}")
        assert bool((err <= bound).all()), (engine, figures[engine])
    RECORD["conditioned_rstd"] = figures
    if os.environ.get("CER_PARITY_RECORD"):               # how far production sits from that regime: |mean| / sigma of every trunk convolution output
        from cer_mvs_amd.synthetic import synthetic_scene
        images, _, _, _ = synthetic_scene(72, 104, 2, seed=0)
        x = images[0].float() * (2 / 255.0) - 1
        survey = {}
        for which, kind in (("fnet", "instance"), ("cnet", "none")):
            outs = {}
            enc_chain_ref64(x, weights(), which + ".", kind, outputs=outs)
            for name, y in outs.items():
                s = instance_stats64(y, eps=0.0).view(y.shape[0], -1, 2)
                survey[f"{which}.{name}"] = float((s[..., 0].abs() * s[..., 1]).max())
        survey["max"] = max(survey.values())
        RECORD["mean_over_sigma_survey_72x104_seed5"] = survey
