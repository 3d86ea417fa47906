"""Every host-side weight packer of csrc/pack.cpp, byte for byte (no GPU): tests/golden/pack_digests.json holds, per case, the sha256 of the
packed buffer and every returned size / code / scale, recorded from the library of the commit named in the file.  Inputs are closed-form (an
integer hash of the flat index mapped to a heavy-tailed float: no library RNG) with planted values for the paths a random tensor misses:

  zero   one 32-channel block of exact zeros                          FP6 block scale at its floor (te = -100, E8M0 byte 16)
  bump   a block whose maximum is 7.875 * 2^k (just above 7.75 * 2^k) the FP6 block scale's one-up step
  tiny   magnitudes near 1e-7                                         lo halves in the f16 subnormal range
  clamp  1e5 and -7e4                                                 the +-65504 clamp (only where the packer clamps)

`python tests/test_pack_digests.py --record` rewrites the golden file from the library in use (CER_MVS_LIB selects another build)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

DIGESTS = os.path.join(GOLDEN, "pack_digests.json")
FILL = 0xA5                                                   # output buffers start as this byte: what a packer leaves unwritten is pinned too
M32 = np.uint64(0xFFFFFFFF)


def _mix(h):
    h = h & M32
    h = ((h ^ (h >> np.uint64(16))) * np.uint64(0x85EBCA6B)) & M32
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def weights(shape, seed, amp=0.3):
    """fp32 [Cout, Cin, taps]: amp * u * 2^-k with u in [-1, 1) and k in 0..7 from two hashes of the flat index (every |w| < amp)."""
    i = np.arange(int(np.prod(shape)), dtype=np.uint64)
    h = _mix(i * np.uint64(0x9E3779B1) + np.uint64(seed) * np.uint64(0x7F4A7C15))
    k = _mix(h + np.uint64(0x165667B1)) & np.uint64(7)
    u = h.astype(np.float64) / 2147483648.0 - 1.0
    return (amp * u * np.ldexp(1.0, -k.astype(np.int64))).astype(np.float32).reshape(shape)


def plant(w, c_zero, c_at, rows=(1, 2, 3, 4, 5), clamp=True):
    """The planted values (module docstring): the zero block at channels c_zero .. c_zero + 31 of rows[0]; the others from channel c_at on,
    one row each: 0.4921875 = 7.875 * 2^-4 exceeds every hashed value, so it is its block's maximum."""
    w = w.copy()
    last = w.shape[2] - 1
    w[rows[0], c_zero:c_zero + 32, :] = 0.0
    w[rows[1], c_at + 3, last // 2] = 0.4921875
    w[rows[2], c_at, 0], w[rows[2], c_at + 5, last], w[rows[2], c_at + 9, last // 2] = 1e-7, -1.3e-7, 0.8e-7
    if clamp:
        w[rows[3], c_at + 1, 0], w[rows[4], c_at + 2, last] = 1e5, -7e4
    return w


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def packed(fn, size, *args):
    """Call a packer with a FILL-ed output buffer of `size` bytes in place of the argument `...`; -> {"ret", "sha256"}."""
    out = np.full(max(int(size), 16), FILL, dtype=np.uint8)
    ret = fn(*[out.ctypes.data if a is ... else a for a in args])
    return {"ret": int(ret), "sha256": hashlib.sha256(out.tobytes()).hexdigest()}


def run_cases(lib):
    from cer_mvs_amd import _lib as L
    res = {}

    # fp32 pack: a ragged tensor padded to 64 channels and the disparity source (nothing to clamp)
    ch, kind = ints(40, 49), ints(0, 1)
    w = plant(weights((32, 89, 9), 1), 0, 0, clamp=False)
    size = lib.cer_conv3x3_packed_size(32, 64 + 64)
    res["pack_f32"] = dict(packed(lib.cer_conv3x3_pack_f32, size * 4, w.ctypes.data, ..., 32, 89, ch, kind, 2), size=size)
    res["pack_f32/rejected"] = packed(lib.cer_conv3x3_pack_f32, 16, w.ctypes.data, ..., 32, 90, ch, kind, 2)

    # f16x3 packs, literal and collapsed
    ch, kind = ints(64, 49, 40), ints(3, 1, 0)
    w = plant(weights((64, 153, 9), 2), 32, 32)
    size = lib.cer_conv3x3_f16x3_packed_size(64, 64 + 64 + 64)
    res["f16x3"] = dict(packed(lib.cer_conv3x3_f16x3_pack, size * 2, w.ctypes.data, ..., 64, 153, ch, kind, 3), size=size)
    res["f16x3/rejected"] = dict(packed(lib.cer_conv3x3_f16x3_pack, 16, w.ctypes.data, ..., 48, 153, ch, kind, 3),
                                 size=lib.cer_conv3x3_f16x3_packed_size(48, 192))
    size = lib.cer_conv3x3_f16x3_collapsed_size(64, ch, kind, 3)
    res["f16x3_collapsed"] = dict(packed(lib.cer_conv3x3_f16x3_pack_collapsed, size * 2, w.ctypes.data, ..., 64, 153, ch, kind, 3), size=size)
    res["f16x3_collapsed/rejected"] = dict(packed(lib.cer_conv3x3_f16x3_pack_collapsed, 16, w.ctypes.data, ..., 64, 152, ch, kind, 3),
                                           size=lib.cer_conv3x3_f16x3_collapsed_size(48, ch, kind, 3))

    # s16 packs.  The shared scale comes from the weights WITHOUT the two huge entries, the packs then see them: with their own scale they would
    # stay below the clamp (the scale's return for them is recorded as log2S_clamp).
    for name, cout, chs, kinds, sxs, forms, c_zero in (("s16", 64, (64, 49, 64), (2, 1, 2), (L.S16_UNIT, L.S16_DISP, L.S16_RELU), (0, 1, 3, 5), 145),
                                                       ("s16_delta", 256, (64,), (2,), (L.S16_RELU,), (0, 2), 32)):
        n, cin = len(chs), sum(chs)
        ch, kind, sx = ints(*chs), ints(*kinds), ints(*sxs)
        base = weights((cout, cin, 9), 3 if n == 3 else 4)
        w0, w = plant(base, c_zero, c_zero, clamp=False), plant(base, c_zero, c_zero)
        log2S = lib.cer_conv3x3_s16_scale(w0.ctypes.data, cout, cin, ch, kind, sx, n)
        res[name + "/scale"] = {"log2S": int(log2S), "log2S_clamp": int(lib.cer_conv3x3_s16_scale(w.ctypes.data, cout, cin, ch, kind, sx, n))}
        for form in forms:
            size = lib.cer_conv3x3_s16_packed_size(cout, ch, kind, n, form)
            res[f"{name}/pack{form}"] = dict(packed(lib.cer_conv3x3_s16_pack, size * 2, w.ctypes.data, ..., cout, cin, ch, kind, sx, n, form, log2S),
                                             size=size)
        if 1 in kinds:
            size = lib.cer_conv3x3_s16_edge_size(cout)
            res[name + "/edge"] = dict(packed(lib.cer_conv3x3_s16_edge_pack, size * 2, w.ctypes.data, ..., cout, cin, ch, kind, sx, n, log2S), size=size)
            res[name + "/scale_rejected"] = {"log2S": int(lib.cer_conv3x3_s16_scale(w.ctypes.data, cout, cin - 1, ch, kind, sx, n))}
            res[name + "/pack_rejected"] = dict(packed(lib.cer_conv3x3_s16_pack, 16, w.ctypes.data, ..., cout, cin, ch, kind, sx, n, 6, log2S),
                                                size=lib.cer_conv3x3_s16_packed_size(cout, ints(64, 48, 64), kind, n, 0))
        else:                                                 # no disparity source: no rim filters
            res[name + "/edge_rejected"] = dict(packed(lib.cer_conv3x3_s16_edge_pack, 16, w.ctypes.data, ..., cout, cin, ch, kind, sx, n, log2S),
                                                size=lib.cer_conv3x3_s16_edge_size(48))

    # delta head projections (one output row: the plants share it, in different 32-channel blocks).  The s16 form scales by its own maximum, so
    # it runs without the huge entries too.
    for C in (128, 256):
        base = weights((1, C, 9), 5 + C)
        w = plant(base, 32, 64, rows=(0,) * 5)
        size = lib.cer_delta_proj_packed_size(C)
        res[f"delta_proj/{C}"] = dict(packed(lib.cer_delta_proj_pack, size * 2, w.ctypes.data, ..., C), size=size)
        size = lib.cer_delta_proj_s16_packed_size(C)
        for tag, ww in (("", plant(base, 32, 64, rows=(0,) * 5, clamp=False)), ("_clamp", w)):
            k = ctypes.c_int(-999)
            r = packed(lib.cer_delta_proj_s16_pack, size * 2, ww.ctypes.data, ..., C, ctypes.byref(k))
            res[f"delta_proj_s16{tag}/{C}"] = dict(r, size=size, log2s=k.value)
    w = weights((1, 200, 9), 6)
    res["delta_proj/rejected"] = dict(packed(lib.cer_delta_proj_pack, 16, w.ctypes.data, ..., 200), size=lib.cer_delta_proj_packed_size(200))
    k = ctypes.c_int(-999)
    res["delta_proj_s16/rejected"] = dict(packed(lib.cer_delta_proj_s16_pack, 16, w.ctypes.data, ..., 200, ctypes.byref(k)),
                                          size=lib.cer_delta_proj_s16_packed_size(200), log2s=k.value)

    # encoder packs: three terms, and the FP6 corrections
    for cout, cin, taps in ((32, 32, 9), (64, 32, 1), (128, 64, 1)):
        w = plant(weights((cout, cin, taps), 7 + cout), 0, cin - 32)
        size = lib.cer_enc_conv_packed_size(cout, cin, taps)
        for name, fn in (("enc", lib.cer_enc_conv_pack), ("enc_f6", lib.cer_enc_conv_pack_f6)):
            res[f"{name}/{cout}x{cin}x{taps}"] = dict(packed(fn, size * 2, w.ctypes.data, ..., cout, cin, taps), size=size)
    res["enc/rejected"] = dict(packed(lib.cer_enc_conv_pack, 16, w.ctypes.data, ..., 128, 64, 4), size=lib.cer_enc_conv_packed_size(128, 64, 4))
    res["enc_f6/rejected"] = packed(lib.cer_enc_conv_pack_f6, 16, w.ctypes.data, ..., 48, 64, 1)

    # stem [32][3][7][7]: it does not clamp
    w = plant(weights((32, 147, 1), 8), 0, 40, clamp=False)
    size = lib.cer_enc_stem_s16_packed_size()
    k = ctypes.c_int(-999)
    res["stem"] = dict(packed(lib.cer_enc_stem_s16_pack, size * 2, w.ctypes.data, ..., ctypes.byref(k)), size=size, log2s=k.value)
    k = ctypes.c_int(-999)
    res["stem/rejected"] = dict(packed(lib.cer_enc_stem_s16_pack, 16, None, ..., ctypes.byref(k)), log2s=k.value)
    return res


_results = {}


def results():
    if not _results:
        from cer_mvs_amd import _lib
        _results.update(run_cases(_lib.load()))
    return _results


GOLD = json.load(open(DIGESTS)) if os.path.exists(DIGESTS) else {"cases": {}}


def test_golden_file_names_its_commit_and_covers_every_case():
    assert len(GOLD["commit"]) == 40 and int(GOLD["commit"], 16) >= 0
    assert sorted(GOLD["cases"]) == sorted(results())
    for fn in ("pack_f32", "f16x3", "f16x3_collapsed", "s16/pack0", "s16/edge", "delta_proj/128", "delta_proj_s16/128", "enc/32x32x9", "enc_f6/32x32x9", "stem"):
        assert GOLD["cases"][fn]["ret"] == 0, fn
    rej = [k for k in GOLD["cases"] if "rejected" in k]
    assert len(rej) == 11 and all(GOLD["cases"][k].get("ret", -1) < 0 and GOLD["cases"][k].get("log2S", -100000) <= -100000 for k in rej)
    empty = hashlib.sha256(bytes([FILL]) * 16).hexdigest()
    assert all(GOLD["cases"][k]["sha256"] == empty for k in rej if "sha256" in GOLD["cases"][k])        # a refused call writes nothing


@pytest.mark.parametrize("case", sorted(GOLD["cases"]))
def test_packed_bytes_match_the_recorded_digests(case):
    assert results()[case] == GOLD["cases"][case]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    commit = subprocess.check_output(["git", "-C", REPO, "rev-parse", "HEAD"], text=True).strip()
    with open(DIGESTS, "w") as f:
        json.dump({"commit": commit, "cases": results()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(results())} cases from {commit}")
