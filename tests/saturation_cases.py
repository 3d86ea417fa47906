"""The clamp sites of the product kernels, who reports each, and the thresholds restated in numpy: shared by tests/test_saturation_cpu.py
(the census against the sources, the rounding facts) and tests/test_saturation_gpu.py (threshold pins, coverage of each check, the
flag-or-parity sweep, the protocol-level tests).  Plain module, no fixtures.

DESIGN.md 3f and include/cer_mvs.h promise that saturation is never silent: a split-f16 kernel that has to clamp an operand to the f16
range raises a bit of the sticky device flag.  ``CENSUS`` is the list of every place in cer-mvs_amd/csrc/*.hip and *.hpp (not
experimental/) where a value is clamped to that range, one row per site:

  file, site       the source file and the function / lambda / epilogue
  tensor           what the value is
  log2s, limit     the power-of-two scale applied before the clamp and the resulting threshold in the tensor's own units
  reporter, bit    "kernel": the launch checks what it clamps (exact: !(x * s <= 65504), before any ReLU, so NaN counts);
                   "writer": a kernel upstream bounds the operand instead; "scan": a later cer_f16_scan_overflow of the stored halves
                   (when: ``when``); "range": in range by construction (``why``); "nobody"
  lines            how many source lines of ``file`` holding the literal 65504 belong to the row

tests/test_saturation_cpu.py counts the lines with that literal per file and compares with the sums here: a new clamp cannot be added
without a row that says who reports it.  ``classes`` names the positions at which the GPU module plants a hot value for the row."""
import os

import numpy as np

F16_MAX = 65504.0
BIT_FEAT, BIT_HIDDEN, BIT_ACT, BIT_DISP = 1, 2, 4, 8
DISP_LIMIT = float(np.float32(5.1175))                 # CER_DISP_LIMIT (csrc/common.hpp)

PIXEL_CLASSES = ("first", "last", "partial_col", "partial_row", "one_row_odd", "interior", "rim")
CH64 = (0, 15, 16, 31, 32, 47, 48, 63)
CH256 = (0, 31, 32, 127, 128, 255)


def row(file, site, tensor, log2s, limit, reporter, bit=0, when="", why="", lines=0, classes=()):
    return dict(file=file, site=site, tensor=tensor, log2s=log2s, limit=limit, reporter=reporter, bit=bit, when=when, why=why, lines=lines,
                classes=tuple(classes))


CENSUS = [
    # ---- cost-volume feature rows (scale 2^6: the reference's / 8 is already applied)
    row("cost_lines.hip", "feat_split_kernel", "feature rows of the cost volume", 6, 1023.5, "kernel", BIT_FEAT, "every launch", lines=3,
        classes=("first", "last", "block_seam", "sign", "channels")),
    row("enc_pc.hip", "PC_EPI_FSPLIT epilogue", "feature rows written by the encoder head (after the head's own scale, 1 / 8)", 6, 1023.5,
        "kernel", BIT_FEAT, "every launch", lines=3, classes=("bias_channel", "input_pixel")),
    # ---- the s16 update loop (conv_s16.hip, lookup.hip): ReLU class at 2^4, unit class at 2^14, disparity features at 2^6
    row("conv_s16_shared.hpp", "sx_split8", "every frag16 / LDS operand split of the s16 kernels (the clamp itself; reported per user below)",
        None, None, "users", lines=2),
    row("lookup.hip", "lookup_encode_kernel, frag16 output", "c1 = relu(conv1x1(lookup))", 4, 4094.0, "kernel", BIT_ACT,
        "every launch, before the ReLU", lines=2, classes=PIXEL_CLASSES + ("channels64",)),
    row("conv_s16.hip", "RELU epilogue (st_split)", "c2 = relu(conv3x3(c1))", 4, 4094.0, "kernel", BIT_ACT, "every launch, before the ReLU",
        lines=1, classes=PIXEL_CLASSES + ("channels64",)),
    row("conv_s16.hip", "DELTA epilogue", "hidden map of the delta head (never reaches memory)", 4, 4094.0, "kernel", BIT_HIDDEN,
        "every launch, before the ReLU", lines=1, classes=PIXEL_CLASSES + ("channels256",)),
    row("conv_s16.hip", "gen_literal / gen_collapsed / rim correction (sx_split8 at disp_scale)", "100 * (d[q] - d[p]), 7 x 7 (9 x 9 collapsed) window",
        6, 10.235, "writer", BIT_DISP,
        "cer_delta_sum_f32 and the delta prologue of the lookup raise bit 8 when !(|d| <= 5.1175): any difference inside a window is then "
        "<= 10.235; a stage starts from zeros or from such an output.  Real disparities are ~1e-3: three orders of magnitude below",
        classes=("first", "last", "interior")),
    row("conv_s16.hip", "GATES epilogue: r * h; GRU epilogue: new h", "hidden state and r * h", 14, 3.998, "range",
        why="sigmoid in [0, 1] times |h| <= 1; the blend (1 - z) h + z tanh(.) is convex in values of magnitude <= 1; the initial h is a tanh"),
    row("conv_s16.hip", "LINEAR epilogue with a frag16 output", "not launched by the update loop (its LINEAR launches write acc32, unclamped)", None,
        None, "nobody"),
    row("conv_s16.hip", "cer_s16_layout_f32 to frag16", "inp (ReLU class), the initial hidden state (unit class)", 4, 4094.0, "scan", BIT_ACT,
        "_S16Loop.hoist scans inp once per forward; the hidden state is a tanh"),
    row("lookup.hip", "lookup_encode_kernel, split32 output (cer_split8)", "c1 of the f16x3 loop", 0, F16_MAX, "nobody"),
    # ---- the wide-range kernels and the encoders: clamp at the f16 maximum in the operand's own units, unreported
    row("common.hpp", "cer_split1 / cer_split2 / cer_split8", "operands of the f16x3 kernels (gru_f16x3.hip) and of the tiled encoder (enc_conv.hip)",
        0, F16_MAX, "nobody", lines=2),
    row("enc_stem.hip", "stem: image rows and normalised activations", "encoder stem operands", 0, F16_MAX, "nobody", lines=3),
    row("enc_pc.hip", "PC_YMAX (the constant is 65504 * 2048: the kernel works on 2048 x the values)", "normalised trunk activations", 0, F16_MAX,
        "nobody", lines=1),
]

KERNEL_REPORTERS = [r for r in CENSUS if r["reporter"] == "kernel"]


def census_lines():
    """{file: lines holding the literal 65504 that the census accounts for}"""
    out = {}
    for r in CENSUS:
        out[r["file"]] = out.get(r["file"], 0) + r["lines"]
    return {f: n for f, n in out.items() if n}


def source_lines(csrc):
    """{file: number of lines of cer-mvs_amd/csrc/<file> (*.hip, *.hpp; not experimental/) that contain the literal 65504}"""
    out = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".hpp")):
            with open(os.path.join(csrc, name)) as f:
                n = sum(1 for line in f if "65504" in line)
            if n:
                out[name] = n
    return out


# ------------------------------------------------------------------------------------------------ thresholds, restated
def f32(v):
    return np.float32(v)


def up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


def hi_half(v, log2s):
    """Bits of the hi half of the split of v at scale 2^log2s as the kernels form it: clamp to +-65504 in fp32, round to nearest even."""
    x = np.clip(np.float32(v) * np.float32(2.0 ** log2s), np.float32(-F16_MAX), np.float32(F16_MAX))
    return int(np.float16(x).view(np.uint16))


def is_clamped(v, log2s):
    return not (abs(float(np.float32(v)) * 2.0 ** log2s) <= F16_MAX)


def scan_hits(v, log2s):
    """What cer_f16_scan_overflow says about the hi half: at the f16 maximum or beyond (infinities, NaN), either sign."""
    return (hi_half(v, log2s) & 0x7FFF) >= 0x7BFF


# ReLU class (scale 2^4).  In-kernel checks are exact; a scan sees the rounded half: clean up to 4093, certain beyond 4094.
ACT_LOG2S, ACT_LIMIT, ACT_SCAN_CLEAN = 4, 4094.0, 4093.0
ACT_CLEAN, ACT_FLAG = f32(4094.0), up(4094.0)
# feature rows (scale 2^6)
FEAT_LOG2S, FEAT_LIMIT = 6, 1023.5
FEAT_CLEAN, FEAT_FLAG = f32(1023.5), up(1023.5)
# disparity (bit 8)
DISP_CLEAN, DISP_FLAG = f32(DISP_LIMIT), up(DISP_LIMIT)
# the flag-or-parity sweep: outside the (4093, 4094] band, so that the outcome of a scan is determined too
SWEEP = (1000.0, 4000.0, 4093.0, 5000.0, 2e4, 1e6)
