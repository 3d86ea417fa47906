"""The inputs of tests/test_wide_parity_gpu.py, shared with tests/test_wide_parity_cpu.py, which runs the same references and bounds on an
fp32 emulation with planted corruptions: the image shapes of the update-loop launches, the tensors one GRU iteration starts from, the
stand-alone ``delta_tail`` cases, and the geometries of the cost-volume walk with their fp32-oracle yardstick.  Deterministic, the same on
every machine; every float64 reference is computed once per session and handed out unchanged."""
import functools
import math

import torch

import parity_check as pc
from test_oracle_golden import hashed

# The smallest shapes at which the kernels can still go wrong (f16x3 kernel: 4 x 32 pixel tiles, fp32 kernel: 8 x 16):
#   1 x 1 every tap outside the image; 3 x 70 shorter than a tile; 4 x 32 exactly one tile; 5 x 33 one row and one column spill into second
#   tiles; 13 x 101 partial tiles on both axes and interior tiles, of which the row at ty0 = 8 has a 9 x 9 window that leaves the image at the
#   bottom; 24 x 96 exact tiling with one interior tile column.
SHAPES = [(1, 1), (3, 70), (4, 32), (5, 33), (13, 101), (24, 96)]
WITH_INTERIOR = {(13, 101), (24, 96)}
MODES = ["f16x3", "fp32"]
CASCADE = [(64, 64, 2), (-1, 320, 2)]
STAGES = ((64, 0.0025 / 64), (44, 0.0025 / 320))            # (D, incre) of that cascade
WEIGHT_SEED = 5


def loop_inputs(h, w, stage):
    """What one stage of the loop starts from, on the CPU in fp32: the folded level-0 volume rows [P, rs], origin, disp [P], the hidden
    state (tanh range) and the context features (ReLU range) [P, 64].  The disparity steps put indices below 0, beyond the row and on
    integers (tests/test_hip_parity.py::test_lookup_edge_cases)."""
    from cer_mvs_amd import ops
    D, incre = STAGES[stage]
    P = h * w
    seed = 7000 + 101 * h + 7 * w + 1000 * stage
    _, _, rs = ops.row_layout(D, 3, compact=True)
    vol = hashed((P, rs), seed + 1, -4.0, 4.0)              # (a 64-channel dot of fnet features / 8: a few units)
    origin = hashed((P,), seed + 2, 0.001, 0.0015)
    steps = hashed((P,), seed + 3, -40.0, 60.0)
    steps[::97] = torch.round(steps[::97])
    for i, v in ((0, -100.0), (1, 1e6), (2, 3.0), (3, -22.0), (P - 1, 1e6), (P - 2, -100.0)):
        if 0 <= i < P:
            steps[i] = v
    disp = origin + steps * incre
    net = torch.tanh(hashed((P, 64), seed + 4, -2.0, 2.0))
    inp = torch.relu(hashed((P, 64), seed + 5, -1.0, 2.0))
    return dict(vol=vol, origin=origin, disp=disp, net=net, inp=inp, D=D, incre=incre)


# ---------------------------------------------------------------------------------------------- delta_tail on its own
# Strips are 16 pixels wide and a block holds 4 of them: widths around one strip, and 33 = three strips, so that at height 5 the 15 strips
# fill three blocks and leave a fourth partial.
DT_CASES = [(C, h, w) for C in (256, 512) for h in (1, 5) for w in (1, 15, 16, 17, 33)]


def delta_tail_inputs(C, h, w):
    seed = 8000 + C + 37 * h + w
    hid = torch.relu(hashed((h * w, C), seed, -1.0, 2.0))
    wt = hashed((9, C), seed + 1, -0.05, 0.05)
    disp = hashed((h * w,), seed + 2, 0.0005, 0.0025)
    return hid, wt, 0.0173, disp


# ---------------------------------------------------------------------------------------------- the cost-volume walk
WALK_SHAPES = [(7, 13), (19, 45)]                           # neither pixel count is a multiple of the 4 pixels a block walks
WALK_DS = [64, 44, 20]
WALK_VS = [1, 3]
WALK_GEOMS = ["lateral", "vertical", "diagonal", "converging"]
WALK_INCRE = (0.0025 / 64, 0.0025 / 320)                    # per stage
WALK_SHIFT_PX = 1500.0                                      # focal length x baseline: 0 .. 3.75 texels over stage 0's hypotheses


def walk_geometry(geom, h, w, V):
    """-> (poses [V + 1, 4, 4], intrinsics [V + 1, 3, 3]) fp32, view 0 the reference (identity pose).  Z stays positive over every
    hypothesis range: the fp32 yardstick is bounded (geometries where it is not are held to a reference built from restated fp32
    coordinates instead: tests/cost_geometry_cases.py, tests/test_cost_geometry_gpu.py)."""
    f = 1.8 * w
    K = torch.tensor([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    b = WALK_SHIFT_PX / f
    poses = torch.eye(4).repeat(V + 1, 1, 1)
    for v in range(1, V + 1):
        sign = -1.0 if v == 2 else 1.0
        if geom == "lateral":
            poses[v, 0, 3] = sign * b * (1 + 0.5 * (v - 1))
        elif geom == "vertical":
            poses[v, 1, 3] = -sign * b * (1 + 0.4 * (v - 1))
        elif geom == "diagonal":                            # + a small in-plane rotation
            a = 0.03 * v
            poses[v, :2, :2] = torch.tensor([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
            poses[v, 0, 3], poses[v, 1, 3] = 0.7 * b * sign, (-0.6, 0.55, -0.1)[v - 1] * b
        elif geom == "converging":                          # rotation about y + the baseline that keeps a point at depth c in view
            th = 0.12 * v * sign
            R = torch.tensor([[math.cos(th), 0.0, math.sin(th)], [0.0, 1.0, 0.0], [-math.sin(th), 0.0, math.cos(th)]])
            c = torch.tensor([0.0, 0.0, b / abs(math.sin(0.12))])
            poses[v, :3, :3] = R
            poses[v, :3, 3] = c - R @ c
        else:
            raise ValueError(geom)
    return poses, K.repeat(V + 1, 1, 1)


@functools.lru_cache(maxsize=None)
def walk_case(geom, stage, h, w, V):
    """-> dict(fmaps [V + 1, 64, h, w], poses, intr, Pij [V, 4, 4] (oracle.cer_oracle.pij_matrices), disp_in [h, w], shift, incre)."""
    from oracle import cer_oracle as O
    seed = 9000 + 13 * h + w + 100 * V + 1000 * stage + WALK_GEOMS.index(geom)
    poses, intr = walk_geometry(geom, h, w, V)
    fmaps = hashed((V + 1, 64, h, w), seed, -2.0, 2.0)
    disp_in = torch.zeros(h, w) if stage == 0 else hashed((h, w), seed + 1, 0.0012, 0.0022)
    Pij = O.pij_matrices(poses, intr, [0] * V, list(range(1, V + 1))).contiguous()
    return dict(fmaps=fmaps, poses=poses, intr=intr, Pij=Pij, disp_in=disp_in, shift=stage == 0, incre=WALK_INCRE[stage])


@functools.lru_cache(maxsize=None)
def walk_reference(geom, stage, h, w, V, D):
    """The float64 restatement on ALL pixels and the fp32 oracle judged by it, per view and folded (mean over the views): -> dict with
    ref / norm [V, P, D] and [P, D] (norm floored at the volume's mean magnitude), origin [P] (the oracle's, fp32), and the yardstick's
    figures {"views": (max, p99.9), "fold": (max, p99.9)} of |oracle - ref| / norm."""
    from oracle import cer_oracle as O
    c = walk_case(geom, stage, h, w, V)
    ref, norm, _ = pc.cost_volume_ref64(c["fmaps"], c["Pij"], D, c["incre"], c["disp_in"], c["shift"])
    yard, origin = O.cost_volume(c["fmaps"], c["poses"], c["intr"], D, c["incre"], c["disp_in"], c["shift"])
    out = {"origin": origin.reshape(-1)}
    figures = {}
    for key, r, n, y in (("views", ref, norm, yard.double()), ("fold", ref.mean(0), norm.mean(0), yard.double().mean(0))):
        n = n.clamp_min(float(r.abs().mean()))
        r2, n2, y2 = (walk_rows(t) for t in (r, n, y))
        rep = pc.check_elementwise(y2, r2, n2, 1.0, where="fp32 oracle", h=h, w=w, tile=(1, 4))
        out[key] = (r2, n2)
        figures[key] = (rep.max_ratio, rep.p999_ratio)
    out["yardstick"] = figures
    return out


def walk_rows(t):
    """[V, P, D] -> [P, V * D] (a view's hypotheses side by side: one row per pixel for the element-wise check); [P, D] stays."""
    return t if t.dim() == 2 else t.permute(1, 0, 2).reshape(t.shape[1], -1)
