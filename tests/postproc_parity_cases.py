"""The inputs of tests/test_postproc_parity_gpu.py, shared with tests/test_postproc_parity_cpu.py, which runs the same checkers on the CPU
oracles and on planted corruptions: the geometric-consistency scenes (cameras of ``parity_check.geo_cameras``, depths of
``synthetic_depth_maps(seed=3)``), the multires shape pairs and the image-preparation geometries.  Deterministic, the same on every machine;
every float64 reference is computed once per session and handed out unchanged."""
import functools

import numpy as np
import torch

import parity_check as pc
from test_oracle_golden import hashed

# (id, H, W, S, (thre1, thre2), special values).  37 x 51 = 1887 pixels: no multiple of 64 or 256, n = 2 and 3 (the vote rule's smallest
# forms); 131 x 257 = 132 blocks of 256 pixels: more than the 64 counters of the mask area, S = 10 the most the kernel takes.
GEO_TIGHT = (33.0, 33.0 * 325)                               # the tightest thresholds the suite uses (tests/test_fusion_gpu.py)
GEO_CASES = [("37x51-S1", 37, 51, 1, (4.0, 1300.0), False), ("37x51-S2", 37, 51, 2, (4.0, 1300.0), False),
             ("67x93-S5", 67, 93, 5, (4.0, 1300.0), False), ("131x257-S10", 131, 257, 10, (4.0, 1300.0), False),
             ("131x257-S10-loose", 131, 257, 10, (0.4, 130.0), False), ("131x257-S10-tight", 131, 257, 10, GEO_TIGHT, False),
             ("67x93-S5-special", 67, 93, 5, (4.0, 1300.0), True)]
GEO_IDS = [c[0] for c in GEO_CASES]
UNDECIDABLE_CAP = 0.01                                       # of the elements of any one output, per level for the masks
BOTH_OUTCOMES = 0.05                                         # of a level's decided mask elements
RIM_SHARE = 0.01                                             # of the (view, pixel) samples


@functools.lru_cache(maxsize=None)
def geo_case(cid):
    """-> dict: depth_ref [H,W], depth_src [S,H,W], K, E ([S+1,...], view 0 the reference), cams [S,60] (fusion.compose_cams, fp32), th, S, H, W."""
    from cer_mvs_amd import fusion
    from cer_mvs_amd.synthetic import synthetic_depth_maps
    _, H, W, S, th, special = GEO_CASES[GEO_IDS.index(cid)]
    K, E = pc.geo_cameras(S + 1, H, W)
    depths = synthetic_depth_maps(H, W, S, seed=3).clone()
    if special:
        d = depths[0]
        d[3::7, 2::11] = 0.0                                 # a sprinkling of zero, negative and NaN reference pixels
        d[5::9, 4::13] *= -1.0
        d[1::12, 6::10] = float("nan")
        depths[2, 20:31, 40:57] = float("nan")               # a source view with a NaN block ...
        depths[4, 44:49, :] = 0.0                            # ... and one with a band of zeros
    src = list(range(1, S + 1))
    cams = fusion.compose_cams(K[0], E[0], K[src], E[src])
    return dict(depth_ref=depths[0].contiguous(), depth_src=depths[src].contiguous(), K=K, E=E, cams=cams, th=th, S=S, H=H, W=W)


@functools.lru_cache(maxsize=None)
def geo_ref(cid):
    c = geo_case(cid)
    return pc.geo_ref64(c["depth_ref"].numpy(), c["depth_src"].numpy(), c["cams"].numpy(), *c["th"])


def geo_oracle_outputs(cid, depth_src=None, padding_mode="zeros"):
    """The fp32 CPU restatement (oracle/fusion_oracle.py) on a case -> the keyword arguments of ``parity_check.check_geo``, as numpy, and
    "drep_raw", the reprojected depth before the m10 gate.  ``depth_src`` / ``padding_mode``: planted corruptions (other source maps; a
    sampler that clamps to the border instead of padding with zeros)."""
    import torch.nn.functional as F
    from oracle import fusion_oracle as FO
    c = geo_case(cid)
    S, K, E = c["S"], c["K"], c["E"]
    src = c["depth_src"] if depth_src is None else depth_src
    rep = lambda t: t[None].repeat(S, *([1] * t.dim()))
    keep = FO.bilinear_sample
    if padding_mode != "zeros":
        def sample(img, x, y):
            H, W = img.shape[-2:]
            return F.grid_sample(img, torch.stack([2 * x / (W - 1) - 1, 2 * y / (H - 1) - 1], dim=-1), padding_mode=padding_mode, align_corners=True)
        FO.bilinear_sample = sample
    try:
        args = (rep(c["depth_ref"]), rep(K[0]), rep(E[0]), src, K[1:], E[1:])
        masks, _, drep, xs, ys, rel = FO.check_geometric_consistency(*args, *c["th"])
        raw = FO.reproject_with_depth(*args)[0]
        geo, est = FO.vote(c["depth_ref"], K[0], E[0], src, K[1:], E[1:], *c["th"])
    finally:
        FO.bilinear_sample = keep
    return dict(xs=xs.numpy(), ys=ys.numpy(), rel=rel.numpy(), drep=drep.numpy(), masks9=torch.stack(masks).to(torch.uint8).numpy(),
                geo_mask=geo.to(torch.uint8).numpy(), depth_est=est.numpy(), drep_raw=raw.numpy())


def vote_from_masks(masks9, drep, depth_ref, cmp_ge=True, upto=None):
    """fusion.py:226-236 on literal outputs (numpy): masks9 [9,S,H,W], drep [S,H,W] (zero outside m10) -> (geo uint8, est fp32)."""
    S = masks9.shape[1]
    n = 1 + S
    cnt = masks9.astype(np.int64).sum(1)
    ge = (lambda a, b: a >= b) if cmp_ge else (lambda a, b: a > b)
    geo = cnt[8] >= n
    for i in range(2, min((n if upto is None else upto), 11)):
        geo = geo | ge(cnt[i - 2], i)
    est = (drep.astype(np.float32).sum(0, dtype=np.float32) + depth_ref) / (cnt[8] + 1).astype(np.float32)
    return geo.astype(np.uint8), est.astype(np.float32)


# ---- multires: (scale-1 shape, scale-2 shape)
MR_SHAPES = [((37, 53), (74, 106)), ((45, 64), (121, 173)), ((60, 80), (60, 80)), ((60, 80), (60, 95)), ((1, 1), (5, 7)), ((1, 9), (4, 30)),
             ((2, 2), (33, 47)), ((50, 70), (23, 31))]
MR_DOWN = [1, 2, 3]
MR_TH = 0.02


def mr_maps(shape1, shape2, seed=21):
    """-> (a, b) float32 numpy: a scale-1 map with zeros and negatives sprinkled in (finite: the resize treats them like any value) and,
    when the sizes are equal (no resize: the select must hand the scale-1 value on as np.where does), NaN and +-inf as well; b within /
    beyond 2 % of the resized scale-1 map, so that both branches of the select are taken."""
    from oracle import multires_oracle as M
    (h1, w1), (h2, w2) = shape1, shape2
    a = hashed((h1, w1), seed, 0.5, 3.0).numpy().copy()
    if h1 * w1 > 4:
        a.reshape(-1)[1::7] = 0.0
        a.reshape(-1)[3::11] *= -1.0
    if (h1, w1) == (h2, w2):
        a[4::13, 3::11] = np.nan
        a[7::17, 5::19] = np.inf
        a[9::23, 2::29] = -np.inf
    with np.errstate(all="ignore"):
        big = M.resize_linear(a, (h2, w2))
    big = np.where(np.isfinite(big), big, 1.0).astype(np.float32)
    b = (big * (1 + 0.05 * hashed((h2, w2), seed + 1, -1.0, 1.0).numpy())).astype(np.float32)
    return a, b


# ---- image preparation: (H0, W0, rescale or (H2, W2), crop (h, w) or None)
PREP_CASES = [(67, 93, 2, None), (67, 93, 0.5, None), (67, 93, 1.37, None), (67, 93, 2, (133, 177)), (67, 93, 0.5, (32, 44)),
              (67, 93, 1.37, (88, 120)), (67, 93, 1, None), (67, 93, 1, (64, 88)), (33, 65, (65, 129), None), (33, 65, (1, 129), None),
              (40, 64, (17, 1), None), (5, 7, (300, 401), None), (5, 7, (300, 401), (297, 400))]
PREP_FORMS = ["f32", "u8", "u8bgr"]


def prep_geometry(H0, W0, rescale, crop):
    """(H2, W2, y0, x0, H, W) of a case: ``ops.prep_geometry`` for a rescale factor, the same centre crop for an explicit resized size."""
    if not isinstance(rescale, tuple):
        from cer_mvs_amd.ops import prep_geometry as g
        return g(H0, W0, rescale, crop)
    H2, W2 = rescale
    if crop is None:
        return H2, W2, 0, 0, H2, W2
    return H2, W2, (H2 - crop[0]) // 2, (W2 - crop[1]) // 2, crop[0], crop[1]


def prep_image(H0, W0, form, seed=11):
    """-> (the kernel's input: float32 [3,H0,W0] or uint8 [H0,W0,3]; the fp32 values it reads as [3,H0,W0] in output channel order)."""
    img = hashed((3, H0, W0), seed + H0, 0.0, 255.0)
    if form == "f32":
        return img.contiguous(), img
    u8 = img.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
    chw = u8.permute(2, 0, 1).float()
    return u8, (chw.flip(0) if form == "u8bgr" else chw).contiguous()
