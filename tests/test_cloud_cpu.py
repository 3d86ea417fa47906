"""Point cloud on the device (csrc/cloud.hip, fusion.point_cloud / color_grid, scan.reconstruct_scan), the parts that need no GPU: the C ABI
and its argument checks, a numpy restatement of the colour grid against the host resize it replaces, the integer-ratio restriction and the
camera helper factored out of ``fusion.fusion``."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

CLOUD_SYMBOLS = ("cer_cloud_partials", "cer_cloud_count_u8", "cer_cloud_emit_f32", "cer_color_grid_f32", "cer_disp_to_depth_f32")


# ---------------------------------------------------------------- numpy restatement of cer_color_grid_f32 (also used by the GPU tests)
def _taps(in_size, out_size):
    """torch's upsample_bilinear2d(align_corners=False) source taps, every operation a float32 operation"""
    scale = np.float32(in_size) / np.float32(out_size)
    s = scale * (np.arange(out_size, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    s = np.maximum(s, np.float32(0))
    i0 = np.minimum(s.astype(np.int32), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, np.float32(1) - l1, l1


def color_grid_numpy(prepared, h, w):
    """prepared float32 [N,3,H,W], values 0..255 -> [N,3,h,w], values 0..1: v / 255, then ly0 * (lx0 a + lx1 b) + ly1 * (lx0 c + lx1 d), every
    product and sum rounded to float32"""
    prepared = np.asarray(prepared, dtype=np.float32)
    H, W = prepared.shape[2:]
    v = prepared / np.float32(255)
    y0, y1, ly0, ly1 = _taps(H, h)
    x0, x1, lx0, lx1 = _taps(W, w)
    a, b = v[:, :, y0[:, None], x0[None, :]], v[:, :, y0[:, None], x1[None, :]]
    c, d = v[:, :, y1[:, None], x0[None, :]], v[:, :, y1[:, None], x1[None, :]]
    ly0, ly1 = ly0[:, None], ly1[:, None]
    out = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
    assert out.dtype == np.float32
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- C ABI
def test_cloud_abi_symbols_are_declared():
    from cer_mvs_amd import _lib as L
    names = L.exported_symbols()
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    for n in CLOUD_SYMBOLS:
        assert n in names
        assert f" {n}(" in hdr
    for n in CLOUD_SYMBOLS[1:]:
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P      # int f(..., stream)
    assert L.ABI_VERSION > 1090
    lib = L.load()                                        # (loads without a GPU; refuses a library that lacks a declared symbol)
    assert lib.cer_abi_version() == L.ABI_VERSION
    mk = open(os.path.join(REPO, "cer-mvs_amd", "csrc", "Makefile")).read()
    assert "cloud.hip" in mk


def test_cloud_partials_counts_tiles():
    from cer_mvs_amd import _lib as L
    lib = L.load()
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    assert "#define CER_CLOUD_TILE 2048" in hdr
    assert lib.cer_cloud_partials(11, 1184, 1600) == 11 * 925
    assert lib.cer_cloud_partials(49, 296, 400) == 49 * 58           # 118 400 pixels: 57.8 tiles
    assert lib.cer_cloud_partials(1, 1, 1) == 1
    assert lib.cer_cloud_partials(3, 37, 51) == 3
    assert lib.cer_cloud_partials(0, 4, 4) == -1 and lib.cer_cloud_partials(1, 0, 4) == -1


def test_cloud_entry_points_refuse_bad_arguments():
    """argument checks run before any launch: null pointers, non-positive sizes, listed views outside 0..N-1, a capacity that is not the total;
    an empty cloud launches nothing and succeeds"""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    ok, bad, neg = (ctypes.c_int * 3)(0, 2, 1), (ctypes.c_int * 3)(0, 3, 1), (ctypes.c_int * 3)(0, -1, 1)
    none = ctypes.POINTER(ctypes.c_int)()
    assert lib.cer_cloud_count_u8(null, 3, 8, 8, ok, 3, fake, fake, fake, null) == -1
    assert lib.cer_cloud_count_u8(fake, 3, 8, 8, none, 3, fake, fake, fake, null) == -1
    assert lib.cer_cloud_count_u8(fake, 3, 8, 8, ok, 0, fake, fake, fake, null) == -1
    assert lib.cer_cloud_count_u8(fake, 3, 0, 8, ok, 3, fake, fake, fake, null) == -1
    assert lib.cer_cloud_count_u8(fake, 3, 8, 8, bad, 3, fake, fake, fake, null) == -1       # view 3 of 3
    assert lib.cer_cloud_count_u8(fake, 3, 8, 8, neg, 3, fake, fake, fake, null) == -1
    assert lib.cer_cloud_count_u8(fake, 3, 8, 8, ok, 3, null, fake, fake, null) == -1
    assert lib.cer_cloud_count_u8(fake, 3, 8, 8, ok, 3, fake, fake, null, null) == -1
    assert lib.cer_cloud_count_u8(fake, 3, 1 << 16, 1 << 15, ok, 3, fake, fake, fake, null) == -2    # 2^31 pixels per view
    emit = lambda order, total, cap, xyz=fake, rgb=fake, masks=fake, cams=fake: lib.cer_cloud_emit_f32(
        masks, fake, cams, fake, 3, 8, 8, order, 3, fake, total, cap, xyz, rgb, null)
    assert emit(ok, 5, 5, masks=null) == -1
    assert emit(ok, 5, 5, cams=null) == -1
    assert emit(bad, 5, 5) == -1
    assert emit(ok, -1, -1) == -1
    assert emit(ok, 5, 4) == -2 and emit(ok, 4, 5) == -2 and emit(ok, 0, 1) == -2            # total and capacity disagree
    assert emit(ok, 5, 5, xyz=null) == -1 and emit(ok, 5, 5, rgb=null) == -1
    assert emit(ok, 0, 0, xyz=null, rgb=null) == 0                                            # n == 0: nothing is launched
    assert lib.cer_color_grid_f32(null, fake, 2, 8, 8, 4, 4, null) == -1
    assert lib.cer_color_grid_f32(fake, fake, 0, 8, 8, 4, 4, null) == -1
    assert lib.cer_color_grid_f32(fake, fake, 2, 67, 93, 17, 23, null) == -2                  # not an integer ratio
    assert lib.cer_color_grid_f32(fake, fake, 2, 8, 8, 4, 2, null) == -2                      # two different ratios
    assert lib.cer_color_grid_f32(fake, fake, 2, 4, 4, 8, 8, null) == -2                      # an enlargement
    assert lib.cer_disp_to_depth_f32(null, fake, 16, null) == -1
    assert lib.cer_disp_to_depth_f32(fake, null, 16, null) == -1
    assert lib.cer_disp_to_depth_f32(fake, fake, 0, null) == -1


def test_python_wrappers_refuse_cpu_tensors_and_ragged_ratios():
    from cer_mvs_amd import fusion
    with pytest.raises(ValueError, match=r"fusion\(\)"):
        fusion.color_grid(torch.zeros(2, 3, 67, 93), 17, 23)
    with pytest.raises(ValueError, match=r"fusion\(\)"):
        fusion.color_grid(torch.zeros(2, 3, 96, 128), 37, 51)
    with pytest.raises(ValueError, match=r"fusion\(\)"):
        fusion.color_grid(torch.zeros(2, 3, 64, 80), 32, 20)             # 2 and 4
    with pytest.raises(RuntimeError, match="CUDA"):
        fusion.color_grid(torch.zeros(2, 3, 64, 80), 16, 20)
    with pytest.raises(RuntimeError, match="CUDA"):
        fusion.point_cloud(torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(2, 4, 4), torch.eye(3).repeat(2, 1, 1),
                           torch.eye(4).repeat(2, 1, 1), torch.zeros(2, 3, 4, 4), [0, 1])


# ---------------------------------------------------------------- colour grid
@pytest.fixture
def host_resize_threads():
    """torch's CPU resize has two arithmetic forms: the separable one the kernel restates, ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d),
    which it runs when it may use more than one thread and the output plane has more than 4-5 thousand pixels (the resized planes below have 11 520 or more), and a four-term sum
    ((w00 a + w01 b) + w10 c) + w11 d otherwise - 22 % of the floats differ in the last bit between the two.  A single-threaded session would
    compare against the other form: pin at least two threads for the comparison."""
    n = torch.get_num_threads()
    torch.set_num_threads(max(2, n))
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("H,W,k", [(64, 80, 1), (240, 320, 2), (1184, 1600, 4), (384, 480, 4), (512, 640, 2)])
def test_color_grid_restatement_equals_the_host_resize(host_resize_threads, H, W, k):
    """the arithmetic cer_color_grid_f32 implements, restated in numpy float32, is F.interpolate(bilinear, align_corners=False) of img / 255
    bit for bit at integer ratios - and so are the colour bytes (c * 255 truncated), a quarter of which sit on an integer boundary at ratio 4"""
    from cer_mvs_amd import fusion
    h, w = H // k, W // k
    g = torch.Generator().manual_seed(H + k)
    img = torch.randint(0, 256, (2, 3, H, W), generator=g).float()
    got = color_grid_numpy(img.numpy(), h, w)
    want = F.interpolate(img / 255.0, size=(h, w), mode="bilinear", align_corners=False).numpy()
    assert np.array_equal(_bits(got), _bits(want))
    # ... and what fusion() itself forms per view: HWC numpy / 255.0, _resize unless the sizes are equal
    hwc = img[1].permute(1, 2, 0).numpy() / 255.0
    assert hwc.dtype == np.float32
    host = hwc if k == 1 else fusion._resize(hwc, h, w)
    assert np.array_equal(_bits(got[1].transpose(1, 2, 0)), _bits(host))
    gb, hb = (got[1].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8), (host * 255).astype(np.uint8)
    assert np.array_equal(gb, hb)
    if k == 4:
        on_edge = (host * 255) == np.floor(host * 255)
        assert on_edge.mean() > 0.15                     # a tolerance on the colours would hide differences exactly there


def test_color_grid_restatement_is_not_exact_at_ragged_ratios(host_resize_threads):
    """why other ratios are refused: the weights round, and about 40 % of the floats differ from the host resize in the last bit"""
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (1, 3, 67, 93), generator=g).float()
    got = color_grid_numpy(img.numpy(), 17, 23)
    want = F.interpolate(img / 255.0, size=(17, 23), mode="bilinear", align_corners=False).numpy()
    diff = _bits(got) != _bits(want)
    assert diff.any() and np.abs(got - want).max() < 1e-6


# ---------------------------------------------------------------- camera helper
def _fusion_fit_before(K, img_shape, dep_shape):
    """the lines fusion() ran before the helper existed, on shapes: (K', scale, flag, index, resized image shape)"""
    K = K.clone()
    scale = float(dep_shape[0]) / img_shape[0]
    flag = 0
    if dep_shape[1] / img_shape[1] > scale:
        scale = float(dep_shape[1]) / img_shape[1]
        flag = 1
    shape = tuple(img_shape)
    if scale != 1.0:
        shape = (int(round(img_shape[0] * scale)), int(round(img_shape[1] * scale)))
    if flag == 0:
        index = int(math.ceil((shape[1] - dep_shape[1]) / 2))
    else:
        index = int(math.ceil((shape[0] - dep_shape[0]) / 2))
    K[:2, :] *= scale
    K[0 if flag == 0 else 1, 2] -= index
    return K, scale, flag, index, shape


@pytest.mark.parametrize("img,dep,flag", [((64, 88), (16, 20), 0), ((1184, 1600), (296, 400), 0), ((72, 80), (16, 20), 1), ((67, 93), (17, 31), 1),
                                          ((16, 20), (16, 20), 0), ((256, 320), (128, 160), 0)])
def test_camera_helper_equals_what_fusion_computed(img, dep, flag):
    from cer_mvs_amd import fusion
    K = torch.tensor([[2892.33, 0.013, 823.205], [0.0, 2883.175, 619.071], [0.0, 0.0, 1.0]])
    want, scale, wflag, index, shape = _fusion_fit_before(K, img, dep)
    assert wflag == flag
    got = fusion.depth_grid_geometry(img[0], img[1], dep[0], dep[1])
    assert got == (scale, flag, shape[0], shape[1], index)
    keep = K.clone()
    K2 = fusion.modify_camera_parameters(K.clone(), got[0], got[4], got[1])
    assert torch.equal(K2, want) and torch.equal(K, keep)
    if img == dep:
        assert got[0] == 1.0 and got[4] == 0 and torch.equal(K2, K)
    if img == (64, 88):
        assert got[4] == 1 and float(K2[0, 2]) == float(torch.tensor(823.205) * 0.25 - 1)


def test_cloud_cams_are_the_float32_inverses_promoted():
    from cer_mvs_amd import fusion
    from cer_mvs_amd.synthetic import synthetic_scene
    _, poses, intr, _ = synthetic_scene(32, 32, 3, seed=2)
    K, E = intr[0].float(), poses[0].float()
    cams = fusion.cloud_cams(K, E)
    assert cams.dtype == torch.float64 and tuple(cams.shape) == (4, fusion.CLOUD_CAM_DOUBLES)
    for i in range(4):
        ki, ei = np.linalg.inv(K[i].numpy()), np.linalg.inv(E[i].numpy())
        assert ki.dtype == np.float32 and ei.dtype == np.float32
        assert np.array_equal(cams[i, :9].numpy(), ki.astype(np.float64).reshape(9))
        assert np.array_equal(cams[i, 9:21].numpy(), ei.astype(np.float64)[:3].reshape(12))
        assert not cams[i, 21:].any()
