"""csrc/cloud.hip on the MI355X: ``fusion.point_cloud`` against the host tail of ``fusion.fusion`` (``backproject`` in numpy float64 + boolean
indexing), ``fusion.color_grid`` against its numpy restatement (tests/test_cloud_cpu.py), ``ops.disp_to_depth`` against ``inference.disp_to_depth``,
the reference capture of the point cloud, and determinism at full size.

The coordinate bound.  Host and device evaluate, per coordinate, the same seven-operation fp64 chain on the same fp64 inputs (x d and y d are exact:
an integer times a float32): c_j = sum_k Kinv[j,k] v_k (three products, two sums), X_i = sum_j Einv[i,j] c_j + Einv[i,3] (three products, three
sums) - numpy in BLAS's order, the kernel as a chain of fma.  With u = 2^-53, a sum of products of m + 1 factors of rounded quantities in ANY order,
fused or not, is within gamma_m S of the exact value, gamma_m = m u / (1 - m u), S the sum of the absolute values of its terms (Higham, Accuracy and
Stability of Numerical Algorithms, Lemma 3.1 / eq. 3.4).  Every term of X_i passes through at most 7 roundings (product and two sums inside c_j, product
and three sums outside), so |computed - exact| <= gamma_7 T for both, with T = sum_j |Einv[i,j]| sum_k |Kinv[j,k] v_k| + |Einv[i,3]|, and the two fp64
values differ by at most 2 gamma_7 T.  The device then rounds once to float32: half a float32 ulp of the value.  Hence
    |xyz_device - xyz_host64| <= 0.5 ulp32(|xyz_host64|) + 2 gamma_7 T,
nothing looser: gamma = 2 gamma_7 ~ 14 * 2^-53 is derived here, not tuned."""
import numpy as np
import pytest
import torch

from conftest import rel_l1
from test_cloud_cpu import _bits, color_grid_numpy

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GAMMA = 2 * (7 * U / (1 - 7 * U))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def ulp32(v):
    """spacing of float32 at |v| (v float64): 2^(e - 24) for 2^(e-1) <= |v| < 2^e, not below the denormal spacing"""
    _, e = np.frexp(np.abs(v))
    return np.where(v == 0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def host_cloud(masks, est, Ks, Es, colors, order):
    """the tail of fusion.fusion() on host arrays: (xyz float64 [n,3], rgb uint8 [n,3], T float64 [n,3])"""
    from cer_mvs_amd import fusion
    xyz, rgb, T = [], [], []
    for ref in order:
        m = masks[ref].astype(bool)
        K, E = Ks[ref].numpy(), Es[ref].numpy()
        xyz.append(fusion.backproject(est[ref], m, K, E))
        rgb.append((colors[ref].transpose(1, 2, 0)[m] * 255).astype(np.uint8))
        ys, xs = np.nonzero(m)                               # row-major, as boolean indexing
        d = est[ref][m].astype(np.float64)
        v = np.abs(np.stack([xs * d, ys * d, d]))            # [3, n]
        Ki, Ei = np.abs(np.linalg.inv(K).astype(np.float64)), np.abs(np.linalg.inv(E).astype(np.float64))
        T.append((Ei[:3, :3] @ (Ki @ v) + Ei[:3, 3:4]).T)
    return np.concatenate(xyz, 0), np.concatenate(rgb, 0), np.concatenate(T, 0)


def assert_cloud(xyz, rgb, masks, est, Ks, Es, colors, order, what=""):
    want_xyz, want_rgb, T = host_cloud(masks, est, Ks, Es, colors, order)
    assert xyz.dtype == np.float32 and rgb.dtype == np.uint8
    assert xyz.shape == want_xyz.shape and rgb.shape == want_rgb.shape, (what, xyz.shape, want_xyz.shape)
    assert np.array_equal(rgb, want_rgb), what
    if len(want_xyz):
        err = np.abs(xyz.astype(np.float64) - want_xyz)
        bound = 0.5 * ulp32(want_xyz) + GAMMA * T
        worst = float((err / bound).max())
        print(f"point_cloud {what}: n = {len(xyz)}, max error / bound = {worst:.3f}, floats equal to float32(host64): "
              f"{float((xyz == want_xyz.astype(np.float32)).mean()):.6f}")
        assert (err <= bound).all(), (what, worst)


def _cameras(N, h, w, seed=3):
    from cer_mvs_amd.synthetic import synthetic_scene
    _, poses, intr, _ = synthetic_scene(32, 32, N - 1, seed=seed)
    K, E = intr[0].clone().float(), poses[0].clone().float()
    K[:, 0, 0] = K[:, 1, 1] = 1.8 * w
    K[:, 0, 2], K[:, 1, 2] = w / 2.0 + 0.37, h / 2.0 - 0.21
    return K, E


def _inputs(N, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    est = (0.4 + 2.0 * torch.rand(N, h, w, generator=g)).float()
    est[:, ::7, ::5] *= -1.0                                 # (untrained depth maps do go negative: same arithmetic)
    est[:, 3::11, 2::13] = 0.0
    col = torch.rand(N, 3, h, w, generator=g)
    grid = torch.randint(0, 256, (N, 3, h, w), generator=g).float() / 255.0          # values that sit on the integer boundaries of c * 255
    pick = torch.rand(N, 3, h, w, generator=g) < 0.5
    return est, torch.where(pick, grid, col).float().contiguous()


def _masks(kind, N, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(N, h, w, dtype=torch.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "corners":
        for i in range(N):
            y, x = ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))[i % 4]
            m[i, y, x] = 255                                 # (any non-zero byte is set, as .astype(bool) on the host)
    elif kind == "quarter":
        m = (torch.rand(N, h, w, generator=g) < 0.25).to(torch.uint8)
    elif kind == "runs":                                     # long empty and long full stretches across tile and wave boundaries
        flat = (torch.arange(N * h * w) // 700) % 3 == 1
        m = flat.reshape(N, h, w).to(torch.uint8)
    return m


@pytest.mark.parametrize("size", [(37, 51), (64, 80), (131, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["zeros", "ones", "corners", "quarter", "runs"])
def test_point_cloud_matches_host_tail(dev, kind, size):
    """n, the order, every colour byte and every coordinate (to the derived bound) against backproject + numpy indexing: empty and full masks, one pixel
    per view in each corner, density 0.25; 37x51 = 1887 and 131x257 = 33 667 pixels are multiples of neither 64 nor 256 nor the 2048-pixel tile"""
    from cer_mvs_amd import fusion
    h, w = size
    N = 5
    K, E = _cameras(N, h, w)
    est, col = _inputs(N, h, w, seed=h + w)
    masks = _masks(kind, N, h, w, seed=7)
    orders = {"all": list(range(N)), "permutation": [3, 0, 4, 1, 2], "subset": [4, 1]}
    for name, order in orders.items():
        xyz, rgb = fusion.point_cloud(masks.to(dev), est.to(dev), K, E, col.to(dev), order)
        assert xyz.is_cuda and rgb.is_cuda and xyz.shape[1:] == (3,) and rgb.shape[1:] == (3,)
        assert len(xyz) == int(masks[order].bool().sum())
        if kind == "zeros":
            assert len(xyz) == 0 and len(rgb) == 0
        assert_cloud(xyz.cpu().numpy(), rgb.cpu().numpy(), masks.numpy(), est.numpy(), K, E, col.numpy(), order, f"{kind} {h}x{w} {name}")


def test_point_cloud_listed_twice_and_more_views_than_a_launch_takes(dev):
    """a view may be listed more than once (it is emitted each time), and a list longer than the 128 views one launch carries is split"""
    from cer_mvs_amd import fusion
    N, h, w = 6, 19, 23
    K, E = _cameras(N, h, w)
    est, col = _inputs(N, h, w, seed=2)
    masks = _masks("quarter", N, h, w, seed=9)
    order = [(5 * i + 2) % N for i in range(301)]
    xyz, rgb = fusion.point_cloud(masks.to(dev), est.to(dev), K, E, col.to(dev), order)
    assert_cloud(xyz.cpu().numpy(), rgb.cpu().numpy(), masks.numpy(), est.numpy(), K, E, col.numpy(), order, "301 listed views")
    with pytest.raises(IndexError):
        fusion.point_cloud(masks.to(dev), est.to(dev), K, E, col.to(dev), [0, N])


@pytest.mark.parametrize("L", [1023, 1024, 1025, 2049])
def test_point_cloud_across_the_scan_chunk_edge(dev, L):
    """19x23 is one tile per view, so the scan sees one partial per listed view: L partials end one short of, on and one past its 1024-partial
    chunk, and two chunks and one over (the carry handed on twice); view 2 is empty, so zero partials sit inside and at both edges of a chunk
    (order[0] = order[1026] = 2, order[1023] = 5, order[1024] = 4).  Every list is also cut into launches of 128 views."""
    from cer_mvs_amd import fusion
    N, h, w = 6, 19, 23
    K, E = _cameras(N, h, w)
    est, col = _inputs(N, h, w, seed=2)
    masks = _masks("quarter", N, h, w, seed=9)
    masks[2] = 0
    order = [(5 * i + 2) % N for i in range(L)]
    xyz, rgb = fusion.point_cloud(masks.to(dev), est.to(dev), K, E, col.to(dev), order)
    assert len(xyz) == sum(int(masks[v].bool().sum()) for v in order)
    assert_cloud(xyz.cpu().numpy(), rgb.cpu().numpy(), masks.numpy(), est.numpy(), K, E, col.numpy(), order, f"{L} listed views")


def _golden_scene(g):
    from cer_mvs_amd.synthetic import synthetic_depth_maps, synthetic_scene, tensor_checksum
    H, W, V = int(g["H"]), int(g["W"]), int(g["V"])
    images, poses, intr, _ = synthetic_scene(H, W, V, seed=int(g["scene_seed"]))
    depths = synthetic_depth_maps(H, W, V, seed=int(g["scene_seed"]))
    assert tensor_checksum(depths) == int(g["depths_checksum"])
    return images[0], depths, intr[0].float(), poses[0].float(), V


def test_point_cloud_matches_reference_capture(dev, golden):
    """with the reference's final masks and the averaged depths the fusion loop computes for them: the captured point cloud of the reference's
    fusion() to the bars of test_fusion_driver_matches_reference_capture (1e-5 relative L1, colours equal) - and the host tail on the same inputs"""
    from cer_mvs_amd import fusion
    g = golden("fusion")
    images, depths, K, E, V = _golden_scene(g)
    N = V + 1
    pairs = [(i, [j for j in range(N) if j != i]) for i in range(N)]
    _, est, _, _ = fusion.fuse_depth_maps(depths.to(dev), K, E, pairs, glb=0.25)
    masks = torch.from_numpy((g["final_masks"] > 0).astype(np.uint8))
    colors = fusion.color_grid(images.to(dev).contiguous(), images.shape[2], images.shape[3])        # equal sizes: img / 255
    assert np.array_equal(_bits(colors.cpu().numpy()), _bits(images.numpy() / np.float32(255)))
    order = [ref for ref, _ in pairs]
    xyz, rgb = fusion.point_cloud(masks.to(dev), est, K, E, colors, order)
    assert len(xyz) == len(g["ply_xyz"]) == int(masks.sum())
    err = rel_l1(xyz.cpu(), torch.from_numpy(g["ply_xyz"]))
    print(f"point_cloud vs the reference's capture: n = {len(xyz)}, rel_l1 = {err:.3e}")
    assert err < 1e-5
    assert np.array_equal(rgb.cpu().numpy(), g["ply_rgb"])
    assert_cloud(xyz.cpu().numpy(), rgb.cpu().numpy(), masks.numpy(), est.cpu().numpy(), K, E, colors.cpu().numpy(), order, "fusion.npz scene")


@pytest.mark.parametrize("H,W,k", [(64, 80, 1), (240, 320, 2), (1184, 1600, 4), (256, 320, 4), (36, 60, 3), (48, 40, 8)])
def test_color_grid_equals_restatement(dev, H, W, k):
    from cer_mvs_amd import fusion
    g = torch.Generator().manual_seed(H * k)
    img = torch.randint(0, 256, (3, 3, H, W), generator=g).float()
    img[2] = torch.rand(3, H, W, generator=g) * 255.0        # (not only byte values)
    got = fusion.color_grid(img.to(dev), H // k, W // k)
    want = color_grid_numpy(img.numpy(), H // k, W // k)
    assert tuple(got.shape) == want.shape
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert np.array_equal((got.cpu().numpy() * np.float32(255)).astype(np.uint8), (want * np.float32(255)).astype(np.uint8))
    with pytest.raises(ValueError, match=r"fusion\(\)"):
        fusion.color_grid(img.to(dev), H // k + 1, W // k)


def test_disp_to_depth_equals_host_function(dev):
    from cer_mvs_amd import ops
    from cer_mvs_amd.inference import disp_to_depth
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(296 * 400, generator=g) * 4 - 1).float()
    special = torch.tensor([0.0, -0.0, 1e-39, -1e-39, 1.4e-45, 1e-38, 3e38, -3e38, float("inf"), float("-inf"), 1.0, -1.0, 3.0, 1e-20, 255.0])
    x[:len(special)] = special
    x[1000:1100] = 0.0
    x[2000:2100] *= 1e-40                                    # denormals
    want = disp_to_depth(x.numpy().reshape(296, 400))
    got = ops.disp_to_depth(x.to(dev).reshape(296, 400))
    assert want.dtype == np.float32 and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    stack = torch.full((3, 296, 400), -7.0, device=dev)      # into a slice of a depth stack
    ops.disp_to_depth(x.to(dev).reshape(1, 1, 296, 400), out=stack[1])
    assert np.array_equal(_bits(stack[1].cpu().numpy()), _bits(want)) and bool((stack[0] == -7).all()) and bool((stack[2] == -7).all())


def test_full_size_is_deterministic_and_complete(dev):
    """1184x1600, 11 views, mask area about 0.25: two runs are byte-equal, n is the mask area, and view 4 checked against the host tail"""
    from cer_mvs_amd import fusion
    N, h, w = 11, 1184, 1600
    K, E = _cameras(N, h, w)
    g = torch.Generator(device=dev).manual_seed(5)
    masks = (torch.rand(N, h, w, device=dev, generator=g) < 0.25).to(torch.uint8)
    est = 0.4 + 2.0 * torch.rand(N, h, w, device=dev, generator=g)
    col = torch.rand(N, 3, h, w, device=dev, generator=g)
    order = list(range(N))
    a = fusion.point_cloud(masks, est, K, E, col, order)
    b = fusion.point_cloud(masks, est, K, E, col, order)
    n = int(masks.sum())
    assert len(a[0]) == len(a[1]) == n and 0.24 < n / masks.numel() < 0.26
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    one = fusion.point_cloud(masks, est, K, E, col, [4])
    lo = int(masks[:4].sum())
    assert torch.equal(one[0].view(torch.int32), a[0][lo:lo + len(one[0])].view(torch.int32)) and torch.equal(one[1], a[1][lo:lo + len(one[1])])
    assert_cloud(one[0].cpu().numpy(), one[1].cpu().numpy(), masks.cpu().numpy(), est.cpu().numpy(), K, E, col.cpu().numpy(), [4], "full size, view 4")
