"""``scan.reconstruct_scan`` on the MI355X against the file pipeline it replaces - ``inference_scan`` -> PFMs -> ``fusion.fusion`` on the session's
prepared images - on a small synthetic scan with hashed weights and a pinned arithmetic form (no calibration forwards): depth maps, masks, averaged
depths, threshold history and colours identical, the points within the bound derived in tests/test_cloud_gpu.py of the file pipeline's float64 points,
the PLY equal byte for byte wherever the floats are; the two-pass form; and the saturation path, which must leave no file behind."""
import numpy as np
import pytest
import torch

from conftest import cached_scene
from test_cloud_gpu import GAMMA, host_cloud, ulp32

pytestmark = pytest.mark.gpu

CASCADE = [(64, 64, 3), (-1, 320, 3)]
M, NF = 6, 4
NAMES = [f"{i:08d}" for i in range(M)]
PAIRS = [[(i + d) % M for d in (2, 5, 1, 3, 4)] for i in range(M)]           # five listed, num_frames keeps four
# the host resize switches to another arithmetic form below roughly 4-5 thousand output pixels: 96 x 120 = 11 520 is well clear
SIZE, GH, GW = (384, 480), 96, 120
PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _model(dev):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    m = RAFT(cascade=CASCADE, test_mode=True, gru_precision="s16", enc_precision="f16x3", cost_precision="x3")
    m.load_state_dict(fill_state_dict(m.state_dict(), seed=9))
    return m.to(dev).eval()


def _scan(H, W):
    images, poses, intr, scale = cached_scene(H, W, M - 1, 4)
    return images[0], poses[0], intr[0], [scale * (1.0 + 0.01 * i) for i in range(M)]


def _fusion_loader(prepared, poses, intr):
    """what the reference's loader yields per reference view, backed by the session's prepared images and intrinsics"""
    out = []
    for i in range(M):
        idx = [i] + PAIRS[i][:NF]
        out.append((prepared[idx][None].clone(), poses[idx][None].clone(), intr[idx][None].clone(), [(NAMES[j],) for j in idx], None))
    return out


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    return head.decode("ascii") + "end_header\n", np.frombuffer(body, dtype=PLY_VERTEX)


@pytest.fixture(scope="module")
def both(dev, tmp_path_factory):
    """the file pipeline (a) and reconstruct_scan (b) on the same scan, once for the module"""
    from cer_mvs_amd import fusion
    from cer_mvs_amd.scan import ScanSession, inference_scan, reconstruct_scan
    tmp = tmp_path_factory.mktemp("reconstruct")
    images, poses, intr, scales = _scan(*SIZE)
    model = _model(dev)
    files = inference_scan(model, images, poses, intr, NAMES, PAIRS, scales, tmp / "a", num_frames=NF, streams=3)
    sess = ScanSession(model, images, poses, intr, streams=1)
    try:
        prepared, K, E = sess.prepared.cpu(), sess.intrinsics.clone(), sess.poses.clone()
        stack = sess.depths(PAIRS, scales, num_frames=NF).cpu().numpy()
    finally:
        sess.close()
    n = torch.get_num_threads()
    torch.set_num_threads(max(2, n))                         # (the host resize's separable form: tests/test_cloud_cpu.py host_resize_threads)
    try:
        a = fusion.fusion(_fusion_loader(prepared, E, K), tmp / "a", suffix=f"_scale1_nf{NF}", glb=0.25)
    finally:
        torch.set_num_threads(n)
    tm = {}
    b = reconstruct_scan(model, images, poses, intr, NAMES, PAIRS, scales, tmp / "b", num_frames=NF, glb=0.25, streams=3, write_depths=True,
                         timings=tm)
    return {"a": a, "b": b, "tmp": tmp, "files": files, "stack": stack, "K": K, "E": E, "prepared": prepared, "timings": tm}


def test_depth_stack_and_written_depths_equal_the_pfms(both):
    from cer_mvs_amd.fusion import read_pfm
    assert len(both["files"]) == M and both["stack"].shape == (M, GH, GW)
    for i, pa in enumerate(both["files"]):
        name = f"{NAMES[i]}_scale1_nf{NF}.pfm"
        assert pa.endswith(name)
        assert np.array_equal(both["stack"][i].view(np.uint32), read_pfm(pa).view(np.uint32)), name          # ScanSession.depths, bit for bit
        assert open(pa, "rb").read() == open(both["tmp"] / "b" / "depths" / name, "rb").read(), name          # write_depths=True, byte for byte
    assert sorted(p.name for p in (both["tmp"] / "b" / "depths").iterdir()) == sorted(f"{n}_scale1_nf{NF}.pfm" for n in NAMES)


def test_fusion_results_are_identical(both):
    a, b = both["a"], both["b"]
    assert set(a) == set(b) == {"masks", "depth_est", "xyz", "rgb", "threshold", "history"}
    assert b["masks"].dtype == a["masks"].dtype == bool and np.array_equal(a["masks"], b["masks"])
    assert np.array_equal(a["depth_est"].view(np.uint32), b["depth_est"].view(np.uint32))
    assert a["threshold"] == b["threshold"] and a["history"] == b["history"] and len(b["history"]) == 10
    print(f"reconstruct_scan: n = {len(b['xyz'])}, mask area = {a['masks'].mean():.4f}, history = {b['history'][-1]}, timings = {both['timings']}")
    assert len(a["xyz"]) == len(b["xyz"]) == int(a["masks"].sum()) > 1000
    assert b["rgb"].dtype == np.uint8 and np.array_equal(a["rgb"], b["rgb"])
    assert both["timings"]["cached"] is True and both["timings"]["d2h_bytes"] > 0


def test_points_are_within_the_bound_of_the_file_pipeline(both):
    from cer_mvs_amd import fusion
    a, b = both["a"], both["b"]
    assert b["xyz"].dtype == np.float32 and a["xyz"].dtype == np.float64
    scale, flag, _, _, index = fusion.depth_grid_geometry(SIZE[0], SIZE[1], GH, GW)
    assert (scale, flag, index) == (0.25, 0, 0)
    Ks = torch.stack([fusion.modify_camera_parameters(both["K"][i].clone().float(), scale, index, flag) for i in range(M)])
    colors = np.zeros((M, 3, GH, GW), np.float32)            # (only T is taken from this call)
    xyz64, _, T = host_cloud(a["masks"], a["depth_est"], Ks, both["E"].float(), colors, list(range(M)))
    assert np.array_equal(xyz64, a["xyz"])                   # the cameras above are the ones fusion() used
    err = np.abs(b["xyz"].astype(np.float64) - a["xyz"])
    bound = 0.5 * ulp32(a["xyz"]) + GAMMA * T
    print(f"reconstruct_scan xyz: max error / bound = {float((err / bound).max()):.3f}, floats equal to float32(host64): "
          f"{float((b['xyz'] == a['xyz'].astype(np.float32)).mean()):.6f}")
    assert (err <= bound).all()


def test_ply_and_masks_are_written_like_fusion_writes_them(both, tmp_path):
    from cer_mvs_amd import fusion
    a, b, tmp = both["a"], both["b"], both["tmp"]
    head, verts = _read_ply(tmp / "b" / "result.ply")
    n = len(b["xyz"])
    assert head == ("ply\nformat binary_little_endian 1.0\n" f"element vertex {n}\n" "property float x\nproperty float y\nproperty float z\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert len(verts) == n
    fusion.write_ply(str(tmp_path / "host.ply"), a["xyz"].astype(np.float32), a["rgb"])
    head_a, verts_a = _read_ply(tmp_path / "host.ply")
    assert head_a == head and len(verts_a) == n
    same = (b["xyz"] == a["xyz"].astype(np.float32)).all(1)
    assert same.mean() > 0.9
    assert verts[same].tobytes() == verts_a[same].tobytes()
    for c in ("red", "green", "blue"):
        assert np.array_equal(verts[c], verts_a[c])
    # what fusion() itself wrote next to the PFMs is that file
    assert open(tmp / "a" / "result.ply", "rb").read() == open(tmp_path / "host.ply", "rb").read()
    # the mask images: fusion() names them <index><suffix>, reconstruct_scan has no suffix to carry
    ext = sorted(p.suffix for p in (tmp / "b" / "mask").iterdir())[0]
    assert sorted(p.name for p in (tmp / "b" / "mask").iterdir()) == sorted(f"{i}{ext}" for i in range(M))
    for i in range(M):
        assert (tmp / "a" / "mask" / f"{i}_scale1_nf{NF}{ext}").read_bytes() == (tmp / "b" / "mask" / f"{i}{ext}").read_bytes()


def test_nothing_is_written_unless_asked(dev, tmp_path):
    from cer_mvs_amd.scan import reconstruct_scan
    images, poses, intr, scales = _scan(128, 160)
    out = reconstruct_scan(_model(dev), images, poses, intr, NAMES, PAIRS, scales, None, num_frames=NF, streams=2, write=False)
    assert out["masks"].shape == (M, 32, 40) and len(out["xyz"]) == int(out["masks"].sum())
    with pytest.raises(ValueError, match="output_folder"):
        reconstruct_scan(_model(dev), images, poses, intr, NAMES, PAIRS, scales, None, num_frames=NF)
    for bad in ((NAMES[:-1], PAIRS, scales), (NAMES, PAIRS[:-1], scales), (NAMES, PAIRS, scales[:-1])):
        with pytest.raises(ValueError, match="one entry per image"):
            reconstruct_scan(None, images, poses, intr, *bad, None, write=False)         # (refused before a model or a session is built)


def test_two_pass_form_equals_merge_then_the_one_pass_tail(dev):
    """rescale=(1, 2): the depth stacks of two sessions, merged per view on the device, fused at the finer grid with the first session's images
    (ratio 2) and cameras"""
    from cer_mvs_amd import fusion
    from cer_mvs_amd.multires import merge
    from cer_mvs_amd.scan import ScanSession, reconstruct_scan
    images, poses, intr, scales = _scan(128, 160)
    model = _model(dev)
    stacks = []
    for s in (1, 2):
        sess = ScanSession(model, images, poses, intr, rescale=s, streams=2)
        try:
            stacks.append(sess.depths(PAIRS, scales, num_frames=NF))
            if s == 1:
                colors = fusion.color_grid(sess.prepared, 64, 80)
                K = torch.stack([fusion.modify_camera_parameters(sess.intrinsics[i].clone(), 0.5, 0, 0) for i in range(M)])
                torch.cuda.synchronize()
        finally:
            sess.close()
    assert tuple(stacks[0].shape) == (M, 32, 40) and tuple(stacks[1].shape) == (M, 64, 80)
    depths = torch.stack([merge(stacks[0][i], stacks[1][i], th=0.02) for i in range(M)])
    fpairs = [(i, PAIRS[i][:NF]) for i in range(M)]
    masks, est, thre, hist = fusion.fuse_depth_maps(depths, K, poses.float(), fpairs, glb=0.25)
    xyz, rgb = fusion.point_cloud(masks, est, K, poses.float(), colors, list(range(M)))
    out = reconstruct_scan(model, images, poses, intr, NAMES, PAIRS, scales, None, rescale=(1, 2), num_frames=NF, streams=2, write=False)
    assert np.array_equal(out["masks"], masks.cpu().numpy().astype(bool)) and out["threshold"] == thre and out["history"] == hist
    assert np.array_equal(out["depth_est"].view(np.uint32), est.cpu().numpy().view(np.uint32))
    assert len(out["xyz"]) == len(xyz) > 0
    assert np.array_equal(out["xyz"].view(np.uint32), xyz.cpu().numpy().view(np.uint32)) and np.array_equal(out["rgb"], rgb.cpu().numpy())
    with pytest.raises(ValueError, match="two-pass"):
        reconstruct_scan(model, images, poses, intr, NAMES, PAIRS, scales, None, rescale=(1, 3), write=False)
    with pytest.raises(ValueError, match="no crop"):
        reconstruct_scan(model, images, poses, intr, NAMES, PAIRS, scales, None, rescale=(1, 2), crop=(64, 96), write=False)


def test_saturation_leaves_no_files_behind(dev, tmp_path):
    """the sticky overflow flag raised the way tests/test_hip_parity.py::test_s16_saturation_raises_the_overflow_flag raises it (a frag16 activation
    beyond the split-f16 range, found by the scan: a defined, flagged clamp): reconstruct_scan raises SaturationError and writes neither a PLY nor a PFM"""
    from cer_mvs_amd import _lib as L, ops
    from cer_mvs_amd.raft import SaturationError
    from cer_mvs_amd.scan import reconstruct_scan
    images, poses, intr, scales = _scan(128, 160)
    model = _model(dev)
    ops.check_overflow(dev)
    x = torch.zeros(16 * 32, 64, device=dev)
    x[5, 7] = 5000.0
    ops.scan_overflow(ops.to_frag16(x, 16, 32, L.S16_RELU))
    try:
        with pytest.raises(SaturationError):
            reconstruct_scan(model, images, poses, intr, NAMES, PAIRS, scales, tmp_path / "out", num_frames=NF, streams=3, write_depths=True)
    finally:
        torch.cuda.synchronize()                             # (snapshots of the forwards that were in flight have landed: drain them)
        ops.check_overflow(dev)                              # (leave the flag clear for whoever runs next)
        ops.overflow_poll(dev)
    left = [p for p in (tmp_path / "out").rglob("*") if p.is_file()] if (tmp_path / "out").exists() else []
    assert left == []
    # and the same call on a clear flag does write them
    out = reconstruct_scan(model, images, poses, intr, NAMES, PAIRS, scales, tmp_path / "out", num_frames=NF, streams=3, write_depths=True)
    assert (tmp_path / "out" / "result.ply").exists() and len(list((tmp_path / "out" / "depths").glob("*.pfm"))) == M
    assert len(out["xyz"]) == int(out["masks"].sum())
