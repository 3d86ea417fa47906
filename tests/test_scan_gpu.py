"""Scan session on the GPU (cer-mvs_amd/scan.py, csrc/scan_ops.hip): image preparation against F.interpolate + centre crop, the feature
store against the per-stack feature head, ``ScanSession.depth`` against ``RAFT.forward`` on the gathered stack (bit for bit), launch
accounting, the fallback, ``inference_scan`` against ``inference()``, calibration and determinism.  Synthetic scenes and hashed weights;
the arithmetic form is pinned unless a case says otherwise."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import cached_scene, rel_l1

pytestmark = pytest.mark.gpu

CASCADE = [(64, 64, 3), (-1, 320, 3)]
PAIRS6 = {0: [3, 1, 5, 2], 2: [5, 0, 4, 1], 5: [1, 4, 0, 3]}          # reference view -> source views, not monotonic


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _model(dev, pinned=True, cascade=CASCADE, **kw):
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict
    if pinned:
        kw = dict(gru_precision="s16f8", enc_precision="f16x3", cost_precision="x3", **kw)
    m = RAFT(cascade=cascade, test_mode=True, **kw)
    m.load_state_dict(fill_state_dict(m.state_dict(), seed=9))
    return m.to(dev).eval()


def _scan(H, W, M=6, seed=4):
    images, poses, intr, scale = cached_scene(H, W, M - 1, seed)
    return images[0], poses[0], intr[0], scale


def _reference(model, sess, ref, srcs, scale):
    idx = [ref] + list(srcs)
    with torch.no_grad():
        return model(sess.stack(ref, srcs), sess.poses[idx][None], sess.intrinsics[idx][None], scale=scale)


# ---------------------------------------------------------------- 1. image preparation
def _prep_reference(img_chw, rescale, crop):
    from cer_mvs_amd.ops import prep_geometry
    H2, W2, y0, x0, H, W = prep_geometry(img_chw.shape[1], img_chw.shape[2], rescale, crop)
    r = F.interpolate(img_chw[None], [H2, W2], mode="bilinear", align_corners=True)[0]
    return r[:, y0:y0 + H, x0:x0 + W]


@pytest.mark.parametrize("form", ["f32", "u8", "u8bgr"])
@pytest.mark.parametrize("rescale,crop", [(1, None), (2, None), (0.5, None), (1.37, None), (1, (64, 88)), (2, (133, 177)), (0.5, (32, 44)),
                                          (1.37, (88, 120))])
def test_image_prep_matches_interpolate_and_crop(dev, form, rescale, crop):
    """scale_operation + crop_operation in one pass: relative L1 <= 1e-6 from F.interpolate(bilinear, align_corners=True) + centre crop
    (the bar tests/test_train_step_gpu.py sets for the same operation), exact copy at s == 1, the same bits on every launch"""
    from cer_mvs_amd import ops
    images, _, _, _ = _scan(67, 93, M=3, seed=11)            # odd sizes
    img = images[1].contiguous()                             # [3,67,93] floats 0..255
    if form == "f32":
        src, chw = img.to(dev), img
    else:
        u8 = img.round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()        # HWC, as an image reader returns it
        src = u8.to(dev)
        chw = u8.permute(2, 0, 1).float()
        if form == "u8bgr":
            chw = chw.flip(0)
    want = _prep_reference(chw, rescale, crop)
    outs = [ops.image_prep(src, rescale, crop, bgr=form == "u8bgr") for _ in range(3)]
    assert tuple(outs[0].shape) == tuple(want.shape)
    err = rel_l1(outs[0].cpu(), want)
    print(f"image_prep {form} s={rescale} crop={crop}: rel_l1 = {err:.3e}")
    assert err <= 1e-6
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    if rescale == 1:
        assert torch.equal(outs[0].cpu(), want)              # no interpolation arithmetic at equal sizes
    # into a slice of a larger buffer (the session's [M,3,H,W])
    buf = torch.full((2,) + tuple(want.shape), -1.0, device=dev)
    ops.image_prep(src, rescale, crop, out=buf[1], bgr=form == "u8bgr")
    assert torch.equal(buf[1], outs[0]) and bool((buf[0] == -1).all())


# ---------------------------------------------------------------- 2. feature store
@pytest.mark.parametrize("size", [(64, 96), (100, 148)])
def test_store_blocks_and_ref_rows_match_the_feature_head(dev, size):
    """block i of a store filled in batches of 1, 3 and 4 == the src_split block of a one-stack call; the interior of a bordered block ==
    the plain map the head writes for a reference view (border 0 and border 2 of the 1x1 head give the same bits)"""
    from cer_mvs_amd import ops
    H, W = size
    images, _, _, _ = _scan(H, W, M=6, seed=5)
    x = images.to(dev)
    m = _model(dev)
    eng_f = m._get_engines(dev)[1]
    assert eng_f.supports_split_head()
    h, w = H // 4, W // 4
    Pb = (h + 4) * (w + 4)
    flag = ops.overflow_flag(dev)
    ref_split = torch.empty(h * w, 128, device=dev, dtype=torch.float16)
    src_split = torch.zeros(5, Pb, 128, device=dev, dtype=torch.float16)
    eng_f.features_split(x, ref_split, src_split, n_ref=1, border=2, scale=0.125, raw=True, flag=flag)
    for batch in (1, 3, 4):
        store = torch.zeros(6, Pb, 128, device=dev, dtype=torch.float16)
        for i0 in range(0, 6, batch):
            i1 = min(6, i0 + batch)
            eng_f.features_split(x[i0:i1], None, store[i0:i1], n_ref=0, border=2, scale=0.125, raw=True, flag=flag)
        assert torch.equal(store[1:], src_split), f"batch {batch}"
        rows = ops.feat_ref_rows(store[0], h, w, border=2)
        assert torch.equal(rows, ref_split), f"batch {batch}"
    # every block's interior equals its own plain head
    for i in (2, 5):
        own = torch.empty(h * w, 128, device=dev, dtype=torch.float16)
        eng_f.features_split(x[i:i + 1], own, None, n_ref=1, border=2, scale=0.125, raw=True, flag=flag)
        assert torch.equal(ops.feat_ref_rows(store[i], h, w), own)
    assert ops.check_overflow(dev) == 0


# ---------------------------------------------------------------- 3. the central test
@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("size", [(256, 320), (1184, 1600)], ids=["256x320", "1184x1600"])
def test_depth_equals_forward_on_the_gathered_stack(dev, size, streams):
    """ScanSession.depth(ref, srcs, scale) is torch.equal to model(stack, poses[idx], intrinsics'[idx], scale) - the per-image encoders, the slot
    indirection and the stage loop are the same code on the same bits"""
    from cer_mvs_amd.scan import ScanSession
    H, W = size
    images, poses, intr, scale = _scan(H, W)
    model = _model(dev)
    plain = copy.deepcopy(model)
    sess = ScanSession(model, images, poses, intr, streams=streams, encode_batch=4)
    try:
        assert sess.cached is True and len(sess) == streams
        assert tuple(sess.prepared.shape) == (6, 3, H, W) and torch.equal(sess.prepared.cpu(), images)
        for rnd in range(2):                                 # (second round: every replica has run, buffers are reused)
            for ref, srcs in PAIRS6.items():
                got = sess.depth(ref, srcs, scale)
                want = _reference(plain, sess, ref, srcs, scale)
                assert got.shape == want.shape == (1, 1, H // 4, W // 4)
                assert torch.isfinite(got).all() and float(got.abs().sum()) > 0
                assert torch.equal(got, want), f"ref {ref} round {rnd}: max diff {float((got - want).abs().max()):.3e}"
        assert model.check_overflow(dev, raise_error=False) == 0
    finally:
        sess.close()


def test_depth_equals_forward_with_rescale_and_crop(dev):
    """the same identity on uint8 input prepared with a resize and a crop (the stack is gathered from the session's prepared images)"""
    from cer_mvs_amd.scan import ScanSession
    images, poses, intr, scale = _scan(100, 132)
    u8 = images.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    model = _model(dev)
    plain = copy.deepcopy(model)
    sess = ScanSession(model, u8, poses, intr, rescale=2, crop=(192, 256), streams=2, encode_batch=3)
    try:
        assert sess.cached and tuple(sess.prepared.shape) == (6, 3, 192, 256)
        for ref, srcs in PAIRS6.items():
            assert torch.equal(sess.depth(ref, srcs, scale), _reference(plain, sess, ref, srcs, scale))
    finally:
        sess.close()


# ---------------------------------------------------------------- 4. launch accounting
ENCODER_ENTRY_POINTS = ("cer_enc_stem_s16", "cer_enc_stem_f32", "cer_enc_pc_conv", "cer_enc_conv_f16x3", "cer_enc_merge_f32", "cer_feat_split_f16")


def _encoder_calls(records):
    names = [r[0] for r in records]
    return {n: names.count(n) for n in ENCODER_ENTRY_POINTS}


def test_depth_launches_no_fnet(dev):
    """library calls of one depth map (_lib.timing: the recorder that stays active under the GRU loop's own _lib.recording, which does
    not nest): the stem and the producer / consumer encoder entry points are called exactly as often as cnet alone calls them"""
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd.scan import ScanSession
    images, poses, intr, scale = _scan(256, 320)
    model = _model(dev)
    plain = copy.deepcopy(model)
    sess = ScanSession(model, images, poses, intr, streams=1)
    try:
        sess.depth(0, PAIRS6[0], scale)                      # (warm: loop objects, launch plans)
        _reference(plain, sess, 0, PAIRS6[0], scale)
        torch.cuda.synchronize()
        rec_ctx, rec_depth, rec_fwd = [], [], []
        with L.timing(rec_ctx), torch.no_grad():
            model._get_engines(dev)[2].context(sess.prepared[0:1], raw=True)
        with L.timing(rec_depth):
            sess.depth(2, PAIRS6[2], scale)
        with L.timing(rec_fwd):
            _reference(plain, sess, 2, PAIRS6[2], scale)
        torch.cuda.synchronize()
        ctx, dep, fwd = _encoder_calls(rec_ctx), _encoder_calls(rec_depth), _encoder_calls(rec_fwd)
        assert ctx["cer_enc_stem_s16"] + ctx["cer_enc_stem_f32"] == 1 and ctx["cer_enc_pc_conv"] > 0
        assert dep == ctx, (dep, ctx)
        assert fwd["cer_enc_pc_conv"] > ctx["cer_enc_pc_conv"]           # (the ordinary forward does run fnet)
        assert [r[0] for r in rec_depth].count("cer_feat_ref_rows_f16") == 1
        # apart from the encoders, the cached forward makes the ordinary forward's calls in the ordinary forward's order
        skip = set(ENCODER_ENTRY_POINTS) | {"cer_enc_stats_reduce_f32", "cer_feat_ref_rows_f16"}
        assert [r[0] for r in rec_depth if r[0] not in skip] == [r[0] for r in rec_fwd if r[0] not in skip]
        assert sess.cached is True
    finally:
        sess.close()


# ---------------------------------------------------------------- 5. fallback
@pytest.mark.parametrize("why", ["LR", "walk", "forced"])
def test_fallback_runs_the_ordinary_forward(dev, why):
    """where the cached path cannot apply the session reports cached == False and hands gathered stacks to the ordinary forward: "LR" encoders,
    the fp32 cost-volume walk (cer_cost_build_algo 1), or on request"""
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd.scan import ScanSession
    images, poses, intr, scale = _scan(256, 320)
    model = _model(dev, encoder_type="LR") if why == "LR" else _model(dev)
    plain = copy.deepcopy(model)
    algo = L.load().cer_cost_build_algo(1) if why == "walk" else None
    try:
        sess = ScanSession(model, images, poses, intr, streams=2, force_uncached=why == "forced")
        try:
            assert sess.cached is False and sess.store is None
            for ref, srcs in PAIRS6.items():
                got = sess.depth(ref, srcs, scale)
                assert torch.isfinite(got).all()
                want = _reference(plain, sess, ref, srcs, scale)
                if why == "LR":
                    # the "LR" encoders run PyTorch-ROCm (MIOpen) convolutions, which do not repeat bit for bit: measured here, the SAME model on
                    # the SAME stack twice differs by 5.7e-6 in its feature maps and 1.1e-9 in the disparity, and the session differs from it
                    # by the same 1.1e-9.  Bit identity cannot be asked of this case (the "walk" and "forced" cases carry it); the project's
                    # parity bar on depth can
                    assert rel_l1(got.cpu(), want.cpu()) <= 1e-4
                else:
                    assert torch.equal(got, want)
        finally:
            sess.close()
    finally:
        if algo is not None:
            L.load().cer_cost_build_algo(algo)


# ---------------------------------------------------------------- 6. inference_scan against inference()
def _read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, sc, data = raw.split(b"\n", 3)
    assert head == b"Pf" and float(sc) < 0
    w, h = (int(v) for v in dims.split())
    return np.flipud(np.frombuffer(data, dtype="<f4").reshape(h, w))


def _list_loader(images, poses, intr, names, pairs, scales):
    """what the reference's loader yields, one reference view at a time, backed by the scan's arrays"""
    for i in range(len(names)):
        idx = [i] + list(pairs[i])
        yield images[idx][None].clone(), poses[idx][None].clone(), intr[idx][None].clone(), [names[i]], scales[i]


@pytest.mark.parametrize("rescale,crop", [(1, None), (2, (184, 248))], ids=["s1", "s2crop"])
def test_inference_scan_writes_what_inference_writes(dev, tmp_path, rescale, crop):
    """rescale 1, no crop: byte-identical PFM files.  rescale 2 + crop: the resize runs on the device instead of in F.interpolate on the host -
    relative L1 of the depth <= 1e-4 (the project's parity bar on depth), every pixel of every view counted"""
    from cer_mvs_amd.inference import inference
    from cer_mvs_amd.scan import inference_scan
    images, poses, intr, scale = _scan(96, 128)
    M = 6
    names = [f"{i:08d}" for i in range(M)]
    pairs = [[(i + d) % M for d in (2, 5, 1, 3)] for i in range(M)]
    scales = [scale * (1.0 + 0.01 * i) for i in range(M)]
    model = _model(dev)
    plain = copy.deepcopy(model)
    a = inference(_list_loader(images, poses, intr, names, pairs, scales), None, tmp_path / "a", rescale=rescale, crop=crop, model=plain,
                  num_frames=4, streams=3, write_min_depth=tmp_path / "a_min")
    tm = {}
    b = inference_scan(model, images, poses, intr, names, pairs, scales, tmp_path / "b", rescale=rescale, crop=crop, num_frames=4, streams=3,
                       write_min_depth=tmp_path / "b_min", timings=tm)
    assert tm["cached"] is True and "encode_s" in tm and "upload_prep_s" in tm
    assert len(a) == len(b) == M
    for pa, pb, name in zip(a, b, names):
        assert pa.endswith(f"{name}_scale{rescale}_nf4.pfm") and pb.endswith(f"{name}_scale{rescale}_nf4.pfm")
        if rescale == 1:
            assert open(pa, "rb").read() == open(pb, "rb").read(), name
            assert open(tmp_path / "a_min" / f"{name}.txt").read() == open(tmp_path / "b_min" / f"{name}.txt").read()
        else:
            da, db = _read_pfm(pa), _read_pfm(pb)
            assert da.shape == db.shape == (crop[0] // 4, crop[1] // 4)
            err = rel_l1(db.copy(), da.copy())
            print(f"inference_scan s={rescale} crop={crop} view {name}: depth rel_l1 = {err:.3e}")
            assert err <= 1e-4, (name, err)


# ---------------------------------------------------------------- 7. calibration
@pytest.mark.parametrize("streams", [1, 3])
def test_auto_calibration_ends_where_a_plain_model_ends(dev, streams):
    """gru_precision="auto", calibration pending: the session feeds the ordinary forward until the form is decided, then encodes the store in
    that form; the decision and every depth map equal a plain model's on the same stacks in the same order"""
    from cer_mvs_amd.scan import ScanSession
    images, poses, intr, scale = _scan(128, 160)
    model = _model(dev, pinned=False)
    assert model.gru_precision == "auto" and model._auto_pending()
    plain = copy.deepcopy(model)
    sess = ScanSession(model, images, poses, intr, streams=streams)
    try:
        assert sess.cached and sess.store is None            # nothing is encoded before the encoders' form is known
        order = [0, 2, 5, 0, 5, 2, 0, 2]
        for n, ref in enumerate(order):
            got = sess.depth(ref, PAIRS6[ref], scale)
            want = _reference(plain, sess, ref, PAIRS6[ref], scale)
            assert torch.equal(got, want), f"depth map {n}"
        assert not model._auto_pending() and not plain._auto_pending()
        assert model.auto_choice == plain.auto_choice and model.auto_choice is not None
        assert bool(model._enc_f6) == bool(plain._enc_f6) and bool(model._cost_x2) == bool(plain._cost_x2)
        for m in sess.pipe.models[1:]:
            assert m.auto_choice == plain.auto_choice and bool(m._enc_f6) == bool(plain._enc_f6)
        assert sess.store is not None and sess._store_key == sess._key()
    finally:
        sess.close()


def test_store_follows_new_weights(dev):
    """parameters changed in place + refresh_weights: the store is keyed on the parameter signature and is encoded again"""
    from cer_mvs_amd.scan import ScanSession
    from cer_mvs_amd.synthetic import fill_state_dict
    images, poses, intr, scale = _scan(128, 160)
    model = _model(dev)
    sess = ScanSession(model, images, poses, intr, streams=2)
    try:
        first = sess.depth(0, PAIRS6[0], scale).clone()
        key = sess._store_key
        model.load_state_dict(fill_state_dict(model.state_dict(), seed=21))
        sess.refresh_weights()
        plain = copy.deepcopy(model)
        for ref in (0, 2, 5):
            assert torch.equal(sess.depth(ref, PAIRS6[ref], scale), _reference(plain, sess, ref, PAIRS6[ref], scale))
        assert sess._store_key != key
        assert not torch.equal(sess.depth(0, PAIRS6[0], scale), first)
    finally:
        sess.close()


def test_session_refuses_a_scan_beyond_max_bytes(dev):
    from cer_mvs_amd.scan import ScanSession
    images, poses, intr, scale = _scan(128, 160)
    need = ScanSession.bytes_needed(6, 128, 160)
    with pytest.raises(MemoryError, match=str(need)):
        ScanSession(_model(dev), images, poses, intr, max_bytes=need - 1)


# ---------------------------------------------------------------- 8. determinism
def test_same_depth_map_twenty_times_over_three_streams(dev):
    from cer_mvs_amd.scan import ScanSession
    images, poses, intr, scale = _scan(256, 320)
    sess = ScanSession(_model(dev), images, poses, intr, streams=3)
    try:
        handles = []
        for n in range(20):
            handles.append((2, sess.submit(2, PAIRS6[2], scale)))
            other = (0, 5)[n % 2]
            handles.append((other, sess.submit(other, PAIRS6[other], scale)))
            if n % 3 == 0:                                   # (shifts which replica the target lands on)
                handles.append((0, sess.submit(0, PAIRS6[0], scale)))
        first = {}
        for ref, hd in handles:
            out = sess.result(hd)
            if ref not in first:
                first[ref] = out.clone()
                assert torch.isfinite(out).all()
            assert torch.equal(out, first[ref]), f"reference view {ref}"
        assert sum(1 for r, _ in handles if r == 2) == 20
        assert sess.check_overflow(raise_error=False) == 0
    finally:
        sess.close()
