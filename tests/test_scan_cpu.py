"""Scan session (cer-mvs_amd/scan.py), the parts that need no GPU: the resident footprint, the intrinsics of the prepared images, the
resize / crop window arithmetic, the C ABI of csrc/scan_ops.hip and the instruction-form guard on the library that carries it."""
import os
import sys

import pytest
import torch

from conftest import REPO


def test_bytes_needed_matches_hand_computed_figures():
    from cer_mvs_amd.scan import ScanSession
    # DTU: 49 images of 1600x1184 -> 400x296 feature grid, bordered 404x300
    images = 49 * 3 * 1184 * 1600 * 4                    # fp32 CHW
    store = 49 * 300 * 404 * 128 * 2                     # f16 hi|lo planes of 64 channels
    assert images == 1_113_907_200 and store == 1_520_332_800
    assert ScanSession.bytes_needed(49, 1184, 1600) == images + store
    # one block is the 31 MB per image the store costs at DTU size
    assert ScanSession.bytes_needed(1, 1184, 1600) - 3 * 1184 * 1600 * 4 == 31_027_200
    # a small odd-ish grid: 6 images of 256x320 -> 64x80, bordered 68x84
    assert ScanSession.bytes_needed(6, 256, 320) == 6 * (3 * 256 * 320 * 4 + 68 * 84 * 256)
    # linear in M
    assert ScanSession.bytes_needed(300, 1080, 1920) == 300 * ScanSession.bytes_needed(1, 1080, 1920)


@pytest.mark.parametrize("rescale,crop", [(1, None), (2, None), (0.5, None), (1.37, None), (1, (64, 88)), (2, (128, 160)),
                                          (0.5, (32, 44)), (1.37, (88, 120)), (2, (133, 177))])
def test_intrinsics_match_scale_and_crop_operation(rescale, crop):
    """exactly the reference driver's arithmetic: rows 0 and 1 times s, then the principal point minus the window origin"""
    from cer_mvs_amd.inference import crop_operation, scale_operation
    from cer_mvs_amd.scan import scan_intrinsics
    H0, W0, M = 67, 93, 5
    g = torch.Generator().manual_seed(3)
    K = torch.zeros(M, 3, 3)
    K[:, 0, 0] = 2890.0 + 10 * torch.rand(M, generator=g)
    K[:, 1, 1] = 2887.0 + 10 * torch.rand(M, generator=g)
    K[:, 0, 2] = W0 / 2 + torch.rand(M, generator=g)
    K[:, 1, 2] = H0 / 2 + torch.rand(M, generator=g)
    K[:, 0, 1] = 0.01 * torch.rand(M, generator=g)       # (a skew term is scaled with its row)
    K[:, 2, 2] = 1.0
    images = torch.rand(M, 3, H0, W0, generator=g) * 255
    keep = K.clone()
    im2, want = scale_operation(images, K, rescale)
    if crop is not None:
        im2, want = crop_operation(im2, want, crop[0], crop[1])
    got = scan_intrinsics(K, H0, W0, rescale, crop)
    assert torch.equal(K, keep)                          # out of place
    assert torch.equal(got, want)
    from cer_mvs_amd.ops import prep_geometry
    assert prep_geometry(H0, W0, rescale, crop)[4:] == tuple(im2.shape[2:])


def test_prep_geometry_truncation_and_odd_windows():
    from cer_mvs_amd.ops import prep_geometry
    # int(s * H) truncates: 1.37 * 67 = 91.79, 1.37 * 93 = 127.41
    assert prep_geometry(67, 93, 1.37) == (91, 127, 0, 0, 91, 127)
    assert prep_geometry(67, 93, 0.5) == (33, 46, 0, 0, 33, 46)
    assert prep_geometry(67, 93, 2) == (134, 186, 0, 0, 134, 186)
    assert prep_geometry(1200, 1600, 1, (1184, 1600)) == (1200, 1600, 8, 0, 1184, 1600)
    # odd differences round the origin down ((H2 - crop_h) // 2), as the reference's crop does
    assert prep_geometry(67, 93, 1, (64, 88)) == (67, 93, 1, 2, 64, 88)
    assert prep_geometry(67, 93, 1.37, (88, 120)) == (91, 127, 1, 3, 88, 120)
    assert prep_geometry(67, 93, 2, (133, 177)) == (134, 186, 0, 4, 133, 177)
    # the whole image as the window
    assert prep_geometry(67, 93, 1, (67, 93)) == (67, 93, 0, 0, 67, 93)
    for bad in ((68, 93), (67, 94), (0, 8)):
        with pytest.raises(ValueError):
            prep_geometry(67, 93, 1, bad)
    with pytest.raises(ValueError):
        prep_geometry(3, 3, 0.2)


def test_scan_abi_symbols_are_declared():
    from cer_mvs_amd import _lib as L
    names = L.exported_symbols()
    for n in ("cer_image_prep_u8", "cer_image_prep_f32", "cer_feat_ref_rows_f16"):
        assert n in names
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P      # int f(..., stream)
    assert L.ABI_VERSION >= 1090
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    for n in ("cer_image_prep_u8", "cer_image_prep_f32", "cer_feat_ref_rows_f16"):
        assert f"int {n}(" in hdr
    lib = L.load()                                        # (loads without a GPU; refuses a library that lacks a declared symbol)
    assert lib.cer_abi_version() == L.ABI_VERSION


def test_scan_entry_points_refuse_bad_arguments():
    """argument checks run before any launch: null pointers, a crop window outside the resized image, misaligned planes"""
    import ctypes
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, odd, null = ctypes.c_void_p(4096), ctypes.c_void_p(4100), None
    assert lib.cer_image_prep_f32(null, fake, 8, 8, 8, 8, 0, 0, 8, 8, null) == -1
    assert lib.cer_image_prep_u8(fake, null, 8, 8, 8, 8, 0, 0, 8, 8, 0, null) == -1
    assert lib.cer_image_prep_f32(fake, fake, 8, 8, 16, 16, 9, 0, 8, 8, null) == -1       # rows 9 .. 16 of a 16-row image
    assert lib.cer_image_prep_f32(fake, fake, 8, 8, 16, 16, 0, -1, 8, 8, null) == -1
    assert lib.cer_image_prep_u8(fake, fake, 8, 8, 4, 4, 0, 0, 4, 5, 0, null) == -1       # window wider than the resized image
    assert lib.cer_image_prep_f32(fake, odd, 8, 8, 8, 8, 0, 0, 8, 8, null) == -3          # 16-byte stores need an aligned plane
    assert lib.cer_feat_ref_rows_f16(null, fake, 4, 4, 2, null) == -1
    assert lib.cer_feat_ref_rows_f16(fake, fake, 0, 4, 2, null) == -1
    assert lib.cer_feat_ref_rows_f16(fake, odd, 4, 4, 2, null) == -3


def test_library_with_scan_kernels_passes_the_isa_guard():
    """the library that now carries csrc/scan_ops.hip holds none of the packed-fp32 forms tools/check_isa.py refuses (scanned here when the
    disassembler is at hand, else the record of build()'s scan must match these bytes)"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_isa
    from cer_mvs_amd import _lib as L
    lib = L.LIB_PATH
    assert os.path.exists(lib)
    if check_isa.have_objdump():
        ncos, n, hits = check_isa.scan(lib)
        assert ncos >= 1 and not hits, hits[:5]
    else:
        assert check_isa.verify_sidecar(lib)
    mk = open(os.path.join(REPO, "cer-mvs_amd", "csrc", "Makefile")).read()
    assert "scan_ops.hip" in mk


def test_session_refuses_what_it_cannot_hold_or_run():
    """constructor checks that come before any device work"""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.scan import ScanSession
    model = RAFT(test_mode=True)                          # on the CPU: there is no CPU path
    imgs = [torch.zeros(3, 64, 96) for _ in range(3)]
    with pytest.raises(RuntimeError, match="GPU"):
        ScanSession(model, imgs, torch.eye(4).repeat(3, 1, 1), torch.eye(3).repeat(3, 1, 1))
    with pytest.raises(RuntimeError, match="test_mode"):
        ScanSession(RAFT(test_mode=False), imgs, torch.eye(4).repeat(3, 1, 1), torch.eye(3).repeat(3, 1, 1))
