"""Greedy radius thinning (csrc/cloud_eval.hip grid_thin_round_kernel, cer-mvs_amd/cloud_eval.py radius_thin), the parts that need no
GPU: the two entry points of ABI 1120 and their argument checks, and the argument checks of the Python layer."""
import ctypes
import os

import pytest
import torch

from conftest import REPO

THIN_SYMBOLS = ("cer_grid_thin_round_f32", "cer_grid_thin_compact_i32")
BIG = 1 << 31


def test_thin_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    names = L.exported_symbols()
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    for n in THIN_SYMBOLS:
        assert n in names
        assert f"int {n}(" in hdr
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P      # int f(..., stream)
    assert L.ABI_VERSION >= 1120
    lib = L.load()                                        # (loads without a GPU; refuses a library that lacks a declared symbol)
    assert lib.cer_abi_version() == L.ABI_VERSION
    assert "ABI 1120" in hdr


def test_thin_entry_points_refuse_bad_arguments():
    """argument checks run before any launch (the pointers are fake: a launch would fault): negative sizes and null pointers CER_EINVAL, sizes
    of 2^31 and beyond CER_ESHAPE, empty inputs succeed with nothing launched"""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    o = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    o_nan = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    no_o = ctypes.POINTER(ctypes.c_double)()

    def rnd(n=8, nc=3, na=5, rec=fake, ck=fake, cs=fake, org=o, cell=0.5, act=fake, radius=1.0, st=fake):
        return lib.cer_grid_thin_round_f32(rec, n, ck, cs, nc, org, cell, act, na, radius, st, null)
    assert rnd(n=-1) == -1 and rnd(na=-1) == -1 and rnd(nc=-1) == -1
    assert rnd(n=BIG) == -2 and rnd(na=BIG) == -2 and rnd(nc=BIG) == -2
    assert rnd(nc=9) == -2 and rnd(na=9) == -2                                    # more cells / more active entries than records
    assert rnd(na=0) == 0 and rnd(na=0, rec=null, st=null) == 0 and rnd(n=0, nc=0, na=0) == 0 and rnd(nc=0) == 0
    assert rnd(rec=null) == -1 and rnd(ck=null) == -1 and rnd(cs=null) == -1 and rnd(st=null) == -1
    assert rnd(org=no_o) == -1 and rnd(org=o_nan) == -1 and rnd(cell=0.0) == -1 and rnd(cell=float("nan")) == -1
    assert rnd(radius=0.0) == -1 and rnd(radius=-1.0) == -1 and rnd(radius=float("nan")) == -1 and rnd(radius=float("inf")) == -1
    assert rnd(radius=5000.0, cell=1.0) == -2                                     # more rings than the walk enumerates
    assert rnd(rec=ctypes.c_void_p(4104)) == -3

    def cmp(n=8, na=5, rec=fake, st=fake, act=fake, part=fake, off=fake, out=ctypes.c_void_p(8192), tot=fake):
        return lib.cer_grid_thin_compact_i32(rec, n, st, act, na, part, off, out, tot, null)
    assert cmp(n=-1) == -1 and cmp(na=-1) == -1 and cmp(n=BIG) == -2 and cmp(na=BIG) == -2 and cmp(na=9) == -2
    assert cmp(na=0) == 0 and cmp(na=0, rec=null, out=null) == 0 and cmp(n=0, na=0) == 0
    assert cmp(rec=null) == -1 and cmp(st=null) == -1 and cmp(part=null) == -1 and cmp(off=null) == -1 and cmp(out=null) == -1
    assert cmp(tot=null) == -1
    assert cmp(out=fake) == -1                                                    # the new list may not be the old one
    assert cmp(rec=ctypes.c_void_p(4104)) == -3


def test_radius_thin_refuses_bad_arguments():
    from cer_mvs_amd import cloud_eval as CE
    p = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.radius_thin(p, 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.radius_thin(p, 0.1, order="index")
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.radius_thin(p, 0.1, order=torch.arange(4))
    with pytest.raises(RuntimeError):                                             # (a float32 message needs a CUDA tensor: test_cloud_thin_gpu.py)
        CE.radius_thin(p.double(), 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.accuracy_completeness(p, p, thin=0.1, thin_method="greedy")
    for radius in (0.0, -1.0, float("nan"), float("inf"), 1e-50):                 # (1e-50 is 0 in float32)
        with pytest.raises(ValueError, match="radius"):
            CE.radius_thin(p, radius)
    for order in ("zigzag", "", None, [0, 1, 2, 3], torch.arange(4, dtype=torch.int32), torch.arange(4.0), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="order"):
            CE.radius_thin(p, 0.1, order=order)
    with pytest.raises(ValueError, match="max_rounds"):
        CE.radius_thin(p, 0.1, max_rounds=0)
    with pytest.raises(ValueError, match="thin_method"):
        CE.accuracy_completeness(p, p, thin=0.1, thin_method="matlab")
    with pytest.raises(ValueError, match="thin_method"):
        CE.accuracy_completeness(p, p, thin_method="matlab")
    assert CE.THIN_ROUNDS_PER_COMPACTION >= 1
