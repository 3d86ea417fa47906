"""Saturation is never silent, the part that needs no GPU: the census of clamp sites (tests/saturation_cases.py) against the product
sources, the thresholds restated in numpy, and which failures the multi-process tests' ``_spawn`` retries."""
import os

import numpy as np
import pytest

from conftest import REPO
import saturation_cases as S

CSRC = os.path.join(REPO, "cer-mvs_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the census is binding
def test_census_accounts_for_every_clamp_line():
    """Per product source file (csrc/*.hip, *.hpp, not experimental/): the number of lines holding the literal 65504 - the clamp constant
    itself, nothing else is searched for - equals what the census records for that file."""
    found, listed = S.source_lines(CSRC), S.census_lines()
    assert found == listed, (
        f"lines holding the literal 65504 per source file {found} differ from what tests/saturation_cases.py accounts for {listed}: a clamp "
        "to the f16 range cannot be added (or removed) without a census row that says who reports it (DESIGN.md 3f)")


def test_census_rows_are_complete():
    for r in S.CENSUS:
        assert os.path.exists(os.path.join(CSRC, r["file"])), r["file"]
        assert r["reporter"] in ("kernel", "writer", "scan", "range", "nobody", "users"), r
        if r["reporter"] in ("kernel", "writer", "scan"):
            assert r["bit"] in (1, 2, 4, 8) and r["when"], r
        if r["reporter"] == "range":
            assert r["why"], r
        if r["reporter"] == "kernel":
            assert r["classes"] and r["lines"] >= 1, r
        if r["limit"] is not None and r["log2s"] is not None and r["reporter"] in ("kernel", "scan", "nobody"):
            assert r["limit"] * 2.0 ** r["log2s"] == S.F16_MAX, r                      # threshold in user units = 65504 / scale
    assert {r["bit"] for r in S.KERNEL_REPORTERS} == {1, 2, 4}


def test_bits_and_limit_match_the_product():
    """The names the model gives the bits, the fallback's mapping and CER_DISP_LIMIT are the ones restated here."""
    with open(os.path.join(REPO, "cer-mvs_amd", "raft.py")) as f:
        raft = f.read()
    what = raft[raft.index("_OVERFLOW_WHAT = {"):raft.index("def check_overflow")]
    for bit in (1, 2, 4, 8):
        assert f'{bit}: "' in what, bit
    assert 'if bits & 14 else mode' in raft                                                # bits 2, 4 and 8 send the fallback to f16x3
    with open(os.path.join(CSRC, "common.hpp")) as f:
        assert "#define CER_DISP_LIMIT 5.1175f" in f.read()


# ------------------------------------------------------------------------------------------------ the thresholds, restated
def test_frag16_rounding_at_scale_2_4():
    """hi becomes 0x7BFF exactly when v > 4093.0 (the tie at 65488 rounds to even); the value is clamped exactly when v > 4094.0."""
    assert S.hi_half(4093.0, 4) == 0x7BFE and S.hi_half(S.up(4093.0), 4) == 0x7BFF             # 65488: the tie goes to the even 65472
    assert S.hi_half(4094.0, 4) == 0x7BFF and S.hi_half(1e6, 4) == 0x7BFF and S.hi_half(np.inf, 4) == 0x7BFF
    assert not S.is_clamped(4094.0, 4) and S.is_clamped(S.up(4094.0), 4)
    rng = np.random.default_rng(0)
    for v in np.concatenate([rng.uniform(0, 4093.0, 2000), [4093.0, 0.0, 1000.0, 4000.0]]).astype(np.float32):
        assert not S.scan_hits(v, 4) and not S.is_clamped(v, 4), v                               # the clean side of every scan-based check
    for v in np.concatenate([rng.uniform(4094.0, 1e5, 2000), [5000.0, 2e4, 1e6, np.inf]]).astype(np.float32):
        if v > 4094.0:
            assert S.scan_hits(v, 4) and S.is_clamped(v, 4), v                                   # the flag side
    for v in np.linspace(4093.0, 4094.0, 50, dtype=np.float32)[1:]:
        assert S.scan_hits(v, 4) and not S.is_clamped(v, 4), v                                   # in between: reported by a scan, not clamped
    assert S.scan_hits(np.nan, 4) and S.scan_hits(-np.inf, 4)


def test_in_kernel_checks_are_exact():
    assert S.ACT_CLEAN == np.float32(4094.0) and S.ACT_FLAG > S.ACT_CLEAN and float(S.ACT_FLAG) - 4094.0 == 2.0 ** -12
    assert not S.is_clamped(S.ACT_CLEAN, 4) and S.is_clamped(S.ACT_FLAG, 4)
    assert not S.is_clamped(S.FEAT_CLEAN, 6) and S.is_clamped(S.FEAT_FLAG, 6) and not S.is_clamped(-S.FEAT_CLEAN, 6) and S.is_clamped(-S.FEAT_FLAG, 6)
    for v in (np.nan, np.inf, -np.inf):
        assert S.is_clamped(v, 4) and S.is_clamped(v, 6) and S.is_clamped(v, 0)
    # x * s <= 65504 exactly when x <= 65504 / s for a power-of-two s: the form the kernels compare in
    for log2s in (4, 6):
        lim = np.float32(S.F16_MAX) / np.float32(2.0 ** log2s)
        for v in (lim, S.up(lim), np.nextafter(lim, np.float32(0))):
            assert (np.float32(v) * np.float32(2.0 ** log2s) <= np.float32(S.F16_MAX)) == (v <= lim)


def test_disparity_limit_keeps_the_generated_features_below_the_clamp():
    """|d| <= CER_DISP_LIMIT for both ends of a difference: 100 * (d[q] - d[p]) * 2^6, formed in fp32 as the generators form it, stays
    within the f16 range - at the extreme pair exactly at 65504 - so bit 8 covers the generators' clamp; one ulp beyond is flagged."""
    d = np.float32(S.DISP_LIMIT)
    assert float(d) <= 5.1175
    diff = np.float32(d - np.float32(-d))
    feat = np.float32(np.float32(100.0) * diff) * np.float32(64.0)
    assert feat <= np.float32(S.F16_MAX), feat
    assert S.DISP_FLAG > d and not (abs(S.DISP_FLAG) <= d)
    assert 65504.0 / 6400.0 == 10.235 and 2 * 5.1175 == 10.235


def test_sweep_values_avoid_the_band():
    assert all(not (4093.0 < v <= 4094.0) for v in S.SWEEP) and any(v > 4094.0 for v in S.SWEEP) and any(v <= 4093.0 for v in S.SWEEP)


# ------------------------------------------------------------------------------------------------ _spawn retries the transport only
def _kinds():
    import torch.distributed as dist
    import torch.multiprocessing as mp
    raised = lambda text: mp.ProcessRaisedException(f"\n\n-- Process 1 terminated with the following error:\nTraceback ...\n{text}\n", 1, 4242)
    from cer_mvs_amd.raft import SaturationError
    return [
        ("DistNetworkError raised by the launcher", lambda mark: dist.DistNetworkError("connection reset"), True),
        ("DistBackendError in a worker", lambda mark: raised("torch.distributed.DistBackendError: gloo: connect failed"), True),
        ("DistNetworkError in a worker", lambda mark: raised("torch.distributed.DistNetworkError: address already in use"), True),
        ("a collective timed out", lambda mark: raised("RuntimeError: [../gloo/transport/tcp/unbound_buffer.cc:81] Timed out waiting; wait timed out"), True),
        ("exit inside init_process_group", lambda mark: (open(f"{mark}.1.begin", "w").close(), mp.ProcessExitedException("process 1 terminated with signal SIGKILL", 1, 4242, -9, signal_name="SIGKILL"))[1], True),
        ("exit after the rendezvous", lambda mark: (open(f"{mark}.0.begin", "w").close(), open(f"{mark}.0.done", "w").close(),
                                                      mp.ProcessExitedException("process 0 terminated with signal SIGSEGV", 0, 4242, -11, signal_name="SIGSEGV"))[2], False),
        ("exit of a worker without a process group", lambda mark: mp.ProcessExitedException("process 0 terminated with exit code 1", 0, 4242, 1), False),
        ("a worker's parity assert", lambda mark: raised("AssertionError: (1, 0.0031)"), False),
        ("an assert that quotes a transport error", lambda mark: raised("torch.distributed.DistNetworkError: quoted above\nAssertionError: rank 1 differs (the peer had timed out earlier)"), False),
        ("a worker's SaturationError", lambda mark: raised(f"cer_mvs_amd.raft.SaturationError: {SaturationError('a split-f16 kernel saturated an operand')}"), False),
        ("a plain RuntimeError", lambda mark: RuntimeError("HIP error: invalid device function"), False),
    ]


@pytest.mark.parametrize("idx", range(11))
def test_spawn_retries_only_transport_failures(monkeypatch, recwarn, idx):
    import test_multirank_gpu as M
    what, make, retried = _kinds()[idx]
    calls = []

    def fake_spawn(fn, args=(), nprocs=1, join=True):
        calls.append((args, os.environ.get(M._INIT_MARK)))
        if len(calls) == 1:
            raise make(os.environ[M._INIT_MARK])

    monkeypatch.setattr(M.mp, "spawn", fake_spawn)
    before = os.environ.get(M._INIT_MARK)
    args = (2, 23456, "slab", "e2e_tiny", "/nowhere")
    if retried:
        M._spawn(lambda *a: None, args, 2)
        assert len(calls) == 2, what
        assert calls[1][0][0] == 2 and calls[1][0][2:] == args[2:] and calls[1][0][1] != 23456      # a fresh port, the rest unchanged
        assert calls[1][1] != calls[0][1]                                                     # (the retry's markers are its own)
        assert any("retrying once" in str(w.message) for w in recwarn.list), what
    else:
        with pytest.raises(Exception) as ei:
            M._spawn(lambda *a: None, args, 2)
        assert len(calls) == 1, f"{what}: retried"
        assert not any("retrying" in str(w.message) for w in recwarn.list)
        assert "Dist" not in type(ei.value).__name__
    assert os.environ.get(M._INIT_MARK) == before


def test_spawn_second_transport_failure_is_a_failure(monkeypatch):
    import torch.distributed as dist
    import test_multirank_gpu as M
    calls = []

    def fake_spawn(fn, args=(), nprocs=1, join=True):
        calls.append(args)
        raise dist.DistNetworkError("connection reset")

    monkeypatch.setattr(M.mp, "spawn", fake_spawn)
    with pytest.warns(UserWarning, match="retrying once"), pytest.raises(dist.DistNetworkError):
        M._spawn(lambda *a: None, (2, 23456), 2)
    assert len(calls) == 2
