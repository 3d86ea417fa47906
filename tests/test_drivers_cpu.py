"""The drivers' shared loop and writer (pipeline.in_flight / checked / running_model, inference.run_jobs / write_depth) without a GPU: a
fake pipeline and a fake core log the order of events, the disparities are CPU tensors [1,1,4,6].  What is pinned: submits and waits
interleave as ``DepthMapPipeline.map`` interleaves them, the overflow flag is polled once per finished forward between its wait and its
file, ``check_overflow`` comes once and last, and a ``SaturationError`` - and only that - removes the files of the last ``len(pipe)``
forwards."""
import pytest
import torch

JOBS = 7


class FakeCore:
    def _raise_overflow(self, bits):
        from cer_mvs_amd.raft import SaturationError
        raise SaturationError(f"saturated ({bits})")


class FakePipe:
    """``len(pipe)`` forwards in flight; every call is logged.  ``bits_at``: the poll behind that finished forward (counted from 1) returns
    bits; ``check_bits``: what the final check finds; ``fail_result_at``: ``result`` of that handle raises a RuntimeError."""

    def __init__(self, n, log, bits_at=None, check_bits=0, fail_result_at=None):
        self.n, self.log, self.bits_at, self.check_bits, self.fail_result_at = n, log, bits_at, check_bits, fail_result_at
        self.core, self.finished = FakeCore(), 0

    def __len__(self):
        return self.n

    def submit(self, i):
        self.log.append(f"s{i}")
        return i

    def result(self, handle):
        self.log.append(f"w{handle}")
        if handle == self.fail_result_at:
            raise RuntimeError("out of memory")
        return torch.full((1, 1, 4, 6), 1.0 / (handle + 2))

    def poll_overflow(self):
        self.finished += 1
        self.log.append(f"p{self.finished - 1}")
        return 4 if self.finished == self.bits_at else 0

    def check_overflow(self):
        self.log.append("c")
        if self.check_bits:
            self.core._raise_overflow(self.check_bits)
        return 0


def _jobs(pipe, n=JOBS, fail_at=None):
    for i in range(n):
        if i == fail_at:
            raise RuntimeError("loader failed")
        yield pipe.submit(i), f"v{i}", 4


@pytest.fixture
def logged_writes(monkeypatch):
    """inference.write_pfm, logging which file it writes"""
    from cer_mvs_amd import inference
    log, plain = [], inference.write_pfm

    def write_pfm(path, image, *a, **k):
        log.append("f" + path.name[1:path.name.index("_")])
        return plain(path, image, *a, **k)
    monkeypatch.setattr(inference, "write_pfm", write_pfm)
    return log


def _run(tmp_path, log, n, jobs=None, **kw):
    from cer_mvs_amd.inference import run_jobs
    (tmp_path / "depths").mkdir(exist_ok=True)
    pipe = FakePipe(n, log, **kw)
    return run_jobs(pipe, pipe.core, jobs(pipe) if jobs else _jobs(pipe), tmp_path, 1, write_min_depth=tmp_path / "min")


def _left(tmp_path):
    return sorted(int(p.name[1:p.name.index("_")]) for p in (tmp_path / "depths").glob("*.pfm"))


def _map_order(n):
    """submits and waits of the pipeline's own ``map`` (its code, on logging stand-ins for ``submit`` and ``result``)"""
    from cer_mvs_amd.pipeline import DepthMapPipeline

    class Logged(DepthMapPipeline):
        def __init__(self):
            self.streams, self.log = [None] * n, []

        def submit(self, i):
            self.log.append(f"s{i}")
            return i

        def result(self, handle):
            self.log.append(f"w{handle}")

        def close(self):
            pass
    pipe = Logged()
    assert len(list(pipe.map((i,) for i in range(JOBS)))) == JOBS
    return pipe.log


@pytest.mark.parametrize("n", [3, 1])
def test_order_of_events(tmp_path, logged_writes, n):
    log = logged_writes
    written = _run(tmp_path, log, n)
    assert [e for e in log if e[0] in "sw"] == _map_order(n)
    if n == 3:
        assert log[:8] == ["s0", "s1", "s2", "w0", "p0", "f0", "s3", "w1"]
        assert log[-7:] == ["w5", "p5", "f5", "w6", "p6", "f6", "c"]
    else:
        assert log == [f"{e}{i}" for i in range(JOBS) for e in "swpf"] + ["c"]
    for i in range(JOBS):                                   # one poll per finished forward, after its wait and before its file
        assert log.count(f"p{i}") == 1 and log.index(f"w{i}") + 1 == log.index(f"p{i}") == log.index(f"f{i}") - 1
    assert log.count("c") == 1 and log[-1] == "c"
    assert written == [str(tmp_path / "depths" / f"v{i}_scale1_nf4.pfm") for i in range(JOBS)] and _left(tmp_path) == list(range(JOBS))
    # the files themselves: the depth is 1 / disparity, the min-depth text half its 10 % quantile
    from cer_mvs_amd.fusion import read_pfm
    assert (read_pfm(written[2]) == 4.0).all() and read_pfm(written[2]).shape == (4, 6)
    assert (tmp_path / "min" / "v2.txt").read_text() == "2.0\n"


def test_poll_finds_bits_at_the_sixth_finished_forward(tmp_path, logged_writes):
    from cer_mvs_amd.raft import SaturationError
    with pytest.raises(SaturationError):
        _run(tmp_path, logged_writes, 3, bits_at=6)
    assert _left(tmp_path) == [0, 1]                         # 2, 3 and 4 removed, 5 and 6 never written
    assert [e for e in logged_writes if e[0] == "f"] == ["f0", "f1", "f2", "f3", "f4"]
    assert "c" not in logged_writes and logged_writes[-2:] == ["w5", "p5"]


def test_final_check_raises(tmp_path, logged_writes):
    from cer_mvs_amd.raft import SaturationError
    with pytest.raises(SaturationError):
        _run(tmp_path, logged_writes, 3, check_bits=2)
    assert [e for e in logged_writes if e[0] == "f"] == [f"f{i}" for i in range(JOBS)]
    assert _left(tmp_path) == [0, 1, 2, 3]


@pytest.mark.parametrize("where", ["jobs", "result"])
def test_another_error_removes_nothing(tmp_path, logged_writes, where):
    with pytest.raises(RuntimeError, match="loader failed" if where == "jobs" else "out of memory"):
        if where == "jobs":
            _run(tmp_path, logged_writes, 3, jobs=lambda pipe: _jobs(pipe, fail_at=5))
        else:
            _run(tmp_path, logged_writes, 3, fail_result_at=3)
    assert _left(tmp_path) == [0, 1, 2]
    assert "c" not in logged_writes


def test_checked_hands_over_entry_and_result_and_checks_once():
    from cer_mvs_amd.pipeline import checked, in_flight
    assert list(in_flight(iter(range(5)), 2)) == list(range(5)) and list(in_flight(iter(()), 3)) == []
    log = []
    pipe = FakePipe(2, log)
    got = list(checked(pipe, pipe.core, (pipe.submit(i) for i in range(3)), lambda h: 10 * h))
    assert got == [(0, 0), (1, 10), (2, 20)]
    assert log == ["s0", "s1", "p0", "s2", "p1", "p2", "c"]


def test_running_model_unwraps_and_restores_training():
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.pipeline import running_model, stream_count, unwrap
    raft = RAFT(test_mode=True)

    class Wrapper(torch.nn.Module):                         # (what nn.DataParallel looks like from here)
        def __init__(self, module):
            super().__init__()
            self.module = module
    other = Wrapper(torch.nn.Linear(2, 2))
    assert unwrap(raft) is raft and unwrap(Wrapper(raft)) is raft and unwrap(other) is other
    raft.train()
    with running_model(raft) as core:
        assert core is raft and not raft.training
    assert raft.training
    with pytest.raises(KeyError):
        with running_model(Wrapper(raft)) as core:
            assert core is raft and not raft.training
            raise KeyError("inside the block")
    assert raft.training
    raft.eval()
    with running_model(raft) as core:
        assert core is raft
    assert not raft.training
    # a model with a view_group runs one depth map at a time
    assert stream_count(raft, 3) == 3 and stream_count(raft, 0) == 1 and stream_count(raft, "2") == 2
    raft.view_group = object()
    assert stream_count(raft, 3) == 1
