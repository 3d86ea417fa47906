"""Host-side pieces of the training step (no GPU): the reference's optimiser schedule (train.py:19-27) and the range table of the
upsample adjoint (csrc/train_ops.hip, cer_upsample_ac_ranges)."""
import numpy as np
import pytest
import torch


def test_fetch_optimizer_reproduces_the_reference_schedule(golden):
    """fetch_optimizer on a CPU RAFT gives the learning rates the reference's own fetch_optimizer gave
    (tests/golden/train_step_tiny.npz = tools/gen_golden.py --only train_step_tiny), exactly."""
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.train import fetch_optimizer
    g = golden("train_step_tiny")
    model = RAFT(cascade=[tuple(int(x) for x in c) for c in g["cascade"]], test_mode=False)
    opt, sch = fetch_optimizer(model, num_steps=int(g["num_steps"]))
    assert isinstance(opt, torch.optim.AdamW) and opt.defaults["weight_decay"] == 5e-5 and opt.defaults["eps"] == 1e-8
    seq = []
    for _ in range(len(g["lr_sequence"])):
        opt.step()
        sch.step()
        seq.append(sch.get_last_lr()[0])
    assert seq == [float(x) for x in g["lr_sequence"]]
    assert seq[:2] == [float(x) for x in g["lr"]]            # the two training steps of the capture ran on the same schedule


def _brute_force_ranges(n_in, n_out):
    """For every input texel, the set of outputs whose two source texels include it - enumerated output by output in float32
    (torch's upsample_bilinear2d, align_corners=True)."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    sets = [set() for _ in range(n_in)]
    for X in range(n_out):
        s = np.float32(scale * np.float32(X))
        i0 = min(int(s), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        sets[i0].add(X)
        sets[i1].add(X)
    return sets


@pytest.mark.parametrize("n_in,n_out", [(1, 1), (1, 5), (5, 1), (3, 8), (16, 64), (8, 64), (13, 50), (24, 96), (7, 7), (50, 13),
                                        (132, 1056)])
def test_upsample_adjoint_range_table_matches_enumeration(n_in, n_out):
    from cer_mvs_amd import ops
    table = ops.upsample_ac_ranges(n_in, n_out)
    assert table.shape == (n_in, 2) and table.dtype == torch.int32
    for j, s in enumerate(_brute_force_ranges(n_in, n_out)):
        lo, hi = int(table[j, 0]), int(table[j, 1])
        if not s:
            assert lo == hi == 0, j
        else:
            assert (lo, hi) == (min(s), max(s) + 1) and len(s) == hi - lo, j     # one contiguous range
