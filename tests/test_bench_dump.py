"""bench.py's --dump-outputs writer and argument checks (host only: the writer is exercised on CPU tensors)."""
import os
import sys

import numpy as np
import pytest
import torch

import bench


def _outputs(n_fwd=10_000, N=16):
    fwd = torch.linspace(-1.0, 1.0, n_fwd, dtype=torch.float32)
    k = torch.arange(N ** 3, dtype=torch.float32)
    adj = torch.complex(k, -k).reshape(1, N, N, N)  # each element's value names its flat position
    return [("forward", fwd), ("adjoint", adj)]


def test_whole_outputs_fit(tmp_path):
    outs = _outputs()
    shapes = bench.dump_outputs(str(tmp_path), outs, budget=10 ** 6)
    fwd = np.load(tmp_path / "forward.npy")
    adj = np.load(tmp_path / "adjoint.npy")
    assert fwd.dtype == np.float32 and adj.dtype == np.float32
    assert shapes == {"forward": [10_000], "adjoint": [1, 16, 16, 16, 2]}
    np.testing.assert_array_equal(fwd, outs[0][1].numpy())
    np.testing.assert_array_equal(adj, torch.view_as_real(outs[1][1]).numpy())


def test_sample_within_budget_and_fixed(tmp_path):
    budget = 50_000  # the forward output (40 000 bytes) whole, 1 250 of the 4 096 complex values of the adjoint
    bench.dump_outputs(str(tmp_path / "a"), _outputs(), budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), _outputs(), budget=budget)
    a = {name: np.load(tmp_path / "a" / (name + ".npy")) for name in ("forward", "adjoint")}
    b = {name: np.load(tmp_path / "b" / (name + ".npy")) for name in ("forward", "adjoint")}
    assert sum(v.nbytes for v in a.values()) <= budget
    assert a["forward"].shape == (10_000,) and a["adjoint"].shape == (1250, 2)
    for name in a:
        np.testing.assert_array_equal(a[name], b[name])
    pos = a["adjoint"][:, 0]
    assert np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < 16 ** 3  # distinct positions, in order
    np.testing.assert_array_equal(a["adjoint"][:, 1], -pos)  # real and imaginary part of the same element


def test_default_budget_under_64mb():
    assert bench.DUMP_BYTES + 2 * 4096 <= 64_000_000  # payload plus two .npy headers


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_checked(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit):
        bench.parse()


def test_steps_and_dump_dir_parsed(monkeypatch, tmp_path):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--dump-outputs", str(tmp_path)])
    args = bench.parse()
    assert args.steps == 3 and os.path.samefile(args.dump_outputs, tmp_path)
