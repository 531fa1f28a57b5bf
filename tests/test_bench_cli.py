"""bench.py's command line and --dump-outputs writer (host logic only; no GPU)."""
import sys
import types

import numpy as np
import pytest
import torch

import bench


def _fake_trainer(n):
    torch.manual_seed(0)
    m = torch.nn.Linear(n, 1)
    e = torch.nn.Linear(n, 1)
    return types.SimpleNamespace(_bench_last_loss=torch.tensor(0.25), _module=m, ema_model=e)


def test_dump_outputs_small_state_is_whole(tmp_path):
    tr = _fake_trainer(7)
    bench.dump_outputs(str(tmp_path / "d"), tr)
    loss = np.load(tmp_path / "d" / "loss.npy")
    assert loss.dtype == np.float32 and loss.tolist() == [0.25]
    for name, mod in (("params", tr._module), ("ema_params", tr.ema_model)):
        a = np.load(tmp_path / "d" / f"{name}.npy")
        ref = torch.cat([p.detach().reshape(-1) for p in mod.parameters()]).numpy()
        assert a.dtype == np.float32 and np.array_equal(a, ref)


def test_dump_outputs_large_state_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 16)
    tr = _fake_trainer(100)
    tr.ema_model = None                      # ranks without an EMA model write none
    bench.dump_outputs(str(tmp_path / "a"), tr)
    bench.dump_outputs(str(tmp_path / "b"), tr)
    a, b = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "b" / "params.npy")
    assert a.shape == (16,) and np.array_equal(a, b)
    flat = torch.cat([p.detach().reshape(-1) for p in tr._module.parameters()]).numpy()
    idx = np.sort(np.random.default_rng(0).integers(0, flat.size, 16))
    assert np.array_equal(a, flat[idx])
    assert not (tmp_path / "a" / "ema_params.npy").exists()


def test_no_train_needs_full(monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--no-train"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and "--full" in capsys.readouterr().err
