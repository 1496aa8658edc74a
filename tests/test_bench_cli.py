"""bench.py's command line and its --dump-outputs writer, CPU side: a plain
run keeps the further legs off, and the dump is float32 / float64 .npy files,
a fixed sample of the parameters, identical from call to call."""
import os
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_keeps_further_legs_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_files(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_PARAM_SAMPLE", 1000)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(50, 40))   # 35+5 and 2000+40 elements
    loss, norm = torch.tensor(0.25), torch.tensor([3.0, 1.0])[0]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, model, loss, norm)
    bench.dump_outputs(b, model, loss, None)
    assert sorted(os.listdir(a)) == ["grad_norm.npy", "loss.npy", "param_norms.npy", "params.npy"]
    assert sorted(os.listdir(b)) == ["loss.npy", "param_norms.npy", "params.npy"]
    got = {f[:-4]: np.load(os.path.join(a, f)) for f in os.listdir(a)}
    assert got["loss"].dtype == np.float32 and got["loss"].tolist() == [0.25]
    assert got["grad_norm"].dtype == np.float32 and got["grad_norm"].tolist() == [3.0]
    ps = [p.detach() for p in model.parameters()]
    assert got["param_norms"].dtype == np.float64
    np.testing.assert_allclose(got["param_norms"], [float(p.double().norm()) for p in ps], rtol=1e-12)
    flat = torch.cat([p.reshape(-1) for p in ps]).numpy()
    s = got["params"]
    assert s.dtype == np.float32 and s.shape == (1000,)
    assert np.isin(s, flat).all()                       # a sample of the parameters themselves
    assert np.array_equal(s, np.load(os.path.join(b, "params.npy")))   # the same one every call
    monkeypatch.setattr(bench, "DUMP_PARAM_SAMPLE", 1 << 20)
    bench.dump_outputs(b, model, loss, None)            # small enough: the whole vector, in order
    assert np.array_equal(np.load(os.path.join(b, "params.npy")), flat)
