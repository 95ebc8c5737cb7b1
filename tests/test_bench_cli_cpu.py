"""The bench scripts on a box without a GPU: they accept the driver's flags (`--gpus N --steps K --warmup W`) and then
stop with an error -- no JSON line, no CPU fallback (the oracle is only ever the `cpu_baseline` leg of a GPU run). And
`bench.py --dump-outputs`'s writer, on CPU tensors."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(torch.cuda.is_available(), reason="the point is the behaviour without a GPU")
@pytest.mark.parametrize("script", ["bench.py", "bench_train.py", "bench_soap.py", "bench_pet_box.py"])
def test_bench_refuses_to_run_without_a_gpu(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--gpus", "1", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert "needs MI355X GPUs" in r.stderr
    assert r.stdout.strip() == ""  # no metric line that could be mistaken for a measurement


def test_bench_flags_of_the_contract_are_declared():
    for script in ("bench.py", "bench_train.py", "bench_soap.py", "bench_pet_box.py"):
        text = open(os.path.join(ROOT, script)).read()
        for flag in ('"--gpus"', '"--steps"', '"--warmup"'):
            assert flag in text, (script, flag)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def _bench_module(monkeypatch):
    import importlib

    monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)   # bench.py sets it on import: keep it out of the suite
    monkeypatch.syspath_prepend(ROOT)
    return importlib.import_module("bench")


def test_dump_outputs_are_what_the_step_returned(monkeypatch, tmp_path):
    """`bench.py --dump-outputs`: the chunks' per-atom energies and dE/dR in input order, float32, and the per-box energies
    as float64 sums."""
    import numpy as np

    bench = _bench_module(monkeypatch)
    g = torch.Generator().manual_seed(0)
    outs = [(torch.randn(2 * bench.ATOMS_PER_BOX, generator=g), torch.randn(2 * bench.ATOMS_PER_BOX, 3, generator=g)),
            (torch.randn(bench.ATOMS_PER_BOX, generator=g), torch.randn(bench.ATOMS_PER_BOX, 3, generator=g))]
    bench.dump_outputs(str(tmp_path), outs, 0, 1)
    assert sorted(os.listdir(tmp_path)) == ["atomic_energy.npy", "box_energy.npy", "positions_gradient.npy"]
    a, gr, e = (np.load(tmp_path / f"{n}.npy") for n in ("atomic_energy", "positions_gradient", "box_energy"))
    assert a.dtype == gr.dtype == np.float32 and e.dtype == np.float64
    assert np.array_equal(a, torch.cat([o[0] for o in outs]).numpy())
    assert np.array_equal(gr, torch.cat([o[1] for o in outs]).numpy())
    np.testing.assert_allclose(e, a.astype(np.float64).reshape(3, -1).sum(axis=1), rtol=1e-12)


def test_dump_outputs_sample_a_fixed_subset_past_the_cap(monkeypatch, tmp_path):
    import numpy as np

    bench = _bench_module(monkeypatch)
    g = torch.Generator().manual_seed(1)
    outs = [(torch.randn(4 * bench.ATOMS_PER_BOX, generator=g), torch.randn(4 * bench.ATOMS_PER_BOX, 3, generator=g))]
    limit = 2 * 300_000   # two ranks: 300 kB each, under the 640 kB of one rank's full arrays
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, 1, 2, limit=limit)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["atomic_energy_rank1.npy", "box_energy_rank1.npy", "positions_gradient_rank1.npy",
                     "sampled_atom_index_rank1.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= limit // 2
    for n in names:   # the same sample every time
        x = np.load(tmp_path / "a" / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, np.load(tmp_path / "b" / n))
    idx = np.load(tmp_path / "a" / "sampled_atom_index_rank1.npy").astype(np.int64)
    assert len(idx) > 10_000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "positions_gradient_rank1.npy"), outs[0][1].numpy()[idx])
    assert len(np.load(tmp_path / "a" / "box_energy_rank1.npy")) == 4   # every box, whole
