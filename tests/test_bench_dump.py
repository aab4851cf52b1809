"""bench.py --dump-outputs: the last timed step's arrays as float .npy files, 64 MB in all, a larger array sampled at the same positions in
every run (two builds compare output for output)."""
import importlib.util
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_tests", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_is_float_bounded_and_the_same_sample_every_run(tmp_path):
    b = _bench()
    state = torch.randn(69, 721, 1440, generator=torch.Generator().manual_seed(1))
    small = torch.arange(12, dtype=torch.float16).reshape(3, 4)
    info = b.dump_outputs(str(tmp_path / "a"), {"pangu_state": state, "small": small})
    b.dump_outputs(str(tmp_path / "b"), {"pangu_state": state.clone(), "small": small})
    files = sorted((tmp_path / "a").glob("*.npy"))
    assert [f.name for f in files] == ["pangu_state.npy", "small.npy"]
    assert sum(f.stat().st_size for f in files) <= 64e6
    for f in files:
        a = np.load(f)
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, np.load(tmp_path / "b" / f.name))
    a = np.load(tmp_path / "a" / "pangu_state.npy")
    assert info["pangu_state"] == {"shape": [69, 721, 1440], "saved": list(a.shape)} and a.shape[0] == 69
    pos = torch.randperm(721 * 1440, generator=torch.Generator().manual_seed(0))[:a.shape[1]].sort().values
    assert np.array_equal(a, state.reshape(69, -1)[:, pos].numpy())          # every channel, the seeded positions, in index order
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.float().numpy())     # small enough: whole, as float32


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_plain_run_leaves_every_extra_run_to_full():
    b = _bench()
    extras = ("no_cpu_baseline", "no_parity", "no_alt_modes", "no_models")
    plain = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and all(getattr(plain, k) for k in extras)
    full = b.parse_args(["--gpus", "1", "--full"])
    assert full.full and not any(getattr(full, k) for k in extras)
    part = b.parse_args(["--full", "--no-models"])
    assert part.no_models and not part.no_parity
