"""bench.py's plain run and its --dump-outputs / --full options.

CPU: dump_outputs writes the three arrays in float64 / float32, whole when they fit the budget and
at the same fixed seeded indices when they do not; the parser has --full off by default.
GPU: a plain run on a small tensor prints the headline line only, times exactly --steps steps, and
dumps the encode + decode results of the same inputs from run to run; --full adds the rest.
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "kernels_ms", "rank_devices", "d2d_copy_GBs", "cpu_baseline", "config3", "pinned_path",
             "config5"}


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("efl_bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_full_is_off_by_default(bench):
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(bench, tmp_path, monkeypatch):
    n = 5000
    M = torch.arange(n, dtype=torch.int64).reshape(50, 100) - 2500
    E = torch.arange(n, dtype=torch.int64).reshape(50, 100) % 7 - 3
    y = torch.arange(n, dtype=torch.float32).reshape(50, 100) / 8
    bench.dump_outputs(str(tmp_path / "whole"), M, E, y, 0, 1)
    got = {k: np.load(tmp_path / "whole" / f"{k}.npy") for k in ("mantissa", "exponent", "decoded")}
    assert got["mantissa"].dtype == np.float64 and got["exponent"].dtype == np.float64
    assert got["decoded"].dtype == np.float32
    assert np.array_equal(got["mantissa"], M.reshape(-1).numpy())
    assert np.array_equal(got["exponent"], E.reshape(-1).numpy())
    assert np.array_equal(got["decoded"], y.reshape(-1).numpy())
    # over the budget: the same seeded element indices in all three arrays, run after run
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 20 * 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), M, E, y, 0, 1)
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in got}
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in got}
    assert all(np.array_equal(a[k], b[k]) for k in got)
    assert all(a[k].shape == (1000,) for k in got)
    idx = (a["mantissa"] + 2500).astype(np.int64)            # M holds index - 2500
    assert np.array_equal(a["exponent"], idx % 7 - 3) and np.array_equal(a["decoded"], idx.astype(np.float32) / 8)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10**6
    # ranks of an N-rank run write their own files and share the budget
    bench.dump_outputs(str(tmp_path / "r"), M, E, y, 1, 2)
    assert sorted(os.listdir(tmp_path / "r")) == ["decoded_rank1.npy", "exponent_rank1.npy", "mantissa_rank1.npy"]
    assert np.load(tmp_path / "r" / "decoded_rank1.npy").shape == (500,)


def _run(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=110, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    rows = 96                                  # 96 x 1024 fp32: whole outputs fit the dump budget
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    out = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", str(rows), "--dump-outputs", d1])
    assert HEADLINE <= set(out) and not FULL_ONLY & set(out)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "GiB/s" and out["higher_is_better"] is True and out["dtype"] == "int64"
    assert out["ms_per_step"] > 0
    # value = bytes of the tensor per step time
    want = rows * 1024 * 4 / 2**30 / (out["ms_per_step"] * 1e-3)
    assert abs(out["value"] - want) <= 0.01 * want + 0.01
    a = {k: np.load(os.path.join(d1, f"{k}.npy")) for k in ("mantissa", "exponent", "decoded")}
    assert all(v.shape == (rows * 1024,) for v in a.values())
    # the decoded fp32 is mantissa x 2^exponent exactly, and the inputs are N(0,1) draws
    assert np.array_equal(a["decoded"].astype(np.float64), np.ldexp(a["mantissa"], a["exponent"].astype(np.int64)))
    assert abs(float(a["decoded"].mean())) < 0.02 and abs(float(a["decoded"].std()) - 1) < 0.02
    # the same arguments give the same inputs, so the same outputs
    _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", str(rows), "--dump-outputs", d2])
    for k, v in a.items():
        assert np.array_equal(v, np.load(os.path.join(d2, f"{k}.npy"))), k


@pytest.mark.gpu
def test_full_run_adds_the_per_kernel_report():
    out = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--rows", "96", "--full", "--no-extras",
                "--no-cpu-baseline"])
    assert HEADLINE <= set(out) and out["full"] is True
    assert {"roofline", "kernels_ms", "rank_devices", "d2d_copy_GBs", "devices_used"} <= set(out)
    assert out["kernels_ms"]["encode"] > 0 and out["kernels_ms"]["decode"] > 0
