"""bench.py's --full and --dump-outputs: a plain run reports the headline only, and the outputs it writes are what the last
timed step computed, at positions that are the same in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_full_is_off_by_default():
    import bench

    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full and b.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_sample_positions_are_fixed():
    import bench

    p = bench.sample_positions(1 << 28, 1000)
    assert np.array_equal(p, bench.sample_positions(1 << 28, 1000))
    assert p.size == 1000 and np.all(np.diff(p) > 0) and p[0] >= 0 and p[-1] < 1 << 28


def test_dump_outputs_exact_and_within_budget(tmp_path):
    import torch

    import bench

    small = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    big = bench.mt19937_keys(5000, 3)
    arrays = {"small": torch.from_numpy(small.view(np.int32).copy()), "big": torch.from_numpy(big.view(np.int32).copy())}
    bench.dump_outputs(str(tmp_path), arrays, 8 * 2 * 1000)            # 1000 float64 values per array
    s = np.load(tmp_path / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small.astype(np.float64))
    b = np.load(tmp_path / "big.npy")
    assert b.dtype == np.float64 and b.size == 1000
    assert np.array_equal(b, big[bench.sample_positions(big.size, 1000)].astype(np.float64))


def _bench(tmp_path, *extra):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--log2-keys", "20", "--dump-outputs", str(out)] + list(extra),
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), out


@pytest.mark.gpu
def test_plain_run_dumps_the_sorted_keys(tmp_path, gpu):
    import bench

    line, out = _bench(tmp_path)
    assert line["unit"] == "Mkeys/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["stages_ms"] is None and line["extra"] == {}
    assert sorted(os.listdir(out)) == ["keys.npy"]
    keys = np.load(out / "keys.npy")
    assert np.array_equal(keys, np.sort(bench.mt19937_keys(1 << 20, 0)).astype(np.float64))


@pytest.mark.gpu
def test_pairs_run_dumps_stable_payloads_and_full_adds_the_roofline(tmp_path, gpu):
    import bench

    line, out = _bench(tmp_path, "--pairs", "--full", "--no-cpu-baseline", "--no-live-traffic")
    assert line["roofline"] is not None and line["stages_ms"] is not None
    assert sorted(os.listdir(out)) == ["keys.npy", "values.npy"]
    src = bench.mt19937_keys(1 << 20, 0)
    order = np.argsort(src, kind="stable")
    assert np.array_equal(np.load(out / "keys.npy"), src[order].astype(np.float64))
    assert np.array_equal(np.load(out / "values.npy"), order.astype(np.float64))
