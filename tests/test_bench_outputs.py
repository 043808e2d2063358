"""bench.py's plain line and --dump-outputs.

dump_outputs() writes float32 arrays, whole when they fit the 64 MB budget
and as a fixed seeded sample (in index order) when they do not; a plain
bench run carries the headline fields and none of the --full legs, really
runs --steps timed steps' worth of work into the line, and its dumped codes
and bitmap bits agree with each other and repeat from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    a = (np.arange(1000) % 7 - 3).astype(np.int8)
    b = np.arange(1000) % 2 == 0
    bench.dump_outputs(str(tmp_path / "whole"), {"a": a, "b": b})
    got = np.load(tmp_path / "whole" / "a.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "whole" / "b.npy"), b.astype(np.float32))
    # a budget of 800 bytes for two arrays: 100 float32 elements each
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 800)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
    s1, s2 = np.load(tmp_path / "s1" / "a.npy"), np.load(tmp_path / "s2" / "a.npy")
    assert s1.dtype == np.float32 and s1.size == 100 and np.array_equal(s1, s2)
    total = sum(os.path.getsize(tmp_path / "s1" / f) - 128 for f in ("a.npy", "b.npy"))
    assert total <= 800
    # the same seeded indices for both arrays (equal sizes), taken in index order
    idx = np.sort(np.random.default_rng(0x5eed0d07).choice(1000, 100, replace=False))
    assert np.array_equal(s1, a[idx].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "s1" / "b.npy"), b[idx].astype(np.float32))


@pytest.mark.gpu
def test_plain_bench_line_and_dump(tmp_path):
    n = 1 << 14
    lines, dumps = [], []
    for k in (0, 1):
        d = tmp_path / f"out{k}"
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--sigs", str(n),
                            "--dump-outputs", str(d)], cwd=REPO, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [x for x in r.stdout.splitlines() if x.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["unit"] == "verifies/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    # value is the steps' signatures over the steps' time (ms_per_step is rounded to 1e-4 ms, and a step of
    # four launches on two streams takes over 0.05 ms: 1e-3 relative)
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    for k in ("roofline", "pipeline", "cpu_baseline", "c4", "tile"):
        assert k not in line, k
    d0, d1 = dumps
    assert sorted(d0) == ["bitmap_bits", "codes"]
    for k in d0:
        assert d0[k].dtype == np.float32 and d0[k].shape == (n,)
        assert np.array_equal(d0[k], d1[k]), k
    assert np.array_equal(d0["bitmap_bits"] == 1, d0["codes"] == 0)
    assert 0.75 < float((d0["codes"] == 0).mean()) < 0.83          # the C2 mix's accept rate
