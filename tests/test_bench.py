"""bench.py's own contract: a plain run times the headline alone, --full adds everything else, --steps is the number of timed
steps, and --dump-outputs writes a fixed, seeded sample of what the last timed step shipped out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse_args()


def test_plain_and_full_arguments(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.steps == 7 and a.warmup == 2 and not a.full
    assert a.headline_only and a.no_timing and a.no_cross_check and a.dump_outputs is None
    a = _args(monkeypatch, "--full")
    assert a.full and a.steps == 200 and not a.headline_only and not a.no_timing and not a.no_cross_check
    assert _args(monkeypatch, "--full", "--legs", "none").headline_only
    # --steps is the number of timed steps in every mode, the greedy dispatch's default included
    assert _args(monkeypatch, "--dispatch", "greedy").steps == 10
    assert _args(monkeypatch, "--dispatch", "greedy", "--steps", "200").steps == 200
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--workload", "cfg5", "--dump-outputs", "x"]):
        with pytest.raises(SystemExit):
            _args(monkeypatch, *bad)


def test_sample_blocks_fixed_and_in_bounds():
    import bench
    assert bench.sample_blocks(0, 0, 0, 0) == []
    assert bench.sample_blocks(1000, 0, 0, 0) == [(0, 1000)]
    for n in (bench.DUMP_BLOCKS * bench.DUMP_ROWS + 1, 10_000, 14_000_000):
        b = bench.sample_blocks(n, 2, 5, 1)
        assert b == bench.sample_blocks(n, 2, 5, 1)                     # the same rows every run
        assert len(b) == bench.DUMP_BLOCKS and all(rows == bench.DUMP_ROWS for _, rows in b)
        starts = [f for f, _ in b]
        assert starts == sorted(set(starts)) and all(f % bench.DUMP_ROWS == 0 and f + r <= n for f, r in b)
    assert bench.sample_blocks(10_000, 0, 0, 0) != bench.sample_blocks(10_000, 0, 1, 0)
    # the most a step can write stays under 64 MB
    per_shipout = bench.DUMP_BLOCKS * bench.DUMP_ROWS * (3 * 4 + 3 * 8 + 2 * 8 + 3 * 2 * 8)
    assert bench.DUMP_SHIPOUTS * per_shipout < 64 << 20


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    """A plain run at 2 % of the cfg3 cloud: the headline fields and nothing of --full; the dump of its last timed step
    agrees with the step's counts and is the same, file for file, in a second run."""
    dumps = []
    for i in range(2):
        out = tmp_path / ("run%d" % i)
        d = _bench(["--gpus", "1", "--scale", "0.02", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["metric"] == "Mvoxels/s evaluated+triangulated" and d["unit"] == "Mvoxels/s" and d["higher_is_better"]
        assert d["dtype"] == "f32" and d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["ms_per_step"] * 3 - d["timed_region_s"] * 1e3) < 1.0      # (both rounded to a microsecond / millisecond)
        for k in ("roofline", "cpu_baseline", "shells", "transfer_inclusive", "mesh_sink", "device_partition",
                  "other_splat_protocol", "kernel_ms_per_step", "leg_errors"):
            assert k not in d, k
        files = sorted(os.listdir(out))
        assert files == sorted(["shipouts.npy", "vertices.npy", "vertices_rows.npy", "triangles.npy", "triangles_rows.npy",
                                "external_keys.npy", "external_keys_rows.npy"])
        arrays = {f[:-4]: np.load(out / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) < 64 << 20
        s = arrays["shipouts"]
        cfg = d["config"]
        assert cfg["shipouts_per_step"] > 0 and cfg["triangles_per_step"] > 0 and cfg["vertices_per_step"] > 0
        assert len(s) == cfg["shipouts_per_step"]
        assert s[:, 2].sum() == cfg["vertices_per_step"] and s[:, 3].sum() == cfg["triangles_per_step"]
        v, vr = arrays["vertices"], arrays["vertices_rows"]
        t, tr = arrays["triangles"], arrays["triangles_rows"]
        assert len(v) == len(vr) > 0 and len(t) == len(tr) > 0 and np.isfinite(v).all()
        assert (vr[:, 1] < s[vr[:, 0].astype(int), 2]).all() and (tr[:, 1] < s[tr[:, 0].astype(int), 3]).all()
        assert (t < s[tr[:, 0].astype(int), 2][:, None]).all()          # indices point into their own ship-out
        kr = arrays["external_keys_rows"]
        assert len(arrays["external_keys"]) == len(kr)
        assert (kr[:, 1] < s[kr[:, 0].astype(int), 2] - s[kr[:, 0].astype(int), 4]).all()
        dumps.append(arrays)
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
