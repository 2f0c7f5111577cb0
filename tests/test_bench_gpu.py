"""GPU: bench.py's command line on a small stream (160x120, 10 mm voxels, 120 frames): a plain run prints the
headline line only, `--steps` sets the timed submaps, `--dump-outputs` writes the loop's outputs as float32
.npy files that a second run with the same arguments reproduces, and `--full` adds the figures beside the metric."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--frames", "120", "--steps", "3", "--warmup", "2", "--width", "160", "--height", "120",
         "--voxel", "0.01", "--buckets", str(1 << 16), "--blocks", str(1 << 15)]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "roofline_ba", "global_solve", "global_dense_end_solve", "raycast", "mesh", "render_in_loop",
             "shard_balance", "cpu_baseline")
NAMES = ("trajectory", "optimized_trajectory", "blocks", "render_depth", "render_normals", "render_colors")


def bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *SMALL, *extra], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines  # one JSON result line
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bench") / "a")
    return bench("--dump-outputs", d), d


def test_plain_run_prints_the_headline_line_only(plain):
    out, _ = plain
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 2 and out["config"]["frames_timed"] == 30
    assert out["loop"]["local_solves"] == 3  # one per timed submap: --steps sets the timed steps
    assert out["value"] > 0 and out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    # value = timed frames / timed seconds, ms_per_step = timed milliseconds / steps
    assert out["ms_per_step"] == pytest.approx(10 * 1e3 / out["value"], rel=1e-9)
    for k in FULL_ONLY:
        assert k not in out, k


def test_dump_outputs_are_float_arrays_a_second_run_reproduces(plain, tmp_path):
    _, d = plain
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    a = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert sum(os.path.getsize(os.path.join(d, n + ".npy")) for n in NAMES) <= 64 << 20
    for n, v in a.items():
        assert v.dtype == np.float32 and v.size > 0 and np.isfinite(v).all(), n
    assert a["trajectory"].shape == (120, 4, 4)
    assert a["blocks"].ndim == 2 and a["blocks"].shape[1] == 3
    assert a["render_depth"].shape[1:] == (480, 640) and (a["render_depth"] > 0).mean() > 0.5
    d2 = str(tmp_path / "b")
    bench("--dump-outputs", d2)
    b = {n: np.load(os.path.join(d2, n + ".npy")) for n in NAMES}
    # the inputs are seeded and the op sequence is repeatable: the same poses up to the order of the solvers' float
    # atomics (1e-4 m: a hundredth of a voxel, far below the 2 mm per-frame drift the solves remove), hence the
    # same blocks but for the few a pose change of that size moves across a block border (under 1 %)
    dt = np.abs(b["trajectory"] - a["trajectory"]).max()
    common = len(set(map(tuple, a["blocks"])) & set(map(tuple, b["blocks"])))
    print(f"trajectory max |diff| {dt:.3g}; blocks {len(a['blocks'])} / {len(b['blocks'])}, common {common}")
    assert b["trajectory"].shape == a["trajectory"].shape and dt <= 1e-4
    assert common >= 0.99 * max(len(a["blocks"]), len(b["blocks"]))


def test_full_adds_the_other_figures():
    out = bench("--full", "--no-cpu-baseline")
    for k in HEADLINE + FULL_ONLY[:-1]:
        assert k in out, k
    assert "cpu_baseline" not in out
    assert out["roofline"]["launches"] > 0 and out["global_dense_end_solve"]["end_phase"]["queueDrained"] == 1
