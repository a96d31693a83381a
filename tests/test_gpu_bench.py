"""bench.py's plain command at a reduced size: one line with the headline and nothing measured beside it, exactly --steps
timed steps, and --dump-outputs writing the last step's outputs, the same from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--warmup", "1", "--side", "1000", "--grid", "256"]
SAMPLE = 1 << 18        # bench.DUMP_SAMPLE: 1e6 particles are more than the dump's sample


def run_bench(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_times_the_headline_alone_and_dumps_its_outputs(tmp_path):
    lines, dumps = [], []
    for k, steps in enumerate((3, 5)):
        d = tmp_path / ("run%d" % k)
        lines.append(run_bench(["--steps", str(steps), "--dump-outputs", str(d)]))
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    for line, steps in zip(lines, (3, 5)):
        assert line["metric"] == "particle-updates/sec (push+deposit+solve)" and line["unit"] == "particle-updates/s", line
        assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["steps"] == steps, line
        assert line["value"] > 0 and line["ms_per_step"] > 0, line
        assert line["roofline"]["launches_timed"] == steps, line
        assert abs(line["value"] - 2.0 * 1000 * 1000 * steps / (line["ms_per_step"] * steps * 1e-3)) <= 1e-6 * line["value"], line
        for key in ("cpu_baseline", "extensions", "strong_c4"):
            assert key not in line, key
    grids, particles = ("density", "moments"), ("position", "velocity")
    for out in dumps:
        assert sorted(out) == sorted(("alive",) + grids + particles + tuple(k + "_nonfinite" for k in grids + particles)), sorted(out)
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
        assert out["density"].shape == out["moments"].shape == (256, 256, 4)
        assert out["density_nonfinite"].shape == out["moments_nonfinite"].shape == (256, 256)
        assert out["position"].shape == out["velocity"].shape == (SAMPLE, 3) and out["alive"].shape == (SAMPLE,)
        assert out["position_nonfinite"].shape == out["velocity_nonfinite"].shape == (SAMPLE,)
        for k in grids + particles:   # a channel bitmask, and a marked value is written as 0
            m = out[k + "_nonfinite"].astype(np.int64)
            assert ((m >= 0) & (m < 1 << out[k].shape[-1])).all() and (out[k][m != 0] == 0).any(axis=-1).all(), k
        assert sum(a.nbytes for a in out.values()) <= 64 << 20
        assert out["alive"].sum() > 0 and out["density"][..., 3].max() > 0
    # the same arguments, the same inputs: a third run with the first one's arguments reproduces its particles and every mask
    # bit for bit, and its grids up to the order of the deposit's float atomics
    d = tmp_path / "again"
    run_bench(["--steps", "3", "--dump-outputs", str(d)])
    again = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    for name in particles + ("alive",) + tuple(k + "_nonfinite" for k in grids + particles):
        assert np.array_equal(again[name], dumps[0][name]), name
    assert np.allclose(again["density"], dumps[0]["density"], rtol=1e-4, atol=1e-6 * np.abs(dumps[0]["density"]).max())


def test_full_run_keeps_the_extension_blocks(tmp_path):
    line = run_bench(["--steps", "2", "--full", "--no-cpu-baseline", "--no-c5", "--c3-particles", "2000000", "--c3-grid", "64",
                      "--c4-grid", "64", "--c4-particles", "4e6", "--c4-ghost", "2"])
    assert line["steps"] == 2 and line["value"] > 0, line
    ext = line["extensions"]
    for key in ("counter_rng", "c2_cic", "dense_sor", "em", "c3"):
        assert key in ext, key
    assert line["strong_c4"]["value"] > 0 and line["strong_c4"]["lost_rank0"] == 0, line["strong_c4"]
