"""GPU: a plain `bench.py --gpus 1` run -- the headline figure only, exactly `--steps` timed steps -- and what `--dump-outputs` writes:
the C2 job's state after the last timed step, bit for bit the CPU oracle's run of the same seeded job."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_its_steps_and_dumps_the_oracles_final_state(kmc, oracle, tmp_path):
    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KMC_BENCH_TEST", "KMC_LAUNCH")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "walker-steps/sec" and line["unit"] == "walker-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["repetitions"] == 1 and line["config"]["generations"] == 2000
    assert line["value"] == pytest.approx(65536 * 2000 / (2 * line["ms_per_step"] * 1e-3), rel=1e-9)       # one timed run of exactly 2 steps
    for key in ("other_configs", "cpu_baseline", "island_mode"):                                           # (--full only)
        assert key not in line, key

    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert set(got) == {"positions", "logp", "naccept", "moment_sum", "moment_sumsq", "nmoment"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["positions"].shape == (65536, 32) and got["nmoment"][0] == line["check"]["nmoment"]
    assert got["naccept"].sum() / 65536 / 1000 == pytest.approx(line["check"]["accept_ratio_mean"], rel=1e-6)

    sys.path.insert(0, ROOT)
    import bench
    th = bench.theta0_c2(65536)
    ref = oracle.emcee(oracle.make_config(oracle.GAUSSIAN_ISO, [0.0, 1.0], 65536, 32, 2000, 1000, 1, 2.0, bench.SEED,
                                          nthreads=min(16, bench.host_threads())), th, store_chain=False)
    assert ref["status"] == 0
    assert (got["positions"] == ref["final_pos"]).all() and (got["naccept"] == ref["naccept"]).all()
    assert np.all(np.abs(got["logp"] - ref["final_logp"]) <= 1e-12 * np.maximum(1.0, np.abs(ref["final_logp"])))
    assert got["nmoment"][0] == ref["nmoment"] and np.allclose(got["moment_sum"], ref["sum"], rtol=1e-11, atol=1e-9)
