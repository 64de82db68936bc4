"""bench.py --dump-outputs and --steps: what the timed path computed in its last step, written as .npy files.

The host tests run the dump on the CPU rehearsal and on plain arrays; the GPU test runs the real workload at a small
batch and holds the dumped state to the CPU oracle run for the same number of steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), env=env, capture_output=True,
                         text=True, timeout=timeout)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _load(d):
    return {fn[:-4]: np.load(os.path.join(d, fn)) for fn in sorted(os.listdir(d)) if fn.endswith(".npy")}


def test_dump_writes_every_filter_when_the_batch_fits(tmp_path):
    B = 10
    outs = {"mean": np.arange(B * 3, dtype=np.float64).reshape(B, 3), "status": np.arange(B, dtype=np.int32),
            "outliers": np.full(B, 2 ** 32 - 1, dtype=np.uint32)}
    bench.dump_outputs(str(tmp_path), outs)
    got = _load(str(tmp_path))
    assert sorted(got) == ["filter_index", "mean", "outliers", "status"]
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["filter_index"], np.arange(B))
    np.testing.assert_array_equal(got["mean"], outs["mean"])
    np.testing.assert_array_equal(got["outliers"], outs["outliers"].astype(np.float64))     # exact in float64


def test_dump_samples_a_large_batch_within_the_budget(tmp_path):
    B, N = 4096, 60
    rng = np.random.default_rng(3)
    outs = {"P": rng.standard_normal((B, N, N)), "mean": rng.standard_normal((B, 69)), "status": np.zeros(B, np.int32)}
    assert sum(a.size for a in outs.values()) * 8 > bench.DUMP_BUDGET            # the whole batch would not fit
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), outs)
    bench.dump_outputs(str(b), outs)
    assert sum(f.stat().st_size for f in a.iterdir()) <= 64 * 10 ** 6
    ga, gb = _load(str(a)), _load(str(b))
    idx = ga["filter_index"].astype(np.int64)
    assert 0 < len(idx) < B and len(np.unique(idx)) == len(idx) and (np.diff(idx) > 0).all()
    np.testing.assert_array_equal(ga["filter_index"], gb["filter_index"])        # the same sample from run to run
    for n in ("P", "mean", "status"):
        assert len(ga[n]) == len(idx)
        np.testing.assert_array_equal(ga[n], outs[n][idx])


def test_dry_run_dumps_and_steps_sets_the_timed_steps(tmp_path):
    j = _bench(["--steps", "13", "--warmup", "2", "--batch", "16", "--dry-run", "--dump-outputs", str(tmp_path / "o")])
    assert j["steps"] == 13 and j["per_rank"][0]["steps"] == 13
    assert j["ms_per_step"] >= 1.0                   # the rehearsal sleeps 1 ms per step
    got = _load(str(tmp_path / "o"))
    assert sorted(got) == ["filter_index", "status"] and got["status"].shape == (16,)


def test_steps_below_one_is_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--steps" in out.stderr


@pytest.mark.gpu
def test_dumped_outputs_are_the_state_after_warmup_and_timed_steps(tmp_path):
    from oracle import oracle as o
    import scenarios as sc
    B, k, m, warmup, steps = 64, 8, 8, 2, 3
    d = str(tmp_path / "out")
    j = _bench(["--steps", str(steps), "--warmup", str(warmup), "--batch", str(B), "--no-cpu-baseline",
                "--dump-outputs", d])
    assert j["steps"] == steps and j["filters_with_numerical_status"] == 0
    got = _load(d)
    assert sorted(got) == ["P", "filter_index", "mean", "outliers", "status"]
    np.testing.assert_array_equal(got["filter_index"], np.arange(B))
    s = sc.synthetic_msckf(B, k, m=m, seed=bench.SEED0)
    N = s["N"]
    mean, P = s["mean"].copy(), s["P"].copy()
    st, _ = o.msckf_step_batch(k, m, warmup + steps, mean, P, s["u"], s["feat"], s["z"], s["Q"], s["R"])
    assert st == 0 and (got["status"].astype(np.int64) & ~bench.ST_ALL_REJECTED == 0).all()
    lay = o.layout(o.MULTI, k)
    for b in range(B):
        Pb = P[b].reshape(N, N).T
        assert np.abs(got["P"][b] - Pb).max() <= 1e-9 * np.abs(Pb).max(), b
        assert np.abs(o.boxminus(lay, got["mean"][b], mean[b])).max() <= 1e-9, b
