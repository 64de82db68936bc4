"""Times slk_step_n (T fused steps in one call) against a loop of T slk_step calls at the same shape, both with
device-resident inputs (torch tensors on cuda:0) and no records, plus slk_step_n with the mean and NEES records.

  python tools/bench_trajectory.py --shape n12_m3_b1024     one shape in this process: one CSV row on stdout
  python tools/bench_trajectory.py --all --out profiles/    every shape, each in a child process of its own under
                                                           `rocprofv3 --kernel-trace --stats` with a time limit;
                                                           stops at the first failing shape

The handle's HIP events give the time of --reps trajectories of T steps (launch and host overhead included); the
per-step times are that divided by T.  --all writes trajectory_<shape>_kernel_stats.csv per shape and
trajectory_times.csv (the rows of every shape).

  python tools/bench_trajectory.py --shape n60_m8_b4096_t200 --diag     the cost of the per-step consistency records
                                                           (slk_step_n_diag): step_n with no records, with the sigma
                                                           record, and with nis + logdet + sigma, in the same process.
Each variant runs --warmup passes, then --passes timed passes of one trajectory each (the handle's HIP events around
one call); one CSV row per variant with the median, the fastest and the slowest pass: the spread of the passes is the
tool's run-to-run spread.  --variants none restricts the run (a library without the records can run that one).
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name: (k, m, measurement model, B, T)
SHAPES = {
    "n12_m3_b1024": (0, 3, "pose", 1024, 200),
    "n18_m2_b1024": (1, 2, "feat", 1024, 200),
    "n60_m8_b1024": (8, 8, "feat", 1024, 50),
    "n60_m8_b4096": (8, 8, "feat", 4096, 50),
    "n60_m8_b4096_t200": (8, 8, "feat", 4096, 200),         # the headline shape of the record-cost measurement (--diag)
}
DIAG_VARIANTS = {"none": (), "sigma": ("sigma",), "all": ("nis", "logdet", "sigma")}
DIAG_HEADER = "shape,N,m,B,T,records,median_step_us,min_step_us,max_step_us,passes"
HEADER = "shape,N,m,B,T,loop_step_us,step_n_us,step_n_records_us"


def run_one(name, reps, warmup):
    import numpy as np
    import torch
    from slkpkg import slk
    import scenarios as sc
    k, m, model, B, T = SHAPES[name]
    s = sc.synthetic_msckf(B, k, m=m if model == "feat" else 8, seed=0x7EA7)
    rng = np.random.default_rng(1)
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    if model == "feat":
        mm, gate, params = slk.MM_FEATURE_PROJ, 1, s["feat"].reshape(B, -1)
        z0 = s["z"]
    else:
        mm, gate, params = slk.MM_POSE_POSITION, 0, np.zeros((B, 1))
        z0 = s["mean"][:, 0:3]
    U = np.repeat(s["u"][None], T, axis=0)
    U[:, :, 0:3] += rng.normal(0, 0.01, (T, B, 3))
    Z = z0[None] + rng.normal(0, 0.02, (T, B, m))
    Ud, Zd, Qd, Rd = d(U), d(Z), d(s["Q"]), d(0.01 * np.eye(m))
    Pd = d(params)
    Ptd = Pd.unsqueeze(0).expand(T, *params.shape)
    truth = d(np.repeat(s["mean"][None], T, axis=0))
    f = slk.Msckf(s["mean"], s["P"])

    def loop():
        for t in range(T):
            f.step(slk.PM_DELTA_POSE, Ud[t], Qd, Zd[t], mm, Pd, Rd, gate=gate)

    def step_n():
        f.step_n(slk.PM_DELTA_POSE, Ud, Qd, Zd, mm, Ptd, Rd, gate=gate)

    def step_n_rec():
        f.step_n(slk.PM_DELTA_POSE, Ud, Qd, Zd, mm, Ptd, Rd, gate=gate, truth=truth, record_mean=True)

    res = []
    for fn in (loop, step_n, step_n_rec):
        f.set_state(s["mean"], s["P"])
        for _ in range(warmup):
            fn()
        f.sync()
        f.timer_start()
        for _ in range(reps):
            fn()
        res.append(1e3 * f.timer_stop() / (reps * T))
    f.close()
    print(f"{name},{12 + 6 * k},{m},{B},{T},{res[0]:.2f},{res[1]:.2f},{res[2]:.2f}", flush=True)


def run_diag(name, passes, warmup, variants):
    import numpy as np
    import torch
    from slkpkg import slk
    import scenarios as sc
    k, m, model, B, T = SHAPES[name]
    assert model == "feat"
    s = sc.synthetic_msckf(B, k, m=m, seed=0x7EA7)
    rng = np.random.default_rng(1)
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    params = s["feat"].reshape(B, -1)
    U = np.repeat(s["u"][None], T, axis=0)
    U[:, :, 0:3] += rng.normal(0, 0.01, (T, B, 3))
    Z = s["z"][None] + rng.normal(0, 0.02, (T, B, m))
    Ud, Zd, Qd, Rd = d(U), d(Z), d(s["Q"]), d(0.01 * np.eye(m))
    Pd = d(params)
    Ptd = Pd.unsqueeze(0).expand(T, *params.shape)
    f = slk.Msckf(s["mean"], s["P"])
    for v in variants:
        kw = {"diag": DIAG_VARIANTS[v]} if DIAG_VARIANTS[v] else {}
        times = []
        for i in range(warmup + passes):
            f.set_state(s["mean"], s["P"])
            f.sync()
            f.timer_start()
            f.step_n(slk.PM_DELTA_POSE, Ud, Qd, Zd, slk.MM_FEATURE_PROJ, Ptd, Rd, gate=1, **kw)
            t = 1e3 * f.timer_stop() / T
            if i >= warmup:
                times.append(t)
        print(f"{name},{12 + 6 * k},{m},{B},{T},{v},{np.median(times):.2f},{min(times):.2f},{max(times):.2f},{passes}", flush=True)
    f.close()


def run_all(out_dir, reps, warmup, limit):
    os.makedirs(out_dir, exist_ok=True)
    rows = [HEADER]
    for name in SHAPES:
        if name.endswith("_t200"):                               # (the --diag shape)
            continue
        tmp = tempfile.mkdtemp(prefix="traj_")
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
               "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--shape", name, "--reps", str(reps),
               "--warmup", str(warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        row = [ln for ln in p.stdout.splitlines() if ln.startswith(name + ",")]
        if p.returncode != 0 or not row:
            sys.stderr.write(f"{name}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}\n")
            return 1
        rows.append(row[0])
        print(row[0], flush=True)
        stats = [os.path.join(dd, fn) for dd, _, fs in os.walk(tmp) for fn in fs if fn.endswith("kernel_stats.csv")]
        if stats:
            shutil.copy(stats[0], os.path.join(out_dir, f"trajectory_{name}_kernel_stats.csv"))
        shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(out_dir, "trajectory_times.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape (--all)")
    ap.add_argument("--diag", action="store_true", help="with --shape: the cost of the per-step consistency records")
    ap.add_argument("--passes", type=int, default=7, help="timed passes per variant (--diag)")
    ap.add_argument("--variants", default="none,sigma,all", help="--diag: comma-separated subset of none, sigma, all")
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.out, a.reps, a.warmup, a.limit))
    if not a.shape:
        ap.error("--shape or --all")
    if a.diag:
        print(DIAG_HEADER)
        run_diag(a.shape, a.passes, a.warmup, a.variants.split(","))
        return
    print(HEADER)
    run_one(a.shape, a.reps, a.warmup)


if __name__ == "__main__":
    main()
