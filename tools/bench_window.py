"""Measures the one-launch window slide (slk_msckf_slide, msckf_slide_kernel) against the sequence it replaces
(slk_msckf_drop_clone + slk_msckf_clone_pose: a mirror pass when P is lower-only, then two msckf_window_kernel gathers).

  python tools/bench_window.py --shape n60_b4096 --mode ops     R x (step, slide) then R x (step, drop, clone): run
                                                                 under `rocprofv3 --kernel-trace --stats` for kernel times
  python tools/bench_window.py --shape n60_b4096 --mode traj    T = 50 steps that slide after every step, device inputs:
                                                                 step_n(slide=0) against the loop of step + drop_clone(0)
                                                                 + clone_pose(); one CSV row (handle events, us per step)
  python tools/bench_window.py --all --out profiles/            every shape: ops under kernel tracing, ops under
                                                                 `--pmc FETCH_SIZE` and under `--pmc WRITE_SIZE` (counters
                                                                 in runs of their own), traj with no profiler; each child
                                                                 under a time limit, stopping at the first failure

The steps before each window operation are the shape's own steps (at N = 60, m = 8: the exact-shape fast path, which
leaves P lower-only, as a trajectory does), so each operation sees the covariance a trajectory hands it.  --all writes
window_<shape>_kernel_stats.csv, window_<shape>_pmc.csv (per-dispatch FETCH_SIZE / WRITE_SIZE of the window kernels, with
the lower-triangle byte count N(N+1)/2 * 8 * B next to them) and window_times.csv.
"""
import argparse
import collections
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name: (k, m, B)
SHAPES = {
    "n60_b1024": (8, 8, 1024),
    "n60_b4096": (8, 8, 4096),
    "n198_b512": (31, 8, 512),
}
T_TRAJ = 50
TIMES_HEADER = "shape,N,m,B,T,loop_step_drop_clone_us,step_n_slide_us"
WINDOW_KERNELS = ("msckf_slide_kernel", "msckf_window_kernel", "slk_mirror_upper_kernel")


def setup(name):
    import numpy as np
    import torch
    from slkpkg import slk
    import scenarios as sc
    k, m, B = SHAPES[name]
    s = sc.synthetic_msckf(B, k, m=m, seed=0x51DE)
    rng = np.random.default_rng(2)
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    U = np.repeat(s["u"][None], T_TRAJ, axis=0)
    U[:, :, 0:3] += rng.normal(0, 0.01, (T_TRAJ, B, 3))
    Z = s["z"][None] + rng.normal(0, 0.02, (T_TRAJ, B, m))
    params = s["feat"].reshape(B, -1)
    ins = dict(U=d(U), Z=d(Z), Q=d(s["Q"]), R=d(s["R"]), P=d(params))
    ins["Pt"] = ins["P"].unsqueeze(0).expand(T_TRAJ, *params.shape)
    return slk, s, ins, (k, m, B)


def run_ops(name, reps):
    slk, s, ins, _ = setup(name)
    f = slk.Msckf(s["mean"], s["P"])

    def step(t):
        f.step(slk.PM_DELTA_POSE, ins["U"][t], ins["Q"], ins["Z"][t], slk.MM_FEATURE_PROJ, ins["P"], ins["R"])

    for t in range(2):                           # warm-up: every kernel of both sequences once
        step(t)
        f.slide(0)
        step(t)
        f.drop_clone(0)
        f.clone_pose()
    f.sync()
    for t in range(reps):
        step(t)
        f.slide(0)
    for t in range(reps):
        step(t)
        f.drop_clone(0)
        f.clone_pose()
    f.sync()
    f.close()
    print(f"ops {name} ok", flush=True)


def run_traj(name, reps, warmup):
    slk, s, ins, (k, m, B) = setup(name)
    f = slk.Msckf(s["mean"], s["P"])

    def loop():
        for t in range(T_TRAJ):
            f.step(slk.PM_DELTA_POSE, ins["U"][t], ins["Q"], ins["Z"][t], slk.MM_FEATURE_PROJ, ins["P"], ins["R"])
            f.drop_clone(0)
            f.clone_pose()

    def step_n():
        f.step_n(slk.PM_DELTA_POSE, ins["U"], ins["Q"], ins["Z"], slk.MM_FEATURE_PROJ, ins["Pt"], ins["R"], slide=0)

    res = []
    for fn in (loop, step_n):
        f.set_state(s["mean"], s["P"])
        for _ in range(warmup):
            fn()
        f.sync()
        f.timer_start()
        for _ in range(reps):
            fn()
        res.append(1e3 * f.timer_stop() / (reps * T_TRAJ))
    f.close()
    print(f"{name},{12 + 6 * k},{m},{B},{T_TRAJ},{res[0]:.2f},{res[1]:.2f}", flush=True)


def child(cmd, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(f"exit status {p.returncode}: {' '.join(cmd)}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}\n")
    return p


def pmc_rows(d):
    """per-dispatch mean of every counter of the window kernels in one counter run's directory"""
    fs = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    acc, n = collections.defaultdict(float), collections.Counter()
    for r in csv.DictReader(open(fs[0])):
        kn = next((w for w in WINDOW_KERNELS if w in r["Kernel_Name"]), None)
        if kn:
            acc[(kn, r["Counter_Name"])] += float(r["Counter_Value"])
            n[(kn, r["Counter_Name"])] += 1
    return {key: (acc[key] / n[key], n[key]) for key in acc}


def run_all(out_dir, reps, limit):
    os.makedirs(out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    times = [TIMES_HEADER]
    for name in SHAPES:
        k, m, B = SHAPES[name]
        N = 12 + 6 * k
        # kernel times
        tmp = tempfile.mkdtemp(prefix="win_")
        p = child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + me
                  + ["--shape", name, "--mode", "ops", "--reps", str(reps)], limit)
        if p.returncode != 0:
            return 1
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if stats:
            shutil.copy(stats[0], os.path.join(out_dir, f"window_{name}_kernel_stats.csv"))
        shutil.rmtree(tmp, ignore_errors=True)
        # counters, one per run
        rows = ["kernel,counter,per_dispatch,dispatches,lower_triangle_kB,whole_matrix_kB"]
        lower_kb = N * (N + 1) // 2 * 8 * B / 1024
        whole_kb = N * N * 8 * B / 1024
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            tmp = tempfile.mkdtemp(prefix="win_")
            p = child(["rocprofv3", "--pmc", ctr, "--output-format", "csv", "-d", tmp, "--"] + me
                      + ["--shape", name, "--mode", "ops", "--reps", "3"], limit)
            if p.returncode != 0:
                return 1
            for (kn, c), (v, cnt) in sorted(pmc_rows(tmp).items()):
                rows.append(f"{kn},{c},{v:.1f},{cnt},{lower_kb:.1f},{whole_kb:.1f}")
            shutil.rmtree(tmp, ignore_errors=True)
        with open(os.path.join(out_dir, f"window_{name}_pmc.csv"), "w") as fh:
            fh.write("\n".join(rows) + "\n")
        print("\n".join(rows), flush=True)
        # trajectories, no profiler
        p = child(me + ["--shape", name, "--mode", "traj"], limit)
        row = [ln for ln in p.stdout.splitlines() if ln.startswith(name + ",")]
        if p.returncode != 0 or not row:
            return 1
        times.append(row[0])
        print(row[0], flush=True)
    with open(os.path.join(out_dir, "window_times.csv"), "w") as fh:
        fh.write("\n".join(times) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--mode", choices=("ops", "traj"), default="traj")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child (--all)")
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.out, a.reps, a.limit))
    if not a.shape:
        ap.error("--shape or --all")
    if a.mode == "ops":
        run_ops(a.shape, a.reps)
    else:
        print(TIMES_HEADER)
        run_traj(a.shape, 5 if a.reps == 20 else a.reps, a.warmup)


if __name__ == "__main__":
    main()
