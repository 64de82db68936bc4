"""Times slk_nees / slk_sample_states (csrc/slk_consistency.hpp) at the shapes of a Monte-Carlo evaluation, next to what
the host-side alternative starts with: slk_get_state of P to (pageable) host memory at the same shape.

  python tools/bench_consistency.py --shape msckf_n60_full       one shape in this process: one CSV row on stdout
  python tools/bench_consistency.py --all --out profiles/        every shape, each in a child process of its own under
                                                                 `rocprofv3 --kernel-trace --stats` with a time limit;
                                                                 stops at the first failing shape

Inputs and outputs of the timed calls are device buffers (torch tensors on cuda:0), so the call time is the launch; the
handle's HIP events give the per-call time over --reps back-to-back calls (launch overhead included), rocprofv3's
kernel statistics the kernel durations alone.  --all writes consistency_<shape>_kernel_stats.csv per shape and
consistency_times.csv (the rows of every shape).
"""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name: (kind, k or (nfk, nfkl), B, op, range (t0, n) / S)
SHAPES = {
    "msckf_n60_full": ("msckf", 8, 4096, "nees", (0, None)),
    "msckf_n60_pose": ("msckf", 8, 4096, "nees", (0, 6)),
    "msckf_n198_full": ("msckf", 31, 512, "nees", (0, None)),
    "msckf_n12_full": ("msckf", 0, 1024, "nees", (0, None)),
    "usckf_n48_full": ("usckf", (3, 9), 4096, "nees", (0, None)),
    "sample_n60_s1": ("msckf", 8, 4096, "sample", 1),
    "sample_n60_s64": ("msckf", 8, 4096, "sample", 64),
}
HEADER = "shape,kind,N,B,op,n_or_S,call_us,get_P_host_ms,P_MB"


def run_one(name, reps, warmup):
    import numpy as np
    import torch
    from slkpkg import slk
    import scenarios as sc
    kind, shp, B, op, arg = SHAPES[name]
    if kind == "msckf":
        s = sc.synthetic_msckf(B, shp, seed=0xBE7C)
        f = slk.Msckf(s["mean"], s["P"])
    else:
        s = sc.synthetic_usckf(B, nfk=shp[0], nfkl=shp[1], seed=0xBE7C)
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=shp[0], nfkl=shp[1])
    N, Nq = f.N, f.Nq
    dev = torch.device("cuda", 0)
    lib, h = f._lib, f._h
    if op == "nees":
        t0, n = arg[0], (N if arg[1] is None else arg[1])
        truth = torch.from_numpy(s["mean"]).to(dev)
        out = torch.empty(B, dtype=torch.float64, device=dev)
        call = lambda: lib.slk_nees(h, truth.data_ptr(), t0, n, out.data_ptr(), None, slk.DEVICE)   # noqa: E731
        n_or_s = n
    else:
        S = arg
        torch.manual_seed(0)
        noise = torch.randn((B, S, N), dtype=torch.float64, device=dev)
        out = torch.empty((B, S, Nq), dtype=torch.float64, device=dev)
        call = lambda: lib.slk_sample_states(h, noise.data_ptr(), S, out.data_ptr(), slk.DEVICE)   # noqa: E731
        n_or_s = S
    torch.cuda.synchronize()
    for _ in range(warmup):
        assert call() == 0
    f.sync()
    f.timer_start()
    for _ in range(reps):
        assert call() == 0
    call_us = 1e3 * f.timer_stop() / reps
    P = np.empty((B, N, N))
    for _ in range(2):
        assert lib.slk_get_state(h, None, C.c_void_p(P.ctypes.data), slk.HOST) == 0
    t = time.perf_counter()
    for _ in range(reps):
        assert lib.slk_get_state(h, None, C.c_void_p(P.ctypes.data), slk.HOST) == 0
    get_ms = 1e3 * (time.perf_counter() - t) / reps
    f.close()
    print(f"{name},{kind},{N},{B},{op},{n_or_s},{call_us:.2f},{get_ms:.3f},{P.nbytes / 1e6:.1f}", flush=True)


def run_all(out_dir, reps, warmup, limit):
    os.makedirs(out_dir, exist_ok=True)
    rows = [HEADER]
    for name in SHAPES:
        tmp = tempfile.mkdtemp(prefix="cons_")
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
        stats = [os.path.join(d, fn) for d, _, fs in os.walk(tmp) for fn in fs if fn.endswith("kernel_stats.csv")]
        if stats:
            shutil.copy(stats[0], os.path.join(out_dir, f"consistency_{name}_kernel_stats.csv"))
        shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(out_dir, "consistency_times.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape (--all)")
    a = ap.parse_args()
    if a.all:
        sys.exit(run_all(a.out, a.reps, a.warmup, a.limit))
    if not a.shape:
        ap.error("--shape or --all")
    print(HEADER)
    run_one(a.shape, a.reps, a.warmup)


if __name__ == "__main__":
    main()
