"""Times slk_ensemble_moments / slk_gather_states (csrc/slk_ensemble.hpp) at the shapes of a filter bank, next to what
the host-side alternative starts with: slk_get_state of P to (pageable) host memory at the same shape.

  python tools/bench_ensemble.py --shape moments_n60_full_g1_mix   one shape in this process: one CSV row on stdout
  python tools/bench_ensemble.py --all --out profiles/             every shape, each in a child process of its own under
                                                                   `rocprofv3 --kernel-trace --stats` with a time limit;
                                                                   stops at the first failing shape

Inputs and outputs of the timed calls are device buffers (torch tensors on cuda:0).  The handle's HIP events give the
per-call time over --reps back-to-back calls after --warmup (launch overhead included); rocprofv3's kernel statistics
give the kernel durations alone: --all sums the average durations of the call's kernels (ens_* / gather_states_kernel) into
kernel_us, splits out the mean-covariance pass and the spread pass, and sets the streaming pass against its algorithmic
bytes B n (n + 1) / 2 * 8 (the gather: bytes read plus written).  --all writes ensemble_<shape>_kernel_stats.csv per
shape and ensemble_times.csv (the rows of every shape).
"""
import argparse
import csv
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

COPY_RATE = 6.29e12      # bytes / s: the measured device copy rate the streaming passes are set against


def _moments(kind, shp, B, rng, G, mode):
    return (kind, shp, B, "moments", dict(range=rng, G=G, mode=mode))


# name: (kind, k or (nfk, nfkl), B, op, arguments)
SHAPES = {}
for _rng, _rn in (((0, None), "full"), ((0, 6), "pose")):
    for _G in (1, 8):
        for _mode in ("mix", "err"):
            SHAPES[f"moments_n60_{_rn}_g{_G}_{_mode}"] = _moments("msckf", 8, 4096, _rng, _G, _mode)
SHAPES["moments_n198_full_g1_mix"] = _moments("msckf", 31, 512, (0, None), 1, "mix")
SHAPES["moments_n12_full_g1_mix"] = _moments("msckf", 0, 1024, (0, None), 1, "mix")
SHAPES["moments_usckf_n48_full_g1_mix"] = _moments("usckf", (3, 9), 4096, (0, None), 1, "mix")
for _nm, _kind, _shp, _B in (("n60", "msckf", 8, 4096), ("n198", "msckf", 31, 512), ("n12", "msckf", 0, 1024),
                             ("usckf_n48", "usckf", (3, 9), 4096)):
    SHAPES[f"gather_{_nm}_complete"] = (_kind, _shp, _B, "gather", dict(lower=False))
    if _nm in ("n60", "usckf_n48"):                      # the shapes whose steps leave P lower-only
        SHAPES[f"gather_{_nm}_lower"] = (_kind, _shp, _B, "gather", dict(lower=True))
HEADER = "shape,kind,N,B,op,n,G,mode,call_us,get_P_host_ms,P_MB,algorithmic_MB"
EXTRA = ",kernel_us,meancov_us,spread_us,stream_fraction_of_copy_rate,beats_get_P"


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
    if op == "moments":
        t0, n = arg["range"][0], (N if arg["range"][1] is None else arg["range"][1])
        G, mode = arg["G"], arg["mode"]
        # a bank as the tests build it (tests/ensemble_ref.py): every group drawn around its first filter with the
        # scenario's covariance, rotations up to 0.3 rad apart, so that the centre iteration makes its usual passes
        import ensemble_ref as er
        bank_name = {("msckf", 8): "msckf_n60", ("msckf", 31): "msckf_n198", ("msckf", 0): "msckf_n12",
                     ("usckf", (3, 9)): "usckf_n48"}[(kind, shp)]
        f.set_state(er.bank(bank_name, G, seed=0xBE7C, B=B)["mean"], None)
        torch.manual_seed(0)
        w = torch.rand(B, dtype=torch.float64, device=dev) + 0.1
        truth = torch.from_numpy(s["mean"]).to(dev) if mode == "err" else None
        cen = torch.empty((G, n if mode == "err" else Nq), dtype=torch.float64, device=dev)
        spr, cov = (torch.empty((G, n, n), dtype=torch.float64, device=dev) for _ in range(2))
        ess = torch.empty(G, dtype=torch.float64, device=dev)
        call = lambda: lib.slk_ensemble_moments(h, G, w.data_ptr(), truth.data_ptr() if truth is not None else None, t0, n,  # noqa: E731
                                                cen.data_ptr(), spr.data_ptr(), cov.data_ptr(), ess.data_ptr(), slk.DEVICE)
        alg = B * n * (n + 1) // 2 * 8
    else:
        n, G, mode = N, 1, "lower" if arg["lower"] else "complete"
        if arg["lower"]:
            if kind == "msckf":
                f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
            else:
                f.step(slk.PM_CONST_VELOCITY, s["u"], s["Q"], s["z"], slk.MM_VO_RELATIVE, None, s["R"])
        src = torch.randint(0, B, (B,), dtype=torch.int32, device=dev)
        call = lambda: lib.slk_gather_states(h, src.data_ptr(), slk.DEVICE)   # noqa: E731
        alg = 2 * 8 * B * (Nq + (N * (N + 1) // 2 if arg["lower"] else N * N))
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
    print(f"{name},{kind},{N},{B},{op},{n},{G},{mode},{call_us:.2f},{get_ms:.3f},{P.nbytes / 1e6:.1f},{alg / 1e6:.2f}", flush=True)


def kernel_times(stats_csv, ncalls):
    """duration (us) per call of each of the call's own kernels: total over the run / calls made (warm-up included; a
    kernel may run more than once per call, as the final reduce does)"""
    out = {}
    with open(stats_csv) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name", "")
            if "ens_" in name or "gather_states_kernel" in name:
                out[name] = float(r["TotalDurationNs"]) / 1e3 / ncalls
    return out


def run_all(out_dir, reps, warmup, limit):
    os.makedirs(out_dir, exist_ok=True)
    rows = [HEADER + EXTRA]
    for name in SHAPES:
        tmp = tempfile.mkdtemp(prefix="ens_")
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
               "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--shape", name, "--reps", str(reps),
               "--warmup", str(warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        row = [ln for ln in p.stdout.splitlines() if ln.startswith(name + ",")]
        if p.returncode != 0 or not row:
            sys.stderr.write(f"{name}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}\n")
            return 1
        stats = [os.path.join(d, fn) for d, _, fs in os.walk(tmp) for fn in fs if fn.endswith("kernel_stats.csv")]
        extra = ",,,,,"
        if stats:
            shutil.copy(stats[0], os.path.join(out_dir, f"ensemble_{name}_kernel_stats.csv"))
            kt = kernel_times(stats[0], reps + warmup)
            total = sum(kt.values())
            cov = sum(v for k, v in kt.items() if "meancov" in k)
            spread = sum(v for k, v in kt.items() if "spread" in k)
            cols = row[0].split(",")
            alg, get_ms = float(cols[11]) * 1e6, float(cols[9])
            stream = cov if cols[4] == "moments" else total
            frac = alg / (stream * 1e-6) / COPY_RATE if stream > 0 else float("nan")
            extra = f",{total:.2f},{cov:.2f},{spread:.2f},{frac:.3f},{int(total * 1e-3 < get_ms)}"
        rows.append(row[0] + extra)
        print(rows[-1], flush=True)
        shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(out_dir, "ensemble_times.csv"), "w") as fh:
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
