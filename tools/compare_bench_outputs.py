"""Compare what `bench.py --dump-outputs DIR` wrote for two or more builds (same arguments, one rank), and measure each
build's distance to the CPU oracle run on the same filters for the same number of steps.

    python tools/compare_bench_outputs.py --steps 210 [--clones 8] [--meas 8] [--no-oracle] DIR_A DIR_B [DIR_C ...]

Every directory is compared with the first.  --steps is warm-up + timed steps of the bench runs.  The oracle needs no GPU.
Exit status 1 if `status` or `outliers` differ anywhere."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("filter_index", "mean", "P", "status", "outliers")}


def rel(a, b):
    """Per filter max |a - b| / max |b|, the measure of the GPU parity tests; the worst filter."""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return float((np.abs(a - b).max(axis=1) / np.maximum(1e-300, np.abs(b).max(axis=1))).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--clones", type=int, default=8)
    ap.add_argument("--meas", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("dirs", nargs="+")
    args = ap.parse_args()
    import bench
    outs = [load(d) for d in args.dirs]
    base, ok = outs[0], True
    idx = base["filter_index"].astype(np.int64)
    print(f"sampled filters: {len(idx)} of {args.batch}, {args.steps} steps")
    for d, o in zip(args.dirs[1:], outs[1:]):
        assert np.array_equal(o["filter_index"], base["filter_index"])
        same = np.array_equal(o["status"], base["status"]), np.array_equal(o["outliers"], base["outliers"])
        ok = ok and all(same)
        print(f"{d} vs {args.dirs[0]}: max rel diff P {rel(o['P'], base['P']):.3e}  mean {rel(o['mean'], base['mean']):.3e}  "
              f"bit-identical P {np.array_equal(o['P'], base['P'])} mean {np.array_equal(o['mean'], base['mean'])}  "
              f"status equal {same[0]}  outliers equal {same[1]}")
    st = base["status"].astype(np.int64)
    print(f"status_or {int(np.bitwise_or.reduce(st))}  filters with status != 0: {int(np.count_nonzero(st))}")
    if not args.no_oracle:
        from oracle import oracle as o
        import scenarios as sc
        o.build()
        k, m = args.clones, args.meas
        s = sc.synthetic_msckf(args.batch, k, m=m, seed=bench.SEED0)
        N, lay = s["N"], o.layout(o.MULTI, k)
        mean = np.ascontiguousarray(s["mean"][idx])
        P = np.ascontiguousarray(np.transpose(s["P"][idx], (0, 2, 1))).reshape(len(idx), -1)
        sto, out = o.msckf_step_batch(k, m, args.steps, mean, P, np.ascontiguousarray(s["u"][idx]), np.ascontiguousarray(s["feat"][idx]),
                                      np.ascontiguousarray(s["z"][idx]), s["Q"], s["R"])
        Po = np.ascontiguousarray(np.transpose(P.reshape(-1, N, N), (0, 2, 1)))
        print(f"CPU oracle: status_or {sto}")
        for d, g in zip(args.dirs, outs):
            dm = max(float(np.abs(o.boxminus(lay, g["mean"][b], mean[b])).max()) for b in range(len(idx)))
            print(f"{d} vs CPU oracle: P {rel(g['P'], Po):.3e}  mean {dm:.3e}")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
