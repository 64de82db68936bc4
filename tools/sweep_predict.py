"""Predict-only timing over the batch size, for the crossover of the one-wave and the two-filters-per-wave Msckf predict kernels:
   SLK_HIP_LIB=<library> python tools/sweep_predict.py [--clones 8] [--calls 200] [--reps 5] B1 B2 ...
Run it once per library (e.g. builds with -DSLK_PREDICT_PAIR_MIN_BATCH=1 and =1000000000: always / never the pair kernel);
prints one line per batch: the median and the minimum over the repetitions of the time per call (HIP events on the handle's
stream around `calls` back-to-back predicts, inputs device-resident, the state reset before every repetition)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batches", type=int, nargs="+")
    ap.add_argument("--clones", type=int, default=8)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from slkpkg import slk
    import scenarios as sc
    for B in a.batches:
        s = sc.synthetic_msckf(B, a.clones, m=8, seed=0x5EED0000)
        f = slk.Msckf(s["mean"], s["P"])
        u = torch.tensor(s["u"], device="cuda")
        Q = torch.tensor(s["Q"], device="cuda")
        torch.cuda.synchronize()
        per = []
        for r in range(a.reps + 1):
            f.set_state(s["mean"], s["P"])
            f.predict(slk.PM_DELTA_POSE, u, Q)
            f.sync()
            f.timer_start()
            for _ in range(a.calls):
                f.predict(slk.PM_DELTA_POSE, u, Q)
            ms = f.timer_stop()
            if r:                                               # (the first repetition warms up)
                per.append(1e3 * ms / a.calls)
        assert (f.status() == 0).all()
        f.close()
        print(f"{os.path.basename(os.environ.get('SLK_HIP_LIB', 'libslk_hip.so'))} k={a.clones} B={B}: "
              f"median {np.median(per):.2f} us  min {min(per):.2f} us per predict", flush=True)


if __name__ == "__main__":
    main()
