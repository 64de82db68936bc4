"""Throughput of the batched Usckf path (BASELINE config 1 shape: N = 48, m = 3, SPD variant).

usage: python tools/bench_usckf.py [--nfk A] [--nfkl B] [--model vo|feature_proj] [--features F] [--no-cpu] [batch ...]
(default 3 + 9 features: N = 48, m = 3; the state is N = 36 + A + B and the update has m = A rows, MM_VO_RELATIVE, or
m = 2F rows, MM_FEATURE_PROJ with F features seen from poses 0, 1, 2 in turn -- N > 96 runs the predict on the
global-workspace kernel, and N > 96 or m > 32 the update on the wide kernel)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    from slkpkg import slk
    import scenarios as sc
    from oracle import oracle as o
    ap = argparse.ArgumentParser()
    ap.add_argument("--nfk", type=int, default=3)
    ap.add_argument("--nfkl", type=int, default=9)
    ap.add_argument("--model", choices=("vo", "feature_proj"), default="vo")
    ap.add_argument("--features", type=int, default=17)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU oracle rate")
    ap.add_argument("batches", type=int, nargs="*")
    args = ap.parse_args()
    nfk, nfkl, N = args.nfk, args.nfkl, 36 + args.nfk + args.nfkl
    fp = args.model == "feature_proj"
    m = 2 * args.features if fp else nfk
    batches = args.batches or [1024, 4096, 16384]
    for B in batches:
        s = sc.synthetic_usckf(B, nfk=nfk, nfkl=nfkl)
        f = slk.Usckf(mean=s["mean"], P=s["P"], nfk=nfk, nfkl=nfkl)
        dev = torch.device("cuda")
        u = torch.from_numpy(s["u"]).to(dev)
        mm, params, zz, RR = slk.MM_VO_RELATIVE, None, s["z"], s["R"]
        if fp:
            feat, zz = sc.usckf_features(s["mean"], poses=tuple(i % 3 for i in range(args.features)))
            mm, params, RR = slk.MM_FEATURE_PROJ, torch.from_numpy(feat.reshape(B, -1)).to(dev), 0.01 * np.eye(m)
        z = torch.from_numpy(np.ascontiguousarray(zz)).to(dev)
        Q = torch.from_numpy(np.ascontiguousarray(s["Q"].T)).to(dev)
        R = torch.from_numpy(np.ascontiguousarray(RR.T)).to(dev)
        for _ in range(5):
            f.step(slk.PM_CONST_VELOCITY, u, Q, z, mm, params, R)
        f.sync()
        K = 100
        f.timer_start()
        for _ in range(K):
            f.step(slk.PM_CONST_VELOCITY, u, Q, z, mm, params, R)
        ms = f.timer_stop() / K
        bad = int(np.count_nonzero(f.status()))
        print(f"Usckf N={N} m={m} B={B}: {B / ms * 1e3:.3e} filter-steps/s, {ms:.4f} ms/step, filters with status {bad}")
    if args.no_cpu or fp:
        return
    s = sc.synthetic_usckf(64, nfk=nfk, nfkl=nfkl)
    t0 = time.perf_counter()
    n = 0
    for b in range(64):
        g = o.Usckf(nfk=nfk, nfkl=nfkl, mean=s["mean"][b], P=s["P"][b])
        uu = s["u"][b]
        pm = o.pm_const_velocity(uu[0:3], uu[3:6], uu[6])
        for _ in range(20):
            g.predict(pm, s["Q"])
            g.update(s["z"][b], o.mm_vo_relative(), s["R"])
            n += 1
    dt = time.perf_counter() - t0
    print(f"CPU oracle (1 thread, includes ctypes call overhead): {n / dt:.1f} filter-steps/s")


if __name__ == "__main__":
    main()
