"""DIAGNOSTIC: per-phase cycles of the exact-shape fast path (slk_step_fast.hpp) from in-kernel stamps (a -DSLK_STAMPS build).
    python tools/phase_profile_fast.py --lib ab/NAME.so [--batch 4096] [--clones 8]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STAMPS = [(0, "entry"), (3, "load + first factorisation (wave 0), mean, small arrays"), (4, "Z = h(X), zbar, innovation: wave 0's, behind its factorisation"), (6, "S (wave 0)"), (7, "gate"),
          (8, "x, b, delta (wave 0) | scan + columns (wave 3)"), (11, "factor update L M"), (12, "mean loop"),
          (13, "correction, odd / even split, mean out"), (14, "rebuild MFMA"), (15, "rank-2 + store")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--clones", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--lib", required=True)
    args = ap.parse_args()
    import torch
    from slkpkg import slk
    import scenarios as sc
    lib = slk.load_library(os.path.join(ROOT, args.lib))
    slk._lib = lib
    lib.slk_debug_set_stamps.argtypes = [C.c_void_p]
    B, k = args.batch, args.clones
    s = sc.synthetic_msckf(B, k, m=8)
    f = slk.Msckf(s["mean"], s["P"])
    dbg = torch.zeros((B, 32), dtype=torch.int64, device="cuda")
    lib.slk_debug_set_stamps(dbg.data_ptr())
    for _ in range(args.steps):
        f.step(slk.PM_DELTA_POSE, s["u"], s["Q"], s["z"], slk.MM_FEATURE_PROJ, s["feat"], s["R"])
    f.sync()
    t = dbg.cpu().numpy().astype(np.float64)
    ok = t[:, 15] > 0
    print(f"filters through the fast path to the end: {int(ok.sum())} / {B}; mean-loop passes: {np.bincount(t[ok][:, 20].astype(int))}")
    tot = np.median(t[ok][:, 15] - t[ok][:, 0])
    print(f"median cycles per filter (s_memtime ticks): {tot:.0f}")
    prev = 0
    for i, name in STAMPS[1:]:
        d = np.median(t[ok][:, i] - t[ok][:, prev])
        print(f"  {name:52s} {d:9.0f}  {100 * d / tot:5.1f} %")
        prev = i
    x = t[ok]
    if (x[:, 23] > 0).all():
        m = lambda a, b: np.median(x[:, a] - x[:, b])
        print(f"  wave 3: at its columns {m(22, 7):.0f} after the gate; block bases + columns {m(23, 22):.0f}")
        print(f"  wave 0: x = S^-1 nu {m(24, 7):.0f} after the gate; b, delta = L b, reference {m(25, 24):.0f}; waits for wave 3 {m(8, 25):.0f}")
    # early h(X): wave 0 releases finished columns of the factor behind the steps of the release plan (fast_release_plan,
    # csrc/slk_math.hpp).  It reaches / leaves the barrier A (or the only one) at the slots 1 / 2, B at 9 / 10, C at 5 / 31: the
    # difference is its wait for a released wave that is late.  Wave 1 evaluates its features from A on (19 = the start of its
    # first pass, 21 = the end of its last one), wave 0 -- single release, fewer than three steps behind it -- behind its last
    # step (17 .. 18; stamp 3 = the end of its factorisation).  Slot 16 = the end of S on wave 1, early (behind C) or not.
    # (a build from before the staggered release: one release, stamped at slot 16)
    if (x[:, 2] > 0).all() and (x[:, 21] > 0).all():
        for name, pre, post in (("A", 1, 2), ("B", 9, 10), ("C", 5, 31)):
            sel = x[:, post] > 0
            if sel.any():
                y = x[sel]
                print(f"  wave 0: barrier {name} on {int(sel.sum())} filters, {np.median(y[:, post] - y[:, 0]):.0f} after entry, "
                      f"{np.median(y[:, 3] - y[:, post]):.0f} before its factorisation ends; it waits {np.median(y[:, post] - y[:, pre]):.0f} there")
        last = np.where(x[:, 10] > 0, x[:, 10], x[:, 2])         # the release behind which the last h(X) starts
        print(f"  wave 1: h(X) starts {m(19, 2):.0f} after the first release, its last pass ends {np.median(x[:, 21] - last):.0f} after the last "
              f"feature release, {m(3, 21):.0f} before wave 0's factorisation ends")
        print(f"  phase 1 behind the factorisation: {m(4, 3):.0f} (stamp 3 to the closing barrier)")
        early = x[:, 31] > 0
        if early.any():
            y = x[early]
            print(f"  early S on {int(early.sum())} filters: starts behind C, takes {np.median(y[:, 16] - y[:, 31]):.0f}, ends "
                  f"{np.median(y[:, 3] - y[:, 16]):.0f} before wave 0's factorisation ends; S behind the closing barrier: {np.median(y[:, 6] - y[:, 4]):.0f}")
        if (~early).any():
            y = x[~early]
            print(f"  S behind the closing barrier on {int((~early).sum())} filters: {np.median(y[:, 6] - y[:, 4]):.0f}")
        if (x[:, 18] > 0).all():
            print(f"  wave 0: h(X) starts {m(17, 3):.0f} after its factorisation, takes {m(18, 17):.0f}; the closing barrier {m(4, 18):.0f}")
    elif (x[:, 16] > 0).all() and (x[:, 21] > 0).all():
        print(f"  wave 0: releases the factor {m(16, 0):.0f} after entry, {m(3, 16):.0f} before its factorisation ends")
        print(f"  wave 1: h(X) starts {m(19, 16):.0f} after the release, takes {m(21, 19):.0f}, is done {m(3, 21):.0f} before wave 0's factorisation ends")
        print(f"  phase 1 behind the factorisation: {m(4, 3):.0f} (stamp 3 to the closing barrier); S: {m(6, 4):.0f}")
        if (x[:, 18] > 0).all():
            print(f"  wave 0: h(X) starts {m(17, 3):.0f} after its factorisation, takes {m(18, 17):.0f}; the closing barrier {m(4, 18):.0f}")
        else:
            print(f"  wave 0: no feature of its own; the closing barrier {m(4, 3):.0f} after its factorisation")
    # which waves left the direct SO(3) series in the first mean-loop pass (bit 0 exp, bit 1 log; wave 1: bits 2 / 3 = its second round)
    for w, slot in enumerate((26, 27, 29, 30)):
        print(f"  mean loop, wave {w}: angle-halving exp / log codes {np.bincount(x[:, slot].astype(int), minlength=4)}")


if __name__ == "__main__":
    main()
