"""Cost of the Msckf EKF update from a registered model (slk_update_ekf_model) against what a caller had to do without
it, at the shape the tile kernel is measured on (N = 60, m = 128).  The state is reset before every timed call (not
timed); every figure is a median.

  kernel     update_ekf with device-resident zmean / H  (the EKF kernel alone); event-timed on the handle's stream
             (slk_timer_*), --warmup (10) + --calls (50) calls
  model      update_ekf_model, device-resident inputs   (linearisation launch + the same kernel); timed the same way
  host       mean download + numpy Jacobian + update_ekf on the host route: wall clock around the synchronised round
             trip (host work is what it measures), --warmup (10) + --calls (50) calls
  traj       step_n(update="ekf", slide=0), T steps in one call, against the loop of step_ekf + slide: wall clock
             around each synchronised pass of T (200) steps, 1 warm-up pass + --traj-passes (5) timed passes each way

--csv FILE appends one line per batch size."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--clones", type=int, default=8)
    ap.add_argument("--meas", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--traj-passes", type=int, default=5)
    ap.add_argument("--traj-steps", type=int, default=200)
    ap.add_argument("--no-traj", action="store_true")
    ap.add_argument("--csv")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda")
    torch.cuda.init()
    from slkpkg import slk
    import scenarios as sc
    import ekf_model_ref as ref
    k, m = args.clones, args.meas
    for B in args.batch:
        s = sc.synthetic_msckf(B, k, m=m, seed=99)
        N = s["N"]
        P = s["P"].reshape(B, N, N)
        p_h = s["feat"].reshape(B, -1)
        z, p, R = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (s["z"], p_h, s["R"]))
        f = slk.Msckf(s["mean"], P)
        zm, H = f.ekf_linearize(slk.MM_FEATURE_PROJ, p, m)
        Hs = H.transpose(1, 2)

        def timed(call, n):
            ts = []
            for i in range(args.warmup + n):
                f.set_state(s["mean"], P)                 # the same well-conditioned problem every time (not timed)
                f.sync()
                f.timer_start()
                call()
                t = f.timer_stop()
                if i >= args.warmup:
                    ts.append(t)
            return float(np.median(ts))
        t_kernel = timed(lambda: f.update_ekf(z, zm, Hs, R), args.calls)
        t_model = timed(lambda: f.update_ekf_model(z, slk.MM_FEATURE_PROJ, p, R), args.calls)
        applied = int((f.status() == 0).sum())

        def host_round_trip():
            mean = f.muState()
            zmh, Hh = ref.linearize_np(mean, s["feat"], k)
            f.update_ekf(s["z"], zmh, Hh, s["R"])
            f.sync()
        th = []
        for i in range(args.warmup + args.calls):
            f.set_state(s["mean"], P)
            f.sync()
            t0 = time.perf_counter()
            host_round_trip()
            if i >= args.warmup:
                th.append((time.perf_counter() - t0) * 1e3)
        t_host = float(np.median(th))
        line = (f"EKF from model N={N} m={m} B={B}: update_ekf (device zmean/H) {t_kernel:.4f} ms, update_ekf_model {t_model:.4f} ms "
                f"(+{t_model - t_kernel:.4f} ms = {100 * (t_model - t_kernel) / t_kernel:.2f} % of the kernel), host round trip "
                f"{t_host:.1f} ms = {t_host / t_model:.0f} x update_ekf_model, {applied}/{B} filters status 0")
        print(line)
        sps_n = sps_1 = float("nan")
        if not args.no_traj:
            T = args.traj_steps
            u0 = s["u"].copy()                                   # no motion: the landmarks stay in front of the clones
            u0[:, 0:3], u0[:, 3:7] = 0.0, (0.0, 0.0, 0.0, 1.0)   # that slide in, so every step is a well-posed update
            u = torch.from_numpy(u0).to(dev)
            Q = torch.from_numpy(s["Q"]).to(dev)
            uT, zT, pT = (a.unsqueeze(0).expand(T, *a.shape) for a in (u, z, p))
            tn, t1 = [], []
            for rep in range(1 + args.traj_passes):              # the first pass warms both ways up
                f.set_state(s["mean"], P)
                f.sync()
                t0 = time.perf_counter()
                f.step_n(slk.PM_DELTA_POSE, uT, Q, zT, slk.MM_FEATURE_PROJ, pT, R, gate=0, slide=0, update="ekf")
                f.sync()
                tn.append(time.perf_counter() - t0)
                f.set_state(s["mean"], P)
                f.sync()
                t0 = time.perf_counter()
                for _ in range(T):
                    f.step_ekf(slk.PM_DELTA_POSE, u, Q, z, slk.MM_FEATURE_PROJ, p, R, gate=False)
                    f.slide(0)
                f.sync()
                t1.append(time.perf_counter() - t0)
            sps_n, sps_1 = T / float(np.median(tn[1:])), T / float(np.median(t1[1:]))
            print(f"EKF trajectory N={N} m={m} B={B} T={T} slide=0: step_n(update='ekf') {sps_n:.1f} steps/s, "
                  f"loop of step_ekf + slide {sps_1:.1f} steps/s, {int((f.status() == 0).sum())}/{B} filters status 0")
        if args.csv:
            new = not os.path.exists(args.csv)
            with open(args.csv, "a") as fh:
                if new:
                    fh.write("N,m,B,update_ekf_ms,update_ekf_model_ms,linearize_percent,host_round_trip_ms,host_over_model,"
                             "step_n_ekf_steps_per_s,single_calls_steps_per_s\n")
                fh.write(f"{N},{m},{B},{t_kernel:.4f},{t_model:.4f},{100 * (t_model - t_kernel) / t_kernel:.2f},{t_host:.1f},"
                         f"{t_host / t_model:.1f},{sps_n:.1f},{sps_1:.1f}\n")
        f.close()


if __name__ == "__main__":
    main()
