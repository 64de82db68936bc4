"""Feature-track update (slk_update_tracks) at k = 8, M = 9, J = 8, m = 120: its time with and without the gate, and the
yardstick it replaces -- slk_get_state, the numpy twin of tests/tracks_ref.py on the host, slk_update_ekf(SLK_HOST).
The twin is timed on the first --twin-filters filters and scaled to the batch (it is a per-filter Python loop).
`--profile` only runs the device calls (for rocprofv3 --kernel-trace --stats); otherwise one CSV line is printed:
    python tools/bench_tracks.py --batch 1024 [--iters 20] [--profile]"""
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--twin-filters", type=int, default=32)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from slkpkg import slk
    import tracks_ref as tr

    k, M, J, m, B = 8, 9, 8, 120, a.batch
    small = tr.scenario(k, M, J, m, B=a.twin_filters)
    reps = -(-B // a.twin_filters)
    s = {key: (np.ascontiguousarray(np.concatenate([v] * reps)[:B]) if key in ("mean", "P", "tracks") else v) for key, v in small.items()}
    chi2 = tr.CHI2_95[:2 * M - 2]
    td, cd, sd = torch.from_numpy(s["tracks"]).cuda(), torch.from_numpy(chi2).cuda(), torch.tensor([s["sigma"]], dtype=torch.float64).cuda()
    z0, I = torch.zeros((B, m), dtype=torch.float64).cuda(), torch.eye(m, dtype=torch.float64).cuda()
    times = {}
    for name in ("update_tracks", "update_tracks_gated", "update_ekf"):
        f = slk.Msckf(s["mean"], s["P"])
        r, H, _ = f.track_linearize(td, sd, m)
        Hc = H.transpose(1, 2)

        def call():
            if name == "update_ekf":
                f.update_ekf(r, z0, Hc, I, gate=False)
            else:
                f.update_tracks(td, sd, m, chi2=cd if name.endswith("gated") else None)
        call()
        f.sync()
        t0 = time.perf_counter()
        for _ in range(a.iters):                              # (the state moves on: the same work every time)
            call()
        f.sync()
        times[name] = (time.perf_counter() - t0) / a.iters * 1e3
    if a.profile:
        return
    # the host round trip of the parent commit: state down, twin, rows up
    f = slk.Msckf(s["mean"], s["P"])
    t0 = time.perf_counter()
    mean, P = f.muState(), f.getPk()
    t1 = time.perf_counter()
    out = [tr.linearize_np(mean[b], P[b], s["tracks"][b], s["sigma"], k, m, chi2) for b in range(a.twin_filters)]
    t2 = time.perf_counter()
    r = np.concatenate([np.stack([o[0] for o in out])] * reps)[:B]
    H = np.concatenate([np.stack([o[1] for o in out])] * reps)[:B]
    t3 = time.perf_counter()
    f.update_ekf(r, np.zeros((B, m)), H, np.eye(m), gate=False)
    f.sync()
    t4 = time.perf_counter()
    host = ((t1 - t0) + (t2 - t1) * B / a.twin_filters + (t4 - t3)) * 1e3
    print("N,m,J,M,B,update_ekf_ms,update_tracks_ms,update_tracks_gated_ms,get_state_ms,twin_ms_scaled,update_ekf_host_ms,"
          "host_round_trip_ms,host_over_update_tracks_gated,transfers_over_update_tracks_gated")
    print(f"{12 + 6 * k},{m},{J},{M},{B},{times['update_ekf']:.4f},{times['update_tracks']:.4f},{times['update_tracks_gated']:.4f},"
          f"{(t1 - t0) * 1e3:.1f},{(t2 - t1) * B / a.twin_filters * 1e3:.1f},{(t4 - t3) * 1e3:.1f},{host:.1f},"
          f"{host / times['update_tracks_gated']:.1f},{((t1 - t0) + (t4 - t3)) * 1e3 / times['update_tracks_gated']:.1f}")


if __name__ == "__main__":
    main()
