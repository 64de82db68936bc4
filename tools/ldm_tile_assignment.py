"""Tile-to-wave maps of the exact-shape factor update L' = L M (csrc/slk_step_fast.hpp, ldm_product_tiled), by enumeration.

Output tile (I, J) of the lower triangle needs M(Kb, J), Kb = J .. I: two matrix instructions per M tile, formed ONCE per
wave and tile column, and four per (tile, Kb) for the product with L(I, Kb).  With JB = the last tile column any
measurement row depends on, tile columns and k-blocks beyond JB are skipped.  Cost of a wave:

    sum over its tile columns J <= JB of  2 (min(Imax(J), JB) - J + 1)  +  4 sum over its tiles (min(I, JB) - J + 1)

The search: fewest matrix instructions in all with nothing skipped (JB = NT - 1), no wave longer than `cap` there and none
holding more than `maxt` accumulators; ties by the longest wave, then the total, at the given JB of interest, then by the
longest wave with nothing skipped.

    python3 tools/ldm_tile_assignment.py            # NT = 4 (cap 30, JB 2: the benchmark) and NT = 3 (cap 18)
"""
import itertools


def tiles(nt):
    return [(i, j) for i in range(nt) for j in range(i + 1)]


def wave_costs(nt, assign, jb):
    cost = [0, 0, 0, 0]
    for w in range(4):
        for j in range(min(jb, nt - 1) + 1):
            rows = [i for (i, jj), ww in assign.items() if ww == w and jj == j]
            if not rows:
                continue
            cost[w] += 2 * (min(max(rows), jb) - j + 1) + 4 * sum(min(i, jb) - j + 1 for i in rows)
    return cost


def search(nt, cap, maxt, jb_focus):
    ts = tiles(nt)
    best, best_key = None, None
    for ws in itertools.product(range(4), repeat=len(ts)):
        if max(ws.count(w) for w in range(4)) > maxt:
            continue
        a = dict(zip(ts, ws))
        full = wave_costs(nt, a, nt - 1)
        if max(full) > cap:
            continue
        foc = wave_costs(nt, a, jb_focus)
        key = (sum(full), max(foc), sum(foc), max(full))
        if best_key is None or key < best_key:
            best, best_key = a, key
    return best


def show(nt, a):
    for w in range(4):
        print("  wave %d: %s" % (w, ", ".join("(%d,%d)" % t for t in sorted(a, key=lambda t: (t[1], -t[0])) if a[t] == w)))
    for jb in range(nt - 1, -1, -1):
        c = wave_costs(nt, a, jb)
        print("  JB = %d: %s = %d" % (jb, " / ".join(map(str, c)), sum(c)))


if __name__ == "__main__":
    for nt, cap, maxt, jb in ((4, 30, 3, 2), (3, 18, 3, 2)):
        print("NT = %d (no wave above %d with nothing skipped, at most %d tiles per wave)" % (nt, cap, maxt))
        show(nt, search(nt, cap, maxt, jb))
