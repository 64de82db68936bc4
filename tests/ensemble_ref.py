"""numpy fp64 twin of slk_ensemble_moments / slk_gather_states, built on the CPU oracle's manifold operators
(oracle.boxminus / oracle.boxplus), and the inputs the ensemble tests share.  The twin follows the definitions of
include/slk.h literally, the pinned mixture iteration included: ref = the mean of the group's first filter; one pass is
dbar = sum w_b (mu_b [-] ref), ref <- ref [+] dbar; stop after the pass with |dbar| <= 1e-12, or after 100 passes.
"""
import numpy as np

from oracle import oracle as o
import scenarios as sc

# (name, kind, layout arguments, B): the shapes of the GPU tests
SHAPES = [
    ("msckf_n12", "msckf", dict(k=0), 1024),
    ("msckf_n60", "msckf", dict(k=8), 4096),
    ("msckf_n198", "msckf", dict(k=31), 512),
    ("msckf_n210", "msckf", dict(k=33), 256),           # the global route of the step kernels
    ("usckf_n48", "usckf", dict(nfk=3, nfkl=9), 512),
    ("usckf_n164", "usckf", dict(nfk=30, nfkl=98), 128),
]
SHAPE_IDS = [s[0] for s in SHAPES]
WEIGHT_KINDS = ["uniform", "random", "zeros", "onehot"]
ROT_SPREAD = 0.3                                        # rad: the most two members of a group differ by, per rotation


def layout_of(kind, args):
    return o.layout(o.MULTI, args["k"]) if kind == "msckf" else o.layout(o.AUGMENTED, 0, args["nfk"], args["nfkl"])


def so3_toffs(lay):
    return [3] + [12 + 6 * c + 3 for c in range(lay.k)] if lay.kind == o.MULTI else [12 * s + 3 for s in range(3)]


def group_counts(B):
    return [1, 8, B]


def ranges(lay):
    N = o.dof(lay)
    last = (N - 6, 6) if lay.kind == o.MULTI and lay.k > 0 else (N - 12, 12)      # the last clone / the last block
    return [(0, N), (0, 6), (3, 3), (4, 5), (7, 1), last]                           # (4, 5) = [4, 9) cuts SO(3) blocks


def scenario(kind, args, B, seed):
    return sc.synthetic_msckf(B, args["k"], seed=seed) if kind == "msckf" else \
        sc.synthetic_usckf(B, nfk=args["nfk"], nfkl=args["nfkl"], seed=seed)


def bank(name, groups, seed=0xE5E, B=None):
    """The filters of shape `name` in `groups` groups: every group is one scenario filter (tests/scenarios.py) and draws
    mu [+] L n around it with the scenario's own covariance, each rotation block of L n clipped to ROT_SPREAD / 2 so
    that two members of a group are at most ROT_SPREAD apart.  The covariances are the scenario's, one per filter.
    Returns dict(lay, B, N, Nq, mean [B, Nq], P [B, N, N]).  B: another batch size than the shape's own."""
    _, kind, args, B0 = SHAPES[SHAPE_IDS.index(name)]
    B = B0 if B is None else B
    lay = layout_of(kind, args)
    N, Bg = o.dof(lay), B // groups
    full = scenario(kind, args, B, seed)
    rng = np.random.default_rng(seed + groups)
    mean = np.empty_like(full["mean"])
    for g in range(groups):
        base = mean[g * Bg] = full["mean"][g * Bg]
        L = np.linalg.cholesky(full["P"][g * Bg]) if Bg > 1 else None
        for b in range(1, Bg):
            d = L @ rng.normal(0, 1, N)
            for t in so3_toffs(lay):
                r = np.linalg.norm(d[t:t + 3])
                if r > ROT_SPREAD / 2:
                    d[t:t + 3] *= ROT_SPREAD / 2 / r
            mean[g * Bg + b] = o.boxplus(lay, base, d)
    return dict(lay=lay, kind=kind, args=args, B=B, N=N, Nq=o.storage(lay), mean=np.ascontiguousarray(mean), P=full["P"])


def step_inputs(name, groups, B, seed=0x57E9):
    """A bank of B filters with the process and measurement inputs of one step around its means (the scenario's inputs,
    the measurements redrawn for the bank's means): (bank, scenario dict for step())."""
    b = bank(name, groups, seed, B)
    s = dict(scenario(b["kind"], b["args"], B, seed))
    s["mean"] = b["mean"]
    if b["kind"] == "msckf":
        s["feat"], s["z"] = sc.msckf_features(b["mean"], b["args"]["k"], s["m"] // 2, np.random.default_rng(seed + 1))
    else:
        s["z"] = b["mean"][:, 39:39 + b["args"]["nfk"]] + np.random.default_rng(seed + 1).normal(0, 0.1, (B, b["args"]["nfk"]))
    return b, s


def weights_of(kind, B, groups, seed=0x3E1):
    """uniform -> None; random; random with about a third zeros; one filter per group (not the first)."""
    if kind == "uniform":
        return None
    rng = np.random.default_rng(seed + groups)
    Bg = B // groups
    if kind == "random":
        return rng.uniform(0.1, 2.0, B)
    if kind == "zeros":
        w = rng.uniform(0.1, 2.0, B)
        w[rng.uniform(0, 1, B) < 0.33] = 0.0
        return w
    w = np.zeros(B)
    w[np.arange(groups) * Bg + Bg // 3] = 1.0
    return w


def truth_of(b, seed=0x7A07):
    """truth_b = mu_b [+] L_b n: an error whose covariance is the filter's own"""
    rng = np.random.default_rng(seed)
    lay, N = b["lay"], b["N"]
    L = np.linalg.cholesky(b["P"])
    return np.stack([o.boxplus(lay, b["mean"][i], L[i] @ rng.normal(0, 1, N)) for i in range(b["B"])])


def normalised_weights(weights, B, groups):
    """(w~ [B], ess [G]); NaN for a group with a negative or non-finite weight or a sum that is not > 0"""
    Bg = B // groups
    w = np.ones(B) if weights is None else np.asarray(weights, dtype=np.float64)
    wn, ess = np.empty(B), np.empty(groups)
    for g in range(groups):
        wg = w[g * Bg:(g + 1) * Bg]
        s = wg.sum()
        if not np.isfinite(wg).all() or (wg < 0).any() or not (s > 0) or not np.isfinite(s):
            wn[g * Bg:(g + 1) * Bg], ess[g] = np.nan, np.nan
        else:
            wn[g * Bg:(g + 1) * Bg], ess[g] = wg / s, s * s / (wg * wg).sum()
    return wn, ess


def manifold_mean(lay, mus, w):
    """the pinned iteration; returns (centre [Nq], passes made)"""
    ref = mus[0].copy()
    for p in range(100):
        dbar = np.zeros(o.dof(lay))
        for b in range(mus.shape[0]):
            dbar += w[b] * o.boxminus(lay, mus[b], ref)
        ref = o.boxplus(lay, ref, dbar)
        if np.linalg.norm(dbar) <= 1e-12:
            break
    return ref, p + 1


class Twin:
    """The filter-by-filter work of one (mean, weights, truth, groups), over the whole state: any range is a slice."""

    def __init__(self, lay, mean, weights=None, truth=None, groups=1):
        self.lay, self.G = lay, groups
        B, N = mean.shape[0], o.dof(lay)
        self.B, self.Bg, self.N = B, B // groups, N
        self.wn, self.ess = normalised_weights(weights, B, groups)
        self.error_mode = truth is not None
        self.passes = np.zeros(groups, dtype=int)
        self.bad = np.isnan(self.ess)
        self.D = np.full((B, N), np.nan)
        self.centre = np.full((groups, N if self.error_mode else mean.shape[1]), np.nan)
        for g in range(groups):
            if self.bad[g]:
                continue
            sl = slice(g * self.Bg, (g + 1) * self.Bg)
            if self.error_mode:
                self.D[sl] = [o.boxminus(lay, truth[b], mean[b]) for b in range(sl.start, sl.stop)]
                self.centre[g] = self.wn[sl] @ self.D[sl]
            else:
                self.centre[g], self.passes[g] = manifold_mean(lay, mean[sl], self.wn[sl])
                self.D[sl] = [o.boxminus(lay, mean[b], self.centre[g]) for b in range(sl.start, sl.stop)]

    def moments(self, P, t0, n):
        """dict(center, spread, mean_cov, ess) as slk_ensemble_moments defines them on [t0, t0 + n)"""
        G, Bg = self.G, self.Bg
        spread, mean_cov = np.full((G, n, n), np.nan), np.full((G, n, n), np.nan)
        for g in range(G):
            if self.bad[g]:
                continue
            sl = slice(g * Bg, (g + 1) * Bg)
            d = self.D[sl, t0:t0 + n]
            if self.error_mode:
                d = d - self.centre[g, t0:t0 + n]
            spread[g] = (d * self.wn[sl, None]).T @ d
            mean_cov[g] = np.einsum("b,bij->ij", self.wn[sl], P[sl, t0:t0 + n, t0:t0 + n])
        center = self.centre[:, t0:t0 + n] if self.error_mode else self.centre
        return dict(center=center, spread=spread, mean_cov=mean_cov, ess=self.ess)


def moments(lay, mean, P, weights=None, truth=None, t0=0, n=None, groups=1):
    n = o.dof(lay) - t0 if n is None else n
    return Twin(lay, mean, weights, truth, groups).moments(P, t0, n)


def gather(mean, P, status, outliers, src):
    """what slk_gather_states leaves: a host index"""
    src = np.asarray(src)
    return mean[src], P[src], status[src], outliers[src]


# ------------------------------------------------------------------ the derived tolerances of the GPU tests
SPREAD_ZERO = 1e-24      # what the issue counts as an all-zero spread ("all zeros to 1e-24 absolute")


def assert_moment_close(got, ref, M, what, rel=1e-10, floor=0.0):
    """|got_ij - ref_ij| <= rel sqrt(M_ii M_jj) (+ floor) per group; NaN exactly where the twin has NaN"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), f"{what}: NaN pattern differs"
    d = np.sqrt(np.abs(np.einsum("gii->gi", M)))
    bound = rel * (d[:, :, None] * d[:, None, :] if got.ndim == 3 else d) + floor
    err = np.abs(np.where(nan, 0.0, got - ref))
    bad = err > np.where(np.isnan(bound), 0.0, bound)
    assert not bad.any(), f"{what}: worst |delta| / bound = {np.nanmax(err / np.where(bound > 0, bound, np.nan)):.3g}"


def check_against_twin(lay, got, ref, error_mode, what=""):
    """The tolerances of the issue: reordering a sum of Bg products perturbs entry (i, j) by at most
    gamma_Bg sum w |x_i| |x_j| <= gamma_Bg sqrt(M_ii M_jj); gamma = 3.6e-12 at Bg = 32768, once for each side.
    That argument takes the summands x as given.  Where a group's mixture is a single filter (one-hot weights, Bg = 1)
    the summands of the spread are nothing but the rounding of mu [-] centre (1e-16), M itself is 1e-32 and no two
    libms agree on it: there, and only there (ess == 1), the spread is compared as the zero it is, to SPREAD_ZERO absolute -- the level the
    all-identical check uses -- which is twelve orders below the bound of any spread that is not zero."""
    M_cov = ref["mean_cov"]
    M_spr = ref["spread"] + (np.einsum("gi,gj->gij", ref["center"], ref["center"]) if error_mode else 0.0)
    assert_moment_close(got["mean_cov"], ref["mean_cov"], M_cov, what + " mean_cov")
    single = np.where(ref["ess"] == 1.0, SPREAD_ZERO, 0.0)[:, None, None]        # (one filter carries the whole group)
    assert_moment_close(got["spread"], ref["spread"], M_spr, what + " spread", floor=single)
    for name in ("spread", "mean_cov"):
        assert (got[name] == np.transpose(got[name], (0, 2, 1)))[~np.isnan(got[name])].all(), what + f" {name} not symmetric"
    if error_mode:
        assert_moment_close(got["center"], ref["center"], M_spr, what + " bias")
    else:
        nan = np.isnan(ref["center"]).any(axis=1)
        assert (np.isnan(got["center"]).all(axis=1) == nan).all(), what + " centre NaN pattern"
        for g in np.flatnonzero(~nan):
            d = np.abs(o.boxminus(lay, got["center"][g], ref["center"][g])).max()
            assert d <= 1e-9, f"{what} centre of group {g}: {d:.3g}"
    if "ess" in got:
        np.testing.assert_allclose(got["ess"], ref["ess"], rtol=1e-12, atol=0, equal_nan=True, err_msg=what + " ess")
