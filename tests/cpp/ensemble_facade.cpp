// slk_ensemble_moments / slk_gather_states through the raw forwarding forms of the GPU-backed header facade: a Msckf with
// k = 3 clones (N = 30) and a Usckf with nfk = 3, nfkl = 2 (N = 41), each one filter with a deterministic SPD covariance
// and a truth state.  For one filter the moments are known in closed form (the centre is the mean or the error, the
// spread zero, mean_cov the covariance block); tests/test_gpu_ensemble_facade.py checks the printed
// "name rows cols v0 v1 ..." lines (column-major) against the Python package and the numpy twin.
#include <cmath>
#include <cstdio>
#include <string>
#include <stdexcept>
#include <vector>

#include <localization/filters/Msckf.hpp>
#include <localization/filters/Usckf.hpp>
#include <localization/filters/MtkWrap.hpp>
#include <localization/filters/State.hpp>

using namespace localization;

typedef MtkWrap<State> WSingleState;
typedef MtkDynamicWrap<MultiState<State, SensorState> > WMultiState;
typedef Msckf<WMultiState, WSingleState> MultiStateFilter;
typedef MtkMultiStateWrap<AugmentedState<-1> > WAugmentedState;
typedef Usckf<WAugmentedState, WSingleState> StateFilterDynamic;

static void dump(const char *name, const slk::Matrix &m)
{
    std::printf("%s %d %d", name, m.rows(), m.cols());
    for (int i = 0; i < m.size(); ++i) std::printf(" %.17g", m.data()[i]);
    std::printf("\n");
}
static void dump_raw(const char *name, const std::vector<double> &v, int rows)
{
    std::printf("%s %d %d", name, rows, (int)v.size() / rows);
    for (double x : v) std::printf(" %.17g", x);
    std::printf("\n");
}

// storage vector with n_so3 unit quaternions at the given offsets, everything else a deterministic pattern
static std::vector<double> storage(int nq, const std::vector<int> &qoff, double phase)
{
    std::vector<double> m(nq);
    for (int i = 0; i < nq; ++i) m[i] = 0.3 * std::sin(0.7 * i + phase) + 0.1 * i;
    for (std::size_t b = 0; b < qoff.size(); ++b) {
        double *q = &m[qoff[b]];
        const double x = 0.1 * std::sin(b + phase), y = 0.08 * std::cos(2.0 * b + phase), z = 0.05 * std::sin(3.0 * b + 1.0);
        const double w = std::sqrt(1.0 - x * x - y * y - z * z);
        q[0] = x; q[1] = y; q[2] = z; q[3] = (b == 1 && phase > 0.5) ? -w : w;   // one truth quaternion with w < 0
    }
    return m;
}
static slk::Matrix spd(int N, double seed)
{
    slk::Matrix A(N, N), P(N, N);
    for (int j = 0; j < N; ++j) for (int i = 0; i < N; ++i) A(i, j) = 0.01 * std::sin(1.3 * i + 0.7 * j + seed);
    P = A * A.transpose();
    for (int i = 0; i < N; ++i) P(i, i) += 0.004 + 0.0001 * i;
    return P;
}

static const slk::Matrix &cov_of(MultiStateFilter &f) { return f.getPk(); }
static const slk::Matrix &cov_of(StateFilterDynamic &f) { return f.PkAugmentedState(); }

template <class Filter>
static void moments_and_gather(const char *tag, Filter &filter, const std::vector<double> &truth, int N, int Nq)
{
    char name[64];
    const int t0 = 4, n = 5;                                                     // cuts two SO(3) blocks
    std::vector<double> bias(n), spread(n * n), cov(n * n), ess(1);
    filter.ensembleMoments(1, 0, truth.data(), t0, n, bias.data(), spread.data(), cov.data(), ess.data());
    std::snprintf(name, sizeof name, "%s_bias", tag);     dump_raw(name, bias, n);
    std::snprintf(name, sizeof name, "%s_espread", tag);  dump_raw(name, spread, n);
    std::snprintf(name, sizeof name, "%s_ecov", tag);     dump_raw(name, cov, n);
    std::snprintf(name, sizeof name, "%s_ess", tag);      dump_raw(name, ess, 1);
    const double w[1] = {2.5};
    std::vector<double> centre(Nq), mspread((std::size_t)N * N), mcov((std::size_t)N * N);
    filter.ensembleMoments(1, w, 0, 0, N, centre.data(), mspread.data(), mcov.data());
    std::snprintf(name, sizeof name, "%s_centre", tag);   dump_raw(name, centre, Nq);
    std::snprintf(name, sizeof name, "%s_mspread", tag);  dump_raw(name, mspread, N);
    std::snprintf(name, sizeof name, "%s_mcov", tag);     dump_raw(name, mcov, N);
    const int self[1] = {0}, outside[1] = {1};
    filter.gatherStates(self);
    dump(std::string(tag).append("_P_after").c_str(), cov_of(filter));
    int thrown = 0;
    try { filter.gatherStates(outside); } catch (const std::runtime_error &) { thrown |= 1; }
    try { filter.ensembleMoments(2, 0, 0, 0, N, centre.data(), 0, 0); } catch (const std::runtime_error &) { thrown |= 2; }
    try { filter.ensembleMoments(1, 0, 0, 0, N, 0, 0, 0); } catch (const std::runtime_error &) { thrown |= 4; }
    std::snprintf(name, sizeof name, "%s_refusals", tag);
    std::printf("%s 1 1 %d\n", name, thrown);
}

int main()
{
    {   // Msckf, k = 3
        const int k = 3, N = 12 + 6 * k, Nq = 13 + 7 * k;
        std::vector<int> qo(1, 3);
        for (int c = 0; c < k; ++c) qo.push_back(13 + 7 * c + 3);
        const std::vector<double> m0 = storage(Nq, qo, 0.0), t0 = storage(Nq, qo, 1.0);
        WMultiState x0;
        x0.sensorsk.resize(k);
        slk_load(x0, m0.data());
        const slk::Matrix P = spd(N, 0.5);
        MultiStateFilter filter(x0, P);
        dump_raw("msckf_mean", m0, Nq);
        dump_raw("msckf_truth", t0, Nq);
        dump("msckf_P", P);
        moments_and_gather("msckf", filter, t0, N, Nq);
    }
    {   // Usckf, nfk = 3, nfkl = 2
        const int nfk = 3, nfkl = 2, N = 36 + nfk + nfkl, Nq = 39 + nfk + nfkl;
        const std::vector<int> qo = {3, 16, 29};
        const std::vector<double> m0 = storage(Nq, qo, 0.0), t0 = storage(Nq, qo, 1.0);
        WAugmentedState x0;
        x0.featuresk.resize(nfk); x0.featuresk_l.resize(nfkl);
        slk_load(x0, m0.data(), nfk, nfkl);
        const slk::Matrix P = spd(N, 1.5);
        StateFilterDynamic filter(x0, P);
        dump_raw("usckf_mean", m0, Nq);
        dump_raw("usckf_truth", t0, Nq);
        dump("usckf_P", P);
        moments_and_gather("usckf", filter, t0, N, Nq);
    }
    return 0;
}
