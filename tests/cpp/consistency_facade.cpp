// NEES and Gaussian state draws through the GPU-backed header facade: a Msckf with k = 3 clones (N = 30) and a Usckf with
// nfk = 3, nfkl = 2 (N = 41), each with a deterministic SPD covariance, a truth state and a noise matrix; then the Msckf window
// grows by one clone through muState() + setPk right before a draw, and the size checks of both facades.  Prints
// "name rows cols v0 v1 ..." lines (column-major) that tests/test_gpu_consistency.py repeats through the Python package.
#include <cmath>
#include <cstdio>
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
static slk::Matrix noise(int N, int S)
{
    slk::Matrix n(N, S);
    for (int s = 0; s < S; ++s) for (int i = 0; i < N; ++i) n(i, s) = std::sin(0.37 * i + 1.91 * s + 0.2);
    return n;
}

int main()
{
    {   // Msckf, k = 3
        const int k = 3, N = 12 + 6 * k, Nq = 13 + 7 * k;
        std::vector<int> qo(1, 3);
        for (int c = 0; c < k; ++c) qo.push_back(13 + 7 * c + 3);
        const std::vector<double> m0 = storage(Nq, qo, 0.0), t0 = storage(Nq, qo, 1.0);
        WMultiState x0, truth;
        x0.sensorsk.resize(k); truth.sensorsk.resize(k);
        slk_load(x0, m0.data()); slk_load(truth, t0.data());
        const slk::Matrix P = spd(N, 0.5);
        MultiStateFilter filter(x0, P);
        dump_raw("msckf_mean", m0, Nq);
        dump_raw("msckf_truth", t0, Nq);
        dump("msckf_P", P);
        slk::Vector err;
        std::printf("msckf_nees_full 1 1 %.17g\n", filter.nees(truth));
        std::printf("msckf_nees_att 1 1 %.17g\n", filter.nees(truth, 3, 3, &err));
        dump("msckf_err_att", err);
        std::printf("msckf_nees_clone 1 1 %.17g\n", filter.nees(truth, N - 6, 6));
        const slk::Matrix nz = noise(N, 3);
        dump("msckf_noise", nz);
        const std::vector<WMultiState> xs = filter.sampleStates(nz);
        std::vector<double> out((std::size_t)xs.size() * Nq);
        for (std::size_t s = 0; s < xs.size(); ++s) slk_store(xs[s], &out[s * Nq]);
        dump_raw("msckf_samples", out, Nq);
        // the window grows through muState() + setPk (the reference's flow): the edit reaches the device with the draw
        WMultiState &ms = filter.muState();
        ms.sensorsk.push_back(ms.sensorsk[0]);
        const int N2 = N + 6, Nq2 = Nq + 7;
        const slk::Matrix P2 = spd(N2, 2.5);
        filter.setPk(P2);
        const slk::Matrix nz2 = noise(N2, 4);
        const std::vector<WMultiState> xs2 = filter.sampleStates(nz2);
        std::vector<double> m2(Nq2), out2((std::size_t)xs2.size() * Nq2);
        slk_store(filter.muState(), m2.data());
        for (std::size_t s = 0; s < xs2.size(); ++s) slk_store(xs2[s], &out2[s * Nq2]);
        dump_raw("grown_mean", m2, Nq2);
        dump("grown_P", P2);
        dump("grown_noise", nz2);
        dump_raw("grown_samples", out2, Nq2);
        int thrown = 0;
        try { filter.sampleStates(noise(N, 2)); } catch (const std::invalid_argument &) { thrown |= 1; }
        try { filter.nees(truth); } catch (const std::invalid_argument &) { thrown |= 2; }     // k clones, the filter has k + 1
        std::printf("msckf_size_checks 1 1 %d\n", thrown);
    }
    {   // Usckf, nfk = 3, nfkl = 2
        const int nfk = 3, nfkl = 2, N = 36 + nfk + nfkl, Nq = 39 + nfk + nfkl;
        const std::vector<int> qo = {3, 16, 29};
        const std::vector<double> m0 = storage(Nq, qo, 0.0), t0 = storage(Nq, qo, 1.0);
        WAugmentedState x0, truth;
        x0.featuresk.resize(nfk); x0.featuresk_l.resize(nfkl);
        truth.featuresk.resize(nfk); truth.featuresk_l.resize(nfkl);
        slk_load(x0, m0.data(), nfk, nfkl); slk_load(truth, t0.data(), nfk, nfkl);
        const slk::Matrix P = spd(N, 1.5);
        StateFilterDynamic filter(x0, P);
        dump_raw("usckf_mean", m0, Nq);
        dump_raw("usckf_truth", t0, Nq);
        dump("usckf_P", P);
        std::printf("usckf_nees_full 1 1 %.17g\n", filter.nees(truth));
        std::printf("usckf_nees_pose 1 1 %.17g\n", filter.nees(truth, 0, 6));
        const slk::Matrix nz = noise(N, 2);
        dump("usckf_noise", nz);
        const std::vector<WAugmentedState> xs = filter.sampleStates(nz);
        std::vector<double> out((std::size_t)xs.size() * Nq);
        for (std::size_t s = 0; s < xs.size(); ++s) slk_store(xs[s], &out[s * Nq]);
        dump_raw("usckf_samples", out, Nq);
        WAugmentedState other = truth;
        other.featuresk.resize(nfk + 1);
        int thrown = 0;
        try { filter.sampleStates(noise(N + 1, 2)); } catch (const std::invalid_argument &) { thrown |= 1; }
        try { filter.nees(other); } catch (const std::invalid_argument &) { thrown |= 2; }
        std::printf("usckf_size_checks 1 1 %d\n", thrown);
    }
    return 0;
}
