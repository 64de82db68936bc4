// Innovation consistency through the GPU-backed header facade: nis(z, h, R) of a Msckf with k = 3 clones (N = 30) for the
// registered feature-projection model (m = 4), the registered position fix (m = 3) and a host functor (the position of
// clone 1 plus the current position, m = 6), and of a Usckf with nfk = 3, nfkl = 2 (N = 41) for the registered
// relative-transform model (m = 3) and a host functor (m = 2); the filters are read back afterwards (nis is read-only).
// Prints "name rows cols v0 v1 ..." lines (column-major) that tests/test_gpu_nis.py repeats through the Python package
// and numpy.
#include <cmath>
#include <cstdio>
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
static void dump_pair(const char *name, double nis, double logdet)
{
    std::printf("%s 2 1 %.17g %.17g\n", name, nis, logdet);
}

static std::vector<double> storage(int nq, const std::vector<int> &qoff, double phase)
{
    std::vector<double> m(nq);
    for (int i = 0; i < nq; ++i) m[i] = 0.3 * std::sin(0.7 * i + phase) + 0.1 * i;
    for (std::size_t b = 0; b < qoff.size(); ++b) {
        double *q = &m[qoff[b]];
        const double x = 0.1 * std::sin(b + phase), y = 0.08 * std::cos(2.0 * b + phase), z = 0.05 * std::sin(3.0 * b + 1.0);
        q[0] = x; q[1] = y; q[2] = z; q[3] = std::sqrt(1.0 - x * x - y * y - z * z);
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

struct ClonePlusPosition            // z = (position of clone 1, current position)
{
    slk::Vector operator()(const WMultiState &x) const
    {
        slk::Vector z(6);
        for (int i = 0; i < 3; ++i) { z[i] = x.sensorsk[1].pos[i]; z[3 + i] = x.statek.pos[i]; }
        return z;
    }
};
struct TwoFeatures                  // z = (featuresk[0], featuresk_l[1])
{
    slk::Vector operator()(const WAugmentedState &x) const
    {
        slk::Vector z(2);
        z[0] = x.featuresk[0]; z[1] = x.featuresk_l[1];
        return z;
    }
};

int main()
{
    {   // Msckf, k = 3
        const int k = 3, N = 12 + 6 * k, Nq = 13 + 7 * k;
        std::vector<int> qo(1, 3);
        for (int c = 0; c < k; ++c) qo.push_back(13 + 7 * c + 3);
        std::vector<double> m0 = storage(Nq, qo, 0.0);
        m0[2] = 0.4;                                              // (the landmarks below stay well in front of every pose)
        for (int c = 0; c < k; ++c) m0[13 + 7 * c + 2] = 0.2 + 0.1 * c;
        WMultiState x0;
        x0.sensorsk.resize(k);
        slk_load(x0, m0.data());
        const slk::Matrix P = spd(N, 0.5);
        MultiStateFilter filter(x0, P);
        dump_raw("msckf_mean", m0, Nq);
        dump("msckf_P", P);
        slk::FeatureProjectionModel h;
        slk::Vector z(4);
        for (int j = 0; j < 2; ++j) {
            h.add(0.5 * (j - 0.5) + 1.0, 0.3 * (0.5 - j) + 1.0, 6.0 + j, j + 1);
            z[2 * j] = 0.05 * (j + 1.0);
            z[2 * j + 1] = -0.03 * (j + 1.0);
        }
        dump_raw("msckf_feat", h.params, 4);
        dump("msckf_feat_z", z);
        const slk::Matrix R4 = 0.01 * slk::Matrix::Identity(4, 4);
        double ld = 0;
        const double n1 = filter.nis(z, h, R4, &ld);
        dump_pair("msckf_feat_nis", n1, ld);
        std::printf("msckf_feat_nis_only 1 1 %.17g\n", filter.nis(z, h, R4));
        slk::Vector zp(3);
        for (int i = 0; i < 3; ++i) zp[i] = m0[13 + 7 + i] + 0.02 * (i + 1);          // pose index 2 = clone 1
        const slk::Matrix R3 = 0.02 * slk::Matrix::Identity(3, 3);
        dump("msckf_pose_z", zp);
        const double n2 = filter.nis(zp, slk::PosePositionModel(2), R3, &ld);
        dump_pair("msckf_pose_nis", n2, ld);
        slk::Vector zf(6);
        for (int i = 0; i < 3; ++i) { zf[i] = m0[13 + 7 + i] - 0.01 * (i + 1); zf[3 + i] = m0[i] + 0.015; }
        const slk::Matrix R6 = 0.015 * slk::Matrix::Identity(6, 6);
        dump("msckf_functor_z", zf);
        const double n3 = filter.nis(zf, ClonePlusPosition(), R6, &ld);
        dump_pair("msckf_functor_nis", n3, ld);
        std::vector<double> m1(Nq);
        slk_store(filter.muState(), m1.data());
        dump_raw("msckf_mean_after", m1, Nq);
        dump("msckf_P_after", filter.getPk());
        std::printf("msckf_status 1 1 %d\n", filter.status());
    }
    {   // Usckf, nfk = 3, nfkl = 2
        const int nfk = 3, nfkl = 2, N = 36 + nfk + nfkl, Nq = 39 + nfk + nfkl;
        const std::vector<int> qo = {3, 16, 29};
        const std::vector<double> m0 = storage(Nq, qo, 0.0);
        WAugmentedState x0;
        x0.featuresk.resize(nfk); x0.featuresk_l.resize(nfkl);
        slk_load(x0, m0.data(), nfk, nfkl);
        const slk::Matrix P = spd(N, 1.5);
        StateFilterDynamic filter(x0, P);
        dump_raw("usckf_mean", m0, Nq);
        dump("usckf_P", P);
        slk::Vector z(3);
        for (int i = 0; i < 3; ++i) z[i] = 0.1 * (i + 1);
        dump("usckf_vo_z", z);
        const slk::Matrix R3 = 0.01 * slk::Matrix::Identity(3, 3);
        double ld = 0;
        const double n1 = filter.nis(z, slk::VoRelativeModel(), R3, &ld);
        dump_pair("usckf_vo_nis", n1, ld);
        slk::Vector zf(2);
        zf[0] = m0[39] + 0.03; zf[1] = m0[39 + nfk + 1] - 0.02;
        dump("usckf_functor_z", zf);
        const slk::Matrix R2 = 0.02 * slk::Matrix::Identity(2, 2);
        const double n2 = filter.nis(zf, TwoFeatures(), R2, &ld);
        dump_pair("usckf_functor_nis", n2, ld);
        dump("usckf_P_after", filter.PkAugmentedState());
        std::printf("usckf_status 1 1 %d\n", filter.status());
    }
    return 0;
}
