// Usckf through the GPU-backed header facade with more than 32 measurement rows (the wide update): an SPD state of
// N = 36 + 30 = 66 (no featuresk_l), setMeasurement(STATEK) with 36 values -> nfk = 36, N = 72, a constant-velocity predict, then
// update(z, VoRelativeModel, R, mt) with 36 rows.  Prints "name rows cols v0 v1 ..." lines (column-major) that
// tests/test_gpu_usckf_wide.py repeats through the Python package and the oracle.
#include <cstdio>
#include <vector>

#include <localization/filters/Usckf.hpp>
#include <localization/filters/MtkWrap.hpp>
#include <localization/filters/State.hpp>

using namespace localization;

typedef MtkWrap<State> WSingleState;
typedef MtkMultiStateWrap<AugmentedState<-1> > WAugmentedState;
typedef Usckf<WAugmentedState, WSingleState> StateFilterDynamic;

static void dump(const char *name, const slk::Matrix &m)
{
    std::printf("%s %d %d", name, m.rows(), m.cols());
    for (int i = 0; i < m.size(); ++i) std::printf(" %.17g", m.data()[i]);
    std::printf("\n");
}
template <class S>
static void dump_mean(const char *name, const S &s, int nq)
{
    std::vector<double> v(nq);
    slk_store(s, v.data());
    std::printf("%s %d 1", name, nq);
    for (int i = 0; i < nq; ++i) std::printf(" %.17g", v[i]);
    std::printf("\n");
}

int main()
{
    const int nfk = 30, nfkl = 0, N = 36 + nfk + nfkl;
    WAugmentedState x0;
    State *st[3] = {&x0.statek, &x0.statek_l, &x0.statek_i};
    for (int b = 0; b < 3; ++b) {
        st[b]->pos << 0.5 + 0.1 * b, -0.3 + 0.05 * b, 1.0 - 0.2 * b;
        st[b]->velo << 0.3, -0.1 * b, 0.2;
        st[b]->angvelo << 0.01 * b, 0.02, -0.01;
    }
    x0.featuresk.resize(nfk); x0.featuresk_l.resize(nfkl);
    for (int i = 0; i < nfk; ++i) x0.featuresk[i] = 2.0 + 0.1 * i;
        slk::Matrix A(N, N), P(N, N);
    for (int j = 0; j < N; ++j) for (int i = 0; i < N; ++i) A(i, j) = 0.004 * (((i * 7 + j * 13) % 11) - 5.0) / 5.0;
    P = A * A.transpose();
    for (int i = 0; i < N; ++i) P(i, i) += 0.0025;
    StateFilterDynamic filter(x0, P);
    dump("wide_ctor_P", filter.PkAugmentedState());
    dump_mean("wide_ctor_mean", filter.muState(), N + 3);
    const int m = 36, N2 = 36 + m + nfkl;
    slk::Vector zk(m);
    for (int i = 0; i < m; ++i) zk[i] = 2.5 + 0.01 * i;
    slk::Matrix Rk = 0.008 * slk::Matrix::Identity(m, m);
    filter.setMeasurement(STATEK, zk, Rk);
    slk::Matrix Q = 0.001 * slk::Matrix::Identity(12, 12);
    slk::Vec3 velo(1.0, 0.2, -0.1), angular_velo(0.01, -0.02, 0.03);
    filter.predict(slk::ConstVelocityModel(velo, angular_velo, 0.01), Q);
    dump("wide_pred_P", filter.PkAugmentedState());
    dump_mean("wide_pred_mean", filter.muState(), N2 + 3);
    slk::Vector z(m);
    for (int i = 0; i < m; ++i) z[i] = 2.52 + 0.01 * i + 0.003 * (i % 5);
    slk::Matrix R = 0.01 * slk::Matrix::Identity(m, m);
    filter.update(z, slk::VoRelativeModel(), R, 0);
    dump("wide_z", z);
    dump("wide_upd_P", filter.PkAugmentedState());
    dump_mean("wide_upd_mean", filter.muState(), N2 + 3);
    std::printf("wide_status 1 1 %d\n", filter.status());
    return 0;
}
