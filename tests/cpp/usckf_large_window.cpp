// Usckf through the GPU-backed header facade at a state above 96 dimensions (the global-workspace path): an SPD state of
// N = 36 + 12 + 42 = 90, setMeasurement(STATEK_L) with 72 values -> N = 120, predict and update with opaque functors (the
// reference's boost::bind form).  Prints "name rows cols v0 v1 ..." lines (column-major) that
// tests/test_gpu_usckf_large.py repeats through the Python package.
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

// process model functor: constant-velocity drift of the position (the Python test applies the same map)
struct DriftModel
{
    double dt;
    WSingleState operator()(const WSingleState &x) const
    {
        WSingleState y = x;
        for (int c = 0; c < 3; ++c) y.pos[c] = x.pos[c] + dt * x.velo[c];
        return y;
    }
};
// measurement functor: the position of statek and the first feature of featuresk_l
struct PositionModel
{
    slk::Vector operator()(const WAugmentedState &x) const
    {
        slk::Vector z(4);
        for (int c = 0; c < 3; ++c) z[c] = x.statek.pos[c];
        z[3] = x.featuresk_l[0];
        return z;
    }
};

int main()
{
    const int nfk = 12, nfkl = 42, N = 36 + nfk + nfkl;
    WAugmentedState x0;
    State *st[3] = {&x0.statek, &x0.statek_l, &x0.statek_i};
    for (int b = 0; b < 3; ++b) {
        st[b]->pos << 0.5 + 0.1 * b, -0.3 + 0.05 * b, 1.0 - 0.2 * b;
        st[b]->velo << 0.3, -0.1 * b, 0.2;
        st[b]->angvelo << 0.01 * b, 0.02, -0.01;
    }
    x0.featuresk.resize(nfk); x0.featuresk_l.resize(nfkl);
    for (int i = 0; i < nfk; ++i) x0.featuresk[i] = 2.0 + 0.1 * i;
    for (int i = 0; i < nfkl; ++i) x0.featuresk_l[i] = 1.0 + 0.05 * i;
    slk::Matrix A(N, N), P(N, N);
    for (int j = 0; j < N; ++j) for (int i = 0; i < N; ++i) A(i, j) = 0.004 * (((i * 7 + j * 13) % 11) - 5.0) / 5.0;
    P = A * A.transpose();
    for (int i = 0; i < N; ++i) P(i, i) += 0.0025;
    StateFilterDynamic filter(x0, P);
    dump("large_ctor_P", filter.PkAugmentedState());
    dump_mean("large_ctor_mean", filter.muState(), N + 3);
    slk::Vector zl(72);
    for (int i = 0; i < 72; ++i) zl[i] = 1.5 + 0.01 * i;
    slk::Matrix Rl = 0.008 * slk::Matrix::Identity(72, 72);
    filter.setMeasurement(STATEK_L, zl, Rl);
    const int N2 = 36 + nfk + 72;
    slk::Matrix Q = 0.001 * slk::Matrix::Identity(12, 12);
    DriftModel f; f.dt = 0.01;
    filter.predict(f, Q);
    dump("large_pred_P", filter.PkAugmentedState());
    dump_mean("large_pred_mean", filter.muState(), N2 + 3);
    slk::Vector z(4);
    z[0] = 0.55; z[1] = -0.28; z[2] = 1.02; z[3] = 1.48;
    slk::Matrix R = 0.01 * slk::Matrix::Identity(4, 4);
    filter.update(z, PositionModel(), R);
    dump("large_upd_P", filter.PkAugmentedState());
    dump_mean("large_upd_mean", filter.muState(), N2 + 3);
    std::printf("large_status 1 1 %d\n", filter.status());
    return 0;
}
