// EKF update from a registered model through the GPU-backed header facade, next to the functor form with a
// hand-written Jacobian: a Msckf with k = 2 clones (N = 24) and 14 features (m = 28) seen from the state and both
// clones, one outlier block.  Three filters from the same state:
//   functor   update(z, h, H, R)      h(mu_state, H) evaluated on the host (the reference's form)
//   model     update(z, model, H, R)  slk::FeatureProjectionModel, linearised on the device (slk_update_ekf_model)
//   custom    update(z, model, H, R, mt) with a caller's chi-square test: slk_ekf_linearize + the caller-gated code
// Prints "name rows cols v0 v1 ..." lines (column-major) that tests/test_gpu_facade_ekf_model.py compares.
#include <cmath>
#include <cstdio>
#include <vector>

#include <localization/filters/Msckf.hpp>
#include <localization/filters/MtkWrap.hpp>
#include <localization/filters/State.hpp>

using namespace localization;

typedef MtkWrap<State> WSingleState;
typedef MtkDynamicWrap<MultiState<State, SensorState> > WMultiState;
typedef Msckf<WMultiState, WSingleState> MultiStateFilter;

static const int K = 2, N = 12 + 6 * K, NQ = 13 + 7 * K, NF = 14, M = 2 * NF;

static void dump(const char *name, const slk::Matrix &m)
{
    std::printf("%s %d %d", name, m.rows(), m.cols());
    for (int i = 0; i < m.size(); ++i) std::printf(" %.17g", m.data()[i]);
    std::printf("\n");
}
static void dump_mean(const char *name, const WMultiState &s)
{
    std::vector<double> v(NQ);
    slk_store(s, v.data());
    std::printf("%s %d 1", name, NQ);
    for (int i = 0; i < NQ; ++i) std::printf(" %.17g", v[i]);
    std::printf("\n");
}

static int storage_offset(int pose) { return pose == 0 ? 0 : 13 + 7 * (pose - 1); }
static int tangent_offset(int pose) { return pose == 0 ? 0 : 12 + 6 * (pose - 1); }

// rotation matrix of a quaternion stored (x, y, z, w), row-major r[3][3]
static void rotation(const double *q, double r[3][3])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    r[0][0] = 1 - 2 * (y * y + z * z); r[0][1] = 2 * (x * y - z * w);     r[0][2] = 2 * (x * z + y * w);
    r[1][0] = 2 * (x * y + z * w);     r[1][1] = 1 - 2 * (x * x + z * z); r[1][2] = 2 * (y * z - x * w);
    r[2][0] = 2 * (x * z - y * w);     r[2][1] = 2 * (y * z + x * w);     r[2][2] = 1 - 2 * (x * x + y * y);
}

// the reference's h(mu_state, H) for stacked feature projections, written by hand: l = R^T (Lw - p),
// z = (l.x, l.y) / l.z, dz/dp = -J R^T, dz/dtheta = J [l]x under p + dp, q * exp(dtheta)
struct FeatureFunctor
{
    const std::vector<double> &params;
    slk::Vector operator()(const WMultiState &mu, slk::Matrix &H) const
    {
        std::vector<double> x(NQ);
        slk_store(mu, x.data());
        slk::Vector zm(M);
        for (int i = 0; i < M; ++i) for (int j = 0; j < N; ++j) H(i, j) = 0.0;
        for (int f = 0; f < NF; ++f) {
            const double *lw = &params[4 * f];
            const int pose = (int)lw[3], sp = storage_offset(pose), tp = tangent_offset(pose);
            double r[3][3], d[3], l[3];
            rotation(&x[sp + 3], r);
            for (int i = 0; i < 3; ++i) d[i] = lw[i] - x[sp + i];
            for (int i = 0; i < 3; ++i) l[i] = r[0][i] * d[0] + r[1][i] * d[1] + r[2][i] * d[2];
            zm[2 * f] = l[0] / l[2];
            zm[2 * f + 1] = l[1] / l[2];
            const double J[2][3] = {{1 / l[2], 0, -l[0] / (l[2] * l[2])}, {0, 1 / l[2], -l[1] / (l[2] * l[2])}};
            const double lx[3][3] = {{0, -l[2], l[1]}, {l[2], 0, -l[0]}, {-l[1], l[0], 0}};
            for (int row = 0; row < 2; ++row)
                for (int c = 0; c < 3; ++c) {
                    double hp = 0, hq = 0;
                    for (int i = 0; i < 3; ++i) { hp -= J[row][i] * r[c][i]; hq += J[row][i] * lx[i][c]; }   // (R^T)(i, c) = r[c][i]
                    H(2 * f + row, tp + c) = hp;
                    H(2 * f + row, tp + 3 + c) = hq;
                }
        }
        return zm;
    }
};

struct ChiSquare2 { bool operator()(const double &d2, int) const { return d2 < 5.99; } };   // a caller's own test object

int main()
{
    // state: poses near (1, -2, 0.5), moderately rotated; clones a little off the current pose
    std::vector<double> m0(NQ, 0.0);
    for (int p = 0; p <= K; ++p) {
        const int sp = storage_offset(p);
        m0[sp] = 1.0 + 0.05 * p; m0[sp + 1] = -2.0 - 0.04 * p; m0[sp + 2] = 0.5 + 0.03 * p;
        const double x = 0.10 + 0.02 * p, y = -0.15 + 0.01 * p, z = 0.20 - 0.03 * p, w = std::sqrt(1 - x * x - y * y - z * z);
        m0[sp + 3] = x; m0[sp + 4] = y; m0[sp + 5] = z; m0[sp + 6] = w;
    }
    for (int i = 0; i < 6; ++i) m0[7 + i] = 0.1 * (i + 1);
    WMultiState x0;
    x0.sensorsk.resize(K);
    slk_load(x0, m0.data());
    slk::Matrix A(N, N), P(N, N);
    for (int j = 0; j < N; ++j) for (int i = 0; i < N; ++i) A(i, j) = 0.02 * std::sin(1.3 * i + 0.7 * j + 0.5);
    P = A * A.transpose();
    for (int i = 0; i < N; ++i) P(i, i) += 0.01;
    // landmarks 4 .. 7 in front of the pose that sees them, measurements = projections + a small offset, one outlier
    slk::FeatureProjectionModel model;
    slk::Vector z(M);
    for (int f = 0; f < NF; ++f) {
        const int pose = f % (K + 1), sp = storage_offset(pose);
        double r[3][3];
        rotation(&m0[sp + 3], r);
        const double l[3] = {0.8 * std::sin(1.7 * f), 0.8 * std::cos(2.3 * f), 4.0 + 3.0 * std::fabs(std::sin(0.9 * f))};
        double lw[3];
        for (int i = 0; i < 3; ++i) lw[i] = m0[sp + i] + r[i][0] * l[0] + r[i][1] * l[1] + r[i][2] * l[2];
        model.add(lw[0], lw[1], lw[2], pose);
        z[2 * f] = l[0] / l[2] + 0.03 * std::sin(3.1 * f);
        z[2 * f + 1] = l[1] / l[2] + 0.03 * std::cos(1.9 * f);
    }
    z[10] += 25.0;
    slk::Matrix R = 0.01 * slk::Matrix::Identity(M, M);
    dump_mean("mean0", x0);
    dump("P0", P);

    MultiStateFilter functor(x0, P), registered(x0, P), custom(x0, P);
    slk::Matrix Hf(M, N), Hm(M, N), Hc(M, N);
    for (int i = 0; i < M; ++i) for (int j = 0; j < N; ++j) Hm(i, j) = -7.0;        // the device form leaves H alone
    FeatureFunctor hf = {model.params};
    const unsigned of = functor.update(z, hf, Hf, R);
    const unsigned om = registered.update(z, model, Hm, R);
    const unsigned oc = custom.update(z, model, Hc, R, ChiSquare2());
    dump_mean("functor_mean", functor.muState());
    dump("functor_P", functor.getPk());
    dump("functor_H", Hf);
    dump_mean("model_mean", registered.muState());
    dump("model_P", registered.getPk());
    dump("model_H", Hm);
    dump_mean("custom_mean", custom.muState());
    dump("custom_P", custom.getPk());
    dump("custom_H", Hc);
    std::printf("outliers 3 1 %u %u %u\n", of, om, oc);
    std::printf("status 3 1 %d %d %d\n", functor.status(), registered.status(), custom.status());
    return 0;
}
