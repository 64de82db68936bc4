// Feature-track update through the GPU-backed header facade: a Msckf with k = 2 clones (N = 24) and 8 tracks of M = 3
// observation slots (m = 24 rows), landmarks 4 .. 7 units in front of the window seen from the state and both clones;
// track 5 has one observation only, track 6 has one observation moved by 25 sigma.  Two filters from the same state:
//   plain   updateTracks(tracks, sigma)
//   gated   updateTracks(tracks, sigma, chi2)
// Prints "name rows cols v0 v1 ..." lines (column-major) that tests/test_gpu_facade_tracks.py compares with the Python
// route on the same inputs.
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

static const int K = 2, N = 12 + 6 * K, NQ = 13 + 7 * K, J = 8, M = 3;

static void dump(const char *name, const slk::Matrix &m)
{
    std::printf("%s %d %d", name, m.rows(), m.cols());
    for (int i = 0; i < m.size(); ++i) std::printf(" %.17g", m.data()[i]);
    std::printf("\n");
}
static void dump_vec(const char *name, const std::vector<double> &v, int rows)
{
    std::printf("%s %d %d", name, rows, (int)v.size() / rows);
    for (std::size_t i = 0; i < v.size(); ++i) std::printf(" %.17g", v[i]);
    std::printf("\n");
}
static void dump_mean(const char *name, const WMultiState &s)
{
    std::vector<double> v(NQ);
    slk_store(s, v.data());
    dump_vec(name, v, NQ);
}

static int storage_offset(int pose) { return pose == 0 ? 0 : 13 + 7 * (pose - 1); }

// rotation matrix of a quaternion stored (x, y, z, w), row-major r[3][3]
static void rotation(const double *q, double r[3][3])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    r[0][0] = 1 - 2 * (y * y + z * z); r[0][1] = 2 * (x * y - z * w);     r[0][2] = 2 * (x * z + y * w);
    r[1][0] = 2 * (x * y + z * w);     r[1][1] = 1 - 2 * (x * x + z * z); r[1][2] = 2 * (y * z - x * w);
    r[2][0] = 2 * (x * z - y * w);     r[2][1] = 2 * (y * z + x * w);     r[2][2] = 1 - 2 * (x * x + y * y);
}

int main()
{
    // poses half a unit apart sideways, moderately rotated
    std::vector<double> m0(NQ, 0.0);
    for (int p = 0; p <= K; ++p) {
        const int sp = storage_offset(p);
        m0[sp] = 1.0 + 0.5 * p; m0[sp + 1] = -2.0 - 0.4 * p; m0[sp + 2] = 0.5 + 0.05 * p;
        const double x = 0.10 + 0.02 * p, y = -0.15 + 0.01 * p, z = 0.20 - 0.03 * p, w = std::sqrt(1 - x * x - y * y - z * z);
        m0[sp + 3] = x; m0[sp + 4] = y; m0[sp + 5] = z; m0[sp + 6] = w;
    }
    for (int i = 0; i < 6; ++i) m0[7 + i] = 0.1 * (i + 1);
    WMultiState x0;
    x0.sensorsk.resize(K);
    slk_load(x0, m0.data());
    slk::Matrix A(N, N), P(N, N);
    for (int j = 0; j < N; ++j) for (int i = 0; i < N; ++i) A(i, j) = 0.002 * std::sin(1.3 * i + 0.7 * j + 0.5);
    P = A * A.transpose();
    for (int i = 0; i < N; ++i) P(i, i) += 1e-4;
    const double sigma = 0.01;
    slk::FeatureTracks tracks(M);
    double r0[3][3];
    rotation(&m0[3], r0);
    for (int j = 0; j < J; ++j) {
        const double l[3] = {0.8 * std::sin(1.7 * j), 0.8 * std::cos(2.3 * j), 4.0 + 3.0 * std::fabs(std::sin(0.9 * j))};
        double lw[3];
        for (int i = 0; i < 3; ++i) lw[i] = m0[i] + r0[i][0] * l[0] + r0[i][1] * l[1] + r0[i][2] * l[2];
        tracks.add();
        for (int s = 0; s < M; ++s) {
            const int pose = (s + j) % (K + 1), sp = storage_offset(pose);
            if (j == 5 && s > 0) continue;                       // one observation: unused
            double r[3][3], d[3], c[3];
            rotation(&m0[sp + 3], r);
            for (int i = 0; i < 3; ++i) d[i] = lw[i] - m0[sp + i];
            for (int i = 0; i < 3; ++i) c[i] = r[0][i] * d[0] + r[1][i] * d[1] + r[2][i] * d[2];
            tracks.observe(j, s, pose, c[0] / c[2] + 0.005 * std::sin(3.1 * j + s), c[1] / c[2] + 0.005 * std::cos(1.9 * j + 2 * s));
        }
    }
    tracks.slots[3 * (6 * M + 1) + 2] += 25 * sigma;             // track 6, slot 1: v moved by 25 sigma
    std::vector<double> chi2(2 * M - 2);
    const double q95[4] = {0.0, 3.841, 5.991, 7.815};
    for (int i = 0; i < 2 * M - 2; ++i) chi2[i] = q95[i];
    dump_mean("mean0", x0);
    dump("P0", P);
    dump_vec("tracks", tracks.slots, 3);
    dump_vec("chi2", chi2, 1);

    MultiStateFilter plain(x0, P), gated(x0, P);
    const std::vector<int> fp = plain.updateTracks(tracks, sigma);
    const std::vector<double> pp = plain.trackPoints();
    const std::vector<int> fg = gated.updateTracks(tracks, sigma, chi2);
    dump_mean("plain_mean", plain.muState());
    dump("plain_P", plain.getPk());
    dump_vec("plain_feat", pp, 4);
    dump_mean("gated_mean", gated.muState());
    dump("gated_P", gated.getPk());
    dump_vec("gated_feat", gated.trackPoints(), 4);
    std::printf("plain_flags %d 1", J);
    for (int j = 0; j < J; ++j) std::printf(" %d", fp[j]);
    std::printf("\ngated_flags %d 1", J);
    for (int j = 0; j < J; ++j) std::printf(" %d", fg[j]);
    std::printf("\nstatus 2 1 %d %d\n", plain.status(), gated.status());
    return 0;
}
