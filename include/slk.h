/*
 * slk.h -- C ABI of the MI355X-native sigma-point Kalman hot path
 *          ("slk" = sigma-point localization kernels).
 *
 * Drop-in boundary for the predict()/update() path of
 *   localization::Msckf<_MultiState,_SingleState>      reference src/filters/Msckf.hpp
 *   localization::Usckf<_AugmentedState,_SingleState>  reference src/filters/Usckf.hpp
 * The reference is a header-only C++ template library with no FFI of its own; this is the
 * interface its filter classes bind to when they are backed by the GPU (the header facade
 * under include/localization/filters/ calls exactly these entry points; INTEGRATION.md shows
 * the binding).  One handle = a BATCH of B independent filters of identical layout on one
 * device; B = 1 reproduces the reference object.
 *
 * Conventions
 *   - fp64 everywhere (the reference scalar is double: src/filters/State.hpp:37-38).
 *   - matrices are column-major (Eigen default), one filter after the other:
 *       mean [B][Nq], P [B][N*N], Q [12*12], R [m*m].
 *   - quaternions are stored (x, y, z, w) like Eigen::Quaternion::coeffs().
 *   - State   storage (13): pos[3] quat[4] velo[3] angvelo[3], tangent DOF 12 (State.hpp:137-149)
 *     Sensor  storage  (7): pos[3] quat[4],                    tangent DOF  6 (State.hpp:242-252)
 *     Msckf mean  = State + k * Sensor            N = 12 + 6k      (State.hpp:336-376)
 *     Usckf mean  = statek, statek_l, statek_i, featuresk[nfk], featuresk_l[nfkl]
 *                                                 N = 36 + nfk + nfkl (State.hpp:529-593)
 *   - every pointer argument is host or device memory as said by the `where` argument of the
 *     call (SLK_HOST: the library stages it through its own device buffers; SLK_DEVICE: used
 *     in place, must be resident on the handle's device).
 *   - return value: 0 = ok, < 0 = API / runtime error (nothing was changed).  Numerical
 *     conditions are per-filter STATUS bits (slk_get_status); the reference has no error
 *     reporting at all (asserts / silently ignored LLT failure: Usckf.hpp:537-538, 620-624).
 *   - a handle is not thread-safe; distinct handles may be used concurrently.  All work of a
 *     handle is ordered on one HIP stream.
 */
#ifndef SLK_H
#define SLK_H

#ifdef __cplusplus
extern "C" {
#endif

#define SLK_ABI_VERSION 1

/* Msckf predict on the plain route (registered process model, no sigma-point emission): batches of at least this many
 * filters run two filters per wave, smaller ones one filter per wave.  The results are bit-identical either way.  The value
 * is the smallest batch from which the pair kernel measured ahead (profiles/ab_predict_pair.log): every batch that has a
 * pair -- its in-row broadcasts issue less than the one-wave kernel's wave-wide ones even for a lone wave. */
#ifndef SLK_PREDICT_PAIR_MIN_BATCH
#define SLK_PREDICT_PAIR_MIN_BATCH 2
#endif

typedef struct slk_filter slk_filter;

enum { SLK_MSCKF = 1, SLK_USCKF = 2 };
enum { SLK_HOST = 0, SLK_DEVICE = 1 };

/* error codes */
enum {
    SLK_OK = 0,
    SLK_E_INVALID = -1,      /* bad argument / size mismatch (reference: assert, Usckf.hpp:325-327) */
    SLK_E_NO_DEVICE = -2,    /* no usable HIP device: the product has NO CPU fallback */
    SLK_E_HIP = -3,          /* HIP runtime error, see slk_last_error() */
    SLK_E_UNSUPPORTED = -4,  /* shape outside what the kernels are built for */
    SLK_E_NOMEM = -5
};

/* per-filter status bits (OR-accumulated until slk_clear_status) */
enum {
    SLK_ST_LLT_FAIL = 1,            /* non-positive Cholesky pivot; that call left the filter unchanged */
    SLK_ST_MEAN_NOT_CONVERGED = 2,  /* manifold mean hit max_it = 10000 (Msckf.hpp:475,489-493) */
    SLK_ST_SINGULAR = 4,            /* innovation covariance not invertible */
    SLK_ST_ALL_REJECTED = 8,        /* every measurement block failed the gate: update skipped (Msckf.hpp:250) */
    SLK_ST_EKF_ROWS = 16,           /* EKF update: fewer rows than state dimensions survive the gate; the reference would
                                       read R.block(0,0,N,N) out of range (Msckf.hpp:806): update skipped */
    SLK_ST_BAD_INDEX = 32           /* a pose index among the parameters of a registered measurement model is outside
                                       0..k (Msckf) / 0..2 (Usckf) or not a number: update skipped (device-resident
                                       parameters; host-resident ones are rejected with SLK_E_INVALID before the launch) */
};

/* cloning modes of Usckf (Usckf.hpp:37-42) */
enum { SLK_STATEK = 1, SLK_STATEK_L = 2, SLK_STATEK_I = 3 };

/* Registered process models f: SingleState -> SingleState (Tier A, run on the GPU).
 * SLK_MODEL_EXTERNAL = opaque host functor (Tier B): the caller maps the sigma points itself. */
enum {
    SLK_MODEL_EXTERNAL = 0,
    SLK_PM_CONST_VELOCITY = 1,  /* test/UsckfUnitTest.cpp:34-49; u = velocity[3] angular_velocity[3] dt  (7) */
    SLK_PM_DELTA_POSE = 2,      /* test/MsckfUnitTest.cpp:33-47; u = dpos[3] dquat[4] velocity[3] angular_velocity[3] (13) */
    SLK_PM_DEAD_RECKON = 3      /* the step before predict fused in: DeadReckon::updatePose delta pose
                                   (src/core/DeadReckon.hpp:129-239, updateAttitude :246-286) feeding the delta-pose model;
                                   u = dt, current velocity[3] angular_velocity[3], previous velocity[3] angular_velocity[3] (13) */
};

/* Registered measurement models h: FullState -> R^m */
enum {
    SLK_MM_VO_RELATIVE = 1,     /* test/UsckfUnitTest.cpp:62-86 (Usckf only); no parameters, m = nfk */
    SLK_MM_FEATURE_PROJ = 2,    /* m/2 landmarks seen as normalised image points from a pose;
                                   params = (m/2) x { landmark xyz, pose index }; pose 0 = current
                                   state, c >= 1 = clone c-1 (Msckf) / 0,1,2 = statek,statek_l,statek_i (Usckf) */
    SLK_MM_POSE_POSITION = 3    /* z = position of pose params[0]; m = 3 */
};

typedef struct {
    int kind;            /* SLK_MSCKF / SLK_USCKF */
    int batch;           /* B >= 1 independent filters */
    int device;          /* HIP device ordinal */
    int n_clones;        /* Msckf: k sensor-pose clones (MultiState::sensorsk.size()) */
    int n_featuresk;     /* Usckf: |featuresk| */
    int n_featuresk_l;   /* Usckf: |featuresk_l| */
    void *stream;        /* hipStream_t to run on, or NULL for a library-owned stream */
} slk_config;

/* ---- lifetime: replaces the filter constructors (Msckf.hpp:80-85, Usckf.hpp:83-103) ---- */
int  slk_create(const slk_config *cfg, slk_filter **out);
void slk_destroy(slk_filter *f);
const char *slk_last_error(void);
int  slk_device_count(void);

int slk_batch(const slk_filter *f);
int slk_dof(const slk_filter *f);       /* N  = getDOF()            (State.hpp:373-376, 590-593) */
int slk_storage(const slk_filter *f);   /* Nq = stored mean length */

/* ---- state access: muState()/getPk()/setPk()/muSingleState() (Msckf.hpp:351-395,
 *      Usckf.hpp:435-526).  mean [B][Nq], P [B][N*N]; either may be NULL. ---- */
int slk_set_state(slk_filter *f, const double *mean, const double *P, int where);
int slk_get_state(slk_filter *f, double *mean, double *P, int where);
double *slk_mean_device_ptr(slk_filter *f);   /* resident buffers, for zero-copy callers */
double *slk_cov_device_ptr(slk_filter *f);    /* (the exact-shape Msckf update kernels store the lower triangle and the
                                                * diagonal tiles of P+ only -- nothing on the device reads more, Msckf.hpp:412, :447 --
                                                * and this call enqueues the mirror pass that completes the strict upper triangle:
                                                * call it again after further steps before reading the upper triangle through the
                                                * pointer; slk_get_state and every other entry point do the same by themselves) */

/* ---- predict(f, Q): Msckf.hpp:89-189, Usckf.hpp:107-244.
 *      u [B][u_stride] model inputs (u_stride 0 = one shared row);
 *      Q 12x12 (q_stride 0 = shared, else per-filter stride in doubles). ---- */
int slk_predict(slk_filter *f, int model, const double *u, int u_stride,
                const double *Q, int q_stride, int where);

/* ---- DeadReckon::updatePose (src/core/DeadReckon.hpp:129-239), delta-pose part, for the whole batch:
 *      u [B][u_stride] = dt v0[3] w0[3] v1[3] w1[3]  ->  delta [B][13] = dpos[3] dquat[4] velocity[3] angular_velocity[3],
 *      which is the `u` of slk_predict(SLK_PM_DELTA_POSE).  The covariance part of the reference
 *      (cov_position = C_vv dt^2, cov_orientation = C_ww dt^2, :167-176) is a scaling left to the caller. ---- */
int slk_dead_reckon(slk_filter *f, const double *u, int u_stride, double *delta, int where);

/* ---- TransformWithUncertainty::operator* (src/core/Transform.cpp:215-254; Jacobians of Pennec & Thirion :35-137) for the
 *      batch: out = t2 * t1 with transforms [B][7] = pos[3] quat[4: x,y,z,w] and covariances [B][36] = 6x6 column-major
 *      in the reference's [r t] order (rotation as a scaled axis first, translation second; Transform.hpp:57-61).
 *      cov2 / cov1 NULL = that side carries no uncertainty (hasUncertainty() false).  additive != 0 is the other branch
 *      of DeadReckon::updatePose's Affine3d overload (src/core/DeadReckon.hpp:306-330): pose = t2 * t1, covariance =
 *      cov2 + cov1 (t2 = prevPose, t1 = deltaPose there).  cov_out may be NULL.
 *      Eigen semantics mirrored (the reference pins no Eigen version and holds no fixture for Transform -- the behaviour
 *      below is pinned by this library's own tests, parity with the reference is UNPINNED): quaternion from the rotation
 *      matrix as Eigen::Quaterniond(linear()); q_to_r (Transform.cpp:44-48) as Eigen >= 3.3's AngleAxisd(q), i.e. angle =
 *      2 atan2(|vec|, |w|) with the axis flipped for w < 0 -- Eigen 3.0 - 3.2 take 2 acos(w) with the axis as it is, which
 *      gives the other representative of the rotation vector (2 pi apart) for a composite quaternion with w < 0. ---- */
int slk_transform_compose(slk_filter *f, const double *t2, const double *cov2, const double *t1, const double *cov1,
                          double *t_out, double *cov_out, int additive, int where);

/* ---- DeadReckon::updatePose, RigidBodyState overload (src/core/DeadReckon.hpp:129-239), whole: delta pose AND the
 *      covariance / posterior legs (:165-176, :200-229), for the batch.
 *      u [B][u_stride] as in slk_dead_reckon; velcov 6x6 column-major (linear 0-2, angular 3-5), c_stride 0 = shared;
 *      an entry that is NaN zeroes the delta covariances (:165-176).
 *      prev  [B][25] = pos[3] quat[4] cov_position[9] cov_orientation[9]            (3x3 column-major)
 *      post  [B][49] = the same 25 + velocity[3] cov_velocity[9] angular_velocity[3] cov_angular_velocity[9]; IN/OUT:
 *                      without use_tf the reference ACCUMULATES into it (position +=, covariances +=, :219-222)
 *      delta [B][31] = pose record (25) + velocity[3] angular_velocity[3]; may be NULL.  delta[0:7] + [25:31] is the `u` of
 *                      SLK_PM_DELTA_POSE.
 *      use_tf != 0: tfPostPose = tfPrevPose * tfDeltaPose through slk_transform_compose's arithmetic (:202-215). ---- */
int slk_dead_reckon_pose(slk_filter *f, const double *u, int u_stride, const double *velcov, int c_stride,
                         const double *prev, double *post, double *delta, int use_tf, int where);

/* ---- AdaptiveAttitudeCov (src/filters/MeasurementModels.hpp:136-286): a batch of B independent objects (history of
 *      m1 residual outer products, r1count, r2count each) resident on the device.  slk_adaptive_matrix is one call of
 *      ::matrix(xk, Pk, z, H, R) per object: xk [B][n], Pk [B][n*n], z [B][3], H [B][3*n] (3 x n column-major),
 *      R 3x3 (r_stride 0 = shared) -> Rout [B][9], which is the R (r_stride 9) of slk_update / slk_step. ---- */
typedef struct slk_adaptive slk_adaptive;
int  slk_adaptive_create(int batch, int device, unsigned m1, unsigned m2, double gamma, unsigned r2count, void *stream,
                         slk_adaptive **out);
void slk_adaptive_destroy(slk_adaptive *a);
int  slk_adaptive_matrix(slk_adaptive *a, int n, const double *xk, const double *Pk, const double *z, const double *H,
                         const double *R, int r_stride, double *Rout, int where);

/* ---- update(z, h, R[, mt]): UKF update, Msckf.hpp:196-277 (chi-square gate per 2-row block
 *      + applyDelta re-draw) and Usckf.hpp:246-308 (whole-vector gate, direct boxplus).
 *      params [B][p_stride] model parameters (0 = shared), z [B][m], R m x m (r_stride 0 = shared).
 *      gate: Msckf 0 = accept all blocks, 1 = accept_mahalanobis_distance (Msckf.hpp:199,844-905);
 *            Usckf 0 = accept_any (Usckf.hpp:249), d = chi-square dof of the whole-vector gate.
 *      Usckf limits: N = 36 + nfk + nfkl > 96 has no state-size limit except device memory: the predict runs on a
 *      global-workspace kernel (one wave per filter), and every update-side call (slk_update, slk_step,
 *      slk_update_from_sigma, slk_update_innovation, slk_update_sigma_points) on the wide update described below, with
 *      its reservation (m = 1 for slk_update_sigma_points).  N <= 96: for N > 48 the state and the update's
 *      measurement arrays share one workgroup's LDS; a call whose carve exceeds 160 KiB is refused with
 *      SLK_E_UNSUPPORTED before any launch, the filter untouched (slk_step too).  At m = nfk (SLK_MM_VO_RELATIVE) that
 *      refuses e.g. N = 96 with nfk = 12, N = 90 with nfk = 18 and N = 80 with nfk = 24; m = 3 / 4 (pose position, two
 *      features) runs at every N <= 96.
 *      Measurement rows: Msckf m <= 32 (a wider call returns SLK_E_INVALID).  Usckf has no row limit: a call with
 *      m > 32 (slk_update, slk_step, slk_update_from_sigma, slk_update_innovation) runs at every N on the wide update
 *      (csrc/slk_usckf_wide.hpp: one workgroup per filter, the m-sized products on fp64 matrix cores); in slk_step the
 *      predict takes its predict-only route first and the wide update is a launch of its own.  It reserves, per filter,
 *      N(N+1)/2 + m(m+1)/2 + m^2 + 2Nm + (2N+1)m + 17 * (max(N, m) rounded up to 16) + 3m + 4N doubles (rounded up to 8),
 *      kept by the handle between calls; a failed reservation returns before any launch. ---- */
int slk_update(slk_filter *f, int model, const double *params, int p_stride,
               const double *z, int m, const double *R, int r_stride, int gate, int where);

/* ---- update(z, h, R, mt) with an ARBITRARY significance test `mt` (Msckf.hpp:220-223, Usckf.hpp:262-302): the test is a
 *      host callable, so the update is split around it.
 *      slk_update_innovation: sigma points, Z = h(X), innovation and S = cov(Z) + R exactly as slk_update computes them,
 *        handed back as SI [B][m*m + m] = S (column-major), innovation; the filter is not modified.  `model` may be
 *        SLK_MODEL_EXTERNAL with Z [B][2N+1][m] = h(X) of slk_update_sigma_points (else Z = NULL).
 *      slk_update_selected (Msckf): the update with the surviving rows decided by the caller -- rowsel [B][m + 2] =
 *        { number of surviving rows, number of outlier blocks, surviving row indices in order } -- instead of the built-in
 *        chi-square loop; everything else as slk_update / slk_update_from_sigma.
 *      (Usckf has a whole-vector test: the caller evaluates mt on S, innovation and then calls slk_update with gate 0
 *      or not at all.) ---- */
int slk_update_innovation(slk_filter *f, int model, const double *params, int p_stride, const double *Z,
                          const double *z, int m, const double *R, int r_stride, double *SI, int where);
int slk_update_selected(slk_filter *f, int model, const double *params, int p_stride, const double *Z,
                        const double *z, int m, const double *R, int r_stride, const int *rowsel, int where);

/* ---- EKF update(z, h, H, R[, mt]): Msckf.hpp:284-349 (Msckf only).  The reference's functor h(mu_state, H) is
 *      evaluated by the caller at the current mean: zmean [B][m] = h(mu), H [B][m*N] = its Jacobian, m x N column-major
 *      per filter (Eigen default), m >= N rows (reduceDimension, :791-816, compresses to N).  R as in slk_update.
 *      gate: 0 = accept all 2-row blocks, 1 = accept_mahalanobis_distance (:285-289, :756-789 incl. its indexing of the
 *      unreduced information matrix and the shifted second erase).  Outliers: slk_get_outliers. ---- */
int slk_update_ekf(slk_filter *f, const double *z, const double *zmean, const double *H, int m,
                   const double *R, int r_stride, int gate, int where);

/* ---- EKF update from a REGISTERED measurement model (Tier A for the EKF update; the reference has no such call: its
 *      functor h(mu_state, H) is host code).  The library linearises the model at the resident mean on the device, so
 *      nothing of the state or of the Jacobian crosses to the host.  Msckf only, model = SLK_MM_FEATURE_PROJ only
 *      (SLK_MM_POSE_POSITION has m = 3 < N rows, SLK_MM_VO_RELATIVE is a Usckf model, SLK_MODEL_EXTERNAL is slk_update_ekf
 *      itself: all SLK_E_INVALID, the filter untouched); params, p_stride as in slk_update; the row rules of
 *      slk_update_ekf (N <= m <= 512, m even).
 *      For feature j with landmark Lw seen from pose c (position p, orientation q, tangent offset tp = 0 for the state,
 *      12 + 6 (c - 1) for clone c - 1), l = R(q)^T (Lw - p):
 *        zmean[2j .. 2j+1] = (l.x / l.z, l.y / l.z)
 *        H[2j .. 2j+1, tp .. tp+2] = -J R(q)^T,  H[2j .. 2j+1, tp+3 .. tp+5] = J [l]x,  every other entry an exact +0.0,
 *        J = [[1/l.z, 0, -l.x/l.z^2], [0, 1/l.z, -l.y/l.z^2]] -- the derivative under the filter's own boxplus
 *        (p + dp, q * exp(dtheta), State.hpp:186-200, :286-296).  Only the mean is read (a lower-only P needs no pass).
 *      Pose indices: host-resident parameters with an index outside 0 .. k (or NaN) are SLK_E_INVALID before any launch;
 *      device-resident ones give that filter SLK_ST_BAD_INDEX, its update is skipped (mean, P, outlier count untouched),
 *      the other filters are unaffected; slk_ekf_linearize fills the zmean / H of such a filter with NaN.
 *      slk_ekf_linearize: zmean [B][m] and H [B][m*N] (m x N column-major per filter, the layout slk_update_ekf takes)
 *        into caller memory; mean and P are not modified.
 *      slk_update_ekf_model: mean, P, status bits and outlier counts are bit-identical to slk_ekf_linearize(SLK_DEVICE)
 *        into caller buffers followed by slk_update_ekf(SLK_DEVICE) on them (two launches: the linearisation into a
 *        workspace of the handle, then slk_update_ekf's kernel of that shape, unchanged) -- except for a filter with a
 *        bad device-resident pose index: here it is skipped and stays untouched, whereas slk_update_ekf fed the NaN
 *        zmean / H of slk_ekf_linearize would run its update on them.
 *        gate (here, in slk_step_ekf and as slk_traj::gate in slk_step_n_ekf) is read as zero / non-zero: 0 = accept
 *        all 2-row blocks, anything else = accept_mahalanobis_distance as in slk_update_ekf (there is no caller-gated
 *        value 2 as in the UKF step).
 *      slk_step_ekf: slk_predict followed by slk_update_ekf_model, bit-identical; the state does not leave the device.
 *      slk_step_n_ekf: slk_step_n_slide (slide may be NULL) with slk_step_ekf as the step: everything slk_step_n and
 *        slk_step_n_slide promise -- every check and every reservation (this workspace and slk_update_ekf's included)
 *        before the first launch, one upload per input on the host route, no host synchronisation between steps, the
 *        records of a step taken after its slide -- with T x (slk_step_ekf, then slk_msckf_drop_clone + slk_msckf_clone_pose
 *        where slide[t] >= 0) as the bit-identical yardstick.  slk_traj is read as by slk_step_n.
 *      Workspace: B * (m * N + m) doubles for zmean and H plus one int per filter (the skip flags of bad pose indices),
 *      rounded up to 8 doubles, kept by the handle between calls like every other workspace, next to slk_update_ekf's
 *      own; a failed reservation returns before any launch. ---- */
int slk_ekf_linearize(slk_filter *f, int model, const double *params, int p_stride, int m,
                      double *zmean, double *H, int where);
int slk_update_ekf_model(slk_filter *f, int model, const double *params, int p_stride,
                         const double *z, int m, const double *R, int r_stride, int gate, int where);
int slk_step_ekf(slk_filter *f, int pmodel, const double *u, int u_stride, const double *Q, int q_stride,
                 int mmodel, const double *params, int p_stride, const double *z, int m,
                 const double *R, int r_stride, int gate, int where);

/* ---- Msckf feature-track update: landmarks of UNKNOWN position (the reference has no such call: its h(mu_state, H) is a
 *      host functor).  A track is one landmark seen from several poses of the window; it is triangulated from the
 *      resident poses and removed from the measurement by projecting onto the left null space of its own Jacobian, all on
 *      the device.  Msckf only.
 *      tracks [B][t_stride] (t_stride 0 = one set shared by every filter, otherwise >= 3 J M): J tracks of M observation
 *      slots { pose index c, u, v }; c as in SLK_MM_FEATURE_PROJ (0 = current state, c >= 1 = clone c - 1), c = -1 an
 *      empty slot; (u, v) the normalised image point.  sigma: the image-noise standard deviation, s_stride 0 = one
 *      shared value, 1 = [B].  2 <= M <= 32, J >= 1; m, the row count handed to the EKF update, obeys the rules of
 *      slk_update_ekf (N <= m <= 512, m even) and m >= J (2M - 3).
 *      Per track, at the resident mean:
 *        1. the slots with c >= 0, pose (p_i, q_i); fewer than two: UNUSED (flag 0); two slots naming one pose: FAILED
 *           (flag -1)
 *        2. d_i = R(q_i) (u_i, v_i, 1)^T normalised, A = sum (I - d_i d_i^T), b = sum (I - d_i d_i^T) p_i, X = A^-1 b by a
 *           3 x 3 Cholesky; a non-positive or NaN pivot: flag -1
 *        3. exactly five Gauss-Newton iterations X <- X - (sum F_i^T F_i)^-1 sum F_i^T e_i on e_i = pi(l_i) - (u_i, v_i),
 *           l_i = R(q_i)^T (X - p_i), F_i = J_i R(q_i)^T, J_i the projection Jacobian above; no early exit.  A
 *           non-positive or NaN pivot, a non-finite X, or a depth l_i.z <= 0 at the final X: flag -1
 *        4. at the final X: r_i = (u_i, v_i) - pi(l_i), H_x,i = the 2 x 6 block of SLK_MM_FEATURE_PROJ with Lw = X at the
 *           pose's tangent offset, H_f,i = F_i; empty slots are zero rows
 *        5. three Householder reflections on the 2M x 3 matrix H_f (Eigen's reflector convention, as slk_update_ekf's
 *           reduceDimension) applied to [H_x | r]; the first three rows are dropped, the other 2M - 3 divided by sigma:
 *           rows j (2M - 3) .. (j + 1)(2M - 3) - 1 of r and H, whitened (measurement noise I)
 *        6. chi2 != NULL: chi2 [2M - 2], resident as `where` says, indexed by dof = 2 n_obs - 3;
 *           gamma = r_j^T (H_j P H_j^T + I)^-1 r_j on the track's rows, P read from its lower triangle only; the track is
 *           kept iff gamma < chi2[dof], otherwise its flag is -2.  The library holds no table: the level is the caller's.
 *      Outputs: r [B][m], H [B][m*N] (m x N column-major, the layout slk_update_ekf takes); rows of a track whose flag is
 *      not 1, rows >= J (2M - 3) and every column outside a row's observed poses are exact +0.0.  feat [B][J][4] (may be
 *      NULL) = { X, flag }, flag 1 = used; X is +0.0 for flag 0 and NaN for flag -1.  Every entry of r, H and feat is
 *      written by the launch itself.  Mean, P, status and outlier counts are not modified; a lower-only P stays so.
 *      Pose indices outside -1 .. k (or NaN): host-resident tracks are SLK_E_INVALID before any launch; device-resident
 *      ones give that filter SLK_ST_BAD_INDEX, its r / H are filled with NaN (its feat with NaN points and flags 0) and in
 *      slk_update_tracks / slk_step_tracks it is skipped.  Every other bad argument (a Usckf handle, M, J, m, a stride, a
 *      NULL tracks / sigma / r / H, `where`, a host-resident sigma <= 0) is SLK_E_INVALID, nothing launched.
 *      slk_update_tracks: the linearisation into a workspace of the handle, then slk_update_ekf's kernel of that shape,
 *        unchanged, with z = r, zmean = 0, R = I_m shared and gate = 0: mean, P and status are bit-identical to
 *        slk_track_linearize(SLK_DEVICE) followed by slk_update_ekf(SLK_DEVICE) on those buffers -- except that a filter
 *        without a used track (or with a bad pose index) is skipped and stays bit for bit what it was, its outlier count
 *        included; every other filter's outlier count reads 0.  Rejected tracks are reported through feat.
 *      slk_step_tracks: slk_predict followed by slk_update_tracks, bit-identical.
 *      Workspace: B (m N + 2 m) + m^2 doubles plus one int per filter, next to slk_update_ekf's own, and B J 4 doubles
 *      for feat on the host route; all reserved before the first launch. ---- */
int slk_track_linearize(slk_filter *f, const double *tracks, int t_stride, int J, int M,
                        const double *sigma, int s_stride, const double *chi2, int m,
                        double *r, double *H, double *feat, int where);
int slk_update_tracks(slk_filter *f, const double *tracks, int t_stride, int J, int M,
                      const double *sigma, int s_stride, const double *chi2, int m, double *feat, int where);
int slk_step_tracks(slk_filter *f, int pmodel, const double *u, int u_stride, const double *Q, int q_stride,
                    const double *tracks, int t_stride, int J, int M, const double *sigma, int s_stride,
                    const double *chi2, int m, double *feat, int where);

/* ---- fused predict + update, one kernel launch, state stays on chip between the two
 *      (the benchmark's "filter step") ---- */
int slk_step(slk_filter *f, int pmodel, const double *u, int u_stride, const double *Q, int q_stride,
             int mmodel, const double *params, int p_stride, const double *z, int m,
             const double *R, int r_stride, int gate, int where);

/* ---- multi-step trajectories: T fused steps in one call (the reference has no such call: its callers loop over
 *      predict / update).  After the call the mean, P (as slk_get_state reads it), the status bits and the outlier
 *      counts are bit-identical to T successive slk_step calls with the same inputs; a filter whose factorisation fails
 *      at step t is left unchanged by that step and gets its status bit, the next steps go on.
 *      Per-step inputs: step t reads X + t * X_tstride for X = u, Q, params, z, R (and truth); each block has exactly the
 *      layout of the matching slk_step argument with the same *_stride meaning.  A *_tstride counts doubles; 0 = every
 *      step uses the same block; a nonzero one shorter than one step's block is SLK_E_INVALID.
 *      Optional records (NULL = not recorded), all [T][B]-major:
 *        mean_hist     [T][B][Nq]  the mean after step t (what slk_get_state returns after the (t + 1)-th single step)
 *        outliers_hist [T][B]      what slk_get_outliers returns after step t
 *        nees_hist     [T][B]      slk_nees(truth_t, nees_t0, nees_n) after step t; truth_t = truth + t * truth_tstride,
 *                                  [B][Nq] (needs truth; the range rules of slk_nees)
 *      Every check runs before any launch (slk_step's checks for every step, T >= 1, where SLK_HOST or SLK_DEVICE, nees_hist needs truth; Msckf
 *      m > 32 and SLK_MODEL_EXTERNAL are refused as in slk_step), and every staging / workspace reservation is made
 *      before the first launch: a failed check or reservation leaves the filter untouched.
 *      SLK_HOST: one upload of each input for all T steps, one synchronised download of the records at the end.
 *      SLK_DEVICE: nothing is copied; asynchronous on the handle's stream.  No host synchronisation between steps.
 *      Each step enqueues slk_step's own launches on the inputs of that step, then that step's records: device-to-device
 *      copies of the mean / outlier counts, and the NEES from a one-wave register factorisation for ranges of n <= 30
 *      (equal to slk_nees to 1e-10 relative, NaN exactly where slk_nees gives NaN) or from slk_nees's own kernel for
 *      wider ranges (bit-identical; its workspace reserved once).
 *      Memory: the host route stages all T steps of every input and of the records in device buffers of the handle,
 *      which keeps them (like every staging buffer) until slk_destroy -- e.g. the mean records alone are T * B * Nq
 *      doubles (450 MB at T = 200, B = 4096, N = 60).  The device route allocates nothing per step. ---- */
typedef struct slk_traj {
    int T;                                                            /* number of steps, >= 1 */
    int pmodel; const double *u; int u_stride; long long u_tstride;   /* step t reads u + t * u_tstride */
    const double *Q; int q_stride; long long q_tstride;
    int mmodel; const double *params; int p_stride; long long p_tstride;
    const double *z; int m; long long z_tstride;                      /* per step [B][m], as slk_step */
    const double *R; int r_stride; long long r_tstride;
    int gate;
    /* optional per-step records (NULL = not recorded) */
    double   *mean_hist;      /* [T][B][Nq]: the mean after step t */
    unsigned *outliers_hist;  /* [T][B]: what slk_get_outliers returns after step t */
    const double *truth; long long truth_tstride; int nees_t0, nees_n;  /* truth of step t: truth + t * truth_tstride, [B][Nq] */
    double   *nees_hist;      /* [T][B]: slk_nees(truth_t, nees_t0, nees_n) after step t (needs truth) */
} slk_traj;
int slk_step_n(slk_filter *f, const slk_traj *t, int where);
/* ---- sliding-window trajectories: slk_step_n with a window slide after chosen steps (the reference has no such call:
 *      its callers push / pop muState().sensorsk and setPk between updates).  slide [T] is a HOST array in both routes
 *      (`where` refers to the trajectory's data as in slk_step_n): slide[t] = -1 leaves the window as it is after step
 *      t, slide[t] = d in 0 .. k - 1 runs slk_msckf_slide(f, d) after step t.  slide == NULL is exactly slk_step_n.
 *      The mean, P (as slk_get_state reads it), the status bits, the outlier counts and every record are bit-identical
 *      to a loop of T x (slk_step, then slk_msckf_drop_clone(d_t) + slk_msckf_clone_pose when d_t >= 0); the records
 *      of step t are taken AFTER its slide.  Every schedule entry is checked with slk_step_n's checks, and the second
 *      state buffer pair is reserved, before the first launch: an entry outside -1 .. k - 1, or a schedule on a Usckf
 *      handle, is SLK_E_INVALID and leaves the filter untouched.  The schedule is a separate argument: slk_traj and
 *      its size are those of slk_step_n. ---- */
int slk_step_n_slide(slk_filter *f, const slk_traj *t, const int *slide, int where);
/* slk_step_n_slide with slk_step_ekf as the step (see slk_update_ekf_model above; slide may be NULL) */
int slk_step_n_ekf(slk_filter *f, const slk_traj *t, const int *slide, int where);
/* ---- per-step consistency records of a trajectory (see slk_nis / slk_get_sigma below).  slk_traj and the three entry
 *      points above stay as they are; the records are a separate argument, like the slide schedule.
 *      d == NULL, or every member NULL, is exactly slk_step_n_slide (ekf == 0) / slk_step_n_ekf (ekf != 0).  With
 *      records, the mean, P, the status bits, the outlier counts and every slk_traj record are bit-identical to the same
 *      call without d: each step's own launches are unchanged, the records are extra launches beside them.
 *        nis_hist    [T][B]     slk_nis of step t's update on the PREDICTED state of step t (before any gate)
 *        logdet_hist [T][B]     its log det S (may be recorded without nis_hist)
 *        sigma_hist  [T][B][N]  slk_get_sigma(0, N) after step t (after its slide, like mean_hist)
 *      The fused step kernels never expose their predicted state, so the NIS record comes from a shadow of the step's
 *      first half: the state is copied device-to-device into a scratch pair of the handle (B (N^2 + Nq) doubles; a
 *      lower-only P is completed in the copy, the filter's own stays lower-only), slk_predict's launch, the emit-4
 *      launch and the statistics kernel of slk_nis run on the copy, then the step runs as always.  The shadow predict is
 *      slk_predict's launch, so nis_hist[t] is bit for bit what slk_predict + slk_nis give on the state before step t (as
 *      slk_get_state reads it); it agrees with the fused step's internal S to rounding only.  The filter's status
 *      bits are not touched by the shadow; a filter whose shadow fails (P not positive definite) records NaN.
 *      Cost: one more predict and one more sigma-point / h(X) / moments pass per step plus the copy of the state: 2.5 x
 *      an unrecorded step at N = 60, m = 8, B = 4096; sigma_hist alone is one small launch.
 *      Everything on the handle's stream, no host synchronisation between steps, every reservation before the first
 *      launch; SLK_HOST: the records come down once at the end.
 *      SLK_E_INVALID, the filter untouched: ekf != 0 with nis_hist or logdet_hist (the EKF kernels form H P H^T + R
 *      internally); everything slk_step_n_slide / slk_step_n_ekf refuse. ---- */
typedef struct slk_traj_diag {
    double *nis_hist;      /* [T][B]    slk_nis of step t's update, taken on the PREDICTED state of step t */
    double *logdet_hist;   /* [T][B]    its log det S (needs nothing else; may be set without nis_hist) */
    double *sigma_hist;    /* [T][B][N] slk_get_sigma(0, N) after step t (after its slide, like mean_hist) */
} slk_traj_diag;           /* every member NULL = not recorded */
int slk_step_n_diag(slk_filter *f, const slk_traj *t, const int *slide, int ekf, const slk_traj_diag *d, int where);

/* ---- Tier B (opaque host functors, the reference's boost::bind form:
 *      UsckfUnitTest.cpp:246,284; MsckfUnitTest.cpp:200-205).  The library draws the sigma
 *      points (generateSigmaPoints, Msckf.hpp:400-468 / Usckf.hpp:532-598), the caller applies
 *      f / h, the library finishes the step with the same kernels as Tier A. ---- */
int slk_predict_sigma_points(slk_filter *f, double *X /* [B][25][13] */, int where);
int slk_predict_from_sigma(slk_filter *f, const double *Y /* [B][25][13] = f(X) */,
                           const double *Q, int q_stride, int where);
int slk_update_sigma_points(slk_filter *f, double *X /* [B][2N+1][Nq] */, int where);
int slk_update_from_sigma(slk_filter *f, const double *Z /* [B][2N+1][m] = h(X) */,
                          const double *z, int m, const double *R, int r_stride, int gate, int where);

/* ---- Usckf bookkeeping: cloning() Usckf.hpp:391-433, setMeasurement() Usckf.hpp:322-389
 *      (changes N; z [B][n], R n x n shared) ---- */
int slk_usckf_cloning(slk_filter *f, int mode);
int slk_usckf_set_measurement(slk_filter *f, int mode, const double *z, int n, const double *R, int where);
/* Msckf sliding window: caller-side push/pop on muState().sensorsk + setPk (Msckf.hpp:381-395) */
int slk_msckf_resize(slk_filter *f, int n_clones);
/* ... and the same on the device, so that a trajectory never round-trips through the host (the reference has no
 *     such call: its callers push/pop muState().sensorsk and setPk, Msckf.hpp:381-395, State.hpp:342, :373-396):
 *     clone_pose appends a SensorState equal to the current pose (pos, orient) whose covariance rows / columns copy
 *     the pose's (J P J^T, J = [I; E_pose]); drop_clone removes clone `index` (0 = oldest) with its 6 rows / columns. */
int slk_msckf_clone_pose(slk_filter *f);
int slk_msckf_drop_clone(slk_filter *f, int index);
/* One slide of the window, k unchanged: drop clone `index` (0 = oldest), then clone the current pose as the newest --
 *     bit for bit what slk_msckf_drop_clone(f, index) followed by slk_msckf_clone_pose(f) give, in one launch and with no
 *     pass that completes P first.  A covariance whose strict upper triangle is stale (after the exact-shape steps) is
 *     read and written as its lower triangle (N (N + 1) / 2 doubles each way per filter) and stays lower-only, to be
 *     completed on demand like after those steps; a complete one is gathered whole.  The mean and P move to the
 *     handle's second buffer pair (slk_mean_device_ptr / slk_cov_device_ptr change, as after clone / drop).
 *     SLK_E_INVALID, the filter untouched: a Usckf handle, k = 0, or an index outside 0 .. k - 1. */
int slk_msckf_slide(slk_filter *f, int index);

/* ---- checkSigmaPoints(): Msckf.hpp:819-839 (Usckf.hpp:769-789 is the same self test).  Re-draws the sigma points of
 *      (mu_state, Pk), takes their manifold mean and covariance on the device and reports per filter
 *      max_cov_err [B] = max |covSigmaPoints - Pk| (the reference asserts <= 1e-6) and mean_err [B] = |mu_state [-] muX|
 *      (the reference asserts mu_state == muX, i.e. isZero(1e-12) of the difference, MtkWrap.hpp:108-112).
 *      The filter is not modified.  Msckf only (the Usckf facade runs the same test on the sigma points of
 *      slk_update_sigma_points). ---- */
int slk_check_sigma_points(slk_filter *f, double *max_cov_err, double *mean_err, int where);

/* ---- Monte-Carlo consistency tools on the resident (mu, P) of every filter (the reference has no such call).
 *      Both are read-only (mean, P, status bits and outlier counts stay as they were), read the LOWER triangle of P only
 *      (a covariance whose strict upper triangle is stale after the exact-shape Msckf steps gives the same answer), run
 *      at every N of both kinds, and enqueue one launch on the handle's stream (host outputs are synchronised).  A
 *      (sub-)block that is not positive definite (a non-positive or NaN Cholesky pivot) gives that filter NaN outputs;
 *      the others are unaffected, the call still returns SLK_OK and sets no status bit.
 *      Both reserve, per filter, (n+1)(n+2)/2 + 33 * (n + 1 rounded up to 16) doubles (rounded up to 8; n = N for
 *      slk_sample_states), kept by the handle between calls; a failed reservation returns before any launch.
 *
 *      slk_nees: normalised estimation error squared on the tangent indices [t0, t0 + n):
 *        e = (truth [-] mu) restricted to the range (truth [B][Nq] in the storage layout; [-] is exactly the filter's
 *        own boxminus, log(mu^-1 q) for every SO(3) block, w < 0 included; a range may start or end inside an SO(3)
 *        block: its components come from that block's full 3-vector),
 *        nees [B] = e^T P_ss^-1 e with P_ss the principal n x n block of P on the range,
 *        err [B][n] = e when not NULL.
 *        SLK_E_INVALID for t0 < 0, n < 1, t0 + n > N or a NULL truth / nees.
 *      slk_sample_states: out [B][S][Nq] = mu_b [+] (L_b noise[b][s]) for noise [B][S][N] supplied by the caller (the
 *        library has no RNG: e.g. standard normal draws made on the device), L_b the lower Cholesky factor of P_b -- the
 *        factor the sigma points are drawn from.  A non-positive-definite P_b fills all S rows of that filter with NaN.
 *        SLK_E_INVALID for S < 1 or a NULL noise / out. ---- */
int slk_nees(slk_filter *f, const double *truth /*[B][Nq]*/, int t0, int n, double *nees /*[B]*/,
             double *err /*[B][n] or NULL*/, int where);
int slk_sample_states(slk_filter *f, const double *noise /*[B][S][N]*/, int S, double *out /*[B][S][Nq]*/, int where);
/* ---- the two consistency statistics that need no ground truth (the reference has no such call).  Both are read-only
 *      like slk_nees: mean, P, status bits and outlier counts stay as they were.
 *
 *      slk_nis: normalised innovation squared of the update slk_update would make with these arguments.  Arguments up
 *        to r_stride exactly as slk_update_innovation (the same checks and refusals: Z only with SLK_MODEL_EXTERNAL,
 *        Msckf m <= 32, Usckf any m), both kinds, every N.
 *        nis [B] = nu^T S^-1 nu, logdet [B] = log det S (NULL = not wanted), with S and nu bit for bit what
 *        slk_update_innovation emits (all m rows, before any gate).  The Gaussian log-likelihood of the measurement is
 *        -0.5 (nis + logdet + m log(2 pi)).
 *        Two launches on the handle's stream: the emit-4 launch of slk_update_innovation into a workspace of the handle
 *        (B (m^2 + m) doubles, reserved before any launch and kept between calls), then innovation_stats_kernel, which
 *        factors S with nu as a bordering row: one wave per filter in registers for m <= 30, four waves on slk_nees's
 *        workspace above (its size at n = m).  Like slk_update_innovation it completes a lower-only P first.
 *        A non-positive or NaN Cholesky pivot of S gives that filter NaN in both outputs; so does an emission that is
 *        skipped (P not positive definite, a bad pose index in device-resident parameters) -- and, unlike
 *        slk_update_innovation, no status bit is set either way.  The call returns SLK_OK, other filters are unaffected.
 *        SLK_E_INVALID for a NULL nis and for everything slk_update_innovation refuses.
 *      slk_get_sigma: sigma [B][n], sigma[b][i] = sqrt(P_b(t0 + i, t0 + i)) on the tangent indices [t0, t0 + n) (the
 *        range rules and errors of slk_nees).  One launch that reads the diagonal only: a lower-only P is not completed
 *        first and stays lower-only.  A negative or NaN diagonal entry gives NaN for that entry.  `where` other than
 *        SLK_HOST / SLK_DEVICE is SLK_E_INVALID. ---- */
int slk_nis(slk_filter *f, int model, const double *params, int p_stride, const double *Z, const double *z, int m,
            const double *R, int r_stride, double *nis /*[B]*/, double *logdet /*[B] or NULL*/, int where);
int slk_get_sigma(slk_filter *f, int t0, int n, double *sigma /*[B][n]*/, int where);

/* ---- across the filters of the batch (the reference has no such call): with slk_nis the loop weight -> estimate ->
 *      resample of a filter bank or a particle cloud stays on the device.
 *
 *      slk_ensemble_moments: the moments of the batch, or of `groups` = G groups of it; group g is the filters
 *        [g B / G, (g + 1) B / G).  weights [B] (NULL = uniform), normalised per group: w~_b = w_b / sum_group w;
 *        ess [G] = (sum w)^2 / sum w^2.  The range [t0, t0 + n) follows the rules of slk_nees (it may cut an SO(3) block).
 *        Error mode (truth [B][Nq] given): e_b = (truth_b [-] mu_b) on the range, exactly as slk_nees takes it;
 *          center [G][n] = ebar = sum w~_b e_b (the bias), spread = sum w~_b (e_b - ebar)(e_b - ebar)^T.
 *        Mixture mode (truth NULL): center [G][Nq] = the weighted manifold mean of the group's means over the WHOLE state,
 *          in the storage layout, by the pinned iteration: ref = the mean of the group's first filter; one pass is
 *          dbar = sum w~_b (mu_b [-] ref) over all N indices, then ref <- ref [+] dbar; it stops after the pass in which
 *          |dbar|_2 <= 1e-12, or after 100 passes.  spread = sum w~_b d_b d_b^T, d_b = (mu_b [-] center) on the range.
 *        Both modes: mean_cov = sum w~_b P_b[range, range].  The moment-matched covariance of the mixture is
 *          spread + mean_cov (the caller adds them); in error mode spread ~ mean_cov is the Monte-Carlo consistency
 *          check.  Population sums: Bessel's factor is the caller's.  spread and mean_cov are [G][n * n], full n x n
 *          column-major, both triangles written from one value (exactly symmetric).
 *        center, spread, mean_cov and ess may each be NULL (not wanted); all four NULL is SLK_E_INVALID.
 *        A group with a negative, NaN or infinite weight, or whose weights do not sum to something > 0 (and finite), gets
 *        NaN in all of its outputs; the other groups are unaffected, the call returns SLK_OK and sets no status bit.
 *        Read-only like slk_nees: mean, P, status bits and outlier counts stay bit for bit what they were.  P is read from
 *        its LOWER triangle only and never factored: a lower-only covariance is not completed and stays lower-only, and P
 *        need not be positive definite.  Both kinds, every N.  Device work is enqueued on the handle's stream (up to
 *        seven launches, no host synchronisation between them); host outputs are synchronised.
 *        Deterministic: every sum over filters runs in a fixed order (per-chunk partials in the workspace, added in
 *        index order; no atomics), and the chunking depends on (B, G, N, n) only, so two calls on the same state give
 *        bit-identical outputs.
 *        Workspace (doubles, rounded up to 8, reserved before any launch and kept by the handle; a failed reservation
 *        returns with nothing launched), with Bg = B / G, E = n (n + 1) / 2, c = Nq in mixture mode and n in error mode:
 *          2 B + G + G c + B n + [Cc > 1] G Cc E + [Cs > 1] G Cs E,
 *          Cs = ceil(Bg / 256) chunks of the spread, Cc = ceil(Bg / F) chunks of the mean covariance with
 *          F = ceil(Bg / min(ceil(Bg / 8), max(1, ceil(2048 / (G ceil(E / 256))))));
 *        a host call adds G n^2 for each of spread and mean_cov that is wanted.
 *        SLK_E_INVALID, nothing launched: groups < 1, B % groups != 0, the range errors of slk_nees, all outputs NULL,
 *        `where` other than SLK_HOST / SLK_DEVICE.  SLK_E_UNSUPPORTED: more than 65535 chunks in a group (16 M filters).
 *
 *      slk_gather_states: filter b becomes a copy of the old filter src[b] -- mean, P, status bits and outlier count --
 *        bit for bit what slk_get_state, a host index and slk_set_state give (plus the same index on status and
 *        outliers): resampling, hypothesis pruning, scenario fan-out.  Drawing the indices from the weights stays with
 *        the caller (the library holds no RNG).  One launch into the handle's second buffers, reserved before it
 *        (slk_mean_device_ptr / slk_cov_device_ptr change, as after slk_msckf_slide).  A lower-only covariance is copied
 *        as its lower triangle (N (N + 1) / 2 doubles each way per filter) and stays lower-only; a complete one is
 *        copied whole.  Both kinds, every N.
 *        An index outside 0 .. B - 1: host-resident src gives SLK_E_INVALID before any launch, the handle untouched;
 *        device-resident src makes that filter keep its own state and sets its SLK_ST_BAD_INDEX, the others unaffected.
 *        SLK_E_INVALID also for a NULL src and for `where` other than SLK_HOST / SLK_DEVICE. ---- */
int slk_ensemble_moments(slk_filter *f, int groups, const double *weights /*[B] or NULL*/,
                         const double *truth /*[B][Nq] or NULL*/, int t0, int n,
                         double *center, double *spread /*[G][n*n]*/, double *mean_cov /*[G][n*n]*/,
                         double *ess /*[G] or NULL*/, int where);
int slk_gather_states(slk_filter *f, const int *src /*[B]*/, int where);

/* ---- arithmetic of the covariance rebuild (Msckf.hpp:665 -> :574-589): SLK_PREC_F64 (default, the
 *      parity path), SLK_PREC_F32 (fp32 MFMA) or SLK_PREC_BF16 (bf16 operands, fp32 accumulation).
 *      The reduced modes exist for the tolerance sweep of BASELINE.json config 5; the reference is
 *      double throughout (State.hpp:37-38). ---- */
enum { SLK_PREC_F64 = 0, SLK_PREC_F32 = 1, SLK_PREC_BF16 = 2 };
int slk_set_rebuild_precision(slk_filter *f, int mode);

/* ---- results of the last update / accumulated status ---- */
int slk_get_outliers(slk_filter *f, unsigned *outliers /* [B], return value of Msckf::update :276 */, int where);
int slk_get_status(slk_filter *f, int *status /* [B] */, int where);
int slk_clear_status(slk_filter *f);
int slk_sync(slk_filter *f);

/* ---- measurement aids (HIP events on the handle's stream) ---- */
int slk_timer_start(slk_filter *f);
int slk_timer_stop(slk_filter *f, float *milliseconds);

/* self test of the fp64 MFMA fragment layout used by the covariance rebuild: multiplies an
 * asymmetric 16x16 pair on the device and checks it on the host.  0 = layout as documented. */
int slk_selftest_mfma(int device);

/* self test of the two-filters-per-wave predict kernel on an odd batch of SLK_PREDICT_PAIR_MIN_BATCH | 1 filters (N = 12),
 * on arrays of its own with guard words behind mean, P and status: 0 = every word the one-wave kernel's and the guards
 * intact; else bit 0 = the kernels differ, bit 1 = a guard word was written, bit 2 = the case itself is off. */
int slk_selftest_predict_pair(int device);

#ifdef __cplusplus
}
#endif
#endif /* SLK_H */
