"""Host-side mirror of the reference filter interface on top of the C ABI (include/slk.h).

Class and method names follow the reference (src/filters/Msckf.hpp, Usckf.hpp): predict,
update, muState, muSingleState, getPk/setPk, PkAugmentedState, cloning, setMeasurement --
batched: every array carries a leading batch dimension B (B = 1 is the reference object).
Matrices are exchanged as numpy [B, rows, cols]; the column-major C-ABI layout is handled
here.  Python is plumbing only: every numerical operation runs in libslk_hip.so on the GPU
and there is NO CPU fallback -- loading or creating fails loudly without a HIP device.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libslk_hip.so")

MSCKF, USCKF = 1, 2
HOST, DEVICE = 0, 1
STATEK, STATEK_L, STATEK_I = 1, 2, 3
MODEL_EXTERNAL, PM_CONST_VELOCITY, PM_DELTA_POSE, PM_DEAD_RECKON = 0, 1, 2, 3
MM_VO_RELATIVE, MM_FEATURE_PROJ, MM_POSE_POSITION = 1, 2, 3
ST_LLT_FAIL, ST_MEAN_NOT_CONVERGED, ST_SINGULAR, ST_ALL_REJECTED, ST_EKF_ROWS, ST_BAD_INDEX = 1, 2, 4, 8, 16, 32
E_INVALID, E_NO_DEVICE, E_HIP, E_UNSUPPORTED, E_NOMEM = -1, -2, -3, -4, -5
PREDICT_PAIR_MIN_BATCH = 2      # SLK_PREDICT_PAIR_MIN_BATCH of include/slk.h: Msckf predict runs two filters per wave from here on

# every symbol include/slk.h declares (checked by the CPU test-suite against the built library)
EXPORTS = [
    "slk_create", "slk_destroy", "slk_last_error", "slk_device_count", "slk_batch", "slk_dof", "slk_storage",
    "slk_set_state", "slk_get_state", "slk_mean_device_ptr", "slk_cov_device_ptr", "slk_predict", "slk_update",
    "slk_step", "slk_predict_sigma_points", "slk_predict_from_sigma", "slk_update_sigma_points",
    "slk_update_from_sigma", "slk_usckf_cloning", "slk_usckf_set_measurement", "slk_msckf_resize",
    "slk_get_outliers", "slk_get_status", "slk_clear_status", "slk_sync", "slk_timer_start", "slk_timer_stop",
    "slk_selftest_mfma", "slk_selftest_predict_pair", "slk_set_rebuild_precision", "slk_dead_reckon", "slk_msckf_clone_pose", "slk_msckf_drop_clone", "slk_update_ekf",
    "slk_check_sigma_points", "slk_update_innovation", "slk_update_selected", "slk_transform_compose",
    "slk_dead_reckon_pose", "slk_adaptive_create", "slk_adaptive_destroy", "slk_adaptive_matrix", "slk_nees",
    "slk_sample_states", "slk_step_n", "slk_step_n_slide", "slk_msckf_slide",
    "slk_ekf_linearize", "slk_update_ekf_model", "slk_step_ekf", "slk_step_n_ekf",
    "slk_nis", "slk_get_sigma", "slk_step_n_diag",
    "slk_ensemble_moments", "slk_gather_states",
    "slk_track_linearize", "slk_update_tracks", "slk_step_tracks",
]


class SlkError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("kind", C.c_int), ("batch", C.c_int), ("device", C.c_int), ("n_clones", C.c_int),
                ("n_featuresk", C.c_int), ("n_featuresk_l", C.c_int), ("stream", C.c_void_p)]


class Traj(C.Structure):
    """struct slk_traj of include/slk.h"""
    _fields_ = [("T", C.c_int),
                ("pmodel", C.c_int), ("u", C.c_void_p), ("u_stride", C.c_int), ("u_tstride", C.c_longlong),
                ("Q", C.c_void_p), ("q_stride", C.c_int), ("q_tstride", C.c_longlong),
                ("mmodel", C.c_int), ("params", C.c_void_p), ("p_stride", C.c_int), ("p_tstride", C.c_longlong),
                ("z", C.c_void_p), ("m", C.c_int), ("z_tstride", C.c_longlong),
                ("R", C.c_void_p), ("r_stride", C.c_int), ("r_tstride", C.c_longlong),
                ("gate", C.c_int),
                ("mean_hist", C.c_void_p), ("outliers_hist", C.c_void_p),
                ("truth", C.c_void_p), ("truth_tstride", C.c_longlong), ("nees_t0", C.c_int), ("nees_n", C.c_int),
                ("nees_hist", C.c_void_p)]


class TrajDiag(C.Structure):
    """struct slk_traj_diag of include/slk.h"""
    _fields_ = [("nis_hist", C.c_void_p), ("logdet_hist", C.c_void_p), ("sigma_hist", C.c_void_p)]


_lib = None


def load_library(path=None):
    """dlopen libslk_hip.so and declare the prototypes.  Raises if the library is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("SLK_HIP_LIB") or LIB_PATH      # SLK_HIP_LIB: A/B runs of experimental builds (tools/ab.sh)
    if not os.path.exists(p):
        raise SlkError(f"{p} not built: run `python slam-localization_amd/build.py` (needs hipcc)")
    lib = C.CDLL(p)
    vp, ip = C.c_void_p, C.c_int
    lib.slk_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.slk_destroy.argtypes = [vp]
    lib.slk_destroy.restype = None
    lib.slk_last_error.restype = C.c_char_p
    for n in ("slk_batch", "slk_dof", "slk_storage", "slk_clear_status", "slk_sync", "slk_timer_start"):
        getattr(lib, n).argtypes = [vp]
    lib.slk_set_state.argtypes = [vp, vp, vp, ip]
    lib.slk_get_state.argtypes = [vp, vp, vp, ip]
    lib.slk_mean_device_ptr.argtypes = [vp]
    lib.slk_mean_device_ptr.restype = vp
    lib.slk_cov_device_ptr.argtypes = [vp]
    lib.slk_cov_device_ptr.restype = vp
    lib.slk_predict.argtypes = [vp, ip, vp, ip, vp, ip, ip]
    lib.slk_dead_reckon.argtypes = [vp, vp, ip, vp, ip]
    lib.slk_update_ekf.argtypes = [vp, vp, vp, vp, ip, vp, ip, ip, ip]
    lib.slk_update.argtypes = [vp, ip, vp, ip, vp, ip, vp, ip, ip, ip]
    lib.slk_step.argtypes = [vp, ip, vp, ip, vp, ip, ip, vp, ip, vp, ip, vp, ip, ip, ip]
    lib.slk_predict_sigma_points.argtypes = [vp, vp, ip]
    lib.slk_predict_from_sigma.argtypes = [vp, vp, vp, ip, ip]
    lib.slk_update_sigma_points.argtypes = [vp, vp, ip]
    lib.slk_update_from_sigma.argtypes = [vp, vp, vp, ip, vp, ip, ip, ip]
    lib.slk_usckf_cloning.argtypes = [vp, ip]
    lib.slk_usckf_set_measurement.argtypes = [vp, ip, vp, ip, vp, ip]
    lib.slk_msckf_resize.argtypes = [vp, ip]
    lib.slk_msckf_clone_pose.argtypes = [vp]
    lib.slk_msckf_drop_clone.argtypes = [vp, ip]
    lib.slk_get_outliers.argtypes = [vp, vp, ip]
    lib.slk_get_status.argtypes = [vp, vp, ip]
    lib.slk_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    lib.slk_selftest_mfma.argtypes = [ip]
    lib.slk_set_rebuild_precision.argtypes = [vp, ip]
    lib.slk_check_sigma_points.argtypes = [vp, vp, vp, ip]
    lib.slk_update_innovation.argtypes = [vp, ip, vp, ip, vp, vp, ip, vp, ip, vp, ip]
    lib.slk_update_selected.argtypes = [vp, ip, vp, ip, vp, vp, ip, vp, ip, vp, ip]
    lib.slk_transform_compose.argtypes = [vp, vp, vp, vp, vp, vp, vp, ip, ip]
    lib.slk_dead_reckon_pose.argtypes = [vp, vp, ip, vp, ip, vp, vp, vp, ip, ip]
    lib.slk_adaptive_create.argtypes = [ip, ip, C.c_uint, C.c_uint, C.c_double, C.c_uint, vp, C.POINTER(vp)]
    lib.slk_adaptive_destroy.argtypes = [vp]
    lib.slk_adaptive_destroy.restype = None
    lib.slk_adaptive_matrix.argtypes = [vp, ip, vp, vp, vp, vp, vp, ip, vp, ip]
    lib.slk_nees.argtypes = [vp, vp, ip, ip, vp, vp, ip]
    lib.slk_sample_states.argtypes = [vp, vp, ip, vp, ip]
    lib.slk_step_n.argtypes = [vp, C.POINTER(Traj), ip]
    lib.slk_step_n_slide.argtypes = [vp, C.POINTER(Traj), vp, ip]
    lib.slk_msckf_slide.argtypes = [vp, ip]
    lib.slk_ekf_linearize.argtypes = [vp, ip, vp, ip, ip, vp, vp, ip]
    lib.slk_update_ekf_model.argtypes = [vp, ip, vp, ip, vp, ip, vp, ip, ip, ip]
    lib.slk_step_ekf.argtypes = [vp, ip, vp, ip, vp, ip, ip, vp, ip, vp, ip, vp, ip, ip, ip]
    lib.slk_step_n_ekf.argtypes = [vp, C.POINTER(Traj), vp, ip]
    lib.slk_nis.argtypes = [vp, ip, vp, ip, vp, vp, ip, vp, ip, vp, vp, ip]
    lib.slk_get_sigma.argtypes = [vp, ip, ip, vp, ip]
    lib.slk_step_n_diag.argtypes = [vp, C.POINTER(Traj), vp, ip, C.POINTER(TrajDiag), ip]
    lib.slk_ensemble_moments.argtypes = [vp, ip, vp, vp, ip, ip, vp, vp, vp, vp, ip]
    lib.slk_gather_states.argtypes = [vp, vp, ip]
    lib.slk_track_linearize.argtypes = [vp, vp, ip, ip, ip, vp, ip, vp, ip, vp, vp, vp, ip]
    lib.slk_update_tracks.argtypes = [vp, vp, ip, ip, ip, vp, ip, vp, ip, vp, ip]
    lib.slk_step_tracks.argtypes = [vp, ip, vp, ip, vp, ip, vp, ip, ip, ip, vp, ip, vp, ip, vp, ip]
    if path is None:
        _lib = lib
    return lib


def device_count():
    return load_library().slk_device_count()


def _check(rc, what):
    if rc != 0:
        msg = load_library().slk_last_error()
        raise SlkError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def _is_dev(a):
    return hasattr(a, "data_ptr")


class _Arg:
    """One marshalled argument: pointer, per-filter stride (0 = shared), location, keep-alive."""

    def __init__(self, ptr, stride, where, keep):
        self.ptr, self.stride, self.where, self.keep = ptr, stride, where, keep


def _rows(a, B, width):
    """Per-filter rows [B, >=width] or one shared row [>=width].  numpy -> host, torch cuda tensor -> device."""
    if a is None:
        return _Arg(None, 0, None, None)
    if _is_dev(a):
        assert a.is_contiguous()
        stride = 0 if a.dim() == 1 else int(a.stride(0))
        assert (a.shape[-1] if a.dim() > 1 else a.numel()) >= width
        return _Arg(a.data_ptr(), stride, DEVICE if a.is_cuda else HOST, a)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim == 1:
        assert a.size >= width, (a.size, width)
        return _Arg(a.ctypes.data, 0, HOST, a)
    a = np.ascontiguousarray(a.reshape(a.shape[0], -1))
    assert a.shape[0] == B and a.shape[1] >= width, (a.shape, B, width)
    return _Arg(a.ctypes.data, a.shape[1], HOST, a)


def _zrows(z, B, m, name="z"):
    """Measurement rows: the C ABI has no stride for z, slk_update / slk_step always read [B][m] doubles.  A single
    row is therefore broadcast to every filter here (numpy), tensors must already hold B * m contiguous float64 values."""
    if _is_dev(z):
        if not z.is_contiguous() or z.numel() != B * m or str(z.dtype) != "torch.float64":
            raise SlkError(f"{name} must be a contiguous float64 tensor of {B} x {m} values, got {z.dtype} {tuple(z.shape)}")
        return _Arg(z.data_ptr(), m, DEVICE if z.is_cuda else HOST, z)
    z = np.asarray(z, dtype=np.float64)
    assert z.shape[-1] == m and (z.ndim == 1 or z.shape[0] in (1, B)), (z.shape, B, m)
    a = np.ascontiguousarray(np.broadcast_to(z.reshape(-1, m), (B, m)))
    return _Arg(a.ctypes.data, m, HOST, a)


def _mat(M, B, n):
    """n x n matrix, shared [n, n] or per-filter [B, n, n] (numpy: row/col indexable; torch device tensors
    must already be column-major per filter -- symmetric matrices are either way)."""
    if _is_dev(M):
        if not M.is_contiguous() or str(M.dtype) != "torch.float64" or tuple(M.shape) not in ((n, n), (B, n, n)):
            raise SlkError(f"matrix must be a contiguous float64 tensor [{n}, {n}] or [{B}, {n}, {n}], "
                           f"got {M.dtype} {tuple(M.shape)}")
        stride = 0 if M.dim() == 2 else int(M.stride(0))
        return _Arg(M.data_ptr(), stride, DEVICE if M.is_cuda else HOST, M)
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 2:
        assert M.shape == (n, n), (M.shape, n)
        a = np.ascontiguousarray(M.T)
        return _Arg(a.ctypes.data, 0, HOST, a)
    assert M.shape == (B, n, n), (M.shape, B, n)
    a = np.ascontiguousarray(np.transpose(M, (0, 2, 1)))
    return _Arg(a.ctypes.data, n * n, HOST, a)


def _steps(a, T, B, width, name, exact=False, per_filter=False):
    """A per-step input with a leading T axis: (pointer, per-filter stride, per-step stride, where, keep-alive).
    [T, w] = one shared row per step, [T, B, w] = per-filter rows (per_filter: only those); w >= width (exact: w ==
    width).  A stride of 0 on the T axis (np.broadcast_to, torch expand) shares one block over every step without a
    copy.  The C ABI reads whole blocks of these sizes, so every shape is checked here."""
    if a is None:
        return None
    shape = tuple(a.shape)
    ok = len(shape) == 3 or (len(shape) == 2 and not per_filter)
    ok = ok and shape[0] == T and (len(shape) == 2 or shape[1] == B)
    ok = ok and (shape[-1] == width if exact else shape[-1] >= width)
    if not ok:
        want = f"[{T}, {B}, {width}]" if per_filter else f"[{T}, ({B},) {'' if exact else '>='}{width}]"
        raise SlkError(f"step_n: {name} must be {want}, got {shape}")
    if _is_dev(a):
        if not a[0].is_contiguous() or str(a.dtype) != "torch.float64":
            raise SlkError(f"step_n: {name} must be a float64 tensor with contiguous steps")
        return (a.data_ptr(), int(a.stride(1)) if a.dim() == 3 else 0, int(a.stride(0)), DEVICE if a.is_cuda else HOST, a)
    a = np.asarray(a, dtype=np.float64)
    if a.strides[0] == 0:
        blk = np.ascontiguousarray(a[0])
        return (blk.ctypes.data, a.shape[2] if a.ndim == 3 else 0, 0, HOST, blk)
    a = np.ascontiguousarray(a)
    return (a.ctypes.data, a.shape[2] if a.ndim == 3 else 0, int(np.prod(a.shape[1:])), HOST, a)


def _where(*args):
    ws = {a.where for a in args if a.where is not None}
    if len(ws) != 1:                                          # (a host address read as a device one is a page fault)
        raise SlkError("all arguments of one call must live on the same side (host or device)")
    return ws.pop()


def _np(model, m):
    return (m // 2) * 4 if model == MM_FEATURE_PROJ else (1 if model == MM_POSE_POSITION else 0)


class _FilterBatch:
    KIND = None

    def __init__(self, batch, device=0, stream=None, n_clones=0, nfk=0, nfkl=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        if self._lib.slk_device_count() <= 0:
            raise SlkError("no HIP device visible: slam-localization_amd has no CPU fallback")
        cfg = Config(self.KIND, batch, device, n_clones, nfk, nfkl, stream)
        _check(self._lib.slk_create(C.byref(cfg), C.byref(self._h)), "slk_create")
        self.B = batch

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.slk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- sizes
    @property
    def N(self):
        return self._lib.slk_dof(self._h)

    @property
    def Nq(self):
        return self._lib.slk_storage(self._h)

    def getDOF(self):                                         # State.hpp:373-376 / :590-593
        return self.N

    # ---- state
    def set_state(self, mean=None, P=None):
        N, Nq = self.N, self.Nq
        m = p = None
        if mean is not None:
            m = np.ascontiguousarray(np.broadcast_to(np.asarray(mean, dtype=np.float64), (self.B, Nq)))
        if P is not None:
            P = np.asarray(P, dtype=np.float64)
            P = np.broadcast_to(P, (self.B, N, N))
            p = np.ascontiguousarray(np.transpose(P, (0, 2, 1)))
        _check(self._lib.slk_set_state(self._h, m.ctypes.data if m is not None else None,
                                       p.ctypes.data if p is not None else None, HOST), "slk_set_state")

    def muState(self):                                        # Msckf.hpp:376-379 / Usckf.hpp:518-521
        m = np.empty((self.B, self.Nq))
        _check(self._lib.slk_get_state(self._h, m.ctypes.data, None, HOST), "slk_get_state")
        return m

    def _getP(self):
        N = self.N
        p = np.empty((self.B, N, N))
        _check(self._lib.slk_get_state(self._h, None, p.ctypes.data, HOST), "slk_get_state")
        return np.ascontiguousarray(np.transpose(p, (0, 2, 1)))

    def device_pointers(self):
        """(mean, P) device addresses of the resident state, for zero-copy callers.  Both change after clone_pose,
        drop_clone, slide and a Usckf setMeasurement (the state moves to the handle's second buffer pair): ask again
        after each.  The exact-shape Msckf steps and a slide of their result leave the strict upper triangle of P stale;
        slk_cov_device_ptr, called here, enqueues the pass that completes it on the handle's stream.  A covariance
        pointer fetched earlier stays valid as an address but not as a complete matrix: after any further step or slide
        its strict upper triangle is stale again, so re-fetch the pointer (call device_pointers() again) after the last
        step and before reading the upper triangle through it; the lower triangle and the diagonal are always current."""
        return self._lib.slk_mean_device_ptr(self._h), self._lib.slk_cov_device_ptr(self._h)

    def status(self):
        s = np.zeros(self.B, dtype=np.int32)
        _check(self._lib.slk_get_status(self._h, s.ctypes.data, HOST), "slk_get_status")
        return s

    def clear_status(self):
        _check(self._lib.slk_clear_status(self._h), "slk_clear_status")

    def outliers(self):
        o = np.zeros(self.B, dtype=np.uint32)
        _check(self._lib.slk_get_outliers(self._h, o.ctypes.data, HOST), "slk_get_outliers")
        return o

    def set_rebuild_precision(self, mode):
        """0 = fp64 (parity path), 1 = fp32 MFMA, 2 = bf16 operands / fp32 accumulation (precision sweep only)."""
        _check(self._lib.slk_set_rebuild_precision(self._h, int(mode)), "slk_set_rebuild_precision")

    def sync(self):
        _check(self._lib.slk_sync(self._h), "slk_sync")

    def timer_start(self):
        _check(self._lib.slk_timer_start(self._h), "slk_timer_start")

    def timer_stop(self):
        ms = C.c_float(0)
        _check(self._lib.slk_timer_stop(self._h, C.byref(ms)), "slk_timer_stop")
        return ms.value

    def _default_gate(self, gate):
        if gate is None:
            return 1 if self.KIND == MSCKF else 0             # Msckf.hpp:199 / Usckf.hpp:249
        return int(gate)

    def _model_params(self, model, params, m, what):
        if params is None:
            raise SlkError(f"{what}: the registered model needs its parameters ((m / 2) x landmark xyz, pose index)")
        return _rows(params, self.B, _np(model, m))

    # ---- Tier A: registered models
    def predict(self, model, u, Q):
        """predict(f, Q), f = registered process model `model` with inputs u (Msckf.hpp:89-95, Usckf.hpp:107-111)."""
        ua = _rows(u, self.B, 7 if model == PM_CONST_VELOCITY else 13)
        qa = _mat(Q, self.B, 12)
        _check(self._lib.slk_predict(self._h, model, ua.ptr, ua.stride, qa.ptr, qa.stride, _where(ua, qa)), "slk_predict")

    def update(self, z, model, params, R, gate=None):
        """update(z, h, R), h = registered measurement model (Msckf.hpp:196-213, Usckf.hpp:246-258)."""
        m = int(z.shape[-1])
        pa = _rows(params, self.B, _np(model, m)) if _np(model, m) else _Arg(None, 0, None, None)
        za, ra = _zrows(z, self.B, m), _mat(R, self.B, m)
        _check(self._lib.slk_update(self._h, model, pa.ptr, pa.stride, za.ptr, m, ra.ptr, ra.stride,
                                    self._default_gate(gate), _where(pa, za, ra)), "slk_update")

    def step(self, pmodel, u, Q, z, mmodel, params, R, gate=None):
        """predict + update fused into one launch (the benchmark's filter step)."""
        m = int(z.shape[-1])
        ua = _rows(u, self.B, 7 if pmodel == PM_CONST_VELOCITY else 13)
        qa = _mat(Q, self.B, 12)
        pa = _rows(params, self.B, _np(mmodel, m)) if _np(mmodel, m) else _Arg(None, 0, None, None)
        za, ra = _zrows(z, self.B, m), _mat(R, self.B, m)
        _check(self._lib.slk_step(self._h, pmodel, ua.ptr, ua.stride, qa.ptr, qa.stride, mmodel, pa.ptr, pa.stride,
                                  za.ptr, m, ra.ptr, ra.stride, self._default_gate(gate), _where(ua, qa, pa, za, ra)),
               "slk_step")

    def step_n(self, pmodel, u, Q, z, mmodel, params, R, gate=None, truth=None, nees_range=None, record_mean=False,
               record_outliers=False, slide=None, update="ukf", diag=()):
        """T fused steps in one call (slk_step_n): the same results as T calls of step() with the inputs of each step.
        update="ekf" (Msckf, slk_step_n_ekf): every step is step_ekf() instead of step() -- predict, then the EKF update
        from the registered model mmodel linearised on the device (N <= m <= 512 rows); the arguments, the records and
        slide= are handled exactly as for the default update="ukf".
        u [T, B, nu] or [T, nu], z [T, B, m], params [T, B, np] or [T, np] (or None), truth [T, B, Nq]: a leading T axis
        always (a stride of 0 there, np.broadcast_to / torch expand, shares one block over all steps); Q and R have the
        shapes step() takes and are shared over the steps.  Records: record_mean -> "mean" [T, B, Nq] (the mean after
        each step), record_outliers -> "outliers" [T, B], truth -> "nees" [T, B] (nees(truth[t], t0, n) after step t,
        nees_range = (t0, n), default the whole state).  numpy in -> host route, numpy records; torch device tensors in
        -> device route, device tensors out.
        slide (slk_step_n_slide): an int d slides the window after every step (drop clone d, clone the current pose),
        or a length-T sequence with -1 (no slide after that step) or d; the records of a step are taken after its
        slide.  The results are those of step() followed by drop_clone(d) + clone_pose() where d >= 0.
        diag (slk_step_n_diag): any of "nis", "logdet", "sigma" adds the records "nis" [T, B] (nis() of step t's update
        on the predicted state of step t), "logdet" [T, B] (its log det S) and "sigma" [T, B, N] (sigma() after step t);
        the state and every other record are bit-identical to the call without diag.  "nis" / "logdet" need
        update="ukf".  The default leaves the call what it was."""
        diag = (diag,) if isinstance(diag, str) else tuple(diag)
        if any(x not in ("nis", "logdet", "sigma") for x in diag):
            raise SlkError(f"step_n: diag takes 'nis', 'logdet', 'sigma', got {diag!r}")
        if update not in ("ukf", "ekf"):
            raise SlkError(f"step_n: update must be 'ukf' or 'ekf', got {update!r}")
        T = int(z.shape[0])
        m = int(z.shape[-1])
        B = self.B
        sched = None
        if slide is not None:
            if np.ndim(slide) == 0:
                sched = np.full(T, int(slide), dtype=np.int32)
            else:
                sched = np.asarray(slide)
                if sched.ndim != 1 or sched.shape[0] != T or not np.issubdtype(sched.dtype, np.integer):
                    raise SlkError(f"step_n: slide must be an int or {T} integers, got {sched.dtype} {sched.shape}")
                sched = np.ascontiguousarray(sched, dtype=np.int32)
        ua = _steps(u, T, B, 7 if pmodel == PM_CONST_VELOCITY else 13, "u")
        za = _steps(z, T, B, m, "z", exact=True, per_filter=True)
        npar = _np(mmodel, m)
        pa = _steps(params, T, B, npar, "params") if npar else None
        ta = _steps(truth, T, B, self.Nq, "truth", exact=True, per_filter=True)
        qa, ra = _mat(Q, B, 12), _mat(R, B, m)
        parts = [x for x in (ua, za, pa, ta) if x is not None]
        where = _where(qa, ra, *[_Arg(x[0], x[1], x[3], x[4]) for x in parts])
        t0, n = (0, self.N) if nees_range is None else (int(nees_range[0]), int(nees_range[1]))
        tr = Traj()
        tr.T = T
        tr.pmodel, tr.u, tr.u_stride, tr.u_tstride = pmodel, ua[0], ua[1], ua[2]
        tr.Q, tr.q_stride, tr.q_tstride = qa.ptr, qa.stride, 0
        tr.mmodel = mmodel
        if pa is not None:
            tr.params, tr.p_stride, tr.p_tstride = pa[0], pa[1], pa[2]
        tr.z, tr.m, tr.z_tstride = za[0], m, za[2]
        tr.R, tr.r_stride, tr.r_tstride = ra.ptr, ra.stride, 0
        tr.gate = self._default_gate(gate)
        out = {}
        if where == DEVICE:
            import torch
            dev = z.device
            torch.cuda.current_stream(dev).synchronize()      # (the handle's stream does not wait for torch's)
            if record_mean:
                out["mean"] = torch.empty((T, B, self.Nq), dtype=torch.float64, device=dev)
            if record_outliers:
                out["outliers"] = torch.empty((T, B), dtype=torch.uint32, device=dev)
            if truth is not None:
                out["nees"] = torch.empty((T, B), dtype=torch.float64, device=dev)
            for x in diag:
                out[x] = torch.empty((T, B, self.N) if x == "sigma" else (T, B), dtype=torch.float64, device=dev)
            ptr = {k: v.data_ptr() for k, v in out.items()}
        else:
            if record_mean:
                out["mean"] = np.empty((T, B, self.Nq))
            if record_outliers:
                out["outliers"] = np.empty((T, B), dtype=np.uint32)
            if truth is not None:
                out["nees"] = np.empty((T, B))
            for x in diag:
                out[x] = np.empty((T, B, self.N) if x == "sigma" else (T, B))
            ptr = {k: v.ctypes.data for k, v in out.items()}
        tr.mean_hist, tr.outliers_hist, tr.nees_hist = ptr.get("mean"), ptr.get("outliers"), ptr.get("nees")
        if ta is not None:
            tr.truth, tr.truth_tstride, tr.nees_t0, tr.nees_n = ta[0], ta[2], t0, n
        if diag:
            dg = TrajDiag(ptr.get("nis"), ptr.get("logdet"), ptr.get("sigma"))
            _check(self._lib.slk_step_n_diag(self._h, C.byref(tr), sched.ctypes.data if sched is not None else None,
                                             int(update == "ekf"), C.byref(dg), where), "slk_step_n_diag")
        elif update == "ekf":
            _check(self._lib.slk_step_n_ekf(self._h, C.byref(tr), sched.ctypes.data if sched is not None else None, where),
                   "slk_step_n_ekf")
        elif sched is None:
            _check(self._lib.slk_step_n(self._h, C.byref(tr), where), "slk_step_n")
        else:
            _check(self._lib.slk_step_n_slide(self._h, C.byref(tr), sched.ctypes.data, where), "slk_step_n_slide")
        if where == DEVICE:
            self.sync()                                        # torch may read the records on any stream
        return out

    # ---- Tier B: opaque host functors (the reference's boost::bind form)
    def predict_sigma_points(self):
        X = np.empty((self.B, 25, 13))
        _check(self._lib.slk_predict_sigma_points(self._h, X.ctypes.data, HOST), "slk_predict_sigma_points")
        return X

    def dead_reckon(self, u):
        """DeadReckon::updatePose delta poses (src/core/DeadReckon.hpp:129-239) for the batch: u = dt v0 w0 v1 w1
        (shared row or [B, 13]) -> [B, 13] = dpos dquat velocity angular_velocity, the `u` of PM_DELTA_POSE.
        numpy in -> numpy out; a torch device tensor in -> a torch device tensor out."""
        ua = _rows(u, self.B, 13)
        if ua.where == DEVICE:
            import torch
            out = torch.empty((self.B, 13), dtype=torch.float64, device=u.device)
            _check(self._lib.slk_dead_reckon(self._h, ua.ptr, ua.stride, out.data_ptr(), DEVICE), "slk_dead_reckon")
            return out
        out = np.empty((self.B, 13))
        _check(self._lib.slk_dead_reckon(self._h, ua.ptr, ua.stride, out.ctypes.data, HOST), "slk_dead_reckon")
        return out

    def transform_compose(self, t2, cov2, t1, cov1, additive=False):
        """TransformWithUncertainty::operator* (src/core/Transform.cpp:215-254) for the batch: t [B, 7] = pos quat,
        cov [B, 6, 6] in [r t] order or None (no uncertainty) -> (t [B, 7], cov [B, 6, 6]).  additive=True is the other
        branch of DeadReckon::updatePose's Affine3d overload (src/core/DeadReckon.hpp:317-323)."""
        B = self.B

        def cm(c):
            if c is None:
                return None
            return np.ascontiguousarray(np.transpose(np.broadcast_to(np.asarray(c, dtype=np.float64), (B, 6, 6)), (0, 2, 1)))
        a2 = np.ascontiguousarray(np.broadcast_to(np.asarray(t2, dtype=np.float64), (B, 7)))
        a1 = np.ascontiguousarray(np.broadcast_to(np.asarray(t1, dtype=np.float64), (B, 7)))
        c2, c1 = cm(cov2), cm(cov1)
        to, co = np.empty((B, 7)), np.empty((B, 6, 6))
        _check(self._lib.slk_transform_compose(self._h, a2.ctypes.data, c2.ctypes.data if c2 is not None else None,
                                               a1.ctypes.data, c1.ctypes.data if c1 is not None else None,
                                               to.ctypes.data, co.ctypes.data, int(bool(additive)), HOST), "slk_transform_compose")
        return to, np.ascontiguousarray(np.transpose(co, (0, 2, 1)))

    def dead_reckon_pose(self, u, velcov, prev, post, use_tf=False):
        """DeadReckon::updatePose, RigidBodyState overload (src/core/DeadReckon.hpp:129-239) for the batch.  Records as in
        include/slk.h: prev [B, 25], post [B, 49] (accumulated into without use_tf), -> (post [B, 49], delta [B, 31]);
        velcov [6, 6] shared or [B, 6, 6]."""
        B = self.B
        ua = _rows(u, B, 13)
        vc = np.asarray(velcov, dtype=np.float64)
        if vc.ndim == 2:
            vca, cs = np.ascontiguousarray(vc.T), 0
        else:
            vca, cs = np.ascontiguousarray(np.transpose(vc, (0, 2, 1))), 36
        pv = np.ascontiguousarray(np.broadcast_to(np.asarray(prev, dtype=np.float64), (B, 25)))
        po = np.array(np.broadcast_to(np.asarray(post, dtype=np.float64), (B, 49)), dtype=np.float64, order="C")
        de = np.empty((B, 31))
        _check(self._lib.slk_dead_reckon_pose(self._h, ua.ptr, ua.stride, vca.ctypes.data, cs, pv.ctypes.data, po.ctypes.data,
                                              de.ctypes.data, int(bool(use_tf)), HOST), "slk_dead_reckon_pose")
        return po, de

    def nees(self, truth, t0=0, n=None, error=False):
        """Normalised estimation error squared of every filter on the tangent indices [t0, t0 + n) (default: to N):
        e = (truth [-] mu) on the range, nees [B] = e^T P_ss^-1 e with P_ss the principal block of P there.  truth
        [B, Nq] (or one shared row) in the storage layout.  error=True returns (nees, e [B, n]).  A block that is not
        positive definite gives NaN for that filter.  numpy in -> numpy out; a torch device tensor in -> torch device
        tensors out (truth [B, Nq], contiguous float64; torch's stream is synchronised before the call, the handle's
        after it)."""
        n = self.N - int(t0) if n is None else int(n)
        B = self.B
        if truth is None:
            tp, where, dev = None, HOST, None
        elif _is_dev(truth):
            if not truth.is_contiguous() or truth.numel() != B * self.Nq or str(truth.dtype) != "torch.float64":
                raise SlkError(f"nees: truth must be a contiguous [{B}, {self.Nq}] tensor, got {tuple(truth.shape)}")
            tp, where, dev = truth.data_ptr(), DEVICE, truth.device
        else:
            truth = np.asarray(truth, dtype=np.float64)
            if truth.shape[-1] != self.Nq or truth.ndim > 2 or (truth.ndim == 2 and truth.shape[0] not in (1, B)):
                raise SlkError(f"nees: truth must be [{B}, {self.Nq}], got {truth.shape}")
            truth = np.ascontiguousarray(np.broadcast_to(truth.reshape(-1, self.Nq), (B, self.Nq)))
            tp, where, dev = truth.ctypes.data, HOST, None
        ne = max(n, 0)
        if where == DEVICE:
            import torch
            torch.cuda.current_stream(dev).synchronize()      # (the handle's stream does not wait for torch's)
            out = torch.empty(B, dtype=torch.float64, device=dev)
            err = torch.empty((B, ne), dtype=torch.float64, device=dev) if error else None
            optr, eptr = out.data_ptr(), (err.data_ptr() if error else None)
        else:
            out = np.empty(B)
            err = np.empty((B, ne)) if error else None
            optr, eptr = out.ctypes.data, (err.ctypes.data if error else None)
        _check(self._lib.slk_nees(self._h, tp, int(t0), n, optr, eptr, where), "slk_nees")
        if where == DEVICE:
            self.sync()                                        # torch may read the outputs on any stream
        return (out, err) if error else out

    def nis(self, z, model, params, R, logdet=False):
        """Normalised innovation squared nu^T S^-1 nu [B] of the update that update(z, model, params, R) would make (all
        rows, before any gate); the filter is not modified.  logdet=True returns (nis, log det S): the Gaussian
        log-likelihood of z is -0.5 * (nis + logdet + m * log(2 pi)).  An S that is not positive definite gives NaN for
        that filter.  Arguments as update() takes them; numpy in -> numpy out, torch device tensors in -> torch device
        tensors out (torch's stream is synchronised before the call, the handle's after it)."""
        m = int(z.shape[-1])
        pa = _rows(params, self.B, _np(model, m)) if _np(model, m) else _Arg(None, 0, None, None)
        za, ra = _zrows(z, self.B, m), _mat(R, self.B, m)
        return self._nis(model, pa, None, za, m, ra, logdet, _where(pa, za, ra), z)

    def _nis(self, model, pa, Zptr, za, m, ra, logdet, where, ztensor):
        B = self.B
        if where == DEVICE:
            import torch
            dev = ztensor.device
            torch.cuda.current_stream(dev).synchronize()      # (the handle's stream does not wait for torch's)
            out = torch.empty(B, dtype=torch.float64, device=dev)
            ld = torch.empty(B, dtype=torch.float64, device=dev) if logdet else None
            optr, lptr = out.data_ptr(), (ld.data_ptr() if logdet else None)
        else:
            out = np.empty(B)
            ld = np.empty(B) if logdet else None
            optr, lptr = out.ctypes.data, (ld.ctypes.data if logdet else None)
        _check(self._lib.slk_nis(self._h, model, pa.ptr, pa.stride, Zptr, za.ptr, m, ra.ptr, ra.stride, optr, lptr, where),
               "slk_nis")
        if where == DEVICE:
            self.sync()                                        # torch may read the outputs on any stream
        return (out, ld) if logdet else out

    def nis_functor(self, z, h, R, logdet=False):
        """nis() with an arbitrary Python callable h: full state [Nq] -> z [m], applied to the sigma points on the host
        (the Tier-B form, as update_functor)."""
        X = self.update_sigma_points()
        Z = np.ascontiguousarray([[h(x) for x in Xb] for Xb in X], dtype=np.float64)
        m = Z.shape[-1]
        za, ra = _zrows(np.asarray(z, dtype=np.float64), self.B, m), _mat(np.asarray(R), self.B, m)
        return self._nis(MODEL_EXTERNAL, _Arg(None, 0, None, None), Z.ctypes.data, za, m, ra, logdet, HOST, None)

    def sigma(self, t0=0, n=None):
        """Standard deviations sqrt(diag P) [B, n] on the tangent indices [t0, t0 + n) (default: to N), read from the
        diagonal on the device: P is not downloaded and a lower-only P is not completed.  A negative or NaN diagonal
        entry gives NaN."""
        n = self.N - int(t0) if n is None else int(n)
        out = np.empty((self.B, max(n, 0)))
        _check(self._lib.slk_get_sigma(self._h, int(t0), n, out.ctypes.data, HOST), "slk_get_sigma")
        return out

    def ensemble_moments(self, weights=None, truth=None, t0=0, n=None, groups=1, ess=False, device=None):
        """Moments across the filters of the batch, or of `groups` = G equal groups of consecutive filters, on the tangent
        indices [t0, t0 + n) (default: to N).  weights [B] (None = uniform) are normalised per group.  Returns a dict:
          truth given (error mode):  "center" [G, n] = the weighted mean of e_b = (truth_b [-] mu_b) (the bias), "spread"
                                     [G, n, n] = the weighted covariance of e_b about it;
          truth None (mixture mode): "center" [G, Nq] = the weighted manifold mean of the means (whole state, storage
                                     layout), "spread" [G, n, n] = sum w_b d_b d_b^T, d_b = (mu_b [-] center) on the range;
          both: "mean_cov" [G, n, n] = sum w_b P_b[range, range]; ess=True adds "ess" [G] = (sum w)^2 / sum w^2.
        The moment-matched covariance of the mixture is spread + mean_cov; population sums (no Bessel factor).  A group
        with a negative or non-finite weight or a weight sum that is not > 0 gets NaN outputs.  The filters are not
        modified and P is not downloaded.  numpy in -> numpy out; torch device tensors in (weights and / or truth,
        contiguous float64) -> torch device tensors out (torch's stream is synchronised before the call, the handle's
        after it).  device = a torch device asks for device tensors out when there is no input to tell by (uniform
        weights, mixture mode)."""
        B, Nq, G = self.B, self.Nq, int(groups)
        n = self.N - int(t0) if n is None else int(n)
        devs = [a for a in (weights, truth) if a is not None and _is_dev(a)]
        if devs and len(devs) != sum(a is not None for a in (weights, truth)):
            raise SlkError("all arguments of one call must live on the same side (host or device)")
        where = DEVICE if devs or (device is not None and weights is None and truth is None) else HOST
        keep = []

        def arg(a, count, name):
            if a is None:
                return None
            if _is_dev(a):
                if not a.is_contiguous() or a.numel() != count or str(a.dtype) != "torch.float64" or not a.is_cuda:
                    raise SlkError(f"ensemble_moments: {name} must be a contiguous float64 device tensor of {count} values")
                keep.append(a)
                return a.data_ptr()
            a = np.asarray(a, dtype=np.float64)
            if name == "truth":
                if a.shape[-1] != Nq or a.ndim > 2 or (a.ndim == 2 and a.shape[0] not in (1, B)):
                    raise SlkError(f"ensemble_moments: truth must be [{B}, {Nq}], got {a.shape}")
                a = np.broadcast_to(a.reshape(-1, Nq), (B, Nq))
            elif a.size != count:
                raise SlkError(f"ensemble_moments: {name} must hold {count} values, got {a.shape}")
            a = np.ascontiguousarray(a)
            keep.append(a)
            return a.ctypes.data

        wp, tp = arg(weights, B, "weights"), arg(truth, B * Nq, "truth")
        Ge, ne = max(G, 0), max(n, 0)
        nc = ne if truth is not None else Nq
        if where == DEVICE:
            import torch
            dev = devs[0].device if devs else torch.device(device)
            torch.cuda.current_stream(dev).synchronize()      # (the handle's stream does not wait for torch's)
            mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
            ptr = lambda a: a.data_ptr()
        else:
            mk = lambda *shape: np.empty(shape)
            ptr = lambda a: a.ctypes.data
        out = {"center": mk(Ge, nc), "spread": mk(Ge, ne, ne), "mean_cov": mk(Ge, ne, ne)}
        if ess:
            out["ess"] = mk(Ge)
        _check(self._lib.slk_ensemble_moments(self._h, G, wp, tp, int(t0), n, ptr(out["center"]), ptr(out["spread"]),
                                              ptr(out["mean_cov"]), ptr(out["ess"]) if ess else None, where),
               "slk_ensemble_moments")
        if where == DEVICE:
            self.sync()                                        # torch may read the outputs on any stream
        return out                                             # (spread and mean_cov are symmetric: row- or column-major)

    def gather(self, src):
        """Filter b becomes a copy of the old filter src[b] (mean, P, status bits, outlier count): resampling, pruning,
        fan-out, in one launch on the device.  src [B] integers: numpy (an index outside 0 .. B - 1 raises, nothing
        changed) or a torch int32 device tensor (such a filter keeps its state and gets ST_BAD_INDEX).  device_pointers()
        change."""
        if _is_dev(src):
            if not src.is_contiguous() or src.numel() != self.B or str(src.dtype) != "torch.int32" or not src.is_cuda:
                raise SlkError(f"gather: src must be a contiguous int32 device tensor of {self.B} indices")
            import torch
            torch.cuda.current_stream(src.device).synchronize()
            _check(self._lib.slk_gather_states(self._h, src.data_ptr(), DEVICE), "slk_gather_states")
            self.sync()                                        # (src may be released after the call)
            return
        src = np.asarray(src)
        if src.size != self.B or not np.issubdtype(src.dtype, np.integer):
            raise SlkError(f"gather: src must be {self.B} integers, got {src.dtype} {src.shape}")
        big = np.ascontiguousarray(src.reshape(-1), dtype=np.int64)
        if big.size and (big.min() < -2 ** 31 or big.max() >= 2 ** 31):
            raise SlkError("gather: index outside 0 .. B - 1")
        idx = np.ascontiguousarray(big, dtype=np.int32)
        _check(self._lib.slk_gather_states(self._h, idx.ctypes.data, HOST), "slk_gather_states")

    def sample_states(self, noise):
        """Gaussian draws from every filter's own (mu, P): out [B, S, Nq] = mu [+] (L n) for noise [B, S, N] (e.g. standard
        normal), L the lower Cholesky factor of P (the factor the sigma points are drawn from).  A P that is not
        positive definite fills that filter's rows with NaN.  numpy in -> numpy out; a torch device tensor in -> a
        torch device tensor out."""
        B, N, Nq = self.B, self.N, self.Nq
        if noise is None:
            _check(self._lib.slk_sample_states(self._h, None, 1, None, HOST), "slk_sample_states")
        if not _is_dev(noise):
            noise = np.asarray(noise, dtype=np.float64)
        if noise.ndim != 3 or noise.shape[0] != B or noise.shape[2] != N:
            raise SlkError(f"sample_states: noise must be [{B}, S, {N}], got {tuple(noise.shape)}")
        S = int(noise.shape[1])
        if _is_dev(noise):
            import torch
            if not noise.is_contiguous() or str(noise.dtype) != "torch.float64":
                raise SlkError("sample_states: noise must be a contiguous float64 tensor")
            torch.cuda.current_stream(noise.device).synchronize()
            out = torch.empty((B, max(S, 0), Nq), dtype=torch.float64, device=noise.device)
            _check(self._lib.slk_sample_states(self._h, noise.data_ptr(), S, out.data_ptr(), DEVICE), "slk_sample_states")
            self.sync()
            return out
        nz = np.ascontiguousarray(noise, dtype=np.float64)
        out = np.empty((B, max(S, 0), Nq))
        _check(self._lib.slk_sample_states(self._h, nz.ctypes.data if S > 0 else None, S, out.ctypes.data, HOST),
               "slk_sample_states")
        return out

    def predict_functor(self, f, Q):
        """predict(f, Q) with an arbitrary Python callable f: state[13] -> state[13], applied on the host."""
        X = self.predict_sigma_points()
        Y = np.ascontiguousarray([[f(x) for x in Xb] for Xb in X], dtype=np.float64)
        qa = _mat(np.asarray(Q), self.B, 12)
        _check(self._lib.slk_predict_from_sigma(self._h, Y.ctypes.data, qa.ptr, qa.stride, HOST), "slk_predict_from_sigma")

    def update_sigma_points(self):
        X = np.empty((self.B, 2 * self.N + 1, self.Nq))
        _check(self._lib.slk_update_sigma_points(self._h, X.ctypes.data, HOST), "slk_update_sigma_points")
        return X

    def update_functor(self, z, h, R, gate=None):
        """update(z, h, R) with an arbitrary Python callable h: full state [Nq] -> z [m]."""
        X = self.update_sigma_points()
        Z = np.ascontiguousarray([[h(x) for x in Xb] for Xb in X], dtype=np.float64)
        m = Z.shape[-1]
        z = np.ascontiguousarray(np.broadcast_to(np.asarray(z, dtype=np.float64), (self.B, m)))
        ra = _mat(np.asarray(R), self.B, m)
        _check(self._lib.slk_update_from_sigma(self._h, Z.ctypes.data, z.ctypes.data, m, ra.ptr, ra.stride,
                                               self._default_gate(gate), HOST), "slk_update_from_sigma")


class Msckf(_FilterBatch):
    """Batched localization::Msckf<MultiState, State> (reference src/filters/Msckf.hpp)."""
    KIND = MSCKF

    def __init__(self, mean, P, device=0, stream=None):
        mean = np.atleast_2d(np.asarray(mean, dtype=np.float64))
        B, Nq = mean.shape
        k = (Nq - 13) // 7
        assert Nq == 13 + 7 * k, "mean must hold State(13) + k * SensorState(7)"
        super().__init__(B, device, stream, n_clones=k)
        self.set_state(mean, P)                              # Msckf(state, P0), Msckf.hpp:80-85

    def muSingleState(self):                                 # Msckf.hpp:356-361
        return self.muState()[:, :13]

    def getPk(self):                                         # Msckf.hpp:386-389
        return self._getP()

    def setPk(self, P):                                      # Msckf.hpp:391-395
        self.set_state(None, P)

    def getPkSingleState(self):                              # Msckf.hpp:368-374
        return self._getP()[:, :12, :12]

    def update_ekf(self, z, zmean, H, R, gate=True):
        """EKF update(z, h, H, R) (Msckf.hpp:284-349): zmean [B, m] = h(mu), H [B, m, N] = its Jacobian (numpy, row/col
        indexable), evaluated by the caller at the current mean like the reference's functor h(mu_state, H).
        Tensors are taken as they are: z, zmean [B, m], H [B, N, m] (= m x N column-major per filter), R [m, m] or
        [B, m, m] column-major, all contiguous float64 and all on the same side; torch's stream is synchronised before a
        device launch."""
        B, N = self.B, self.N
        m = int(np.shape(z)[-1])
        za, zma, ra = _zrows(z, B, m), _zrows(zmean, B, m, "zmean"), _mat(R, B, m)
        if _is_dev(H):
            ha = _zrows(H, B, m * N, "H")
        else:
            Hc = np.ascontiguousarray(np.transpose(np.asarray(H, dtype=np.float64).reshape(B, m, N), (0, 2, 1)))
            ha = _Arg(Hc.ctypes.data, m * N, HOST, Hc)
        where = _where(za, zma, ha, ra)
        if where == DEVICE:
            import torch
            torch.cuda.current_stream(H.device).synchronize()  # (the handle's stream does not wait for torch's)
        _check(self._lib.slk_update_ekf(self._h, za.ptr, zma.ptr, ha.ptr, m, ra.ptr, ra.stride, int(bool(gate)), where),
               "slk_update_ekf")

    def ekf_linearize(self, model, params, m):
        """zmean [B, m] = h(mu) and H [B, m, N] = dh/d(tangent) at the resident mean of the registered measurement model
        `model` (MM_FEATURE_PROJ), computed on the device (slk_ekf_linearize); the filter is not modified.  params as
        update() takes them.  numpy params -> numpy arrays.  A torch device tensor -> device tensors: H is a [B, m, N]
        view of the column-major storage, so H.transpose(1, 2) is the contiguous [B, N, m] tensor update_ekf() takes."""
        B, N, m = self.B, self.N, int(m)
        pa = self._model_params(model, params, m, "ekf_linearize")
        if pa.where == DEVICE:
            import torch
            torch.cuda.current_stream(params.device).synchronize()   # (the handle's stream does not wait for torch's)
            zm = torch.empty((B, m), dtype=torch.float64, device=params.device)
            Hs = torch.empty((B, N, m), dtype=torch.float64, device=params.device)
            _check(self._lib.slk_ekf_linearize(self._h, model, pa.ptr, pa.stride, m, zm.data_ptr(), Hs.data_ptr(), DEVICE),
                   "slk_ekf_linearize")
            self.sync()                                        # torch may read the outputs on any stream
            return zm, Hs.transpose(1, 2)
        zm, Hs = np.empty((B, m)), np.empty((B, N, m))
        _check(self._lib.slk_ekf_linearize(self._h, model, pa.ptr, pa.stride, m, zm.ctypes.data, Hs.ctypes.data, HOST),
               "slk_ekf_linearize")
        return zm, np.ascontiguousarray(np.transpose(Hs, (0, 2, 1)))

    def update_ekf_model(self, z, model, params, R, gate=True):
        """EKF update(z, h, H, R) (Msckf.hpp:284-349) with h and H from the registered model `model` linearised at the
        resident mean on the device (slk_update_ekf_model): bit-identical to ekf_linearize() + update_ekf() on device
        tensors, with nothing leaving the device.  z, params, R as update() takes them; N <= m <= 512 rows.  Device
        tensors are read asynchronously on the handle's stream: keep them alive until sync()."""
        m = int(np.shape(z)[-1])
        pa = self._model_params(model, params, m, "update_ekf_model")
        za, ra = _zrows(z, self.B, m), _mat(R, self.B, m)
        where = _where(pa, za, ra)
        if where == DEVICE:
            import torch
            torch.cuda.current_stream(z.device).synchronize()  # (the handle's stream does not wait for torch's)
        _check(self._lib.slk_update_ekf_model(self._h, model, pa.ptr, pa.stride, za.ptr, m, ra.ptr, ra.stride,
                                              int(bool(gate)), where), "slk_update_ekf_model")

    def step_ekf(self, pmodel, u, Q, z, mmodel, params, R, gate=True):
        """predict() followed by update_ekf_model(), bit for bit, in one call (slk_step_ekf)."""
        m = int(np.shape(z)[-1])
        ua = _rows(u, self.B, 7 if pmodel == PM_CONST_VELOCITY else 13)
        qa = _mat(Q, self.B, 12)
        pa = self._model_params(mmodel, params, m, "step_ekf")
        za, ra = _zrows(z, self.B, m), _mat(R, self.B, m)
        where = _where(ua, qa, pa, za, ra)
        if where == DEVICE:
            import torch
            torch.cuda.current_stream(z.device).synchronize()  # (the handle's stream does not wait for torch's)
        _check(self._lib.slk_step_ekf(self._h, pmodel, ua.ptr, ua.stride, qa.ptr, qa.stride, mmodel, pa.ptr, pa.stride,
                                      za.ptr, m, ra.ptr, ra.stride, int(bool(gate)), where), "slk_step_ekf")

    def _track_args(self, tracks, sigma, chi2, what):
        """tracks [B, J, M, 3] or shared [J, M, 3] of { pose index, u, v }; sigma a number, a one-element array or [B];
        chi2 None or [2M - 2].  numpy -> host, torch device tensors -> device (a Python number for sigma goes where
        the tracks are)."""
        if tracks is None or sigma is None:
            raise SlkError(f"{what}: tracks and sigma are needed")
        shape = tuple(tracks.shape)
        if len(shape) not in (3, 4) or shape[-1] != 3 or (len(shape) == 4 and shape[0] != self.B):
            raise SlkError(f"{what}: tracks must be [{self.B}, J, M, 3] or [J, M, 3], got {shape}")
        J, M = int(shape[-3]), int(shape[-2])
        if _is_dev(tracks):
            import torch
            if not tracks.is_contiguous() or str(tracks.dtype) != "torch.float64":
                raise SlkError(f"{what}: tracks must be a contiguous float64 tensor")
            ta = _Arg(tracks.data_ptr(), 3 * J * M if len(shape) == 4 else 0, DEVICE if tracks.is_cuda else HOST, tracks)
            if not _is_dev(sigma):
                sigma = torch.as_tensor(np.atleast_1d(np.asarray(sigma, dtype=np.float64)), device=tracks.device)
            if chi2 is not None and not _is_dev(chi2):
                chi2 = torch.as_tensor(np.ascontiguousarray(chi2, dtype=np.float64), device=tracks.device)
        else:
            t = np.ascontiguousarray(tracks, dtype=np.float64)
            ta = _Arg(t.ctypes.data, 3 * J * M if len(shape) == 4 else 0, HOST, t)
        if _is_dev(sigma):
            if sigma.numel() not in (1, self.B) or not sigma.is_contiguous() or str(sigma.dtype) != "torch.float64":
                raise SlkError(f"{what}: sigma must hold 1 or {self.B} contiguous float64 values")
            sa = _Arg(sigma.data_ptr(), 0 if sigma.numel() == 1 else 1, DEVICE if sigma.is_cuda else HOST, sigma)
        else:
            sg = np.ascontiguousarray(np.atleast_1d(np.asarray(sigma, dtype=np.float64)).ravel())
            if sg.size not in (1, self.B):
                raise SlkError(f"{what}: sigma must hold 1 or {self.B} values, got {sg.size}")
            sa = _Arg(sg.ctypes.data, 0 if sg.size == 1 else 1, HOST, sg)
        if chi2 is None:
            ca = _Arg(None, 0, None, None)
        elif _is_dev(chi2):
            if chi2.numel() < 2 * M - 2 or not chi2.is_contiguous() or str(chi2.dtype) != "torch.float64":
                raise SlkError(f"{what}: chi2 must hold {2 * M - 2} contiguous float64 values")
            ca = _Arg(chi2.data_ptr(), 0, DEVICE if chi2.is_cuda else HOST, chi2)
        else:
            ch = np.ascontiguousarray(chi2, dtype=np.float64).ravel()
            if ch.size < 2 * M - 2:
                raise SlkError(f"{what}: chi2 must hold {2 * M - 2} values (indexed by 2 n_obs - 3), got {ch.size}")
            ca = _Arg(ch.ctypes.data, 0, HOST, ch)
        where = _where(ta, sa, ca)
        if where == DEVICE:
            import torch
            torch.cuda.current_stream(tracks.device).synchronize()   # (the handle's stream does not wait for torch's)
        return ta, sa, ca, J, M, where

    def track_linearize(self, tracks, sigma, m, chi2=None):
        """(r [B, m], H [B, m, N], feat [B, J, 4]) of the feature tracks at the resident mean (slk_track_linearize): each
        track is triangulated from the window's poses and projected onto the left null space of its landmark Jacobian;
        rows j (2M - 3) .. of track j, whitened by sigma, so that update_ekf(r, 0, H, I, gate=False) is the update.
        feat[b, j] = (X, flag): 1 used, 0 unused, -1 failed, -2 gated out by chi2 (indexed by 2 n_obs - 3).  The filter
        is not modified.  numpy -> numpy; device tensors -> device tensors, H a [B, m, N] view of the column-major storage
        as ekf_linearize() returns it."""
        B, N, m = self.B, self.N, int(m)
        ta, sa, ca, J, M, where = self._track_args(tracks, sigma, chi2, "track_linearize")
        if where == DEVICE:
            import torch
            r = torch.empty((B, m), dtype=torch.float64, device=tracks.device)
            Hs = torch.empty((B, N, m), dtype=torch.float64, device=tracks.device)
            feat = torch.empty((B, J, 4), dtype=torch.float64, device=tracks.device)
            _check(self._lib.slk_track_linearize(self._h, ta.ptr, ta.stride, J, M, sa.ptr, sa.stride, ca.ptr, m, r.data_ptr(),
                                                 Hs.data_ptr(), feat.data_ptr(), DEVICE), "slk_track_linearize")
            self.sync()                                        # torch may read the outputs on any stream
            return r, Hs.transpose(1, 2), feat
        r, Hs, feat = np.empty((B, m)), np.empty((B, N, m)), np.empty((B, J, 4))
        _check(self._lib.slk_track_linearize(self._h, ta.ptr, ta.stride, J, M, sa.ptr, sa.stride, ca.ptr, m, r.ctypes.data,
                                             Hs.ctypes.data, feat.ctypes.data, HOST), "slk_track_linearize")
        return r, np.ascontiguousarray(np.transpose(Hs, (0, 2, 1))), feat

    def update_tracks(self, tracks, sigma, m, chi2=None):
        """The multi-state-constraint update from feature tracks (slk_update_tracks): track_linearize() into a workspace
        of the handle, then the EKF update on it -- bit-identical to track_linearize() + update_ekf(r, 0, H, I,
        gate=False) on device tensors, with nothing leaving the device.  Returns feat [B, J, 4] (numpy or device tensor,
        as the tracks are).  A filter without a used track stays bit for bit what it was."""
        ta, sa, ca, J, M, where = self._track_args(tracks, sigma, chi2, "update_tracks")
        feat, fptr = self._feat_out(tracks, J, where)
        _check(self._lib.slk_update_tracks(self._h, ta.ptr, ta.stride, J, M, sa.ptr, sa.stride, ca.ptr, int(m), fptr, where),
               "slk_update_tracks")
        if where == DEVICE:
            self.sync()
        return feat

    def step_tracks(self, pmodel, u, Q, tracks, sigma, m, chi2=None):
        """predict() followed by update_tracks(), bit for bit, in one call (slk_step_tracks)."""
        ua = _rows(u, self.B, 7 if pmodel == PM_CONST_VELOCITY else 13)
        qa = _mat(Q, self.B, 12)
        ta, sa, ca, J, M, where = self._track_args(tracks, sigma, chi2, "step_tracks")
        if _where(ua, qa) != where:
            raise SlkError("all arguments of one call must live on the same side (host or device)")
        feat, fptr = self._feat_out(tracks, J, where)
        _check(self._lib.slk_step_tracks(self._h, pmodel, ua.ptr, ua.stride, qa.ptr, qa.stride, ta.ptr, ta.stride, J, M,
                                         sa.ptr, sa.stride, ca.ptr, int(m), fptr, where), "slk_step_tracks")
        if where == DEVICE:
            self.sync()
        return feat

    def _feat_out(self, tracks, J, where):
        if where == DEVICE:
            import torch
            feat = torch.empty((self.B, J, 4), dtype=torch.float64, device=tracks.device)
            return feat, feat.data_ptr()
        feat = np.empty((self.B, J, 4))
        return feat, feat.ctypes.data

    def checkSigmaPoints(self):
        """checkSigmaPoints() (Msckf.hpp:819-839) on the device: returns (max |covSigmaPoints - Pk| [B],
        |mu_state [-] muX| [B]); the reference asserts <= 1e-6 and == 0 (isZero(1e-12))."""
        ce, me = np.empty(self.B), np.empty(self.B)
        _check(self._lib.slk_check_sigma_points(self._h, ce.ctypes.data, me.ctypes.data, HOST), "slk_check_sigma_points")
        return ce, me

    def clone_pose(self):
        """Device-side muState().sensorsk.push_back(current pose) + setPk(J P J^T) (Msckf.hpp:381-395)."""
        _check(self._lib.slk_msckf_clone_pose(self._h), "slk_msckf_clone_pose")

    def drop_clone(self, index=0):
        """Device-side erase of clone `index` (0 = oldest) with its covariance rows / columns."""
        _check(self._lib.slk_msckf_drop_clone(self._h, int(index)), "slk_msckf_drop_clone")

    def slide(self, index=0):
        """One slide of the window, k unchanged: drop_clone(index) + clone_pose() in one launch, bit for bit."""
        _check(self._lib.slk_msckf_slide(self._h, int(index)), "slk_msckf_slide")


class Usckf(_FilterBatch):
    """Batched localization::Usckf<AugmentedState, State> (reference src/filters/Usckf.hpp)."""
    KIND = USCKF

    def __init__(self, mean=None, P=None, nfk=0, nfkl=0, state_single=None, P0_single=None, device=0, stream=None):
        if state_single is not None:
            # Usckf(single_state, P0_single), Usckf.hpp:90-103: place the state, then clone twice
            s = np.atleast_2d(np.asarray(state_single, dtype=np.float64))
            B = s.shape[0]
            super().__init__(B, device, stream, nfk=0, nfkl=0)
            mean = np.zeros((B, 39))
            mean[:, [6, 19, 32]] = 1.0
            mean[:, 26:39] = s
            P = np.zeros((B, 36, 36))
            P[:, 24:36, 24:36] = P0_single
            self.set_state(mean, P)
            self.cloning(STATEK_I)
            self.cloning(STATEK_L)
        else:
            mean = np.atleast_2d(np.asarray(mean, dtype=np.float64))
            B = mean.shape[0]
            assert mean.shape[1] == 39 + nfk + nfkl
            super().__init__(B, device, stream, nfk=nfk, nfkl=nfkl)
            self.set_state(mean, P)                          # Usckf(state, P0), Usckf.hpp:83-86

    def cloning(self, mode):                                 # Usckf.hpp:391-433
        _check(self._lib.slk_usckf_cloning(self._h, int(mode)), "slk_usckf_cloning")

    def setMeasurement(self, mode, z, R):                    # Usckf.hpp:322-389
        z = np.atleast_1d(np.asarray(z, dtype=np.float64))
        n = z.shape[-1]
        zb = np.ascontiguousarray(np.broadcast_to(z, (self.B, n)))
        Rc = np.ascontiguousarray(np.asarray(R, dtype=np.float64).T)
        assert Rc.shape == (n, n)                            # assert (z_k_i.size() == R.rows()), :325-327
        _check(self._lib.slk_usckf_set_measurement(self._h, int(mode), zb.ctypes.data, n, Rc.ctypes.data, HOST),
               "slk_usckf_set_measurement")

    def muSingleState(self, which=STATEK_I):                 # Usckf.hpp:457-478
        o = {STATEK: 0, STATEK_L: 13, STATEK_I: 26}.get(which, 26)
        return self.muState()[:, o:o + 13]

    def PkAugmentedState(self):                              # Usckf.hpp:523-526
        return self._getP()

    def PkSingleState(self, which=STATEK_I):                 # Usckf.hpp:493-516
        o = {STATEK: 0, STATEK_L: 12, STATEK_I: 24}.get(which, 24)
        return self._getP()[:, o:o + 12, o:o + 12]


class AdaptiveAttitudeCov:
    """Batch of B independent localization::AdaptiveAttitudeCov objects (src/filters/MeasurementModels.hpp:136-286)
    resident on the device; matrix() is one call of the reference's ::matrix per object and returns the adapted
    measurement noise [B, 3, 3] -- the R of update()."""

    def __init__(self, batch, m1, m2, gamma, r2count, device=0, stream=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        _check(self._lib.slk_adaptive_create(batch, device, m1, m2, gamma, r2count, stream, C.byref(self._h)), "slk_adaptive_create")
        self.B = batch

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.slk_adaptive_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def matrix(self, xk, Pk, z, H, R):
        B = self.B
        x = np.ascontiguousarray(np.asarray(xk, dtype=np.float64).reshape(B, -1))
        n = x.shape[1]
        P = np.ascontiguousarray(np.transpose(np.asarray(Pk, dtype=np.float64).reshape(B, n, n), (0, 2, 1)))
        zz = np.ascontiguousarray(np.asarray(z, dtype=np.float64).reshape(B, 3))
        Hc = np.ascontiguousarray(np.transpose(np.asarray(H, dtype=np.float64).reshape(B, 3, n), (0, 2, 1)))
        ra = _mat(np.asarray(R), B, 3)
        out = np.empty((B, 3, 3))
        _check(self._lib.slk_adaptive_matrix(self._h, n, x.ctypes.data, P.ctypes.data, zz.ctypes.data, Hc.ctypes.data, ra.ptr,
                                             ra.stride, out.ctypes.data, HOST), "slk_adaptive_matrix")
        return np.ascontiguousarray(np.transpose(out, (0, 2, 1)))
