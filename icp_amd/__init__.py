"""icp_amd — MI355X-native photogeometric ICP iteration engine (host-side Python mirror).

Thin ctypes binding of the C-ABI in include/icp_amd.h (icp_amd/libicp_amd.so, hand-written HIP
for gfx950).  The classes keep the names and argument meaning of the reference's
cl_algo::ICP::ICPStep<CR,CW> / ICP<CR,CW> (include/ICP/algorithms.hpp:2234-2496 of nlamprian/ICP).

There is no CPU fallback: if the shared library is missing, or no gfx950 device is visible,
calls raise.  Nothing in this package imports oracle/.
"""
import ctypes as C
import os

import numpy as np

__all__ = ["ICP", "ICPStep", "ICPError", "Memory", "Quality", "Pairs", "PAIR", "ErrorMetric", "Normals", "ICPStepConfigT", "ICPStepConfigW",
           "PowerMode", "ReduceMode", "TransformKind", "ICPBatch", "batch_partition", "power_method", "KernelObject", "kernel_lms", "kernel_reps", "kernel_weights", "kernel_mean", "kernel_devs", "kernel_s", "ReduceScan", "lib", "lib_path", "reduce", "scan", "ReduceConfig", "synth_pair", "synth_cloud_vga", "punch_holes", "HOLES_SCATTERED", "HOLES_CONTIGUOUS", "synth_pair_scene", "SCENE_CURVED", "SCENE_WALL", "device_count", "DIST_ID", "grid_intrinsics", "landmark_intrinsics"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("ICP_AMD_LIB", os.path.join(_HERE, "libicp_amd.so"))   # override: A/B builds of the same ABI

DIST_ID = np.dtype([("dist", np.float32), ("id", np.uint32)])


class ICPError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("icp_amd error %d: %s" % (code, msg))
        self.code = code


class ICPStepConfigT:            # include/ICP/algorithms.hpp:1544
    EIGEN = 0
    POWER_METHOD = 1


class ICPStepConfigW:            # include/ICP/algorithms.hpp:1560
    REGULAR = 0
    WEIGHTED = 1


REJECT_INVALID = 1                # ICP_REJECT_INVALID (include/icp_amd.h): correspondence rejection of pairs with an invalid endpoint


class ErrorMetric:                # icp_set_error_metric (include/icp_amd.h)
    POINT_TO_POINT = 0
    POINT_TO_PLANE = 1
    COLORED = 2                   # point-to-plane plus kappa times a photometric term (set_color_weight)


class RobustLoss:                # icp_set_robust_loss (include/icp_amd.h): the IRLS weight omega (u) of u = s^2 / k^2
    NONE = 0                      # off (the default)
    HUBER = 1                     # u <= 1 ? 1 : 1 / sqrt (u)
    CAUCHY = 2                    # 1 / (1 + u)
    TUKEY = 3                     # u < 1 ? (1 - u)^2 : 0
    NAMES = {"none": NONE, "huber": HUBER, "cauchy": CAUCHY, "tukey": TUKEY}


class Normals:                    # icp_set_normals: where the fixed frame's point-to-plane normals come from
    GIVEN = 0                     # written by the user (Memory.NORMALS_F)
    GRID = 1                      # computed by buildRBC from F read as a row-major grid


_i32, _u32, _f32 = C.c_int, C.c_uint32, C.c_float

# The per-registration options, by the stem n of their C names (include/icp_amd.h): the argument types behind the handle of icp_set_<n>
# and icp_batch_set_<n> — icp_get_<n> takes pointers to the same, in the same order —, and the values a fresh handle holds (icp_options'
# initialisers, icp_amd/csrc/icp_host.h).  lib() declares the three entry points of every row; _Options holds the setter and the getter.
_OPTIONS = {
    "rejection": ((_i32, _f32), (0, 0.0)),
    "trimming": ((_f32,), (1.0,)),
    "unique": ((_i32,), (0,)),
    "median_rejection": ((_f32,), (0.0,)),
    "adaptive_trimming": ((_f32, _f32, _u32), (0.0, 0.0, 0)),
    "reciprocal": ((_i32, _f32), (0, 0.0)),
    "projective": ((_i32, _u32, _f32, _f32, _f32, _f32, _u32), (0, 0, 0.0, 0.0, 0.0, 0.0, 0)),
    "normal_rejection": ((_i32, _f32), (0, 0.0)),
    "boundary_rejection": ((_u32,), (0,)),
    "robust_loss": ((_i32, _f32), (0, 0.0)),
    "error_metric": ((_i32, _f32), (0, 0.0)),
    "normals": ((_i32, _u32), (0, 0)),
    "color_weight": ((_f32,), (0.0,)),
    "plane_to_plane": ((_f32,), (0.0,)),
    "symmetric": ((_i32,), (0,)),
}


def _max_dist_arg(max_dist):
    """max_dist of set_rejection -> the C argument (None: 0.0, no distance test); the library validates it."""
    return 0.0 if max_dist is None else float(max_dist)


class PowerMode:
    LITERAL = 0
    SQUARED = 1


class ReduceMode:
    REFERENCE_ORDER = 0
    FUSED = 1


class TransformKind:             # ICPTransformConfig (include/ICP/algorithms.hpp:1189) + the second quaternion kernel
    QUATERNION = 0
    QUATERNION_2 = 1
    MATRIX = 2


class Memory:                    # icp_mem in include/icp_amd.h
    F, M, T, TK, MEANS, S, NN_ID, W, SUM_W, REPS, RBC_N, RBC_O, RBC_PERM, RBC_OWNER, RBC_XP, RID, R, RK, NN, QT, TRIM, \
        NORMALS_F, PLANE_SYSTEM, COLOR_GRAD_F, NORMALS_M, UNIQUE, PAIR_FILTER, RECIPROCAL, REVERSE_ID, PROJECTIVE, MEDIAN, TRIM_ADAPTIVE = range(32)
    # reference spellings (ICPStep::Memory, include/ICP/algorithms.hpp:2241-2267)
    D_IN_F, D_IN_M, D_IO_T, H_IO_T = F, M, T, T


class _State(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("q", C.c_float * 4), ("t", C.c_float * 3), ("s", C.c_float),
                ("Rk", C.c_float * 9), ("qk", C.c_float * 4), ("tk", C.c_float * 3), ("sk", C.c_float),
                ("k", C.c_uint32), ("converged", C.c_uint32), ("power_iterations", C.c_uint32),
                ("reserved", C.c_uint32)]


class Quality(C.Structure):
    """icp_quality_t (include/icp_amd.h): fitness, inlier RMSE, the sum of the inliers' squared distances, the 6 x 6 information matrix
    (row-major, rotation first), and the counts (n = m, counted moving points, inliers)."""
    _fields_ = [("fitness", C.c_double), ("inlier_rmse", C.c_double), ("sum_geo", C.c_double), ("information", C.c_double * 36),
                ("n", C.c_uint32), ("n_moving", C.c_uint32), ("n_inliers", C.c_uint32), ("reserved", C.c_uint32)]

    def information_matrix(self):
        return np.array(self.information, np.float64).reshape(6, 6)


class Pairs:                     # icp_correspondences (include/icp_amd.h): which pairs the set holds
    EVALUATED = 0                 # the inliers of icp_evaluate's rule at the same max_dist (the handle's opt-in rules have no influence)
    LAST_ITERATION = 1            # the pairs the solver used in the last executed iteration: ICP_MEM_W != 0


PAIR = np.dtype([("moving", "<u4"), ("fixed", "<u4"), ("geo", "<f4"), ("weight", "<f4")])       # icp_pair_t


class _Pair(C.Structure):
    """icp_pair_t (include/icp_amd.h): one member pair of a correspondence set, 16 bytes."""
    _fields_ = [("moving", C.c_uint32), ("fixed", C.c_uint32), ("geo", C.c_float), ("weight", C.c_float)]


_lib = None


def lib_path():
    return _SO


def lib():
    """Loads icp_amd/libicp_amd.so; raises if it has not been built (`make` or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ICPError(-1, "%s not found: build it with `make` (hipcc --offload-arch=gfx950); "
                           "there is no CPU fallback" % _SO)
    L = C.CDLL(_SO)
    vp, u32, i32, f32, f64 = C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_double

    def sig(name, res, *args):
        f = getattr(L, name, None)
        if f is None:
            if "ICP_AMD_LIB" in os.environ:          # an A/B build of an older ABI (tools/diag/ab.sh): entry points it lacks stay unbound
                return
            raise AttributeError("%s does not export %s" % (_SO, name))
        f.restype = res
        f.argtypes = list(args)

    sig("icp_create", i32, C.POINTER(vp), i32, i32, i32)
    sig("icp_destroy", i32, vp)
    sig("icp_init", i32, vp, u32, u32, f32, f32, u32, f64, f64)
    sig("icp_init_batched", i32, vp, u32, u32, u32, f32, f32, u32, f64, f64)
    sig("icp_write", i32, vp, i32, vp, i32)
    sig("icp_write_b", i32, vp, u32, i32, vp, i32)
    sig("icp_read", i32, vp, i32, vp, C.c_size_t)
    sig("icp_read_b", i32, vp, u32, i32, vp, C.c_size_t)
    sig("icp_mem_size", C.c_size_t, vp, i32)
    sig("icp_device_ptr", i32, vp, i32, C.POINTER(vp))
    sig("icp_adopt_device_buffer", i32, vp, i32, vp)
    sig("icp_build_rbc", i32, vp)
    sig("icp_step", i32, vp, i32)
    sig("icp_run", i32, vp, C.POINTER(u32))
    sig("icp_run_stats", i32, vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32))
    sig("icp_set_run_depth", i32, vp, u32, i32)
    sig("icp_run_timeline", i32, vp, C.POINTER(f64))
    sig("icp_set_output_mode", i32, vp, i32)
    sig("icp_launch_stats", i32, vp, C.POINTER(f64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), i32)
    sig("icp_run_fixed", i32, vp, u32)
    sig("icp_run_fixed_fresh", i32, vp, u32)
    sig("icp_sync", i32, vp)
    sig("icp_get_alpha", i32, vp, C.POINTER(f32))
    sig("icp_set_alpha", i32, vp, f32)
    sig("icp_get_scaling", i32, vp, C.POINTER(f32))
    sig("icp_set_scaling", i32, vp, f32)
    sig("icp_set_metric_scale", i32, vp, f32)
    sig("icp_get_metric_scale", i32, vp, C.POINTER(f32))
    for name, (types, _) in _OPTIONS.items():
        sig("icp_set_" + name, i32, vp, *types)
        sig("icp_get_" + name, i32, vp, *[C.POINTER(t) for t in types])
        sig("icp_batch_set_" + name, i32, vp, *types)
    sig("icp_get_max_iterations", i32, vp, C.POINTER(u32))
    sig("icp_set_max_iterations", i32, vp, u32)
    sig("icp_get_angle_threshold", i32, vp, C.POINTER(f64))
    sig("icp_set_angle_threshold", i32, vp, f64)
    sig("icp_get_translation_threshold", i32, vp, C.POINTER(f64))
    sig("icp_set_translation_threshold", i32, vp, f64)
    sig("icp_set_power_mode", i32, vp, i32)
    sig("icp_set_reduce_mode", i32, vp, i32)
    sig("icp_state", i32, vp, C.POINTER(_State))
    sig("icp_state_b", i32, vp, u32, C.POINTER(_State))
    sig("icp_evaluate", i32, vp, f32, C.POINTER(Quality), u32)
    sig("icp_batch_evaluate", i32, vp, u32, f32, C.POINTER(Quality))
    sig("icp_correspondences", i32, vp, i32, f32, C.POINTER(u32), u32)
    sig("icp_correspondences_read", i32, vp, u32, vp, u32, C.POINTER(u32))
    sig("icp_correspondences_device_ptr", i32, vp, u32, C.POINTER(vp), C.POINTER(vp))
    sig("icp_batch_correspondences", i32, vp, u32, i32, f32, vp, u32, C.POINTER(u32))
    sig("icp_write_cloud", i32, vp, i32, vp, i32)
    sig("icp_transform_cloud", i32, vp, vp, vp, u32)
    sig("icp_transform_cloud_ex", i32, vp, i32, vp, vp, vp, u32)
    sig("icp_track_next", i32, vp, vp, i32, C.POINTER(u32), C.POINTER(i32))
    sig("icp_track_reset", i32, vp)
    sig("icp_track_form", i32, vp, C.POINTER(i32))
    sig("icp_track_submit", i32, vp, vp, i32)
    sig("icp_track_collect", i32, vp, C.POINTER(u32), vp, C.POINTER(i32))
    sig("icp_track_staging", i32, vp, u32, C.POINTER(vp))
    sig("icp_batch_create", i32, C.POINTER(vp), C.POINTER(i32), i32, i32, i32)
    sig("icp_batch_destroy", i32, vp)
    sig("icp_batch_init", i32, vp, u32, u32, u32, f32, f32, u32, f64, f64)
    sig("icp_batch_set_modes", i32, vp, i32, i32)
    sig("icp_batch_write", i32, vp, u32, i32, vp)
    sig("icp_batch_build_rbc", i32, vp)
    sig("icp_batch_run", i32, vp)
    sig("icp_batch_run_fixed", i32, vp, u32, i32)
    sig("icp_batch_state", i32, vp, u32, C.POINTER(_State))
    sig("icp_batch_read", i32, vp, u32, i32, vp, C.c_size_t)
    sig("icp_batch_size", i32, vp, C.POINTER(u32), C.POINTER(u32))
    sig("icp_batch_time_run_fixed", i32, vp, u32, u32, C.POINTER(f64))
    sig("icp_batch_time_run_fixed_slots", i32, vp, u32, u32, u32, C.POINTER(f64), vp)
    sig("icp_batch_partition", i32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32))
    sig("icp_batch_last_error", C.c_char_p, vp)
    sig("icp_pyramid_create", i32, C.POINTER(vp), i32, i32, i32)
    sig("icp_pyramid_destroy", i32, vp)
    sig("icp_pyramid_init", i32, vp, u32, u32, C.POINTER(u32), f32, f32, C.POINTER(u32), f64, f64)
    sig("icp_pyramid_set_reduction", i32, vp, i32, f32)
    sig("icp_pyramid_get_reduction", i32, vp, C.POINTER(i32), C.POINTER(f32))
    sig("icp_pyramid_levels", i32, vp, C.POINTER(u32))
    sig("icp_pyramid_level", i32, vp, u32, C.POINTER(vp))
    sig("icp_pyramid_write", i32, vp, i32, vp, i32)
    sig("icp_pyramid_write_cloud", i32, vp, i32, vp, i32)
    sig("icp_pyramid_reset_transform", i32, vp)
    sig("icp_pyramid_build_rbc", i32, vp)
    sig("icp_pyramid_run", i32, vp, C.POINTER(u32))
    sig("icp_pyramid_run_fixed", i32, vp, C.POINTER(u32))
    sig("icp_pyramid_sync", i32, vp)
    sig("icp_pyramid_pending", i32, vp, C.POINTER(i32))
    sig("icp_pyramid_time_build", i32, vp, i32, u32, C.POINTER(f32))
    sig("icp_pyramid_last_error", C.c_char_p, vp)
    sig("icp_time_run_fixed", i32, vp, u32, u32, i32, C.POINTER(f32))
    sig("icp_time_run_fixed_tail", i32, vp, u32, u32, i32, C.POINTER(f32), C.POINTER(u32))
    sig("icp_reset_transform", i32, vp)
    sig("icp_time_kernels", i32, vp, u32, C.POINTER(f32))
    sig("icp_profile_run", i32, vp, u32, vp, C.POINTER(f32))
    sig("icp_time_masked", i32, vp, u32, u32, u32, C.POINTER(f32))
    sig("icp_launches_per_iteration", i32, vp, C.POINTER(u32))
    sig("icp_run_form", i32, vp, C.POINTER(i32))
    sig("icp_search_layout", i32, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32))
    sig("icp_power_method", i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(u32))
    sig("icp_kernel_lms", i32, i32, vp, vp)
    sig("icp_kernel_reps", i32, i32, vp, u32, u32, vp)
    sig("icp_kernel_weights", i32, i32, vp, u32, vp, C.POINTER(f64))
    sig("icp_kernel_mean", i32, i32, i32, vp, vp, vp, f64, u32, vp)
    sig("icp_kernel_devs", i32, i32, vp, vp, vp, u32, vp, vp)
    sig("icp_kernel_s", i32, i32, i32, vp, vp, vp, u32, f32, vp)
    sig("icp_kernel_last_error", C.c_char_p)
    sig("icp_ko_create", i32, C.POINTER(vp), i32, i32, u32, u32, f32)
    sig("icp_ko_destroy", i32, vp)
    sig("icp_ko_adopt", i32, vp, i32, vp)
    sig("icp_ko_device_ptr", i32, vp, i32, C.POINTER(vp))
    sig("icp_ko_slot_bytes", C.c_size_t, vp, i32)
    sig("icp_ko_write", i32, vp, i32, vp)
    sig("icp_ko_read", i32, vp, i32, vp)
    sig("icp_ko_run", i32, vp)
    sig("icp_ko_set_scaling", i32, vp, f32)
    sig("icp_reduce", i32, i32, i32, vp, u32, u32, vp)
    sig("icp_scan", i32, i32, i32, vp, u32, u32, vp)
    sig("icp_reduce_scan_last_error", C.c_char_p)
    sig("icp_rs_create", i32, C.POINTER(vp), i32, i32, u32, u32)
    sig("icp_rs_write", i32, vp, vp)
    sig("icp_rs_run", i32, vp)
    sig("icp_rs_read", i32, vp, vp)
    sig("icp_rs_device_ptr", i32, vp, i32, C.POINTER(vp))
    sig("icp_rs_time", i32, vp, u32, C.POINTER(f32))
    sig("icp_rs_destroy", i32, vp)
    sig("icp_last_error", C.c_char_p, vp)
    sig("icp_version", C.c_char_p)
    sig("icp_device_count", i32, C.POINTER(i32))
    sig("icp_device_pci_bus_id", i32, i32, C.c_char_p, C.c_size_t)
    sig("icp_numa_cpulist", i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig("icp_batch_slot_cpus", i32, vp, u32, C.c_char_p, C.c_size_t)
    sig("icp_synth_pair", i32, C.c_uint64, u32, f32, vp, vp, f32, f32, f32, vp, vp)
    sig("icp_synth_cloud_vga", i32, C.c_uint64, i32, vp)
    sig("icp_track_register_source", i32, vp, vp, C.c_size_t)
    sig("icp_track_unregister_source", i32, vp, vp)
    sig("icp_synth_pair_scene", i32, C.c_uint64, u32, i32, f32, vp, vp, f32, f32, vp, vp, vp)
    sig("icp_synth_punch_holes", i32, C.c_uint64, u32, u32, i32, f32, i32, vp)
    _lib = L
    return L


class ReduceConfig:              # include/ICP/algorithms.hpp:52-57
    MIN, MAX, SUM = 0, 1, 2


def reduce(a, config=ReduceConfig.SUM, device=0):
    """Row-wise reduce of a rows x cols array — cl_algo::ICP::Reduce<C,T> (MIN: float, MAX: uint32, SUM: float)."""
    dt = np.uint32 if config == ReduceConfig.MAX else np.float32
    a = np.ascontiguousarray(a, dt)
    if a.ndim != 2:
        raise ValueError("expected a rows x cols array")
    out = np.empty(a.shape[0], dt)
    rc = lib().icp_reduce(device, config, _p(a), a.shape[1], a.shape[0], _p(out))
    if rc:
        raise ICPError(rc, lib().icp_reduce_scan_last_error().decode())
    return out


def scan(a, inclusive=True, device=0):
    """Row-wise integer scan of a rows x cols array — cl_algo::ICP::Scan<INCLUSIVE|EXCLUSIVE,int>."""
    a = np.ascontiguousarray(a, np.int32)
    if a.ndim != 2:
        raise ValueError("expected a rows x cols array")
    out = np.empty_like(a)
    rc = lib().icp_scan(device, int(inclusive), _p(a), a.shape[1], a.shape[0], _p(out))
    if rc:
        raise ICPError(rc, lib().icp_reduce_scan_last_error().decode())
    return out


class ReduceScan:
    """Resident Reduce / Scan object (icp_rs_*): kind = ReduceConfig.MIN / MAX / SUM, or "inclusive" / "exclusive" scan.
    Device buffers live with the object; run() enqueues kernels only; time(reps) = mean microseconds per run."""

    def __init__(self, kind, cols, rows, device=0):
        self._L = lib()
        self._kind = {"inclusive": 3, "exclusive": 4}.get(kind, kind)
        self._dt = np.int32 if self._kind >= 3 else (np.uint32 if self._kind == ReduceConfig.MAX else np.float32)
        self.cols, self.rows = cols, rows
        self._r = C.c_void_p()
        rc = self._L.icp_rs_create(C.byref(self._r), device, self._kind, cols, rows)
        if rc:
            self._r = None
            raise ICPError(rc, self._L.icp_reduce_scan_last_error().decode())

    def _chk(self, rc):
        if rc:
            raise ICPError(rc, self._L.icp_reduce_scan_last_error().decode())

    def write(self, a):
        a = np.ascontiguousarray(a, self._dt)
        if a.shape != (self.rows, self.cols):
            raise ValueError("expected a %d x %d array" % (self.rows, self.cols))
        self._chk(self._L.icp_rs_write(self._r, _p(a)))

    def run(self):
        self._chk(self._L.icp_rs_run(self._r))

    def read(self):
        out = np.empty((self.rows, self.cols) if self._kind >= 3 else self.rows, self._dt)
        self._chk(self._L.icp_rs_read(self._r, _p(out)))
        return out

    def device_ptr(self, output=True):
        """Device address of the input buffer (output=False) or of the output buffer every run writes (output=True):
        the facade's get(D_IN / D_OUT), fixed for the object's lifetime."""
        p = C.c_void_p()
        self._chk(self._L.icp_rs_device_ptr(self._r, int(bool(output)), C.byref(p)))
        return p.value

    def time(self, reps=100):
        us = C.c_float()
        self._chk(self._L.icp_rs_time(self._r, reps, C.byref(us)))
        return us.value

    def close(self):
        if getattr(self, "_r", None):
            self._L.icp_rs_destroy(self._r)
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def power_method(S, means, rot=ICPStepConfigT.POWER_METHOD, mode=PowerMode.LITERAL, device=0):
    """ICPPowerMethod (include/ICP/algorithms.hpp:1451-1537): S[11], means[8] -> (Tk[8], Rk[3,3], loop trips) by one wave of the
    engine's rotation solver on the device (rot = EIGEN: the SVD branch)."""
    S = np.ascontiguousarray(S, np.float32).reshape(-1)
    means = np.ascontiguousarray(means, np.float32).reshape(-1)
    if S.size != 11 or means.size != 8:
        raise ValueError("expected S[11] and means[8]")
    Tk, Rk, it = np.empty(8, np.float32), np.empty(9, np.float32), C.c_uint32()
    rc = lib().icp_power_method(device, rot, mode, _p(S), _p(means), _p(Tk), _p(Rk), C.byref(it))
    if rc:
        raise ICPError(rc, lib().icp_last_error(None).decode())
    return Tk, Rk.reshape(3, 3), it.value


def _kchk(rc):
    if rc:
        raise ICPError(rc, lib().icp_kernel_last_error().decode())


def kernel_lms(cloud, device=0):
    """ICPLMs: 640 x 480 float8 cloud -> the 128 x 128 landmarks (getLMs)."""
    cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 8)
    if cloud.shape[0] != 640 * 480:
        raise ValueError("expected a 640x480 float8 cloud")
    out = np.empty((16384, 8), np.float32)
    _kchk(lib().icp_kernel_lms(device, _p(cloud), _p(out)))
    return out


def kernel_reps(F, nr, device=0):
    """ICPReps: nr representatives of a square landmark set (getReps with the grid side sqrt(m))."""
    F = np.ascontiguousarray(F, np.float32).reshape(-1, 8)
    out = np.empty((nr, 8), np.float32)
    _kchk(lib().icp_kernel_reps(device, _p(F), F.shape[0], nr, _p(out)))
    return out


def kernel_weights(nn_id, device=0):
    """ICPWeights: {dist, id}[n] -> (W[n], sum of weights)."""
    nn_id = np.ascontiguousarray(nn_id, DIST_ID)
    W, sw = np.empty(nn_id.shape[0], np.float32), C.c_double()
    _kchk(lib().icp_kernel_weights(device, _p(nn_id), nn_id.shape[0], _p(W), C.byref(sw)))
    return W, sw.value


def kernel_mean(F, M, W=None, sum_w=1.0, device=0):
    """ICPMean<REGULAR> (W is None) / ICPMean<WEIGHTED>: [mean_F, 0 | mean_M, 0]."""
    F = np.ascontiguousarray(F, np.float32).reshape(-1, 8)
    M = np.ascontiguousarray(M, np.float32).reshape(-1, 8)
    Wp = None if W is None else np.ascontiguousarray(W, np.float32)
    out = np.empty(8, np.float32)
    _kchk(lib().icp_kernel_mean(device, int(W is not None), _p(F), _p(M), None if Wp is None else _p(Wp), float(sum_w), F.shape[0], _p(out)))
    return out


def kernel_devs(F, M, mean8, device=0):
    """ICPDevs: (DF[n, 4], DM[n, 4])."""
    F = np.ascontiguousarray(F, np.float32).reshape(-1, 8)
    M = np.ascontiguousarray(M, np.float32).reshape(-1, 8)
    mean8 = np.ascontiguousarray(mean8, np.float32)
    DF, DM = np.empty((F.shape[0], 4), np.float32), np.empty((F.shape[0], 4), np.float32)
    _kchk(lib().icp_kernel_devs(device, _p(F), _p(M), _p(mean8), F.shape[0], _p(DF), _p(DM)))
    return DF, DM


def kernel_s(DM, DF, W=None, c=1e-6, device=0):
    """ICPS<REGULAR> (W is None) / ICPS<WEIGHTED>: S[11]."""
    DM = np.ascontiguousarray(DM, np.float32).reshape(-1, 4)
    DF = np.ascontiguousarray(DF, np.float32).reshape(-1, 4)
    Wp = None if W is None else np.ascontiguousarray(W, np.float32)
    out = np.empty(11, np.float32)
    _kchk(lib().icp_kernel_s(device, int(W is not None), _p(DM), _p(DF), None if Wp is None else _p(Wp), DM.shape[0], c, _p(out)))
    return out


class KernelObject:
    """Resident per-kernel object (icp_ko_*): the reference's ICPLMs / ICPReps / ICPWeights / ICPMean<> / ICPDevs / ICPS<> with device
    buffers that live with the object.  kind: "lms", "reps", "weights", "mean", "mean_weighted", "devs", "s", "s_weighted"; slots (Memory
    objects) as listed in include/icp_amd.h.  get(slot) = the device pointer; adopt(slot, ptr) before the slot's first use wires another
    object's buffer in (no copy); run() enqueues kernels only."""
    KINDS = {"lms": 0, "reps": 1, "weights": 2, "mean": 3, "mean_weighted": 4, "devs": 5, "s": 6, "s_weighted": 7}

    def __init__(self, kind, n=0, aux=0, c=1e-6, device=0):
        self._L = lib()
        self._k = C.c_void_p()
        _kchk(self._L.icp_ko_create(C.byref(self._k), device, self.KINDS[kind], n, aux, c))

    def close(self):
        if getattr(self, "_k", None):
            self._L.icp_ko_destroy(self._k)
            self._k = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get(self, slot):
        p = C.c_void_p()
        _kchk(self._L.icp_ko_device_ptr(self._k, slot, C.byref(p)))
        return p.value

    def adopt(self, slot, device_ptr):
        _kchk(self._L.icp_ko_adopt(self._k, slot, C.c_void_p(device_ptr)))

    def write(self, slot, a):
        a = np.ascontiguousarray(a)
        if a.nbytes != self._L.icp_ko_slot_bytes(self._k, slot):
            raise ValueError("slot %d holds %d bytes, got %d" % (slot, self._L.icp_ko_slot_bytes(self._k, slot), a.nbytes))
        _kchk(self._L.icp_ko_write(self._k, slot, _p(a)))

    def read(self, slot, dtype=np.float32):
        out = np.empty(self._L.icp_ko_slot_bytes(self._k, slot) // np.dtype(dtype).itemsize, dtype)
        _kchk(self._L.icp_ko_read(self._k, slot, _p(out)))
        return out

    def run(self):
        _kchk(self._L.icp_ko_run(self._k))

    def set_scaling(self, c):
        """ICPS::setScaling: the factor c of the next run()."""
        _kchk(self._L.icp_ko_set_scaling(self._k, c))


def device_count():
    n = C.c_int(0)
    lib().icp_device_count(C.byref(n))
    return n.value


def device_pci_bus_id(device):
    """PCI bus id of a device ("0000:c1:00.0")."""
    buf = C.create_string_buffer(64)
    rc = lib().icp_device_pci_bus_id(device, buf, len(buf))
    if rc:
        raise ICPError(rc, "icp_device_pci_bus_id (%d)" % device)
    return buf.value.decode()


def numa_cpulist(pci_bus_id, sysfs_root=None):
    """cpulist of the NUMA node a PCI device hangs on, from a sysfs tree ("" when the tree has no answer): where icp_batch_create pins
    the host thread of a device slot by default (host code only: works without a GPU)."""
    buf = C.create_string_buffer(4096)
    rc = lib().icp_numa_cpulist(sysfs_root.encode() if sysfs_root else None, pci_bus_id.encode(), buf, len(buf))
    if rc:
        raise ICPError(rc, "icp_numa_cpulist")
    return buf.value.decode()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def synth_pair(side, seed=0x1C9D5EED, rot_deg=3.0, axis=(0.3, 0.9, 0.1), t=(25.0, -10.0, 15.0),
               noise_mm=1.0, noise_rgb=0.01, zero_fraction=0.0):
    """Synthetic fixed/moving landmark pair (side*side points each), SURVEY.md §8d. Host only."""
    F = np.empty((side * side, 8), np.float32)
    M = np.empty((side * side, 8), np.float32)
    ax = np.asarray(axis, np.float32)
    tt = np.asarray(t, np.float32)
    rc = lib().icp_synth_pair(seed, side, rot_deg, _p(ax), _p(tt), noise_mm, noise_rgb, zero_fraction, _p(F), _p(M))
    if rc:
        raise ICPError(rc, "icp_synth_pair")
    return F, M


def synth_cloud_vga(seed=0x1C9D5EED, moved=False):
    """Synthetic 640x480 float8 cloud; `moved` = frame number of a sequence (False / 0: the scene, True / 1: one step)."""
    cloud = np.empty((480 * 640, 8), np.float32)
    rc = lib().icp_synth_cloud_vga(seed, int(moved), _p(cloud))
    if rc:
        raise ICPError(rc, "icp_synth_cloud_vga")
    return cloud


HOLES_SCATTERED, HOLES_CONTIGUOUS = 0, 1
SCENE_CURVED, SCENE_WALL = 0, 1


def synth_pair_scene(side, scene=SCENE_CURVED, seed=0x1C9D5EED, rot_deg=3.0, axis=(0.3, 0.9, 0.1), t=(25.0, -10.0, 15.0),
                     noise_mm=1.0, noise_rgb=0.01):
    """(F, M, T_true): a synthetic pair of the chosen scene and the ground truth [q | t, 1] that maps M onto F.  SCENE_WALL: the
    reference's kg_pc8d_wall stand-in (data/README.md:11-16) — a textured plane moved in its own plane. Host only."""
    F = np.empty((side * side, 8), np.float32)
    M = np.empty((side * side, 8), np.float32)
    T = np.empty(8, np.float32)
    ax = np.asarray(axis, np.float32)
    tt = np.asarray(t, np.float32)
    rc = lib().icp_synth_pair_scene(seed, side, scene, rot_deg, _p(ax), _p(tt), noise_mm, noise_rgb, _p(F), _p(M), _p(T))
    if rc:
        raise ICPError(rc, "icp_synth_pair_scene")
    return F, M, T


def punch_holes(cloud, width, height, pattern=HOLES_SCATTERED, fraction=0.1, keep_rgb=True, seed=0x1C9D5EED):
    """A copy of `cloud` (width x height float8 points) with a Kinect frame's invalid pixels: xyz = 0, the colour kept
    (reference src/kinect_frame_grabber.cpp:246-262) unless keep_rgb is False (all holes identical). Host only."""
    out = np.ascontiguousarray(cloud, np.float32).copy()
    assert out.size == width * height * 8
    rc = lib().icp_synth_punch_holes(seed, width, height, pattern, fraction, int(bool(keep_rgb)), _p(out))
    if rc:
        raise ICPError(rc, "icp_synth_punch_holes")
    return out


# The memory objects (icp_mem, include/icp_amd.h): the dtype and the columns of the array a read returns (None: flat), and the object's
# elements of that dtype per registration, fixed + per_point * m.  (None, None): only a handle sizes it (icp_mem_size): ICPBatch.read does
# not serve it.
_MEM = {                          # mem: (dtype, columns, fixed, per_point)
    Memory.F: (np.float32, 8, 0, 8), Memory.M: (np.float32, 8, 0, 8), Memory.RBC_XP: (np.float32, 8, None, None),
    Memory.T: (np.float32, None, 8, 0), Memory.TK: (np.float32, None, 8, 0), Memory.MEANS: (np.float32, None, 8, 0),
    Memory.S: (np.float32, None, 11, 0), Memory.NN_ID: (DIST_ID, None, 0, 1), Memory.W: (np.float32, None, 0, 1),
    Memory.SUM_W: (np.float64, None, None, None), Memory.REPS: (np.float32, 8, None, None), Memory.RBC_N: (np.uint32, None, None, None),
    Memory.RBC_O: (np.uint32, None, None, None), Memory.RBC_PERM: (np.uint32, None, None, None), Memory.RBC_OWNER: (np.uint32, None, None, None),
    Memory.RID: (np.uint32, None, 0, 1), Memory.R: (np.float32, 3, 9, 0), Memory.RK: (np.float32, 3, 9, 0),
    Memory.NN: (np.float32, 4, 0, 4), Memory.QT: (np.float32, 4, 0, 4), Memory.TRIM: (np.uint32, None, 4, 0),
    Memory.NORMALS_F: (np.float32, 4, 0, 4), Memory.PLANE_SYSTEM: (np.float64, None, 28, 0), Memory.COLOR_GRAD_F: (np.float32, 4, 0, 4),
    Memory.NORMALS_M: (np.float32, 4, 0, 4), Memory.UNIQUE: (np.uint32, None, 2, 0), Memory.PAIR_FILTER: (np.uint32, None, 4, 0),
    Memory.RECIPROCAL: (np.uint32, None, 4, 0), Memory.REVERSE_ID: (DIST_ID, None, 0, 1), Memory.PROJECTIVE: (np.uint32, None, 4, 0),
    Memory.MEDIAN: (np.uint32, None, 4, 0),
    Memory.TRIM_ADAPTIVE: (np.uint32, None, 4, 0),
}
_MEM_DTYPE = {mem: row[:2] for mem, row in _MEM.items()}           # (dtype, columns) alone
_MEM_WRITTEN = (Memory.T, Memory.F, Memory.M, Memory.NORMALS_F, Memory.COLOR_GRAD_F, Memory.NORMALS_M)      # what icp_write takes


def _mem_elements(mem, m):
    """Elements of its dtype that `mem` holds per registration of m points; KeyError for an object the table does not size."""
    fixed, per_point = _MEM[mem][2:]
    if fixed is None:
        raise KeyError(mem)
    return fixed + per_point * m


def _write_floats(mem, m):
    """Floats a write of `mem` takes: T 8, NORMALS_F / COLOR_GRAD_F / NORMALS_M m x 4, F / M m x 8 (and m x 8 for an object the library
    takes no writes of: it says so itself)."""
    return _mem_elements(mem, m) if mem in _MEM_WRITTEN else m * 8


def grid_intrinsics(side):
    """(fx, fy, cx, cy) in grid units of the side x side landmark grids synth_pair / synth_pair_scene sample from their 640 x 480 pinhole
    image (ICPStep.set_projective): 595 side / 640, 595 side / 480, 319.5 side / 640, 239.5 side / 480."""
    return 595.0 * side / 640.0, 595.0 * side / 480.0, 319.5 * side / 640.0, 239.5 * side / 480.0


def landmark_intrinsics():
    """(fx, fy, cx, cy) in grid units of the 128 x 128 landmarks write_cloud samples from a 640 x 480 frame (column 65 + 4 i, row 49 + 3 j):
    595 / 4, 595 / 3, (319.5 - 65) / 4, (239.5 - 49) / 3 (ICPStep.set_projective)."""
    return 595.0 / 4.0, 595.0 / 3.0, (319.5 - 65.0) / 4.0, (239.5 - 49.0) / 3.0


def _projective_args(grid_width, fx, fy, cx, cy, radius):
    """The arguments of icp_set_projective / icp_batch_set_projective behind the handle (grid_width None or 0: off)."""
    if not grid_width:
        return 0, 0, 1.0, 1.0, 0.0, 0.0, 0
    return 1, int(grid_width), float(fx), float(fy), float(cx), float(cy), int(radius)


class _Options:
    """The per-registration options of _OPTIONS, once for every class that holds them: a setter turns its arguments into the C arguments
    and hands them to _set (name, *cargs), a getter decodes the C values _get (name) returns.  ICPStep sets and asks the library's handle;
    ICPBatch sets every registration and answers with what was last set on the batch."""

    def set_rejection(self, invalid=False, max_dist=None):
        """Correspondence rejection (icp_set_rejection; not reference behaviour, off by default): pairs with an invalid endpoint (a
        point at the origin) and / or pairs farther apart than `max_dist` (geometric, the cloud's units; None: no distance test) get
        the weight 0.  The search itself is unchanged."""
        self._set("rejection", REJECT_INVALID if invalid else 0, _max_dist_arg(max_dist))

    def rejection(self):
        """(invalid, max_dist) as set: max_dist None when there is no distance test."""
        fl, md = self._get("rejection")
        return bool(fl & REJECT_INVALID), (None if md == 0.0 or md == float("inf") else md)

    def set_trimming(self, keep=1.0):
        """Trimmed ICP (icp_set_trimming; not reference behaviour, off by default): every iteration keeps the closest fraction
        `keep` in (0, 1] of the pairs rejection leaves and gives the rest the weight 0; 1.0 switches it off.  read(Memory.TRIM) gives
        the last iteration's (t bits, n, K, accepted).  Kinect data needs set_rejection(invalid=True) alongside it."""
        self._set("trimming", float(keep))

    def trimming(self):
        """The keep fraction as set (1.0: off)."""
        return self._get("trimming")[0]

    def set_unique(self, on=True):
        """One-to-one correspondences (icp_set_unique; not reference behaviour, off by default): of the pairs that share a fixed
        point only the closest keeps its weight (ties: the lowest query index), the others get the weight 0.  It acts after
        rejection and before trimming and the robust loss.  read(Memory.UNIQUE) gives the last iteration's (candidates, winners)."""
        self._set("unique", int(on))

    def unique(self):
        """Whether one-to-one correspondences are on."""
        return bool(self._get("unique")[0])

    def set_median_rejection(self, factor):
        """Median-distance rejection (icp_set_median_rejection; not reference behaviour, 0 = off, the default): every iteration rejects
        the pairs farther apart than factor times the median pair distance of that iteration (geo > factor^2 * the lower median of
        geo).  It acts behind one-to-one and in front of trimming and the robust loss.  read(Memory.MEDIAN) gives the last
        iteration's (t_med bits, n, thr bits, accepted)."""
        self._set("median_rejection", float(factor))

    def median_rejection(self):
        """The factor of median-distance rejection (0: off)."""
        return self._get("median_rejection")[0]

    def set_adaptive_trimming(self, min_fraction=0.05, max_fraction=0.95, power=4):
        """Adaptive trimming (icp_set_adaptive_trimming; not reference behaviour, power 0 = off, the default): trimming whose kept
        fraction every iteration chooses itself, between min_fraction and max_fraction, by minimising (sum of the closest geo) /
        (their number)^power over a table of thresholds — the fractional RMSD of Fractional ICP with lambda = (power - 1) / 2.
        power is 2 .. 8.  It excludes set_trimming(keep < 1) and stands in its place, behind median-distance rejection and in front of
        the robust loss.  read(Memory.TRIM) gives the last iteration's (t bits, n, K, accepted) — K / n is the kept fraction —,
        read(Memory.TRIM_ADAPTIVE) its (winning bin, r_lo, r_hi, candidate bins)."""
        self._set("adaptive_trimming", float(min_fraction), float(max_fraction), int(power))

    def adaptive_trimming(self):
        """(min_fraction, max_fraction, power) of adaptive trimming ((0, 0, 0): off)."""
        return self._get("adaptive_trimming")

    def set_reciprocal(self, on=True, max_gap=0.0):
        """Reciprocal correspondences (icp_set_reciprocal; not reference behaviour, off by default): a pair (m_i, f_j) keeps its weight
        only if the moving point f_j finds when it searches the moving frame — a second RBC, over M, which the engine keeps up to date
        by itself — is m_i, or lies within `max_gap` (the cloud's units) of it; every other pair gets the weight 0.  It acts after the
        boundary and normal rules and before one-to-one correspondences, trimming and the robust loss.  read(Memory.RECIPROCAL) gives
        the last iteration's (n, exact, near, accepted), read(Memory.REVERSE_ID) the back search's (dist, id) per fixed point."""
        self._set("reciprocal", int(on), float(max_gap) if on else 0.0)

    def reciprocal(self):
        """max_gap of reciprocal correspondences, None while the rule is off."""
        on, gap = self._get("reciprocal")
        return gap if on else None

    def set_normal_rejection(self, min_cos=None):
        """Rejection by normal compatibility (icp_set_normal_rejection; not reference behaviour, off by default): a pair whose
        fixed normal and rotated moving normal enclose an angle with a cosine below `min_cos` (in [-1, 1]) gets the weight 0; a pair
        without both normals too.  None: off.  It needs NORMALS_F and NORMALS_M (set_normals), under every metric, and acts before
        one-to-one correspondences, trimming and the robust loss.  read(Memory.PAIR_FILTER) gives the last iteration's
        (n, at_boundary, incompatible, accepted)."""
        on = min_cos is not None
        self._set("normal_rejection", int(on), float(min_cos) if on else 0.0)

    def normal_rejection(self):
        """The cosine threshold of normal rejection, None while it is off."""
        on, min_cos = self._get("normal_rejection")
        return min_cos if on else None

    def set_projective(self, grid_width=None, fx=1.0, fy=1.0, cx=0.0, cy=0.0, radius=0):
        """Projective data association (icp_set_projective; not reference behaviour, off by default): instead of searching the RBC, every
        moving point is transformed, projected through the pinhole model (fx, fy, cx, cy in grid units: grid_intrinsics,
        landmark_intrinsics) onto F read as a row-major grid `grid_width` wide, and paired with the closest valid fixed point of the
        (2 radius + 1)^2 window around its cell; a point that lands outside the grid or on an empty window is a rejected pair.
        radius in [0, 8]; point-to-point needs radius >= 1.  grid_width None or 0: off.  read(Memory.PROJECTIVE) gives the last
        iteration's (n, hits, outside, empty)."""
        self._set("projective", *_projective_args(grid_width, fx, fy, cx, cy, radius))

    def projective(self):
        """(grid_width, fx, fy, cx, cy, radius) of projective data association, None while it is off."""
        on, *values = self._get("projective")
        return tuple(values) if on else None

    def set_boundary_rejection(self, grid_width=None):
        """Rejection at the fixed grid's boundary (icp_set_boundary_rejection; not reference behaviour, off by default): F is read as
        a row-major grid `grid_width` wide, and a pair whose fixed point lies on the grid's rim, is invalid or has an invalid grid
        neighbour gets the weight 0.  None or 0: off."""
        self._set("boundary_rejection", int(grid_width or 0))

    def boundary_rejection(self):
        """The grid width of boundary rejection, None while it is off."""
        return self._get("boundary_rejection")[0] or None

    def set_robust_loss(self, loss=RobustLoss.NONE, scale=0.0):
        """Robust loss (icp_set_robust_loss; not reference behaviour, off by default): every pair's weight is multiplied by the
        loss's IRLS weight omega (s^2 / scale^2) of its own residual s, for every error metric.  `scale` k (finite, > 0, the cloud's
        units) is ignored with RobustLoss.NONE.  Point-to-point: read(Memory.W) gives the weights after it."""
        self._set("robust_loss", int(loss), float(scale))

    def robust_loss(self):
        """(loss, scale) as set ((0, 0.0): off)."""
        return self._get("robust_loss")

    def set_error_metric(self, metric=ErrorMetric.POINT_TO_POINT, point_weight=0.0):
        """Point-to-plane ICP (icp_set_error_metric; not reference behaviour, off by default): each iteration minimises the
        point-to-plane error plus `point_weight` (mu >= 0) times the point-to-point error, linearised, solved by LDL^T on the device.
        The normals of the fixed frame come from set_normals.  read(Memory.PLANE_SYSTEM) gives the last system and its status."""
        self._set("error_metric", int(metric), float(point_weight))

    def error_metric(self):
        """(metric, point_weight) as set."""
        return self._get("error_metric")

    def set_normals(self, source=Normals.GIVEN, grid_width=0):
        """Where the fixed frame's normals come from: Normals.GIVEN (write(Memory.NORMALS_F, m x 4 floats)) or Normals.GRID (buildRBC
        computes them from F read as a row-major grid `grid_width` wide; m must be a multiple of it)."""
        self._set("normals", int(source), int(grid_width))

    def normals(self):
        """(source, grid_width) as set."""
        return self._get("normals")

    def set_color_weight(self, kappa):
        """Colored ICP's photometric weight kappa (icp_set_color_weight; finite, >= 0, default 0, mm^2 per intensity^2): used with
        set_error_metric(ErrorMetric.COLORED, mu).  The fixed frame's intensity gradients are Memory.COLOR_GRAD_F (m x 4 floats
        [gx gy gz C]): computed by buildRBC with Normals.GRID, written by the user with Normals.GIVEN."""
        self._set("color_weight", float(kappa))

    def color_weight(self):
        """kappa as set."""
        return self._get("color_weight")[0]

    def set_plane_to_plane(self, epsilon):
        """Generalized ICP (icp_set_plane_to_plane; not reference behaviour): with ErrorMetric.POINT_TO_PLANE every pair's residual is
        weighed by (C_Q + C_P)^-1, the covariances R diag(epsilon, 1, 1) R^T of the two frames' normals.  epsilon in (0, 1]; 0 (the
        default) is off.  The moving frame's normals are Memory.NORMALS_M (m x 4 floats): computed from M with Normals.GRID (by
        buildRBC and every later write of M), written by the user with Normals.GIVEN."""
        self._set("plane_to_plane", float(epsilon))

    def plane_to_plane(self):
        """epsilon as set (0: off)."""
        return self._get("plane_to_plane")[0]

    def set_symmetric(self, on=True):
        """Symmetric ICP (icp_set_symmetric; Rusinkiewicz 2019; not reference behaviour): with ErrorMetric.POINT_TO_PLANE every pair's
        residual is taken along the mean of the two frames' normals and the rotation is split evenly between the frames.  The moving
        frame's normals are Memory.NORMALS_M, as for set_plane_to_plane (with which, as with ErrorMetric.COLORED, it does not
        combine): computed from M with Normals.GRID (by buildRBC and every later write of M), written by the user with Normals.GIVEN."""
        self._set("symmetric", int(bool(on)))

    def symmetric(self):
        """Whether the symmetric objective is switched on."""
        return bool(self._get("symmetric")[0])


class ICPStep(_Options):
    """One ICP iteration engine — mirror of cl_algo::ICP::ICPStep<CR,CW>.

    Reference                                   here
    ICPStep(env, infoRBC, infoICP)              ICPStep(device=0, CR=POWER_METHOD, CW=WEIGHTED)
    init(m, nr, a=1e2, c=1e-6, staging)         init(m, nr, a=1e2, c=1e-6, batch=1)
    write(mem, ptr, block)                      write(mem, array, block=False, batch_index=0)
    read(mem, block)                            read(mem, batch_index=0) -> numpy array
    buildRBC() / run(config=False)              buildRBC() / run(config=False)
    getAlpha/setAlpha/getScaling/setScaling     same names
    members Rk qk tk sk R q t s                 properties of the same names (blocking read)
    """

    def __init__(self, device=0, CR=ICPStepConfigT.POWER_METHOD, CW=ICPStepConfigW.WEIGHTED):
        self._L = lib()
        self._h = C.c_void_p()
        rc = self._L.icp_create(C.byref(self._h), device, CR, CW)
        if rc:
            msg = self._L.icp_last_error(None).decode()
            self._h = None
            raise ICPError(rc, msg)
        self.m = self.nr = 0
        self.batch = 1
        self._max_it, self._ang, self._tra = 40, 0.001, 0.01

    def close(self):
        if getattr(self, "_h", None):
            self._L.icp_destroy(self._h)           # (unregisters what track_register page-locked)
            self._h = None
            self.__dict__.pop("_registered", None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise ICPError(rc, self._L.icp_last_error(self._h).decode())

    def _out(self, fn, *args):
        """fn (handle, *args) with every ctypes type among `args` replaced by a pointer to a fresh object of it: the tuple of what the
        library wrote into them."""
        out = [a() if isinstance(a, type) else a for a in args]
        self._chk(fn(self._h, *[C.byref(o) if isinstance(a, type) else o for a, o in zip(args, out)]))
        return tuple(o.value for a, o in zip(args, out) if isinstance(a, type))

    def _set(self, name, *cargs):
        self._chk(getattr(self._L, "icp_set_" + name)(self._h, *cargs))

    def _get(self, name):
        return self._out(getattr(self._L, "icp_get_" + name), *_OPTIONS[name][0])

    # -- reference API ---------------------------------------------------------------------
    def init(self, m, nr, a=1e2, c=1e-6, batch=1):
        self._chk(self._L.icp_init_batched(self._h, batch, m, nr, a, c, self._max_it, self._ang, self._tra))
        self.m, self.nr, self.batch = m, nr, batch
        self.__dict__.pop("_registered", None)     # (icp_init unregisters the frame buffers of an earlier configuration)

    def write(self, mem=Memory.D_IN_F, ptr=None, block=False, batch_index=0):
        arr = None
        if ptr is not None:
            arr = np.ascontiguousarray(ptr, dtype=np.float32)
            want = _write_floats(mem, self.m)
            if arr.size != want:
                raise ValueError("write(%d): expected %d floats, got %d" % (mem, want, arr.size))
        self._chk(self._L.icp_write_b(self._h, batch_index, mem, _p(arr) if arr is not None else None, int(block)))

    def read(self, mem=Memory.H_IO_T, batch_index=0):
        nbytes = self._L.icp_mem_size(self._h, mem)
        if nbytes == 0:
            raise ValueError("unknown memory object %r" % (mem,))
        dt, cols = _MEM_DTYPE[mem]
        out = np.empty(nbytes // np.dtype(dt).itemsize, dt)
        self._chk(self._L.icp_read_b(self._h, batch_index, mem, _p(out), nbytes))
        return out.reshape(-1, cols) if cols else out

    def buildRBC(self):
        self._chk(self._L.icp_build_rbc(self._h))

    def run(self, config=False):
        """ICPStep::run — one iteration (enqueue only)."""
        self._chk(self._L.icp_step(self._h, int(config)))

    def getAlpha(self):
        return self._out(self._L.icp_get_alpha, C.c_float)[0]

    def setAlpha(self, a):
        self._chk(self._L.icp_set_alpha(self._h, a))

    def getScaling(self):
        return self._out(self._L.icp_get_scaling, C.c_float)[0]

    def setScaling(self, c):
        self._chk(self._L.icp_set_scaling(self._h, c))

    def setMetricScale(self, f_g):
        """Absolute scale of the metric: reported dist = f_g (geo + a pho); matters for the weights only."""
        self._chk(self._L.icp_set_metric_scale(self._h, f_g))

    def getMetricScale(self):
        return self._out(self._L.icp_get_metric_scale, C.c_float)[0]

    # -- extensions ------------------------------------------------------------------------
    def setPowerMode(self, mode):
        self._chk(self._L.icp_set_power_mode(self._h, mode))

    def setReduceMode(self, mode):
        self._chk(self._L.icp_set_reduce_mode(self._h, mode))

    def sync(self):
        self._chk(self._L.icp_sync(self._h))

    def run_fixed(self, iterations):
        """ICP::run(timer) — exactly `iterations` steps, no convergence test (enqueue only)."""
        self._chk(self._L.icp_run_fixed(self._h, iterations))

    def run_fixed_fresh(self, iterations):
        """reset_transform() + run_fixed(iterations) as one graph (enqueue only)."""
        self._chk(self._L.icp_run_fixed_fresh(self._h, iterations))

    def write_cloud(self, which, cloud):
        cloud = np.ascontiguousarray(cloud, np.float32)
        if cloud.size != 640 * 480 * 8:
            raise ValueError("expected a 640x480 float8 cloud")
        self._chk(self._L.icp_write_cloud(self._h, which, _p(cloud), 1))

    def track_next(self, cloud, warm_start=False):
        """Frame-to-frame tracking: feeds the next 640x480 float8 frame; returns k (iterations) once there is a previous
        frame to register against, else None.  One upload per frame; the previous landmarks stay on the device."""
        cloud = np.ascontiguousarray(cloud, np.float32)
        if cloud.size != 640 * 480 * 8:
            raise ValueError("expected a 640x480 float8 cloud")
        k, registered = self._out(self._L.icp_track_next, _p(cloud), int(warm_start), C.c_uint32, C.c_int)
        return k if registered else None

    def track_form(self):
        """1: tracked frames alternate between two streams behind device-side gates; 0: one stream, host-ordered (icp_track_form)."""
        return self._out(self._L.icp_track_form, C.c_int)[0]

    def track_reset(self):
        self._chk(self._L.icp_track_reset(self._h))

    def track_submit(self, cloud, warm_start=False):
        """Enqueues a frame (upload of its band + getLMs on the copy stream, buildRBC + as many iterations of a host-driven checked run as the
        last two registrations suggest; later track_* calls top it up): returns at once.
        `cloud`: a 640x480 float8 array, or the index (0 / 1) of one of the engine's pinned frame buffers (track_staging)."""
        if isinstance(cloud, int):
            ptr = C.c_void_p(self.track_staging(cloud).ctypes.data)
        else:
            cloud = np.ascontiguousarray(cloud, np.float32)
            if cloud.size != 640 * 480 * 8:
                raise ValueError("expected a 640x480 float8 cloud")
            ptr = _p(cloud)
        self._chk(self._L.icp_track_submit(self._h, ptr, int(warm_start)))

    def track_collect(self):
        """Result of the oldest frame in flight (blocking): (k, T[8]) or None for the first frame of a sequence."""
        T = np.empty(8, np.float32)
        k, registered = self._out(self._L.icp_track_collect, C.c_uint32, _p(T), C.c_int)
        return (k, T) if registered else None

    def track_staging(self, slot):
        """Pinned host buffer `slot` (0 / 1) for a whole frame, as a (307200, 8) float32 array: fill it, then track_submit(slot)."""
        p = C.c_void_p()
        self._chk(self._L.icp_track_staging(self._h, slot, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(640 * 480, 8))

    def track_register(self, frames):
        """Page-locks the caller's own frame array(s) (C-contiguous float32, one or more 640x480x8 frames) as DMA sources."""
        a = np.asarray(frames)
        assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and a.nbytes >= 640 * 480 * 32
        self._chk(self._L.icp_track_register_source(self._h, _p(a), a.nbytes))
        # (the array stays alive while its pages are locked: the engine unregisters what is left at init / close)
        self.__dict__.setdefault("_registered", {})[a.ctypes.data] = a

    def track_unregister(self, frames):
        a = np.asarray(frames)
        self._chk(self._L.icp_track_unregister_source(self._h, _p(a)))
        self.__dict__.get("_registered", {}).pop(a.ctypes.data, None)

    def track_pipelined(self, frames, warm_start=False, depth=2, pinned=False):
        """Feeds a sequence with `depth` frames in flight; returns [None | (k, T)] per frame.  pinned: every frame is first copied
        into one of the engine's two pinned frame buffers (what a capture loop that writes there directly would skip)."""
        out, inflight = [], 0
        for i, f in enumerate(frames):
            if inflight >= depth:
                out.append(self.track_collect())
                inflight -= 1
            if pinned:
                self.track_staging(i & 1)[...] = np.asarray(f, np.float32).reshape(-1, 8)
                self.track_submit(i & 1, warm_start)
            else:
                self.track_submit(f, warm_start)
            inflight += 1
        while inflight:
            out.append(self.track_collect())
            inflight -= 1
        return out

    def transform_cloud(self, cloud, T=None, kind=TransformKind.QUATERNION):
        """ICPTransform: the handle's current T (default), or an explicit one — [q | t, s] for the quaternion kinds,
        a row-major 4x4 for TransformKind.MATRIX."""
        cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 8)
        out = np.empty_like(cloud)
        if T is None:
            if kind != TransformKind.QUATERNION:
                raise ValueError("an explicit T is required for this kind")
            self._chk(self._L.icp_transform_cloud(self._h, _p(cloud), _p(out), cloud.shape[0]))
        else:
            T = np.ascontiguousarray(T, np.float32).reshape(-1)
            if T.size != (16 if kind == TransformKind.MATRIX else 8):
                raise ValueError("T has %d floats" % T.size)
            self._chk(self._L.icp_transform_cloud_ex(self._h, kind, _p(T), _p(cloud), _p(out), cloud.shape[0]))
        return out

    def time_run_fixed(self, iterations, reps, from_identity=False):
        return self._out(self._L.icp_time_run_fixed, iterations, reps, int(from_identity), C.c_float)[0]

    def time_run_fixed_tail(self, iterations, reps, from_identity=False):
        """`reps` passes, HIP events around all but the first: (ms over the timed passes, number of timed passes)."""
        return self._out(self._L.icp_time_run_fixed_tail, iterations, reps, int(from_identity), C.c_float, C.c_uint32)

    def reset_transform(self):
        """T <- identity, k <- 0 (enqueue only)."""
        self._chk(self._L.icp_reset_transform(self._h))

    def launches_per_iteration(self):
        """Kernel launches per iteration of run() / run_fixed(): 4 (reference order), 2 (fused) or 1 (fused, chained)."""
        return self._out(self._L.icp_launches_per_iteration, C.c_uint32)[0]

    def run_form(self):
        """0 separate launches per stage, 1 chained (one launch per iteration)."""
        return self._out(self._L.icp_run_form, C.c_int)[0]

    def search_layout(self):
        """(dense, representatives per LDS tile, stage-2 form) of the search kernel in use (diagnostic, see icp_search_layout)."""
        return self._out(self._L.icp_search_layout, C.c_int, C.c_int, C.c_int)

    def time_masked(self, mask, iterations=40, reps=20):
        """us per iteration of a graph holding only the kernels in `mask` (diagnostic)."""
        return self._out(self._L.icp_time_masked, mask, iterations, reps, C.c_float)[0] * 1e3 / (iterations * reps)

    def profile_run(self, iterations=40, print_table=False):
        """ICP::run(timer) (include/ICP/algorithms.hpp:2482-2494): `iterations` steps with per-step, per-stage times.
        Returns (table[iterations][4] in ms: search, means, sij, finalize; total ms); print_table: the reference's
        ProfilingInfo-style summary (mean / min / max / total per stage)."""
        t = np.zeros((iterations, 4), np.float32)
        tot = C.c_float()
        self._chk(self._L.icp_profile_run(self._h, iterations, _p(t), C.byref(tot)))
        if print_table:
            print(" ICP::run (timer): %d steps, %.3f ms in all" % (iterations, tot.value))
            print(" %-10s %10s %10s %10s %10s" % ("stage", "mean [us]", "min [us]", "max [us]", "total [ms]"))
            for k, name in enumerate(("search", "means", "sij", "finalize")):
                c = t[:, k] * 1e3
                print(" %-10s %10.2f %10.2f %10.2f %10.3f" % (name, c.mean(), c.min(), c.max(), c.sum() / 1e3))
            s = t.sum(1) * 1e3
            print(" %-10s %10.2f %10.2f %10.2f %10.3f" % ("step", s.mean(), s.min(), s.max(), s.sum() / 1e3))
        return t, tot.value

    def time_kernels(self, reps):
        out = (C.c_float * 4)()
        self._chk(self._L.icp_time_kernels(self._h, reps, out))
        return dict(zip(("search", "means", "sij", "finalize"), [float(v) for v in out]))

    def state(self, batch_index=0):
        st = _State()
        self._chk(self._L.icp_state_b(self._h, batch_index, C.byref(st)))
        return st

    def evaluate(self, max_dist=0.0, count=None):
        """Registration quality at the current transform (icp_evaluate; blocking): a list of Quality records, one per registration
        0 .. count - 1 (count None: the whole batch).  max_dist: the largest distance of an inlier pair, in the cloud's units (None, 0
        or inf: no distance test).  The handle's options have no influence, and the call disturbs nothing an iteration reads or writes."""
        n = self.batch if count is None else int(count)
        out = (Quality * max(n, 1))()
        self._chk(self._L.icp_evaluate(self._h, _max_dist_arg(max_dist), out, n))
        return list(out)[:n]

    def correspondences(self, source=Pairs.EVALUATED, max_dist=0.0, batch_index=0):
        """The correspondence set of registration batch_index (icp_correspondences + icp_correspondences_read; blocking): a structured
        array of dtype PAIR (moving, fixed, geo, weight), one record per member pair in ascending query index.  Pairs.EVALUATED: the
        inliers of evaluate() at the same max_dist; Pairs.LAST_ITERATION: the pairs with a weight != 0 in the last executed iteration
        (max_dist must be 0).  One launch set computes the sets of the whole batch; the others stay readable (correspondences_read)."""
        counts = (C.c_uint32 * self.batch)()
        self._chk(self._L.icp_correspondences(self._h, source, _max_dist_arg(max_dist), counts, self.batch))
        return self.correspondences_read(batch_index)

    def correspondences_read(self, batch_index=0):
        """The set of registration batch_index as the last correspondences() computed it (icp_correspondences_read)."""
        n = C.c_uint32()
        rc = self._L.icp_correspondences_read(self._h, batch_index, None, 0, C.byref(n))
        if rc and not (rc == 1 and n.value):               # (ICP_EINVAL with a count: the set is there and needs room)
            self._chk(rc)
        out = np.empty(n.value, PAIR)
        if n.value:
            self._chk(self._L.icp_correspondences_read(self._h, batch_index, _p(out), n.value, C.byref(n)))
        return out

    def _vec(self, name, shape=None):
        a = np.array(getattr(self.state(), name), dtype=np.float32)
        return a.reshape(shape) if shape else a

    R = property(lambda s: s._vec("R", (3, 3)))
    Rk = property(lambda s: s._vec("Rk", (3, 3)))
    q = property(lambda s: s._vec("q"))
    qk = property(lambda s: s._vec("qk"))
    t = property(lambda s: s._vec("t"))
    tk = property(lambda s: s._vec("tk"))
    s = property(lambda s: float(s.state().s))
    sk = property(lambda s: float(s.state().sk))
    k = property(lambda s: int(s.state().k))


class ICP(ICPStep):
    """Full registration loop — mirror of cl_algo::ICP::ICP<CR,CW> (include/ICP/algorithms.hpp:2433-2496)."""

    def init(self, m, nr, a=1e2, c=1e-6, max_iterations=40, angle_threshold=0.001,
             translation_threshold=0.01, batch=1):
        self._max_it, self._ang, self._tra = max_iterations, angle_threshold, translation_threshold
        super().init(m, nr, a, c, batch)

    def run(self):
        """ICP::run — iterate until check() stops (blocking); returns k."""
        return self._out(self._L.icp_run, C.c_uint32)[0]

    def step(self, config=False):
        ICPStep.run(self, config)

    def run_stats(self):
        """(iteration launches enqueued, final k, launches past the last live iteration) of the last finished checked run."""
        return self._out(self._L.icp_run_stats, C.c_uint32, C.c_uint32, C.c_uint32)

    def run_timeline(self):
        """Host timeline of the last run() in us: [0, launches enqueued, first progress seen, decided, end enqueued, FINAL seen]."""
        t = (C.c_double * 6)()
        self._chk(self._L.icp_run_timeline(self._h, t))
        return [float(x) for x in t]

    def launch_stats(self, reset=False):
        """(longest launch call in us, calls slower than 10 us, calls) of the checked runs since init / the last reset."""
        return self._out(self._L.icp_launch_stats, C.c_double, C.c_uint64, C.c_uint64, int(reset))

    def set_output_mode(self, every_iteration=False):
        """Per-query outputs of checked runs: stored by every iteration, or (default) reproduced on the first read (icp_set_output_mode)."""
        self._chk(self._L.icp_set_output_mode(self._h, int(every_iteration)))

    def set_run_depth(self, depth=3, adaptive=True):
        """Launches kept queued behind the one in flight by checked runs; adaptive=False: one graph of max_iterations launches."""
        self._chk(self._L.icp_set_run_depth(self._h, depth, int(adaptive)))

    def getMaxIterations(self):
        return self._out(self._L.icp_get_max_iterations, C.c_uint32)[0]

    def setMaxIterations(self, n):
        self._chk(self._L.icp_set_max_iterations(self._h, n))
        self._max_it = n

    def getAngleThreshold(self):
        return self._out(self._L.icp_get_angle_threshold, C.c_double)[0]

    def setAngleThreshold(self, deg):
        self._chk(self._L.icp_set_angle_threshold(self._h, deg))
        self._ang = deg

    def getTranslationThreshold(self):
        return self._out(self._L.icp_get_translation_threshold, C.c_double)[0]

    def setTranslationThreshold(self, mm):
        self._chk(self._L.icp_set_translation_threshold(self._h, mm))
        self._tra = mm


def batch_partition(registrations, n_slots, i):
    """(slot, index inside the slot, registrations of that slot) of registration i — icp_batch_partition (no device needed)."""
    slot, idx, cnt = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = lib().icp_batch_partition(registrations, n_slots, i, C.byref(slot), C.byref(idx), C.byref(cnt))
    if rc:
        raise ICPError(rc, "icp_batch_partition: bad arguments")
    return slot.value, idx.value, cnt.value


class ICPBatch(_Options):
    """B independent registrations over a list of devices inside the library (icp_batch_*, include/icp_amd.h):
    registration i -> device slot i mod n, one host thread and one stream per slot, no collective."""

    def __init__(self, devices, CR=ICPStepConfigT.POWER_METHOD, CW=ICPStepConfigW.WEIGHTED):
        self._L = lib()
        self._b = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        rc = self._L.icp_batch_create(C.byref(self._b), devs, len(devices), CR, CW)
        if rc:
            msg = self._L.icp_batch_last_error(None).decode()
            self._b = None
            raise ICPError(rc, msg)
        self.m = 0

    def _chk(self, rc):
        if rc:
            raise ICPError(rc, self._L.icp_batch_last_error(self._b).decode())

    def slot_cpus(self, slot):
        """The CPUs the host thread of a device slot was pinned to ([] = not pinned)."""
        buf = C.create_string_buffer(16384)
        self._chk(self._L.icp_batch_slot_cpus(self._b, slot, buf, len(buf)))
        return [int(x) for x in buf.value.decode().split(",") if x]

    def close(self):
        if getattr(self, "_b", None):
            self._L.icp_batch_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init(self, registrations, m, nr, a=1e2, c=1e-6, max_iterations=40, angle_threshold=0.001, translation_threshold=0.01):
        self._chk(self._L.icp_batch_init(self._b, registrations, m, nr, a, c, max_iterations, angle_threshold, translation_threshold))
        self.m, self.registrations = m, registrations

    def set_modes(self, reduce_mode, power_mode):
        self._chk(self._L.icp_batch_set_modes(self._b, reduce_mode, power_mode))

    def _set(self, name, *cargs):
        self._chk(getattr(self._L, "icp_batch_set_" + name)(self._b, *cargs))
        # (the library has no icp_batch_get_*: the batch answers with what it last set, as the C types hold it)
        self.__dict__.setdefault("_options", {})[name] = tuple(t(v).value for t, v in zip(_OPTIONS[name][0], cargs))

    def _get(self, name):
        return self.__dict__.get("_options", {}).get(name, _OPTIONS[name][1])

    def write(self, i, mem, ptr):
        arr = np.ascontiguousarray(ptr, dtype=np.float32)
        want = _write_floats(mem, self.m)
        if arr.size != want:
            raise ValueError("write(%d): expected %d floats, got %d" % (mem, want, arr.size))
        self._chk(self._L.icp_batch_write(self._b, i, mem, _p(arr)))

    def buildRBC(self):
        self._chk(self._L.icp_batch_build_rbc(self._b))

    def run(self):
        self._chk(self._L.icp_batch_run(self._b))

    def run_fixed(self, iterations, from_identity=True):
        self._chk(self._L.icp_batch_run_fixed(self._b, iterations, int(from_identity)))

    def time_run_fixed(self, iterations, reps):
        """Wall-clock seconds of `reps` passes on all slots at once."""
        s = C.c_double()
        self._chk(self._L.icp_batch_time_run_fixed(self._b, iterations, reps, C.byref(s)))
        return s.value

    def time_run_fixed_slots(self, iterations, reps, warmup=1):
        """(wall-clock seconds of `reps` passes on all slots at once, HIP-event ms of every slot's own passes)."""
        s = C.c_double()
        n = C.c_uint32()
        self._chk(self._L.icp_batch_size(self._b, None, C.byref(n)))
        ms = np.zeros(n.value, np.float32)
        self._chk(self._L.icp_batch_time_run_fixed_slots(self._b, iterations, reps, warmup, C.byref(s), _p(ms)))
        return s.value, ms

    def state(self, i):
        st = _State()
        self._chk(self._L.icp_batch_state(self._b, i, C.byref(st)))
        return st

    def evaluate(self, i, max_dist=0.0):
        """ICPStep.evaluate of registration i: its Quality record (icp_batch_evaluate)."""
        q = Quality()
        self._chk(self._L.icp_batch_evaluate(self._b, i, _max_dist_arg(max_dist), C.byref(q)))
        return q

    def correspondences(self, i, source=Pairs.EVALUATED, max_dist=0.0):
        """ICPStep.correspondences of registration i (icp_batch_correspondences): its set as a structured array of dtype PAIR."""
        n = C.c_uint32()
        out = np.empty(self.m, PAIR)                       # (a set has at most m members)
        self._chk(self._L.icp_batch_correspondences(self._b, i, source, _max_dist_arg(max_dist), _p(out), self.m, C.byref(n)))
        return out[:n.value].copy()

    def read(self, i, mem):
        dt, cols = _MEM_DTYPE[mem]
        n = _mem_elements(mem, self.m)
        out = np.empty(n, dt)
        self._chk(self._L.icp_batch_read(self._b, i, mem, _p(out), out.nbytes))
        return out.reshape(-1, cols) if cols else out


class PyramidReduction:          # icp_pyramid_set_reduction (include/icp_amd.h)
    MEAN, PICK = 0, 1


PYRAMID_MAX_LEVELS = 5            # ICP_PYRAMID_MAX_LEVELS


class _PyramidLevel(ICP):
    """The borrowed handle of a pyramid level as an ICP object: every setter, getter, read, state(), evaluate() and correspondences() of ICP; it never
    destroys the handle (close() only lets go of it).  Not for init, writes of F / M, adoption or tracking (include/icp_amd.h)."""

    def __init__(self, handle, m, nr, max_iterations, angle_threshold, translation_threshold):
        self._L = lib()
        self._h = handle
        self.m, self.nr, self.batch = m, nr, 1
        self._max_it, self._ang, self._tra = max_iterations, angle_threshold, translation_threshold

    def close(self):
        self._h = None

    def _refuse(self, what):
        raise ICPError(4, "%s would take the pyramid's levels apart: use ICPPyramid (include/icp_amd.h, icp_pyramid_level)" % what)

    def init(self, *args, **kwargs):
        self._refuse("init of a level")

    def write(self, mem=Memory.D_IN_F, ptr=None, block=False, batch_index=0):
        if mem in (Memory.F, Memory.M):
            self._refuse("a write of F or M into a level")
        super().write(mem, ptr, block, batch_index)

    def write_cloud(self, which, cloud):
        self._refuse("write_cloud into a level")

    def track_next(self, *args, **kwargs):
        self._refuse("tracking on a level")

    track_submit = track_collect = track_staging = track_register = track_unregister = track_pipelined = track_reset = track_next


class ICPPyramid:
    """Coarse-to-fine registration (icp_pyramid_*, include/icp_amd.h): one engine handle per level on one device, the levels of F and M
    built on the device from level 0 by one launch, T handed from each level to the next finer one on the device.  The result is level
    0's: level(0).read(Memory.T), level(0).state(), level(0).evaluate(), level(0).correspondences()."""

    def __init__(self, device=0, CR=ICPStepConfigT.POWER_METHOD, CW=ICPStepConfigW.WEIGHTED):
        self._L = lib()
        self._p = C.c_void_p()
        rc = self._L.icp_pyramid_create(C.byref(self._p), device, CR, CW)
        if rc:
            msg = self._L.icp_pyramid_last_error(None).decode()
            self._p = None
            raise ICPError(rc, msg)
        self.levels = self.m = self.side = 0
        self._levels = []

    def _chk(self, rc):
        if rc:
            raise ICPError(rc, self._L.icp_pyramid_last_error(self._p).decode())

    def close(self):
        if getattr(self, "_p", None):
            for lv in self._levels:
                lv.close()
            self._levels = []
            self._L.icp_pyramid_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def init(self, m, nr, a=1e2, c=1e-6, max_iterations=40, angle_threshold=0.001, translation_threshold=0.01):
        """nr: one count per level, finest first (its length is the number of levels); max_iterations: one number for all levels or
        one per level."""
        nr = [int(v) for v in nr]
        levels = len(nr)
        its = [int(max_iterations)] * levels if np.isscalar(max_iterations) else [int(v) for v in max_iterations]
        if len(its) != levels:
            raise ValueError("max_iterations: expected %d entries, got %d" % (levels, len(its)))
        for lv in self._levels:
            lv.close()
        self._levels = []
        self.levels = 0
        self._chk(self._L.icp_pyramid_init(self._p, levels, m, (C.c_uint32 * max(levels, 1))(*nr), a, c,
                                           (C.c_uint32 * max(levels, 1))(*its), angle_threshold, translation_threshold))
        self.levels, self.m, self.side = levels, m, int(round(m ** 0.5))
        for l in range(levels):
            h = C.c_void_p()
            self._chk(self._L.icp_pyramid_level(self._p, l, C.byref(h)))
            self._levels.append(_PyramidLevel(h, (self.side >> l) ** 2, nr[l], its[l], angle_threshold, translation_threshold))

    def level(self, l):
        """The ICP object over the borrowed handle of level l (0: the finest)."""
        if not 0 <= l < self.levels:
            h = C.c_void_p()
            self._chk(self._L.icp_pyramid_level(self._p, l if l >= 0 else 0xFFFFFFFF, C.byref(h)))
        return self._levels[l]

    def set_reduction(self, kind=PyramidReduction.MEAN, max_dz=0.0):
        """How a level is made from the one below it: MEAN (of the valid points of each 2 x 2 block within max_dz * 2^(l-1) of the first
        valid one in z; 0 or inf: no band) or PICK (the block's first point).  Takes effect at the next write."""
        self._chk(self._L.icp_pyramid_set_reduction(self._p, kind, max_dz))

    def reduction(self):
        k, z = C.c_int(), C.c_float()
        self._chk(self._L.icp_pyramid_get_reduction(self._p, C.byref(k), C.byref(z)))
        return k.value, z.value

    def write(self, mem, ptr=None, block=False):
        arr = None
        if ptr is not None:
            arr = np.ascontiguousarray(ptr, dtype=np.float32)
            want = _write_floats(mem, self.m)
            if arr.size != want:
                raise ValueError("write(%d): expected %d floats, got %d" % (mem, want, arr.size))
        self._chk(self._L.icp_pyramid_write(self._p, mem, _p(arr) if arr is not None else None, int(block)))

    def write_cloud(self, which, cloud, block=False):
        arr = np.ascontiguousarray(cloud, dtype=np.float32)
        if arr.size != 640 * 480 * 8:
            raise ValueError("write_cloud: expected a 640 x 480 x 8 cloud")
        self._chk(self._L.icp_pyramid_write_cloud(self._p, which, _p(arr), int(block)))

    def buildRBC(self):
        self._chk(self._L.icp_pyramid_build_rbc(self._p))

    def run(self):
        """A checked run per level, coarsest first (blocking); returns the iteration counts, finest first."""
        k = (C.c_uint32 * PYRAMID_MAX_LEVELS)()
        self._chk(self._L.icp_pyramid_run(self._p, k))
        return [int(v) for v in k[:self.levels]]

    def run_fixed(self, iterations):
        """Exactly iterations[l] steps per level (finest first); enqueue only — sync() waits."""
        its = [int(v) for v in iterations]
        if len(its) != self.levels:
            raise ValueError("run_fixed: expected %d counts, got %d" % (self.levels, len(its)))
        self._chk(self._L.icp_pyramid_run_fixed(self._p, (C.c_uint32 * max(len(its), 1))(*its)))

    def reset_transform(self):
        self._chk(self._L.icp_pyramid_reset_transform(self._p))

    def sync(self):
        self._chk(self._L.icp_pyramid_sync(self._p))

    def pending(self):
        """True while what the last run_fixed enqueued is still in flight (a query, not a wait)."""
        v = C.c_int()
        self._chk(self._L.icp_pyramid_pending(self._p, C.byref(v)))
        return bool(v.value)

    def time_build(self, mem=Memory.F, reps=20):
        """Mean ms of the construction launch of F or M alone (HIP events around it)."""
        ms = C.c_float()
        self._chk(self._L.icp_pyramid_time_build(self._p, mem, reps, C.byref(ms)))
        return ms.value
