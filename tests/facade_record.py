"""What the Python facade (icp_amd/__init__.py, icp_amd/register.py) does with its arguments, recorded without the library and without a
device: record(pkg, reg) drives every option setter and getter, the scalar get / set pairs, the reads and writes and register.py's
functions of the package it is given over a stand-in for the library that logs every call, and returns the log, the return values, the
exceptions and the public surface as plain JSON data.  tests/golden/python_facade_calls.json is record() of the commit before the
facade's options moved into one table (the same icp_amd/__init__.py and register.py loaded as a scratch package);
tests/test_python_facade_cpu.py compares the working tree's record() with it.

    python tests/facade_record.py <directory that holds the icp_amd package to record> > tests/golden/python_facade_calls.json
"""
import contextlib
import ctypes as C
import hashlib
import inspect
import io
import json
import os
import sys
import types

import numpy as np

INF = float("inf")
MESSAGE = "the stub says no"
STATUS = 7

# every option's setter: its defaults, its off spelling, values float32 does not hold (0.1, 60.3), positional and by keyword
SETTER_CALLS = {
    "set_rejection": [((), {}), ((False, None), {}), ((True, 60.3), {}), ((), {"invalid": True}), ((), {"max_dist": 0.1}), ((False, 0), {}),
                      ((True, INF), {}), ((1, 5), {})],
    "set_trimming": [((), {}), ((1.0,), {}), ((0.1,), {}), ((), {"keep": 0.7}), ((1,), {})],
    "set_unique": [((), {}), ((False,), {}), ((), {"on": True}), ((0,), {}), ((1,), {})],
    "set_median_rejection": [((0,), {}), ((2.5,), {}), ((), {"factor": 0.1}), ((), {})],
    "set_adaptive_trimming": [((), {}), ((0.0, 0.0, 0), {}), ((0.1, 0.9, 3), {}), ((), {"min_fraction": 0.4, "max_fraction": 1, "power": 2})],
    "set_reciprocal": [((), {}), ((False,), {}), ((True, 0.1), {}), ((False, 5.0), {}), ((), {"max_gap": 60.3}), ((0, 0.1), {})],
    "set_normal_rejection": [((), {}), ((None,), {}), ((0.1,), {}), ((), {"min_cos": -1}), ((0,), {}), ((60.3,), {})],
    "set_projective": [((), {}), ((None,), {}), ((128, 60.3, 0.1, 63.5, 47.5, 2), {}), ((0,), {}),
                       ((64,), {"fx": 0.1, "fy": 0.2, "cx": 1, "cy": 2, "radius": 1}), ((), {"grid_width": 16}), ((0, 60.3, 0.1), {})],
    "set_boundary_rejection": [((), {}), ((None,), {}), ((128,), {}), ((0,), {}), ((), {"grid_width": 16})],
    "set_robust_loss": [((), {}), ((0, 0.0), {}), ((3, 60.3), {}), ((), {"loss": 1, "scale": 0.1})],
    "set_error_metric": [((), {}), ((0, 0.0), {}), ((1, 0.1), {}), ((), {"metric": 2, "point_weight": 60.3})],
    "set_normals": [((), {}), ((0, 0), {}), ((1, 128), {}), ((), {"source": 1, "grid_width": 16})],
    "set_color_weight": [((0,), {}), ((0.1,), {}), ((), {"kappa": 60.3}), ((), {})],
    "set_plane_to_plane": [((0,), {}), ((0.1,), {}), ((), {"epsilon": 1}), ((), {})],
    "set_symmetric": [((), {}), ((False,), {}), ((), {"on": 1}), ((0,), {}), ((2,), {})],
}

# every option's getter: the C values the library is made to answer with — on, off, 0 and inf
GETTER_VALUES = {
    "rejection": [(0, 0.0), (1, 0.0), (1, 60.3), (0, INF), (3, 0.1), (2, 5.0)],
    "trimming": [(1.0,), (0.1,)],
    "unique": [(0,), (1,), (2,)],
    "median_rejection": [(0.0,), (60.3,)],
    "adaptive_trimming": [(0.0, 0.0, 0), (0.1, 0.9, 3)],
    "reciprocal": [(0, 0.0), (1, 0.0), (1, 0.1), (0, 60.3)],
    "normal_rejection": [(0, 0.0), (1, 0.0), (1, 0.1), (0, 0.1), (1, -1.0)],
    "projective": [(0, 0, 0.0, 0.0, 0.0, 0.0, 0), (1, 128, 60.3, 0.1, 63.5, 47.5, 2), (0, 128, 60.3, 0.1, 63.5, 47.5, 2), (1, 16, 1.0, 1.0, 0.0, 0.0, 0)],
    "boundary_rejection": [(0,), (128,)],
    "robust_loss": [(0, 0.0), (3, 60.3)],
    "error_metric": [(0, 0.0), (2, 0.1)],
    "normals": [(0, 0), (1, 128)],
    "color_weight": [(0.0,), (0.1,)],
    "plane_to_plane": [(0.0,), (0.1,)],
    "symmetric": [(0,), (1,)],
}

# the other methods that hand the library pointers to fill: (class names, method, arguments)
OUT_CALLS = [
    (("ICPStep", "ICP"), "getAlpha", ()), (("ICPStep", "ICP"), "getScaling", ()), (("ICPStep", "ICP"), "getMetricScale", ()),
    (("ICPStep", "ICP"), "setAlpha", (0.1,)), (("ICPStep", "ICP"), "setScaling", (60.3,)), (("ICPStep", "ICP"), "setMetricScale", (0.1,)),
    (("ICPStep", "ICP"), "setPowerMode", (1,)), (("ICPStep", "ICP"), "setReduceMode", (0,)),
    (("ICPStep", "ICP"), "launches_per_iteration", ()), (("ICPStep", "ICP"), "run_form", ()), (("ICPStep", "ICP"), "search_layout", ()),
    (("ICPStep", "ICP"), "track_form", ()), (("ICPStep", "ICP"), "track_collect", ()), (("ICPStep", "ICP"), "track_next", ("cloud", True)),
    (("ICPStep", "ICP"), "time_run_fixed", (40, 3, True)), (("ICPStep", "ICP"), "time_run_fixed_tail", (40, 3)),
    (("ICPStep", "ICP"), "time_masked", (5, 40, 20)), (("ICPStep", "ICP"), "read", (2,)), (("ICPStep", "ICP"), "read", (99,)),
    (("ICPStep",), "run", (True,)),
    (("ICP",), "run", ()), (("ICP",), "run_stats", ()), (("ICP",), "launch_stats", ()), (("ICP",), "launch_stats", (True,)),
    (("ICP",), "getMaxIterations", ()), (("ICP",), "getAngleThreshold", ()), (("ICP",), "getTranslationThreshold", ()),
    (("ICP",), "setMaxIterations", (7,)), (("ICP",), "setAngleThreshold", (0.1,)), (("ICP",), "setTranslationThreshold", (60.3,)),
    (("ICPBatch",), "set_modes", (1, 0)), (("ICPBatch",), "time_run_fixed", (40, 3)),
]

M, NR = 256, 4


def plain(v):
    """v as JSON data: tuples as lists, arrays by shape and dtype, ctypes objects by value, pointers as a word."""
    if isinstance(v, (tuple, list)):
        return [plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return "array %s %s" % (v.dtype.name if v.dtype.names is None else "record", list(v.shape))
    if isinstance(v, C.c_void_p):
        return "pointer"
    if hasattr(v, "_obj"):                                 # (what byref returns)
        return "out " + type(v._obj).__name__
    if isinstance(v, (C._SimpleCData,)):
        return plain(v.value)
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


class Library:
    """Stands in for the shared library: every icp_* entry point logs (name, arguments behind the handle), fills the pointers it is handed
    from `values` (or with 3, 4, .. and 0.1, 0.2, ..) and returns `status`."""

    def __init__(self):
        self.log, self.status, self.values = [], 0, None

    def __getattr__(self, name):
        if not name.startswith("icp_"):
            raise AttributeError(name)
        if name.endswith("last_error"):
            return lambda handle=None: MESSAGE.encode()
        if name == "icp_mem_size":
            return lambda handle, mem: 32 if mem == 2 else 0

        def entry(handle, *args):
            self.log.append([name, plain(args)])
            outs = [a._obj for a in args if hasattr(a, "_obj")]
            for i, o in enumerate(outs):
                if self.values is not None:
                    o.value = self.values[i]
                elif isinstance(o, (C.c_float, C.c_double)):
                    o.value = 0.1 * (i + 1)
                elif not isinstance(o, C.c_void_p):
                    o.value = 3 + i
            return self.status
        return entry

    def take(self):
        log, self.log = self.log, []
        return log


def make(pkg, cls_name, lib):
    """An object of the class without its constructor: the library's stand-in, a handle, and a registration's sizes."""
    cls = getattr(pkg, cls_name)
    obj = object.__new__(cls)
    obj._L = lib
    setattr(obj, {"ICPBatch": "_b", "ICPPyramid": "_p"}.get(cls_name, "_h"), C.c_void_p(1))
    obj.m, obj.nr, obj.batch = M, NR, 1
    return obj


def let_go(obj):
    for handle in ("_h", "_b", "_p"):
        if handle in obj.__dict__:
            setattr(obj, handle, None)


def call(lib, obj, method, args=(), kwargs={}):
    """One call: what it returned or raised, and what it asked of the library."""
    f = getattr(obj, method, None)
    if f is None:
        return {"absent": True}
    args = tuple(np.zeros((640 * 480, 8), np.float32) if isinstance(a, str) and a == "cloud" else a for a in args)
    entry = {}
    try:
        entry["returns"] = plain(f(*args, **kwargs))
    except Exception as e:
        entry["raises"] = [type(e).__name__, str(e) if not isinstance(e, TypeError) else ""]      # (a TypeError names the function: kept out)
    entry["calls"] = lib.take()
    return entry


def record_options(pkg):
    out = {}
    for cls_name in ("ICPStep", "ICP", "ICPBatch"):
        lib = Library()
        rec = out[cls_name] = {"setters": {}, "getters": {}, "refused": {}, "others": []}
        for setter, calls in SETTER_CALLS.items():
            obj = make(pkg, cls_name, lib)
            entries = rec["setters"][setter] = []
            for args, kwargs in calls:
                lib.status, lib.values = 0, None
                e = call(lib, obj, setter, args, kwargs)
                e["args"], e["kwargs"] = plain(args), plain(kwargs)
                if cls_name == "ICPBatch":                 # (what the batch then answers: it asks the library nothing)
                    e["then"] = call(lib, obj, setter[4:])
                entries.append(e)
            let_go(obj)
            # a refused call raises with the library's message, on a fresh object and after an accepted call: the batch keeps what it held
            obj = make(pkg, cls_name, lib)
            steps = rec["refused"][setter] = []
            for (args, kwargs), status in ((calls[2], STATUS), (calls[1], 0), (calls[2], STATUS)):
                lib.status, lib.values = status, None
                e = call(lib, obj, setter, args, kwargs)
                if cls_name == "ICPBatch":
                    e["then"] = call(lib, obj, setter[4:])
                elif status:
                    e["getter"] = call(lib, obj, setter[4:])
                steps.append(e)
            let_go(obj)
        if cls_name != "ICPBatch":
            obj = make(pkg, cls_name, lib)
            for getter, answers in GETTER_VALUES.items():
                entries = rec["getters"][getter] = []
                for values in answers:
                    lib.status, lib.values = 0, values
                    entries.append(call(lib, obj, getter))
            let_go(obj)
        obj = make(pkg, cls_name, lib)
        for classes, method, args in OUT_CALLS:
            if cls_name in classes:
                for status in (0, STATUS):
                    lib.status, lib.values = status, None
                    e = call(lib, obj, method, args)
                    e["method"], e["args"], e["status"] = method, plain(args), status
                    rec["others"].append(e)
        let_go(obj)
    return out


def record_memory(pkg):
    """Reads of every memory object through the batch (the byte count it asks for), writes with a wrong size (the count they want)."""
    out = {"batch_read": {}, "write": {}, "mem_dtype": {}}
    lib = Library()
    batch = make(pkg, "ICPBatch", lib)
    for mem in range(34):
        out["batch_read"][str(mem)] = call(lib, batch, "read", (0, mem))
    objs = {n: make(pkg, n, lib) for n in ("ICPStep", "ICPBatch", "ICPPyramid")}
    for mem in range(34):
        wrong = np.zeros(3, np.float32)
        out["write"][str(mem)] = {"ICPStep": call(lib, objs["ICPStep"], "write", (mem, wrong)), "ICPBatch": call(lib, objs["ICPBatch"], "write", (0, mem, wrong)),
                                  "ICPPyramid": call(lib, objs["ICPPyramid"], "write", (mem, wrong))}
    for mem, (dt, cols) in pkg._MEM_DTYPE.items():
        out["mem_dtype"][str(mem)] = [np.dtype(dt).str if np.dtype(dt).names is None else "record", cols]
    for o in [batch] + list(objs.values()):
        let_go(o)
    return out


def record_surface(pkg, reg):
    """Every public name of the four classes and of register.py's functions: its signature and its docstring's digest."""
    def entry(f):
        if not callable(f):
            return type(f).__name__
        return [str(inspect.signature(f)), hashlib.sha1((f.__doc__ or "").encode()).hexdigest()[:12]]
    out = {}
    for cls_name in ("ICPStep", "ICP", "ICPBatch", "ICPPyramid"):
        cls = getattr(pkg, cls_name)
        out[cls_name] = {n: entry(getattr(cls, n)) for n in sorted(dir(cls)) if not n.startswith("_")}
    out["register"] = {n: entry(getattr(reg, n)) for n in ("register_clouds", "register_and_evaluate", "register_with_pairs", "main")}
    return out


class Handle:
    """Stands in for ICP / ICPPyramid / a pyramid level in register.py: logs every method call."""

    def __init__(self, log, who):
        self._log, self._who = log, who

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def method(*args, **kwargs):
            self._log.append([self._who, name, plain(args), plain(kwargs)])
            if name == "level":
                return Handle(self._log, "level %d" % args[0])
            return {"run": [5, 4, 3] if self._who == "pyramid" else 5, "read": np.array([0, 0, 0.6, 0.8, 1, 2, 3, 1], np.float32),
                    "evaluate": [types.SimpleNamespace(fitness=0.5, inlier_rmse=1.5, n_inliers=3, n_moving=4)], "correspondences": "pairs", "transform_cloud": "moved"}.get(name)
        return method


REGISTER_OPTIONS = {
    "all off": {},
    "all on": dict(device=1, a=60.3, c=1e-5, max_iterations=7, angle_threshold=0.1, translation_threshold=0.2, reduce_mode=0, reject_invalid=True,
                   max_dist=60.3, trim=0.7, point_to_plane=0.1, colored=0.2, robust=(3, 60.3), one_to_one=True, normal_angle=30.0,
                   reject_boundary=True, reciprocal=0.1, projective=2, median_factor=2.5),
    "moving normals": dict(plane_to_plane=0.001, max_dist=0.0, reject_invalid=False),
    "symmetric": dict(symmetric=True, point_to_plane=0.1),
    "adaptive trim": dict(adaptive_trim=(0.4, 1.0, 3), reject_invalid=True),
    "pyramid": dict(pyramid=(3, 24.0), projective=0, point_to_plane=0.0, trim=0.9, reject_boundary=True),
}

MAIN_ERRORS = [["--trim", "0"], ["--trim", "1.5"], ["--plane-to-plane", "0"], ["--plane-to-plane", "2"], ["--adaptive-trim", "0.5"],
               ["--adaptive-trim", "0.9:0.1"], ["--adaptive-trim", "0.1:0.9:9"], ["--adaptive-trim", "0.1:0.9", "--trim", "0.5"],
               ["--adaptive-trim", "--trim", "0.5"], ["--median-factor", "0"], ["--median-factor", "inf"], ["--point-to-plane", "-1"],
               ["--colored", "nan"], ["--reciprocal", "-1"], ["--evaluate", "-1"], ["--normal-angle", "200"], ["--projective", "9"],
               ["--projective", "x"], ["--robust", "foo"], ["--robust", "huber:x"], ["--robust", "huber:0"], ["--pyramid", "9"],
               ["--pyramid", "x"], ["--pyramid", "2:-1"], ["--no-such-option"]]

MAIN_RUNS = [[], ["--evaluate", "10"], ["--pairs", os.devnull], ["--evaluate", "0", "--pairs", os.devnull],
             ["--device", "1", "-a", "60.3", "--reject-invalid", "--max-dist", "60.3", "--trim", "0.7", "--one-to-one", "--median-factor", "2.5",
              "--reciprocal", "--projective", "--normal-angle", "30", "--reject-boundary", "--point-to-plane", "0.1", "--colored", "0.2",
              "--robust", "tukey:50", "--evaluate", "10", "-o", "OUT"],
             ["--adaptive-trim", "--plane-to-plane", "0.001", "--reciprocal", "0.1", "--projective", "0", "--pyramid", "3:24"],
             ["--adaptive-trim", "0.4:1:3", "--symmetric", "--pyramid", "2"]]


@contextlib.contextmanager
def stand_ins(reg):
    """register.py with Handle objects for ICP and ICPPyramid and no file access: yields (the log of their calls, what np.save was given)."""
    log = []
    saved = {n: getattr(reg, n) for n in ("ICP", "ICPPyramid", "load_pc8d", "save_pc8d")}
    reg.ICP = lambda device=0: log.append(["ICP", plain(device)]) or Handle(log, "icp")
    reg.ICPPyramid = lambda device=0: log.append(["ICPPyramid", plain(device)]) or Handle(log, "pyramid")
    reg.load_pc8d = lambda path: "cloud " + path
    reg.save_pc8d = lambda path, cloud: log.append(["save_pc8d", path, plain(cloud)])
    saves = []
    np_save, np.save = np.save, lambda f, a: saves.append(plain(a))
    try:
        yield log, saves
    finally:
        np.save = np_save
        for n, v in saved.items():
            setattr(reg, n, v)


def record_register(reg):
    out = {"functions": {}, "unknown option": {}, "main errors": [], "main runs": []}
    with stand_ins(reg) as (log, saves):
        for label, options in REGISTER_OPTIONS.items():
            entry = out["functions"][label] = {}
            for name, args in (("register_clouds", ("F", "M")), ("register_and_evaluate", ("F", "M", 10.0)), ("register_and_evaluate", ("F", "M", None)),
                               ("register_with_pairs", ("F", "M")), ("register_with_pairs", ("F", "M", 0.0)), ("register_with_pairs", ("F", "M", 60.3))):
                del log[:]
                result = list(getattr(reg, name)(*args, **options))
                result[2] = "ms"                           # (the latency: a time)
                entry["%s %s" % (name, plain(args[2:]))] = {"returns": plain(result), "calls": list(log)}
        for name, args in (("register_clouds", ("F", "M")), ("register_and_evaluate", ("F", "M", 1.0)), ("register_with_pairs", ("F", "M"))):
            del log[:]
            try:
                getattr(reg, name)(*args, no_such_option=1)
                out["unknown option"][name] = "returns"
            except Exception as e:
                out["unknown option"][name] = [type(e).__name__, list(log)]
        for argv in MAIN_ERRORS:
            err = io.StringIO()
            try:
                with contextlib.redirect_stderr(err):
                    reg.main(["f", "m"] + argv)
                out["main errors"].append([argv, "returns"])
            except SystemExit as e:
                out["main errors"].append([argv, e.code, err.getvalue().strip().split("error: ")[-1]])
        for argv in MAIN_RUNS:
            del log[:]
            del saves[:]
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                reg.main(["f", "m"] + argv)
            out["main runs"].append({"argv": argv, "calls": list(log), "saved": list(saves),
                                     "prints": [line for line in text.getvalue().split("\n") if "Latency" not in line]})
    return out


def record(pkg, reg):
    return {"options": record_options(pkg), "memory": record_memory(pkg), "surface": record_surface(pkg, reg), "register": record_register(reg)}


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    import icp_amd
    from icp_amd import register
    json.dump(record(icp_amd, register), sys.stdout, indent=0, sort_keys=True)
