"""The Python facade states each option once (icp_amd._OPTIONS, icp_amd._Options, icp_amd._MEM, register.py's record) and behaves as it did
when every option was written out per class: facade_record.record() of the working tree against tests/golden/python_facade_calls.json,
the record of the commit before.  Two differences are deliberate and asserted on their own: ICPBatch.normal_rejection() answers with the
float32 the library holds, and ICPBatch has the eight getters it lacked.  The tests marked gpu tie the two tables to the library."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

import facade_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_BATCH_GETTERS = ["adaptive_trimming", "color_weight", "error_metric", "median_rejection", "normals", "plane_to_plane", "robust_loss", "symmetric"]


def f32(v):
    return float(np.float32(v))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "python_facade_calls.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded():
    """record() of the working tree, through JSON as the golden file went."""
    import icp_amd
    from icp_amd import register
    return json.loads(json.dumps(facade_record.record(icp_amd, register)))


def differences(want, got, path=""):
    """The paths at which two JSON values differ."""
    if type(want) is not type(got):
        return ["%s: %r -> %r" % (path, want, got)]
    if isinstance(want, dict):
        out = ["%s/%s: only in one" % (path, k) for k in sorted(set(want) ^ set(got))]
        return out + [d for k in sorted(set(want) & set(got)) for d in differences(want[k], got[k], "%s/%s" % (path, k))]
    if isinstance(want, list):
        if len(want) != len(got):
            return ["%s: %d -> %d entries" % (path, len(want), len(got))]
        return [d for i, (w, g) in enumerate(zip(want, got)) for d in differences(w, g, "%s/%d" % (path, i))]
    return [] if want == got or (want != want and got != got) else ["%s: %r -> %r" % (path, want, got)]


def test_step_classes_call_the_library_as_before(golden, recorded):
    """ICPStep and ICP: every setter's C arguments, every getter's decoding of scripted C values (on, off, 0, inf), every refused call's
    ICPError with the library's message, and the scalar get / set pairs — the same calls, return values and exceptions."""
    for cls in ("ICPStep", "ICP"):
        assert not differences(golden["options"][cls], recorded["options"][cls], cls)
        assert sorted(recorded["options"][cls]["setters"]) == sorted(facade_record.SETTER_CALLS)
        for setter, steps in recorded["options"][cls]["refused"].items():
            for e in (steps[0], steps[2]):
                assert e["raises"] == ["ICPError", "icp_amd error %d: %s" % (facade_record.STATUS, facade_record.MESSAGE)], (cls, setter)
                assert e["getter"]["raises"] == e["raises"]


def test_batch_calls_the_library_as_before(golden, recorded):
    """ICPBatch: the same C arguments to icp_batch_set_<n>, the same answers of the seven getters it had — but for normal_rejection, which
    is float32 now —, and nothing remembered of a refused call."""
    want = json.loads(json.dumps(golden["options"]["ICPBatch"]))
    for phase in ("setters", "refused"):
        for setter, entries in want[phase].items():
            for e, got in zip(entries, recorded["options"]["ICPBatch"][phase][setter]):
                if e["then"] == {"absent": True}:
                    assert setter[4:] in NEW_BATCH_GETTERS and got["then"]["calls"] == [] and "returns" in got["then"]
                    e["then"] = got["then"]
                elif setter == "set_normal_rejection" and isinstance(e["then"]["returns"], float):
                    e["then"]["returns"] = f32(e["then"]["returns"])
    assert not differences(want, recorded["options"]["ICPBatch"], "ICPBatch")
    for setter, (fresh, accepted, after) in recorded["options"]["ICPBatch"]["refused"].items():
        message = ["ICPError", "icp_amd error %d: %s" % (facade_record.STATUS, facade_record.MESSAGE)]
        assert fresh["raises"] == message and after["raises"] == message and "returns" in accepted, setter
        assert after["then"] == accepted["then"] and fresh["then"]["calls"] == [], setter


def test_batch_normal_rejection_is_the_float32_the_library_holds(golden, recorded, engine):
    """Deliberate difference 1: the batch answered 0.1 as it was given; it answers what ICPStep.normal_rejection() answers."""
    i = facade_record.SETTER_CALLS["set_normal_rejection"].index(((0.1,), {}))
    assert golden["options"]["ICPBatch"]["setters"]["set_normal_rejection"][i]["then"]["returns"] == 0.1
    lib = facade_record.Library()
    batch, step = facade_record.make(engine, "ICPBatch", lib), facade_record.make(engine, "ICP", lib)
    batch.set_normal_rejection(0.1)
    lib.values = (1, 0.1)
    assert batch.normal_rejection() == step.normal_rejection() == f32(0.1) != 0.1
    facade_record.let_go(batch), facade_record.let_go(step)


def test_batch_getters_decode_what_was_set_as_the_step_decodes_the_library(engine):
    """All fifteen getters of the batch, the eight new ones among them (deliberate difference 2): after every setter call the batch answers
    what ICPStep's getter answers when the library returns the arguments that call sent, held in their C types; before any call, what
    ICPStep answers for _OPTIONS' fresh-handle values."""
    lib = facade_record.Library()
    step = facade_record.make(engine, "ICP", lib)
    for setter, calls in facade_record.SETTER_CALLS.items():
        name, batch = setter[4:], facade_record.make(engine, "ICPBatch", lib)
        types, fresh = engine._OPTIONS[name]
        lib.values = fresh
        assert getattr(batch, name)() == getattr(step, name)(), name
        for args, kwargs in calls:
            lib.take()
            try:
                getattr(batch, setter)(*args, **kwargs)
            except TypeError:
                continue
            (entry, sent), = lib.take()
            assert entry == "icp_batch_set_" + name
            lib.values = tuple(t(v).value for t, v in zip(types, sent))
            assert getattr(batch, name)() == getattr(step, name)(), (setter, args, kwargs)
        facade_record.let_go(batch)
    facade_record.let_go(step)


def test_memory_objects_are_sized_and_typed_as_before(golden, recorded, engine):
    """ICPBatch.read asks for the same bytes of every object (KeyError for SUM_W, REPS and RBC_*, and for unknown ones), a write wants the
    same number of floats in every class, and _MEM_DTYPE holds the same (dtype, columns) — as a view of _MEM."""
    assert not differences(golden["memory"], recorded["memory"], "memory")
    assert engine._MEM_DTYPE == {mem: row[:2] for mem, row in engine._MEM.items()} and len(engine._MEM) == 32
    for mem in (engine.Memory.SUM_W, engine.Memory.REPS, engine.Memory.RBC_N, engine.Memory.RBC_O, engine.Memory.RBC_PERM, engine.Memory.RBC_OWNER,
                engine.Memory.RBC_XP, 32):
        assert recorded["memory"]["batch_read"][str(mem)]["raises"][0] == "KeyError"


def test_public_surface_is_the_parents_plus_eight_batch_getters(golden, recorded, engine):
    """Every public name of ICPStep, ICP, ICPBatch, ICPPyramid and of register.py's functions keeps its signature and its docstring; the
    batch gains exactly the eight getters, and its option methods carry ICPStep's docstrings."""
    want, got = golden["surface"], recorded["surface"]
    assert [len(want[c]) for c in ("ICPStep", "ICPBatch", "ICPPyramid")] == [80, 36, 14]
    for part in ("ICPStep", "ICP", "ICPPyramid", "register"):
        assert not differences(want[part], got[part], part)
    assert sorted(set(got["ICPBatch"]) - set(want["ICPBatch"])) == NEW_BATCH_GETTERS and not set(want["ICPBatch"]) - set(got["ICPBatch"])
    options = [n for name in engine._OPTIONS for n in ("set_" + name, name)]
    for name, entry in got["ICPBatch"].items():
        if name in options:
            assert entry == want["ICPStep"][name], name                    # (signature and docstring are ICPStep's, as they were before)
        else:
            assert entry == want["ICPBatch"][name], name
    assert engine.ICPBatch.set_trimming.__doc__ == engine.ICPStep.set_trimming.__doc__ and "Trimmed ICP" in engine.ICPBatch.set_trimming.__doc__


def test_every_option_is_stated_once(engine):
    """The setters and getters are ordinary functions of _Options alone; the package's source defines each once, declares no option's
    entry point by hand and keeps no shadow attribute; ICPBatch.read has no size table of its own."""
    src = open(os.path.join(ROOT, "icp_amd", "__init__.py")).read()
    assert len(engine._OPTIONS) == 15
    for name, (types, fresh) in engine._OPTIONS.items():
        assert len(types) == len(fresh) and all(issubclass(t, C._SimpleCData) for t in types), name
        for method in ("set_" + name, name):
            assert inspect.isfunction(vars(engine._Options)[method]) and len(re.findall(r"def %s\(" % method, src)) == 1, method
            for cls in (engine.ICPStep, engine.ICP, engine.ICPBatch):
                assert getattr(cls, method) is vars(engine._Options)[method] and method not in vars(cls)
        assert not re.search(r'sig\("icp_(set|get|batch_set)_%s"' % name, src), name
        assert 'getattr(self, "_%s"' % name not in src and "self._%s =" % name not in src, name
    assert "sizes" not in inspect.getsource(engine.ICPBatch.read)


def test_options_table_against_the_header(engine):
    """For every row the header declares icp_set_<n>, icp_get_<n> and icp_batch_set_<n> with as many arguments behind the handle as the row
    has types, of those types (the getter: pointers to them); every icp_batch_set_* of the header but set_modes has a row; and the library
    was declared accordingly."""
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "icp_amd.h")).read(), flags=re.S)
    decl = {m.group(1): [a.strip() for a in m.group(2).split(",")] for m in re.finditer(r"\bint\s+(icp_\w+)\s*\(([^)]*)\)\s*;", code)}
    spelled = {C.c_int: "int", C.c_uint32: "uint32_t", C.c_float: "float"}
    L = engine.lib()
    for name, (types, _) in engine._OPTIONS.items():
        for entry, handle, star in (("icp_set_", "icp_handle", ""), ("icp_get_", "icp_handle", "*"), ("icp_batch_set_", "icp_batch_handle", "")):
            args = decl[entry + name]
            assert args[0].split()[0] == handle and len(args) == 1 + len(types), entry + name
            for a, t in zip(args[1:], types):
                assert re.fullmatch(r"%s\s*%s\s*\w+" % (spelled[t], re.escape(star)), a), (entry + name, a)
            want = [C.c_void_p] + [C.POINTER(t) if star else t for t in types]
            assert getattr(L, entry + name).argtypes == want and getattr(L, entry + name).restype is C.c_int, entry + name
    assert sorted(n[len("icp_batch_set_"):] for n in decl if n.startswith("icp_batch_set_") and n != "icp_batch_set_modes") == sorted(engine._OPTIONS)


def test_register_applies_its_options_as_before(golden, recorded):
    """register_clouds, register_and_evaluate and register_with_pairs over recording stand-ins for ICP and ICPPyramid: the same calls in
    the same order and the same return shapes for every option set — all off, all that go together, the moving-normal metrics, adaptive
    in trimming's place, a pyramid —, and main the same for whole command lines, with the same printout."""
    assert sorted(recorded["register"]["functions"]) == sorted(facade_record.REGISTER_OPTIONS)
    assert not differences(golden["register"]["functions"], recorded["register"]["functions"], "functions")
    assert not differences(golden["register"]["main runs"], recorded["register"]["main runs"], "main runs")
    on = [c[1] for c in recorded["register"]["functions"]["all on"]["register_clouds []"]["calls"] if len(c) == 4]
    assert on.index("set_normals") < on.index("set_error_metric") and on.index("set_unique") < on.index("set_median_rejection") < on.index("set_trimming")
    adaptive = [c[1] for c in recorded["register"]["main runs"][6]["calls"] if len(c) == 4]
    assert "set_adaptive_trimming" in adaptive and "set_trimming" not in adaptive


def test_main_refuses_bad_arguments_with_the_same_messages(golden, recorded):
    assert not differences(golden["register"]["main errors"], recorded["register"]["main errors"], "main errors")
    said = {" ".join(argv): text for argv, code, text in recorded["register"]["main errors"] if code == 2}
    assert len(said) == len(facade_record.MAIN_ERRORS)
    assert said["--trim 0"] == "argument --trim: must be in (0, 1], got 0" and said["--plane-to-plane 2"] == "argument --plane-to-plane: must be in (0, 1], got 2"
    assert said["--adaptive-trim 0.5"] == "argument --adaptive-trim: must be MIN:MAX[:Q], got 0.5"
    assert said["--adaptive-trim 0.9:0.1"].startswith("argument --adaptive-trim: must be MIN:MAX[:Q] with 0 < MIN <= MAX <= 1 and Q in 2 .. 8")
    assert said["--adaptive-trim 0.1:0.9 --trim 0.5"] == "--adaptive-trim and --trim exclude each other"


def test_register_functions_take_register_clouds_options_by_name(golden, recorded):
    """An option register_clouds does not have is a TypeError in all three, before anything is created."""
    assert recorded["register"]["unknown option"] == golden["register"]["unknown option"]
    assert all(v == ["TypeError", []] for v in recorded["register"]["unknown option"].values())


# -- on the device: the tables against the library ------------------------------------------------------------------------------------

ROUND_TRIPS = {          # per setter: arguments float32 does not hold, then the off spelling
    "set_rejection": [(True, 60.3), (False, None)], "set_trimming": [(0.7,), (1.0,)], "set_unique": [(True,), (False,)],
    "set_median_rejection": [(2.3,), (0,)], "set_adaptive_trimming": [(0.1, 0.9, 3), (0.0, 0.0, 0)], "set_reciprocal": [(True, 0.1), (False,)],
    "set_projective": [(16, 60.3, 0.1, 7.3, 7.7, 2), (None,)], "set_normal_rejection": [(0.1,), (None,)], "set_boundary_rejection": [(16,), (None,)],
    "set_robust_loss": [(3, 60.3), (0, 0.0)], "set_error_metric": [(1, 0.1), (0, 0.0)], "set_normals": [(1, 16), (0, 0)],
    "set_color_weight": [(0.1,), (0,)], "set_plane_to_plane": [(0.1,), (0,)], "set_symmetric": [(True,), (False,)],
}


@pytest.mark.gpu
def test_fresh_handles_hold_the_tables_values(engine):
    """A fresh ICP(0), not initialised, holds _OPTIONS' fresh-handle values in the library, and every getter answers what the getter of
    a fresh ICPBatch([0]) answers."""
    g, b = engine.ICP(0), engine.ICPBatch([0])
    for name, (_, fresh) in engine._OPTIONS.items():
        assert g._get(name) == fresh and b._get(name) == fresh, name
        assert getattr(g, name)() == getattr(b, name)(), name
    g.close(), b.close()


@pytest.mark.gpu
def test_batch_and_handle_answer_alike_after_every_setter(engine):
    assert sorted(ROUND_TRIPS) == sorted("set_" + n for n in engine._OPTIONS)
    g, b = engine.ICP(0), engine.ICPBatch([0])
    for setter, calls in ROUND_TRIPS.items():
        for args in calls:
            getattr(g, setter)(*args), getattr(b, setter)(*args)
            assert getattr(g, setter[4:])() == getattr(b, setter[4:])(), (setter, args)
    assert g.normal_rejection() is None and b.rejection() == (False, None)
    g.close(), b.close()


@pytest.mark.gpu
def test_memory_table_sizes_what_the_library_sizes(engine):
    """16 x 16 points, 4 representatives: every object _MEM sizes has icp_mem_size's bytes, and those it does not size are the
    representatives', the RBC's lists and the sum of weights."""
    g = engine.ICP(0)
    g.init(256, 4)
    sized = [mem for mem, row in engine._MEM.items() if row[2] is not None]
    assert len(sized) == 25
    for mem in sized:
        assert engine._mem_elements(mem, 256) * np.dtype(engine._MEM[mem][0]).itemsize == engine.lib().icp_mem_size(g._h, mem) > 0, mem
    g.close()


@pytest.mark.gpu
def test_a_refused_batch_setter_leaves_the_getter_alone(engine):
    b = engine.ICPBatch([0])
    b.set_trimming(0.7)
    with pytest.raises(engine.ICPError):
        b.set_trimming(0.0)
    assert b.trimming() == f32(0.7)
    with pytest.raises(engine.ICPError):
        b.set_normal_rejection(60.3)
    assert b.normal_rejection() is None
    b.close()
