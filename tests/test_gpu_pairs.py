"""The correspondence set on the device (icp_correspondences, include/icp_amd.h) against its numpy restatement (pairs_ref.py).

Expectations are built as tests/test_gpu_quality.py builds them: the oracle's search at the handle's transform gives ids, PF and PM,
pairs_ref the set.  Comparison is exact: the count, then the first `count` records by their raw bytes; records behind the count are
never read (the Python layer copies `count` records and no more)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import icp_checks as K
import pairs_ref
import quality_ref
from pairs_ref import check_set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESTATE, EINVAL = 4, 1


def search_at(oracle, F, M, T, nr):
    """(ids, PF, PM) of the oracle's search at T."""
    nn_id, _ = K.oracle_search(oracle, F, M, T, nr)
    ids = nn_id["id"].copy()
    return ids, np.ascontiguousarray(F[ids][:, :4]), np.ascontiguousarray(oracle.transform_q(M, T)[:, :4])


def expected(oracle, F, M, T, nr, max_dist):
    """(the ICP_PAIRS_EVALUATED set, the number of counted moving points) from the oracle's search at T."""
    ids, PF, PM = search_at(oracle, F, M, T, nr)
    counted, _, _ = quality_ref.masks(M, PF, PM, max_dist)
    return pairs_ref.evaluated(M, PF, PM, ids, max_dist), int(np.count_nonzero(counted))


def plain(engine, side, nr, fused=True, batch=1, it=40):
    return K.make_handle(engine, side * side, nr, fused, K.WEIGHTED, K.POWER, fused, batch, it)


def start_at(engine, g, F, M, T):
    K.load(engine, g, F, M)
    g.buildRBC()
    g.write(engine.Memory.T, T, block=True)


def last_of(engine, g, b=0):
    """pairs_ref.last_iteration of the four per-query outputs read back from registration b of g."""
    Mem = engine.Memory
    return pairs_ref.last_iteration(g.read(Mem.NN_ID, b), g.read(Mem.W, b), g.read(Mem.NN, b), g.read(Mem.QT, b))


# (side, |R|): m = 900, fewer than four blocks and a ragged last one; 2500, nblk = 10, no power of two; the latency layout; the dense layout
SHAPES = [(30, 4), (50, 4), (128, 256), (256, 1024)]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", SHAPES)
def test_evaluated_shapes(engine, oracle, side, nr, fused):
    """After 3 fixed iterations, max_dist from pick_max_dist at the handle's T: the set is the reference's, its length evaluate's n_inliers."""
    F, M = engine.synth_pair(side)
    g = plain(engine, side, nr, fused)
    K.load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed(3)
    T = g.read(engine.Memory.T).copy()
    assert g.search_layout()[0] == (1 if (side, nr) == (256, 1024) else 0)
    max_dist = K.pick_max_dist(oracle, F, M, T, nr, frac=0.3)
    want, n_counted = expected(oracle, F, M, T, nr, max_dist)
    assert 0.1 <= len(want) / n_counted <= 0.9, "the reference accepts %d of %d counted points" % (len(want), n_counted)
    got = g.correspondences(engine.Pairs.EVALUATED, max_dist)
    check_set(got, want, "side %d nr %d fused %d" % (side, nr, fused))
    assert len(got) == g.evaluate(max_dist)[0].n_inliers
    g.close()


def test_empty_blocks_and_waves(engine, oracle):
    """Holes punched into M at side 50 (blocks of 256 pairs, waves of 64): rows 0:256 — the first block is empty; 512:1024 — two middle
    blocks; 1100:1164 — a run of 64 inside block 4 that straddles two of its waves; and 1536:1600, the first wave of block 6, which
    leaves one whole wave empty.  No distance test.  The expectation has members on both sides of every gap (the first has only a far
    side)."""
    side, nr = 50, 4
    gaps = [(0, 256), (512, 1024), (1100, 1164), (1536, 1600)]
    F, M = engine.synth_pair(side)
    M = M.copy()
    for a, b in gaps:
        M[a:b, :3] = 0.0
    T = K._t0()
    want, _ = expected(oracle, F, M, T, nr, 0.0)
    member = np.zeros(side * side, bool)
    member[want["moving"]] = True
    for a, b in gaps:
        assert not member[a:b].any() and member[b] and (a == 0 or member[a - 1]), (a, b)
    assert member[256:512].all() and member[1024:1100].all() and member[1164:1536].all()
    g = plain(engine, side, nr)
    start_at(engine, g, F, M, T)
    check_set(g.correspondences(engine.Pairs.EVALUATED, 0.0), want, "holes in M")
    assert len(want) == g.evaluate(0.0)[0].n_inliers
    g.close()


def _batch_pairs(engine, side):
    return [engine.synth_pair(side, seed=s, rot_deg=r, t=t) for s, r, t in
            ((0x51, 3.0, (25.0, -10.0, 15.0)), (0x52, 2.8, (24.0, -9.0, 14.0)), (0x53, 3.2, (26.0, -11.0, 16.0)))]


def test_batch_of_three(engine, oracle):
    """One launch set, three sets: each the reference's at that registration's own T, with one max_dist (registration 0's) for all; a
    second call at a micrometre; icp_batch_correspondences on an ICPBatch of 3 gives the same bytes."""
    side, nr = 30, 4
    m = side * side
    pairs = _batch_pairs(engine, side)
    g = plain(engine, side, nr, batch=3)
    for b, (F, M) in enumerate(pairs):
        K.load(engine, g, F, M, b)
    g.buildRBC()
    g.run_fixed(3)
    Ts = [g.read(engine.Memory.T, b).copy() for b in range(3)]
    max_dist = K.pick_max_dist(oracle, pairs[0][0], pairs[0][1], Ts[0], nr, frac=0.3)
    wants = [expected(oracle, F, M, Ts[b], nr, max_dist)[0] for b, (F, M) in enumerate(pairs)]
    assert len({len(w) for w in wants}) == 3, [len(w) for w in wants]
    L = engine.lib()
    counts = (C.c_uint32 * 3)()
    assert L.icp_correspondences(g._h, engine.Pairs.EVALUATED, max_dist, counts, 3) == 0
    assert list(counts) == [len(w) for w in wants]
    sets = [g.correspondences_read(b) for b in range(3)]
    for b in range(3):
        check_set(sets[b], wants[b], "registration %d" % b)
    two = (C.c_uint32 * 2)(7, 7)
    assert L.icp_correspondences(g._h, engine.Pairs.EVALUATED, max_dist, two, 1) == 0 and list(two) == [len(wants[0]), 7]
    B = engine.ICPBatch([0])
    B.init(3, m, nr, K.A, K.C_)
    B.set_modes(engine.ReduceMode.FUSED, engine.PowerMode.SQUARED)
    for b, (F, M) in enumerate(pairs):
        B.write(b, engine.Memory.F, F); B.write(b, engine.Memory.M, M)
    B.buildRBC()
    B.run_fixed(3, True)
    for b in range(3):
        K.assert_bits(B.read(b, engine.Memory.T), Ts[b], "T of registration %d" % b)
        assert B.correspondences(b, engine.Pairs.EVALUATED, max_dist).tobytes() == sets[b].tobytes(), b
    B.close()
    # a micrometre: the expectation is computed, not assumed
    tiny = [expected(oracle, F, M, Ts[b], nr, 1e-6)[0] for b, (F, M) in enumerate(pairs)]
    assert L.icp_correspondences(g._h, engine.Pairs.EVALUATED, 1e-6, counts, 3) == 0
    assert list(counts) == [len(w) for w in tiny]
    for b in range(3):
        n = C.c_uint32(99)
        if len(tiny[b]) == 0:
            assert L.icp_correspondences_read(g._h, b, None, 0, C.byref(n)) == 0 and n.value == 0
        check_set(g.correspondences_read(b), tiny[b], "registration %d at a micrometre" % b)
    print("a micrometre:", [len(w) for w in tiny])
    g.close()


def _outputs(engine, g):
    Mem = engine.Memory
    return {n: g.read(getattr(Mem, n)).copy() for n in ("T", "S", "NN_ID", "W", "NN", "QT")}


def _same(a, b, what):
    for n in a:
        x, y = a[n], b[n]
        if n == "NN_ID":
            assert np.array_equal(x["id"], y["id"]), "%s: ids" % what
            x, y = x["dist"], y["dist"]
        K.assert_bits(x, y, "%s: %s" % (what, n))


def _raw(q):
    return C.string_at(C.addressof(q), C.sizeof(q))


def test_disturbs_nothing(engine):
    """Two identical handles; one asks for both sets between run_fixed (2) and a further step: T, the four per-query outputs and S are
    equal by bits afterwards, evaluate's record has the same bytes before and after.  Then a checked run with lazy outputs: EVALUATED
    leaves them reproducible."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    a, b = plain(engine, side, nr), plain(engine, side, nr)
    for g in (a, b):
        K.load(engine, g, F, M)
        g.buildRBC()
        g.run_fixed(2)
    before = _outputs(engine, a)
    q0 = _raw(a.evaluate(20.0)[0])
    ev = a.correspondences(engine.Pairs.EVALUATED, 20.0)
    last = a.correspondences(engine.Pairs.LAST_ITERATION)
    assert 0 < len(ev) <= side * side and 0 < len(last) <= side * side
    assert _raw(a.evaluate(20.0)[0]) == q0
    _same(_outputs(engine, a), before, "outputs behind the two sets")
    a.step(); b.step()
    _same(_outputs(engine, a), _outputs(engine, b), "run_fixed, correspondences, step")
    assert a.state().k == b.state().k == 3
    ka, kb = a.run(), b.run()
    assert ka == kb
    assert len(a.correspondences(engine.Pairs.EVALUATED, 10.0)) == a.evaluate(10.0)[0].n_inliers
    _same(_outputs(engine, a), _outputs(engine, b), "lazy outputs behind the evaluated set")
    a.close(); b.close()


@pytest.mark.parametrize("rule", ["trimming", "one-to-one"])
def test_last_iteration_shows_the_rules(engine, rule):
    """One WEIGHTED step at side 128 on the holes pair with ICP_REJECT_INVALID and trimming 0.75 / one-to-one: the count is the rule's
    own (ICP_MEM_TRIM's accepted, ICP_MEM_UNIQUE's winners), the set pairs_ref's of the four arrays read back from the handle."""
    side, nr = 128, 256
    m = side * side
    F, M = K.holes_pair(engine, side, 0x1C9D5EED)
    opts = dict(trimming=0.75) if rule == "trimming" else dict(unique=True)
    g = K.make_handle(engine, m, nr, True, K.WEIGHTED, K.POWER, True, rejection=(True, None), **opts)
    K.one_step(engine, g, F, M, K._t0())
    got = g.correspondences(engine.Pairs.LAST_ITERATION)
    words = g.read(engine.Memory.TRIM if rule == "trimming" else engine.Memory.UNIQUE)
    assert len(got) == int(words[3] if rule == "trimming" else words[1]), (len(got), words)
    assert 0 < len(got) < m
    want = last_of(engine, g)
    check_set(got, want, rule)
    assert len(np.unique(got["weight"])) > 100 and not (got["weight"] == 1).any()       # (WEIGHTED: the weights carry non-trivial bits)
    if rule == "one-to-one":
        assert len(np.unique(got["fixed"])) == len(got)
    g.close()


def test_last_iteration_at_the_largest_size(engine):
    """m = 2^20, the largest icp_init accepts: nblk = 4096, every thread of the last block sums 16 block counts.  One step with
    trimming 0.75; the set is pairs_ref's of the arrays read back, its length ICP_MEM_TRIM's accepted."""
    side, nr = 1024, 4096
    m = side * side
    F, M = engine.synth_pair(side)
    g = K.make_handle(engine, m, nr, True, K.WEIGHTED, K.POWER, True, trimming=0.75)
    K.one_step(engine, g, F, M, K._t0())
    got = g.correspondences(engine.Pairs.LAST_ITERATION)
    want = last_of(engine, g)
    assert m // 2 < len(want) < m and len(want) == int(g.read(engine.Memory.TRIM)[3])
    check_set(got, want, "2^20")
    g.close()


def test_last_iteration_behind_a_lazy_run(engine):
    """After a checked run with lazy outputs the set is the one built from the arrays a twin handle reads; after the same run followed
    by a write of F the call returns ICP_ESTATE, as icp_read (ICP_MEM_W) does; max_dist != 0 is refused."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    a, b, c = (plain(engine, side, nr) for _ in range(3))
    ks = []
    for g in (a, b, c):
        K.load(engine, g, F, M)
        g.buildRBC()
        ks.append(g.run())
    assert ks[0] == ks[1] == ks[2] > 1
    got = a.correspondences(engine.Pairs.LAST_ITERATION)
    check_set(got, last_of(engine, b), "behind icp_run")
    assert len(got) == side * side
    check_set(got, last_of(engine, a), "the handle's own arrays")
    c.write(engine.Memory.F, F)
    with pytest.raises(engine.ICPError) as e:
        c.read(engine.Memory.W)
    assert e.value.code == ESTATE
    with pytest.raises(engine.ICPError) as e:
        c.correspondences(engine.Pairs.LAST_ITERATION)
    assert e.value.code == ESTATE
    with pytest.raises(engine.ICPError) as e:
        a.correspondences(engine.Pairs.LAST_ITERATION, 5.0)
    assert e.value.code == EINVAL
    for g in (a, b, c):
        g.close()


def test_arguments_and_states(engine):
    side, nr = 30, 4
    F, M = engine.synth_pair(side)
    L = engine.lib()
    g = plain(engine, side, nr, batch=2)
    counts = (C.c_uint32 * 4)()
    n = C.c_uint32()
    buf = np.empty(side * side, pairs_ref.PAIR)

    def rc(*a):
        return L.icp_correspondences(g._h, *a)

    for b in range(2):
        K.load(engine, g, F, M, b)
    assert rc(0, 0.0, counts, 1) == ESTATE and b"icp_build_rbc" in L.icp_last_error(g._h)       # before icp_build_rbc
    assert rc(1, 0.0, counts, 1) == ESTATE
    g.buildRBC()
    assert L.icp_correspondences_read(g._h, 0, buf.ctypes.data, len(buf), C.byref(n)) == ESTATE   # no set yet
    assert L.icp_correspondences_device_ptr(g._h, 0, None, None) == ESTATE
    assert rc(2, 0.0, counts, 1) == EINVAL and rc(-1, 0.0, counts, 1) == EINVAL                   # a bad source
    assert rc(0, 0.0, counts, 3) == EINVAL and rc(0, 0.0, counts, 0) == EINVAL                    # count above the batch, count 0
    assert rc(0, 0.0, None, 1) == EINVAL
    assert rc(0, -1.0, counts, 1) == EINVAL and rc(0, float("nan"), counts, 1) == EINVAL
    assert rc(1, 1.0, counts, 1) == EINVAL
    assert L.icp_correspondences_read(g._h, 0, buf.ctypes.data, len(buf), C.byref(n)) == ESTATE   # (refused calls computed none)
    assert rc(0, float("inf"), counts, 2) == 0 and counts[0] == counts[1] == side * side          # (no distance test)
    count = counts[0]
    assert L.icp_correspondences_read(g._h, 1, buf.ctypes.data, count - 1, C.byref(n)) == EINVAL and n.value == count
    assert L.icp_correspondences_read(g._h, 2, buf.ctypes.data, len(buf), C.byref(n)) == EINVAL
    assert L.icp_correspondences_read(g._h, 1, buf.ctypes.data, count, C.byref(n)) == 0 and n.value == count
    assert np.array_equal(buf["moving"][:count], np.arange(count))
    rec, word = C.c_void_p(), C.c_void_p()
    assert L.icp_correspondences_device_ptr(g._h, 1, C.byref(rec), C.byref(word)) == 0 and rec.value and word.value
    rec0 = C.c_void_p()
    assert L.icp_correspondences_device_ptr(g._h, 0, C.byref(rec0), None) == 0 and rec.value - rec0.value == 16 * side * side
    with pytest.raises(engine.ICPError) as e:
        g.correspondences(7)
    assert e.value.code == EINVAL
    g.init(side * side, nr, K.A, K.C_, batch=2)                                                   # a new init: the set is gone
    assert L.icp_correspondences_read(g._h, 0, buf.ctypes.data, len(buf), C.byref(n)) == ESTATE
    g.close()


def test_pyramid_level_inherits_it(engine):
    """The borrowed handle of a pyramid's level 0: the set of a plain handle at the same F, M and T, by bytes."""
    side, nr = 64, 64
    F, M = engine.synth_pair(side)
    p = engine.ICPPyramid(0)
    p.init(side * side, [nr, nr], K.A, K.C_)
    p.write(engine.Memory.F, F); p.write(engine.Memory.M, M)
    p.buildRBC()
    p.run()
    lv = p.level(0)
    T = lv.read(engine.Memory.T).copy()
    got = lv.correspondences(engine.Pairs.EVALUATED, 3.0)
    assert len(got) == lv.evaluate(3.0)[0].n_inliers and 0 < len(got) < side * side
    assert len(lv.correspondences(engine.Pairs.LAST_ITERATION)) == side * side
    g = plain(engine, side, nr)
    start_at(engine, g, F, M, T)
    check_set(got, g.correspondences(engine.Pairs.EVALUATED, 3.0), "level 0 against a plain handle")
    g.close()
    p.close()


def test_command_line_writes_the_set(engine, tmp_path, capsys):
    """`python -m icp_amd.register --evaluate 10 --pairs FILE` (in process) on a pair of 640 x 480 clouds: the file holds the evaluated
    set of register_with_pairs, its length is the printed count and the printed inlier count."""
    import re
    from icp_amd import register
    cloud_f, cloud_m = engine.synth_cloud_vga(moved=False), engine.synth_cloud_vga(moved=True)
    pf, pm, out = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "pairs.npy"
    cloud_f.astype("<f4").tofile(pf)
    cloud_m.astype("<f4").tofile(pm)
    register.main([str(pf), str(pm), "--evaluate", "10", "--pairs", str(out)])
    text = capsys.readouterr().out
    got = np.load(out)
    assert got.dtype == pairs_ref.PAIR and 0 < len(got) < 16384
    assert int(re.search(r"Correspondences\s+:\s+(\d+)", text).group(1)) == len(got)
    assert int(re.search(r"Inliers\s+:\s+(\d+) of", text).group(1)) == len(got)
    assert (np.diff(got["moving"].astype(np.int64)) > 0).all() and (got["fixed"] < 16384).all() and (got["weight"] == 1).all()
    assert (got["geo"] <= np.float32(100.0)).all()
    _, _, _, _, quality, members = register.register_with_pairs(cloud_f, cloud_m, 10.0)
    assert members.tobytes() == got.tobytes() and quality.n_inliers == len(got)
    assert len(register.register_with_pairs(cloud_f, cloud_m)[5]) >= len(got)                    # (no distance test)


def _fnv1a(data):
    h = 14695981039346656037
    for byte in data:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_facade_program(engine):
    """tests/cpp/pairs_facade_test.cpp (built by build ()): cl_algo::ICP::ICP::correspondences () on a registration run through the
    facade gives the count and the checksum of this module's own call on the same data."""
    exe = os.path.join(ROOT, "tests", "cpp", "pairs_facade_test")
    assert os.path.exists(exe), "tests/cpp/pairs_facade_test is built by build() / make pairs_facade_test"
    side, nr, max_dist = 64, 64, 3.0
    out = subprocess.run([exe, str(side), str(nr), "%g" % max_dist], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = dict(l.split(None, 1) for l in out.stdout.splitlines())
    F, M = engine.synth_pair(side)
    g = plain(engine, side, nr)
    K.load(engine, g, F, M)
    g.buildRBC()
    k = g.run()
    ev = g.correspondences(engine.Pairs.EVALUATED, max_dist)
    last = g.correspondences(engine.Pairs.LAST_ITERATION)
    assert int(lines["k"]) == k
    n, h, _, inl = lines["EVALUATED"].split()
    assert (int(n), int(h, 16)) == (len(ev), _fnv1a(ev.tobytes())) and int(inl) == len(ev)
    assert 0 < len(ev) < side * side
    n, h = lines["LAST"].split()
    assert (int(n), int(h, 16)) == (len(last), _fnv1a(last.tobytes())) and len(last) == side * side
    g.close()
