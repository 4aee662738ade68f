"""Registration quality on the device (icp_evaluate, include/icp_amd.h) against its numpy restatement (quality_ref.py).

The expectation is always built the same way: the oracle's search at the handle's transform gives the correspondences, quality_ref the
numbers; the 22 sums are compared by their raw bits, the three counts exactly, fitness and the inlier RMSE within 1 ulp of the host
formula.  Every case proves on the expectation alone that the rule has pairs to accept and pairs to refuse."""
import ctypes as C

import numpy as np
import pytest

import icp_checks as K
import quality_ref
import robust_ref
from quality_ref import check_record

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = 4, 1


def raw(q):
    return C.string_at(C.addressof(q), C.sizeof(q))


def expected(oracle, F, M, T, nr, max_dist):
    """(quality_ref.Quality, PF, PM) from the oracle's search at T."""
    nn_id, _ = K.oracle_search(oracle, F, M, T, nr)
    PF = np.ascontiguousarray(F[nn_id["id"]][:, :4])
    PM = np.ascontiguousarray(oracle.transform_q(M, T)[:, :4])
    return quality_ref.evaluate(M, PF, PM, max_dist), PF, PM


def non_trivial(want, what):
    share = want.n_inliers / want.n_moving
    assert 0.1 <= share <= 0.9, "%s: the reference accepts %d of %d counted points" % (what, want.n_inliers, want.n_moving)


def plain(engine, side, nr, fused=True, batch=1, it=40):
    return K.make_handle(engine, side * side, nr, fused, K.WEIGHTED, K.POWER, fused, batch, it)


def start_at(engine, g, F, M, T, b=0):
    g.write(engine.Memory.F, F, batch_index=b); g.write(engine.Memory.M, M, batch_index=b)
    g.buildRBC()
    g.write(engine.Memory.T, T, block=True, batch_index=b)


# (side, |R|): m = 900, fewer than four blocks; 2500, no multiple of 256 (the padded second tree); the latency layout; the dense layout
SHAPES = [(30, 4), (50, 4), (128, 256), (256, 1024)]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("side,nr", SHAPES)
def test_shapes(engine, oracle, side, nr, fused):
    """After 3 fixed iterations, max_dist from pick_max_dist at the handle's final T."""
    m = side * side
    F, M = engine.synth_pair(side)
    g = plain(engine, side, nr, fused)
    K.load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed(3)
    T = g.read(engine.Memory.T).copy()
    assert g.state().k == 3
    assert g.search_layout()[0] == (1 if (side, nr) == (256, 1024) else 0)
    max_dist = K.pick_max_dist(oracle, F, M, T, nr, frac=0.3)
    want, _, _ = expected(oracle, F, M, T, nr, max_dist)
    non_trivial(want, "side %d" % side)
    check_record(g.evaluate(max_dist)[0], want, m, "side %d nr %d fused %d" % (side, nr, fused))
    g.close()


def test_no_distance_test(engine, oracle):
    """max_dist = 0 (and None, and +inf): every pair with two valid endpoints and a finite distance is an inlier."""
    side, nr = 50, 4
    F, M = engine.synth_pair(side)
    g = plain(engine, side, nr)
    K.load(engine, g, F, M)
    g.buildRBC()
    g.run_fixed(3)
    T = g.read(engine.Memory.T).copy()
    want, _, _ = expected(oracle, F, M, T, nr, 0.0)
    assert want.n_inliers == want.n_moving == side * side
    q = g.evaluate(0.0)[0]
    check_record(q, want, side * side, "max_dist 0")
    assert q.fitness == 1.0
    assert raw(g.evaluate(None)[0]) == raw(q) and raw(g.evaluate(float("inf"))[0]) == raw(q)
    g.close()


def test_holes(engine, oracle):
    """Invalid moving points are not in n_moving; pairs that land on an invalid fixed point are no inliers.  The scene's valid points
    lie a metre from the origin and never meet a hole of F, so five of M's holes are moved a millimetre off the origin: they count, their
    nearest fixed points are holes a few mm away — well inside max_dist —, and only the rule about f keeps them out."""
    side, nr = 128, 256
    m = side * side
    F, M = K.holes_pair(engine, side, 0x1C9D5EED)
    M = M.copy()
    near = np.nonzero((M[:, :3] == 0).all(axis=1))[0][::97][:5]
    M[near, :3] = np.array([[1.0, 0.5, -0.5], [-1.0, 0.25, 0.5], [0.5, 1.0, 1.0], [0.25, -1.0, 0.5], [1.0, 1.0, -1.0]], np.float32)
    T = K._t0()
    g = K.make_handle(engine, m, nr, True, K.WEIGHTED, K.POWER, True, rejection=(True, None))
    start_at(engine, g, F, M, T)
    max_dist = K.pick_max_dist(oracle, F, M, T, nr, frac=0.3)
    want, PF, _ = expected(oracle, F, M, T, nr, max_dist)
    assert m / 2 < want.n_moving < m, want.n_moving
    on_hole = want.counted & (PF[:, :3] == 0).all(axis=1)
    assert on_hole[near].all() and not want.inlier[on_hole].any(), np.count_nonzero(on_hole)
    assert (want.geo[near] <= quality_ref.threshold(max_dist)[1]).all(), (want.geo[near], max_dist)
    non_trivial(want, "holes")
    check_record(g.evaluate(max_dist)[0], want, m, "holes")
    g.close()


def test_edge_of_the_rule(engine, oracle):
    """A max_dist whose (float) (max_dist^2) equals one pair's geo bit for bit makes that pair an inlier; the next float down makes
    it none."""
    side, nr = 50, 4
    m = side * side
    F, M = engine.synth_pair(side)
    T = K._t0()
    g = plain(engine, side, nr)
    start_at(engine, g, F, M, T)
    base, PF, PM = expected(oracle, F, M, T, nr, 0.0)
    geo = base.geo
    order = np.argsort(geo)
    pick = None
    for j in order[m // 3: 2 * m // 3]:                  # (a pair in the middle of the distribution: both sides of the edge are populated)
        s = np.float32(np.sqrt(np.float64(geo[j])))
        for md in (np.nextafter(s, np.float32(0)), s, np.nextafter(s, np.float32(np.inf))):
            if quality_ref.threshold(md)[1].view(np.uint32) == geo[j].view(np.uint32):
                pick = (int(j), np.float32(md))
                break
        if pick:
            break
    assert pick is not None
    j, md = pick
    below = np.nextafter(md, np.float32(0))
    assert quality_ref.threshold(below)[1] < geo[j]
    at = quality_ref.evaluate(M, PF, PM, float(md))
    under = quality_ref.evaluate(M, PF, PM, float(below))
    assert at.inlier[j] and not under.inlier[j] and at.n_inliers > under.n_inliers
    non_trivial(at, "edge")
    non_trivial(under, "edge, one float down")
    qa, qu = g.evaluate(float(md))[0], g.evaluate(float(below))[0]
    check_record(qa, at, m, "edge")
    check_record(qu, under, m, "edge, one float down")
    assert qa.n_inliers > qu.n_inliers
    g.close()


def test_nan_in_a_moving_point(engine, oracle):
    """A NaN coordinate in one row of M: no NaN in any output, and the counts drop by that pair."""
    side, nr = 50, 4
    m = side * side
    F, M = engine.synth_pair(side)
    T = K._t0()
    max_dist = K.pick_max_dist(oracle, F, M, T, nr, frac=0.3)
    clean, _, _ = expected(oracle, F, M, T, nr, max_dist)
    non_trivial(clean, "clean")
    j = int(np.nonzero(clean.inlier)[0][clean.n_inliers // 2])
    Mn = M.copy()
    Mn[j, 1] = np.nan
    want, _, _ = expected(oracle, F, Mn, T, nr, max_dist)
    assert (want.n_moving, want.n_inliers) == (clean.n_moving - 1, clean.n_inliers - 1)
    g = plain(engine, side, nr)
    start_at(engine, g, F, Mn, T)
    q = g.evaluate(max_dist)[0]
    check_record(q, want, m, "NaN")
    out = np.array([q.fitness, q.inlier_rmse, q.sum_geo] + list(q.information))
    assert np.isfinite(out).all()
    g.close()


def _batch_pairs(engine, side):
    return [engine.synth_pair(side, seed=s, rot_deg=r, t=t) for s, r, t in
            ((0x51, 3.0, (25.0, -10.0, 15.0)), (0x52, 2.8, (24.0, -9.0, 14.0)), (0x53, 3.2, (26.0, -11.0, 16.0)))]


def test_batch_of_three(engine, oracle):
    """One call, three records, each the single handle's and the reference's; icp_batch_evaluate gives the same records."""
    side, nr = 50, 4
    m = side * side
    pairs = _batch_pairs(engine, side)
    g = plain(engine, side, nr, batch=3)
    for b, (F, M) in enumerate(pairs):
        K.load(engine, g, F, M, b)
    g.buildRBC()
    g.run_fixed(3)
    max_dist = K.pick_max_dist(oracle, pairs[0][0], pairs[0][1], g.read(engine.Memory.T, 0).copy(), nr, frac=0.5)   # (one distance for all three)
    recs = g.evaluate(max_dist)
    assert len(recs) == 3 and len(g.evaluate(max_dist, count=2)) == 2
    assert raw(g.evaluate(max_dist, count=2)[1]) == raw(recs[1])
    B = engine.ICPBatch([0])
    B.init(3, m, nr, K.A, K.C_)
    B.set_modes(engine.ReduceMode.FUSED, engine.PowerMode.SQUARED)
    for b, (F, M) in enumerate(pairs):
        B.write(b, engine.Memory.F, F); B.write(b, engine.Memory.M, M)
    B.buildRBC()
    B.run_fixed(3, True)
    for b, (F, M) in enumerate(pairs):
        s = plain(engine, side, nr)
        K.load(engine, s, F, M)
        s.buildRBC()
        s.run_fixed(3)
        T = s.read(engine.Memory.T).copy()
        K.assert_bits(g.read(engine.Memory.T, b), T, "T of registration %d" % b)
        want, _, _ = expected(oracle, F, M, T, nr, max_dist)
        non_trivial(want, "registration %d" % b)
        single = s.evaluate(max_dist)[0]
        check_record(single, want, m, "single handle %d" % b)
        assert raw(recs[b]) == raw(single), b
        assert raw(B.evaluate(b, max_dist)) == raw(single), b
        s.close()
    assert len({raw(r) for r in recs}) == 3
    B.close()
    g.close()


def test_independent_of_the_handles_settings(engine, oracle):
    """The same T written into handles with trimming, one-to-one, Tukey, point-to-plane and REGULAR weighting: the records are
    bit-identical to the plain handle's."""
    side, nr = 50, 4
    m = side * side
    F, M = engine.synth_pair(side)
    T = K._t0()
    max_dist = K.pick_max_dist(oracle, F, M, T, nr, frac=0.3)
    want, _, _ = expected(oracle, F, M, T, nr, max_dist)
    non_trivial(want, "settings")
    g = plain(engine, side, nr)
    start_at(engine, g, F, M, T)
    ref = g.evaluate(max_dist)[0]
    check_record(ref, want, m, "plain")
    g.close()
    handles = {
        "trimming": lambda: K.make_handle(engine, m, nr, True, K.WEIGHTED, K.POWER, True, trimming=0.7),
        "one-to-one": lambda: K.make_handle(engine, m, nr, True, K.WEIGHTED, K.POWER, True, unique=True),
        "Tukey": lambda: K.make_handle(engine, m, nr, True, K.WEIGHTED, K.POWER, True, robust_loss=(robust_ref.TUKEY, 30.0)),
        "rejection": lambda: K.make_handle(engine, m, nr, False, K.WEIGHTED, K.POWER, False, rejection=(True, 3.0), boundary=side),
        "point-to-plane": lambda: K.make_plane(engine, side, nr),
        "REGULAR": lambda: K.make_handle(engine, m, nr, True, K.REGULAR, K.EIGEN, True),
    }
    for name, make in handles.items():
        h = make()
        start_at(engine, h, F, M, T)
        assert raw(h.evaluate(max_dist)[0]) == raw(ref), name
        h.step()                                         # (and behind an iteration of the handle's own kind, at T again)
        h.write(engine.Memory.T, T, block=True)
        assert raw(h.evaluate(max_dist)[0]) == raw(ref), name + ", after a step"
        h.close()


def _outputs(engine, g):
    Mem = engine.Memory
    return {n: g.read(getattr(Mem, n)).copy() for n in ("T", "R", "S", "TK", "NN_ID", "RID", "NN", "QT", "W")}


def _same(a, b, what):
    for n in a:
        x, y = a[n], b[n]
        if n == "NN_ID":
            assert np.array_equal(x["id"], y["id"]), "%s: ids" % what
            x, y = x["dist"], y["dist"]
        K.assert_bits(x, y, "%s: %s" % (what, n))


# chained (fused, the latency-bound size), separate (fused, the dense size), reference order
FORMS = [("chained", 128, 256, True, 1), ("separate", 256, 1024, True, 0), ("reference-order", 128, 256, False, 0)]


@pytest.mark.parametrize("name,side,nr,fused,form", FORMS)
def test_disturbs_nothing_between_iterations(engine, name, side, nr, fused, form):
    """step, evaluate, step leaves the bits of step, step — state and all five per-query outputs —, the same for two fixed runs (the
    chained form's launches), and the evaluation in between leaves the outputs of the iteration before it as they were."""
    F, M = engine.synth_pair(side)
    a, b = plain(engine, side, nr, fused), plain(engine, side, nr, fused)
    for g in (a, b):
        K.load(engine, g, F, M)
        g.buildRBC()
        assert g.run_form() == form
    lpi = a.launches_per_iteration()
    a.step(); b.step()
    before = _outputs(engine, a)
    q1 = a.evaluate(20.0)[0]
    _same(_outputs(engine, a), before, name + ": outputs behind an evaluation")
    assert a.evaluate(0.5)[0].n_inliers < q1.n_inliers
    a.step(); b.step()
    _same(_outputs(engine, a), _outputs(engine, b), name + ": step, evaluate, step")
    a.run_fixed(2); b.run_fixed(2)
    a.evaluate(20.0)
    a.run_fixed(2); b.run_fixed(2)
    _same(_outputs(engine, a), _outputs(engine, b), name + ": run_fixed, evaluate, run_fixed")
    assert a.state().k == b.state().k == 6
    assert (a.run_form(), a.launches_per_iteration()) == (form, lpi)
    a.close(); b.close()


def test_disturbs_no_lazy_outputs(engine, oracle):
    """After icp_run with lazy outputs: evaluate, then read — the outputs equal those of a twin that never evaluated, and a fresh
    registration behind the evaluation ends where the twin's ends."""
    side, nr = 128, 256
    F, M = engine.synth_pair(side)
    a, b = plain(engine, side, nr), plain(engine, side, nr)
    for g in (a, b):
        K.load(engine, g, F, M)
        g.buildRBC()
    ka, kb = a.run(), b.run()
    assert ka == kb and ka > 1
    q = a.evaluate(10.0)[0]
    assert q.n_moving == side * side and 0 < q.n_inliers
    # the headline use — icp_run, then evaluate — against the reference at the transform the run ended with (the twin's read-back T)
    T = b.read(engine.Memory.T).copy()
    max_dist = K.pick_max_dist(oracle, F, M, T, nr, frac=0.3)
    want, _, _ = expected(oracle, F, M, T, nr, max_dist)
    non_trivial(want, "behind icp_run")
    check_record(a.evaluate(max_dist)[0], want, side * side, "behind icp_run")
    _same(_outputs(engine, a), _outputs(engine, b), "lazy outputs behind an evaluation")
    assert raw(a.evaluate(10.0)[0]) == raw(q)
    for g in (a, b):                                     # a fresh registration behind the evaluation
        g.reset_transform()
        g.buildRBC()
    assert a.run() == b.run() == ka
    a.evaluate(10.0)
    _same(_outputs(engine, a), _outputs(engine, b), "a second registration")
    a.close(); b.close()


def _rot_of(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_meaning(engine):
    """At the ground truth of a noise-free pair every point has its partner: fitness is 1 at max_dist = 5 mm and the RMSE is below
    0.1 mm.  With T the identity and the frames 30 mm apart, fitness at 5 mm is below that at 50 mm.

    The first statement needs a pair in which a partner exists.  icp_synth_pair_scene samples its moving frame half a grid cell away
    from the fixed one (a second exposure sees other surface points), so at its own T_true8 the nearest fixed point of a moving point is
    about half a cell's diagonal away whatever the transform: at side 64 the device reports fitness 0 at 5 mm for it (0 of 4096; the
    figures of that pair are printed).  The bounds are therefore asserted on the scene's fixed frame and T_true8 with the moving frame
    made of the same surface points: M = T_true8^-1 (F) in float64, rounded to float."""
    side, nr = 64, 64
    F, Ms, T_true = engine.synth_pair_scene(side, noise_mm=0.0, noise_rgb=0.0)
    Rq, tt = _rot_of(T_true[:4]), T_true[4:7].astype(np.float64)
    M = F.copy()
    M[:, :3] = ((F[:, :3].astype(np.float64) - tt) @ Rq).astype(np.float32)          # (P = Rq M + tt  =>  M = Rq^T (P - tt))
    g = plain(engine, side, nr)
    start_at(engine, g, F, M, T_true)
    q = g.evaluate(5.0)[0]
    print("ground truth, the same surface points", q.fitness, q.inlier_rmse, q.n_inliers, q.n_moving)
    assert q.fitness == 1.0 and q.n_inliers == q.n_moving == side * side
    assert q.inlier_rmse < 0.1
    A = q.information_matrix()
    assert np.array_equal(A, A.T) and (np.linalg.eigvalsh(A) > 0).all() and A[3, 3] == A[4, 4] == A[5, 5] == side * side
    start_at(engine, g, F, Ms, T_true)
    for d in (5.0, 15.0, 50.0):
        qs = g.evaluate(d)[0]
        print("ground truth, the scene's own moving frame, max_dist", d, qs.fitness, qs.inlier_rmse, qs.n_inliers, qs.n_moving)
    g.close()
    F, M, _ = engine.synth_pair_scene(side, rot_deg=0.0, t=(30.0, 0.0, 0.0), noise_mm=0.0, noise_rgb=0.0)
    g = plain(engine, side, nr)
    K.load(engine, g, F, M)
    g.buildRBC()
    near, far = g.evaluate(5.0)[0], g.evaluate(50.0)[0]
    print("30 mm apart", near.fitness, far.fitness)
    assert near.fitness < far.fitness
    g.close()


def test_arguments_and_states(engine):
    side, nr = 30, 4
    F, M = engine.synth_pair(side)
    L = engine.lib()
    g = plain(engine, side, nr, batch=2)
    out = (engine.Quality * 4)()

    def rc(*a):
        return L.icp_evaluate(g._h, *a)

    for b in range(2):
        K.load(engine, g, F, M, b)
    assert rc(0.0, out, 1) == ESTATE and b"icp_build_rbc" in L.icp_last_error(g._h)          # before icp_build_rbc
    g.buildRBC()
    assert rc(0.0, out, 1) == 0 and rc(0.0, out, 2) == 0
    assert rc(0.0, None, 1) == EINVAL
    assert rc(0.0, out, 0) == EINVAL
    assert rc(0.0, out, 3) == EINVAL
    assert rc(-1.0, out, 1) == EINVAL
    assert rc(float("nan"), out, 1) == EINVAL
    assert L.icp_evaluate(None, 0.0, out, 1) == EINVAL
    with pytest.raises(engine.ICPError) as e:
        g.evaluate(-0.5)
    assert e.value.code == EINVAL
    assert rc(float("inf"), out, 2) == 0                                                          # (no distance test)
    g.init(side * side, nr, K.A, K.C_)                                                            # a new init: not built again
    assert L.icp_evaluate(g._h, 0.0, out, 1) == ESTATE
    g.close()
    B = engine.ICPBatch([0])
    q = engine.Quality()
    assert L.icp_batch_evaluate(B._b, 0, 0.0, C.byref(q)) == ESTATE                               # before icp_batch_init
    B.init(2, side * side, nr, K.A, K.C_)
    assert L.icp_batch_evaluate(B._b, 0, 0.0, C.byref(q)) == ESTATE                               # before the RBC
    for b in range(2):
        B.write(b, engine.Memory.F, F); B.write(b, engine.Memory.M, M)
    B.buildRBC()
    assert L.icp_batch_evaluate(B._b, 1, 0.0, C.byref(q)) == 0 and q.n_moving == side * side
    assert L.icp_batch_evaluate(B._b, 2, 0.0, C.byref(q)) == EINVAL
    assert L.icp_batch_evaluate(B._b, 0, 0.0, None) == EINVAL
    assert L.icp_batch_evaluate(B._b, 0, -1.0, C.byref(q)) == EINVAL
    B.close()


def test_tracked_handles_are_refused(engine):
    """ICP_ESTATE on a handle that has tracked a frame since icp_init / icp_track_reset."""
    g = engine.ICP(0)
    g.init(16384, 256, K.A, K.C_)
    F, M = engine.synth_pair(128)
    K.load(engine, g, F, M)
    g.buildRBC()
    assert g.evaluate(10.0)[0].n_moving == 16384
    assert g.track_next(engine.synth_cloud_vga()) is None
    with pytest.raises(engine.ICPError) as e:
        g.evaluate(10.0)
    assert e.value.code == ESTATE and "track" in str(e.value)
    assert g.track_next(engine.synth_cloud_vga(moved=1)) is not None
    with pytest.raises(engine.ICPError) as e:
        g.evaluate(10.0)
    assert e.value.code == ESTATE and "track" in str(e.value)
    g.close()
