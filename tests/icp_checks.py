"""Step checks shared by the GPU test modules — TEST INFRASTRUCTURE (a plain module: pytest collects nothing from it).

pytest rewrites `assert` only in the modules it collects, so every assert here carries its own message.

1. basics: constants, the bit-for-bit comparison, scenes and the numpy rules several features share;
2. the reference-order / fused parity checks against a whole OracleICP (parity_make, check_rbc, parity_check_step);
3. the weight-rule family (rejection, trimming, one-to-one, the pair filter, the robust loss on point-to-point): a feature's numpy rule
   names the rows that weigh nothing (`zero`), check_pieces compares the step with the oracle's pieces fed those rows zeroed;
4. the plane family (point-to-plane, colored, plane-to-plane, symmetric, their robust forms): a `restate` callable wraps the metric's
   float64 restatement, check_last compares the last iteration with it;
5. the route of an iteration: every opt-in pass composed (composed_rule; bit 4 of a mask is the reciprocal rule, fed the oracle's back
   search: back_at), the step checks against it, and the ICP_PAIRS_LAST_ITERATION set against it (check_route_pairs); the same route
   headed by the projection in the search's place (PROJ_ROUTE_SCENES, ProjectiveWant: projective_ref.project is the expectation);
6. the scenes of the correspondence sets in every search layout (LAYOUT_CASES, layout_scene), and the same scenes with the reciprocal rule
   between their rejection and their trimming (layout_reciprocal);
7. the reciprocal rule's own scenes: a registration that is done at once beside two that are not (converged_pairs), a moving frame with
   non-finite rows (messy_scene)."""
import collections
import functools

import numpy as np

import colored_ref
import gicp_ref
import p2pl_ref
import pair_filter_ref
import pairs_ref
import quality_ref
import reciprocal_ref
import robust_ref
import sym_ref
import unique_ref

# ---- 1. basics --------------------------------------------------------------------------------------------------------------------

A, C_ = 2e2, 1e-6
POWER, EIGEN = 1, 0
REGULAR, WEIGHTED = 0, 1
P2P, P2PL, COLORED = 0, 1, 2
GIVEN, GRID = 0, 1
MODES = [(POWER, False), (POWER, True), (EIGEN, False)]
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1], np.float32)
IDENTITY.flags.writeable = False
SIZES = {"small": (32, 64), "A": (128, 256), "B": (256, 1024)}
STEP_SIZES = [(128, 256), (50, 4), (256, 1024)]                  # m = 16384; 2500 (no multiple of 256); 65536 with nr = 1024
LOSSES = [robust_ref.HUBER, robust_ref.CAUCHY, robust_ref.TUKEY]
SCALE = {robust_ref.HUBER: 8.0, robust_ref.CAUCHY: 12.0, robust_ref.TUKEY: 30.0}     # (mm: each cuts into the residuals of the scenes)


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a.view(np.uint32)


def assert_bits(got, want, what):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(bits(got).reshape(-1) != bits(want).reshape(-1))[0]
    assert bad.size == 0, "%s: %d of %d words differ, first at %d: got %r want %r" % (
        what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def assert_bits_nan(got, want, what):
    """Bit for bit, except that a NaN of `want` asks for a NaN only (a degenerate S — one accepted pair — leaves the solver's NaN:
    payload bits are no part of the rule)."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: the NaN masks differ: got %r want %r" % (what, got, want)
    assert_bits(got[~nan], want[~nan], what)


def set_modes(engine, g, power_fast=False, fused=False):
    """Explicit modes (the handle's defaults are the benchmarked ones: squared + fused)."""
    g.setPowerMode(engine.PowerMode.SQUARED if power_fast else engine.PowerMode.LITERAL)
    g.setReduceMode(engine.ReduceMode.FUSED if fused else engine.ReduceMode.REFERENCE_ORDER)


def _t0():
    """A non-identity starting transform: 1 degree about a skew axis, a few mm."""
    ax = np.array([0.3, 0.9, 0.1]) / np.linalg.norm([0.3, 0.9, 0.1])
    h = np.deg2rad(1.0) / 2
    return np.array([*(np.sin(h) * ax), np.cos(h), 4.0, -3.0, 2.0, 1.0], np.float32)


def holes_pair(engine, side, seed, name="blobs30"):
    """Scene level: the benchmark pair with the invalid points of case `name` in both frames."""
    from icp_amd import workloads as W
    return W.holes_pair(engine, name, side, seed=seed)


def punch_cloud(engine, X, side, seed):
    """Cloud level: contiguous (15 %) and scattered (5 %) holes in one set."""
    X = engine.punch_holes(X, side, side, engine.HOLES_CONTIGUOUS, 0.15, True, seed=seed)
    return engine.punch_holes(X, side, side, engine.HOLES_SCATTERED, 0.05, True, seed=seed + 1)


def messy_grid(engine, side, seed):
    """A fixed set with holes, NaN / inf coordinates and points at the origin."""
    F, _ = engine.synth_pair(side, seed=seed)
    F = punch_cloud(engine, F, side, seed)
    rng = np.random.default_rng(seed)
    idx = rng.choice(side * side, 40, replace=False)
    F[idx[:10], 0] = np.nan
    F[idx[10:20], 1] = np.inf
    F[idx[20:30], 2] = -np.inf
    F[idx[30:], :3] = 0.0
    return F


def _partial_overlap(engine):
    """synth_pair_scene(128) with a frame-to-frame motion (1 degree, (8, -4, 5) mm) and the last quarter of M's rows moved 150 mm
    towards the camera: a surface F has no counterpart for."""
    F, M, T_true = engine.synth_pair_scene(128, rot_deg=1.0, t=(8.0, -4.0, 5.0))
    M = M.copy()
    M[np.arange(128 * 128) >= 96 * 128, 2] -= 150.0
    return F, M, T_true


def _outlier_scene(engine):
    """The curved scene with about 20 % of the moving landmarks gross outliers: a contiguous band of 26 grid rows pulled 300 mm toward
    the sensor (an occluder only the moving frame sees)."""
    F, M, T_true = engine.synth_pair_scene(128, engine.SCENE_CURVED)
    M = M.copy()
    rows = slice(50 * 128, 76 * 128)
    z = M[rows, 2].astype(np.float64)
    f = np.where(z > 0, (z - 300.0) / z, 1.0).astype(np.float32)
    M[rows, :3] *= f[:, None]
    return F, M, T_true


def _errors(T, T_true):
    """(rotation error in degrees, translation error in mm) of T against T_true."""
    from icp_amd import workloads as W
    return W.rotation_error_deg(T, T_true), float(np.linalg.norm(T[4:7].astype(np.float64) - T_true[4:7].astype(np.float64)))


def register(engine, F, M, metric, mu=0.0, kappa=0.0):
    """(T, k, converged) of a free run of a fresh handle with the metric on."""
    g = engine.ICP(0)
    g.init(F.shape[0], 256, A, C_)
    if metric != P2P:
        g.set_normals(GRID, int(round(np.sqrt(F.shape[0]))))
        if metric == COLORED:
            g.set_color_weight(kappa)
        g.set_error_metric(metric, mu)
    load(engine, g, F, M)
    g.buildRBC()
    k = g.run()
    T = g.read(engine.Memory.T).copy()
    conv = g.state().converged
    g.close()
    return T, k, conv


def geo_of(PF, PM):
    g = (PM[:, :3] - PF[:, :3]).astype(np.float32)
    return (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]


def rejected_set(M, PF, PM, invalid, max_dist):
    """The rule of include/icp_amd.h in numpy: M = the moving set (untransformed), PF / PM = (matched fixed xyz, w) / (transformed
    moving xyz, dist) per query."""
    rej = np.zeros(M.shape[0], bool)
    if invalid:
        rej |= (M[:, :3] == 0).all(axis=1) | (PF[:, :3] == 0).all(axis=1)
    if max_dist:
        d2 = np.float32(max_dist) * np.float32(max_dist)
        rej |= ~(geo_of(PF, PM) <= d2)
    return rej


def trim_rule(PF, PM, W0, keep):
    """(accepted mask, [t bits, n, K, accepted]) by the rule: candidates are the pairs of weight != 0 (W0: after rejection, before
    trimming) with a finite geo; K = ceil (keep n); t = the K-th smallest geo; accepted: candidates with geo <= t."""
    geo = geo_of(PF, PM)
    cand = (W0 != 0) & np.isfinite(geo)
    n = int(np.count_nonzero(cand))
    if n == 0:
        return np.zeros(PF.shape[0], bool), np.zeros(4, np.uint32)
    K = min(int(np.ceil(np.float64(np.float32(keep)) * n)), n)
    t = np.sort(geo[cand])[K - 1]
    acc = cand & (geo <= t)
    return acc, np.array([t.view(np.uint32), n, K, np.count_nonzero(acc)], np.uint32)


def search_weights(nn_id, weighted):
    """The weights of the search's distances: 100 / (100 + dist), or ones in REGULAR mode."""
    dist = nn_id["dist"].astype(np.float32)
    return (np.float32(100.0) / (np.float32(100.0) + dist)).astype(np.float32) if weighted else np.ones_like(dist)


def weights_before_trim(nn_id, M, PF, PM, weighted, invalid, max_dist=None):
    W0 = search_weights(nn_id, weighted)
    W0[rejected_set(M, PF, PM, invalid, max_dist)] = 0.0
    return W0


def oracle_search(oracle, F, M, T, nr, a=A):
    o = oracle.OracleICP(F.shape[0], nr, a, C_, threads=8)
    o.write_f(F); o.write_m(M); o.build_rbc(); o.write_t(T)
    o.step()
    return o.nn_id, o.rid


def pick_max_dist(oracle, F, M, T, nr, frac=0.12, nn_id=None):
    """A distance that rejects about `frac` of the pairs whose endpoints are both valid, at T (nn_id: the oracle's search at T, when the
    caller has it already)."""
    if nn_id is None:
        nn_id, _ = oracle_search(oracle, F, M, T, nr)
    tM = oracle.transform_q(M, T)
    NN = F[nn_id["id"]]
    ok = ~((M[:, :3] == 0).all(axis=1) | (NN[:, :3] == 0).all(axis=1))
    g = (tM[:, :3] - NN[:, :3]).astype(np.float64)
    geo = (g * g).sum(axis=1)[ok]
    return float(np.sqrt(np.quantile(geo, 1.0 - frac)))


@functools.lru_cache(maxsize=None)
def _scene(side, nr, name):
    import icp_amd as engine
    from oracle import oracle
    F, M = engine.synth_pair(side) if name == "clean" else holes_pair(engine, side, 0x1C9D5EED)
    T = _t0()
    nn_id, rid = oracle_search(oracle, F, M, T, nr)
    for a in (F, M, T, nn_id, rid):
        a.flags.writeable = False
    return F, M, T, name == "holes", (nn_id, rid)


def scene(engine, oracle, side, nr, name):
    """(F, M, T, invalid flag, the oracle's (nn_id, rid) at T) of the "clean" pair or the blobs30 "holes" pair, read-only: built and
    searched once per session.  (engine and oracle are the session's fixtures: asking for them builds both libraries first.)"""
    return _scene(side, nr, name)


def scenes_A(engine, oracle):
    """name -> scene at side 128 with 256 representatives."""
    return {name: scene(engine, oracle, 128, 256, name) for name in ("clean", "holes")}


# ---- 2. parity against a whole OracleICP --------------------------------------------------------------------------------------

def parity_make(engine, oracle, side, nr, rot=1, weighted=1, power_fast=False, zero_fraction=0.0, seed=0x1C9D5EED,
                max_iterations=40, fused=False):
    m = side * side
    F, M = engine.synth_pair(side, seed=seed, zero_fraction=zero_fraction)
    g = engine.ICP(0, rot, weighted)
    g.init(m, nr, A, C_, max_iterations=max_iterations)
    set_modes(engine, g, power_fast, fused)
    g.write(engine.Memory.F, F)
    g.write(engine.Memory.M, M)
    o = oracle.OracleICP(m, nr, A, C_, rot=rot, weighted=weighted, power_fast=power_fast, threads=8,
                         max_iterations=max_iterations, fused=fused)
    o.write_f(F)
    o.write_m(M)
    return g, o, F, M


def check_rbc(engine, g, o):
    Mem = engine.Memory
    assert_bits(g.read(Mem.REPS), o.reps, "representatives")
    assert np.array_equal(g.read(Mem.RBC_OWNER), o.rbc_owner), "owner"
    assert np.array_equal(g.read(Mem.RBC_N), o.rbc_N), "N"
    assert np.array_equal(g.read(Mem.RBC_O), o.rbc_O), "O"
    assert np.array_equal(g.read(Mem.RBC_PERM), o.rbc_perm), "perm"


def parity_check_step(engine, g, o, weighted=True):
    Mem = engine.Memory
    assert np.array_equal(g.read(Mem.RID), o.rid), "nearest representative"
    gn, on = g.read(Mem.NN_ID), o.nn_id
    assert np.array_equal(gn["id"], on["id"]), "correspondence ids: %d differ" % np.count_nonzero(gn["id"] != on["id"])
    assert_bits(gn["dist"], on["dist"], "correspondence distances")
    if weighted:
        assert_bits(g.read(Mem.W), o.W, "weights")
        assert_bits(g.read(Mem.SUM_W), np.array([o.sum_w]), "sum of weights")
    assert_bits(g.read(Mem.MEANS), o.means, "means")
    assert_bits(g.read(Mem.S), o.S, "S")
    assert_bits(g.read(Mem.TK), o.Tk, "Tk")
    assert_bits(g.read(Mem.RK).reshape(3, 3), o.Rk, "Rk")
    assert_bits(g.read(Mem.R).reshape(3, 3), o.R, "R")
    assert_bits(g.read(Mem.T), o.T, "T")


# ---- 3. the weight-rule family ------------------------------------------------------------------------------------------------

def make_handle(engine, m, nr, fused, weighted, rot, power_fast, batch=1, max_iterations=40, rejection=None, boundary=None,
                normal_rejection=None, unique=None, trimming=None, robust_loss=None):
    """A point-to-point handle with explicit modes.  The options are applied in this order, each only when given (not None):
    rejection = (invalid, max_dist); boundary = grid width; normal_rejection = (grid width of the GRID normals, min_cos);
    unique = flag; trimming = keep; robust_loss = (loss, scale)."""
    g = engine.ICP(0, rot, weighted)
    g.init(m, nr, A, C_, max_iterations, batch=batch)
    set_modes(engine, g, power_fast, fused)
    if rejection is not None:
        g.set_rejection(*rejection)
    if boundary is not None:
        g.set_boundary_rejection(boundary)
    if normal_rejection is not None:
        g.set_normals(GRID, normal_rejection[0])
        g.set_normal_rejection(normal_rejection[1])
    if unique is not None:
        g.set_unique(unique)
    if trimming is not None:
        g.set_trimming(trimming)
    if robust_loss is not None:
        g.set_robust_loss(*robust_loss)
    return g


def only_invalid(invalid):
    """make_handle's rejection option for "the invalid-point rule when the scene has holes, else untouched"."""
    return (True, None) if invalid else None


def one_step(engine, g, F, M, T):
    """Load the pair, build, start at T, step.  Returns R as the step's search used it."""
    g.write(engine.Memory.F, F); g.write(engine.Memory.M, M)
    g.buildRBC()
    g.write(engine.Memory.T, T, block=True)
    R0 = g.read(engine.Memory.R).ravel().copy()
    g.step()
    return R0


def step_batch(engine, g, pairs, T):
    """one_step for a handle of len (pairs) registrations, all from T."""
    for b, (F, M) in enumerate(pairs):
        g.write(engine.Memory.F, F, batch_index=b); g.write(engine.Memory.M, M, batch_index=b)
    g.buildRBC()
    for b in range(len(pairs)):
        g.write(engine.Memory.T, T, batch_index=b, block=True)
    g.step()


def correspondences(engine, g, want=None, b=0):
    """The nn_id the rules and the oracle's pieces are fed: the oracle's (want = its (nn_id, rid); check_pieces compares the engine's
    with it) or, without one, the engine's own."""
    return want[0] if want is not None else g.read(engine.Memory.NN_ID, batch_index=b)


def expected_pieces(oracle, F, M, T, nn_id, side, fused, weighted, rot, power_fast, zero, weights=None):
    """(W, sum_w, means, S, Tk) of one step at T from the oracle's pieces with the rows `zero` (trimmed, rejected, ..) zeroed.
    weights: arbitrary weights W' in place of the search's (the robust loss; in reference order sum W is then
    robust_ref.sum_w_reference, orc_weights' tree over arbitrary weights)."""
    tM = oracle.transform_q(M, T)
    NNz, tMz = np.ascontiguousarray(F[nn_id["id"]]), tM.copy()
    NNz[zero] = 0.0
    tMz[zero] = 0.0
    if fused or weights is not None:
        W = search_weights(nn_id, weighted) if weights is None else weights
        if weights is None:
            W[zero] = 0.0
    if fused:
        sw, means, S = oracle.moments_fused(NNz, tMz, W, side, C_)
    else:
        if weights is None:
            D = nn_id.copy()
            if not weighted:
                D["dist"] = 0.0                      # 100 / (100 + 0) = 1: the weights of REGULAR mode, w in {0, 1}
            D["dist"][zero] = np.inf                 # 100 / (100 + inf) = +0
            W, sw = oracle.weights(D)
        else:
            sw = robust_ref.sum_w_reference(W)
        means = oracle.mean_weighted(NNz, tMz, W, sw)
        DF, DM = oracle.devs(NNz, tMz, means)
        S = oracle.sij(DM, DF, W, C_)
    if rot == POWER:
        Tk, _ = oracle.power_method(S, means, fast=power_fast)
    else:
        _, Tk = oracle.svd_rotation(S, means)
    return W, sw, means, S, Tk


def check_search(engine, g, want, b=0):
    """The engine's correspondences, distances and nearest representatives against the oracle's (nn_id, rid).  want a ProjectiveWant
    (the projection heads the route): ICP_MEM_NN_ID — the misses' 0xFFFFFFFF included —, the matched fixed points of ICP_MEM_NN,
    ICP_MEM_QT and the words of ICP_MEM_PROJECTIVE against projective_ref.project's."""
    Mem = engine.Memory
    if isinstance(want, ProjectiveWant):
        got = check_projective_outputs(engine, g, want.res, b)
        assert got[1] > 0, "ICP_MEM_PROJECTIVE %r: no hit" % (got,)
        return
    nn_id, rid = want
    gn = g.read(Mem.NN_ID, batch_index=b)
    assert np.array_equal(gn["id"], nn_id["id"]), "correspondence ids: %d differ" % np.count_nonzero(gn["id"] != nn_id["id"])
    assert_bits(gn["dist"], nn_id["dist"], "correspondence distances")
    assert np.array_equal(g.read(Mem.RID, batch_index=b), rid), "nearest representative"


def check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, zero, want=None, b=0, weights=None):
    """The engine's step from T (already taken): the search against the oracle's (want = its (nn_id, rid) at T; None: the engine's own
    correspondences feed the oracle's pieces), then W, sum W, means, S and Tk bit for bit against expected_pieces with the rows `zero`
    zeroed, and "a row in zero has the weight +0".  Returns the expected W."""
    Mem = engine.Memory
    if want is not None:
        check_search(engine, g, want, b)
    nn_id = correspondences(engine, g, want, b)
    W, sw, means, S, Tk = expected_pieces(oracle, F, M, T, nn_id, side, fused, weighted, rot, power_fast, zero, weights)
    gW = g.read(Mem.W, batch_index=b)
    assert_bits(gW, W, "weights")
    nonzero = np.count_nonzero(np.ascontiguousarray(gW[zero]).view(np.uint32))
    assert nonzero == 0, "a trimmed, rejected or losing pair's weight is +0: %d are not" % nonzero
    assert_bits(g.read(Mem.SUM_W, batch_index=b), np.array([sw]), "sum of weights")
    assert_bits(g.read(Mem.MEANS, batch_index=b), means, "means")
    assert_bits(g.read(Mem.S, batch_index=b), S, "S")
    assert_bits_nan(g.read(Mem.TK, batch_index=b), Tk, "Tk")
    return W


def assert_words(engine, g, mem, counts, b=0):
    """A feature's result words (ICP_MEM_TRIM, ICP_MEM_UNIQUE, ICP_MEM_PAIR_FILTER) against the numpy rule's."""
    got = g.read(getattr(engine.Memory, mem), batch_index=b)
    assert np.array_equal(got, counts), "ICP_MEM_%s: got %r want %r" % (mem, got, counts)
    return got


def check_rejection_step(engine, oracle, g, F, M, T, side, nr, fused, weighted, rot, power_fast, invalid, max_dist, b=0):
    """Rejection: the rejected set of the oracle's search equals the one of the engine's own outputs; then the pieces."""
    Mem = engine.Memory
    want = oracle_search(oracle, F, M, T, nr)
    check_search(engine, g, want, b)
    NN, tM = F[want[0]["id"]], oracle.transform_q(M, T)
    rej = rejected_set(M, NN[:, :4], tM[:, :4], invalid, max_dist)
    PF, PM = g.read(Mem.NN, batch_index=b), g.read(Mem.QT, batch_index=b)
    assert np.array_equal(rejected_set(M, PF, PM, invalid, max_dist), rej), "rejected set"
    assert rej.any() and not rej.all(), "rejected set: %d of %d" % (np.count_nonzero(rej), rej.size)
    check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, rej, want, b)
    return rej


def check_trim_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, invalid, keep, want=None, b=0):
    """Trimming: ICP_MEM_TRIM against trim_rule on the engine's own NN / QT, then the pieces.  Returns (accepted, the words)."""
    Mem = engine.Memory
    nn_id = correspondences(engine, g, want, b)
    PF, PM = g.read(Mem.NN, batch_index=b), g.read(Mem.QT, batch_index=b)
    acc, trim = trim_rule(PF, PM, weights_before_trim(nn_id, M, PF, PM, weighted, invalid), keep)
    assert_words(engine, g, "TRIM", trim, b)
    check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, ~acc, want, b)
    return acc, trim


def unique_rule_of(engine, g, M, weighted, invalid, b=0, nn_id=None):
    """(winner mask, rows that weigh nothing, [n, winners], weights before the rule) from the engine's outputs of registration b."""
    Mem = engine.Memory
    if nn_id is None:
        nn_id = g.read(Mem.NN_ID, batch_index=b)
    PF, PM = g.read(Mem.NN, batch_index=b), g.read(Mem.QT, batch_index=b)
    W0 = weights_before_trim(nn_id, M, PF, PM, weighted, invalid)
    win, cand, counts = unique_ref.unique_rule(nn_id["id"], PF, PM, W0)
    return win, (W0 == 0) | (cand & ~win), counts, W0


def check_unique_step(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, invalid, want=None, b=0):
    """One-to-one: ICP_MEM_UNIQUE, the pieces, and "a winner keeps its weight".  Returns (winners, counts)."""
    win, zero, counts, _ = unique_rule_of(engine, g, M, weighted, invalid, b, correspondences(engine, g, want, b))
    assert_words(engine, g, "UNIQUE", counts, b)
    check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, zero, want, b)
    lost = np.count_nonzero(g.read(engine.Memory.W, batch_index=b)[win] == 0)
    assert lost == 0, "a winner keeps its weight: %d do not" % lost
    return win, counts


def pair_filter_rule_of(engine, g, F, M, R0, weighted, invalid, gw, min_cos, b=0, nn_id=None):
    """(rows that weigh nothing, counts, weights before the rules, (at_boundary, incompatible, accepted))."""
    Mem = engine.Memory
    if nn_id is None:
        nn_id = g.read(Mem.NN_ID, batch_index=b)
    PF, PM = g.read(Mem.NN, batch_index=b), g.read(Mem.QT, batch_index=b)
    W0 = weights_before_trim(nn_id, M, PF, PM, weighted, invalid)
    NF = NM = None
    if min_cos is not None:
        NF, NM = g.read(Mem.NORMALS_F, batch_index=b), g.read(Mem.NORMALS_M, batch_index=b)
    bnd, inc, acc, counts = pair_filter_ref.pair_filter(nn_id["id"], W0, F, gw, NF, NM, R0, min_cos)
    return ~acc, counts, W0, (bnd, inc, acc)


def check_pair_filter_step(engine, oracle, g, F, M, T, R0, side, fused, weighted, rot, power_fast, invalid, gw, min_cos, want=None, b=0):
    """The pair filter: ICP_MEM_PAIR_FILTER, the pieces, "an accepted pair keeps its weight" and the NN output's weights."""
    Mem = engine.Memory
    zero, counts, W0, masks = pair_filter_rule_of(engine, g, F, M, R0, weighted, invalid, gw, min_cos, b, correspondences(engine, g, want, b))
    got = g.read(Mem.PAIR_FILTER, batch_index=b)
    print("ICP_MEM_PAIR_FILTER", got.tolist(), "numpy", counts.tolist())
    assert_words(engine, g, "PAIR_FILTER", counts, b)
    assert got[0] == got[1] + got[2] + got[3], "ICP_MEM_PAIR_FILTER: n is not the sum of its parts: %r" % got
    W = check_pieces(engine, oracle, g, F, M, T, side, fused, weighted, rot, power_fast, zero, want, b)
    lost = np.count_nonzero(g.read(Mem.W, batch_index=b)[masks[2]] == 0)
    assert lost == 0, "an accepted pair keeps its weight: %d do not" % lost
    assert_bits(g.read(Mem.NN, batch_index=b)[:, 3], W, "the NN output's weights")
    return counts, masks


# the robust loss on point-to-point: the weights W' come from numpy (robust_ref.p2p_weights on the engine's own NN / QT after rejection
# and trimming), and the pieces are fed W' with the rows of W' == 0 zeroed

def p2p_expected(oracle, g, engine, M, T, side, fused, weighted, rot, power_fast, invalid, max_dist, keep, loss, scale, b=0):
    """(W', sum W, means, S, Tk) of the step the engine took from T, from its own outputs."""
    Mem = engine.Memory
    nn_id = g.read(Mem.NN_ID, batch_index=b)
    W = _robust_weights(engine, g, nn_id, M, weighted, invalid, max_dist, keep, loss, scale, b)
    return expected_pieces(oracle, g.read(Mem.F, batch_index=b), M, T, nn_id, side, fused, weighted, rot, power_fast, W == 0, W)


def _robust_weights(engine, g, nn_id, M, weighted, invalid, max_dist, keep, loss, scale, b):
    Mem = engine.Memory
    PF, PM = g.read(Mem.NN, batch_index=b), g.read(Mem.QT, batch_index=b)
    W0 = weights_before_trim(nn_id, M, PF, PM, weighted, invalid, max_dist)
    if keep < 1.0:
        acc, _ = trim_rule(PF, PM, W0, keep)
        W0[~acc] = 0.0
    return robust_ref.p2p_weights(W0, PF, PM, loss, scale)


def check_p2p(oracle, g, engine, M, T, side, fused, weighted, rot, power_fast, invalid=False, max_dist=None, keep=1.0,
              loss=robust_ref.CAUCHY, scale=12.0, b=0):
    Mem = engine.Memory
    W = _robust_weights(engine, g, g.read(Mem.NN_ID, batch_index=b), M, weighted, invalid, max_dist, keep, loss, scale, b)
    return check_pieces(engine, oracle, g, g.read(Mem.F, batch_index=b), M, T, side, fused, weighted, rot, power_fast, W == 0, None, b, W)


def check_p2p_or_identity(oracle, g, engine, M, T, side, fused, weighted, rot, power_fast, invalid=False, max_dist=None, keep=1.0,
                          loss=robust_ref.CAUCHY, scale=12.0, b=0):
    """check_p2p, or — when the restatement's sum W is 0 — the header's identity step: W' all +0, sum W, means and S zero, T as it
    was, Tk the identity.  Returns (W', whether nothing was accepted)."""
    Mem = engine.Memory
    W, sw, _, _, _ = p2p_expected(oracle, g, engine, M, T, side, fused, weighted, rot, power_fast, invalid, max_dist, keep, loss, scale, b)
    if sw != 0:
        return check_p2p(oracle, g, engine, M, T, side, fused, weighted, rot, power_fast, invalid, max_dist, keep, loss, scale, b), False
    gW = g.read(Mem.W, batch_index=b)
    assert_bits(gW, W, "W'")
    assert (np.ascontiguousarray(gW).view(np.uint32) == 0).all() and g.read(Mem.SUM_W, batch_index=b)[0] == 0, "W' and sum W are +0"
    assert (g.read(Mem.MEANS, batch_index=b) == 0).all() and (g.read(Mem.S, batch_index=b) == 0).all(), "means and S are zero"
    assert_bits(g.read(Mem.T, batch_index=b), T, "T behind a step that accepts nothing")
    assert_bits(g.read(Mem.TK, batch_index=b), IDENTITY, "Tk behind a step that accepts nothing")
    return W, True


def p2p_handle(engine, m, nr, fused, weighted, rot, power_fast, loss, scale, invalid=False, max_dist=None, keep=1.0, batch=1, it=40):
    return make_handle(engine, m, nr, fused, weighted, rot, power_fast, batch, it,
                       rejection=(invalid, max_dist) if invalid or max_dist else None, trimming=keep if keep < 1.0 else None,
                       robust_loss=(loss, scale))


# ---- 4. the plane family ----------------------------------------------------------------------------------------------------------

def make_plane(engine, side, nr, weighted=WEIGHTED, mu=0.05, normals=GRID, batch=1, max_iterations=40, rot=POWER, fused=None,
               power_fast=None, metric=P2PL, kappa=None, plane_to_plane=None, symmetric=None, trimming=None, robust_loss=None):
    """A handle with a plane metric on.  The options are applied in this order, each only when given: fused / power_fast (either one
    given sets both modes; the other then defaults to the handle's own default, on); the normals; kappa (COLORED: 1000 unless given);
    the metric with mu; plane_to_plane = epsilon; symmetric = flag; trimming = keep; robust_loss = (loss, scale)."""
    g = engine.ICP(0, rot, weighted)
    g.init(side * side, nr, A, C_, max_iterations, batch=batch)
    if fused is not None or power_fast is not None:
        set_modes(engine, g, power_fast is None or power_fast, fused is None or fused)
    g.set_normals(normals, side if normals == GRID else 0)
    if metric == COLORED:
        g.set_color_weight(1000.0 if kappa is None else kappa)
    g.set_error_metric(metric, mu)
    if plane_to_plane is not None:
        g.set_plane_to_plane(plane_to_plane)
    if symmetric is not None:
        g.set_symmetric(symmetric)
    if trimming is not None:
        g.set_trimming(trimming)
    if robust_loss is not None:
        g.set_robust_loss(*robust_loss)
    return g


def load(engine, g, F, M, b=0):
    g.write(engine.Memory.F, F, batch_index=b)
    g.write(engine.Memory.M, M, batch_index=b)


def before(engine, g, b=0):
    Mem = engine.Memory
    return g.read(Mem.T, b).copy(), g.read(Mem.R, b).ravel().copy(), g.state(b).k


# restate (read, PF, PM, ids, T0, R0) -> (system, T, R, Tk, Rk): read (name) is the engine's table ICP_MEM_<name> of the registration

def restate_p2pl(mu, normals=None):
    return lambda read, PF, PM, ids, T0, R0: p2pl_ref.step(PF, PM, ids, read("NORMALS_F") if normals is None else normals, mu, T0, R0)


def restate_colored(mu, kappa):
    return lambda read, PF, PM, ids, T0, R0: colored_ref.step(PF, PM, ids, read("NORMALS_F"), read("COLOR_GRAD_F"),
                                                              read("M").reshape(-1, 8), mu, kappa, T0, R0)


def restate_gicp(mu, eps, loss=None, scale=None):
    return lambda read, PF, PM, ids, T0, R0: gicp_ref.step(PF, PM, ids, read("NORMALS_F"), read("NORMALS_M"), mu, eps, T0, R0, loss, scale)


def restate_symmetric(mu, loss=None, scale=None):
    return lambda read, PF, PM, ids, T0, R0: sym_ref.step(PF, PM, ids, read("NORMALS_F"), read("NORMALS_M"), mu, T0, R0, loss, scale)


def restate_robust(metric, loss, scale, mu=0.05, kappa=1e3, M=None):
    return lambda read, PF, PM, ids, T0, R0: robust_ref.plane_step(PF, PM, ids, read("NORMALS_F"), mu, loss, scale, T0, R0,
                                                                   read("COLOR_GRAD_F") if metric == COLORED else None, M, kappa)


def check_last(engine, g, restate, T0, R0, k0, b=0, steps=1, weights=None):
    """The last iteration of registration b against the restatement fed the device's own outputs and the state (T0, R0, k0) before the
    `steps` iterations (k0 None: the caller does not know it, k is not compared).  weights: a numpy rule's weights, fed in place of
    the device's own weight column.  Returns the system."""
    Mem = engine.Memory
    PF, PM, ids = g.read(Mem.NN, b), g.read(Mem.QT, b), g.read(Mem.NN_ID, b)["id"]
    miss = ids >= PF.shape[0]                                     # (a miss of the projection: id 0xFFFFFFFF, the record of a rejected pair)
    if miss.any():
        assert not PF[miss].any(), "a pair without a fixed point has the record (0, 0, 0, +0) (registration %d)" % b
        ids = np.where(miss, np.uint32(0), ids)                   # (the restatements index their tables with it; its weight is +0)
    if weights is not None:
        PF = PF.copy()
        PF[:, 3] = weights
    system, T, R, Tk, Rk = restate(lambda name: g.read(getattr(Mem, name), b), PF, PM, ids, T0, R0)
    assert_bits(g.read(Mem.PLANE_SYSTEM, b), system, "PLANE_SYSTEM (registration %d)" % b)
    assert_bits(g.read(Mem.T, b), T, "T (registration %d)" % b)
    assert_bits(g.read(Mem.R, b).ravel(), R, "R (registration %d)" % b)
    assert_bits(g.read(Mem.TK, b), Tk, "TK (registration %d)" % b)
    assert_bits(g.read(Mem.RK, b).ravel(), Rk, "RK (registration %d)" % b)
    st = g.state(b)
    if k0 is not None:
        assert st.k == k0 + steps, "k (registration %d): got %d want %d" % (b, st.k, k0 + steps)
    assert st.power_iterations == 0, "power_iterations (registration %d): %d" % (b, st.power_iterations)
    return system


def check_step(engine, g, restate, b=0):
    """One step of handle g (all registrations), checked for registration b against the restatement.  Returns the system."""
    T0, R0, k0 = before(engine, g, b)
    g.step()
    return check_last(engine, g, restate, T0, R0, k0, b)


def check_fixed_run(engine, g, n, restate):
    """A fixed run of n iterations: its last iteration against the restatement, from the state n - 1 steps leave (stepped on the same
    handle, whose steps are checked one by one elsewhere)."""
    g.reset_transform(); g.buildRBC()
    for _ in range(n - 1):
        g.step()
    T0, R0, _ = before(engine, g)
    g.reset_transform(); g.buildRBC()
    g.run_fixed(n)
    return check_last(engine, g, restate, T0, R0, 0, 0, steps=n)


def plane_handle(engine, side, nr, metric, loss, scale, mu=0.05, kappa=1e3, normals=GRID, fused=True, batch=1, it=40, keep=1.0):
    """A robust plane handle: the default rotation and weighting, the squared power start."""
    return make_plane(engine, side, nr, WEIGHTED, mu, normals, batch, it, fused=fused, power_fast=True, metric=metric, kappa=kappa,
                      trimming=keep if keep < 1.0 else None, robust_loss=(loss, scale))


def check_plane(engine, g, metric, loss, scale, T0, R0, mu=0.05, kappa=1e3, M=None, b=0):
    return check_last(engine, g, restate_robust(metric, loss, scale, mu, kappa, M), T0, R0, None, b)


# ---- 5. the route of an iteration: every opt-in pass composed, in icp_route_of's order -------------------------------------------
#
# The search's weights (invalid points and the maximum distance rejected), then the pair filter, the reciprocal rule, one-to-one, trimming
# and — on point-to-point — the robust loss, each fed what the stage before left.  The rules are the single ones above and in the *_ref modules.

RouteOptions = collections.namedtuple("RouteOptions", "weighted invalid max_dist gw min_cos unique keep loss scale max_gap", defaults=(None,))
RouteOptions.__doc__ = """What composed_rule needs of a handle's options.  Off is: gw None (the boundary rule), min_cos None (the
normal rule), unique False, keep None (trimming), loss None, max_gap None (reciprocal correspondences; 0.0 is on: exact pairs only)."""
RouteResult = collections.namedtuple("RouteResult", "W0 filter unique trim words W_before_loss W reciprocal", defaults=(None,))
RouteResult.__doc__ = """W0: the weights behind the search's rejection;  filter: (at_boundary, incompatible, accepted);  unique:
(winners, candidates);  trim: the accepted mask;  reciprocal: (exact, near, accepted) — a stage that is off has None there —;  words:
name -> what ICP_MEM_<name> reports (PAIR_FILTER, RECIPROCAL, UNIQUE, TRIM; None while the stage is off);  W_before_loss: the weights the
plane moments read;  W: W'."""


def route_options(mask, max_dist, min_cos, side, keep=0.75, loss=robust_ref.CAUCHY, scale=None, weighted=True, invalid=True, max_gap=None):
    """The options of mask (bit 0 the pair filter — the boundary rule at the grid width `side` and the normal rule at min_cos —, bit 1
    one-to-one, bit 2 trimming, bit 3 the robust loss, bit 4 reciprocal correspondences at max_gap) over rejection by invalid points
    and max_dist."""
    assert not mask & 16 or max_gap is not None, "mask %d asks for the reciprocal rule and there is no max_gap" % mask
    return RouteOptions(weighted, invalid, max_dist, side if mask & 1 else None, min_cos if mask & 1 else None, bool(mask & 2),
                        keep if mask & 4 else None, loss if mask & 8 else None, (SCALE[loss] if scale is None else scale) if mask & 8 else None,
                        max_gap if mask & 16 else None)


def composed_rule(nn_id, PF, PM, F, M, R0, NF, NM, o, plane=False, back=None):
    """The weights of an iteration with the passes of `o` (a RouteOptions) on, by the single rules in the route's order.  NF / NM: the
    two normal tables (read only when the normal rule is on).  plane: a plane metric — the loss is the moments' business, W is
    W_before_loss.  back: ((nn_id, rid) of the back search at the step's T, the inverse's ok flag) — reciprocal_ref.back_search's
    result, read only when the reciprocal rule is on (back_at caches it per scene and T).  A stage that is off passes its input through
    and reports no words."""
    ids = nn_id["id"]
    W0 = weights_before_trim(nn_id, M, PF, PM, o.weighted, o.invalid, o.max_dist)
    W, words = W0.copy(), {"PAIR_FILTER": None, "RECIPROCAL": None, "UNIQUE": None, "TRIM": None}
    flt = rcp = unq = trm = None
    if o.gw or o.min_cos is not None:
        bnd, inc, acc, words["PAIR_FILTER"] = pair_filter_ref.pair_filter(ids, W, F, o.gw, NF, NM, R0, o.min_cos)
        flt = (bnd, inc, acc)
        W = np.where(acc, W, np.float32(0)).astype(np.float32)
    if o.max_gap is not None:
        assert back is not None, "the reciprocal rule is on and composed_rule has no back search"
        (rev, _), ok = back
        exact, near, zero, words["RECIPROCAL"] = reciprocal_ref.reciprocal_rule(ids, rev["id"], PM, W, o.max_gap, ok)
        rcp = (exact, near, exact | near)
        W = np.where(zero, np.float32(0), W).astype(np.float32)
    if o.unique:
        win, cand, words["UNIQUE"] = unique_ref.unique_rule(ids, PF, PM, W)
        unq = (win, cand)
        W = unique_ref.weights_after(W, win, cand)
    if o.keep is not None:
        trm, words["TRIM"] = trim_rule(PF, PM, W, o.keep)
        W = np.where(trm, W, np.float32(0)).astype(np.float32)
    Wl = W if plane or o.loss is None else robust_ref.p2p_weights(W, PF, PM, o.loss, o.scale)
    return RouteResult(W0, flt, unq, trm, words, W, Wl, rcp)


@functools.lru_cache(maxsize=64)
def _back_at(key, T_bytes):
    from oracle import oracle
    F, M, nr = _BACK_SCENES[key]
    back, ok = reciprocal_ref.back_search(oracle, F, M, np.frombuffer(T_bytes, np.float32), nr)
    for a in back:
        a.flags.writeable = False
    return back, ok


_BACK_SCENES = {}


def back_at(key, F, M, T, nr):
    """reciprocal_ref.back_search (oracle, F, M, T, nr), searched once per (key, T): key names the pair (F, M) with nr."""
    _BACK_SCENES.setdefault(key, (F, M, nr))
    return _back_at(key, np.ascontiguousarray(T, np.float32).tobytes())


def stage_shares(r, o):
    """name -> (candidates, removed, kept) of every stage of the result r that is on; for the loss `removed` counts the candidates
    whose weight is neither their input weight nor zero."""
    out = {}
    if r.words["PAIR_FILTER"] is not None:
        n, b, i, a = (int(x) for x in r.words["PAIR_FILTER"])
        if o.gw:
            out["boundary"] = (n, b, n - b)
        if o.min_cos is not None:
            out["normal"] = (n, i, n - i)
        out["filter"] = (n, b + i, a)
    if r.words["RECIPROCAL"] is not None:
        n, a = int(r.words["RECIPROCAL"][0]), int(r.words["RECIPROCAL"][3])
        out["reciprocal"] = (n, n - a, a)
    if r.words["UNIQUE"] is not None:
        n, w = (int(x) for x in r.words["UNIQUE"])
        out["unique"] = (n, n - w, w)
    if r.words["TRIM"] is not None:
        n, a = int(r.words["TRIM"][1]), int(r.words["TRIM"][3])
        out["trim"] = (n, n - a, a)
    if o.loss is not None and r.W is not r.W_before_loss:
        cand = r.W_before_loss != 0
        out["loss"] = (int(np.count_nonzero(cand)), int(np.count_nonzero(cand & (r.W != r.W_before_loss) & (r.W != 0))),
                       int(np.count_nonzero(cand & (r.W != 0))))
    return out


def assert_every_stage_bites(r, o, what):
    """Every stage that is on removes (the loss: re-weighs) at least 2 % of its own candidates and keeps at least half of them; the
    search's rejection rejects some pair by either of its rules.  Returns stage_shares."""
    shares = stage_shares(r, o)
    for name, (n, removed, kept) in shares.items():
        assert n > 0 and 50 * removed >= n and 2 * kept >= n, "%s: stage %s has %d candidates, removes %d, keeps %d" % (what, name, n, removed, kept)
    m = r.W0.shape[0]
    assert 0 < np.count_nonzero(r.W0 == 0) < m // 2, "%s: the search rejects %d of %d" % (what, np.count_nonzero(r.W0 == 0), m)
    return shares


def pick_min_cos(oracle, F, M, T, nr, width, frac=0.1):
    """A threshold the normal rule rejects about `frac` of its candidates with, at T: that quantile of the cosines between the grid
    normals (p2pl_ref.grid_normals, `width` wide) of the reference's pairs that have both normals and no boundary point."""
    nn_id, _ = oracle_search(oracle, F, M, T, nr)
    ids = nn_id["id"]
    NF, NM = p2pl_ref.grid_normals(F, width), p2pl_ref.grid_normals(M, width)
    cos = pair_filter_ref.cosines(NF[ids], NM, oracle.quat_to_rot(T[:4]))
    ok = np.isfinite(cos) & ~pair_filter_ref.boundary_mask(F, width)[ids] & ~(M[:, :3] == 0).all(axis=1)
    return float(np.float32(np.quantile(cos[ok], frac)))


def pick_scale(oracle, F, M, T, nr, max_dist, frac=0.9):
    """A loss scale the residuals of about `frac` of the pairs that survive the search's rejection (at T) stay below."""
    nn_id, _ = oracle_search(oracle, F, M, T, nr)
    PF, PM = F[nn_id["id"]], oracle.transform_q(M, T)
    geo = geo_of(PF, PM)[~rejected_set(M, PF, PM, True, max_dist)]
    return float(np.float32(np.sqrt(np.quantile(geo.astype(np.float64), frac))))


# The scenes of the composed checks.  The benchmark pair at _t0 () matches far fewer than half of its queries one to one (its frames lie
# 25 mm and more apart, and the 8-d metric follows the colour: 29 % winners at side 128, 27 % at side 150), so one-to-one could not
# keep half of its candidates there.  These pairs are the same synthetic frames moved by about what _t0 () undoes, with 10 % of either
# frame punched out in blobs of its own: at _t0 () most queries have a fixed point to themselves, some share one, and every stage has
# pairs to remove and to keep.  name -> (side, |R|, seed, rotation in degrees, translation in mm).
ROUTE_SCENES = {"30": (30, 4, 0x20C7E, 1.0, (4.0, -3.0, 2.0)), "150": (150, 4, 0x20C7F, 1.0, (4.0, -3.0, 2.0)),
                "A": (128, 256, 0x20C80, 1.0, (4.0, -3.0, 2.0)), "batch0": (128, 64, 0x20C81, 1.0, (4.0, -3.0, 2.0)),
                "batch1": (128, 64, 0x20C82, 1.2, (6.0, -2.0, 3.0)), "batch2": (128, 64, 0x20C83, 0.8, (3.0, -4.0, 1.0))}
ROUTE_BATCH = ("batch0", "batch1", "batch2")                     # one handle, one set of options: batch0's, proven on each of the three
ROUTE_KEEP = 0.75
ROUTE_GAP_KEEP = 0.7
RouteScene = collections.namedtuple("RouteScene", "side nr F M T want R0 PF PM NF NM max_dist min_cos scale max_gap back projective",
                                    defaults=(None,))

# The projection at the head of a route (icp_set_projective in the RBC search's place): the same pairs of frames, the expectation of a
# step projective_ref.project at the step's T.  name -> the scene of ROUTE_SCENES it shares its frames with, or a pair of its own (two
# more at side 150 for the batch of three: 3 x 22500 points is also a shape the kernel serves in four rounds per block).
PROJ_ROUTE_SCENES = {"p30": "30", "p150": "150", "p150b1": (150, 4, 0x20C84, 1.2, (6.0, -2.0, 3.0)), "p150b2": (150, 4, 0x20C85, 0.8, (3.0, -4.0, 1.0))}
PROJ_ROUTE_BATCH = ("p150", "p150b1", "p150b2")                  # one handle, one set of options: p150's, proven on each of the three
PROJ_ROUTE_RADIUS = 1                                            # (r = 0 leaves one-to-one nothing to remove: a cell has one query or two)
ProjectiveWant = collections.namedtuple("ProjectiveWant", "nn_id res")
ProjectiveWant.__doc__ = """The expectation of a step behind the projection, in the place of the oracle's (nn_id, rid): nn_id = the rule's
pairs with the misses clipped (id 0, dist +inf: what every rule and the oracle's pieces index F with; a miss weighs nothing), res =
projective_ref.project's Result."""


def projective_want(F, M, T, side, r=PROJ_ROUTE_RADIUS):
    """projective_ref.project at T with the grid's own intrinsics, WEIGHTED, as a ProjectiveWant."""
    import icp_amd as engine
    import projective_ref
    from oracle import oracle
    res = projective_ref.project(oracle, F, M, T, side, engine.grid_intrinsics(side), r, True)
    nn_id = projective_ref.clipped(res.nn_id, res.miss)
    for a in (nn_id,) + tuple(res):
        a.flags.writeable = False
    return ProjectiveWant(nn_id, res)


def projective_handle(engine, m, nr, fused, weighted, rot, power_fast, gw, intr, r, batch=1, **options):
    """make_handle, then the projection (grid width gw, intrinsics intr, radius r) on the handle."""
    g = make_handle(engine, m, nr, fused, weighted, rot, power_fast, batch, **options)
    g.set_projective(gw, *intr, radius=r)
    return g


def check_projective_outputs(engine, g, res, b=0):
    """NN_ID (ids — a miss's 0xFFFFFFFF included —, distance bits), the matched fixed points, QT and ICP_MEM_PROJECTIVE of registration b
    against the restatement (res: projective_ref.project's Result).  Returns the words."""
    Mem = engine.Memory
    gn = g.read(Mem.NN_ID, batch_index=b)
    assert np.array_equal(gn["id"], res.nn_id["id"]), "projective ids: %d differ" % np.count_nonzero(gn["id"] != res.nn_id["id"])
    assert_bits(gn["dist"], res.nn_id["dist"], "projective distances")
    assert_bits(g.read(Mem.NN, batch_index=b)[:, :3], res.NN[:, :3], "matched fixed points")
    assert_bits_nan(g.read(Mem.QT, batch_index=b), res.QT, "transformed moving points and distances")
    got = assert_words(engine, g, "PROJECTIVE", res.counts, b)
    assert got[0] == got[1] + got[2] + got[3], "ICP_MEM_PROJECTIVE %r: hits + outside + empty is not n" % (got,)
    return got


def check_projective_step(engine, oracle, g, res, F, M, T, side, fused, weighted, rot, power_fast, b=0, zero=None, pieces=None):
    """check_projective_outputs, then W, NN.w, sum W, means, S and Tk against the oracle's pieces fed the rule's pairs.  zero: further
    rows that weigh nothing (icp_set_rejection's distance test); pieces: projective_ref.pieces of these arguments where the caller
    has them already."""
    import projective_ref
    Mem = engine.Memory
    got = check_projective_outputs(engine, g, res, b)
    W, sw, means, S, Tk = pieces or projective_ref.pieces(oracle, res, F, M, T, side, fused, weighted, rot, power_fast, zero)
    gW = g.read(Mem.W, batch_index=b)
    assert_bits(gW, W, "weights")
    nonzero = np.count_nonzero(np.ascontiguousarray(gW[res.miss]).view(np.uint32))
    assert nonzero == 0, "a miss has the weight +0: %d have not" % nonzero
    assert_bits(g.read(Mem.NN, batch_index=b)[:, 3], W, "the NN output's weights")
    assert_bits(g.read(Mem.SUM_W, batch_index=b), np.array([sw]), "sum of weights")
    assert_bits(g.read(Mem.MEANS, batch_index=b), means, "means")
    assert_bits(g.read(Mem.S, batch_index=b), S, "S")
    assert_bits_nan(g.read(Mem.TK, batch_index=b), Tk, "Tk")
    return got


def route_want(oracle, s, T):
    """The expectation of a step of the scene s from T: the oracle's search, or the projection's rule where it heads the route."""
    if s.projective is not None:
        return projective_want(s.F, s.M, T, s.side, s.projective[5])
    return oracle_search(oracle, s.F, s.M, T, s.nr)


def route_pairs_of(oracle, s, want, T):
    """(PF, PM) of the expectation `want` at T: the matched fixed points and the transformed moving set."""
    if s.projective is not None:
        return want.res.NN, want.res.QT
    return s.F[want[0]["id"]], oracle.transform_q(s.M, T)


def _route_frames(side, seed, rot_deg, t):
    import icp_amd as engine
    F, M = engine.synth_pair(side, seed=seed, rot_deg=rot_deg, t=t)
    F = engine.punch_holes(F, side, side, engine.HOLES_CONTIGUOUS, 0.10, True, seed=seed + 101)
    M = engine.punch_holes(M, side, side, engine.HOLES_CONTIGUOUS, 0.10, True, seed=seed + 202)
    return F, M


def _projective_route_scene(name):
    """The scene `name` of PROJ_ROUTE_SCENES: T = _t0 (), the rule's pairs at r = PROJ_ROUTE_RADIUS, and the options: max_dist the 0.88
    quantile of the hits' own geometric distances (the RBC scene's max_dist rejects more than half of "150" at r <= 1), min_cos and
    the scales those of the scene it shares its frames with.  tests/test_route_rule_cpu.py proves that every stage bites under them."""
    import icp_amd as engine
    from oracle import oracle
    spec = PROJ_ROUTE_SCENES[name]
    if isinstance(spec, str):
        base = route_scene(spec)
        side, nr, F, M = base.side, base.nr, base.F, base.M
    else:
        side, nr = spec[:2]
        F, M = _route_frames(side, *spec[2:])
    T = _t0()
    for a in (F, M, T):
        a.flags.writeable = False
    want = projective_want(F, M, T, side)
    PF, PM = want.res.NN, want.res.QT
    if name in PROJ_ROUTE_BATCH[1:]:
        s0 = route_scene(PROJ_ROUTE_BATCH[0])
        max_dist, min_cos, scale = s0.max_dist, s0.min_cos, s0.scale
    else:
        geo = geo_of(PF, PM)[~want.res.miss]
        max_dist, min_cos, scale = float(np.float32(np.sqrt(np.quantile(geo.astype(np.float64), 0.88)))), base.min_cos, base.scale
    s = RouteScene(side, nr, F, M, T, want, oracle.quat_to_rot(T[:4]).ravel(), PF, PM, p2pl_ref.grid_normals(F, side),
                   p2pl_ref.grid_normals(M, side), max_dist, min_cos, scale, None, None,
                   (side,) + tuple(engine.grid_intrinsics(side)) + (PROJ_ROUTE_RADIUS,))
    for a in (s.R0, s.NF, s.NM):
        a.flags.writeable = False
    return s


@functools.lru_cache(maxsize=None)
def route_scene(name):
    """The scene `name` of ROUTE_SCENES, read-only, from the engine's host-side generators and the oracle alone: the pair, T = _t0 (),
    the oracle's (nn_id, rid) and R at T, PF = F[ids], PM = the transformed moving set, the grid normals of both frames, and the
    options chosen on the reference's pairs: max_dist rejects 12 % of the valid pairs (pick_max_dist), min_cos 10 % of the normal
    rule's candidates (pick_min_cos); the scales are SCALE's but Tukey's, which 90 % of the surviving residuals stay below
    (pick_scale: SCALE's 30 mm is beyond most residuals of the 30 x 30 grid); max_gap accepts ROUTE_GAP_KEEP of the reciprocal rule's
    candidates behind the search's rejection, the filter off (reciprocal_ref.pick_gap on `back`, the oracle's back search at T).  A
    strictly reciprocal set (max_gap = 0) is one to one already and would leave one-to-one nothing to remove
    (tests/test_route_rule_cpu.py).  keep is ROUTE_KEEP."""
    from oracle import oracle
    if name in PROJ_ROUTE_SCENES:
        return _projective_route_scene(name)
    side, nr, seed, rot_deg, t = ROUTE_SCENES[name]
    F, M = _route_frames(side, seed, rot_deg, t)
    T = _t0()
    want = oracle_search(oracle, F, M, T, nr)
    for a in (F, M, T):
        a.flags.writeable = False
    back = back_at(name, F, M, T, nr)
    assert back[1], "_t0 () has an inverse"
    PF, PM = np.ascontiguousarray(F[want[0]["id"]]), oracle.transform_q(M, T)
    if name in ROUTE_BATCH[1:]:
        s0 = route_scene(ROUTE_BATCH[0])
        max_dist, min_cos, scale, max_gap = s0.max_dist, s0.min_cos, s0.scale, s0.max_gap
    else:
        max_dist, min_cos = float(np.float32(pick_max_dist(oracle, F, M, T, nr))), pick_min_cos(oracle, F, M, T, nr, side)
        scale = dict(SCALE)
        scale[robust_ref.TUKEY] = pick_scale(oracle, F, M, T, nr, max_dist)
        max_gap = reciprocal_ref.pick_gap(want[0]["id"], back[0][0]["id"], PM, weights_before_trim(want[0], M, PF, PM, True, True, max_dist),
                                          keep=ROUTE_GAP_KEEP)
    s = RouteScene(side, nr, F, M, T, want, oracle.quat_to_rot(T[:4]).ravel(), PF, PM, p2pl_ref.grid_normals(F, side),
                   p2pl_ref.grid_normals(M, side), max_dist, min_cos, scale, max_gap, back)
    for a in want + s[6:11]:
        a.flags.writeable = False
    return s


def route_scene_options(s, mask, loss=robust_ref.CAUCHY):
    return route_options(mask, s.max_dist, s.min_cos, s.side, ROUTE_KEEP, loss, s.scale[loss], max_gap=s.max_gap)


@functools.lru_cache(maxsize=None)
def route_proof(name, mask, loss=robust_ref.CAUCHY, plane=False):
    """(RouteResult, stage shares) of composed_rule on the scene's reference pairs at _t0 (), every stage proven to bite."""
    s = route_scene(name)
    o = route_scene_options(s, mask, loss)
    r = composed_rule(s.want[0], s.PF, s.PM, s.F, s.M, s.R0, s.NF, s.NM, o, plane, s.back)
    return r, assert_every_stage_bites(r, o, "scene %s, mask %d, loss %d" % (name, mask, loss))


ROUTE_WORDS = {"PAIR_FILTER": 4, "UNIQUE": 2, "TRIM": 4, "RECIPROCAL": 4}
ROUTE_METRICS = ("p2pl", "colored", "gicp", "sym")
GICP_EPS = 1e-3


def route_handle(engine, side, nr, o, metric="p2p", fused=None, batch=1, it=40, projective=None):
    """A handle with the options o on.  metric "p2p": explicit modes, fused + the squared power start or reference order + the
    literal one; a plane metric of ROUTE_METRICS (mu = 0.05, kappa = 1000, epsilon = GICP_EPS): the handle's default modes.
    projective: (grid width, fx, fy, cx, cy, radius) — a RouteScene's — puts the projection in the search's place."""
    g = _route_handle(engine, side, nr, o, metric, fused, batch, it)
    if projective is not None:
        g.set_projective(*projective[:5], radius=projective[5])
    return g


def _route_handle(engine, side, nr, o, metric, fused, batch, it):
    loss = (o.loss, o.scale) if o.loss is not None else None
    if metric == "p2p":
        g = make_handle(engine, side * side, nr, fused, o.weighted, POWER, fused, batch, it, rejection=(o.invalid, o.max_dist),
                        boundary=o.gw, normal_rejection=(side, o.min_cos) if o.min_cos is not None else None,
                        unique=True if o.unique else None, trimming=o.keep, robust_loss=loss)
        if o.max_gap is not None:
            g.set_reciprocal(True, o.max_gap)
        return g
    g = make_plane(engine, side, nr, WEIGHTED if o.weighted else REGULAR, batch=batch, max_iterations=it,
                   metric=COLORED if metric == "colored" else P2PL, plane_to_plane=GICP_EPS if metric == "gicp" else None,
                   symmetric=True if metric == "sym" else None, trimming=o.keep, robust_loss=loss)
    g.set_rejection(o.invalid, o.max_dist)
    if o.gw:
        g.set_boundary_rejection(o.gw)
    if o.min_cos is not None:
        g.set_normal_rejection(o.min_cos)
    if o.unique:
        g.set_unique(True)
    if o.max_gap is not None:
        g.set_reciprocal(True, o.max_gap)
    return g


def route_restate(metric, o, M):
    """The plane metric's restatement, with the loss of o when it has one."""
    if metric == "gicp":
        return restate_gicp(0.05, GICP_EPS, o.loss, o.scale)
    if metric == "sym":
        return restate_symmetric(0.05, o.loss, o.scale)
    if o.loss is not None:
        return restate_robust(COLORED if metric == "colored" else P2PL, o.loss, o.scale, M=M)
    return restate_colored(0.05, 1000.0) if metric == "colored" else restate_p2pl(0.05)


def check_back_search(engine, g, back, b=0, what=""):
    """ICP_MEM_REVERSE_ID of registration b — every fixed point's id, and the bits of dist — against the oracle's back search."""
    got, rev = g.read(engine.Memory.REVERSE_ID, batch_index=b), back[0][0]
    assert np.array_equal(got["id"], rev["id"]), "back search ids (%s): %d differ" % (what, np.count_nonzero(got["id"] != rev["id"]))
    assert_bits(got["dist"], rev["dist"], "back search distances (%s)" % what)


def _route_rule(engine, g, F, M, NF, NM, R0, want, o, plane, b, proof, what, back=None):
    """The search against the oracle's, with the reciprocal rule on ICP_MEM_REVERSE_ID against the oracle's back search (back), the
    normal tables against the grid normals, then composed_rule on the engine's NN / QT: the
    four result words against the rule's (zeros while a stage is off) and against `proof`'s (a RouteResult from the reference's pairs:
    the first step's), every stage biting by the proof's conditions; without a proof every stage still removes some pair and keeps half."""
    Mem = engine.Memory
    check_search(engine, g, want, b)
    if o.max_gap is not None:
        check_back_search(engine, g, back, b, what)
    if plane or o.min_cos is not None:
        assert_bits(g.read(Mem.NORMALS_F, b), NF, "NORMALS_F against the grid normals (%s)" % what)
    if o.min_cos is not None:
        assert_bits(g.read(Mem.NORMALS_M, b), NM, "NORMALS_M against the grid normals (%s)" % what)
    PF, PM = g.read(Mem.NN, b), g.read(Mem.QT, b)
    r = composed_rule(want[0], PF, PM, F, M, R0, NF, NM, o, plane, back)
    for name, n in ROUTE_WORDS.items():
        words = r.words[name] if r.words[name] is not None else np.zeros(n, np.uint32)
        got = assert_words(engine, g, name, words, b)
        if proof is not None:
            proven = proof.words[name] if proof.words[name] is not None else np.zeros(n, np.uint32)
            assert np.array_equal(got, proven), "%s: ICP_MEM_%s %r, from the reference's pairs %r" % (what, name, got, proven)
    if proof is not None:                                         # (the proven step: the words just compared are the proof's)
        shares = assert_every_stage_bites(r, o, what)
    else:                                                         # (a later step, at a T no proof covers: the passes still have work)
        shares = stage_shares(r, o)
        for name in ("filter", "reciprocal", "unique", "trim", "loss"):
            n, removed, kept = shares.get(name, (1, 1, 1))
            assert removed > 0 and 2 * kept >= n, "%s: stage %s has %d candidates, removes %d, keeps %d" % (what, name, n, removed, kept)
    print(what, "shares", shares)
    return r, PF, PM


def check_route_step(engine, oracle, g, F, M, NF, NM, T, R0, want, o, fused, b=0, proof=None, what="", back=None):
    """A point-to-point step from (T, R0), already taken, with the passes of o on: _route_rule, then ICP_MEM_W against W', sum W,
    means, S and Tk by check_pieces, "an accepted pair keeps its weight" (under the loss: the loss's weight of its search weight) and
    the NN output's weights.  Returns the RouteResult."""
    Mem = engine.Memory
    r, PF, PM = _route_rule(engine, g, F, M, NF, NM, R0, want, o, False, b, proof, what, back)
    side = int(round(np.sqrt(F.shape[0])))
    check_pieces(engine, oracle, g, F, M, T, side, fused, o.weighted, POWER, fused, r.W == 0, want, b, r.W if o.loss is not None else None)
    gW = g.read(Mem.W, b)
    assert_bits(gW, r.W, "W' (%s)" % what)
    acc = r.W_before_loss != 0
    alone = r.W0 if o.loss is None else robust_ref.p2p_weights(r.W0, PF, PM, o.loss, o.scale)
    assert_bits(gW[acc], alone[acc], "an accepted pair keeps its weight (%s)" % what)
    assert_bits(PF[:, 3], gW, "the NN output's weights (%s)" % what)
    return r


def check_route_plane_step(engine, g, F, M, NF, NM, T0, R0, k0, want, o, restate, b=0, proof=None, what="", back=None):
    """A plane metric's step from (T0, R0, k0), already taken: _route_rule, the NN output's weights and ICP_MEM_W against the composed
    weights before the loss, then check_last with the restatement fed the rule's weights.  Returns the RouteResult."""
    Mem = engine.Memory
    r, PF, _ = _route_rule(engine, g, F, M, NF, NM, R0, want, o, True, b, proof, what, back)
    assert_bits(PF[:, 3], r.W_before_loss, "the NN output's weights (%s)" % what)
    assert_bits(g.read(Mem.W, b), r.W_before_loss, "ICP_MEM_W (%s)" % what)
    check_last(engine, g, restate, T0, R0, k0, b, weights=r.W_before_loss)
    return r


def last_stage_count(r, o, plane):
    """(what decides, the number of pairs the iteration used) by include/icp_amd.h: the word of the last acting stage of o —
    ICP_MEM_TRIM's accepted, else ICP_MEM_UNIQUE's winners, else ICP_MEM_RECIPROCAL's accepted, else ICP_MEM_PAIR_FILTER's accepted, with no
    stage on the pairs the search left a weight —; a point-to-point loss acts behind all of them and may zero further weights: the pairs it leaves one."""
    if not plane and o.loss is not None:
        return "W'", int(np.count_nonzero(r.W))
    if o.keep is not None:
        return "TRIM", int(r.words["TRIM"][3])
    if o.unique:
        return "UNIQUE", int(r.words["UNIQUE"][1])
    if o.max_gap is not None:
        return "RECIPROCAL", int(r.words["RECIPROCAL"][3])
    if o.gw or o.min_cos is not None:
        return "PAIR_FILTER", int(r.words["PAIR_FILTER"][3])
    return "W0", int(np.count_nonzero(r.W0))


def check_route_pairs(engine, g, ids, PF, PM, r, plane, o, b, what):
    """The ICP_PAIRS_LAST_ITERATION set of registration b behind a step with the passes of o on, against an expectation nothing of which
    is read from the handle: ids = the oracle's nn_id at the step's T, PF = F[ids], PM = the oracle's transformed moving set, r = the
    RouteResult of the step (a plane metric keeps the search's weight: W_before_loss; point-to-point shows the loss: W).  The count,
    then the raw bytes; the count is the last acting stage's word (last_stage_count; the device's own word as well); `moving` ascends
    strictly and every weight is ICP_MEM_W[moving] by its bits.  Returns the device's set."""
    Mem = engine.Memory
    want = pairs_ref.last_iteration(ids, r.W_before_loss if plane else r.W, PF[:, :4], PM[:, :4])
    got = g.correspondences(engine.Pairs.LAST_ITERATION, batch_index=b)
    pairs_ref.check_set(got, want, "the LAST_ITERATION set (%s)" % what)
    name, n = last_stage_count(r, o, plane)
    assert len(got) == n, "%s: %d records, the last acting stage (%s) leaves %d" % (what, len(got), name, n)
    if name in ROUTE_WORDS:
        word = int(g.read(getattr(Mem, name), b)[ROUTE_WORDS[name] - 1])
        assert len(got) == word, "%s: %d records, ICP_MEM_%s says %d" % (what, len(got), name, word)
    assert (np.diff(got["moving"].astype(np.int64)) > 0).all(), "%s: moving does not ascend strictly" % what
    assert_bits(got["weight"], g.read(Mem.W, b)[got["moving"]], "the set's weights against ICP_MEM_W[moving] (%s)" % what)
    return got


# ---- 6. the correspondence sets in every search layout --------------------------------------------------------------------------------
#
# (side, |R|, batch, fused, zero_fraction of synth_pair or the name of a holes case, search_layout ()): test_stage2_lanes_as_candidates'
# and test_holes_dense_layouts' shapes below 2^20 points.  One 256-tile with lanes = candidates; several 256-tiles with exact ties at the
# origin, fused and in reference order; dense by batch with lanes = candidates and with the lanes of a query; the 1024-tile; the origin
# list behind more than 1024 representatives.
LAYOUT_CASES = [(256, 256, 1, True, 0.0, (1, 256, 1)), (256, 512, 1, True, 0.1, (1, 256, 1)), (256, 512, 1, False, 0.1, (1, 256, 1)),
                (128, 64, 3, True, 0.0, (1, 256, 1)), (64, 64, 9, True, 0.0, (1, 256, 0)), (256, 8192, 1, True, 0.0, (1, 1024, 0)),
                (192, 2048, 1, True, "blobs30", (1, 256, 0))]
LAYOUT_KEEP = 0.75
LayoutScene = collections.namedtuple("LayoutScene", "pairs T max_dist options wants PF PM rules")


@functools.lru_cache(maxsize=None)
def layout_scene(side, nr, batch, zero):
    """The scene of a LAYOUT_CASES row, read-only, from the host-side generators and the oracle alone: a pair per registration (another
    seed and rotation each, as test_stage2_lanes_as_candidates makes them — but the rotation grows with the registration, 3 + b / 2
    degrees: with that test's 3 - 0.75 b the later frames of nine lie so close at _t0 () that max_dist rejects nothing, trimming keeps
    3071 or 3072 pairs of every one of them and the evaluation holds all their points; here every registration has a count of its own
    in both sets, tests/test_pairs_routes_cpu.py), T = _t0 (), max_dist by pick_max_dist on registration 0
    (rounded to the engine's float), the options — rejection of invalid points and beyond max_dist, trimming to LAYOUT_KEEP, WEIGHTED —,
    and per registration the oracle's (nn_id, rid) at T, PF = F[ids], PM = the transformed moving set and composed_rule's result."""
    import icp_amd as engine
    from oracle import oracle
    if isinstance(zero, str):
        pairs = [holes_pair(engine, side, 0x1C9D5EED + 11 * b, zero) for b in range(batch)]
    else:
        pairs = [engine.synth_pair(side, seed=0x1C9D5EED + 11 * b, rot_deg=3.0 + 0.5 * b, zero_fraction=zero) for b in range(batch)]
    T = _t0()
    wants = [oracle_search(oracle, F, M, T, nr) for F, M in pairs]
    max_dist = float(np.float32(pick_max_dist(oracle, pairs[0][0], pairs[0][1], T, nr, nn_id=wants[0][0])))
    o = RouteOptions(True, True, max_dist, None, None, False, LAYOUT_KEEP, None, None)
    PF = [np.ascontiguousarray(F[w[0]["id"]]) for (F, _), w in zip(pairs, wants)]
    PM = [oracle.transform_q(M, T) for _, M in pairs]
    rules = [composed_rule(w[0], pf, pm, F, M, None, None, None, o) for (F, M), w, pf, pm in zip(pairs, wants, PF, PM)]
    for a in [T] + [x for p in pairs for x in p] + [x for w in wants for x in w] + PF + PM:
        a.flags.writeable = False
    return LayoutScene(pairs, T, max_dist, o, wants, PF, PM, rules)


def evaluated_expectation(oracle, F, M, T, nr, max_dist, want=None):
    """(the ICP_PAIRS_EVALUATED set, quality_ref's Quality) from the oracle's search at T (want: that search, when the caller has it)."""
    nn_id, _ = oracle_search(oracle, F, M, T, nr) if want is None else want
    ids = nn_id["id"]
    PF, PM = np.ascontiguousarray(F[ids][:, :4]), np.ascontiguousarray(oracle.transform_q(M, T)[:, :4])
    return pairs_ref.evaluated(M, PF, PM, ids, max_dist), quality_ref.evaluate(M, PF, PM, max_dist)


LAYOUT_GAP_KEEP = 0.6
LayoutReciprocal = collections.namedtuple("LayoutReciprocal", "max_gap options backs rules")


@functools.lru_cache(maxsize=None)
def layout_reciprocal(side, nr, batch, zero):
    """layout_scene with the reciprocal rule between its rejection and its trimming, from the oracle alone: max_gap accepts
    LAYOUT_GAP_KEEP of registration 0's candidates (reciprocal_ref.pick_gap), the options, and per registration the oracle's back
    search at _t0 () — every fixed point a query, the invalid ones at the origin included — and composed_rule's result."""
    sc = layout_scene(side, nr, batch, zero)
    backs = [back_at(("layout", side, nr, batch, zero, b), F, M, sc.T, nr) for b, (F, M) in enumerate(sc.pairs)]
    max_gap = reciprocal_ref.pick_gap(sc.wants[0][0]["id"], backs[0][0][0]["id"], sc.PM[0], sc.rules[0].W0, keep=LAYOUT_GAP_KEEP)
    o = sc.options._replace(max_gap=max_gap)
    rules = [composed_rule(w[0], pf, pm, F, M, None, None, None, o, back=back)
             for (F, M), w, pf, pm, back in zip(sc.pairs, sc.wants, sc.PF, sc.PM, backs)]
    return LayoutReciprocal(max_gap, o, backs, rules)


def origin_rows(X):
    return (X[:, :3] == 0).all(axis=1)


def layout_reciprocal_conditions(words, finals, counted, origin_share, what):
    """What keeps the layout test of the reciprocal rule from passing vacuously, on the values given (the oracle's in
    tests/test_reciprocal_cpu.py, the device's in tests/test_gpu_reciprocal.py): per registration words = ICP_MEM_RECIPROCAL's
    (n, exact, near, accepted), finals = the size of the final set, counted = the points icp_evaluate counts; origin_share = the share
    of back answers that name an origin row of M (None for a scene without holes).  exact and near are each at least 2 % of the
    candidates, accepted is between 40 % and 90 % of them, the final set between 10 % and 90 % of the counted points, the accepted
    counts of a batch are pairwise distinct, and at least 5 % of the back answers of a scene with holes are ties at the origin."""
    for b, (w, final, c) in enumerate(zip(words, finals, counted)):
        n, exact, near, acc = (int(x) for x in w)
        assert n > 0 and 50 * exact >= n and 50 * near >= n, "%s, registration %d: %d candidates, %d exact, %d near" % (what, b, n, exact, near)
        assert 0.4 * n <= acc <= 0.9 * n and acc == exact + near, "%s, registration %d: %d of %d candidates accepted" % (what, b, acc, n)
        assert 0.1 * c <= final <= 0.9 * c, "%s, registration %d: the final set holds %d of %d counted points" % (what, b, final, c)
    accepted = [int(w[3]) for w in words]
    assert len(set(accepted)) == len(accepted), "%s: the accepted counts of the batch are not pairwise distinct: %r" % (what, accepted)
    if origin_share is not None:
        assert origin_share >= 0.05, "%s: %.3f of the back answers name an origin row of M" % (what, origin_share)


# ---- 7. the reciprocal rule's own scenes ---------------------------------------------------------------------------------------------

def converged_pairs():
    """Three registrations for one handle at (128, 64): batch0's F as both frames — at the identity every valid point finds itself at
    distance 0 in both directions, so a checked run is done with it at k = 1 —, then batch1 and batch2."""
    s = [route_scene(n) for n in ROUTE_BATCH]
    return [(s[0].F, s[0].F), (s[1].F, s[1].M), (s[2].F, s[2].M)]


def messy_moving(engine, side, seed):
    """(F, M, the clean M): synth_pair with M treated as messy_grid treats F — contiguous and scattered holes, ten NaN, ten +inf and ten
    -inf coordinates, ten more points at the origin."""
    F, clean = engine.synth_pair(side, seed=seed)
    M = punch_cloud(engine, clean.copy(), side, seed)
    rng = np.random.default_rng(seed)
    idx = rng.choice(side * side, 40, replace=False)
    M[idx[:10], 0] = np.nan
    M[idx[10:20], 1] = np.inf
    M[idx[20:30], 2] = -np.inf
    M[idx[30:], :3] = 0.0
    return F, M, clean


MessyScene = collections.namedtuple("MessyScene", "F M clean T max_dist max_gap want back finite PF PM W0 rule")
MESSY_SHAPES = [(50, 4), (64, 64)]


@functools.lru_cache(maxsize=None)
def messy_scene(side, nr):
    """A pair whose moving frame — the back search's database — has non-finite rows, from the oracle alone: T = _t0 (), max_dist by
    pick_max_dist on the clean pair, max_gap the 40 % quantile of the non-exact gaps, the oracle's forward and back search, the rows
    of M that are finite, PF / PM, the weights behind the search's rejection (a non-finite row has +0 there: its geo is no number
    <= max_dist^2) and reciprocal_rule's (exact, near, zero, words)."""
    import icp_amd as engine
    from oracle import oracle
    F, M, clean = messy_moving(engine, side, 0x5EED + side)
    T = _t0()
    max_dist = float(np.float32(pick_max_dist(oracle, F, clean, T, nr)))
    want = oracle_search(oracle, F, M, T, nr)
    for a in (F, M, clean, T):
        a.flags.writeable = False
    back = back_at(("messy", side, nr), F, M, T, nr)
    finite = np.isfinite(M[:, :3]).all(axis=1)
    PF, PM = np.ascontiguousarray(F[want[0]["id"]]), oracle.transform_q(M, T)
    with np.errstate(all="ignore"):
        W0 = weights_before_trim(want[0], M, PF, PM, True, True, max_dist)
        max_gap = float(np.float32(np.quantile(reciprocal_ref.gaps(want[0]["id"], back[0][0]["id"], PM, W0), 0.4)))
        rule = reciprocal_ref.reciprocal_rule(want[0]["id"], back[0][0]["id"], PM, W0, max_gap, back[1])
    return MessyScene(F, M, clean, T, max_dist, max_gap, want, back, finite, PF, PM, W0, rule)


def messy_conditions(finite, W0, rev_ids, words, what):
    """30 rows of M are not finite; none of them is a candidate; no back answer names one; the rule has exact, near and rejected pairs."""
    m = finite.shape[0]
    assert np.count_nonzero(~finite) == 30 and not W0[~finite].any(), "%s: a non-finite row is no candidate" % what
    assert (rev_ids < m).all() and finite[rev_ids].all(), "%s: %d back answers name a non-finite row" % (what, np.count_nonzero(~finite[np.minimum(rev_ids, m - 1)]))
    n, exact, near, acc = (int(x) for x in words)
    assert n == np.count_nonzero(W0) and 50 * exact >= n and 50 * near >= n and acc == exact + near and 0.2 * n <= acc <= 0.9 * n, (what, words)
