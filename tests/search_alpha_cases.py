"""The search over the whole range of alpha — TEST INFRASTRUCTURE (a plain module: pytest collects nothing from it): the alphas, the
scenes and the oracle's searches that tests/test_gpu_search_alpha.py compares the engine with and tests/test_search_alpha_cpu.py proves
the premises of.  Everything here comes from the CPU oracle alone and is computed once per session.

The alphas, by name (every one is a float32; icp_set_alpha refuses 0, NaN and +-inf only):
  neg_winners  negative and large: a quarter and more of the winning distances d = fma (a, pho, geo) are below zero, the others above.
               The order of negative floats is not the order of their bits, which is what a reduction over (distance bits, position) keys
               has to get right;
  neg_small    negative, with hardly a winner below zero: the search's pruning (it rests on d >= geo) is off — the `a > 0` tests — and
               nothing else differs;
  tiny, denormal   a pho vanishes beside geo: the invalid points of a frame (all at the origin) tie geometrically, and the tie rule
               (lowest index) decides their queries;
  huge         a pho overflows for part of the candidates: a query's distances are +inf unless a colour is near enough, "a nearest
               distance that is not below +inf names no representative", seeds and bounds of +inf.  The synthetic frames' colours lie in
               [0.05, 0.95]: pho stays below 3, a pho overflows for no float a, and at 1e30 every distance is finite.  The huge case
               therefore runs the same frames with their colours on the 8-bit scale of a capture (times 255, HUGE_COLOUR_SCALE), and takes
               its alpha by the grid's side (HUGE_BY_SIDE: a denser grid has nearer colours): the values at which part of the queries have
               no finite distance and part have one.  tests/test_search_alpha_cpu.py asserts both shares on every scene.

A Scene is a pair of frames with a representative count; a Case is what one GPU test runs: the scenes of a handle (one per registration
of the batch), the reduction mode and the layout the handle must report."""
import collections
import functools

import numpy as np

import icp_checks

F32 = np.float32
HUGE_COLOUR_SCALE = F32(255.0)
HUGE_BY_SIDE = {32: 3e36, 64: 1e37, 128: 3e37, 256: 1e38}
ALPHAS = collections.OrderedDict([("neg_winners", -1e5), ("neg_small", -1e-3), ("tiny", 1e-30), ("denormal", 1e-40), ("huge", None)])


def alpha_of(name, side):
    """The alpha of case `name` on a grid `side` wide, as the float32 the engine stores."""
    return float(F32(HUGE_BY_SIDE[side] if name == "huge" else ALPHAS[name]))


assert 0 < alpha_of("denormal", 0) < float(np.finfo(F32).tiny), "a float32 denormal"
TIE_ALPHAS = ("tiny", "denormal")

Scene = collections.namedtuple("Scene", "side nr kind b zf")
Scene.__doc__ = """kind "synth": engine.synth_pair (side, seed = 0x1C9D5EED + 11 b, rot_deg = 3 - 0.75 b, zero_fraction = zf) — the pairs of
test_stage2_lanes_as_candidates —;  kind = a name of workloads.HOLES: workloads.holes_pair (engine, kind, side)."""
Case = collections.namedtuple("Case", "name scenes fused layout chained env")
Case.__doc__ = """scenes: one Scene per registration of the handle;  fused: the reduction mode (and the squared power start with it);
layout: what search_layout () must report;  chained: what run_form () must report;  env: ICP_AMD_S2WAVE for icp_init, or None."""

LATENCY, LANES_256, WAVE_256, LANES_1024 = (0, 1024, 0), (1, 256, 0), (1, 256, 1), (1, 1024, 0)


def _synth(side, nr, batch=1, zf=0.0):
    return tuple(Scene(side, nr, "synth", b, zf) for b in range(batch))


def _cases():
    out = [Case("latency-32x16", _synth(32, 16), True, LATENCY, 1, None),
           Case("latency-128x256", _synth(128, 256), True, LATENCY, 1, None),
           Case("latency-128x256-reference-order", _synth(128, 256), False, LATENCY, 0, None)]
    # the dense shapes (side, nr, batch, layout), clean and once more with 10 % identical invalid points in both frames
    dense = [("single-lanes-64x64x9", 64, 64, 9, LANES_256), ("single-wave-128x64x3", 128, 64, 3, WAVE_256),
             ("masked-lanes-128x1024", 128, 1024, 1, LANES_256), ("masked-lanes-256x1024", 256, 1024, 1, LANES_256),
             ("masked-wave-256x512", 256, 512, 1, WAVE_256), ("tile1024-lanes-256x8192", 256, 8192, 1, LANES_1024)]
    for zf in (0.0, 0.1):
        for name, side, nr, batch, layout in dense:
            out.append(Case(name + ("-zeros" if zf else ""), _synth(side, nr, batch, zf), True, layout, 0, None))
        out.append(Case("masked-wave-256x512-reference-order" + ("-zeros" if zf else ""), _synth(256, 512, 1, zf), False, WAVE_256, 0, None))
    # one list of about 20 000 identical points (ks_list_tail with and without bounds) in both forms of stage 2, and the same holes with
    # their colours kept: the origin list's colour boxes and explicit tie rule
    holes = (Scene(256, 1024, "blobs30_rgb0", 0, 0.0),)
    out.append(Case("holes-rgb0-lanes-256x1024", holes, True, LANES_256, 0, None))
    out.append(Case("holes-rgb0-wave-256x1024", holes, True, WAVE_256, 0, "1"))
    out.append(Case("holes-colour-lanes-256x1024", (Scene(256, 1024, "blobs30", 0, 0.0),), True, LANES_256, 0, None))
    return out


CASES = _cases()
SCENES = sorted({s for c in CASES for s in c.scenes})
INVALID_SCENES = [s for s in SCENES if s.zf or s.kind != "synth"]          # the scenes with invalid points


def frames(scene, name=None):
    """(F, M) of the scene as alpha case `name` sees it (the huge case: colours times HUGE_COLOUR_SCALE), read-only."""
    return _frames(scene, name == "huge")


@functools.lru_cache(maxsize=64)
def _frames(scene, scaled):
    import icp_amd as engine
    from icp_amd import workloads as W
    if scene.kind == "synth":
        F, M = engine.synth_pair(scene.side, seed=0x1C9D5EED + 11 * scene.b, rot_deg=3.0 - 0.75 * scene.b, zero_fraction=scene.zf)
    else:
        F, M = W.holes_pair(engine, scene.kind, scene.side)
    if scaled:
        F[:, 4:7] *= HUGE_COLOUR_SCALE
        M[:, 4:7] *= HUGE_COLOUR_SCALE
    F.flags.writeable = False
    M.flags.writeable = False
    return F, M


@functools.lru_cache(maxsize=None)
def transforms(scene):
    """The three transforms every search is teacher-forced with: the identity, icp_checks._t0 () and the T the oracle reaches after three
    steps at alpha = 200 (the benchmarked modes) on the scene — queries near their partners, where ties and small distances are."""
    from oracle import oracle
    F, M = frames(scene)
    o = oracle.OracleICP(F.shape[0], scene.nr, icp_checks.A, icp_checks.C_, threads=8, power_fast=True, fused=True)
    o.write_f(F); o.write_m(M); o.build_rbc()
    for _ in range(3):
        o.step()
    T3 = o.T
    assert np.isfinite(T3).all(), (scene, T3)
    return (np.array(icp_checks.IDENTITY), icp_checks._t0(), T3)


Searched = collections.namedtuple("Searched", "reps owner N O perm steps")
Searched.__doc__ = """The oracle at one alpha case on one scene: the RBC structure (what check_rbc compares) and, per transform of transforms (),
(nn_id, rid) of the serial scan."""


class _Rbc:
    """What icp_checks.check_rbc reads of an OracleICP."""

    def __init__(self, s):
        self.reps, self.rbc_owner, self.rbc_N, self.rbc_O, self.rbc_perm = s.reps, s.owner, s.N, s.O, s.perm


@functools.lru_cache(maxsize=64)
def searched(scene, name):
    """The oracle's construction and its three teacher-forced searches at the alpha of case `name` (REGULAR weights: nothing behind the search depends on
    the distances, and nothing behind the search is compared)."""
    from oracle import oracle
    F, M = frames(scene, name)
    o = oracle.OracleICP(F.shape[0], scene.nr, alpha_of(name, scene.side), icp_checks.C_, weighted=icp_checks.REGULAR, threads=8)
    o.write_f(F); o.write_m(M); o.build_rbc()
    steps = []
    for T in transforms(scene):
        o.write_t(T)
        o.step()
        steps.append((o.nn_id, o.rid))
    out = Searched(o.reps, o.rbc_owner, o.rbc_N, o.rbc_O, o.rbc_perm, tuple(steps))
    for a in out[:5] + tuple(x for st in steps for x in st):
        a.flags.writeable = False
    return out


def rbc_of(scene, name):
    return _Rbc(searched(scene, name))


def tie_queries(scene, name, step):
    """The queries of search `step` whose scanned list holds two candidates with bit-equal minimal distance: the list scanned in
    DESCENDING position (oracle.nn_brute over the reversed list: a strict '<', so the highest position among equals) names another member
    than the serial scan.  A query with an empty list, or without a distance below +inf, is none."""
    from oracle import oracle
    F, M = frames(scene, name)
    s, alpha = searched(scene, name), alpha_of(name, scene.side)
    nn_id, rid = s.steps[step]
    Q = oracle.transform_q(M, transforms(scene)[step])
    XP = np.ascontiguousarray(F[s.perm])
    tie = np.zeros(F.shape[0], bool)
    order = np.argsort(rid, kind="stable")
    bounds = np.searchsorted(rid[order], np.arange(scene.nr + 1))
    for r in np.unique(rid):
        n, o = int(s.N[r]), int(s.O[r])
        if n < 2:
            continue
        q = order[bounds[r]:bounds[r + 1]]
        back = oracle.nn_brute(np.ascontiguousarray(Q[q]), np.ascontiguousarray(XP[o:o + n][::-1]), alpha)
        last = s.perm[o + n - 1 - back["id"].astype(np.int64)]
        tie[q] = (last != nn_id["id"][q]) & (nn_id["dist"][q] < np.inf)
    return tie
