"""The registration of a cloud against the TSDF volume itself (include/icp_amd.h: icp_tsdf_register) as tests/tsdf_register_ref.py restates
it, held against the analytic corner scene of tsdf_ref.py and at the edges of its membership rule.  No device."""
import numpy as np

import tsdf_ref as T
import tsdf_register_ref as G
from tsdf_register_ref import (IDENTITY, START, TRUE_1, TRUE_5, p12 as _p12, corner, edge_points, edge_volume, frame_cloud, plane_volume, points,
                               pose_errors)

F32 = np.float32


def test_one_degree_pair():
    """The 1 degree / 9.9 mm pair at 64^3: at least 0.8 of the 4800 points are members in the first iteration, and five iterations end
    within 0.1 degrees and 1.0 mm of the truth (three times what the float64 prototype of the rule reached, 0.037 degrees / 0.32 mm).
    The restatement has 4452 members in the first iteration and reaches 0.0359 degrees / 0.319 mm after five (rmse 1.135)."""
    _, vol = corner()
    cloud = frame_cloud(TRUE_1)
    assert cloud.shape[0] == 4800
    first = G.register(vol, cloud, _p12(START), 1)
    assert first.members >= 0.8 * 4800, first.members
    rec = G.register(vol, cloud, _p12(START), 5, 0.0, 0.0)
    rot, tra = pose_errors(rec.pose, TRUE_1)
    print("1 degree pair: members %d of 4800, after 5 iterations %.4f degrees %.3f mm, rmse %.3f" % (first.members, rot, tra, rec.rmse))
    assert rec.iterations == 5 and not rec.singular
    assert rot < 0.1 and tra < 1.0, (rot, tra)


def test_five_degree_pair():
    """The 5 degree / 54 mm pair: within 0.1 degrees / 1.0 mm after 12 iterations (the prototype: 0.024 degrees / 0.21 mm).  The restatement
    reaches 0.0235 degrees / 0.213 mm."""
    _, vol = corner()
    rec = G.register(vol, frame_cloud(TRUE_5), _p12(START), 12, 0.0, 0.0)
    rot, tra = pose_errors(rec.pose, TRUE_5)
    print("5 degree pair: after 12 iterations %.4f degrees %.3f mm" % (rot, tra))
    assert rot < 0.1 and tra < 1.0, (rot, tra)


def test_one_plane_is_singular():
    """G_x and G_y are exact zeros on an axis-aligned plane: three pivots are 0.  Singular, the pose unchanged bit for bit, no iteration."""
    vol = plane_volume()
    rng = np.random.default_rng(2)
    cloud = points(np.stack([rng.uniform(3, 12, 200), rng.uniform(3, 12, 200), rng.uniform(5, 9, 200)], 1))
    terms, member = G.point_terms(vol, cloud, *T._pose(IDENTITY))
    assert member.sum() > 100 and np.all(terms[:, 9] == 0) and np.all(terms[:, 15] == 0)       # J_3 J_3 and J_4 J_4: g_x g_x, g_y g_y
    pose = IDENTITY.copy(); pose[3] = 0.25
    rec = G.register(vol, cloud, pose, 5)
    assert rec.singular and not rec.converged and rec.iterations == 0 and rec.members == member.sum() and rec.rmse > 0
    assert np.array_equal(rec.pose.view(np.uint32), pose.view(np.uint32))


def test_no_members():
    vol = plane_volume()
    rec = G.register(vol, points([[100.0, 3.0, 3.0], [-5.0, 2.0, 2.0], [3.0, 3.0, 50.0]]), IDENTITY, 3)
    assert rec.singular and rec.members == 0 and rec.rmse == 0.0 and rec.iterations == 0 and not np.any(rec.sys)
    assert np.array_equal(rec.pose.view(np.uint32), IDENTITY.view(np.uint32))


def test_membership_at_its_edges():
    vol = edge_volume()
    cases = edge_points()
    cloud = points([c[1] for c in cases])
    Rm, t = T._pose(IDENTITY)
    terms, member = G.point_terms(vol, cloud, Rm, t)
    for (name, xyz, want), got in zip(cases, member):
        assert bool(got) == want, (name, xyz)
    assert np.all(np.isfinite(terms)) and not np.any(terms[~member])
    assert np.all(terms[member, 27] == 1.0)
    # the exact values: S = +1 and -1 at z = 12 and z = 3 (z0 = 7.3, mu = 4: clipped well before), and the hole is in one sample only
    known, S = T.sample(vol, [cloud[:, a] for a in range(3)])
    at = {c[0]: i for i, c in enumerate(cases)}
    assert S[at["S exactly +1"]] == 1 and S[at["S exactly -1"]] == -1 and known[at["S exactly +1"]] and abs(S[at["S just inside"]]) < 1
    assert known[at["a W == 0 corner in the -x sample only"]]
    # the sums see the members only
    s = G.reduce_terms(terms)
    assert s[27] == member.sum()


def test_convergence_flags():
    _, vol = corner()
    cloud = frame_cloud(TRUE_1)
    big = G.register(vol, cloud, _p12(START), 20, 5.0, 100.0)              # thresholds above the first step's size
    assert big.converged and big.iterations == 1 and not big.singular
    short = G.register(vol, cloud, _p12(START), 2, 0.0, 0.0)
    assert not short.converged and short.iterations == 2 and not short.singular


def test_trees_are_the_plane_systems():
    """reduce_terms over 29 columns is p2pl_ref.reduce_terms column by column (257 blocks: a padded tree)."""
    import p2pl_ref as P
    rng = np.random.default_rng(5)
    x = rng.normal(size=(65537, 29))
    want = P.reduce_terms(x[:, :27])
    got = G.reduce_terms(x)
    assert np.array_equal(got[:27], want)
