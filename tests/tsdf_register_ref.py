"""A cloud registered against the TSDF volume itself, restated in numpy (the rule of include/icp_amd.h: icp_tsdf_register).  The samples
are tsdf_ref.sample's fp32; the 29 terms, both halving trees, the LDL^T (p2pl_ref.ldlt_solve) and the step are float64 in the stated
order.  A plain module: it collects no tests."""
import functools
import math

import numpy as np

import rgbd_ref

import p2pl_ref as P
import tsdf_ref as T

F32 = np.float32
BLOCK, TERMS, MAX_N = 256, 29, 1 << 20
ANGLE_THRESHOLD, TRANSLATION_THRESHOLD = 0.001, 0.01


class Record:
    def __init__(self, pose, iterations, converged, singular, members, rmse, sys):
        self.pose, self.iterations, self.converged, self.singular = pose, iterations, converged, singular
        self.members, self.rmse, self.sys = members, rmse, sys


def point_terms(vol, cloud, R, t):
    """(terms (n, 29) float64, member (n,) bool) of the points at the pose R (3, 3), t (3,) float32."""
    c = vol.cfg
    xyz = [np.ascontiguousarray(cloud[:, a], F32) for a in range(3)]
    valid = ~((xyz[0] == 0) & (xyz[1] == 0) & (xyz[2] == 0))
    with np.errstate(all="ignore"):
        w = T._world(R, t, xyz)
        vx = F32(c["voxel"])
        member, S = T.sample(vol, w)
        member = member & valid
        G = []
        for a in range(3):
            wp, wm = list(w), list(w)
            wp[a], wm[a] = w[a] + vx, w[a] - vx
            kp, sp = T.sample(vol, wp)
            km, sm = T.sample(vol, wm)
            member &= kp & km
            G.append(sp - sm)
        member &= np.abs(S) < F32(1)
        mu, voxel = float(F32(c["mu"])), float(vx)
        r = -(mu * S.astype(np.float64))
        kg = mu / (voxel + voxel)
        g = [G[a].astype(np.float64) * kg for a in range(3)]
        wd = [w[a].astype(np.float64) for a in range(3)]
        J = [wd[1] * g[2] - wd[2] * g[1], wd[2] * g[0] - wd[0] * g[2], wd[0] * g[1] - wd[1] * g[0], g[0], g[1], g[2]]
        out = np.zeros((cloud.shape[0], TERMS))
        k = 0
        for a in range(6):
            for b in range(a, 6):
                out[:, k] = J[a] * J[b]
                k += 1
        for a in range(6):
            out[:, 21 + a] = J[a] * r
        out[:, 27] = 1.0
        out[:, 28] = r * r
    out[~member] = 0.0
    return out, member


def reduce_terms(terms):
    """The 29 sums: the halving tree inside blocks of 256 points, then over the block partials zero-padded to a power of two."""
    n = terms.shape[0]
    nblk = -(-n // BLOCK)
    x = np.zeros((nblk * BLOCK, TERMS))
    x[:n] = terms
    part = P._halve(x.reshape(nblk, BLOCK, TERMS))
    size = 1
    while size < nblk:
        size *= 2
    y = np.zeros((size, TERMS))
    y[:nblk] = part
    return P._halve(np.ascontiguousarray(y.T))


def step(R, t, x):
    """(R', t', Tk) of the increment x = (omega, tau) at R (3, 3), t (3,) float32."""
    hx, hy, hz = x[0] * 0.5, x[1] * 0.5, x[2] * 0.5
    inv = 1.0 / math.sqrt(((hx * hx + hy * hy) + hz * hz) + 1.0)
    qx, qy, qz, qw = hx * inv, hy * inv, hz * inv, inv
    dR = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
          [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
          [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]]
    Rd, td = [[float(v) for v in row] for row in R], [float(v) for v in t]
    Rn, tn = np.zeros((3, 3), F32), np.zeros(3, F32)
    for a in range(3):
        for b in range(3):
            Rn[a, b] = F32((dR[a][0] * Rd[0][b] + dR[a][1] * Rd[1][b]) + dR[a][2] * Rd[2][b])
        tn[a] = F32(((dR[a][0] * td[0] + dR[a][1] * td[1]) + dR[a][2] * td[2]) + x[3 + a])
    return Rn, tn, np.array([qx, qy, qz, qw, x[3], x[4], x[5], 1.0], F32)


def register(vol, cloud, pose12, max_iterations=20, angle_threshold=None, translation_threshold=None):
    """icp_tsdf_register: a Record."""
    ang = ANGLE_THRESHOLD if angle_threshold is None else angle_threshold
    tra = TRANSLATION_THRESHOLD if translation_threshold is None else translation_threshold
    cloud = np.asarray(cloud, F32)
    assert 1 <= cloud.shape[0] <= MAX_N
    R, t = (a.copy() for a in T._pose(pose12))
    k, converged, singular, members, rmse, sys = 0, False, False, 0, 0.0, np.zeros(27)
    for _ in range(max_iterations):
        s = reduce_terms(point_terms(vol, cloud, R, t)[0])
        x, ok = P.ldlt_solve(s[:27])
        members, sys = int(s[27]), s[:27].copy()
        rmse = math.sqrt(s[28] / s[27]) if s[27] > 0 else 0.0
        if not ok or not s[27] > 0:
            singular = True
            break
        R, t, Tk = step(R, t, x)
        k += 1
        if P.check_converged(Tk, ang, tra):
            converged = True
            break
    pose = np.concatenate([R, t[:, None]], 1).reshape(12).astype(F32)
    return Record(pose, k, converged, singular, members, rmse, sys)


def track_to_volume(vol, cam, frames, pose0, lattice, max_iterations=20):
    """icp_amd.tsdf.track_to_volume on the restatement: `lattice` (depth, rgb) gives the landmarks the front end writes into M.
    [(pose, Record or None)]; the volume is integrated in place."""
    pose = np.asarray(pose0, F32).reshape(12).copy()
    out = []
    for i, (depth, rgb) in enumerate(frames):
        rec = None
        if i:
            rec = register(vol, lattice(depth, rgb), pose, max_iterations)
            pose = rec.pose.copy()
        T.integrate(vol, cam, pose, depth, rgb)
        out.append((pose.copy(), rec))
    return out


# ---- the scenes the CPU and the GPU tests share --------------------------------------------------------------------------------------

def p12(P):
    return np.ascontiguousarray(P, np.float64).reshape(12).astype(F32)


def pose_errors(pose12, P_true):
    P = np.asarray(pose12, np.float64).reshape(3, 4)
    c = (np.trace(P[:, :3].T @ P_true[:, :3]) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.linalg.norm(P[:, 3] - P_true[:, 3]))


@functools.lru_cache(maxsize=None)
def corner():
    cam = T.corner_camera()
    vol, _ = T.fuse_corner(T.corner_volume(), cam)
    vol.dw.flags.writeable = False
    return cam, vol


def frame_cloud(P_true):
    cam, _ = corner()
    depth, rgb = T.render_corner(P_true, cam)[:2]
    return rgbd_ref.cloud(depth, rgb, cam)


START = T.look_at(T.EYE_CAST)
TRUE_1 = T.rotate_pose(START, (0.3, 1.0, 0.2), 1.0, (8, -5, 3))
TRUE_5 = T.rotate_pose(START, (0.3, 1.0, 0.2), 5.0, (40, -30, 20))


def plane_volume(n=16, mu=4.0, z0=7.3):
    """D = clamp ((z - z0) / mu), W = 1: one axis-aligned plane, voxels of 1 from the origin."""
    vol = T.Volume(T.volume_config(n, n, n, 1.0, (0.0, 0.0, 0.0), mu))
    k = np.arange(n, dtype=F32)[:, None, None]
    vol.dw[..., 0] = np.clip((k - F32(z0)) / F32(mu), -1, 1)
    vol.dw[..., 1] = 1
    return vol


IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)


def points(xyz):
    c = np.zeros((len(xyz), 8), F32)
    c[:, :3] = xyz
    c[:, 3] = c[:, 7] = 1
    return c


def edge_points(n=16):
    """(name, xyz, member) at the edges of the membership rule of plane_volume (n) with the hole and the exact values written by
    edge_volume: the centre's cell needs 1 <= floor <= n - 3 on every axis for its six offset samples to have cells."""
    return [("inside", (6.5, 6.5, 7.5), True),
            ("the last cell with all offsets", (n - 2.5, 6.5, 7.5), True),
            ("centre in the last cell of x: the +x sample has none", (n - 1.5, 6.5, 7.5), False),
            ("one voxel beyond", (n - 0.5, 6.5, 7.5), False),
            ("centre in the first cell of y: the -y sample has none", (6.5, 0.5, 7.5), False),
            ("a W == 0 corner in the -x sample only", (4.5, 10.5, 7.5), False),
            ("the same cell row one further: all known", (5.5, 10.5, 7.5), True),
            ("S exactly +1", (6.5, 6.5, 12.0), False),
            ("S exactly -1", (6.5, 6.5, 3.0), False),
            ("S just inside", (6.5, 6.5, 10.5), True),
            ("NaN", (np.nan, 6.5, 7.5), False), ("+inf", (6.5, np.inf, 7.5), False), ("-inf", (6.5, 6.5, -np.inf), False),
            ("the invalid point", (0.0, 0.0, 0.0), False), ("minus zeros", (-0.0, -0.0, -0.0), False),
            ("one minus zero", (6.5, -0.0, 7.5), False)]


def edge_volume(n=16):
    vol = plane_volume(n)
    vol.dw[7, 10, 3, 1] = 0             # voxel (3, 10, 7): a corner of the cell of (3.5, 10.5, 7.5) only
    vol.dw.flags.writeable = False
    return vol
