"""The TSDF volume restated in numpy (the rule of include/icp_amd.h: icp_tsdf_t, icp_tsdf_integrate, icp_tsdf_raycast), and a float64
analytic renderer of a room corner to hold that rule against.

Everything of the rule is float32 with each operation on its own (numpy fuses nothing), as icp_tsdf.hip evaluates it with
-ffp-contract=off; dots are (a0 b0 + a1 b1) + a2 b2.  A volume here is the logical layout icp_tsdf_read exchanges: dw (nz, ny, nx, 2)
and rgb (nz, ny, nx, 3).  A camera is an rgbd_ref.config dict.  A plain module: it collects no tests."""
import numpy as np

from rgbd_ref import valid_counts

F32 = np.float32


def volume_config(nx, ny, nz, voxel, origin, mu, w_max=64.0, colour=0):
    return dict(nx=nx, ny=ny, nz=nz, voxel=voxel, origin=tuple(origin), mu=mu, w_max=w_max, colour=colour)


# every out-of-range field of icp_tsdf_t (the refusal tests, CPU and GPU, go through them)
BAD_FIELDS = [("nx", 1), ("nx", 1025), ("ny", 0), ("ny", 1025), ("nz", 1), ("nz", 4096), ("voxel", 0.0), ("voxel", -1.0), ("voxel", float("inf")),
              ("voxel", float("nan")), ("origin", (0.0, float("nan"), 0.0)), ("origin", (float("inf"), 0.0, 0.0)), ("mu", 0.0), ("mu", float("nan")),
              ("mu", float("inf")), ("w_max", 0.0), ("w_max", 1.5), ("w_max", 65537.0), ("w_max", float("nan")), ("colour", 2)]


class Volume:
    def __init__(self, cfg):
        self.cfg = dict(cfg)
        self.dw = np.zeros((cfg["nz"], cfg["ny"], cfg["nx"], 2), F32)
        self.rgb = np.zeros((cfg["nz"], cfg["ny"], cfg["nx"], 3), F32) if cfg["colour"] else None


def _pose(pose12):
    P = np.asarray(pose12, F32).reshape(3, 4)
    return P[:, :3], P[:, 3]


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def integrate(vol, cam, pose12, depth, rgb=None):
    """One frame into the volume, in place.  Returns the voxel classes as boolean (nz, ny, nx) arrays: behind (q_z <= 0), outside
    (of the image), invalid (count), occluded (s < -mu), front (e = 1, changed), changed."""
    c = vol.cfg
    R, t = _pose(pose12)
    vx, mu, wmax = F32(c["voxel"]), F32(c["mu"]), F32(c["w_max"])
    idx = [np.arange(c[n], dtype=F32) for n in ("nx", "ny", "nz")]
    p = [F32(c["origin"][a]) + idx[a] * vx for a in range(3)]
    d = [p[0][None, None, :] - t[0], p[1][None, :, None] - t[1], p[2][:, None, None] - t[2]]
    q = [_dot3(R[0, a], d[0], R[1, a], d[1], R[2, a], d[2]) for a in range(3)]
    front_of_camera = q[2] > 0
    H, Wd = cam["height"], cam["width"]
    with np.errstate(all="ignore"):
        u = (F32(cam["fx"]) * (q[0] / q[2]) + F32(cam["cx"])) + F32(0.5)
        v = (F32(cam["fy"]) * (q[1] / q[2]) + F32(cam["cy"])) + F32(0.5)
        inside = front_of_camera & (u >= 0) & (u < F32(Wd)) & (v >= 0) & (v < F32(H))
        px = np.where(inside, np.floor(u), 0).astype(np.int64)
        py = np.where(inside, np.floor(v), 0).astype(np.int64)
    cnt = np.asarray(depth).reshape(H, Wd)
    ok = valid_counts(cnt, cam)
    seen = inside & ok[py, px]
    z = cnt[py, px].astype(F32) * F32(cam["depth_scale"])
    s = z - q[2]
    changed = seen & (s >= -mu)
    with np.errstate(all="ignore"):
        e = np.minimum(F32(1), s / mu)
    D, Wt = vol.dw[..., 0], vol.dw[..., 1]
    W1 = Wt + F32(1)
    vol.dw[..., 0] = np.where(changed, (D * Wt + e) / W1, D)
    if c["colour"] and rgb is not None:
        col = np.asarray(rgb, np.uint8).reshape(H, Wd, 3)[py, px].astype(F32) / F32(255)
        vol.rgb[...] = np.where(changed[..., None], (vol.rgb * Wt[..., None] + col) / W1[..., None], vol.rgb)
    vol.dw[..., 1] = np.where(changed, np.minimum(W1, wmax), Wt)
    return dict(behind=~front_of_camera, outside=front_of_camera & ~inside, invalid=inside & ~seen, occluded=seen & ~changed,
                front=changed & (e == 1), changed=changed)


def _lerp(a, b, t):
    return a + t * (b - a)


def sample(vol, w, colour=False):
    """S at the world points w = (x, y, z) arrays: (known, value) and, with colour, the (.., 3) trilinear colour of the same cell."""
    c = vol.cfg
    vx = F32(c["voxel"])
    n = (c["nx"], c["ny"], c["nz"])
    with np.errstate(all="ignore"):
        g = [(w[a] - F32(c["origin"][a])) / vx for a in range(3)]
        fl = [np.floor(g[a]) for a in range(3)]
        cell = np.ones(g[0].shape, bool)
        for a in range(3):
            cell &= (fl[a] >= 0) & (fl[a] <= F32(n[a] - 2))
        i = [np.where(cell, fl[a], 0).astype(np.int64) for a in range(3)]
        f = [g[a] - fl[a] for a in range(3)]
    known = cell.copy()
    cor = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                rec = vol.dw[i[2] + dz, i[1] + dy, i[0] + dx]
                known &= rec[..., 1] > 0
                cor[dx, dy, dz] = rec[..., 0]

    def tri(v, f):
        with np.errstate(all="ignore"):
            c00, c10 = _lerp(v[0, 0, 0], v[1, 0, 0], f[0]), _lerp(v[0, 1, 0], v[1, 1, 0], f[0])
            c01, c11 = _lerp(v[0, 0, 1], v[1, 0, 1], f[0]), _lerp(v[0, 1, 1], v[1, 1, 1], f[0])
            return _lerp(_lerp(c00, c10, f[1]), _lerp(c01, c11, f[1]), f[2])

    val = tri(cor, f)
    if not colour:
        return known, val
    col = np.zeros(g[0].shape + (3,), F32)
    if vol.rgb is not None:
        for ch in range(3):
            col[..., ch] = tri({k: vol.rgb[i[2] + k[2], i[1] + k[1], i[0] + k[0], ch] for k in cor}, f)
    return known, val, col


def march_trips(mu, z_near, z_far):
    """N of the rule (the march makes N + 1 samples); the call is refused unless it is <= 4095."""
    return int(np.floor((F32(z_far) - F32(z_near)) / (F32(0.5) * F32(mu))))


def _world(R, t, x):
    return [_dot3(R[a, 0], x[0], R[a, 1], x[1], R[a, 2], x[2]) + t[a] for a in range(3)]


def raycast(vol, cam, pose12, z_near, z_far, side=0, info=None):
    """(cloud (n, 8), normals (n, 4), depth lambda* (n,) with nan where there is no hit) of every pixel (side = 0, n = width * height,
    row-major) or of the side x side landmarks of the camera's lattice.  info: a dict that receives, per ray, what the tests' conditions
    on their own inputs ask about: n_star (-1: none), seen_before (a sample before n* was known), prev_known (sample n* - 1 was),
    cross, cell_known (S (h) is), grad_known, lam_exact (lambda* == lambda_{n*} bit for bit)."""
    c = vol.cfg
    R, t = _pose(pose12)
    if side:
        uu = (cam["x0"] + cam["step_x"] * np.arange(side))[None, :].repeat(side, 0).reshape(-1)
        vv = (cam["y0"] + cam["step_y"] * np.arange(side))[:, None].repeat(side, 1).reshape(-1)
    else:
        uu = np.arange(cam["width"])[None, :].repeat(cam["height"], 0).reshape(-1)
        vv = np.arange(cam["height"])[:, None].repeat(cam["width"], 1).reshape(-1)
    uf, vf = uu.astype(F32), vv.astype(F32)
    fx, fy, cx, cy = (F32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    ax, ay = (uf - cx) / fx, (vf - cy) / fy
    delta = F32(0.5) * F32(c["mu"])
    zn = F32(z_near)
    N = march_trips(c["mu"], z_near, z_far)
    assert 0 <= N <= 4095
    n_rays = uu.size
    live = np.ones(n_rays, bool)                       # n* not met yet
    prev_known = np.zeros(n_rays, bool)
    prev_s = np.zeros(n_rays, F32)
    cross = np.zeros(n_rays, bool)
    n_star, seen, seen_before, pk_at = np.full(n_rays, -1), np.zeros(n_rays, bool), np.zeros(n_rays, bool), np.zeros(n_rays, bool)
    s0, s1, lam0 = np.zeros(n_rays, F32), np.zeros(n_rays, F32), np.zeros(n_rays, F32)
    lam_prev = zn
    for n in range(N + 1):
        if not live.any():
            break
        lam = zn + F32(n) * delta
        known, s = sample(vol, _world(R, t, [ax * lam, ay * lam, np.full(n_rays, lam, F32)]))
        stop = live & known & (s <= 0)
        hit = stop & prev_known & (prev_s > 0) & (n >= 1)
        cross |= hit
        n_star[stop], seen_before[stop], pk_at[stop] = n, seen[stop], prev_known[stop]
        seen |= known
        s0 = np.where(hit, prev_s, s0)
        s1 = np.where(hit, s, s1)
        lam0 = np.where(hit, lam_prev, lam0)
        live &= ~stop
        prev_known, prev_s, lam_prev = known, s, lam
    with np.errstate(all="ignore"):
        lam_star = lam0 + delta * (s0 / (s0 - s1))
        X, Y, Z = (uf - cx) * lam_star / fx, (vf - cy) * lam_star / fy, lam_star
    h = _world(R, t, [X, Y, Z])
    known_h, _, col = sample(vol, h, colour=True)
    ok = cross & known_h
    vx = F32(c["voxel"])
    G, grad_known = [], np.ones(n_rays, bool)
    for a in range(3):
        hp, hm = list(h), list(h)
        hp[a], hm[a] = h[a] + vx, h[a] - vx
        kp, sp = sample(vol, hp)
        km, sm = sample(vol, hm)
        grad_known &= kp & km
        G.append(sp - sm)
    with np.errstate(all="ignore"):
        ln = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
        has_n = ok & grad_known & (ln > 0)
        nw = [G[a] / ln for a in range(3)]
        nc = [_dot3(R[0, a], nw[0], R[1, a], nw[1], R[2, a], nw[2]) for a in range(3)]
        flip = _dot3(nc[0], X, nc[1], Y, nc[2], Z) > 0
    if info is not None:
        with np.errstate(all="ignore"):
            lam_n = zn + n_star.astype(F32) * delta
        info.update(n_star=n_star, seen_before=seen_before, prev_known=pk_at, cross=cross, cell_known=known_h, grad_known=grad_known,
                    lam_exact=ok & (lam_star == lam_n))
    cloud = np.zeros((n_rays, 8), F32)
    cloud[:, 3] = cloud[:, 7] = 1
    nrm = np.zeros((n_rays, 4), F32)
    for a, comp in enumerate((X, Y, Z)):
        cloud[:, a] = np.where(ok, comp, F32(0))
        cloud[:, 4 + a] = np.where(ok, col[:, a], F32(0))
        nrm[:, a] = np.where(has_n, np.where(flip, -nc[a], nc[a]), F32(0))
    return cloud, nrm, np.where(ok, lam_star, F32(np.nan))


def compose_pose(pose12, T8):
    """pose o (R (q), t) of the engine's T = [qx qy qz qw | tx ty tz s] in float64, rounded once; (pose12 float32, scale)."""
    P = np.asarray(pose12, np.float64).reshape(3, 4)
    T = np.asarray(T8, np.float64).reshape(8)
    x, y, z, w = T[:4] / np.linalg.norm(T[:4])
    Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    out = np.empty((3, 4))
    out[:, :3] = P[:, :3] @ Rq
    out[:, 3] = P[:, :3] @ T[4:7] + P[:, 3]
    return out.reshape(12).astype(F32), F32(T[7])


# ---- the analytic scene: the room corner x = 0, y = 0, z = 0 seen from the positive octant ---------------------------------------

TARGET = (150.0, 150.0, 150.0)
EYES = ((800, 700, 600), (700, 800, 650), (760, 760, 560), (820, 650, 700), (650, 820, 600), (740, 700, 760))
EYE_CAST = (770, 730, 640)


def corner_camera(width=80, height=60, fx=75.0, cx=39.5, cy=29.5, **kw):
    from rgbd_ref import config
    return config(width=width, height=height, fx=fx, fy=fx, cx=cx, cy=cy, depth_scale=1.0, **kw)


def look_at(eye, target=TARGET, up=(0.0, 0.0, 1.0)):
    """Camera -> world [R | t] (3, 4) float64: z_c looks from eye to target, y_c points down."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    zc = target - eye
    zc /= np.linalg.norm(zc)
    yc = -(up - (up @ zc) * zc)
    yc /= np.linalg.norm(yc)
    xc = np.cross(yc, zc)
    return np.concatenate([np.stack([xc, yc, zc], 1), eye[:, None]], 1)


def rotate_pose(P, axis, degrees, shift):
    """P o (a rotation about `axis` of the camera, then a shift in the camera's frame), float64 (3, 4)."""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    th = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rr = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    out = np.empty((3, 4))
    out[:, :3] = P[:, :3] @ Rr
    out[:, 3] = P[:, :3] @ np.asarray(shift, np.float64) + P[:, 3]
    return out


def render_corner(P, cam):
    """The corner seen through the pinhole camera at pose P (3, 4) float64: depth (H, W) uint16 = rint of the nearest positive ray-plane
    distance along z, rgb (H, W, 3) uint8 a function of the world point, plane (H, W) the index of the plane hit, z (H, W) the exact
    depth, crease (H, W) the distance along z to the second-nearest plane minus z."""
    H, W = cam["height"], cam["width"]
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones_like(u)], -1)
    dw = dc @ P[:, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.where(dw < 0, -P[:, 3] / dw, np.inf)
    order = np.sort(lam, -1)
    z = order[..., 0]
    plane = np.argmin(lam, -1)
    pw = P[:, 3] + dw * z[..., None]
    rgb = np.stack([127.5 + 127.5 * np.sin(pw[..., (a + 1) % 3] / 90.0 + a) * np.cos(pw[..., (a + 2) % 3] / 130.0) for a in range(3)], -1)
    assert z.max() < 65535
    return np.rint(z).astype(np.uint16), np.rint(rgb).astype(np.uint8), plane, z, order[..., 1] - z


def corner_volume(n=64, voxel=16.0, mu=48.0, colour=0, w_max=64.0, dims=None):
    nx, ny, nz = dims or (n, n, n)
    return volume_config(nx, ny, nz, voxel, (-64.0, -64.0, -64.0), mu, w_max, colour)


def fuse_corner(cfg, cam, eyes=EYES, with_rgb=False):
    """The eyes' frames fused into a fresh volume of the restatement; (volume, [pose12 float32])."""
    vol = Volume(cfg)
    poses = []
    for eye in eyes:
        P = look_at(eye)
        depth, rgb, _, _, _ = render_corner(P, cam)
        p12 = P.reshape(12).astype(F32)
        integrate(vol, cam, p12, depth, rgb if with_rgb else None)
        poses.append(p12)
    return vol, poses


def corner_figures(vol, cam, P, z_near=200.0, z_far=1600.0, cast=None):
    """What the tests assert of a ray cast of the fused corner from pose P against the analytic scene: the share of hits, the depth
    errors on the hits, the share of hits with a normal, the normals' angles (degrees) on hits more than 100 away from a crease."""
    cloud, nrm, lam = cast if cast is not None else raycast(vol, cam, P.reshape(12).astype(F32), z_near, z_far)
    _, _, plane, z, crease = render_corner(P, cam)
    hit = ~np.isnan(lam)
    err = np.abs(lam.astype(np.float64) - z.reshape(-1))[hit]
    has_n = hit & (np.abs(nrm[:, :3]).sum(1) > 0)
    true_n = P[:, :3].T[:, plane.reshape(-1)].T          # e_plane in the camera's frame: it points toward the camera
    cosang = np.clip((nrm[:, :3].astype(np.float64) * true_n).sum(1), -1, 1)
    far = has_n & (crease.reshape(-1) > 100.0)
    ang = np.degrees(np.arccos(cosang[far]))
    return dict(hits=hit.mean(), err=err, normals=has_n.sum() / max(1, hit.sum()), angles=ang)
