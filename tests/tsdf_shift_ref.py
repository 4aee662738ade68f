"""The moving volume restated in numpy (the rule of include/icp_amd.h, "Moving volume": icp_tsdf_shift, icp_tsdf_extract_surface_region,
icp_tsdf_kept_box, icp_tsdf_follow), on the volumes of tsdf_ref.py, and the moving scene the CPU and GPU tests share.

A shifted volume carries its window with it: vol.base (the origin given at create) and vol.window (the cumulative shift), beside
vol.cfg["origin"], the current origin.  A plain module: it collects no tests."""
import numpy as np

import tsdf_ref as T
import tsdf_surface_ref as S

F32 = np.float32
WINDOW_MAX = 1 << 24


def window(vol):
    """(base, cumulative shift) of a volume; a volume that was never shifted has its origin and zeros."""
    return getattr(vol, "base", tuple(vol.cfg["origin"])), getattr(vol, "window", (0, 0, 0))


def origin_of(base, c, voxel):
    """origin_a = base_a + (float) c_a * voxel in float32, each operation rounded on its own."""
    with np.errstate(over="ignore", invalid="ignore"):
        return tuple(F32(base[a]) + F32(c[a]) * F32(voxel) for a in range(3))


def refused(vol, s):
    """The shift is ICP_EINVAL: a cumulative shift past 2^24 or an origin that is not finite."""
    base, c = window(vol)
    new = [int(c[a]) + int(s[a]) for a in range(3)]
    return any(abs(x) > WINDOW_MAX for x in new) or not np.all(np.isfinite(origin_of(base, new, vol.cfg["voxel"])))


def _moved(x, s):
    """x (nz, ny, nx, ..) with new [k, j, i] = old [k + s_z, j + s_y, i + s_x] where that exists, zero bits elsewhere."""
    out = np.zeros_like(x)
    n = (x.shape[2], x.shape[1], x.shape[0])
    src, dst = [], []
    for a in range(3):
        lo, hi = max(0, -s[a]), min(n[a], n[a] - s[a])          # the new indices with an old voxel behind them
        if lo >= hi:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo + s[a], hi + s[a]))
    out[dst[2], dst[1], dst[0]] = x[src[2], src[1], src[0]]
    return out


def shift(vol, s):
    """A new tsdf_ref.Volume: vol's window moved by s voxels — contents (as bit patterns), cumulative shift and origin by the rule."""
    s = tuple(int(x) for x in s)
    assert not refused(vol, s)
    base, c = window(vol)
    new = tuple(c[a] + s[a] for a in range(3))
    out = T.Volume(dict(vol.cfg, origin=tuple(float(o) for o in origin_of(base, new, vol.cfg["voxel"]))))
    out.base, out.window = base, new
    out.dw = _moved(vol.dw.view(np.uint32), s).view(F32)
    out.rgb = None if vol.rgb is None else _moved(vol.rgb.view(np.uint32), s).view(F32)
    return out


def kept_box(cfg, s):
    """(lo, hi): lo_a = max (0, s_a) (at most n_a), hi_a = max (lo_a, min (n_a, n_a + s_a))."""
    n = (cfg["nx"], cfg["ny"], cfg["nz"])
    lo = tuple(min(n[a], max(0, int(s[a]))) for a in range(3))
    hi = tuple(max(lo[a], min(n[a], n[a] + int(s[a]))) for a in range(3))
    return lo, hi


def inside(info, lo, hi, v_only=False):
    """Per member of tsdf_surface_ref.extract's info: both its ends v and v + e_a lie in the box (v_only: the low end alone, the rule that
    loses members)."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    v = info["index"].reshape(-1, 3)
    w = v.copy()
    if v.shape[0]:
        w[np.arange(v.shape[0]), info["axis"]] += 1
    vin = np.all((v >= lo) & (v < hi), axis=1)
    return vin if v_only else vin & np.all((w >= lo) & (w < hi), axis=1)


def extract_region(vol, lo, hi, outside=False, min_weight=1.0, info=None):
    """(cloud, normals) of the members of tsdf_surface_ref.extract that are INSIDE the box (outside: every other one), in its order."""
    I = {}
    cloud, nrm = S.extract(vol, min_weight, I)
    keep = inside(I, lo, hi) != bool(outside)
    if info is not None:
        info.update({k: x[keep] for k, x in I.items()})
    return cloud[keep], nrm[keep]


def follow(cfg, point, threshold):
    """The shift that centres the window on `point`, in float64: d_a = (point_a - (origin_a + 0.5 (n_a - 1) voxel)) / voxel; zeros while
    max |d_a| <= threshold, else rint (d_a) (ties to even) on every axis."""
    n = (cfg["nx"], cfg["ny"], cfg["nz"])
    voxel = float(F32(cfg["voxel"]))
    d = [(float(F32(point[a])) - (float(F32(cfg["origin"][a])) + 0.5 * (n[a] - 1.0) * voxel)) / voxel for a in range(3)]
    if max(abs(x) for x in d) <= threshold:
        return (0, 0, 0)
    return tuple(int(np.rint(x)) for x in d)


def follow_point(pose12, distance):
    """pose . (0, 0, distance) in float64, rounded to float32: what the generators hand to follow ()."""
    P = np.asarray(pose12, np.float64).reshape(3, 4)
    return (P[:, 2] * float(distance) + P[:, 3]).astype(F32)


# ---- the moving scene: the room corner seen by a camera that translates along the wall y = 0 ------------------------------------------

SCENE_DIMS, SCENE_VOXEL, SCENE_MU = (40, 40, 40), 16.0, 48.0          # a 640 cube from (-64, -64, -64): too short for the path
SCENE_FOLLOW = (560.0, 6)                                             # the point 560 in front of the camera, 6 voxels of slack
SCENE_STEP = 110.0                                                    # world x per frame


def scene_volume(colour=0):
    return T.volume_config(*SCENE_DIMS, SCENE_VOXEL, (-64.0, -64.0, -64.0), SCENE_MU, 64.0, colour)


def scene_poses(frames=6):
    """Camera -> world poses (3, 4) float64: the eye slides along +x beside the wall y = 0, the view direction fixed."""
    eye0, target0 = np.array([420.0, 560.0, 380.0]), np.array([300.0, 0.0, 120.0])
    return [T.look_at(eye0 + [SCENE_STEP * f, 0, 0], target0 + [SCENE_STEP * f, 0, 0]) for f in range(frames)]


def run_scene(cam, poses12, frames, follow_=None, colour=0):
    """The frames integrated at the given poses into a fresh volume of the restatement; with follow_ = (distance, threshold) the volume
    follows the camera as the generators make it.  (volume, [(s, cloud, normals) per shift], [voxels changed per frame])."""
    vol = T.Volume(scene_volume(colour))
    shifts, changed = [], []
    for pose, (depth, rgb) in zip(poses12, frames):
        changed.append(int(T.integrate(vol, cam, pose, depth, rgb if colour else None)["changed"].sum()))
        if follow_ is not None:
            s = follow(vol.cfg, follow_point(pose, follow_[0]), follow_[1])
            if any(s):
                lo, hi = kept_box(vol.cfg, s)
                shifts.append((s,) + extract_region(vol, lo, hi, True))
                vol = shift(vol, s)
    return vol, shifts, changed


# ---- the written volumes of tests/test_gpu_tsdf_surface.py, written out again for the shift's CPU and GPU tests ---------------------------

PLANE_DIMS = (24, 20, 12)


def plane(z0=6.3, holes=False, dims=PLANE_DIMS, mu=4.0):
    """The tilted plane: D = clip ((z0 + 0.11 i - 0.07 j - k) / mu), W = 1 (0 in a random 3 % with `holes`), a colour that varies along
    every axis; voxels of 1 from the origin."""
    nx, ny, nz = dims
    vol = T.Volume(T.volume_config(nx, ny, nz, 1.0, (0.0, 0.0, 0.0), mu, colour=1))
    k, j, i = np.meshgrid(np.arange(nz, dtype=F32), np.arange(ny, dtype=F32), np.arange(nx, dtype=F32), indexing="ij")
    vol.dw[..., 0] = np.clip(((F32(z0) + F32(0.11) * i - F32(0.07) * j) - k) / F32(mu), -1, 1)
    vol.dw[..., 1] = 1
    if holes:
        vol.dw[..., 1][np.random.default_rng(11).random(i.shape) < 0.03] = 0
    vol.rgb[..., 0], vol.rgb[..., 1], vol.rgb[..., 2] = i / nx, j / ny, k / nz
    return vol


def random_volume(dims=PLANE_DIMS, seed=13):
    """A random D in (-0.9, 0.9) with W = 1: half of all edges are members, at the volume's faces as anywhere."""
    vol = T.Volume(T.volume_config(*dims, 1.0, (0.0, 0.0, 0.0), 4.0))
    vol.dw[..., 0] = np.random.default_rng(seed).uniform(-0.9, 0.9, vol.dw.shape[:3]).astype(F32)
    vol.dw[..., 1] = 1
    return vol


def checkerboard(dims=(70, 9, 5)):
    """Signs in a checkerboard, W = 1: every edge is a member, three per lane; an odd nx, rows that end inside a wave."""
    nx, ny, nz = dims
    vol = T.Volume(T.volume_config(nx, ny, nz, 1.0, (0.0, 0.0, 0.0), 4.0))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol.dw[..., 0] = np.where((i + j + k) % 2 == 0, F32(0.5), F32(-0.5))
    vol.dw[..., 1] = 1
    return vol
