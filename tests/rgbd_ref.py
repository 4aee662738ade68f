"""The RGB-D front end restated in numpy (the rule of include/icp_amd.h: icp_rgbd_t, icp_write_rgbd, icp_kernel_rgbd).

Integer sums in uint64, the one division in float64, everything else in float32 with each operation on its own (numpy fuses
nothing), as icp_rgbd.hip evaluates it with -ffp-contract=off.  The normals are p2pl_ref.grid_normals of the whole vertex map.
A plain module: it collects no tests."""
import numpy as np

from p2pl_ref import grid_normals

F32 = np.float32

DEFAULTS = dict(width=640, height=480, fx=595.0, fy=595.0, cx=319.5, cy=239.5, depth_scale=1.0, d_min=1, d_max=65535,
                x0=65, y0=49, step_x=4, step_y=3, radius=0, range=30)


def config(**kw):
    """The header's table with `kw` in place of its values."""
    c = dict(DEFAULTS)
    assert not set(kw) - set(c), set(kw) - set(c)
    c.update(kw)
    return c


def valid_counts(depth, cfg):
    d = np.asarray(depth).astype(np.int64)
    return (d != 0) & (d >= cfg["d_min"]) & (d <= cfg["d_max"])


def sums(depth, cfg):
    """(N, D) of every pixel as uint64 (both 0 where the centre is invalid): N = sum w_s w_r c_q, D = sum w_s w_r."""
    H, W, r, S = cfg["height"], cfg["width"], cfg["radius"], cfg["range"]
    c = np.asarray(depth).reshape(H, W).astype(np.int64)
    ok = valid_counts(c, cfg)
    N = np.zeros((H, W), np.uint64)
    D = np.zeros((H, W), np.uint64)
    cp = np.pad(c, r)
    okp = np.pad(ok, r)                                               # (outside the image: does not count)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ws = max(0, (r + 1) ** 2 - dx * dx - dy * dy)
            cq = cp[r + dy:r + dy + H, r + dx:r + dx + W]
            wr = np.maximum(0, S * S - (cq - c) ** 2)
            w = np.where(ok & okp[r + dy:r + dy + H, r + dx:r + dx + W], ws * wr, 0).astype(np.uint64)
            N += w * cq.astype(np.uint64)
            D += w
    return N, D


def depth_map(depth, cfg):
    """z of every pixel, (H, W) float32."""
    H, W = cfg["height"], cfg["width"]
    c = np.asarray(depth).reshape(H, W)
    ok = valid_counts(c, cfg)
    if cfg["radius"] == 0:
        q = c.astype(F32)
    else:
        N, D = sums(c, cfg)
        assert int(N.max(initial=0)) < 2 ** 53
        q = (N.astype(np.float64) / np.where(ok, D, 1).astype(np.float64)).astype(F32)
    with np.errstate(over="ignore"):
        return np.where(ok, q * F32(cfg["depth_scale"]), F32(0)).astype(F32)


def cloud(depth, rgb, cfg):
    """The float8 cloud of the whole image, (H * W, 8) float32."""
    H, W = cfg["height"], cfg["width"]
    z = depth_map(depth, cfg)
    u = np.arange(W, dtype=F32)[None, :]
    v = np.arange(H, dtype=F32)[:, None]
    out = np.zeros((H, W, 8), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        out[..., 0] = (u - F32(cfg["cx"])) * z / F32(cfg["fx"])
        out[..., 1] = (v - F32(cfg["cy"])) * z / F32(cfg["fy"])
    out[..., 2] = z
    out[..., 3] = 1
    if rgb is not None:
        out[..., 4:7] = np.asarray(rgb, np.uint8).reshape(H, W, 3).astype(F32) / F32(255)
    out[..., 7] = 1
    return out.reshape(H * W, 8)


def normals(cloud8, cfg):
    """The normals of the whole vertex map, (H * W, 4) float32."""
    return grid_normals(cloud8, cfg["width"])


def lattice(cfg, side):
    """Flat pixel indices of the side x side landmarks, landmark j * side + i = pixel (x0 + step_x i, y0 + step_y j)."""
    x = cfg["x0"] + cfg["step_x"] * np.arange(side)
    y = cfg["y0"] + cfg["step_y"] * np.arange(side)
    assert x[-1] < cfg["width"] and y[-1] < cfg["height"], "the lattice must lie inside the image"
    return (y[:, None] * cfg["width"] + x[None, :]).reshape(-1)


def landmarks(depth, rgb, cfg, side, with_normals=False):
    """(landmarks (side^2, 8), normals (side^2, 4) or None)."""
    C8 = cloud(depth, rgb, cfg)
    at = lattice(cfg, side)
    return C8[at], (normals(C8, cfg)[at] if with_normals else None)
