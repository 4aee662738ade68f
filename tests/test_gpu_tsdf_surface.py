"""GPU tests of the surface extraction (icp_tsdf_surface.hip, icp_amd/tsdf.py: extract_surface) against its numpy restatement
(tsdf_surface_ref.py): every record bit for bit, every count equal.  Every condition on a test's own inputs is asserted on the
restatement first, so that no comparison is one of empty clouds."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import tsdf_ref as T
import tsdf_surface_ref as S
from icp_checks import assert_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
F32 = np.float32
RUN, SCAN_TILE = 1024, 1024                 # voxels of a block of the sweep, block counts of a tile of the scan (icp_tsdf_surface.hip)


def _device_volume(cfg):
    from icp_amd import tsdf
    return tsdf.TSDFVolume(tsdf.TSDFConfig(**cfg))


def _written(vol):
    dev = _device_volume(vol.cfg)
    dev.write(vol.dw, vol.rgb)
    return dev


def _assert_volume(dev, ref, what):
    dw, col = dev.read()
    assert_bits(dw, ref.dw, what + ": {D, W}")
    if ref.rgb is not None:
        assert_bits(col, ref.rgb, what + ": colour")


def _assert_surface(dev, ref, min_weight, what, want=None):
    """extract_surface with and without normals against the restatement; returns the restatement's (cloud, normals)."""
    cloud, nrm = want if want is not None else S.extract(ref, min_weight)
    got, gotn = dev.extract_surface(min_weight)
    assert got.shape[0] == cloud.shape[0], (what, got.shape[0], cloud.shape[0])
    assert_bits(got, cloud, what + ": cloud")
    assert_bits(gotn, nrm, what + ": normals")
    only, none = dev.extract_surface(min_weight, normals=False)
    assert none is None
    assert_bits(only, cloud, what + ": cloud without normals")
    return cloud, nrm


def _with_normal(nrm):
    return np.any(nrm[:, :3] != 0, axis=1)


def _raw(dev, min_weight, normals, capacity, cloud, nrm, opt=True):
    """The C entry itself: (status, count)."""
    from icp_amd import tsdf
    o, count = tsdf.icp_tsdf_surface_t(min_weight, normals), C.c_uint32(0xDEAD)
    rc = tsdf._lib().icp_tsdf_extract_surface(dev._t, C.byref(o) if opt else None, capacity, None if cloud is None else cloud.ctypes.data,
                                              None if nrm is None else nrm.ctypes.data, C.byref(count))
    return rc, count.value


# ---- 1. the fused corner ----------------------------------------------------------------------------------------------------------------

CORNER_DIMS = (64, 56, 48)


@functools.lru_cache(maxsize=None)
def _corner_frames():
    cam = T.corner_camera()
    out = []
    for eye in T.EYES:
        P = T.look_at(eye)
        depth, rgb = T.render_corner(P, cam)[:2]
        out.append((P.reshape(12).astype(F32), depth, rgb))
    return cam, out


@pytest.mark.parametrize("colour", [1, 0], ids=["colour", "no colour"])
def test_fused_corner(engine, colour):
    from icp_amd import rgbd
    cam, frames = _corner_frames()
    cfg = T.corner_volume(dims=CORNER_DIMS, colour=colour)
    ref, dev = T.Volume(cfg), _device_volume(cfg)
    for pose, depth, rgb in frames:
        T.integrate(ref, cam, pose, depth, rgb if colour else None)
        dev.integrate(rgbd.RGBDConfig(**cam), pose, depth, rgb if colour else None)
    _assert_volume(dev, ref, "the fused corner")
    counts = []
    for min_weight in (1.0, 2.0):
        info = {}
        want = S.extract(ref, min_weight, info)
        f = S.corner_surface_figures(*want)
        per_axis = np.bincount(info["axis"], minlength=3)
        print("min_weight %g: %d points %s, farthest %.2f, with a normal %.3f" % (min_weight, f["count"], per_axis, f["dist"].max(), f["normals"]))
        assert f["count"] > 3000 and per_axis.min() > 500 and f["dist"].max() < 8.0 and 0.8 < f["normals"] < 1.0
        assert (want[0][:, 4:7].max(0) > 0.5).all() if colour else (want[0][:, 4:7] == 0).all()
        _assert_surface(dev, ref, min_weight, "min_weight %g" % min_weight, want)
        counts.append(f["count"])
    assert counts[1] < counts[0]
    _assert_volume(dev, ref, "the volume after the extractions")
    dev.close()


# ---- 2. written volumes -------------------------------------------------------------------------------------------------------------------

PLANE_DIMS = (24, 20, 12)


def _plane(z0=6.3, holes=None, dims=PLANE_DIMS, mu=4.0):
    """The tilted plane of test_gpu_tsdf.py's written volumes: D = clip ((z0 + 0.11 i - 0.07 j - k) / mu), W = 1 (0 where `holes`), a
    colour that varies along every axis; voxels of 1 from the origin."""
    nx, ny, nz = dims
    vol = T.Volume(T.volume_config(nx, ny, nz, 1.0, (0.0, 0.0, 0.0), mu, colour=1))
    k, j, i = np.meshgrid(np.arange(nz, dtype=F32), np.arange(ny, dtype=F32), np.arange(nx, dtype=F32), indexing="ij")
    vol.dw[..., 0] = np.clip(((F32(z0) + F32(0.11) * i - F32(0.07) * j) - k) / F32(mu), -1, 1)
    vol.dw[..., 1] = 1
    if holes is not None:
        vol.dw[..., 1][holes(i, j, k)] = 0
    vol.rgb[..., 0], vol.rgb[..., 1], vol.rgb[..., 2] = i / nx, j / ny, k / nz
    return vol


def _sparse(dims, voxels, colour=0):
    """A volume with W = 0 everywhere but at voxels {(i, j, k): (D, W)}."""
    vol = T.Volume(T.volume_config(*dims, 1.5, (-2.0, 1.0, 0.5), 4.0, colour=colour))
    for (i, j, k), (d, w) in voxels.items():
        vol.dw[k, j, i] = (d, w)
    return vol


def _lin(vol, idx):
    return (idx[:, 2] * vol.cfg["ny"] + idx[:, 1]) * vol.cfg["nx"] + idx[:, 0]


def _case(name):
    """(volume, min_weight, the condition on (info, cloud, normals, volume) that makes the case what it is called)."""
    below1 = np.nextafter(F32(1), F32(0))
    if name == "2 x 2 x 2, one member on each axis":
        vol = _sparse((2, 2, 2), {(0, 0, 0): (-0.5, 1), (1, 0, 0): (0.5, 1), (0, 1, 0): (0.25, 1), (0, 0, 1): (0.75, 1)}, colour=1)
        vol.rgb[...] = np.arange(24, dtype=F32).reshape(2, 2, 2, 3) / F32(24)
        return vol, 1.0, lambda I, c, n, v: list(I["axis"]) == [0, 1, 2] and (I["index"] == 0).all()
    if name == "tilted plane, nothing a multiple of 64":
        def cond(I, c, n, v):
            rows = _lin(v, I["index"]) // v.cfg["nx"]
            blocks = _lin(v, I["index"]) // RUN
            return (np.bincount(I["axis"], minlength=3).min() >= 10 and c.shape[0] > 400 and _with_normal(n).sum() > 100 and (~_with_normal(n)).sum() > 10
                    and np.unique(blocks).size >= 3 and np.unique(rows).size > 50 and (c[:, 4:7].std(0) > 0.01).all())
        return _plane(), 1.0, cond
    if name == "tilted plane with 3 % holes":
        holes = lambda i, j, k: np.random.default_rng(11).random(i.shape) < 0.03
        def cond(I, c, n, v):
            interior = np.all((I["index"] >= 1) & (I["index"] + 2 < np.array(PLANE_DIMS)), axis=1)      # both ends' neighbours are inside
            full = S.extract(_plane())[0].shape[0]
            return ((v.dw[..., 1] == 0).mean() > 0.02 and c.shape[0] < full and (interior & ~I["grad_known"]).sum() >= 10
                    and (~_with_normal(n)).sum() >= 10 and _with_normal(n).sum() >= 50 and not (_with_normal(n) & ~I["grad_known"]).any())
        return _plane(holes=holes), 1.0, cond
    if name == "the last row, column and slice but one":
        def cond(I, c, n, v):
            nx, ny, nz = PLANE_DIMS
            ok = S.usable(v.dw)
            D = v.dw[..., 0].reshape(-1)
            pos = (D > 0)
            u = ok.reshape(-1)
            g = np.arange(D.size)
            i, j = g % nx, (g // nx) % ny
            # edges a kernel that forgot where a row or a slice ends would find: a usable last voxel whose linear successor is usable, of the other sign
            wrap_x = (i == nx - 1) & (g + 1 < D.size)
            wrap_y = (j == ny - 1) & (g + nx < D.size)
            false_x = (u[g[wrap_x]] & u[g[wrap_x] + 1] & (pos[g[wrap_x]] != pos[g[wrap_x] + 1])).sum()
            false_y = (u[g[wrap_y]] & u[g[wrap_y] + nx] & (pos[g[wrap_y]] != pos[g[wrap_y] + nx])).sum()
            last = [((I["axis"] == a) & (I["index"][:, a] == PLANE_DIMS[a] - 2)).sum() for a in range(3)]
            beyond = [((I["axis"] == a) & (I["index"][:, a] >= PLANE_DIMS[a] - 1)).sum() for a in range(3)]
            print("members at the last edge of x, y, z:", last, " false members of a wrapped sweep:", false_x, false_y)
            return min(last) >= 3 and sum(beyond) == 0 and false_x >= 3 and false_y >= 3 and ok[-1].any() and ok[:, -1].any() and ok[:, :, -1].any()
        # (a random D in (-0.9, 0.9) with W = 1: half of all edges are members, at the volume's faces as anywhere)
        vol = T.Volume(T.volume_config(*PLANE_DIMS, 1.0, (0.0, 0.0, 0.0), 4.0))
        vol.dw[..., 0] = np.random.default_rng(13).uniform(-0.9, 0.9, vol.dw.shape[:3]).astype(F32)
        vol.dw[..., 1] = 1
        return vol, 1.0, cond
    if name == "checkerboard, three members per lane":
        nx, ny, nz = 70, 9, 5
        vol = T.Volume(T.volume_config(nx, ny, nz, 1.0, (0.0, 0.0, 0.0), 4.0))
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        vol.dw[..., 0] = np.where((i + j + k) % 2 == 0, F32(0.5), F32(-0.5))
        vol.dw[..., 1] = 1
        return vol, 1.0, lambda I, c, n, v: c.shape[0] == S.edge_count(nx, ny, nz) == 8425 and (np.bincount(_lin(v, I["index"])) == 3).sum() == 69 * 8 * 4
    if name == "D exactly +0 and -0 at a crossing":
        vol = T.Volume(T.volume_config(5, 3, 3, 1.0, (0.0, 0.0, 0.0), 4.0))
        vol.dw[..., 0], vol.dw[..., 1] = 0.5, 1
        vol.dw[1, 1, 1, 0], vol.dw[1, 1, 3, 0] = 0.0, -0.0
        def cond(I, c, n, v):
            t = I["t"]
            return (c.shape[0] == 12 and ((t == 0) & np.signbit(t)).sum() == 3 and ((t == 0) & ~np.signbit(t)).sum() == 3 and (t == 1).sum() == 6
                    and np.signbit(v.dw[1, 1, 3, 0]) and not np.signbit(v.dw[1, 1, 1, 0]))
        return vol, 1.0, cond
    if name == "fabsf (D) == 1 is not usable, the float below 1 is":
        vol = _sparse((4, 2, 2), {(0, 0, 0): (1.0, 1), (1, 0, 0): (-0.5, 1), (0, 1, 0): (below1, 1), (1, 1, 0): (-0.5, 1),
                                  (2, 0, 0): (-1.0, 1), (3, 0, 0): (0.5, 1), (2, 1, 0): (-below1, 1), (3, 1, 0): (0.5, 1)})
        return vol, 1.0, lambda I, c, n, v: I["index"].tolist() == [[0, 1, 0], [2, 1, 0]] and list(I["axis"]) == [0, 0] and below1 < 1
    if name == "W == min_weight is usable, the float below it is not":
        below3 = np.nextafter(F32(3), F32(0))
        vol = _sparse((2, 2, 2), {(0, 0, 0): (0.5, below3), (1, 0, 0): (-0.5, 3), (0, 1, 0): (0.5, 3), (1, 1, 0): (-0.5, 3)})
        return vol, 3.0, lambda I, c, n, v: I["index"].tolist() == [[0, 1, 0]] and S.extract(v, float(below3))[0].shape[0] == 2
    if name == "NaN in D is no member":
        vol = _sparse((2, 2, 2), {(0, 0, 0): (np.nan, 1), (1, 0, 0): (0.5, 1), (0, 1, 0): (-0.5, 1), (1, 1, 0): (0.5, 1)})      # (NaN > 0) != (0.5 > 0)
        return vol, 1.0, lambda I, c, n, v: I["index"].tolist() == [[0, 1, 0]] and np.isnan(v.dw[0, 0, 0, 0])
    if name == "NaN in W is no member":
        vol = _sparse((2, 2, 2), {(0, 0, 0): (-0.5, np.nan), (1, 0, 0): (0.5, 1), (0, 1, 0): (-0.5, 1), (1, 1, 0): (0.5, 1)})
        return vol, 1.0, lambda I, c, n, v: I["index"].tolist() == [[0, 1, 0]] and np.isnan(v.dw[0, 0, 0, 1])
    if name == "a NaN neighbour D with W > 0 gives a zero normal":
        vol = _plane(dims=(9, 8, 12))
        vol.dw[8, 4, 4, 0] = np.nan                                            # above the surface (z = 6.46 there): a gradient sample only
        def cond(I, c, n, v):
            clean = S.extract(_plane(dims=(9, 8, 12)))
            lost = _with_normal(clean[1]) & ~_with_normal(n)
            return clean[0].shape[0] == c.shape[0] and lost.sum() >= 1 and I["grad_known"][lost].all() and _with_normal(n).sum() >= 10
        return vol, 1.0, cond
    raise KeyError(name)


CASES = ["2 x 2 x 2, one member on each axis", "tilted plane, nothing a multiple of 64", "tilted plane with 3 % holes",
         "the last row, column and slice but one", "checkerboard, three members per lane", "D exactly +0 and -0 at a crossing",
         "fabsf (D) == 1 is not usable, the float below 1 is", "W == min_weight is usable, the float below it is not", "NaN in D is no member",
         "NaN in W is no member", "a NaN neighbour D with W > 0 gives a zero normal"]


@pytest.mark.parametrize("name", CASES)
def test_written_volumes(engine, name):
    vol, min_weight, condition = _case(name)
    info = {}
    want = S.extract(vol, min_weight, info)
    assert condition(info, want[0], want[1], vol), name
    dev = _written(vol)
    _assert_surface(dev, vol, min_weight, name, want)
    _assert_volume(dev, vol, name + ": the volume afterwards")
    dev.close()


def test_an_empty_volume_leaves_the_outputs_untouched(engine):
    cfg = T.volume_config(24, 20, 12, 1.0, (0.0, 0.0, 0.0), 4.0, colour=1)
    ref, dev = T.Volume(cfg), _device_volume(cfg)
    assert S.extract(ref)[0].shape == (0, 8)
    cloud, nrm = np.full((4, 8), -7, F32), np.full((4, 4), -7, F32)
    assert _raw(dev, 1.0, 1, 4, cloud, nrm) == (0, 0)
    assert (cloud == -7).all() and (nrm == -7).all()
    got, gotn = dev.extract_surface()
    assert got.shape == (0, 8) and gotn.shape == (0, 4)
    dev.close()


# ---- 3. the scan at scale -------------------------------------------------------------------------------------------------------------------

def test_the_scan_at_scale(engine):
    """160 x 96 x 80 voxels: 1200 blocks of the sweep, more than icp_pairs' 4096-block form serves per registration only in a volume, and two
    tiles of the scan of the block counts.  The scan's second level is one block by construction (a volume has at most 1024 tiles): it has
    no second tile at any size, here it scans two sums.  A checkerboard of signs inside a random 3 % of the 8^3 cells, W = 0 elsewhere;
    the magnitudes vary (0.25 .. 0.75), because a checkerboard of one magnitude has the gradient 0 and would compare zero normals only."""
    nx, ny, nz = 160, 96, 80
    vol = T.Volume(T.volume_config(nx, ny, nz, 4.0, (-320.0, -192.0, 0.0), 16.0))
    on = np.random.default_rng(7).random((nz // 8, ny // 8, nx // 8)) < 0.03
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol.dw[..., 0] = np.where((i + j + k) % 2 == 0, 1, -1) * np.random.default_rng(8).uniform(0.25, 0.75, i.shape)
    vol.dw[..., 1] = on[k // 8, j // 8, i // 8]
    info = {}
    want = S.extract(vol, 1.0, info)
    nblk = (nx * ny * nz + RUN - 1) // RUN
    per_block = np.bincount(_lin(vol, info["index"]) // RUN, minlength=nblk)
    empty = per_block == 0
    runs = np.diff(np.flatnonzero(np.concatenate([[False], ~empty, [False]])))     # gaps between members' blocks
    print("%d members in %d of %d blocks, %d tiles of the scan, the longest stretch of empty blocks %d" % (want[0].shape[0], (~empty).sum(), nblk, -(-nblk // SCAN_TILE), runs.max() - 1))
    assert nblk > 1024 and -(-nblk // SCAN_TILE) == 2
    assert per_block[:SCAN_TILE].sum() > 0 and per_block[SCAN_TILE:].sum() > 0 and per_block[SCAN_TILE:].sum() != want[0].shape[0]
    assert 0.2 < empty.mean() < 0.9 and runs.max() - 1 >= 8 and want[0].shape[0] > 50000 and _with_normal(want[1]).sum() > 10000
    dev = _written(vol)
    _assert_surface(dev, vol, 1.0, "the scan at scale", want)
    dev.close()


# ---- 4. capacity ----------------------------------------------------------------------------------------------------------------------------

def test_capacity(engine):
    vol = _plane()
    cloud, nrm = S.extract(vol)
    n = cloud.shape[0]
    assert n > 400
    dev = _written(vol)
    assert _raw(dev, 1.0, 1, 0, None, None) == (0, n)                       # the counting call
    assert _raw(dev, 1.0, 0, 0, None, None, opt=False) == (0, n)            # opt == NULL: the defaults
    for cap in (1, n - 1, n, n + 5):
        for normals in (1, 0):
            got, gotn = np.full((cap + 3, 8), -7, F32), np.full((cap + 3, 4), -7, F32)
            assert _raw(dev, 1.0, normals, cap, got, gotn if normals else None) == (0, n), cap
            m = min(n, cap)
            assert_bits(got[:m], cloud[:m], "capacity %d: the prefix" % cap)
            assert (got[m:] == -7).all() and (gotn[m:] == -7).all(), cap
            if normals:
                assert_bits(gotn[:m], nrm[:m], "capacity %d: the prefix's normals" % cap)
            else:
                assert (gotn == -7).all()
        c3 = dev.extract_surface(capacity=cap)
        assert c3[2] == n and c3[0].shape[0] == min(n, cap) == c3[1].shape[0]
        assert_bits(c3[0], cloud[:min(n, cap)], "extract_surface (capacity=%d)" % cap)
    _assert_volume(dev, vol, "the volume afterwards")
    dev.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_everything_as_it_was(engine):
    from icp_amd import tsdf
    vol = _plane()
    dev = _written(vol)
    n = S.extract(vol)[0].shape[0]
    cloud, nrm = np.full((n, 8), -7, F32), np.full((n, 4), -7, F32)
    L, t = tsdf._lib(), dev._t

    def refused(rc, count=None):
        assert rc == EINVAL and b"icp_tsdf_extract_surface" in L.icp_tsdf_last_error(t), (rc, L.icp_tsdf_last_error(t))
        assert count is None or count == 0xDEAD
        assert (cloud == -7).all() and (nrm == -7).all()
        _assert_volume(dev, vol, "the volume after a refusal")

    o = tsdf.icp_tsdf_surface_t(1.0, 1)
    refused(L.icp_tsdf_extract_surface(t, C.byref(o), n, cloud.ctypes.data, nrm.ctypes.data, None))              # a NULL count
    for bad in (0.5, 0.0, -1.0, float("nan"), float("inf")):
        refused(*_raw(dev, bad, 1, n, cloud, nrm))
    for bad in (2, 0xFFFFFFFF):
        refused(*_raw(dev, 1.0, bad, n, cloud, nrm))
    refused(*_raw(dev, 1.0, 1, n, None, nrm))                               # a NULL output with a capacity
    refused(*_raw(dev, 1.0, 0, n, None, None))
    refused(*_raw(dev, 1.0, 1, n, cloud, None))                             # normals wanted
    with pytest.raises(engine.ICPError) as e:
        dev.extract_surface(min_weight=0.0)
    assert e.value.code == EINVAL and "min_weight" in str(e.value)
    assert _raw(dev, 1.0, 1, n, cloud, nrm) == (0, n)                       # and the same arguments made good pass
    dev.close()


# ---- 6. the layers above --------------------------------------------------------------------------------------------------------------------

def test_cpp_facade_program():
    """tests/cpp/tsdf_surface_facade_test.cpp: TSDFVolume::extractSurface against the C-ABI it wraps and the rule as a host loop."""
    exe = os.path.join(ROOT, "tests", "cpp", "tsdf_surface_facade_test")
    assert os.path.exists(exe), "tests/cpp/tsdf_surface_facade_test is built by build() / make tsdf_surface_facade_test"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tsdf surface facade ok" in out.stdout, (out.stdout, out.stderr)


def test_timing_entry_times_the_extraction(engine):
    vol = _plane()
    assert S.extract(vol)[0].shape[0] > 400
    dev = _written(vol)
    assert dev.time_kernel(2, reps=2) > 0
    _assert_volume(dev, vol, "the volume after the timed extractions")
    _assert_surface(dev, vol, 1.0, "after the timed extractions")
    empty = _device_volume(vol.cfg)
    assert empty.time_kernel(2, reps=2) > 0                                 # (no member: the scatter is not launched)
    dev.close(); empty.close()


def test_extract_surface_after_track_to_model(engine):
    """The product of the pipeline: four frames tracked against the model, then the model's surface, against the restatement's surface of
    the restatement's volume fused at the same poses."""
    import icp_checks as K
    from icp_amd import rgbd, tsdf
    # test_gpu_tsdf.py's tracking set-up: 320 x 240 pixels, a lattice of 64 x 64 landmarks, 1 degree and 9.85 mm a frame, point-to-plane
    d = T.corner_camera(width=320, height=240, fx=300.0, cx=159.5, cy=119.5, x0=2, y0=3, step_x=5, step_y=3)
    P = [T.look_at(T.EYE_CAST)]
    for _ in range(3):
        P.append(T.rotate_pose(P[-1], (0.3, 1.0, 0.2), 1.0, (6.0, -5.0, 6.0)))
    frames = [T.render_corner(p, d)[:2] for p in P]
    cfg = T.corner_volume(colour=1)
    g, dev = engine.ICP(0), _device_volume(cfg)
    g.init(64 * 64, 64, 2e2, 1e-6)
    rgbd.set_config(g, rgbd.RGBDConfig(**d))
    g.set_normals(K.GIVEN, 0)
    g.set_error_metric(K.P2PL, 0.05)
    g.set_rejection(invalid=True)
    poses = [pose for pose, _, _ in tsdf.track_to_model(g, dev, frames, P[0].reshape(12).astype(F32), 200.0, 1600.0, normals=True)]
    ref = T.Volume(cfg)
    for pose, (depth, rgb) in zip(poses, frames):
        T.integrate(ref, d, pose, depth, rgb)
    assert len(poses) == 4
    _assert_volume(dev, ref, "the volume after four frames")
    cloud, nrm = S.extract(ref)
    f = S.corner_surface_figures(cloud, nrm)
    print("after four tracked frames: %d points, farthest from its quarter-plane %.2f, with a normal %.3f" % (f["count"], f["dist"].max(), f["normals"]))
    assert f["count"] > 3000 and f["dist"].max() < 8.0 and f["normals"] > 0.8 and (cloud[:, 4:7].max(0) > 0.5).all()
    _assert_surface(dev, ref, 1.0, "the tracked model", (cloud, nrm))
    g.close(); dev.close()
