"""GPU tests of the mesh extraction (icp_tsdf_surface.hip, icp_amd/tsdf.py: extract_mesh) against its numpy restatement (tsdf_mesh_ref.py):
vertices and normals bit for bit and equal to extract_surface's, triangles array_equal, both counts equal, the volume unchanged.  Every
condition on a test's own inputs is asserted on the restatement first.  The tilted plane, the corner's frames and the two-tile volume are
test_gpu_tsdf_surface.py's constructions, written out again here (a test module imports no test module)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import tsdf_mesh_ref as M
import tsdf_ref as T
import tsdf_surface_ref as S
from icp_checks import assert_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = 1, 3
F32 = np.float32
RUN, SCAN_TILE = 1024, 1024                 # voxels of a block of the sweeps, block counts of a tile of the scan (icp_tsdf_surface.hip)
CORNER_DIMS, PLANE_DIMS = (64, 56, 48), (24, 20, 12)


# ---- the volumes and checks that the surface's GPU tests use too ------------------------------------------------------------------------------

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


def _assert_surface(dev, ref, min_weight, what, want):
    got, gotn = dev.extract_surface(min_weight)
    assert_bits(got, want[0], what + ": cloud")
    assert_bits(gotn, want[1], what + ": normals")


@functools.lru_cache(maxsize=None)
def _corner_frames():
    cam = T.corner_camera()
    out = []
    for eye in T.EYES:
        P = T.look_at(eye)
        depth, rgb = T.render_corner(P, cam)[:2]
        out.append((P.reshape(12).astype(F32), depth, rgb))
    return cam, out


def _plane(z0=6.3, holes=None, dims=PLANE_DIMS, mu=4.0):
    """D = clip ((z0 + 0.11 i - 0.07 j - k) / mu), W = 1 (0 where `holes`), a colour that varies along every axis; voxels of 1 from the origin."""
    nx, ny, nz = dims
    vol = T.Volume(T.volume_config(nx, ny, nz, 1.0, (0.0, 0.0, 0.0), mu, colour=1))
    k, j, i = np.meshgrid(np.arange(nz, dtype=F32), np.arange(ny, dtype=F32), np.arange(nx, dtype=F32), indexing="ij")
    vol.dw[..., 0] = np.clip(((F32(z0) + F32(0.11) * i - F32(0.07) * j) - k) / F32(mu), -1, 1)
    vol.dw[..., 1] = 1
    if holes is not None:
        vol.dw[..., 1][holes(i, j, k)] = 0
    vol.rgb[..., 0], vol.rgb[..., 1], vol.rgb[..., 2] = i / nx, j / ny, k / nz
    return vol


def _assert_mesh(dev, ref, min_weight, what, want=None):
    """extract_mesh with and without normals against the restatement and against extract_surface; returns the restatement's mesh."""
    cloud, nrm, tri = want if want is not None else M.extract(ref, min_weight)
    got, gotn, gott = dev.extract_mesh(min_weight)
    assert (got.shape[0], gott.shape[0]) == (cloud.shape[0], tri.shape[0]), (what, got.shape, gott.shape, cloud.shape, tri.shape)
    assert_bits(got, cloud, what + ": vertices")
    assert_bits(gotn, nrm, what + ": normals")
    assert gott.dtype == np.uint32 and np.array_equal(gott, tri), what + ": triangles"
    pts, ptsn = dev.extract_surface(min_weight)
    assert_bits(got, pts, what + ": vertices against extract_surface")
    assert_bits(gotn, ptsn, what + ": normals against extract_surface")
    only, none, tri2 = dev.extract_mesh(min_weight, normals=False)
    assert none is None and np.array_equal(tri2, tri)
    assert_bits(only, cloud, what + ": vertices without normals")
    return cloud, nrm, tri


def _raw(dev, min_weight, normals, vcap, cloud, nrm, tcap, tri, opt=True, counts=(True, True)):
    """The C entry itself: (status, vertex count, triangle count)."""
    from icp_amd import tsdf
    o, nv, nt = tsdf.icp_tsdf_surface_t(min_weight, normals), C.c_uint32(0xDEAD), C.c_uint32(0xBEEF)
    rc = tsdf._lib().icp_tsdf_extract_mesh(dev._t, C.byref(o) if opt else None, vcap, None if cloud is None else cloud.ctypes.data,
                                           None if nrm is None else nrm.ctypes.data, C.byref(nv) if counts[0] else None,
                                           tcap, None if tri is None else tri.ctypes.data, C.byref(nt) if counts[1] else None)
    return rc, nv.value, nt.value


# ---- 1. the fused corner ----------------------------------------------------------------------------------------------------------------

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
        want = M.extract(ref, min_weight)
        print("min_weight %g: %d vertices, %d triangles" % (min_weight, want[0].shape[0], want[2].shape[0]))
        assert want[0].shape[0] > 3000 and want[2].shape[0] > 5000
        _assert_mesh(dev, ref, min_weight, "min_weight %g" % min_weight, want)
        counts.append(want[2].shape[0])
    assert counts[1] < counts[0]
    _assert_volume(dev, ref, "the volume after the extractions")
    dev.close()


# ---- 2. written volumes -------------------------------------------------------------------------------------------------------------------

def _signs(dims, positive, mag=0.5):
    """W = 1 everywhere, D = +mag where positive (i, j, k) else -mag."""
    nx, ny, nz = dims
    vol = T.Volume(T.volume_config(nx, ny, nz, 1.0, (0.0, 0.0, 0.0), 4.0))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol.dw[..., 0] = np.where(positive(i, j, k), F32(mag), F32(-mag))
    vol.dw[..., 1] = 1
    return vol


def _one_cell(n):
    table, _ = M.case_table()
    case = [c for c in range(256) if len(table[c]) == n][0]
    vol = _signs((2, 2, 2), lambda i, j, k: (case >> (i + 2 * j + 4 * k)) & 1 == 1)
    return vol, 1.0, lambda I, c, n_, t, v: t.shape[0] == n and I["case"].tolist() == [case]


def _random(dims, seed):
    vol = T.Volume(T.volume_config(*dims, 1.0, (0.0, 0.0, 0.0), 4.0))
    vol.dw[..., 0] = np.random.default_rng(seed).uniform(-0.9, 0.9, vol.dw.shape[:3]).astype(F32)
    vol.dw[..., 1] = 1
    return vol


def _spoiled(what):
    """The tilted plane with one voxel on the surface made unusable: its eight cells are inactive, the neighbouring edges stay members."""
    dims, at = (9, 8, 12), (6, 4, 4)                                           # (k, j, i): z = 6.46 there
    vol = _plane(dims=dims)
    clean = M.extract(_plane(dims=dims))
    if what == "D":
        vol.dw[at][0] = np.nan
    elif what == "W":
        vol.dw[at][1] = np.nan
    else:
        vol.dw[at][0] = 1.0

    def cond(I, c, n, t, v):
        k, j, i = at
        around = I["active"][k - 1:k + 1, j - 1:j + 1, i - 1:i + 1]
        info = {}
        S.extract(v, 1.0, info)
        near = np.all(np.abs(info["index"] - np.array([i, j, k])) <= 1, axis=1)
        return around.size == 8 and not around.any() and near.sum() >= 4 and t.shape[0] < clean[2].shape[0] and I["active"].sum() > 100
    return vol, 1.0, cond


def _case(name):
    """(volume, min_weight, the condition on (info, cloud, normals, triangles, volume) that makes the case what it is called)."""
    if name.startswith("one cell, "):
        return _one_cell(int(name.split()[2]))
    if name == "two cells that share an ambiguous face":
        vol = _signs((3, 2, 2), lambda i, j, k: np.where(i == 1, (j + k) % 2 == 0, i == 2))
        def cond(I, c, n, t, v):
            info = {}
            S.extract(v, 1.0, info)
            on_face = np.flatnonzero((info["index"][:, 0] == 1) & (info["axis"] != 0))       # the vertices on the shared face's four edges
            d = M.directed_edges(t)
            inside = d[np.isin(d[:, 0], on_face) & np.isin(d[:, 1], on_face)]
            once, lone, _ = M.edge_figures(t)
            paired = {(x, y) for x, y in inside.tolist()} == {(y, x) for x, y in inside.tolist()}
            return on_face.size == 4 and inside.shape[0] == 4 and paired and once and I["case"].size == 2
        return vol, 1.0, cond
    if name == "random, all 256 cases, where a row and a slice end":
        dims = PLANE_DIMS
        def cond(I, c, n, t, v):
            nx, ny, nz = dims
            ok, pos = S.usable(v.dw).reshape(-1), (v.dw[..., 0] > 0).reshape(-1)
            g = np.arange(ok.size)
            i, j = g % nx, (g // nx) % ny
            off = [0, 1, nx, nx + 1, nx * ny, nx * ny + 1, nx * ny + nx, nx * ny + nx + 1]
            false_cells = []
            for wrap in ((i == nx - 1), (j == ny - 1)):                       # cells a sweep that forgot where a row or a slice ends would find
                gg = g[wrap & (g + off[7] < ok.size)]
                usable8 = np.all([ok[gg + o] for o in off], axis=0)
                signs = np.sum([pos[gg + o] for o in off], axis=0)
                false_cells.append(int((usable8 & (signs > 0) & (signs < 8)).sum()))
            once, lone, _ = M.edge_figures(t)
            print("false cells of a wrapped sweep:", false_cells, " cases:", np.unique(I["cases"][I["active"]]).size)
            return (min(false_cells) >= 3 and np.unique(I["cases"][I["active"]]).size == 256 and once and np.unique(t).size == c.shape[0]
                    and I["active"].all())
        return _random(dims, 13), 1.0, cond
    if name == "tilted plane, nothing a multiple of 64":
        def cond(I, c, n, t, v):
            return t.shape[0] > 700 and np.unique(I["cell"] // RUN).size >= 3 and M.edge_figures(t)[0]
        return _plane(), 1.0, cond
    if name == "tilted plane with 3 % holes":
        holes = lambda i, j, k: np.random.default_rng(11).random(i.shape) < 0.03
        def cond(I, c, n, t, v):
            mem = S.members(v.dw)
            nz, ny, nx = v.dw.shape[:3]
            has = np.zeros((nz - 1, ny - 1, nx - 1), bool)                    # cells with a member among their twelve edges
            for e in range(12):
                c0 = M.edge_ends(e)[0]
                bx, by, bz = c0 & 1, (c0 >> 1) & 1, c0 >> 2
                has |= mem[e // 4][bz:nz - 1 + bz, by:ny - 1 + by, bx:nx - 1 + bx]
            unreferenced = c.shape[0] - np.unique(t).size
            print("cells with members but inactive: %d, members that no triangle references: %d" % ((has & ~I["active"]).sum(), unreferenced))
            return (has & ~I["active"]).sum() >= 10 and unreferenced >= 5 and t.shape[0] > 300
        return _plane(holes=holes), 1.0, cond
    if name == "checkerboard, four triangles per cell":
        nx, ny, nz = 70, 9, 5
        vol = _signs((nx, ny, nz), lambda i, j, k: (i + j + k) % 2 == 0)
        def cond(I, c, n, t, v):
            per_wave_step = np.bincount(I["cell"] // 64)
            return t.shape[0] == 4 * 69 * 8 * 4 and (np.bincount(I["cell"])[I["cell"]] == 4).all() and per_wave_step.max() == 256 > 255
        return vol, 1.0, cond
    if name == "a voxel with fabsf (D) == 1":
        return _spoiled("1")
    if name == "a voxel with NaN in D":
        return _spoiled("D")
    if name == "a voxel with NaN in W":
        return _spoiled("W")
    if name == "D exactly +0 and -0":
        vol = T.Volume(T.volume_config(5, 3, 3, 1.0, (0.0, 0.0, 0.0), 4.0))
        vol.dw[..., 0], vol.dw[..., 1] = 0.5, 1
        vol.dw[1, 1, 1, 0], vol.dw[1, 1, 3, 0] = 0.0, -0.0
        def cond(I, c, n, t, v):
            p = c[t.astype(np.int64)][:, :, :3]                                # (m, 3 vertices, xyz)
            same = np.all(p[:, 0] == p[:, 1], 1) | np.all(p[:, 1] == p[:, 2], 1) | np.all(p[:, 2] == p[:, 0], 1)
            distinct = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])
            once, lone, _ = M.edge_figures(t)
            return c.shape[0] == 12 and t.shape[0] == 16 and distinct.all() and same.sum() >= 8 and once and lone.shape[0] == 0
        return vol, 1.0, cond
    raise KeyError(name)


CASES = ["one cell, %d triangles" % n for n in range(1, 6)] + [
    "two cells that share an ambiguous face", "random, all 256 cases, where a row and a slice end", "tilted plane, nothing a multiple of 64",
    "tilted plane with 3 % holes", "checkerboard, four triangles per cell", "a voxel with fabsf (D) == 1", "a voxel with NaN in D",
    "a voxel with NaN in W", "D exactly +0 and -0"]


@pytest.mark.parametrize("name", CASES)
def test_written_volumes(engine, name):
    vol, min_weight, condition = _case(name)
    info = {}
    want = M.extract(vol, min_weight, info)
    assert condition(info, want[0], want[1], want[2], vol), name
    dev = _written(vol)
    _assert_mesh(dev, vol, min_weight, name, want)
    _assert_volume(dev, vol, name + ": the volume afterwards")
    dev.close()


# ---- 3. the scan at scale -------------------------------------------------------------------------------------------------------------------

def test_the_scan_at_scale(engine):
    """test_gpu_tsdf_surface.py's 160 x 96 x 80 construction: 1200 blocks of the sweeps, two tiles of the scan of the triangle block counts,
    triangles in both, stretches of empty blocks."""
    nx, ny, nz = 160, 96, 80
    vol = T.Volume(T.volume_config(nx, ny, nz, 4.0, (-320.0, -192.0, 0.0), 16.0))
    on = np.random.default_rng(7).random((nz // 8, ny // 8, nx // 8)) < 0.03
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol.dw[..., 0] = np.where((i + j + k) % 2 == 0, 1, -1) * np.random.default_rng(8).uniform(0.25, 0.75, i.shape)
    vol.dw[..., 1] = on[k // 8, j // 8, i // 8]
    info = {}
    want = M.extract(vol, 1.0, info)
    nblk = (nx * ny * nz + RUN - 1) // RUN
    per_block = np.bincount(info["cell"] // RUN, minlength=nblk)
    empty = per_block == 0
    runs = np.diff(np.flatnonzero(np.concatenate([[False], ~empty, [False]])))
    print("%d vertices, %d triangles in %d of %d blocks, the longest stretch of empty blocks %d" % (want[0].shape[0], want[2].shape[0], (~empty).sum(), nblk, runs.max() - 1))
    assert nblk > 1024 and -(-nblk // SCAN_TILE) == 2
    assert per_block[:SCAN_TILE].sum() > 0 and per_block[SCAN_TILE:].sum() > 0 and per_block[SCAN_TILE:].sum() != want[2].shape[0]
    assert 0.2 < empty.mean() < 0.9 and runs.max() - 1 >= 8 and want[2].shape[0] > 50000 and per_block.max() > 255
    dev = _written(vol)
    _assert_mesh(dev, vol, 1.0, "the scan at scale", want)
    dev.close()


# ---- 4. capacity ----------------------------------------------------------------------------------------------------------------------------

def test_capacity(engine):
    vol = _plane()
    cloud, nrm, tri = M.extract(vol)
    n, m = cloud.shape[0], tri.shape[0]
    assert n > 400 and m > 700
    dev = _written(vol)
    assert _raw(dev, 1.0, 1, 0, None, None, 0, None) == (0, n, m)                # the counting call makes both counts
    assert _raw(dev, 1.0, 0, 0, None, None, 0, None, opt=False) == (0, n, m)
    SENT = 0xA5A5A5A5

    def call(vcap, tcap, normals=1):
        got, gotn, gott = np.full((vcap + 3, 8), -7, F32), np.full((vcap + 3, 4), -7, F32), np.full((tcap + 3, 3), SENT, np.uint32)
        assert _raw(dev, 1.0, normals, vcap, got, gotn if normals else None, tcap, gott) == (0, n, m), (vcap, tcap)
        a, b = min(n, vcap), min(m, tcap)
        assert_bits(got[:a], cloud[:a], "vertex capacity %d: the prefix" % vcap)
        assert (got[a:] == -7).all() and (gotn[a:] == -7).all(), vcap
        if normals:
            assert_bits(gotn[:a], nrm[:a], "vertex capacity %d: the prefix's normals" % vcap)
        else:
            assert (gotn == -7).all()
        assert np.array_equal(gott[:b], tri[:b]) and (gott[b:] == SENT).all(), tcap

    for cap in (1, n - 1, n, n + 5):
        call(cap, m)
        call(cap, m, normals=0)
    for cap in (1, m - 1, m, m + 5):
        call(n, cap)
    call(0, m)                                                                   # no vertex is written: the indices are the full ones
    call(n, 0)
    c5 = dev.extract_mesh(vertex_capacity=7, triangle_capacity=9)
    assert c5[3:] == (n, m) and c5[0].shape[0] == 7 == c5[1].shape[0] and np.array_equal(c5[2], tri[:9])
    c5 = dev.extract_mesh(triangle_capacity=m)
    assert c5[3:] == (n, m) and c5[0].shape[0] == 0 and np.array_equal(c5[2], tri)
    _assert_volume(dev, vol, "the volume afterwards")
    dev.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_everything_as_it_was(engine):
    from icp_amd import tsdf
    vol = _plane()
    dev = _written(vol)
    want = M.extract(vol)
    n, m = want[0].shape[0], want[2].shape[0]
    cloud, nrm, tri = np.full((n, 8), -7, F32), np.full((n, 4), -7, F32), np.full((m, 3), 0xA5A5A5A5, np.uint32)
    L, t = tsdf._lib(), dev._t

    def refused(res, counts=(0xDEAD, 0xBEEF)):
        assert res[0] == EINVAL and b"icp_tsdf_extract_mesh" in L.icp_tsdf_last_error(t), (res, L.icp_tsdf_last_error(t))
        assert res[1:] == counts
        assert (cloud == -7).all() and (nrm == -7).all() and (tri == 0xA5A5A5A5).all()
        _assert_volume(dev, vol, "the volume after a refusal")

    refused(_raw(dev, 1.0, 1, n, cloud, nrm, m, tri, counts=(False, True)))          # a NULL vertex count
    refused(_raw(dev, 1.0, 1, n, cloud, nrm, m, tri, counts=(True, False)))          # a NULL triangle count
    for bad in (0.5, 0.0, -1.0, float("nan"), float("inf")):
        refused(_raw(dev, bad, 1, n, cloud, nrm, m, tri))
    for bad in (2, 0xFFFFFFFF):
        refused(_raw(dev, 1.0, bad, n, cloud, nrm, m, tri))
    refused(_raw(dev, 1.0, 1, n, None, nrm, m, tri))                                 # a NULL output with a capacity
    refused(_raw(dev, 1.0, 0, n, None, None, m, tri))
    refused(_raw(dev, 1.0, 1, n, cloud, None, m, tri))                               # normals wanted
    refused(_raw(dev, 1.0, 1, n, cloud, nrm, m, None))                               # triangles wanted
    refused(_raw(dev, 1.0, 1, 0, None, None, 1, None))
    with pytest.raises(engine.ICPError) as e:
        dev.extract_mesh(min_weight=0.0)
    assert e.value.code == EINVAL and "min_weight" in str(e.value)
    assert _raw(dev, 1.0, 1, n, cloud, nrm, m, tri) == (0, n, m)                     # and the same arguments made good pass
    assert_bits(cloud, want[0], "made good: vertices")
    assert np.array_equal(tri, want[2])
    dev.close()


# ---- 6. an empty volume ---------------------------------------------------------------------------------------------------------------------

def test_an_empty_volume_leaves_the_outputs_untouched(engine):
    cfg = T.volume_config(24, 20, 12, 1.0, (0.0, 0.0, 0.0), 4.0, colour=1)
    ref, dev = T.Volume(cfg), _device_volume(cfg)
    want = M.extract(ref)
    assert want[0].shape == (0, 8) and want[2].shape == (0, 3)
    cloud, nrm, tri = np.full((4, 8), -7, F32), np.full((4, 4), -7, F32), np.full((4, 3), 9, np.uint32)
    assert _raw(dev, 1.0, 1, 4, cloud, nrm, 4, tri) == (0, 0, 0)
    assert (cloud == -7).all() and (nrm == -7).all() and (tri == 9).all()
    got = dev.extract_mesh()
    assert got[0].shape == (0, 8) and got[1].shape == (0, 4) and got[2].shape == (0, 3)
    dev.close()


# ---- 7. interleaving ------------------------------------------------------------------------------------------------------------------------

def test_interleaved_with_extract_surface(engine):
    vol = _plane()
    want = M.extract(vol)
    assert want[2].shape[0] > 700
    dev = _written(vol)
    _assert_surface(dev, vol, 1.0, "extract_surface before", want[:2])
    _assert_mesh(dev, vol, 1.0, "extract_mesh between", want)
    _assert_surface(dev, vol, 1.0, "extract_surface after", want[:2])
    _assert_volume(dev, vol, "the volume afterwards")
    dev.close()


# ---- 8. the size limit ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz, refused", [(822, True), (821, False)])
def test_the_size_limit(engine, nz, refused):
    from icp_amd import tsdf
    assert (5 * 1023 * 1023 * (nz - 1) > 2 ** 32 - 1) == refused
    try:
        dev = _device_volume(T.volume_config(1024, 1024, nz, 1.0, (0.0, 0.0, 0.0), 4.0))
    except engine.ICPError as e:
        if e.code == ENOMEM:
            pytest.skip("the device cannot hold 1024 x 1024 x %d voxels" % nz)
        raise
    res = _raw(dev, 1.0, 0, 0, None, None, 0, None)
    if refused:
        assert res == (EINVAL, 0xDEAD, 0xBEEF) and b"icp_tsdf_extract_mesh" in tsdf._lib().icp_tsdf_last_error(dev._t)
    else:
        assert res == (0, 0, 0)
    dev.close()


# ---- 9. the layers above --------------------------------------------------------------------------------------------------------------------

def test_cpp_facade_program():
    """tests/cpp/tsdf_mesh_facade_test.cpp: TSDFVolume::extractMesh against the C-ABI it wraps."""
    exe = os.path.join(ROOT, "tests", "cpp", "tsdf_mesh_facade_test")
    assert os.path.exists(exe), "tests/cpp/tsdf_mesh_facade_test is built by build() / make tsdf_mesh_facade_test"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tsdf mesh facade ok" in out.stdout, (out.stdout, out.stderr)


def test_timing_entry_times_the_mesh(engine):
    vol = _plane()
    assert M.extract(vol)[2].shape[0] > 700
    dev = _written(vol)
    empty = _device_volume(vol.cfg)
    for what in (5, 6, 7):
        assert dev.time_kernel(what, reps=2) > 0
        assert empty.time_kernel(what, reps=2) > 0                             # (no triangle: the cell sweep alone, or nothing between the events)
    _assert_volume(dev, vol, "the volume after the timed extractions")
    _assert_mesh(dev, vol, 1.0, "after the timed extractions")
    dev.close(); empty.close()


def test_extract_mesh_after_track_to_model(engine):
    """The product of the pipeline: test_extract_surface_after_track_to_model's four tracked frames, then the model's mesh."""
    import icp_checks as K
    from icp_amd import rgbd, tsdf
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
    want = M.extract(ref)
    print("after four tracked frames: %d vertices, %d triangles" % (want[0].shape[0], want[2].shape[0]))
    assert want[0].shape[0] > 3000 and want[2].shape[0] > 5000 and M.edge_figures(want[2])[0]
    _assert_mesh(dev, ref, 1.0, "the tracked model", want)
    g.close(); dev.close()
