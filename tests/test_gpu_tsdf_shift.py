"""GPU tests of the moving volume (icp_tsdf_shift.hip, icp_tsdf_surface.hip: icp_tsdf_extract_surface_region; icp_amd/tsdf.py: shift,
window, extract_surface_region, the generators' follow) against its numpy restatement (tsdf_shift_ref.py): every voxel, origin and record
bit for bit, every count equal.  Every condition that makes a case what it is called is asserted on the restatement first.

Not tested: volumes whose byte offsets pass 2^32 (1024^3 voxels, or colour from 2^28 voxels on).  A test of that size does not fit in
seconds; the size_t arithmetic of k_tsdf_shift is checked by reading the code."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import rgbd_ref as R
import tsdf_ref as T
import tsdf_register_ref as G
import tsdf_shift_ref as H
import tsdf_surface_ref as S
from icp_checks import assert_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
F32 = np.float32
RUN = 1024                                  # voxels of a block of the sweep (icp_tsdf_surface.hip)
SHIFTS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, -1), (3, -2, 5), (-7, 4, -3), (23, 0, 0), (24, 0, 0), (0, -100, 0), (0, 0, 0)]


def _device(vol):
    """A device volume with the restatement's contents (and, never shifted yet, its origin)."""
    from icp_amd import tsdf
    assert H.window(vol)[1] == (0, 0, 0)
    dev = tsdf.TSDFVolume(tsdf.TSDFConfig(**vol.cfg))
    dev.write(vol.dw, vol.rgb)
    return dev


def _assert_state(dev, ref, what, surface=False):
    """Contents, origin and window of the device against the restatement's; with `surface` the full extraction with normals too."""
    dw, col = dev.read()
    assert_bits(dw, ref.dw, what + ": {D, W}")
    if ref.rgb is not None:
        assert_bits(col, ref.rgb, what + ": colour")
    want = np.array(ref.cfg["origin"], F32)
    assert_bits(np.array(dev.get_config().origin, F32), want, what + ": the origin of get_config")
    assert_bits(np.array(dev.cfg.origin, F32), want, what + ": the origin of the cached configuration")
    assert dev.window() == tuple(H.window(ref)[1]), (what, dev.window(), H.window(ref))
    if surface:
        cloud, nrm = S.extract(ref)
        got, gotn = dev.extract_surface()
        assert got.shape[0] == cloud.shape[0], (what, got.shape[0], cloud.shape[0])
        assert_bits(got, cloud, what + ": the surface")
        assert_bits(gotn, nrm, what + ": its normals")
        return cloud.shape[0]


def _key(vol, info):
    return 3 * ((info["index"][:, 2] * vol.cfg["ny"] + info["index"][:, 1]) * vol.cfg["nx"] + info["index"][:, 0]) + info["axis"]


def _plane_with_edges():
    """The tilted plane with colour and 3 % holes, one NaN with a payload and one -0 in D."""
    vol = H.plane(holes=True)
    vol.dw[6, 9, 11, 0] = np.array([0x7FC12345], np.uint32).view(F32)[0]
    vol.dw[5, 8, 10] = (F32(-0.0), 1)
    return vol


# ---- 1. the shift against the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tilted plane with colour and holes", "checkerboard 70 x 9 x 5", "2 x 2 x 2"])
def test_shift_against_the_restatement(engine, name):
    if name.startswith("tilted"):
        vol = _plane_with_edges()
        assert (vol.dw[..., 1] == 0).mean() > 0.02 and np.isnan(vol.dw[..., 0]).sum() == 1
    elif name.startswith("checkerboard"):
        vol = H.checkerboard()
        vol.dw[2, 4, 33, 0], vol.dw[2, 4, 34, 0] = np.array([0xFFC00001], np.uint32).view(F32)[0], F32(-0.0)
        assert vol.cfg["nx"] % 64 and vol.rgb is None
    else:
        vol = T.Volume(T.volume_config(2, 2, 2, 1.5, (-2.0, 1.0, 0.5), 4.0, colour=1))
        vol.dw[...] = np.array([[-0.5, 1], [0.5, 1], [0.25, 1], [-0.0, 1], [0.75, 2], [np.nan, 1], [-0.25, 3], [0.5, 1]], F32).reshape(2, 2, 2, 2)
        vol.rgb[...] = np.arange(24, dtype=F32).reshape(2, 2, 2, 3) / F32(24)
    dev = _device(vol)
    cur = vol
    dims = (vol.cfg["nx"], vol.cfg["ny"], vol.cfg["nz"])
    survived_nan = survived_zero = emptied = members = 0
    for s in SHIFTS:
        # the contents are written again before every shift (the large shifts empty the volume); the window accumulates
        fresh = T.Volume(cur.cfg)
        fresh.dw, fresh.rgb = vol.dw.copy(), None if vol.rgb is None else vol.rgb.copy()
        fresh.base, fresh.window = H.window(cur)
        dev.write(vol.dw, vol.rgb)
        cur = H.shift(fresh, s)
        assert dev.shift(s) is None
        nan = np.isnan(cur.dw[..., 0])
        if nan.any():                                          # the NaN's payload and sign, and the -0, where they stay inside
            survived_nan += 1
            assert cur.dw[..., 0].view(np.uint32)[nan][0] in (0x7FC12345, 0xFFC00001, np.array([np.nan], F32).view(np.uint32)[0])
        survived_zero += int(((cur.dw[..., 0] == 0) & np.signbit(cur.dw[..., 0]) & (cur.dw[..., 1] > 0)).any())
        assert (not cur.dw.view(np.uint32).any()) == any(abs(s[a]) >= dims[a] for a in range(3)), s        # |s_a| >= n_a empties the volume
        emptied += int(not cur.dw.view(np.uint32).any())
        members += _assert_state(dev, cur, "%s after the shift %s" % (name, (s,)), surface=True)
    total = tuple(sum(s[a] for s in SHIFTS) for a in range(3))
    assert H.window(cur)[1] == total and dev.window() == total
    assert emptied >= 2 and survived_nan >= 2 and survived_zero >= 2 and members > 0
    dev.close()


def test_a_thousand_shifts_round_once(engine):
    from icp_amd import tsdf
    cfg = T.volume_config(2, 2, 2, 0.1, (0.3, -7.7, 1e3), 0.4)
    dev = tsdf.TSDFVolume(tsdf.TSDFConfig(**cfg))
    for _ in range(1000):
        dev.shift((1, -1, 1))
    once = H.shift(T.Volume(cfg), (1000, -1000, 1000))
    _assert_state(dev, once, "1000 shifts of one voxel")
    acc = np.array(cfg["origin"], F32)
    for _ in range(1000):
        acc = acc + np.array([1, -1, 1], F32) * F32(0.1)
    assert not np.array_equal(acc.view(np.uint32), np.array(once.cfg["origin"], F32).view(np.uint32))        # (accumulated, it would differ)
    dev.close()


# ---- 2. every kernel sees the moved window ---------------------------------------------------------------------------------------------------

def test_every_entry_sees_the_moved_window(engine):
    from icp_amd import rgbd
    cam = T.corner_camera()
    rc = rgbd.RGBDConfig(**cam)
    cfg = T.corner_volume(colour=1, dims=(48, 44, 40))
    ref = T.Volume(cfg)
    dev = _device(ref)
    frames = []
    for eye in T.EYES[:4]:
        P = T.look_at(eye)
        frames.append((P.reshape(12).astype(F32),) + T.render_corner(P, cam)[:2])
    for pose, depth, rgb in frames[:3]:
        T.integrate(ref, cam, pose, depth, rgb)
        dev.integrate(rc, pose, depth, rgb)
    s = (3, -2, 4)
    ref = H.shift(ref, s)
    dev.shift(s)
    _assert_state(dev, ref, "the fused corner after the shift")
    pose, depth, rgb = frames[3]
    changed = T.integrate(ref, cam, pose, depth, rgb)["changed"]
    dev.integrate(rc, pose, depth, rgb)
    entered = np.zeros(changed.shape, bool)
    entered[-4:], entered[:, :2] = True, True                  # the slabs that entered empty: k >= nz - 4, j < 2
    assert changed.sum() > 5000 and (changed & entered).sum() > 100
    _assert_state(dev, ref, "a frame integrated after the shift", surface=True)
    view = G.p12(T.look_at(T.EYE_CAST))
    cloud, nrm, lam = T.raycast(ref, cam, view, 200.0, 1600.0)
    hits = ~np.isnan(lam)
    assert hits.sum() > 2000 and np.any(nrm[:, :3] != 0, axis=1).sum() > 1500
    got, gotn = dev.raycast(rc, view, 200.0, 1600.0)
    assert_bits(got, cloud, "the ray cast after the shift")
    assert_bits(gotn, nrm, "its normals")
    moving = R.cloud(*T.render_corner(G.TRUE_1, cam)[:2], cam)
    want = G.register(ref, moving, G.p12(G.START), 3)
    assert want.members > 1000 and not want.singular and want.iterations >= 1
    rec = dev.register(moving, G.p12(G.START), 3)
    assert_bits(rec.pose, want.pose, "the registration after the shift: pose")
    assert (rec.iterations, rec.members, rec.singular) == (want.iterations, want.members, want.singular)
    assert_bits(rec.sys, want.sys, "the registration after the shift: the 27 sums")
    # against a volume that kept the stale origin the same calls give something else
    stale = T.Volume(dict(ref.cfg, origin=cfg["origin"]))
    stale.dw, stale.rgb = ref.dw, ref.rgb
    assert not np.array_equal(T.raycast(stale, cam, view, 200.0, 1600.0)[0], cloud)
    dev.close()


# ---- 3. two buffers --------------------------------------------------------------------------------------------------------------------------

def test_the_two_buffers(engine):
    vol = _plane_with_edges()
    dev = _device(vol)
    there = H.shift(vol, (5, 0, 0))
    back = H.shift(there, (-5, 0, 0))
    assert vol.dw[:, :, :5].view(np.uint32).any() and not back.dw[:, :, :5].view(np.uint32).any() and not back.rgb[:, :, :5].view(np.uint32).any()
    assert np.array_equal(back.dw[:, :, 5:].view(np.uint32), vol.dw[:, :, 5:].view(np.uint32)) and H.window(back)[1] == (0, 0, 0)
    dev.shift((5, 0, 0))
    _assert_state(dev, there, "shifted by (5, 0, 0)")
    dev.shift((-5, 0, 0))
    _assert_state(dev, back, "and back: the slab that re-enters is empty", surface=True)
    # three shifts in a row: the live buffers are the second pair; write, read and reset act on them
    cur = back
    for s in ((1, 2, 0), (0, -1, 1), (2, 0, -1)):
        cur = H.shift(cur, s)
        dev.shift(s)
    _assert_state(dev, cur, "three shifts in a row", surface=True)
    other = H.random_volume()
    written = T.Volume(dict(cur.cfg))
    written.base, written.window = H.window(cur)
    written.dw = other.dw.copy()
    written.rgb = np.random.default_rng(3).random(cur.rgb.shape).astype(F32)
    dev.write(written.dw, written.rgb)
    _assert_state(dev, written, "written after the shifts", surface=True)
    nxt = H.shift(written, (0, 0, 2))
    dev.shift((0, 0, 2))
    _assert_state(dev, nxt, "shifted after the write", surface=True)
    dev.reset()
    empty = T.Volume(dict(nxt.cfg))
    empty.base, empty.window = H.window(nxt)
    assert H.window(empty)[1] == (3, 1, 2)
    assert _assert_state(dev, empty, "reset keeps the window and clears the voxels", surface=True) == 0
    dev.close()


# ---- 4. region extraction ------------------------------------------------------------------------------------------------------------------

def _boxes(dims):
    nx, ny, nz = dims
    boxes = {"mid block to mid block": ((5, ny // 3, 1), (nx - 5, ny - 2, nz - 1)), "empty": ((3, 3, 2), (3, ny, nz)), "full": ((0, 0, 0), dims),
             "one voxel": ((5, 6, 3), (6, 7, 4)), "one cell": ((5, 6, 3), (7, 8, 5))}
    for a, n in enumerate(dims):
        w = max(1, n // 5)
        lo, hi = [0, 0, 0], list(dims)
        hi[a] = w
        boxes["low face of axis %d" % a] = (tuple(lo), tuple(hi))
        lo, hi = [0, 0, 0], list(dims)
        lo[a] = n - w
        boxes["high face of axis %d" % a] = (tuple(lo), tuple(hi))
    return boxes


def _assert_region(dev, full, lo, hi, what):
    """Both kinds of the box against the restatement's filter of the full extraction; (inside count, outside count)."""
    cloud, nrm, info = full
    counts = []
    for outside in (False, True):
        keep = H.inside(info, lo, hi) != outside
        got, gotn = dev.extract_surface_region(lo, hi, outside)
        assert got.shape[0] == keep.sum(), (what, outside, got.shape[0], keep.sum())
        assert_bits(got, cloud[keep], "%s, %s: cloud" % (what, "OUTSIDE" if outside else "INSIDE"))
        assert_bits(gotn, nrm[keep], "%s, %s: normals" % (what, "OUTSIDE" if outside else "INSIDE"))
        only, none = dev.extract_surface_region(lo, hi, outside, normals=False)
        assert none is None
        assert_bits(only, cloud[keep], "%s, %s: cloud without normals" % (what, "OUTSIDE" if outside else "INSIDE"))
        counts.append(int(keep.sum()))
    assert sum(counts) == cloud.shape[0]
    return counts


@pytest.mark.parametrize("name", ["tilted plane with colour and holes", "random D", "checkerboard 70 x 9 x 5"])
def test_region_extraction(engine, name):
    vol = _plane_with_edges() if name.startswith("tilted") else H.random_volume() if name.startswith("random") else H.checkerboard()
    dims = (vol.cfg["nx"], vol.cfg["ny"], vol.cfg["nz"])
    info = {}
    full = S.extract(vol, 1.0, info) + (info,)
    assert full[0].shape[0] > 400
    dev = _device(vol)
    boxes = _boxes(dims)
    lo, hi = boxes["mid block to mid block"]
    first, last = (lo[2] * dims[1] + lo[1]) * dims[0] + lo[0], ((hi[2] - 1) * dims[1] + hi[1] - 1) * dims[0] + hi[0] - 1
    assert first % RUN and (last + 1) % RUN and first // RUN < last // RUN, (first, last)
    both = 0
    for what, (lo, hi) in boxes.items():
        n_in, n_out = _assert_region(dev, full, lo, hi, "%s, %s" % (name, what))
        print("%s, %s %s %s: %d inside, %d outside" % (name, what, lo, hi, n_in, n_out))
        if what == "empty" or what == "one voxel":
            assert n_in == 0
        if what == "full":
            assert n_out == 0
        if what == "one cell" and name.startswith("checkerboard"):
            assert n_in == 12
        both += n_in > 0 and n_out > 0
        _assert_state(dev, vol, "%s: the volume after the region %s" % (name, what))
    assert both >= 5
    dev.close()


def _raw_region(dev, lo, hi, mode, min_weight, normals, capacity, cloud, nrm, region=True):
    from icp_amd import tsdf
    o, count = tsdf.icp_tsdf_surface_t(min_weight, normals), C.c_uint32(0xDEAD)
    box = tsdf.icp_tsdf_region_t((C.c_uint32 * 3)(*lo), (C.c_uint32 * 3)(*hi), mode)
    rc = tsdf._lib().icp_tsdf_extract_surface_region(dev._t, C.byref(o), C.byref(box) if region else None, capacity,
                                                     None if cloud is None else cloud.ctypes.data, None if nrm is None else nrm.ctypes.data, C.byref(count))
    return rc, count.value


def test_region_capacity(engine):
    vol = H.plane()
    info = {}
    cloud, nrm = S.extract(vol, 1.0, info)
    lo, hi = (0, 0, 0), (24, 11, 12)
    for mode in (0, 1):
        keep = H.inside(info, lo, hi) != bool(mode)
        n = int(keep.sum())
        assert 100 < n < cloud.shape[0] - 100
        dev = _device(vol)
        assert _raw_region(dev, lo, hi, mode, 1.0, 1, 0, None, None) == (0, n)                       # the counting call
        for cap in (1, n - 1, n, n + 5):
            for normals in (1, 0):
                got, gotn = np.full((cap + 3, 8), -7, F32), np.full((cap + 3, 4), -7, F32)
                assert _raw_region(dev, lo, hi, mode, 1.0, normals, cap, got, gotn if normals else None) == (0, n), cap
                m = min(n, cap)
                assert_bits(got[:m], cloud[keep][:m], "capacity %d: the prefix" % cap)
                assert (got[m:] == -7).all() and (gotn[m:] == -7).all(), cap
                if normals:
                    assert_bits(gotn[:m], nrm[keep][:m], "capacity %d: the prefix's normals" % cap)
                else:
                    assert (gotn == -7).all()
            c3 = dev.extract_surface_region(lo, hi, bool(mode), capacity=cap)
            assert c3[2] == n and c3[0].shape[0] == min(n, cap) == c3[1].shape[0]
        _assert_state(dev, vol, "the volume afterwards")
        dev.close()


def test_region_at_the_scan_at_scale(engine):
    """160 x 96 x 80 voxels, the two-tile scan case of tests/test_gpu_tsdf_surface.py (1200 blocks of the sweep): slabs of width 12 along z
    (the sweep covers a run of blocks), y and x (whole waves inside or outside the box)."""
    nx, ny, nz = 160, 96, 80
    vol = T.Volume(T.volume_config(nx, ny, nz, 4.0, (-320.0, -192.0, 0.0), 16.0))
    on = np.random.default_rng(7).random((nz // 8, ny // 8, nx // 8)) < 0.03
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol.dw[..., 0] = np.where((i + j + k) % 2 == 0, 1, -1) * np.random.default_rng(8).uniform(0.25, 0.75, i.shape)
    vol.dw[..., 1] = on[k // 8, j // 8, i // 8]
    info = {}
    full = S.extract(vol, 1.0, info) + (info,)
    assert full[0].shape[0] > 50000 and (nx * ny * nz + RUN - 1) // RUN > 1024
    dev = _device(vol)
    for what, lo, hi in (("z slab", (0, 0, 30), (nx, ny, 42)), ("low z slab", (0, 0, 0), (nx, ny, 12)), ("kept box of a shift along -z", (0, 0, 0), (nx, ny, nz - 12)),
                         ("y slab", (0, 40, 0), (nx, 52, nz)), ("x slab", (70, 0, 0), (82, ny, nz))):
        n_in, n_out = _assert_region(dev, full, lo, hi, what)
        print("%s: %d inside, %d outside" % (what, n_in, n_out))
        assert n_in > 1000 and n_out > 1000
    assert H.kept_box(vol.cfg, (0, 0, -12)) == ((0, 0, 0), (nx, ny, nz - 12))
    _assert_state(dev, vol, "the volume afterwards")
    dev.close()


# ---- 5. shift and extract lose nothing -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voxel, origin", [(1.0, (0.0, 0.0, 0.0)), (0.37, (0.3, -7.7, 5.1))], ids=["unit voxels", "voxels of 0.37"])
def test_shift_and_extract_lose_nothing(engine, voxel, origin):
    vol = H.plane()
    vol.cfg.update(voxel=voxel, origin=origin)
    old_info = {}
    old = S.extract(vol, 1.0, old_info)
    assert old[0].shape[0] > 400
    left = 0
    for s in ((6, 0, 0), (0, -5, 0), (0, 0, 4), (-3, 2, -1)):
        dev = _device(vol)
        lo, hi = H.kept_box(vol.cfg, s)
        want_leaving = H.extract_region(vol, lo, hi, True)
        after = H.shift(vol, s)
        leaving = dev.shift(s, extract=True)
        assert leaving[0].shape[0] == want_leaving[0].shape[0]
        left += leaving[0].shape[0]
        assert_bits(leaving[0], want_leaving[0], "shift %s: the leaving cloud" % (s,))
        assert_bits(leaving[1], want_leaving[1], "shift %s: its normals" % (s,))
        new_info = {}
        new = S.extract(after, 1.0, new_info)
        _assert_state(dev, after, "after shift %s" % (s,), surface=True)
        assert leaving[0].shape[0] + new[0].shape[0] == old[0].shape[0]
        stay = H.inside(old_info, lo, hi)
        assert stay.sum() == new[0].shape[0] > 100
        assert np.array_equal(old_info["index"][stay] - np.array(s), new_info["index"]) and np.array_equal(old_info["axis"][stay], new_info["axis"])
        # The positions of a member that stays.  Both sides evaluate p = fl (o + fl (fl (idx + t) * voxel)) with the same t (the ends' D are the
        # same bits), and in real numbers both are base + (c + idx + t) voxel.  With M >= every magnitude that appears (the origins, n voxel,
        # the coordinates): fl (idx + t) is off by <= ulp (n) / 2, which the product scales to < ulp (n voxel) <= ulp (M); the product and the
        # sum round by <= ulp (M) / 2 each: 2 ulp (M) a side.  An origin is fl (base + fl (c voxel)): <= ulp (M) from its real value.  So the two
        # positions differ by at most (2 + 1) + (2 + 1) = 6 ulp (M).
        M = max(np.abs(old[0][:, :3]).max(), np.abs(new[0][:, :3]).max(), np.abs(np.array(after.cfg["origin"], F32)).max(), np.abs(np.array(origin, F32)).max(),
                max(H.PLANE_DIMS) * voxel)
        diff = np.abs(old[0][stay][:, :3].astype(np.float64) - new[0][:, :3].astype(np.float64)).max()
        print("shift %s: %d leave, %d stay, positions differ by at most %.3g = %.2f ulp of %.3f" % (s, leaving[0].shape[0], new[0].shape[0], diff, diff / np.spacing(F32(M)), M))
        assert diff <= 6 * float(np.spacing(F32(M)))
        assert_bits(old[0][stay][:, 3:], new[0][:, 3:], "shift %s: the colours of the members that stay" % (s,))
        dev.close()
    assert left > 300                                          # (the plane lies above k = 4: the shift (0, 0, 4) drops no member)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_everything_as_it_was(engine):
    from icp_amd import tsdf
    vol = H.plane()
    dev = _device(vol)
    dev.shift((1, 0, -1))
    ref = H.shift(vol, (1, 0, -1))
    n = S.extract(ref)[0].shape[0]
    assert n > 300
    cloud, nrm = np.full((n, 8), -7, F32), np.full((n, 4), -7, F32)
    L, t = tsdf._lib(), dev._t
    full = ((0, 0, 0), H.PLANE_DIMS)

    def refused(rc, count=None, entry=b"icp_tsdf_extract_surface_region"):
        assert rc == EINVAL and entry in L.icp_tsdf_last_error(t), (rc, L.icp_tsdf_last_error(t))
        assert count is None or count == 0xDEAD
        assert (cloud == -7).all() and (nrm == -7).all()
        _assert_state(dev, ref, "after a refusal")

    o = tsdf.icp_tsdf_surface_t(1.0, 1)
    box = tsdf.icp_tsdf_region_t((C.c_uint32 * 3)(0, 0, 0), (C.c_uint32 * 3)(*H.PLANE_DIMS), 0)
    refused(L.icp_tsdf_extract_surface_region(t, C.byref(o), C.byref(box), n, cloud.ctypes.data, nrm.ctypes.data, None))       # a NULL count
    refused(*_raw_region(dev, *full, 0, 1.0, 1, n, cloud, nrm, region=False))                                           # a NULL region
    for a in range(3):
        lo, hi = [0, 0, 0], list(H.PLANE_DIMS)
        lo[a], hi[a] = 5, 4
        refused(*_raw_region(dev, lo, hi, 0, 1.0, 1, n, cloud, nrm))                                                   # lo > hi
        lo, hi = [0, 0, 0], list(H.PLANE_DIMS)
        hi[a] += 1
        refused(*_raw_region(dev, lo, hi, 1, 1.0, 1, n, cloud, nrm))                                                   # hi > n
    for mode in (2, 0xFFFFFFFF):
        refused(*_raw_region(dev, *full, mode, 1.0, 1, n, cloud, nrm))
    for bad in (0.5, 0.0, -1.0, float("nan"), float("inf")):                                                                          # the surface options' own
        refused(*_raw_region(dev, *full, 0, bad, 1, n, cloud, nrm))
    for bad in (2, 0xFFFFFFFF):
        refused(*_raw_region(dev, *full, 0, 1.0, bad, n, cloud, nrm))
    refused(*_raw_region(dev, *full, 0, 1.0, 1, n, None, nrm))
    refused(*_raw_region(dev, *full, 0, 1.0, 0, n, None, None))
    refused(*_raw_region(dev, *full, 0, 1.0, 1, n, cloud, None))
    with pytest.raises(engine.ICPError) as e:
        dev.extract_surface_region((0, 0, 0), (25, 20, 12))
    assert e.value.code == EINVAL and "hi" in str(e.value)
    # the shift
    refused(L.icp_tsdf_shift(t, None), entry=b"icp_tsdf_shift")
    refused(L.icp_tsdf_get_window(t, None), entry=b"icp_tsdf_get_window")
    assert _raw_region(dev, *full, 0, 1.0, 1, n, cloud, nrm) == (0, n)                                                                # the same arguments made good pass
    assert_bits(cloud, S.extract(ref)[0], "the full box after the refusals")
    dev.close()
    # |c| > 2^24, reached by two shifts: the first passes (and empties the volume), the second is refused
    dev = _device(vol)
    cloud[:], nrm[:] = -7, -7
    t = dev._t
    dev.shift((2 ** 24 - 5, 0, -2 ** 24))
    ref = H.shift(vol, (2 ** 24 - 5, 0, -2 ** 24))
    assert H.refused(ref, (6, 0, 0)) and H.refused(ref, (0, 0, -1)) and not H.refused(ref, (5, 0, 1))
    refused(L.icp_tsdf_shift(t, (C.c_int32 * 3)(6, 0, 0)), entry=b"icp_tsdf_shift")
    refused(L.icp_tsdf_shift(t, (C.c_int32 * 3)(0, 0, -1)), entry=b"icp_tsdf_shift")
    with pytest.raises(engine.ICPError) as e:
        dev.shift((2 ** 31 - 1, 0, 0))
    assert e.value.code == EINVAL and "2^24" in str(e.value)
    dev.shift((5, 0, 1))
    ref = H.shift(ref, (5, 0, 1))
    _assert_state(dev, ref, "the bound itself passes")
    assert dev.window() == (2 ** 24, 0, 1 - 2 ** 24)
    dev.close()
    # an origin that overflows to infinity
    big = T.Volume(T.volume_config(2, 2, 2, 1e38, (3e38, 0.0, -3e38), 1e38))
    big.dw[...] = np.array([[-0.5, 1], [0.5, 1], [0.25, 1], [-0.25, 1], [0.75, 2], [0.1, 1], [-0.25, 3], [0.5, 1]], F32).reshape(2, 2, 2, 2)
    dev, ref = _device(big), big
    t = dev._t
    assert H.refused(big, (1, 0, 0)) and H.refused(big, (0, 0, -1)) and not H.refused(big, (-1, 0, 1))
    refused(L.icp_tsdf_shift(t, (C.c_int32 * 3)(1, 0, 0)), entry=b"icp_tsdf_shift")
    refused(L.icp_tsdf_shift(t, (C.c_int32 * 3)(0, 0, -1)), entry=b"icp_tsdf_shift")
    dev.shift((-1, 0, 1))
    _assert_state(dev, H.shift(big, (-1, 0, 1)), "the same volume shifted the other way")
    dev.close()


# ---- 7. the generators -------------------------------------------------------------------------------------------------------------------------

SCENE_CAM = dict(x0=2, y0=3, step_x=2, step_y=1)               # a lattice of 32 x 32 landmarks in the 80 x 60 image


@functools.lru_cache(maxsize=None)
def _scene():
    cam = T.corner_camera(**SCENE_CAM)
    poses = H.scene_poses(6)
    return cam, [G.p12(P) for P in poses], [T.render_corner(P, cam)[:2] for P in poses]


def _handle(engine, cam):
    from icp_amd import rgbd
    g = engine.ICP(0)
    g.init(32 * 32, 16, 2e2, 1e-6)
    rgbd.set_config(g, rgbd.RGBDConfig(**cam))
    return g


@pytest.mark.parametrize("which", ["track_to_volume", "track_to_model"])
def test_generators_follow_the_camera(engine, which):
    from icp_amd import tsdf
    cam, p12, frames = _scene()

    def run(**kw):
        g, dev = _handle(engine, cam), tsdf.TSDFVolume(tsdf.TSDFConfig(**H.scene_volume(1)))
        if which == "track_to_volume":
            out = list(tsdf.track_to_volume(g, dev, frames, p12[0], 10, **kw))
        else:
            out = list(tsdf.track_to_model(g, dev, frames, p12[0], 200.0, 1600.0, **kw))
        g.close()
        return out, dev

    left = []
    got, dev = run(follow=H.SCENE_FOLLOW, on_shift=lambda s, cloud, nrm: left.append((tuple(s), cloud.copy(), nrm.copy())))
    poses = [y[0] for y in got]
    assert len(poses) == 6
    assert_bits(poses[0], p12[0], "the first pose")
    ref, shifts, changed = H.run_scene(cam, poses, frames, H.SCENE_FOLLOW, colour=1)
    print("%s with follow: shifts %s, leaving %s, window %s, voxels changed per frame %s" % (which, [s for s, _, _ in shifts], [c.shape[0] for _, c, _ in shifts], H.window(ref)[1], changed))
    assert len(shifts) >= 1 and sum(c.shape[0] for _, c, _ in shifts) > 0
    assert [s for s, _, _ in left] == [tuple(s) for s, _, _ in shifts]
    for (s, c, n), (_, wc, wn) in zip(left, shifts):
        assert_bits(c, wc, "%s: the cloud that left with %s" % (which, (s,)))
        assert_bits(n, wn, "%s: its normals" % which)
    _assert_state(dev, ref, which + ": the volume after the last frame", surface=True)
    dev.close()
    # follow=None: the yields of a run without the keyword
    plain, dev_a = run()
    none, dev_b = run(follow=None, on_shift=None)
    assert len(plain) == len(none) == 6
    for a, b in zip(plain, none):
        assert_bits(a[0], b[0], which + ": poses with follow=None")
        if which == "track_to_model":
            assert a[1:] == b[1:]
        else:
            assert (a[1] is None) == (b[1] is None) and (a[1] is None or (a[1].iterations, a[1].members, a[1].singular) == (b[1].iterations, b[1].members, b[1].singular))
    assert dev_a.window() == dev_b.window() == (0, 0, 0)
    da, db = dev_a.read(), dev_b.read()
    assert_bits(da[0], db[0], which + ": the volumes with follow=None")
    fixed = H.run_scene(cam, [y[0] for y in plain], frames, None, colour=1)[0]
    _assert_state(dev_a, fixed, which + ": without follow the volume stays where it was")
    dev_a.close(); dev_b.close()


# ---- 8, 9. the layers above ----------------------------------------------------------------------------------------------------------------

def test_cpp_facade_program():
    """tests/cpp/tsdf_shift_facade_test.cpp: TSDFVolume::shift, window, extractSurfaceRegion, keptBox and shiftAndExtract against the C-ABI
    they wrap and the rule as host loops."""
    exe = os.path.join(ROOT, "tests", "cpp", "tsdf_shift_facade_test")
    assert os.path.exists(exe), "tests/cpp/tsdf_shift_facade_test is built by build() / make tsdf_shift_facade_test"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tsdf shift facade ok" in out.stdout, (out.stdout, out.stderr)


def test_timing_entries(engine):
    vol = _plane_with_edges()
    dev = _device(vol)
    dev.shift((0, 1, 0))                                       # (the second buffers exist and are the live ones' twins)
    ref = H.shift(vol, (0, 1, 0))
    for s in ((0, 0, 3), (2, -1, 0), (0, 0, -2)):
        assert dev.time_shift(10, s, reps=3) > 0
        _assert_state(dev, ref, "after the timed shifts by %s" % (s,))
        assert dev.time_shift(11, s, reps=3) > 0
        _assert_state(dev, ref, "after the timed region extractions for %s" % (s,), surface=True)
    fresh = _device(vol)                                       # never shifted: the timing entry allocates the second buffers itself
    assert fresh.time_shift(10, (1, 1, 1), reps=2) > 0 and fresh.time_shift(11, (0, 0, 0), reps=2) > 0
    _assert_state(fresh, vol, "a volume that was only timed", surface=True)
    dev.close(); fresh.close()
