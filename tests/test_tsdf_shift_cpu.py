"""CPU tests of the moving volume: the host-only entries (icp_tsdf_kept_box, icp_tsdf_follow) through the library against the numpy
restatement (tsdf_shift_ref.py), the properties of the rule that make a shift lose nothing — checked on the restatement, so that an
engine that equals it bit for bit cannot be bit-exactly wrong —, the origin's arithmetic, the kernels' resources, and the moving scene end
to end on the restatement."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tsdf_ref as T
import tsdf_shift_ref as H
import tsdf_surface_ref as S

F32 = np.float32


def _config(cfg):
    from icp_amd import tsdf
    return tsdf.TSDFConfig(**cfg)


# ---- kept_box and follow through the library ------------------------------------------------------------------------------------------

def test_kept_box_against_the_restatement():
    from icp_amd import tsdf
    dims = [(24, 20, 12), (2, 2, 2), (70, 9, 5), (1024, 2, 513)]
    values = lambda n: sorted({0, 1, -1, 3, -3, n - 1, 1 - n, n, -n, n + 1, -n - 1, 100000, -100000, 2 ** 31 - 1, -2 ** 31})
    checked = beyond = 0
    for nx, ny, nz in dims:
        cfg = T.volume_config(nx, ny, nz, 1.0, (0.0, 0.0, 0.0), 4.0)
        for a in range(3):
            for v in values((nx, ny, nz)[a]):
                for other in (0, 1, -2):
                    s = [other] * 3
                    s[a] = v
                    lo, hi = H.kept_box(cfg, s)
                    assert tsdf.kept_box(_config(cfg), s) == (lo, hi), (cfg, s)
                    assert all(0 <= lo[b] <= hi[b] <= (nx, ny, nz)[b] for b in range(3))
                    checked += 1
                    if abs(v) >= (nx, ny, nz)[a]:
                        assert lo[a] == hi[a], (s, lo, hi)        # the box is empty: everything leaves
                        beyond += 1
    assert checked > 400 and beyond > 100
    # the box is what the shift keeps: exactly the old voxels that have a new voxel
    cfg = T.volume_config(6, 5, 4, 1.0, (0.0, 0.0, 0.0), 4.0)
    vol = T.Volume(cfg)
    vol.dw[..., 1] = 1
    for s in itertools.product((-7, -2, 0, 1, 4), (-5, -1, 0, 2), (-4, 0, 3)):
        lo, hi = H.kept_box(cfg, s)
        assert int(H.shift(vol, s).dw[..., 1].sum()) == int(np.prod([hi[a] - lo[a] for a in range(3)])), s
    L = tsdf._lib()
    c, box, s3 = _config(cfg)._c(), tsdf.icp_tsdf_region_t(), (C.c_int32 * 3)(1, 2, 3)
    assert L.icp_tsdf_kept_box(None, s3, C.byref(box)) == 1 and L.icp_tsdf_kept_box(C.byref(c), None, C.byref(box)) == 1
    assert L.icp_tsdf_kept_box(C.byref(c), s3, None) == 1
    assert L.icp_tsdf_kept_box(C.byref(c), s3, C.byref(box)) == 0 and box.mode == tsdf.REGION_OUTSIDE == 1


def test_follow_against_the_restatement():
    from icp_amd import tsdf
    rng = np.random.default_rng(5)
    moved = stayed = at_threshold = halves = 0
    for dims, voxel, origin in (((24, 20, 12), 1.0, (0.0, 0.0, 0.0)), ((64, 64, 64), 16.0, (-64.0, -64.0, -64.0)), ((256, 255, 3), 4.0, (-512.3, 77.7, 1e4)),
                                ((2, 2, 2), 0.37, (1.0, -2.0, 3.0))):
        cfg = T.volume_config(*dims, voxel, origin, 4.0 * voxel)
        centre = [float(F32(origin[a])) + 0.5 * (dims[a] - 1.0) * float(F32(voxel)) for a in range(3)]
        points = [tuple(centre[a] + d * voxel for a in range(3)) for d in (0, 1, -1, 2.5, -2.5, 3, -3, 3.5, -3.5, 4.5, 1000.25)]
        points += [tuple(centre[a] + (d if a == b else 0.25) * voxel for a in range(3)) for b in range(3) for d in (3, -3, 5.5, -6.5, 2.5)]
        points += [tuple(rng.normal(centre, 30 * voxel)) for _ in range(40)]
        for p in points:
            for threshold in (0, 1, 3, 8, 2 ** 31):
                want = H.follow(cfg, p, threshold)
                assert tsdf.follow(_config(cfg), p, threshold) == want, (cfg, p, threshold)
                d = [(float(F32(p[a])) - centre[a]) / float(F32(voxel)) for a in range(3)]
                far = max(abs(x) for x in d)
                moved += any(want)
                stayed += not any(want)
                if far == threshold:
                    at_threshold += 1
                    assert want == (0, 0, 0)                    # d exactly at the threshold stays
                if far > threshold and any(abs(x) % 1 == 0.5 for x in d):
                    halves += 1
                    assert all(want[a] == (round(d[a])) for a in range(3))      # ties to even, as lrint and Python's round
    print("follow: %d moved, %d stayed, %d exactly at the threshold, %d with a d at .5" % (moved, stayed, at_threshold, halves))
    assert moved > 100 and stayed > 100 and at_threshold >= 10 and halves >= 10
    L = tsdf._lib()
    c, out, pt = _config(cfg)._c(), (C.c_int32 * 3)(), (C.c_float * 3)(0, 0, 0)
    assert L.icp_tsdf_follow(None, pt, 1, out) == 1 and L.icp_tsdf_follow(C.byref(c), None, 1, out) == 1 and L.icp_tsdf_follow(C.byref(c), pt, 1, None) == 1
    for bad in (float("nan"), float("inf"), 1e30):
        assert L.icp_tsdf_follow(C.byref(c), (C.c_float * 3)(0, bad, 0), 1, out) == 1
    assert L.icp_tsdf_shift(None, out) == 1 and L.icp_tsdf_get_window(None, out) == 1
    assert L.icp_tsdf_extract_surface_region(None, None, None, 0, None, None, None) == 1


def test_python_struct_is_the_headers():
    import os
    import subprocess
    from icp_amd import tsdf
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('#include "icp_amd.h"\nint main(void){ icp_tsdf_region_t r; r.lo[0] = 1u; r.hi[2] = 2u; r.mode = ICP_TSDF_REGION_OUTSIDE; (void) r;\n'
            "return (int) sizeof (icp_tsdf_region_t) - 28 + ICP_TSDF_REGION_INSIDE; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(root, "include"), "-x", "c", "-", "-c", "-o", "/dev/null"],
                       input=code.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert C.sizeof(tsdf.icp_tsdf_region_t) == 28 and [n for n, _ in tsdf.icp_tsdf_region_t._fields_] == ["lo", "hi", "mode"]


# ---- the rule's properties, on the restatement --------------------------------------------------------------------------------------------

def _random_boxes(dims, count, rng):
    boxes = []
    for _ in range(count):
        lo = [int(rng.integers(0, n + 1)) for n in dims]
        hi = [int(rng.integers(l, n + 1)) for l, n in zip(lo, dims)]
        boxes.append((tuple(lo), tuple(hi)))
    return boxes


@pytest.mark.parametrize("name", ["random volume", "tilted plane"])
def test_inside_and_outside_partition_the_extraction(name):
    vol = H.random_volume() if name == "random volume" else H.plane()
    info = {}
    cloud, nrm = S.extract(vol, 1.0, info)
    key = 3 * ((info["index"][:, 2] * vol.cfg["ny"] + info["index"][:, 1]) * vol.cfg["nx"] + info["index"][:, 0]) + info["axis"]
    assert cloud.shape[0] > 400 and np.all(np.diff(key) > 0)
    rng = np.random.default_rng(21)
    boxes = _random_boxes(H.PLANE_DIMS, 40, rng) + [((0, 0, 0), H.PLANE_DIMS), ((3, 3, 3), (3, 9, 9)), ((5, 6, 7), (6, 7, 8))]
    boxes += [((0, 0, 0), (24, 20, 7)), ((0, 0, 6), (24, 20, 12)), ((4, 3, 2), (20, 15, 9)), ((0, 0, 0), (12, 20, 12)), ((0, 8, 0), (24, 20, 12))]      # across the plane
    both = 0
    for lo, hi in boxes:
        Ii, Io = {}, {}
        ci, ni = H.extract_region(vol, lo, hi, False, 1.0, Ii)
        co, no = H.extract_region(vol, lo, hi, True, 1.0, Io)
        assert ci.shape[0] + co.shape[0] == cloud.shape[0], (lo, hi)
        ki = 3 * ((Ii["index"][:, 2] * vol.cfg["ny"] + Ii["index"][:, 1]) * vol.cfg["nx"] + Ii["index"][:, 0]) + Ii["axis"]
        ko = 3 * ((Io["index"][:, 2] * vol.cfg["ny"] + Io["index"][:, 1]) * vol.cfg["nx"] + Io["index"][:, 0]) + Io["axis"]
        assert not np.intersect1d(ki, ko).size and np.array_equal(np.sort(np.concatenate([ki, ko])), key)
        order = np.argsort(np.concatenate([ki, ko]), kind="stable")
        assert np.array_equal(np.concatenate([ci, co])[order].view(np.uint32), cloud.view(np.uint32))
        assert np.array_equal(np.concatenate([ni, no])[order].view(np.uint32), nrm.view(np.uint32))
        both += ci.shape[0] > 0 and co.shape[0] > 0
    assert both >= 12
    assert H.extract_region(vol, (0, 0, 0), H.PLANE_DIMS)[0].shape[0] == cloud.shape[0]                  # the full box: every member INSIDE
    assert H.extract_region(vol, (3, 3, 3), (3, 9, 9), True)[0].shape[0] == cloud.shape[0]               # an empty box: every member OUTSIDE


def test_extract_then_shift_loses_no_member():
    """OUTSIDE of kept_box (s), then the shift: the leaving members and the new volume's members number exactly the old ones.  A rule that
    looked at a member's low end alone would drop the members whose low end stays and whose high end leaves."""
    vol = H.random_volume()
    info = {}
    total = S.extract(vol, 1.0, info)[0].shape[0]
    nx, ny, nz = H.PLANE_DIMS
    shifts = [(5, 0, 0), (-5, 0, 0), (0, 4, 0), (0, -4, 0), (0, 0, 3), (0, 0, -3), (2, -3, 1), (-6, 2, -2), (nx, 0, 0), (0, -100, 0)]
    for s in shifts:
        lo, hi = H.kept_box(vol.cfg, s)
        leaving = H.extract_region(vol, lo, hi, True)[0].shape[0]
        after = S.extract(H.shift(vol, s))[0].shape[0]
        straddle = int((H.inside(info, lo, hi, v_only=True) & ~H.inside(info, lo, hi)).sum())
        v_only = int((~H.inside(info, lo, hi, v_only=True)).sum())
        print("shift %s: %d leave, %d stay, %d with the low end in the box and the high end outside" % (s, leaving, after, straddle))
        assert leaving + after == total, s
        assert H.extract_region(vol, lo, hi, False)[0].shape[0] == after
        if any(x < 0 for x in s) and all(abs(x) < n for x, n in zip(s, H.PLANE_DIMS)):
            assert straddle >= 3 and v_only + after == total - straddle < total, s       # the low-end rule falls short by exactly these
    assert S.extract(H.shift(vol, (nx, 0, 0)))[0].shape[0] == 0


# ---- the origin ---------------------------------------------------------------------------------------------------------------------------

def test_the_origin_is_recomputed_never_accumulated():
    cfg = T.volume_config(2, 2, 2, 0.1, (0.3, -7.7, 1e3), 0.4)
    one = T.Volume(cfg)
    for _ in range(1000):
        one = H.shift(one, (1, -1, 1))
    once = H.shift(T.Volume(cfg), (1000, -1000, 1000))
    assert np.array_equal(np.array(one.cfg["origin"], F32).view(np.uint32), np.array(once.cfg["origin"], F32).view(np.uint32)) and H.window(one)[1] == (1000, -1000, 1000)
    acc = np.array(cfg["origin"], F32)
    for _ in range(1000):
        acc = acc + np.array([1, -1, 1], F32) * F32(0.1)
    assert not np.array_equal(acc.view(np.uint32), np.array(once.cfg["origin"], F32).view(np.uint32))    # (what accumulation would give)
    # the bound: |c| = 2^24 passes, 2^24 + 1 is refused, whichever way it is reached
    v = H.shift(T.Volume(cfg), (2 ** 24, -2 ** 24, 0))
    assert H.window(v)[1] == (2 ** 24, -2 ** 24, 0) and H.refused(v, (1, 0, 0)) and H.refused(v, (0, -1, 0)) and not H.refused(v, (-1, 1, 5))
    assert H.refused(T.Volume(cfg), (2 ** 24 + 1, 0, 0)) and int(F32(2 ** 24 + 1)) != 2 ** 24 + 1
    big = T.volume_config(2, 2, 2, 1e38, (3e38, 0.0, 0.0), 1e38)
    assert H.refused(T.Volume(big), (1, 0, 0)) and not H.refused(T.Volume(big), (-1, 0, 0))              # 3e38 + 1e38 is no float


# ---- the kernels' resources -----------------------------------------------------------------------------------------------------------------

def test_shift_kernels_compile_for_gfx950_without_scratch():
    from kernel_resources import kernel_resources
    res = kernel_resources("icp_amd/csrc/icp_tsdf_shift.hip")
    assert sorted(res) == ["k_tsdf_shift"], sorted(res)
    for n, r in res.items():
        assert r["scratch"] == 0 and r.get("dynamic_stack") in (None, "False") and r["lds"] == 0, (n, r)
    res = kernel_resources("icp_amd/csrc/icp_tsdf_surface.hip")
    region = [n for n in res if "k_tsdf_surface_count_region" in n]
    assert len(region) == 2, sorted(res)
    for n in region:
        assert res[n]["scratch"] == 0 and res[n].get("dynamic_stack") in (None, "False"), (n, res[n])


# ---- the moving scene, end to end on the restatement ------------------------------------------------------------------------------------------

def test_the_volume_follows_the_camera_along_the_wall():
    """The room corner at 80 x 60 pixels, six frames of a camera that slides 110 a frame along the wall y = 0, 40^3 voxels of 16: the cube is
    640 long and the path's views leave it.  Measured with this restatement (the figures the assertions guard): with follow, six shifts,
    4936 points in the leaving clouds and the final extraction together, the farthest 4.20 from its quarter-plane, x up to 1072 (the cube
    ended at 576); without follow the frames change 17860, 15104, 10839, 6707, 3220, 899 voxels."""
    cam = T.corner_camera()
    poses = H.scene_poses(6)
    frames = [T.render_corner(P, cam)[:2] for P in poses]
    p12 = [P.reshape(12).astype(F32) for P in poses]
    vol, shifts, changed = H.run_scene(cam, p12, frames, H.SCENE_FOLLOW)
    fixed, none, changed_fixed = H.run_scene(cam, p12, frames, None)
    assert not none and H.window(fixed)[1] == (0, 0, 0)
    cloud, nrm = S.extract(vol)
    every = np.concatenate([c for _, c, _ in shifts] + [cloud])
    every_n = np.concatenate([n for _, _, n in shifts] + [nrm])
    f = S.corner_surface_figures(every, every_n)
    end = -64.0 + 16.0 * H.SCENE_DIMS[0]
    print("with follow: shifts %s, window %s, %d points (%s leaving), farthest %.2f, x up to %.0f of a cube that ended at %.0f; voxels changed per frame %s, without follow %s"
          % ([s for s, _, _ in shifts], H.window(vol)[1], f["count"], [c.shape[0] for _, c, _ in shifts], f["dist"].max(), every[:, 0].max(), end, changed, changed_fixed))
    assert len(shifts) >= 3 and sum(c.shape[0] for _, c, _ in shifts) > 1000 and cloud.shape[0] > 1000
    assert (every[:, 0] > end).sum() > 500                      # the model holds points beyond the original cube
    assert f["dist"].max() < 8.0                                # the fused corner's bound for voxels of 16
    assert changed_fixed[-1] < changed_fixed[0] // 4 and changed[-1] > changed[0] // 2
