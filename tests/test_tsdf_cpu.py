"""CPU tests of the TSDF volume: the header's struct as C, compose_pose against float64, the argument checks that need no device, the
kernels' resources, and the rule itself (tsdf_ref.py) against an analytic scene, so that an engine that equals the restatement bit for
bit cannot be bit-exactly wrong."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_header_struct_is_plain_c():
    code = ('#include "icp_amd.h"\n'
            "int main(void){ icp_tsdf_t c; icp_tsdf_handle t = 0; c.nx = 64u; c.origin[2] = -1.f; c.w_max = 64.f; c.colour = 1u; (void) c; (void) t;\n"
            "return (int) sizeof (icp_tsdf_t) - 40; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-c", "-o", "/dev/null"],
                       input=code.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_python_struct_is_the_headers():
    from icp_amd import tsdf
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    body = hdr[hdr.index("typedef struct {\n    uint32_t nx, ny, nz;"):hdr.index("} icp_tsdf_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*\]", "", n).strip() for decl in re.findall(r"(?:uint32_t|float)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in tsdf.icp_tsdf_t._fields_] == list(tsdf.TSDFConfig.FIELDS) and C.sizeof(tsdf.icp_tsdf_t) == 40
    c = tsdf.TSDFConfig(24, 20, 12, 16.0, (-1, 2, 3), 48.0, 2.0, True)
    assert tsdf.TSDFConfig._from_c(c._c()).as_dict() == c.as_dict()


def test_compose_pose_against_float64():
    """out = pose o (R (q), t) in double, rounded once; the scale handed back, not applied; in place allowed; a zero quaternion refused."""
    from icp_amd import tsdf
    rng = np.random.default_rng(3)
    for _ in range(50):
        Q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        pose = np.concatenate([Q, rng.normal(scale=900.0, size=(3, 1))], 1).reshape(12).astype(F32)
        T8 = np.concatenate([rng.normal(size=4) * rng.uniform(0.5, 2.0), rng.normal(scale=50.0, size=3), [rng.uniform(0.9, 1.1)]]).astype(F32)
        got, s = tsdf.compose_pose(pose, T8)
        want, sw = T.compose_pose(pose, T8)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and F32(s) == sw == T8[7]
    ident, s = tsdf.compose_pose(pose, [0, 0, 0, 1, 0, 0, 0, 1])
    assert np.array_equal(ident, pose) and s == 1.0
    L = tsdf._lib()
    p = pose.copy()
    assert L.icp_tsdf_compose_pose(p.ctypes.data, T8.ctypes.data, p.ctypes.data, None) == 0 and np.array_equal(p, got)      # in place, no scale
    with pytest.raises(Exception):
        tsdf.compose_pose(pose, np.zeros(8, F32))
    with pytest.raises(ValueError):
        tsdf.compose_pose(pose[:11], T8)
    assert L.icp_tsdf_compose_pose(None, T8.ctypes.data, p.ctypes.data, None) == 1


BAD_FIELDS = T.BAD_FIELDS


def test_refusals_that_need_no_device():
    """Every out-of-range field of icp_tsdf_t is ICP_EINVAL with a message, before the device is looked at; NULL arguments are too."""
    from icp_amd import tsdf
    L = tsdf._lib()
    good = dict(nx=8, ny=8, nz=8, voxel=16.0, origin=(0.0, 0.0, 0.0), mu=48.0, w_max=64.0, colour=0)
    for field, value in BAD_FIELDS:
        c = tsdf.TSDFConfig(**dict(good, **{field: value}))._c()
        t = C.c_void_p(1)
        assert L.icp_tsdf_create(C.byref(t), 0, C.byref(c)) == 1 and not t.value, (field, value)
        assert b"icp_tsdf_create" in L.icp_tsdf_last_error(None), (field, value)
    c = tsdf.TSDFConfig(**good)._c()
    t = C.c_void_p()
    assert L.icp_tsdf_create(None, 0, C.byref(c)) == 1 and L.icp_tsdf_create(C.byref(t), 0, None) == 1
    for f in (L.icp_tsdf_destroy, L.icp_tsdf_reset):
        assert f(None) == 1
    assert L.icp_tsdf_get_config(None, C.byref(c)) == 1 and L.icp_tsdf_read(None, None, None) == 1 and L.icp_tsdf_write(None, None, None) == 1
    assert L.icp_tsdf_integrate(None, None, None, None, None) == 1 and L.icp_tsdf_raycast(None, None, None, 1.0, 2.0, 0, None, None) == 1
    assert L.icp_tsdf_raycast_to(None, None, 0, None, None, 1.0, 2.0, 0) == 1
    assert L.icp_tsdf_time(None, 0, None, None, None, None, 1.0, 2.0, 0, 1, None) == 1


def test_tsdf_kernels_compile_for_gfx950_without_scratch():
    from kernel_resources import kernel_resources
    res = kernel_resources("icp_amd/csrc/icp_tsdf.hip")
    assert sorted(res) == ["k_tsdf_integrate", "k_tsdf_raycast"], sorted(res)
    for n, r in res.items():
        assert r["scratch"] == 0 and r.get("dynamic_stack") in (None, "False") and r["lds"] == 0, (n, r)


def test_restatement_by_hand_on_one_voxel():
    """One voxel through the integrate rule written out operation by operation: twice seen (the running mean and the cap), then occluded."""
    cfg = T.volume_config(2, 2, 2, 10.0, (0.0, 0.0, 100.0), 30.0, w_max=1.0, colour=1)
    cam = T.corner_camera(width=4, height=4, fx=2.0, cx=1.5, cy=1.5)
    pose = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)
    vol = T.Volume(cfg)
    depth = np.full((4, 4), 115, np.uint16)
    rgb = np.full((4, 4, 3), 51, np.uint8)
    cls = T.integrate(vol, cam, pose, depth, rgb)
    # voxel (0, 0, 0) at (0, 0, 100): u = (2 * (0 / 100) + 1.5) + 0.5 = 2 -> pixel (2, 2); s = 15; e = 0.5
    assert vol.dw[0, 0, 0].tolist() == [0.5, 1.0] and vol.rgb[0, 0, 0, 0] == F32(51) / F32(255) and cls["changed"][0, 0, 0]
    # voxel (0, 0, 1) at z = 110: s = 5, e = 5 / 30
    assert vol.dw[1, 0, 0, 0] == F32(5) / F32(30)
    depth[:] = 160
    T.integrate(vol, cam, pose, depth, None)
    # e = min (1, 60 / 30) = 1; D' = (0.5 * 1 + 1) / 2; W' = min (2, 1) = 1; no colour image: C stays
    assert vol.dw[0, 0, 0].tolist() == [0.75, 1.0] and vol.rgb[0, 0, 0, 0] == F32(51) / F32(255)
    depth[:] = 60
    cls = T.integrate(vol, cam, pose, depth, rgb)
    assert cls["occluded"][0, 0, 0] and not cls["changed"].any() and vol.dw[0, 0, 0].tolist() == [0.75, 1.0]       # s = -40 < -mu
    depth[:] = 0
    assert T.integrate(vol, cam, pose, depth, rgb)["invalid"][0, 0, 0]


# The rule against the analytic room corner.  Measured with this restatement (the figures the assertions guard):
#   64^3 voxels of 16, mu 48: hits 0.9806; |lambda* - depth| max 11.22, median 0.42, p99 4.71; normals on 0.9533 of the hits;
#                             angles max 10.08 deg, median 2.10 deg
#   32^3 voxels of 32, mu 96: hits 0.9163; |lambda* - depth| max 25.48
@pytest.mark.parametrize("n, voxel, mu, min_hits", [(64, 16.0, 48.0, 0.95), (32, 32.0, 96.0, 0.9)])
def test_rule_reconstructs_the_analytic_corner(n, voxel, mu, min_hits):
    cam = T.corner_camera()
    vol, _ = T.fuse_corner(T.corner_volume(n, voxel, mu), cam)
    f = T.corner_figures(vol, cam, T.look_at(T.EYE_CAST))
    print("hits %.4f  err max %.2f median %.2f p99 %.2f  normals %.4f  angles max %.2f median %.2f" %
          (f["hits"], f["err"].max(), np.median(f["err"]), np.percentile(f["err"], 99), f["normals"], f["angles"].max(), np.median(f["angles"])))
    assert f["hits"] >= min_hits                    # 0.9806 / 0.9163
    assert f["err"].max() < voxel                   # 11.22 of 16 / 25.48 of 32
    if n == 64:
        assert f["normals"] >= 0.9                  # 0.9533
        assert f["angles"].size > 1000 and f["angles"].max() <= 15.0      # 10.08 degrees
