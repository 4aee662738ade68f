"""CPU tests of the surface extraction: the rule itself (tsdf_surface_ref.py) against the analytic room corner, so that an engine that
equals the restatement bit for bit cannot be bit-exactly wrong; the options' struct as C; the PLY files of icp_amd.io."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tsdf_ref as T
import tsdf_surface_ref as S
from icp_checks import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_header_struct_is_plain_c_and_pythons():
    from icp_amd import tsdf
    code = ('#include "icp_amd.h"\n'
            "int main(void){ icp_tsdf_surface_t o; o.min_weight = 1.f; o.normals = 1u; (void) o;\n"
            "return (int) sizeof (icp_tsdf_surface_t) - 8; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-c", "-o", "/dev/null"],
                       input=code.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert [n for n, _ in tsdf.icp_tsdf_surface_t._fields_] == ["min_weight", "normals"] and C.sizeof(tsdf.icp_tsdf_surface_t) == 8


# (points, on x / y / z) as the restatement gives them: regression values
COUNTS = {1.0: (7106, (2422, 2462, 2222)), 2.0: (6912, (2366, 2404, 2142))}


@pytest.mark.parametrize("min_weight", [1.0, 2.0])
def test_the_rule_against_the_analytic_corner(min_weight):
    """The room corner fused from six eyes into 64^3 voxels of 16: every point within half a voxel edge of its quarter-plane, nine in ten
    with a normal, the normals away from the creases within 20 degrees of the plane's and pointing into the room.  Measured: min_weight 1
    7106 points, farthest 4.24, 0.947 with a normal, 13.04 degrees; min_weight 2 6912 points, 3.54, 0.967, 13.04 degrees."""
    cam = T.corner_camera()
    vol, _ = T.fuse_corner(T.corner_volume(), cam)
    info = {}
    cloud, nrm = S.extract(vol, min_weight, info)
    f = S.corner_surface_figures(cloud, nrm)
    per_axis = tuple(int(x) for x in np.bincount(info["axis"], minlength=3))
    print("min_weight %g: %d points (%d / %d / %d on x / y / z), farthest from its quarter-plane %.2f, share with a normal %.3f, "
          "largest angle on %d points away from the creases %.2f degrees"
          % ((min_weight, f["count"]) + per_axis + (f["dist"].max(), f["normals"], f["angles"].size, f["angles"].max())))
    assert f["dist"].max() < 8.0
    assert f["normals"] >= 0.9
    assert f["angles"].size > 1000 and f["angles"].max() < 20.0
    assert (f["count"], per_axis) == COUNTS[min_weight]
    # the form of a record, the order, and t
    assert (cloud[:, 3] == 1).all() and (cloud[:, 7] == 1).all() and (cloud[:, 4:7] == 0).all() and (nrm[:, 3] == 0).all()
    nx, ny = vol.cfg["nx"], vol.cfg["ny"]
    key = 3 * ((info["index"][:, 2] * ny + info["index"][:, 1]) * nx + info["index"][:, 0]) + info["axis"]
    assert (np.diff(key) > 0).all()
    assert (info["t"] >= 0).all() and (info["t"] <= 1).all()
    unit = np.linalg.norm(nrm[:, :3].astype(np.float64), axis=1)[np.any(nrm[:, :3] != 0, axis=1)]
    assert np.abs(unit - 1).max() < 1e-6


def test_a_higher_min_weight_keeps_a_subset_and_mu_of_half_a_voxel_edge_yields_nothing():
    cam = T.corner_camera()
    vol, _ = T.fuse_corner(T.corner_volume(), cam)
    one, two = S.members(vol.dw, 1.0), S.members(vol.dw, 2.0)
    assert all((b <= a).all() for a, b in zip(one, two)) and sum(int(a.sum()) for a in one) > sum(int(b.sum()) for b in two)
    # a plane seen along z, as one frame from below fuses it: D = clip ((z0 - k) / mu).  mu = half the voxel edge: neighbours differ by 2
    for z0 in (6.0, 6.3, 6.5, 6.9):
        thin, wide = T.Volume(T.volume_config(6, 5, 12, 1.0, (0.0, 0.0, 0.0), 0.5)), T.Volume(T.volume_config(6, 5, 12, 1.0, (0.0, 0.0, 0.0), 1.0))
        for v in (thin, wide):
            v.dw[..., 0] = np.clip((F32(z0) - np.arange(12, dtype=F32)[:, None, None]) / F32(v.cfg["mu"]), -1, 1)
            v.dw[..., 1] = 1
        assert S.extract(thin)[0].shape == (0, 8) and S.extract(thin)[1].shape == (0, 4)
        assert S.extract(wide)[0].shape == ((30, 8) if z0 != 6.0 else (0, 8))      # (z0 = 6: D = 1, 0, -1 — a zero between truncated values)


def test_a_zero_between_positive_neighbours_gives_two_coincident_points():
    vol = T.Volume(T.volume_config(3, 2, 2, 2.0, (1.0, 2.0, 3.0), 4.0))
    vol.dw[..., 0], vol.dw[..., 1] = 0.5, 1
    vol.dw[0, 0, 1, 0] = 0.0
    info = {}
    cloud, _ = S.extract(vol, info=info)
    on_x = info["axis"] == 0
    assert on_x.sum() == 2 and list(info["t"][on_x]) == [1.0, 0.0] and np.signbit(info["t"][on_x][1])
    assert_bits(cloud[on_x][0], cloud[on_x][1], "the two points")
    assert list(cloud[on_x][0][:3]) == [3.0, 2.0, 3.0]


def test_ply_round_trip(tmp_path):
    from icp_amd import io
    rng = np.random.default_rng(5)
    n = 1000
    cloud = np.zeros((n, 8), F32)
    cloud[:, :3] = rng.normal(0, 500, (n, 3))
    cloud[:, 3] = cloud[:, 7] = 1
    cloud[:, 4:7] = rng.random((n, 3))
    cloud[0, 4:7] = (-0.2, 1.3, 0.5)                                        # clipped; 127.5 rounds to even
    nrm = np.zeros((n, 4), F32)
    nrm[:, :3] = rng.normal(0, 1, (n, 3))
    want_bytes = np.clip(np.rint(cloud[:, 4:7] * F32(255)), 0, 255).astype(np.uint8)
    assert list(want_bytes[0]) == [0, 255, 128]
    for with_normals in (True, False):
        path = str(tmp_path / ("n%d.ply" % with_normals))
        io.save_ply(path, cloud, nrm if with_normals else None)
        raw = open(path, "rb").read()
        head, _, body = raw.partition(b"end_header\n")
        lines = head.decode("ascii").split("\n")
        assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and "element vertex %d" % n in lines
        props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
        assert props == [["float", a] for a in ("x", "y", "z") + (("nx", "ny", "nz") if with_normals else ())] + [["uchar", a] for a in ("red", "green", "blue")]
        assert len(body) == n * (27 if with_normals else 15)
        got, gotn = io.load_ply(path)
        assert_bits(got[:, :4], cloud[:, :4], "points")
        assert_bits(got[:, 7], cloud[:, 7], "the last lane")
        assert np.array_equal(np.rint(got[:, 4:7] * F32(255)).astype(np.uint8), want_bytes)
        assert_bits(got[:, 4:7], want_bytes.astype(F32) / F32(255), "colours")
        if with_normals:
            assert_bits(gotn, nrm, "normals")
        else:
            assert gotn is None
    with pytest.raises(ValueError):
        io.save_ply(str(tmp_path / "bad.ply"), cloud, nrm[:5])
    open(str(tmp_path / "not.ply"), "wb").write(b"plx\n")
    with pytest.raises(ValueError):
        io.load_ply(str(tmp_path / "not.ply"))
    io.save_ply(str(tmp_path / "empty.ply"), np.zeros((0, 8), F32))
    got, gotn = io.load_ply(str(tmp_path / "empty.ply"))
    assert got.shape == (0, 8) and gotn is None
