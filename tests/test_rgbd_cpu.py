"""CPU tests of the RGB-D front end: the numpy restatement (rgbd_ref.py) against the rule written out by hand and against exact
rationals, the filter's invariants, the bound behind the exact conversion, the header's struct as C, the kernels' resources, and
the command line over a stand-in library."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rgbd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_unfiltered_rule_is_the_writers_formula():
    """r = 0 on hand-made pixels: X = (u - cx) z / fx, Y = (v - cy) z / fy, Z = z = count * scale, colour / 255, the two 1 lanes; an
    invalid count gives xyz = +-0 with its colour kept."""
    cfg = R.config(width=4, height=3, fx=500.0, fy=510.0, cx=1.5, cy=0.75, depth_scale=0.5, d_min=10, d_max=3000, radius=0)
    depth = np.array([[100, 0, 9, 10], [3000, 3001, 777, 65535], [1234, 2, 2999, 11]], np.uint16)
    rgb = (np.arange(36, dtype=np.uint8) * 7).reshape(3, 4, 3)
    got = R.cloud(depth, rgb, cfg).reshape(3, 4, 8)
    for v in range(3):
        for u in range(4):
            c = int(depth[v, u])
            z = F32(c) * F32(0.5) if (c != 0 and 10 <= c <= 3000) else F32(0)
            x = F32(F32(F32(u) - F32(1.5)) * z) / F32(500.0)
            y = F32(F32(F32(v) - F32(0.75)) * z) / F32(510.0)
            want = np.array([x, y, z, 1, F32(rgb[v, u, 0]) / F32(255), F32(rgb[v, u, 1]) / F32(255), F32(rgb[v, u, 2]) / F32(255), 1], F32)
            assert np.array_equal(got[v, u].view(np.uint32), want.view(np.uint32)), (u, v)
    assert np.all(got[0, 1, :3] == 0) and np.signbit(got[0, 1, 0]) and got[0, 1, 4] == F32(21) / F32(255)     # a hole left of cx: x = -0
    assert np.array_equal(R.cloud(depth, None, cfg)[:, 4:7], np.zeros((12, 3), F32))


def _exact(depth, cfg, u, v):
    """z of one pixel from exact rationals, rounded once to float32, then times the scale."""
    H, W, r, S = cfg["height"], cfg["width"], cfg["radius"], cfg["range"]
    ok = lambda c: c != 0 and cfg["d_min"] <= c <= cfg["d_max"]
    c0 = int(depth[v, u])
    if not ok(c0):
        return F32(0)
    N = D = 0
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            x, y = u + dx, v + dy
            if 0 <= x < W and 0 <= y < H and ok(int(depth[y, x])):
                cq = int(depth[y, x])
                w = max(0, (r + 1) ** 2 - dx * dx - dy * dy) * max(0, S * S - (cq - c0) ** 2)
                N += w * cq
                D += w
    return F32(float(Fraction(N, D))) * F32(cfg["depth_scale"])        # (Fraction -> float is correctly rounded: the rule's one division)


def test_filter_equals_exact_rationals():
    """A handful of pixels: an edge, a hole beside the centre, the window clipped at an image corner."""
    rng = np.random.default_rng(5)
    H, W = 9, 11
    depth = (1000 + rng.integers(-12, 13, (H, W))).astype(np.uint16)
    depth[:, 6:] += 40                                                 # an edge of 40 counts between columns 5 and 6
    depth[4, 4] = 0                                                    # a hole beside (5, 4) and (3, 4)
    for r, S in ((1, 30), (2, 30), (3, 50), (6, 4095)):
        cfg = R.config(width=W, height=H, radius=r, range=S, depth_scale=0.001)
        z = R.depth_map(depth, cfg)
        for (u, v) in ((5, 4), (6, 4), (3, 4), (4, 4), (0, 0), (W - 1, H - 1), (0, H - 1), (5, 0)):
            assert z[v, u].view(np.uint32) == _exact(depth, cfg, u, v).view(np.uint32), (r, S, u, v)
        assert z[4, 4] == 0                                            # holes are not filled


def test_constant_plane_is_untouched():
    for c in (1, 777, 65535):
        depth = np.full((13, 15), c, np.uint16)
        for r in range(0, 7):
            for S in (1, 30, 4095):
                z = R.depth_map(depth, R.config(width=15, height=13, radius=r, range=S, depth_scale=0.25))
                assert np.array_equal(z, np.full((13, 15), F32(c) * F32(0.25), F32)), (c, r, S)


def test_a_step_of_S_counts_is_left_alone_and_one_less_is_not():
    S = 30
    for r in (1, 3, 6):
        for step, same in ((S, True), (S - 1, False)):
            depth = np.full((16, 16), 1000, np.uint16)
            depth[:, 8:] += step
            z = R.depth_map(depth, R.config(width=16, height=16, radius=r, range=S))
            assert np.array_equal(z, depth.astype(F32)) == same, (r, step)
            if not same:
                assert np.array_equal(z[:, :8 - r], depth[:, :8 - r].astype(F32))       # (away from the step nothing moves)


def test_the_numerator_stays_below_2_to_the_53():
    r, S = 6, 4095
    ws = sum(max(0, (r + 1) ** 2 - dx * dx - dy * dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1))
    assert ws == 3765
    assert ws * S * S * 65535 < 2 ** 53
    # the restatement reaches the bound's case: a window full of 65535 (w_r = S^2 everywhere)
    depth = np.full((13, 13), 65535, np.uint16)
    N, D = R.sums(depth, R.config(width=13, height=13, radius=r, range=S))
    assert int(N[6, 6]) == ws * S * S * 65535 and int(D[6, 6]) == ws * S * S


def test_header_compiles_as_c_with_the_configuration():
    code = ('#include "icp_amd.h"\n'
            "int (*set) (icp_handle, const icp_rgbd_t *) = icp_set_rgbd; int (*get) (icp_handle, icp_rgbd_t *) = icp_get_rgbd;\n"
            "int (*wr) (icp_handle, int, const uint16_t *, const uint8_t *, int, int) = icp_write_rgbd;\n"
            "int (*kn) (int, const icp_rgbd_t *, const uint16_t *, const uint8_t *, void *, float *) = icp_kernel_rgbd;\n"
            "int (*ts) (icp_handle, const uint16_t *, const uint8_t *, int) = icp_track_submit_rgbd;\n"
            "int (*tn) (icp_handle, const uint16_t *, const uint8_t *, int, uint32_t *, int *) = icp_track_next_rgbd;\n"
            "int main(void){ icp_rgbd_t c; c.width = 640u; c.range = 30u; c.fx = 595.f; (void) c; return (int) sizeof (icp_rgbd_t) - 60; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-c", "-o", "/dev/null"],
                       input=code.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_python_struct_is_the_headers():
    from icp_amd import rgbd
    hdr = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    body = hdr[hdr.index("typedef struct {\n    uint32_t width, height;"):hdr.index("} icp_rgbd_t;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"(?:uint32_t|float)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in rgbd.icp_rgbd_t._fields_] and C.sizeof(rgbd.icp_rgbd_t) == 60
    assert rgbd.RGBDConfig.kinect() == rgbd.RGBDConfig() and rgbd.RGBDConfig().as_dict() == R.DEFAULTS
    assert rgbd.RGBDConfig(radius=3) != rgbd.RGBDConfig()


def test_rgbd_kernels_compile_for_gfx950_without_scratch():
    from kernel_resources import kernel_resources
    res = kernel_resources("icp_amd/csrc/icp_rgbd.hip")
    assert sorted(res) == ["k_rgbd_dense", "k_rgbd_lattice"], sorted(res)
    for n, r in res.items():
        assert r["scratch"] == 0 and r.get("dynamic_stack") in (None, "False"), (n, r)
    assert res["k_rgbd_dense"]["lds"] <= 4096


class _StandIn:
    """A library whose icp_kernel_rgbd is the restatement (the command line's path from files to file needs no device)."""

    def __init__(self):
        self.calls = []

    def icp_kernel_rgbd(self, device, cfg, depth, rgb, cloud, nrm):
        c = cfg._obj
        d = {n: getattr(c, n) for n, _ in type(c)._fields_}
        n = c.width * c.height
        dep = np.ctypeslib.as_array(C.cast(depth, C.POINTER(C.c_uint16)), shape=(n,))
        col = None if not rgb else np.ctypeslib.as_array(C.cast(rgb, C.POINTER(C.c_uint8)), shape=(n * 3,))
        out = np.ctypeslib.as_array(C.cast(cloud, C.POINTER(C.c_float)), shape=(n, 8))
        out[:] = R.cloud(dep, col, d)
        self.calls.append(d)
        return 0


def test_command_line_round_trip(tmp_path, monkeypatch):
    from icp_amd import io, rgbd
    rng = np.random.default_rng(11)
    depth = rng.integers(0, 5000, (480, 640)).astype(np.uint16)
    rgb = rng.integers(0, 256, (480, 640, 3)).astype(np.uint8)
    depth.astype("<u2").tofile(tmp_path / "d.raw")
    rgb.tofile(tmp_path / "c.raw")
    lib = _StandIn()
    monkeypatch.setattr(rgbd, "_lib", lambda: lib)
    assert rgbd.main([str(tmp_path / "d.raw"), str(tmp_path / "c.raw"), str(tmp_path / "o.bin"), "--radius", "2", "--range", "40", "--fx", "580"]) == 0
    assert lib.calls[0]["radius"] == 2 and lib.calls[0]["range"] == 40 and lib.calls[0]["fx"] == 580.0 and lib.calls[0]["fy"] == 595.0
    got = io.load_pc8d(str(tmp_path / "o.bin"))
    want = R.cloud(depth, rgb, R.config(radius=2, range=40, fx=580.0))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a wrong size is refused before anything is written
    depth[:100].astype("<u2").tofile(tmp_path / "short.raw")
    assert rgbd.main([str(tmp_path / "short.raw"), "-", str(tmp_path / "no.bin")]) == 1 and not os.path.exists(tmp_path / "no.bin")


def test_images_are_checked_as_write_cloud_checks_its_cloud():
    from icp_amd import rgbd
    with pytest.raises(ValueError):
        rgbd._images(np.zeros((480, 640), np.float32), None, 640, 480)
    with pytest.raises(ValueError):
        rgbd._images(np.zeros((480, 639), np.uint16), None, 640, 480)
    with pytest.raises(ValueError):
        rgbd._images(np.zeros((480, 640), np.uint16), np.zeros((480, 640), np.uint8), 640, 480)
    d, c = rgbd._images(np.zeros((480, 640), np.uint16), np.zeros((480, 640, 3), np.uint8), 640, 480)
    assert d.flags.c_contiguous and c.flags.c_contiguous
