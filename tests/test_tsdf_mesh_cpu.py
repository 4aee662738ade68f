"""CPU tests of the mesh extraction: the case table of the library against the restatement's own generator (tsdf_mesh_ref.py) and against
what a closed triangulation of a cube must be; the rule on a random volume, a sphere, a torus and the fused room corner, so that an engine
that equals the restatement cannot be exactly wrong; the header as C; the PLY files with faces."""
import collections
import os
import struct
import subprocess

import numpy as np
import pytest

import tsdf_mesh_ref as M
import tsdf_ref as T
import tsdf_surface_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EINVAL = 1


# ---- the table ----------------------------------------------------------------------------------------------------------------------------

def test_the_library_table_is_the_generated_one():
    import ctypes as C
    from icp_amd import tsdf
    table, _ = M.case_table()
    for case in range(256):
        assert tuple(tsdf.mesh_case(case)) == table[case], case
    n, edges = C.c_uint32(77), (C.c_uint8 * 15)(*([9] * 15))
    for bad in (256, 257, 0xFFFFFFFF):
        assert tsdf._lib().icp_tsdf_mesh_case(bad, C.byref(n), edges) == EINVAL
        assert n.value == 77 and list(edges) == [9] * 15
    assert tsdf._lib().icp_tsdf_mesh_case(255, C.byref(n), edges) == 0 and n.value == 0 and list(edges) == [0] * 15
    with pytest.raises(tsdf.icp_amd.ICPError):
        tsdf.mesh_case(256)


def test_the_table_regression_figures():
    table, moved = M.case_table()
    per_case = [len(t) for t in table]
    assert max(per_case) == 5 and sum(per_case) == 820 and moved == 18
    assert dict(collections.Counter(per_case)) == {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32}
    assert per_case[0] == per_case[255] == 0


@pytest.mark.parametrize("case", range(256))
def test_a_case_is_a_closed_triangulation_of_its_loops(case):
    tris = M.case_table()[0][case]
    crossing = M.crossing_edges(case)
    assert sorted({e for t in tris for e in t}) == crossing                     # every crossing edge is used, and nothing else
    directed = [(t[q], t[(q + 1) % 3]) for t in tris for q in range(3)]
    assert len(set(directed)) == len(directed)                                   # every directed segment at most once
    used = collections.Counter(frozenset(d) for d in directed)
    face = {frozenset(s) for s in M.face_segments(case)}
    assert len(face) == len(M.face_segments(case))
    assert {s for s, n in used.items() if n == 1} == face                        # the open segments are exactly the faces' (rule 2)
    for s, n in used.items():
        if s not in face:
            a, b = tuple(s)
            assert n == 2 and (a, b) in directed and (b, a) in directed          # an interior diagonal: twice, in opposite directions
            assert not M.share_a_face(a, b)                                      # and in no cube face


# ---- volumes ------------------------------------------------------------------------------------------------------------------------------

def _volume(dims, D):
    nx, ny, nz = dims
    vol = T.Volume(T.volume_config(nx, ny, nz, 1.0, (0.0, 0.0, 0.0), 4.0))
    vol.dw[..., 0], vol.dw[..., 1] = D, 1
    return vol


def _grid(dims):
    nx, ny, nz = dims
    return np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")


def test_a_random_volume_is_closed_up_to_its_boundary():
    dims = (13, 12, 11)
    vol = _volume(dims, np.random.default_rng(13).uniform(-0.9, 0.9, dims[::-1]).astype(F32))
    info = {}
    cloud, _, tri = M.extract(vol, 1.0, info)
    assert info["active"].all() and np.unique(info["cases"]).size == 256         # all 256 cases occur
    once, lone, _ = M.edge_figures(tri)
    assert once                                                                  # every directed edge is used once
    assert np.unique(tri).size == cloud.shape[0] and tri.max() == cloud.shape[0] - 1        # every member is referenced
    p = cloud[:, :3]
    a, b = p[lone[:, 0]], p[lone[:, 1]]
    on_one_face = np.zeros(lone.shape[0], bool)
    for ax in range(3):
        for side in (0.0, float(dims[ax] - 1)):
            on_one_face |= (a[:, ax] == side) & (b[:, ax] == side)
    assert lone.shape[0] > 100 and on_one_face.all()                             # an unpaired edge lies on a boundary face of the volume


CENTRE = np.array([11.3, 11.6, 11.45])


def _solid(name):
    """(sdf (nz, ny, nx) float64, outward direction at points (n, 3), Euler characteristic, analytic area)."""
    k, j, i = _grid((24, 24, 24))
    x, y, z = i - CENTRE[0], j - CENTRE[1], k - CENTRE[2]
    if name == "sphere":
        r = 7.4
        return np.sqrt(x * x + y * y + z * z) - r, lambda p: p - CENTRE, 2, 4 * np.pi * r * r
    R, r = 7.2, 2.6

    def outward(p):
        q = p - CENTRE
        rho = np.linalg.norm(q[:, :2], axis=1, keepdims=True)
        return q - np.concatenate([q[:, :2] / rho * R, np.zeros((q.shape[0], 1))], 1)
    return np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r, outward, 0, 4 * np.pi ** 2 * R * r


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_a_closed_surface(name):
    """24^3 voxels of 1, D = clip (sdf / 4, -1, 1), W = 1: a sphere of radius 7.4 and a torus of radii 7.2 / 2.6.  No unpaired edge,
    V - E + F = 2 and 0, every triangle's normal points outward, and the area is that of a chord mesh: just short of the analytic one.
    Measured: the sphere 0.9943 of 4 pi r^2 (1018 vertices, 2032 triangles), the torus 0.9913 of 4 pi^2 R r (1158 vertices, 2316 triangles)."""
    sdf, outward, euler, analytic = _solid(name)
    vol = _volume((24, 24, 24), np.clip(sdf / 4.0, -1, 1).astype(F32))
    cloud, _, tri = M.extract(vol)
    once, lone, n_edges = M.edge_figures(tri)
    assert once and lone.shape[0] == 0
    assert np.unique(tri).size == cloud.shape[0]
    assert cloud.shape[0] - n_edges + tri.shape[0] == euler
    area, normal = M.areas_and_normals(cloud, tri)
    p = cloud[:, :3].astype(np.float64)
    centroid = (p[tri[:, 0]] + p[tri[:, 1]] + p[tri[:, 2]]) / 3
    solid = area > 0
    assert solid.sum() > 0.99 * tri.shape[0] and (np.sum(normal * outward(centroid), axis=1)[solid] > 0).all()
    print("%s: %d vertices, %d triangles, area %.4f of the analytic" % (name, cloud.shape[0], tri.shape[0], area.sum() / analytic))
    assert 0.98 <= area.sum() / analytic <= 1.0


# (vertices, triangles) of the fused corner as the restatement gives them: regression values
CORNER_COUNTS = {1.0: (7106, 13769), 2.0: (6912, 13409)}


@pytest.mark.parametrize("min_weight", [1.0, 2.0])
def test_the_rule_against_the_analytic_corner(min_weight):
    """The room corner of test_tsdf_surface_cpu.py (six eyes, 64^3 voxels of 16): every triangle's vertices within 8.0 of the quarter-planes;
    of the triangles whose three vertices have normals and lie more than 100 from a crease, the share whose geometric normal has a positive
    dot product with each of the three vertex normals.  Measured on the restatement, which is deterministic: min_weight 1 all of 8149 such triangles, min_weight 2 all of 8062; so all is asserted."""
    cam = T.corner_camera()
    vol, _ = T.fuse_corner(T.corner_volume(), cam)
    cloud, nrm, tri = M.extract(vol, min_weight)
    f = S.corner_surface_figures(cloud, nrm)
    assert f["dist"].max() < 8.0 and tri.max() < cloud.shape[0]                 # (every vertex, so every triangle's)
    assert M.edge_figures(tri)[0]
    has_n = np.any(nrm[:, :3] != 0, axis=1)
    far = np.sort(np.abs(cloud[:, :3].astype(np.float64)), 1)[:, 1] > 100.0
    t = tri[(has_n & far)[tri].all(1)]
    _, normal = M.areas_and_normals(cloud, t)
    agree = np.all([np.sum(normal * nrm[t[:, q], :3], axis=1) > 0 for q in range(3)], axis=0)
    print("min_weight %g: %d vertices, %d triangles, %d far from a crease with normals, of which %.4f agree with their vertex normals"
          % (min_weight, cloud.shape[0], tri.shape[0], t.shape[0], agree.mean()))
    assert (cloud.shape[0], tri.shape[0]) == CORNER_COUNTS[min_weight]
    assert t.shape[0] > 5000 and agree.all()


# ---- plain checks -------------------------------------------------------------------------------------------------------------------------

def test_header_is_plain_c():
    code = ('#include "icp_amd.h"\n'
            "int main(void){ uint32_t n = 0, m = 0; uint8_t e[15]; icp_tsdf_surface_t o; o.min_weight = 1.f; o.normals = 0u;\n"
            "if (icp_tsdf_mesh_case (3u, &n, e) != ICP_OK) return 1;\n"
            "return icp_tsdf_extract_mesh ((icp_tsdf_handle) 0, &o, 0u, (void *) 0, (float *) 0, &n, 0u, (uint32_t *) 0, &m); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-c", "-o", "/dev/null"],
                       input=code.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def _small_mesh():
    rng = np.random.default_rng(5)
    cloud = np.ones((6, 8), F32)
    cloud[:, :3] = rng.uniform(-100, 100, (6, 3))
    cloud[:, 4:7] = rng.integers(0, 256, (6, 3)) / F32(255)
    nrm = np.zeros((6, 4), F32)
    nrm[:, :3] = rng.uniform(-1, 1, (6, 3))
    return cloud, nrm, np.array([[0, 1, 2], [2, 1, 3], [5, 4, 0]], np.uint32)


def test_ply_with_faces_round_trips(tmp_path):
    from icp_amd import io
    cloud, nrm, faces = _small_mesh()
    for normals in (nrm, None):
        path = str(tmp_path / "mesh.ply")
        io.save_ply(path, cloud, normals, faces)
        c, n, f = io.load_ply_mesh(path)
        assert np.array_equal(c, cloud) and f.dtype == np.uint32 and np.array_equal(f, faces)
        assert n is None if normals is None else np.array_equal(n, nrm)
        with pytest.raises(ValueError):
            io.load_ply(path)                                                    # load_ply keeps refusing a face element
        head = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
        assert head[-3:-1] == ["element face 3", "property list uchar int vertex_indices"]
    io.save_ply(str(tmp_path / "none.ply"), cloud, nrm, np.zeros((0, 3), np.uint32))
    assert io.load_ply_mesh(str(tmp_path / "none.ply"))[2].shape == (0, 3)
    io.save_ply(str(tmp_path / "cloud.ply"), cloud, nrm)
    c, n, f = io.load_ply_mesh(str(tmp_path / "cloud.ply"))
    assert f is None and np.array_equal(c, cloud) and np.array_equal(n, nrm)
    with pytest.raises(ValueError):
        io.save_ply(str(tmp_path / "bad.ply"), cloud, nrm, np.array([[0, 1, 6]]))


def test_ply_without_faces_is_the_file_it_was(tmp_path):
    """The bytes written out by hand from the format save_ply documents: the header, then per point x y z (nx ny nz) as float and the colour as bytes."""
    from icp_amd import io
    cloud, nrm, faces = _small_mesh()
    for normals in (nrm, None):
        names = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals is not None else [])
        head = ["ply", "format binary_little_endian 1.0", "comment icp_amd", "element vertex 6"] + ["property float " + n for n in names]
        head += ["property uchar red", "property uchar green", "property uchar blue", "end_header"]
        want = ("\n".join(head) + "\n").encode("ascii")
        for p in range(6):
            want += struct.pack("<3f", *cloud[p, :3])
            if normals is not None:
                want += struct.pack("<3f", *normals[p, :3])
            want += struct.pack("<3B", *[int(np.rint(c * 255)) for c in cloud[p, 4:7].astype(np.float64)])
        path = str(tmp_path / "cloud.ply")
        io.save_ply(path, cloud, normals)
        assert open(path, "rb").read() == want
        io.save_ply(path, cloud, normals, faces)                                 # and the faces follow those bytes
        got = open(path, "rb").read()
        body = want.split(b"end_header\n")[1]
        assert got.endswith(body + b"".join(struct.pack("<B3i", 3, *t) for t in faces.tolist()))
