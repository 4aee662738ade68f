"""The mesh extraction of the TSDF volume restated in numpy (the rule of include/icp_amd.h: icp_tsdf_extract_mesh): the case table generated
by its rule, the triangles of a tsdf_ref.Volume in the rule's order, and what the tests ask of a mesh's topology.  The vertices are
tsdf_surface_ref.extract's members.  A plain module: it collects no tests."""
import functools

import numpy as np

import tsdf_surface_ref as S

F32 = np.float32


# ---- the cube ---------------------------------------------------------------------------------------------------------------------------

def edge_ends(e):
    """The two corners (c = bx + 2 by + 4 bz) of local edge e = 4 a + m: the low end, the high end."""
    a, m = divmod(e, 4)
    b1, b2 = [b for b in range(3) if b != a]
    c0 = ((m & 1) << b1) | ((m >> 1) << b2)
    return c0, c0 | (1 << a)


def edge_faces(e):
    """The two cube faces 2 f + side (f: the axis the face is across) that local edge e lies on."""
    a, m = divmod(e, 4)
    b1, b2 = [b for b in range(3) if b != a]
    return 2 * b1 + (m & 1), 2 * b2 + (m >> 1)


def share_a_face(e, f):
    return bool(set(edge_faces(e)) & set(edge_faces(f)))


def _midpoint(e):
    c0, _ = edge_ends(e)
    p = np.array([(c0 >> b) & 1 for b in range(3)], float)
    p[e // 4] = 0.5
    return p


def crossing_edges(case):
    return [e for e in range(12) if ((case >> edge_ends(e)[0]) ^ (case >> edge_ends(e)[1])) & 1]


def face_segments(case):
    """Rule 2: the segments (pairs of local edge ids) that the six faces draw."""
    segs = []
    for face in range(6):
        on = [e for e in crossing_edges(case) if face in edge_faces(e)]
        assert len(on) in (0, 2, 4)
        if len(on) == 2:
            segs.append((on[0], on[1]))
        elif len(on) == 4:
            f, side = divmod(face, 2)
            for c in range(8):
                if ((c >> f) & 1) == side and (case >> c) & 1:             # a positive corner of the face is cut off singly
                    pair = [e for e in on if c in edge_ends(e)]
                    assert len(pair) == 2
                    segs.append((pair[0], pair[1]))
    return segs


def case_loops(case):
    """Rules 3 to 5: [(loop in its direction from its smallest edge id, apex position s)] in ascending order of the smallest edge id."""
    nb = {}
    for x, y in face_segments(case):
        nb.setdefault(x, []).append(y)
        nb.setdefault(y, []).append(x)
    assert all(len(v) == 2 and v[0] != v[1] for v in nb.values())
    left, loops = set(nb), []
    while left:
        e0 = min(left)
        r, prev = [e0], None
        while True:
            nxt = [x for x in nb[r[-1]] if x != prev][0] if prev is not None else nb[r[-1]][0]
            if nxt == e0:
                break
            prev = r[-1]
            r.append(nxt)
        left -= set(r)
        P = [_midpoint(e) for e in r]
        area = sum(np.cross(P[i], P[(i + 1) % len(r)]) for i in range(len(r)))
        up = np.zeros(3)
        for e in r:
            up[e // 4] += -1.0 if (case >> edge_ends(e)[0]) & 1 else 1.0   # from the non-positive end to the positive end
        d = float(area @ up)
        assert d != 0.0
        if d < 0:
            r = [r[0]] + r[:0:-1]
        n = len(r)
        apex = [s for s in range(n) if not any(share_a_face(r[s], r[(s + i) % n]) for i in range(2, n - 1))]
        assert apex, (case, r)
        loops.append((r, apex[0]))
    return loops


@functools.lru_cache(maxsize=None)
def case_table():
    """((triangles of case 0), .., (of case 255)): each a tuple of triples of local edge ids, and the number of loops whose apex moved."""
    table, moved = [], 0
    for case in range(256):
        tris = []
        for r, s in case_loops(case):
            n = len(r)
            moved += s != 0
            tris += [(r[s], r[(s + i) % n], r[(s + i + 1) % n]) for i in range(1, n - 1)]
        table.append(tuple(tris))
    return tuple(table), moved


# ---- the mesh of a volume -----------------------------------------------------------------------------------------------------------------

def cell_cases(dw, min_weight=1.0):
    """(active (nz - 1, ny - 1, nx - 1) bool, case uint8 of the same shape)."""
    ok = S.usable(dw, min_weight)
    with np.errstate(invalid="ignore"):
        pos = dw[..., 0] > 0
    nz, ny, nx = ok.shape
    active = np.ones((nz - 1, ny - 1, nx - 1), bool)
    case = np.zeros(active.shape, np.uint8)
    for c in range(8):
        bx, by, bz = c & 1, (c >> 1) & 1, c >> 2
        sl = (slice(bz, nz - 1 + bz), slice(by, ny - 1 + by), slice(bx, nx - 1 + bx))
        active &= ok[sl]
        case |= pos[sl].astype(np.uint8) << c
    return active, case


def member_positions(dw, min_weight=1.0):
    """(3, nz, ny, nx) int64: the position of member (v, a) in the rule's order, -1 where the edge is no member; and the member count."""
    mem = np.stack(S.members(dw, min_weight))                          # [a][k][j][i]
    flat = np.moveaxis(mem, 0, -1).reshape(-1)                         # index 3 * lin + a
    pos = np.where(flat, np.cumsum(flat) - 1, -1)
    return np.moveaxis(pos.reshape(mem.shape[1:] + (3,)), -1, 0), int(flat.sum())


def triangles(dw, min_weight=1.0, info=None):
    """(m, 3) uint32 vertex indices in the rule's order: ascending cell index, inside a cell in table order.  info: a dict that receives
    `cell` (m,) the linear index of each triangle's cell, `case` the case of every active cell with triangles."""
    table, _ = case_table()
    active, case = cell_cases(dw, min_weight)
    pos, _ = member_positions(dw, min_weight)
    nz, ny, nx = dw.shape[:3]
    count = np.array([len(t) for t in table])
    ids = np.zeros((256, 5, 3), np.int64)
    for c, tris in enumerate(table):
        ids[c, :len(tris)] = np.array(tris, np.int64).reshape(-1, 3)
    low = np.array([edge_ends(x)[0] for x in range(12)])
    k, j, i = np.nonzero(active & (count[case] > 0))
    cs = case[k, j, i]
    out, cells = [], []
    for t in range(5):
        sel = count[cs] > t
        tri = np.empty((int(sel.sum()), 3), np.int64)
        edges = ids[cs[sel], t]
        for q in range(3):
            e = edges[:, q]
            c0 = low[e]
            tri[:, q] = pos[e // 4, k[sel] + (c0 >> 2), j[sel] + ((c0 >> 1) & 1), i[sel] + (c0 & 1)]
        assert (tri >= 0).all()
        out.append(tri)
        cells.append(np.stack([(k[sel] * ny + j[sel]) * nx + i[sel], np.full(tri.shape[0], t)], 1))
    tri, cells = np.concatenate(out), np.concatenate(cells)
    order = np.lexsort((cells[:, 1], cells[:, 0]))
    if info is not None:
        info.update(cell=cells[order, 0], case=cs, active=active, cases=case)
    return tri[order].astype(np.uint32)


def extract(vol, min_weight=1.0, info=None):
    """(cloud (n, 8), normals (n, 4), triangles (m, 3) uint32) of a tsdf_ref.Volume."""
    cloud, nrm = S.extract(vol, min_weight)
    return cloud, nrm, triangles(vol.dw, min_weight, info)


# ---- what a mesh's topology is asked -------------------------------------------------------------------------------------------------------

def directed_edges(tri):
    """(3 m, 2) int64: every triangle's three directed edges."""
    t = tri.astype(np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_figures(tri):
    """(every directed edge occurs once, the (u, 2) directed edges without an opposite partner, the number of undirected edges)."""
    d = directed_edges(tri)
    big = int(d.max()) + 1 if d.size else 1
    key, back = d[:, 0] * big + d[:, 1], d[:, 1] * big + d[:, 0]
    once = np.unique(key).size == key.size
    lone = d[~np.isin(key, back)]
    return once, lone, np.unique(np.minimum(key, back)).size


def areas_and_normals(cloud, tri):
    p = cloud[:, :3].astype(np.float64)
    n = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    return 0.5 * np.linalg.norm(n, axis=1), n
