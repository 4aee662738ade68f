"""Point-cloud files.  The reference's demos: raw little-endian 640x480 float8 `[x y z 1 r g b 1]`
(`data/kg_pc8d_{1,2}.bin`, 9 830 400 bytes; reader examples/registration.cpp:285-337, writer
src/kinect_frame_grabber.cpp:252-272).  Any viewer: binary little-endian PLY (save_ply / load_ply), for clouds of any size — the
surface of a TSDF volume (icp_amd.tsdf.TSDFVolume.extract_surface), and with faces its mesh (extract_mesh; load_ply_mesh reads it).
Host code only."""
import numpy as np

VGA_POINTS = 640 * 480


def load_pc8d(path):
    a = np.fromfile(path, dtype="<f4")
    if a.size != VGA_POINTS * 8:
        raise ValueError("%s: expected %d bytes (640x480 float8), got %d" % (path, VGA_POINTS * 32, a.size * 4))
    return a.reshape(VGA_POINTS, 8)


def save_pc8d(path, cloud):
    cloud = np.ascontiguousarray(cloud, dtype="<f4")
    if cloud.size != VGA_POINTS * 8:
        raise ValueError("expected a 640x480 float8 cloud")
    cloud.tofile(path)


_PLY_XYZ, _PLY_NORMAL, _PLY_RGB = ("x", "y", "z"), ("nx", "ny", "nz"), ("red", "green", "blue")


_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _ply_dtype(normals):
    return np.dtype([(n, "<f4") for n in _PLY_XYZ + (_PLY_NORMAL if normals else ())] + [(n, "u1") for n in _PLY_RGB])


def save_ply(path, cloud, normals=None, faces=None):
    """An (n, 8) cloud `[x y z 1 r g b 1]`, and its (n, 4) normals if given, as a binary little-endian PLY: float x y z, float nx ny nz
    with normals, uchar red green blue = rint (255 c) clipped to 0 .. 255.  With faces, an (m, 3) array of vertex indices, also an
    `element face` of `property list uchar int vertex_indices`."""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 8)
    n = cloud.shape[0]
    rec = np.empty(n, _ply_dtype(normals is not None))
    for a, name in enumerate(_PLY_XYZ):
        rec[name] = cloud[:, a]
    if normals is not None:
        normals = np.asarray(normals, np.float32).reshape(-1, 4)
        if normals.shape[0] != n:
            raise ValueError("expected one normal per point")
        for a, name in enumerate(_PLY_NORMAL):
            rec[name] = normals[:, a]
    with np.errstate(invalid="ignore"):
        byte = np.clip(np.rint(np.nan_to_num(cloud[:, 4:7]) * np.float32(255)), 0, 255).astype(np.uint8)
    for a, name in enumerate(_PLY_RGB):
        rec[name] = byte[:, a]
    head = ["ply", "format binary_little_endian 1.0", "comment icp_amd", "element vertex %d" % n]
    head += ["property %s %s" % ("uchar" if rec.dtype[name] == np.uint8 else "float", name) for name in rec.dtype.names]
    face = None
    if faces is not None:
        faces = np.asarray(faces).reshape(-1, 3)
        if faces.size and (faces.min() < 0 or faces.max() >= n):
            raise ValueError("expected vertex indices below the number of points")
        face = np.empty(faces.shape[0], _PLY_FACE)
        face["n"], face["v"] = 3, faces
        head += ["element face %d" % faces.shape[0], "property list uchar int vertex_indices"]
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        if face is not None:
            f.write(face.tobytes())


def load_ply(path):
    """A file save_ply wrote without faces: (cloud (n, 8) with the colour as byte / 255, normals (n, 4) or None)."""
    return _load_ply(path, False)[:2]


def load_ply_mesh(path):
    """A file save_ply wrote, with or without faces: (cloud, normals or None, faces (m, 3) uint32 or None)."""
    return _load_ply(path, True)


def _load_ply(path, with_faces):
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        n, props, fmt, m, face_property = None, [], None, None, False
        for line in iter(f.readline, b""):
            w = line.decode("ascii").split()
            if w[:1] == ["end_header"]:
                break
            if w[:1] == ["format"]:
                fmt = w[1]
            elif w[:2] == ["element", "vertex"]:
                n = int(w[2])
            elif with_faces and w[:2] == ["element", "face"] and n is not None and m is None:
                m = int(w[2])
            elif w[:1] == ["element"]:
                raise ValueError("%s: only a vertex element is supported" % path)
            elif m is not None and w[:1] == ["property"]:
                if w != ["property", "list", "uchar", "int", "vertex_indices"] or face_property:
                    raise ValueError("%s: expected the face property save_ply writes, got %r" % (path, w))
                face_property = True
            elif w[:1] == ["property"]:
                props.append((w[2], w[1]))
        else:
            raise ValueError("%s: no end_header" % path)
        if fmt != "binary_little_endian" or n is None:
            raise ValueError("%s: expected a binary_little_endian PLY with a vertex element" % path)
        normals = any(name == "nx" for name, _ in props)
        want = _ply_dtype(normals)
        if [(name, {"float": "<f4", "uchar": "u1"}.get(kind)) for name, kind in props] != [(name, want[name].str.replace("|", "")) for name in want.names]:
            raise ValueError("%s: expected the properties save_ply writes, got %r" % (path, props))
        data = f.read()
    if m is not None and not face_property:
        raise ValueError("%s: a face element without its property" % path)
    if len(data) != n * want.itemsize + (m or 0) * _PLY_FACE.itemsize:
        raise ValueError("%s: expected %d bytes of vertices%s, got %d" % (path, n * want.itemsize, "" if m is None else " and %d of faces" % (m * _PLY_FACE.itemsize), len(data)))
    faces = None
    if m is not None:
        face = np.frombuffer(data[n * want.itemsize:], _PLY_FACE)
        if (face["n"] != 3).any():
            raise ValueError("%s: only triangles are supported" % path)
        faces = face["v"].astype(np.uint32)
        data = data[:n * want.itemsize]
    rec = np.frombuffer(data, want)
    cloud = np.zeros((n, 8), np.float32)
    cloud[:, 3] = cloud[:, 7] = 1
    for a, name in enumerate(_PLY_XYZ):
        cloud[:, a] = rec[name]
    for a, name in enumerate(_PLY_RGB):
        cloud[:, 4 + a] = rec[name].astype(np.float32) / np.float32(255)
    nrm = None
    if normals:
        nrm = np.zeros((n, 4), np.float32)
        for a, name in enumerate(_PLY_NORMAL):
            nrm[:, a] = rec[name]
    return cloud, nrm, faces
