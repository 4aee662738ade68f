"""Diagnostic (not a test): what the RGB-D front end costs, in one process on one synthetic sequence (five 640 x 480 frames walked back and
forth, as bench.py's tracking pass walks them).  Medians of `--reps` (20) samples each:
  - pipelined tracking, two frames in flight, cold and warm: float8 frames from pageable memory and from pinned memory (the
    frames registered as DMA sources: the band goes by DMA), image frames at r = 0 and r = 3 (a sample = `--hops` frames);
  - a blocking icp_write_rgbd beside a blocking icp_write_cloud;
  - the lattice form and the dense form alone (device events around 20 launches) at r = 0, 3, 6, with and without normals;
  - the host's numpy back-projection of the same frame (one thread's worth: numpy's elementwise loops).
    python tools/diag/rgbd_time.py [--reps N] [--hops N] [--json FILE]"""
import argparse
import ctypes as C
import gc
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np          # noqa: E402
import icp_amd              # noqa: E402
from icp_amd import rgbd    # noqa: E402

ORDER = [0, 1, 2, 3, 4, 3, 2, 1]
pc = time.perf_counter


def frames():
    """The sequence as a sensor delivers it — z quantised to counts, the colour to bytes — and the float8 clouds a host makes of exactly those
    images (one array: its rows are registered as DMA sources below): at r = 0 both kinds of frame give the same landmarks, so the same k."""
    synth = [icp_amd.synth_cloud_vga(moved=f).reshape(480, 640, 8) for f in range(5)]
    depth = [np.ascontiguousarray(np.rint(c[..., 2]).astype(np.uint16)) for c in synth]
    colour = [np.ascontiguousarray(np.rint(c[..., 4:7] * 255).astype(np.uint8)) for c in synth]
    clouds = np.stack([host_back_projection(d, c).reshape(-1, 8) for d, c in zip(depth, colour)])
    return clouds, depth, colour


def host_back_projection(depth, colour):
    """The reference's writer in numpy: what a host does per frame to make the float8 cloud the engine takes today."""
    z = depth.astype(np.float32)
    u = np.arange(640, dtype=np.float32)[None, :]
    v = np.arange(480, dtype=np.float32)[:, None]
    out = np.empty((480, 640, 8), np.float32)
    out[..., 0] = (u - np.float32(319.5)) * z / np.float32(595)
    out[..., 1] = (v - np.float32(239.5)) * z / np.float32(595)
    out[..., 2] = z
    out[..., 3] = 1
    out[..., 4:7] = colour.astype(np.float32) / np.float32(255)
    out[..., 7] = 1
    return out


def median_us(call, reps):
    call(); call()
    t = []
    for _ in range(reps):
        t0 = pc(); call(); t.append((pc() - t0) * 1e6)
    return round(statistics.median(t), 2)


def pipelined_fps(g, submit, hops, reps):
    """Median frames/s of `reps` passes of `hops` frames with two in flight (submit frame i, then collect frame i - 1); 8 untimed frames first."""
    g.track_reset()
    for i in range(8):
        submit(i)
        if i >= 1:
            g.track_collect()
    g.track_collect()
    fps, ks = [], []
    i0 = 8
    gc.collect(); gc.disable()
    for _ in range(reps):
        t0 = pc()
        for i in range(i0, i0 + hops):
            submit(i)
            if i > i0:
                ks.append(g.track_collect()[0])
        ks.append(g.track_collect()[0])
        fps.append(hops / (pc() - t0))
        i0 += hops
    gc.enable()
    return round(statistics.median(fps), 1), round(float(np.mean(ks)), 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hops", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    clouds, depth, colour = frames()
    L = rgbd._lib()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    out = {"reps": a.reps, "hops_per_sample": a.hops}

    # upload bytes per frame
    box = lambda r: (min(480, 49 + 3 * 127 + r + 1) - max(0, 49 - r)) * (min(640, 65 + 4 * 127 + r + 1) - max(0, 65 - r)) * 2
    out["upload_bytes_per_frame"] = {"float8 band": 128 * 509 * 32, "images r=0": box(0) + 128 * 509 * 3, "images r=3": box(3) + 128 * 509 * 3,
                                     "images r=0 without colour": box(0)}
    print("upload bytes per frame:", json.dumps(out["upload_bytes_per_frame"]), flush=True)

    # tracking
    out["tracking_frames_per_s"] = {}
    for name, warm in (("cold", False), ("warm", True)):
        g = icp_amd.ICP(0)
        g.init(16384, 256, 2e2, 1e-6)
        h = g._h
        res = {}
        seq = lambda i: ORDER[i % len(ORDER)]
        res["float8 pageable"] = pipelined_fps(g, lambda i: g._chk(L.icp_track_submit(h, p(clouds[seq(i)]), int(warm))), a.hops, a.reps)
        g.track_reset()
        g.track_register(clouds)
        res["float8 pinned (registered sources)"] = pipelined_fps(g, lambda i: g._chk(L.icp_track_submit(h, p(clouds[seq(i)]), int(warm))), a.hops, a.reps)
        g.track_reset()
        g.track_unregister(clouds)
        for r in (0, 3):
            g.track_reset()
            rgbd.set_config(g, rgbd.RGBDConfig(radius=r))
            res["images r=%d" % r] = pipelined_fps(
                g, lambda i: g._chk(L.icp_track_submit_rgbd(h, p(depth[seq(i)]), p(colour[seq(i)]), int(warm))), a.hops, a.reps)
        g.close()
        out["tracking_frames_per_s"][name] = {k: {"frames_per_s": v[0], "mean_k": v[1]} for k, v in res.items()}
        for k, v in res.items():
            print("tracking %-5s %-46s %9.1f frames/s   (mean k %.2f)" % (name, k, v[0], v[1]), flush=True)

    # blocking writes
    g = icp_amd.ICP(0)
    g.init(16384, 256, 2e2, 1e-6)
    h = g._h
    w = {"icp_write_cloud (9.83 MB float8)": median_us(lambda: g._chk(L.icp_write_cloud(h, icp_amd.Memory.M, p(clouds[1]), 1)), a.reps)}
    for r, n in ((0, 0), (3, 0), (3, 1)):
        rgbd.set_config(g, rgbd.RGBDConfig(radius=r))
        w["icp_write_rgbd r=%d%s" % (r, " + normals" if n else "")] = median_us(
            lambda: g._chk(L.icp_write_rgbd(h, icp_amd.Memory.M, p(depth[1]), p(colour[1]), n, 1)), a.reps)
    out["blocking_write_us"] = w
    for k, v in w.items():
        print("blocking %-40s %9.2f us" % (k, v), flush=True)

    # the kernels alone
    out["kernel_us"] = {}
    for r in (0, 3, 6):
        rgbd.set_config(g, rgbd.RGBDConfig(radius=r))
        for form, dense in (("lattice", 0), ("dense 640 x 480", 1)):
            for n in (0, 1):
                us = statistics.median(rgbd.time_kernel(g, dense, depth[1], colour[1], normals=n, reps=20) for _ in range(a.reps))
                key = "%s r=%d%s" % (form, r, " + normals" if n else "")
                out["kernel_us"][key] = round(us, 2)
                print("kernel   %-40s %9.2f us" % (key, us), flush=True)
    g.close()

    # the host
    out["host_numpy_back_projection_us"] = median_us(lambda: host_back_projection(depth[1], colour[1]), a.reps)
    print("host     numpy back-projection of one frame          %9.2f us" % out["host_numpy_back_projection_us"], flush=True)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
