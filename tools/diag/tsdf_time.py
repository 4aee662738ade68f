"""Diagnostic (not a test): what the TSDF volume costs, on one synthetic 640 x 480 frame.  Medians of `--reps` (20) samples of icp_tsdf_time
(device events around 20 launches):
  - k_tsdf_integrate at 256^3 and 512^3 voxels over the same 3.07 m cube, with and without colour, and beside each figure the bytes the
    launch must move — the touched voxels' records, read and written — as a fraction of the HBM rate to compare against
    (6.29 TB/s measured with a float4 copy; 8.0 TB/s is the specification);
  - k_tsdf_raycast dense at 640 x 480 and on the 128 x 128 lattice, with normals, on the 256^3 volume; beside the lattice form a blocking
    icp_write_rgbd (what makes the same landmarks of a frame) and the search stage of an iteration (icp_time_kernels) from the same run;
  - the end-to-end errors of tests/test_gpu_tsdf.py::test_frame_to_model_end_to_end (frame-to-model against its frame-to-frame twin);
  - with --surface (and nothing else then): the surface extraction of the corner scene of tests/tsdf_ref.py — six 640 x 480 frames fused
    into 256^3 and 512^3 voxels over the scene's 1.02 m cube, mu = 3 voxel edges —: the launches of one extraction as a group
    (icp_tsdf_time, what = 2) against one read of the volume's {D, W} at the HBM rate, the two scan launches (what = 3) and the
    scatter and points launches (what = 4) alone, the
    blocking calls with the copy to the host, and what they replace: a blocking icp_tsdf_read plus the numpy restatement on the host
    (the restatement at 256^3 only: at 512^3 its temporaries do not fit a workstation's memory).
  - with --mesh (and nothing else then): the mesh extraction of the same scene and volumes: the launches of one extract_mesh as a group
    (what = 5) beside those of extract_surface with normals (what = 2) from the same run, the cell sweep (what = 6) and the triangle
    pass (what = 7) alone, each against one read of {D, W} at the HBM rate; the blocking call with both capacities given and with the
    counting call first; the vertex and triangle counts.
    python tools/diag/tsdf_time.py [--reps N] [--skip-512] [--surface | --mesh]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import icp_amd              # noqa: E402
from icp_amd import rgbd, tsdf    # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
Z_NEAR, Z_FAR = 400.0, 3800.0


def frame():
    c = icp_amd.synth_cloud_vga().reshape(480, 640, 8)
    return np.ascontiguousarray(np.rint(c[..., 2]).astype(np.uint16)), np.ascontiguousarray(np.rint(c[..., 4:7] * 255).astype(np.uint8))


def volume(n, colour):
    voxel = 3072.0 / n
    return tsdf.TSDFVolume(tsdf.TSDFConfig(n, n, n, voxel, (-1536.0, -1536.0, 300.0), 4.0 * voxel, 64.0, colour))


def median(call, reps):
    return statistics.median(call() for _ in range(reps))


def blocking(call, reps):
    call(); call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t)


def corner_volumes(a):
    """The corner scene of tests/tsdf_ref.py fused from six 640 x 480 frames into 256^3 and 512^3 voxels over its 1.02 m cube, mu = 3 voxel edges."""
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import tsdf_ref as T                # noqa: E402
    d = T.corner_camera(width=640, height=480, fx=600.0, cx=319.5, cy=239.5)
    cam = rgbd.RGBDConfig(**d)
    frames = [(T.look_at(eye).reshape(12).astype(np.float32),) + T.render_corner(T.look_at(eye), d)[:2] for eye in T.EYES]
    for n in (256,) if a.skip_512 else (256, 512):
        voxel = 1024.0 / n
        v = tsdf.TSDFVolume(tsdf.TSDFConfig(n, n, n, voxel, (-64.0, -64.0, -64.0), 3.0 * voxel, 64.0, 1))
        for pose, depth, colour in frames:
            v.integrate(cam, pose, depth, colour)
        yield n, v
        v.close()


def surface(a):
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import tsdf_ref as T                # noqa: E402
    import tsdf_surface_ref as S        # noqa: E402
    for n, v in corner_volumes(a):
        floor = n ** 3 * 8 / HBM_MEASURED * 1e6
        cloud, nrm, count = v.extract_surface(capacity=0)
        group = median(lambda: v.time_kernel(2, reps=20), a.reps)
        scan = median(lambda: v.time_kernel(3, reps=20), a.reps)
        scatter = median(lambda: v.time_kernel(4, reps=20), a.reps)
        print("surface %d^3: %d points (%.2f %% of %d edges), %d blocks of the sweep" % (n, count, 100.0 * count / (3 * n * n * (n - 1)), 3 * n * n * (n - 1), n ** 3 // 1024), flush=True)
        print("surface %d^3 launches of one extraction %9.2f us   one read of {D, W} at 6.29 TB/s %7.2f us: ratio %.2f" % (n, group, floor, group / floor), flush=True)
        print("surface %d^3 the two scan launches      %9.2f us   %.1f %% of the extraction" % (n, scan, 100.0 * scan / group), flush=True)
        print("surface %d^3 scatter and points alone   %9.2f us   (the sweep: the rest, %.2f us = %.2f of the read)" % (n, scatter, group - scan - scatter, (group - scan - scatter) / floor), flush=True)
        one = blocking(lambda: v.extract_surface(capacity=count), a.reps)
        two = blocking(lambda: v.extract_surface(), a.reps)
        cnt = blocking(lambda: v.extract_surface(capacity=0), a.reps)
        print("surface %d^3 blocking extract_surface   %9.2f us with the capacity given, %9.2f us with the counting call first, %9.2f us the counting call alone  (%.1f MB to the host)"
              % (n, one, two, cnt, count * 48 / 1e6), flush=True)
        t0 = time.perf_counter(); dw, col = v.read(); t_read = time.perf_counter() - t0
        print("surface %d^3 blocking icp_tsdf_read     %9.2f ms  (%.0f MB of {D, W}, %.0f MB of colour)" % (n, t_read * 1e3, dw.nbytes / 1e6, col.nbytes / 1e6), flush=True)
        if n == 256:
            ref = T.Volume(v.get_config().as_dict())
            ref.dw, ref.rgb = dw, col
            t0 = time.perf_counter(); want = S.extract(ref); t_host = time.perf_counter() - t0
            got = v.extract_surface()
            same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, want))
            print("surface %d^3 the numpy restatement on the host %9.2f ms  (%d points, %s the device's bit for bit)" % (n, t_host * 1e3, want[0].shape[0], "equal to" if same else "DIFFERENT FROM"), flush=True)
        else:
            print("surface %d^3 the numpy restatement on the host: not measured" % n, flush=True)
        del dw, col


def mesh(a):
    for n, v in corner_volumes(a):
        floor = n ** 3 * 8 / HBM_MEASURED * 1e6
        _, _, _, nv, nt = v.extract_mesh(vertex_capacity=0, triangle_capacity=0)
        points = median(lambda: v.time_kernel(2, reps=20), a.reps)
        group = median(lambda: v.time_kernel(5, reps=20), a.reps)
        cells = median(lambda: v.time_kernel(6, reps=20), a.reps)
        tris = median(lambda: v.time_kernel(7, reps=20), a.reps)
        print("mesh %d^3: %d vertices, %d triangles (%.2f a vertex)" % (n, nv, nt, nt / max(nv, 1)), flush=True)
        print("mesh %d^3 launches of one extract_mesh     %9.2f us = %.2f of one read of {D, W} at 6.29 TB/s (%.2f us)" % (n, group, group / floor, floor), flush=True)
        print("mesh %d^3 launches of one extract_surface  %9.2f us = %.2f of the read: the mesh costs %.2f us more" % (n, points, points / floor, group - points), flush=True)
        print("mesh %d^3 the cell sweep alone             %9.2f us = %.2f of the read" % (n, cells, cells / floor), flush=True)
        print("mesh %d^3 the triangle pass alone          %9.2f us = %.2f of the read  (the second scan: the rest, %.2f us)" % (n, tris, tris / floor, group - points - cells - tris), flush=True)
        one = blocking(lambda: v.extract_mesh(vertex_capacity=nv, triangle_capacity=nt), a.reps)
        two = blocking(lambda: v.extract_mesh(), a.reps)
        cnt = blocking(lambda: v.extract_mesh(vertex_capacity=0, triangle_capacity=0), a.reps)
        print("mesh %d^3 blocking extract_mesh            %9.2f us with both capacities given, %9.2f us with the counting call first, %9.2f us the counting call alone  (%.1f MB to the host)"
              % (n, one, two, cnt, (nv * 48 + nt * 12) / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-512", action="store_true")
    ap.add_argument("--surface", action="store_true")
    ap.add_argument("--mesh", action="store_true")
    a = ap.parse_args()
    if a.surface:
        return surface(a)
    if a.mesh:
        return mesh(a)
    depth, colour = frame()
    cam = rgbd.RGBDConfig()
    print("frame: %d of %d pixels valid, depth %d .. %d" % ((depth != 0).sum(), depth.size, depth[depth != 0].min(), depth.max()), flush=True)
    kept = None
    for n in (256,) if a.skip_512 else (256, 512):
        touched = None
        for with_colour in (0, 1):
            v = volume(n, with_colour)
            us = median(lambda: v.time_kernel(0, cam, IDENTITY, depth, colour if with_colour else None, reps=20), a.reps)
            if touched is None:
                touched = int(np.count_nonzero(v.read()[0][..., 1]))
            moved = touched * (48 if with_colour else 16)
            rate = moved / (us * 1e-6)
            print("integrate %d^3 %-14s %9.2f us   %d of %d voxels touched, %.1f MB read and written: %.2f TB/s = %.2f of 6.29 TB/s measured (%.2f of 8.0 TB/s)"
                  % (n, "with colour" if with_colour else "without colour", us, touched, n ** 3, moved / 1e6, rate / 1e12, rate / HBM_MEASURED, rate / HBM_SPEC), flush=True)
            if n == 256 and with_colour:
                kept = v
            else:
                v.close()
    cloud, nrm = kept.raycast(cam, IDENTITY, Z_NEAR, Z_FAR, side=128)
    print("ray cast of the 256^3 volume: %d of 16384 landmarks hit, %d with a normal" % ((cloud[:, 2] != 0).sum(), np.any(nrm[:, :3] != 0, axis=1).sum()), flush=True)
    for name, side in (("dense 640 x 480", 0), ("lattice 128 x 128", 128)):
        us = median(lambda: kept.time_kernel(1, cam, IDENTITY, z_near=Z_NEAR, z_far=Z_FAR, side=side, reps=20), a.reps)
        print("ray cast  %-24s %9.2f us   (%d samples a ray at most)" % (name, us, int((Z_FAR - Z_NEAR) / (0.5 * kept.cfg.mu)) + 1), flush=True)
    g = icp_amd.ICP(0)
    g.init(16384, 256, 2e2, 1e-6)

    def blocking(call):
        call(); call()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); call(); t.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(t)

    print("blocking  icp_tsdf_raycast_to F    %9.2f us" % blocking(lambda: kept.raycast_to(g, icp_amd.Memory.F, IDENTITY, Z_NEAR, Z_FAR, normals=True)), flush=True)
    print("blocking  icp_write_rgbd M         %9.2f us" % blocking(lambda: rgbd.write(g, icp_amd.Memory.M, depth, colour)), flush=True)
    g.buildRBC()
    print("search stage of an iteration     %9.2f us   (icp_time_kernels, 16384 landmarks, 256 representatives)" % (g.time_kernels(50)["search"] * 1e3), flush=True)
    g.close(); kept.close()
    # the end-to-end registration of the GPU test
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools", "diag")]
    import test_gpu_tsdf as G          # noqa: E402
    dev = G._fuse_on_device((64, 64, 64), 1)
    model, twin, start = G.frame_to_model_errors(icp_amd, dev)
    dev.close()
    print("end to end (corner scene, 64^3 voxels of 16 mm; the motion is %.2f degrees and %.2f mm):" % start)
    print("  frame-to-model      k %2d   rotation error %.4f degrees   translation error %.3f mm" % (model[0], model[2], model[3]))
    print("  frame-to-frame twin k %2d   rotation error %.4f degrees   translation error %.3f mm" % (twin[0], twin[2], twin[3]), flush=True)


if __name__ == "__main__":
    main()
