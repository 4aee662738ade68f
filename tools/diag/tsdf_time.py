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
  - with --register (and nothing else then): a cloud registered against the volume itself (icp_tsdf_register) on the same scene at 256^3:
    the two launches of one iteration as a group (what = 8) and k_tsdf_reg_moments alone (what = 9) over the 16 384 lattice landmarks
    and over the dense 307 200 pixels of a frame 1 degree / 9.9 mm from the start pose; a blocking register of 10 iterations; the
    end-to-end error of that registration; and in the same run, on the same volume, the route it replaces: a blocking raycast_to with
    normals, buildRBC, a point-to-plane iteration, and a blocking track_to_model step beside a blocking register_from of 10 iterations,
    each with its end-to-end error.  Written to profiles/tsdf_register_time.txt as well.
  - with --shift (and nothing else then): the moving volume on the same scene at 256^3 and 512^3, without and with colour: k_tsdf_shift
    alone (what = 10) for a shift of n / 8 voxels along x, y and z against two passes over the volume's bytes at the HBM rate; the launches
    of one region extraction (what = 11) for the kept box of each of those shifts — the n / 8 slab that leaves — beside the full
    extraction (what = 2) and a blocking icp_tsdf_reset of the same run; a blocking shift (extract=True) along z (the volume written
    again before each sample) against the route it replaces: icp_tsdf_read, a numpy roll, icp_tsdf_write.  Written to
    profiles/tsdf_shift_time.txt as well.
    python tools/diag/tsdf_time.py [--reps N] [--skip-512] [--surface | --mesh | --register | --shift]"""
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


def corner_volumes(a, colour=1):
    """The corner scene of tests/tsdf_ref.py fused from six 640 x 480 frames into 256^3 and 512^3 voxels over its 1.02 m cube, mu = 3 voxel edges."""
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import tsdf_ref as T                # noqa: E402
    d = T.corner_camera(width=640, height=480, fx=600.0, cx=319.5, cy=239.5)
    cam = rgbd.RGBDConfig(**d)
    frames = [(T.look_at(eye).reshape(12).astype(np.float32),) + T.render_corner(T.look_at(eye), d)[:2] for eye in T.EYES]
    for n in (256,) if a.skip_512 else (256, 512):
        voxel = 1024.0 / n
        v = tsdf.TSDFVolume(tsdf.TSDFConfig(n, n, n, voxel, (-64.0, -64.0, -64.0), 3.0 * voxel, 64.0, colour))
        for pose, depth, rgb in frames:
            v.integrate(cam, pose, depth, rgb if colour else None)
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


def register(a):
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    import rgbd_ref as R                # noqa: E402
    import tsdf_ref as T                # noqa: E402
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    a.skip_512 = True
    d = T.corner_camera(width=640, height=480, fx=600.0, cx=319.5, cy=239.5, x0=2, y0=3, step_x=5, step_y=3)
    start = T.look_at(T.EYE_CAST)
    true = T.rotate_pose(start, (0.3, 1.0, 0.2), 1.0, (8, -5, 3))
    depth, colour = T.render_corner(true, d)[:2]
    dense = R.cloud(depth, colour, d)
    pose = start.reshape(12).astype(np.float32)

    def errors(p):
        P = np.asarray(p, np.float64).reshape(3, 4)
        c = (np.trace(P[:, :3].T @ true[:, :3]) - 1.0) / 2.0
        return np.degrees(np.arccos(np.clip(c, -1.0, 1.0))), np.linalg.norm(P[:, 3] - true[:, 3])

    for n, v in corner_volumes(a):
        for name, cloud in (("16 384 lattice landmarks", R.landmarks(depth, colour, d, 128)[0]), ("307 200 dense pixels", dense)):
            group = median(lambda: v.time_register(8, cloud, pose, reps=20), a.reps)
            moments = median(lambda: v.time_register(9, cloud, pose, reps=20), a.reps)
            call = blocking(lambda: v.register(cloud, pose, 10, 0.0, 0.0), a.reps)
            rec = v.register(cloud, pose, 10, 0.0, 0.0)
            say("register %d^3 %-26s one iteration (two launches) %8.2f us   k_tsdf_reg_moments alone %8.2f us   (%d blocks, %d members)"
                % (n, name, group, moments, -(-cloud.shape[0] // 256), rec.members))
            say("register %d^3 %-26s blocking register of 10 iterations, host cloud %9.2f us   ends %.4f degrees / %.3f mm from the truth (start %.4f / %.3f), rmse %.3f"
                % ((n, name, call) + errors(rec.pose) + errors(pose) + (rec.rmse,)))
        # the route this replaces, in the same run on the same volume: the view of the volume into F with normals, buildRBC, point-to-plane
        # iterations with a search (the handle of tests/test_gpu_tsdf.py: 128 x 128 landmarks here, 256 representatives, point weight 0.05)
        import icp_checks as K              # noqa: E402
        Mem = icp_amd.Memory
        g = icp_amd.ICP(0)
        g.init(16384, 256, 2e2, 1e-6)
        rgbd.set_config(g, rgbd.RGBDConfig(**d))
        g.set_normals(K.GIVEN, 0)
        g.set_error_metric(K.P2PL, 0.05)
        g.set_rejection(invalid=True)
        z_near, z_far = 200.0, 1600.0
        cast = blocking(lambda: v.raycast_to(g, Mem.F, pose, z_near, z_far, normals=True), a.reps)
        cast_kernel = median(lambda: v.time_kernel(1, rgbd.RGBDConfig(**d), pose, z_near=z_near, z_far=z_far, side=128, reps=20), a.reps)
        build = blocking(lambda: (g.buildRBC(), g.sync()), a.reps)
        rgbd.write(g, Mem.M, depth, colour)

        def twenty_steps():
            for _ in range(20):
                g.step()
            g.sync()

        g.reset_transform()
        step20 = blocking(twenty_steps, a.reps) / 20.0
        step1 = blocking(lambda: (g.step(), g.sync()), a.reps)
        say("route    %d^3 blocking raycast_to F with normals %8.2f us (k_tsdf_raycast on the lattice alone %8.2f us)   buildRBC + sync %8.2f us   one point-to-plane iteration: %8.2f us blocking, %8.2f us each of 20 enqueued"
            % (n, cast, cast_kernel, build, step1, step20))

        def model_step():
            v.raycast_to(g, Mem.F, pose, z_near, z_far, normals=True)
            g.buildRBC()
            rgbd.write(g, Mem.M, depth, colour)
            g.reset_transform()
            k = g.run()
            return tsdf.compose_pose(pose, g.read(Mem.T))[0], k

        def volume_step():
            rgbd.write(g, Mem.M, depth, colour)
            return v.register_from(g, Mem.M, pose, 10, 0.0, 0.0)

        t_model = blocking(model_step, a.reps)
        p_model, k_model = model_step()
        t_volume = blocking(volume_step, a.reps)
        t_from = blocking(lambda: v.register_from(g, Mem.M, pose, 10, 0.0, 0.0), a.reps)
        rec = volume_step()
        say("step     %d^3 blocking track_to_model step without integrate (raycast_to, buildRBC, write M, run: k = %d, compose) %9.2f us   ends %.4f degrees / %.3f mm from the truth"
            % ((n, k_model, t_model) + errors(p_model)))
        say("step     %d^3 blocking track_to_volume step without integrate (write M, register_from of 10 iterations)          %9.2f us   ends %.4f degrees / %.3f mm from the truth   (register_from alone %9.2f us, %d members)"
            % ((n, t_volume) + errors(rec.pose) + (t_from, rec.members)))
        g.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tsdf_register_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def shift(a):
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for colour in (0, 1):
        for n, v in corner_volumes(a, colour):
            name = "shift %d^3 %-14s" % (n, "with colour" if colour else "without colour")
            nbytes = n ** 3 * (24 if colour else 8)
            floor = 2.0 * nbytes / HBM_MEASURED * 1e6
            full = median(lambda: v.time_kernel(2, reps=20), a.reps)
            reset_us = None
            _, _, count = v.extract_surface(capacity=0)
            say("%s the full extraction's launches %9.2f us (%d points)   two passes over %.0f MB at 6.29 TB/s %8.2f us" % (name, full, count, nbytes / 1e6, floor))
            for axis, s in (("x", (n // 8, 0, 0)), ("y", (0, n // 8, 0)), ("z", (0, 0, n // 8)), ("-z", (0, 0, -(n // 8)))):
                us = median(lambda: v.time_shift(10, s, reps=20), a.reps)
                reg = median(lambda: v.time_shift(11, s, reps=20), a.reps)
                lo, hi = tsdf.kept_box(v.cfg, s)
                _, _, leaving = v.extract_surface_region(lo, hi, True, capacity=0)
                say("%s n / 8 along %-2s  k_tsdf_shift %9.2f us = %.2f of the two passes (%.2f TB/s)   the leaving slab's extraction %9.2f us = %.2f of the full one (%d points)"
                    % (name, axis, us, us / floor, 2.0 * nbytes / (us * 1e-6) / 1e12, reg, reg / full, leaving))
            dw, col = v.read()
            reps = a.reps if n <= 256 else min(a.reps, 5)
            s = (0, 0, n // 8)
            t = []
            for _ in range(reps):
                v.write(dw, col)
                t0 = time.perf_counter(); cloud, nrm = v.shift(s, extract=True); t.append((time.perf_counter() - t0) * 1e3)
            v.write(dw, col)
            t0 = time.perf_counter(); v.shift(s); t_plain = (time.perf_counter() - t0) * 1e3
            host = []
            for _ in range(3 if n <= 256 else 1):
                v.write(dw, col)
                t0 = time.perf_counter()
                d2, c2 = v.read()
                d3 = np.zeros_like(d2); d3[:n - s[2]] = d2[s[2]:]
                c3 = None
                if c2 is not None:
                    c3 = np.zeros_like(c2); c3[:n - s[2]] = c2[s[2]:]
                v.write(d3, c3)
                host.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); v.reset(); reset_us = (time.perf_counter() - t0) * 1e6
            say("%s blocking shift (extract=True) along z %9.3f ms (%d points to the host), shift alone %9.3f ms   read + numpy + write %9.1f ms   blocking icp_tsdf_reset %9.2f us"
                % (name, statistics.median(t), cloud.shape[0], t_plain, statistics.median(host), reset_us))
            del dw, col
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tsdf_shift_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-512", action="store_true")
    ap.add_argument("--surface", action="store_true")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--register", action="store_true")
    ap.add_argument("--shift", action="store_true")
    a = ap.parse_args()
    if a.surface:
        return surface(a)
    if a.mesh:
        return mesh(a)
    if a.register:
        return register(a)
    if a.shift:
        return shift(a)
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
