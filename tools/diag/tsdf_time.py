"""Diagnostic (not a test): what the TSDF volume costs, on one synthetic 640 x 480 frame.  Medians of `--reps` (20) samples of icp_tsdf_time
(device events around 20 launches):
  - k_tsdf_integrate at 256^3 and 512^3 voxels over the same 3.07 m cube, with and without colour, and beside each figure the bytes the
    launch must move — the touched voxels' records, read and written — as a fraction of the HBM rate to compare against
    (6.29 TB/s measured with a float4 copy; 8.0 TB/s is the specification);
  - k_tsdf_raycast dense at 640 x 480 and on the 128 x 128 lattice, with normals, on the 256^3 volume; beside the lattice form a blocking
    icp_write_rgbd (what makes the same landmarks of a frame) and the search stage of an iteration (icp_time_kernels) from the same run;
  - the end-to-end errors of tests/test_gpu_tsdf.py::test_frame_to_model_end_to_end (frame-to-model against its frame-to-frame twin).
    python tools/diag/tsdf_time.py [--reps N] [--skip-512]"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-512", action="store_true")
    a = ap.parse_args()
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
