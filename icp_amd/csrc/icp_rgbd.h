// icp_rgbd.h — what the host-side translation units share with the RGB-D front end (icp_rgbd.hip): the arguments of its two kernels,
// their launchers, and the checks of an icp_rgbd_t that icp_set_rgbd, icp_write_rgbd and icp_kernel_rgbd have in common.
#pragma once
#include "../../include/icp_amd.h"
#include "icp_kernels.h"

// One launch.  Image pixel (u, v) has its count at depth[(v - dy0) * dpitch + (u - dx0)] and its colour at
// rgb[(((v - cy0) / cstep) * cpitch + (u - cx0)) * 3]: the dense form holds whole images (origins 0, pitches = width, cstep = 1); the lattice
// form holds whatever covers the lattice's bounding box grown by radius (+ 1 with normals) and the lattice's own colour rows —
// icp_write_rgbd whole image rows, tracking the packed region (icp_rgbd_region).  rgb, nrm: may be null.
struct icp_rgbd_args {
    icp_rgbd_t c;
    const uint16_t *depth; const uint8_t *rgb;
    uint32_t dx0, dy0, dpitch;
    uint32_t cx0, cy0, cpitch, cstep;
    uint32_t side;                               // lattice form: side x side landmarks
    float4 *out, *nrm;                           // [pixels or landmarks][2] float4, [pixels or landmarks] float4
};

// What the lattice form reads of an image pair: depth rows [dy0, dy1) x columns [dx0, dx1), the bounding box grown by radius (+ 1 with
// normals) and clipped to the image; colour rows y0, y0 + step_y, .. (side of them) x columns [x0, cx1).
struct icp_rgbd_region {
    uint32_t dx0, dx1, dy0, dy1, cx1;
    size_t depth_bytes (bool packed, uint32_t width) const { return (size_t) (dy1 - dy0) * (packed ? dx1 - dx0 : width) * sizeof (uint16_t); }
};
icp_rgbd_region icp_rgbd_region_of (const icp_rgbd_t &c, uint32_t side, bool normals);

void icp_launch_rgbd_dense (const icp_rgbd_args &a, hipStream_t s);
void icp_launch_rgbd_lattice (const icp_rgbd_args &a, hipStream_t s);

// the table of include/icp_amd.h
icp_rgbd_t icp_rgbd_default ();
// nullptr, or which range of the header's `c` leaves (the lattice fields included)
const char *icp_rgbd_refusal (const icp_rgbd_t &c);
// the lattice of side x side landmarks lies inside the image
bool icp_rgbd_lattice_fits (const icp_rgbd_t &c, uint32_t side);
