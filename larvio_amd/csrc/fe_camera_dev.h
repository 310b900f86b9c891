// fe_camera_dev.h - the FORWARD camera model (device code only): normalised undistorted coordinates -> distorted -> pixel.  Everything else in
// the library only undistorts (undistort_point, fe_track_dev.h).  FP64, no contraction, every expression in the order
// larvio_amd/localize.py::distort writes it (include/lvk_c.h, lvk_map_select_queries, states it), so a numpy restatement has the same bits
// for radtan; the equidistant model calls atan, whose last bit is the math library's.
#pragma once
#include "lvk_internal.h"
#include <math.h>

// (x, y) with r2 = x x + y y -> (xd, yd); model 0 radtan (k1, k2, p1, p2), 1 equidistant (k1..k4)
__device__ __forceinline__ void cam_distort(int model, const double* dist, double x, double y, double r2, double& xd, double& yd)
{
    if (model == 0) {
        const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3];
        const double rad = 1.0 + (k2 * r2 + k1) * r2;
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
    } else {
        const double r = sqrt(r2);
        const double th = atan(r), t2 = th * th;
        const double thd = th * (1.0 + t2 * (dist[0] + t2 * (dist[1] + t2 * (dist[2] + t2 * dist[3]))));
        const double s = r > 1e-8 ? thd / r : 1.0;
        xd = x * s; yd = y * s;
    }
}

// the pixel of (x, y): px = fx xd + cx, py = fy yd + cy
__device__ __forceinline__ void cam_project(const CamParams& cam, double x, double y, double r2, double& px, double& py)
{
    double xd, yd;
    cam_distort(cam.model, cam.dist, x, y, r2, xd, yd);
    px = cam.intr[0] * xd + cam.intr[2];
    py = cam.intr[1] * yd + cam.intr[3];
}
