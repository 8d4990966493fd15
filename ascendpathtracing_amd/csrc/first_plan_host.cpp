// first_plan_host.cpp -- libfirstplan_mi355x.so: the CPU twin of the first-bounce plan (pt_first_plan.h), a library of its own so that
// librender_mi355x.so's export list stays what it is.  No GPU, nothing of HIP: the same text the plan kernel and the frame kernel run.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "pt_first_plan.h"

extern "C" {

// The record for a width x height frame of the table `spheres` ([10][8] floats: rows r2, x, y, z, ...).  camera14: pos, g, cx, cy
// (12 doubles; null = the reference's camera for that shape).  -> 0, or 1 for a null pointer or an empty shape.
__attribute__((visibility("default"))) int apt_first_plan_host(uint32_t width, uint32_t height, const float *spheres, double eps,
                                                               const double *camera12, int32_t *record16) {
    if (!spheres || !record16 || !width || !height) return 1;
    apt::Camera cam;
    apt::camera_init(cam, width, height);
    if (camera12) {
        for (int i = 0; i < 3; ++i) { cam.pos[i] = camera12[i]; cam.g[i] = camera12[3 + i]; cam.cx[i] = camera12[6 + i]; cam.cy[i] = camera12[9 + i]; }
    }
    apt::FirstPlanGeom g;
    apt::first_plan_setup(cam, width, height, spheres, (float)eps, g);
    apt::first_plan_premise_origin(g);
    for (int k = 0; k < apt::kFirstPlanWords; ++k) record16[k] = apt::first_plan_entry(g, k);
    return 0;
}

// The camera the record above is made for: pos, g, cx, cy of the reference's frame (12 doubles).
__attribute__((visibility("default"))) int apt_first_plan_camera_host(uint32_t width, uint32_t height, double *camera12) {
    if (!camera12 || !width || !height) return 1;
    apt::Camera cam;
    apt::camera_init(cam, width, height);
    for (int i = 0; i < 3; ++i) { camera12[i] = cam.pos[i]; camera12[3 + i] = cam.g[i]; camera12[6 + i] = cam.cx[i]; camera12[9 + i] = cam.cy[i]; }
    return 0;
}

// first_plan_mask() for one pixel: bit k = sphere k cannot be the first hit of any of its camera rays.
__attribute__((visibility("default"))) uint32_t apt_first_plan_mask_host(const int32_t *record16, uint32_t width, uint32_t height, uint32_t col, uint32_t row) {
    return record16 ? apt::first_plan_mask(record16, width, height, col, row) : 0u;
}

}
