// project_view.h -- the inverse of the pinhole camera (pt_project_view, include/pt/pt.h): one definition for the host
// entry point (scene.cpp) and the temporal kernel (hip/pt_temporal.hip), so the two cannot drift apart.  The
// arithmetic is the header's, one rounded f32 operation at a time (every TU is compiled without contraction).
#pragma once

#include "pt/pt.h"

#ifdef __HIPCC__
#define PT_HOST_DEVICE __host__ __device__
#else
#define PT_HOST_DEVICE
#endif

namespace pt {

// What a NULL view projects as: right = +x, up = +y, back = +z, film 1 x 1.
PT_HOST_DEVICE inline pt_view identity_view()
{
    pt_view v;
    v.right[0] = 1.0f; v.right[1] = 0.0f; v.right[2] = 0.0f;
    v.up[0] = 0.0f; v.up[1] = 1.0f; v.up[2] = 0.0f;
    v.back[0] = 0.0f; v.back[1] = 0.0f; v.back[2] = 1.0f;
    v.film_w = 1.0f;
    v.film_h = 1.0f;
    return v;
}

// The continuous pixel coordinates at which the pinhole ray of (cam, view) passes through P; false (and *sx, *sy
// whatever the arithmetic gave) when P is not in front of the camera.
PT_HOST_DEVICE inline bool project_view(const pt_camera& cam, const pt_view& view, float Px, float Py, float Pz, float* sx, float* sy)
{
    const float qx = Px - cam.pos.x, qy = Py - cam.pos.y, qz = Pz - cam.pos.z;
    const float cx = (view.right[0] * qx + view.right[1] * qy) + view.right[2] * qz;
    const float cy = (view.up[0] * qx + view.up[1] * qy) + view.up[2] * qz;
    const float cz = (view.back[0] * qx + view.back[1] * qy) + view.back[2] * qz;
    const bool front = cz < 0.0f;
    const float gx = (cx * cam.dist_from_film) / cz;
    const float gy = (cy * cam.dist_from_film) / cz;
    *sx = (gx / view.film_w + 0.5f) * (float)cam.pxl_width;
    *sy = (gy / view.film_h + 0.5f) * (float)cam.pxl_height;
    return front;
}

}  // namespace pt
