// pgtt_raycast_host.h — the host side that libpgtt_render.so, libpgtt_depth.so and libpgtt_lidar.so share on top of the side libraries' prelude
// (pgtt_side_host.h: error string, HIP_TRY, check_device): the check of the robot primitives and the device copies of the scene (model,
// primitives, the ray-ready terrain table).  Everything is in an anonymous namespace and nothing of it is exported.  `who` is the entry
// point's name, the prefix of its messages.
#pragma once
#include <cmath>
#include <vector>

#include "../../include/pgtt_render.h"
#include "pgtt_side_host.h"

namespace {

constexpr int kTabWords = 16;           // ray-ready box, world frame: centre[3], local axes in world coordinates r0[3] r1[3] r2[3], half extents[3], pad

int check_geoms(const PgttRenderGeom* geoms, int ngeom, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (ngeom < 0 || ngeom > PGTT_RENDER_MAX_GEOM) return fail(PGTT_E_ARG, p + "ngeom must be in [0, PGTT_RENDER_MAX_GEOM]");
  for (int g = 0; g < ngeom; g++) {
    if (geoms[g].body < 0 || geoms[g].body >= PGTT_NBODY) return fail(PGTT_E_ARG, p + "geom body outside [0, PGTT_NBODY)");
    if (geoms[g].type < PGTT_RENDER_SPHERE || geoms[g].type > PGTT_RENDER_BOX) return fail(PGTT_E_ARG, p + "unknown geom type");
    if (!(geoms[g].size[0] > 0.f) || (geoms[g].type != PGTT_RENDER_SPHERE && !(geoms[g].size[1] > 0.f)) ||
        (geoms[g].type == PGTT_RENDER_BOX && !(geoms[g].size[2] > 0.f)))
      return fail(PGTT_E_ARG, p + "geom sizes must be positive");
  }
  return PGTT_OK;
}

struct SceneTables {
  int device = 0;
  PgttModel* d_model = nullptr;
  PgttRenderGeom* d_geoms = nullptr;
  float* d_boxes = nullptr;      // [T][B][kTabWords]
  int T = 0, B = 0;

  // after check_device: what is allocated before a failure is the owner's to release()
  int upload(const PgttModel* model, const PgttRenderGeom* geoms, int ngeom) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(&d_model, sizeof(PgttModel)));
    HIP_TRY(hipMalloc(&d_geoms, PGTT_RENDER_MAX_GEOM * sizeof(PgttRenderGeom)));
    HIP_TRY(hipMemcpy(d_model, model, sizeof(PgttModel), hipMemcpyHostToDevice));
    if (ngeom > 0) HIP_TRY(hipMemcpy(d_geoms, geoms, ngeom * sizeof(PgttRenderGeom), hipMemcpyHostToDevice));
    return PGTT_OK;
  }

  // boxes: [T][B][10] as pgtt_set_terrain takes them (centre, quaternion wxyz, half extents); T = 0 removes the terrain.  A refusal leaves the
  // table that is there in place.
  int set_terrain(const float* boxes, int nT, int nB, const char* who) {
    const std::string p = std::string(who) + ": ";
    if (nT < 0 || nB < 0 || nB > PGTT_MAX_BOX) return fail(PGTT_E_ARG, p + "need 0 <= B <= PGTT_MAX_BOX, T >= 0");
    if (nT > 0 && (!boxes || nB == 0)) return fail(PGTT_E_ARG, p + "null table");
    // the box's local axes: columns of the rotation of the NORMALISED quaternion, in double
    std::vector<float> tab((size_t)nT * nB * kTabWords, 0.f);
    for (size_t i = 0; i < (size_t)nT * nB; i++) {
      const float* r = boxes + 10 * i;
      float* t = tab.data() + kTabWords * i;
      double w = r[3], x = r[4], y = r[5], z = r[6];
      const double qn = std::sqrt(w * w + x * x + y * y + z * z);
      if (!(qn > 0.0)) return fail(PGTT_E_ARG, p + "zero quaternion");
      w /= qn; x /= qn; y /= qn; z /= qn;
      const double ax[9] = {w * w + x * x - y * y - z * z, 2 * (x * y + w * z), 2 * (x * z - w * y),
                            2 * (x * y - w * z), w * w - x * x + y * y - z * z, 2 * (y * z + w * x),
                            2 * (x * z + w * y), 2 * (y * z - w * x), w * w - x * x - y * y + z * z};
      t[0] = r[0]; t[1] = r[1]; t[2] = r[2];
      for (int k = 0; k < 9; k++) t[3 + k] = (float)ax[k];
      t[12] = r[7]; t[13] = r[8]; t[14] = r[9];
    }
    HIP_TRY(hipSetDevice(device));
    if (d_boxes) { HIP_TRY(hipFree(d_boxes)); d_boxes = nullptr; }
    T = 0; B = 0;
    if (nT == 0) return PGTT_OK;
    HIP_TRY(hipMalloc(&d_boxes, tab.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(d_boxes, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    T = nT; B = nB;
    return PGTT_OK;
  }

  void release() {
    hipSetDevice(device);
    if (d_model) hipFree(d_model);
    if (d_geoms) hipFree(d_geoms);
    if (d_boxes) hipFree(d_boxes);
    d_model = nullptr; d_geoms = nullptr; d_boxes = nullptr; T = 0; B = 0;
  }
};

}  // namespace
