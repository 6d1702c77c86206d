// pgtt_sensor.hip.h — what the two onboard ray sensors, libpgtt_depth.so (pgtt_depth.hip) and libpgtt_lidar.so (pgtt_lidar.hip), state in common on
// top of the ray casters' core (pgtt_raycast.hip.h, pgtt_raycast_host.h).  Included by those two units only.
// Device: the workgroup's shape and the LDS records' size, the sphere and capsule tests for a ray from the frame's origin along a unit d, the noise
// tail of a reading, and the one-thread kernel that advances a sensor's tick counter.
// Host: the checks of the config fields both sensors have, with both libraries' messages; the mount quaternion's normalisation; the copy of
// what both argument structs hold; the launch pair of a tick.  Everything is in an anonymous namespace; `who` is the entry point's name.
// NOT here: the body chain, the placement with its compaction, hit_box, the culls and the pixel / ray loops.  They stand inline in both kernels,
// and pgtt_raycast.hip.h records what moving them does to the device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pgtt_raycast.hip.h"
#include "pgtt_raycast_host.h"
#include "pgtt_side_device.hip.h"

namespace {

constexpr int kLanes = 256;             // lanes per workgroup = per env
constexpr int kWaves = kLanes / 64;
constexpr int kBoxWords = 16;           // LDS box, sensor frame: ray origin in the box frame[3], axes r0 r1 r2 [9], half extents[3], pad
constexpr int kGeomWords = 16;          // LDS geom, sensor frame: centre[3], axes r0 r1 r2 [9], size[3], type
static_assert(PGTT_MAX_BOX <= kLanes && PGTT_RENDER_MAX_GEOM <= 64, "one lane per box, the geoms in one wave");

// sphere / capsule for a ray from the origin along the UNIT direction d: t = distance along the ray
__device__ __forceinline__ float hit_sphere(V3 oc, V3 d, float r) {
  const float b = dot(oc, d), cc = dot(oc, oc) - r * r, disc = b * b - cc;
  if (disc < 0.f) return INFINITY;
  const float t = -b - sqrtf(disc);
  return t > 0.f ? t : INFINITY;
}
// the cylinder's quadratic in its cross-product form; a <= 1e-12 baba, decided before h: the ray runs along the axis (see pgtt_raycast.hip.h)
__device__ __forceinline__ float hit_capsule(V3 d, V3 c, V3 ax, float r, float hl) {
  const V3 pa = c - hl * ax, ba = (2.f * hl) * ax, oa = -1.f * pa;
  const V3 bd = cross(ba, d), bo = cross(ba, oa);
  const float baba = dot(ba, ba), bard = dot(ba, d), baoa = dot(ba, oa);
  const float a = dot(bd, bd), b = dot(bd, bo), cc = dot(bo, bo) - r * r * baba;
  if (!(a > 1e-12f * baba)) return fminf(hit_sphere(oa, d, r), hit_sphere(oa - ba, d, r));
  const float h = b * b - a * cc;
  if (h < 0.f) return INFINITY;
  const float t = (-b - sqrtf(h)) / a, y = baoa + t * bard;
  if (y > 0.f && y < baba) return t > 0.f ? t : INFINITY;
  return hit_sphere(y <= 0.f ? oa : oa - ba, d, r);
}

// the noise of reading idx (pixel or ray) of env e at `tick`, on the clamped val: the draws of `stream` keyed as the env's own are (pgtt.h);
// a dropout reads far_m, every other reading is scaled by 1 + sigma z and clamped again
__device__ __forceinline__ float noisy(float val, unsigned long long seed, long long env_off, int e, long long tick, unsigned stream, int idx,
                                       float sigma, float dropout, float near_m, float far_m) {
  unsigned c0 = (unsigned)(env_off + e), c1 = (unsigned)tick, c2 = stream, c3 = (unsigned)idx;
  philox4x32_10((unsigned)seed, (unsigned)(seed >> 32), c0, c1, c2, c3);
  const float k24 = 1.0f / 16777216.0f;
  const float u0 = (float)(c0 >> 8) * k24, u1 = (float)(c1 >> 8) * k24, u2 = (float)(c2 >> 8) * k24;
  const float z = sqrtf(-2.f * logf(1.f - u1)) * cosf(6.283185307179586f * u2);
  return u0 < dropout ? far_m : fminf(fmaxf(val * (1.f + sigma * z), near_m), far_m);
}

// enqueued behind a tick: the next one reads the counter advanced, and no workgroup of this one reads it changed
__global__ void __launch_bounds__(64) sensor_advance_kernel(int64_t* counter) {
  if (threadIdx.x == 0 && blockIdx.x == 0) counter[0] = counter[0] + 1;
}

// ---------------------------------------------------------------- host
// |q| in double
double quat_norm(const float* q) {
  double n = 0.0;
  for (int i = 0; i < 4; i++) n += (double)q[i] * q[i];
  return std::sqrt(n);
}

// the fields PgttDepthConfig and PgttLidarConfig both have, checked in the order both libraries always did
template <class Cfg>
int check_sensor_config(const Cfg* cfg, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (!(cfg->near > 0.f) || !(cfg->near < cfg->far) || !std::isfinite(cfg->far)) return fail(PGTT_E_ARG, p + "need 0 < near < far, finite");
  if (cfg->mount_body < 0 || cfg->mount_body >= PGTT_NBODY) return fail(PGTT_E_ARG, p + "mount_body outside [0, PGTT_NBODY)");
  if (cfg->every < 1) return fail(PGTT_E_ARG, p + "every must be >= 1");
  if (cfg->see_robot != 0 && cfg->see_robot != 1) return fail(PGTT_E_ARG, p + "see_robot must be 0 or 1");
  if (!(cfg->noise_sigma >= 0.f) || !std::isfinite(cfg->noise_sigma)) return fail(PGTT_E_ARG, p + "noise_sigma must be >= 0");
  if (!(cfg->dropout >= 0.f) || !(cfg->dropout < 1.f)) return fail(PGTT_E_ARG, p + "dropout must be in [0, 1)");
  const double qn = quat_norm(cfg->mount_quat);
  if (!(qn > 0.0) || !std::isfinite(qn)) return fail(PGTT_E_ARG, p + "mount_quat must be a non-zero quaternion");
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(cfg->mount_pos[i])) return fail(PGTT_E_ARG, p + "mount_pos must be finite");
  return PGTT_OK;
}

// a checked config as the handle keeps it: mount_quat normalised in double
template <class Cfg>
Cfg with_unit_mount(const Cfg& cfg) {
  Cfg c = cfg;
  const double qn = quat_norm(cfg.mount_quat);
  for (int i = 0; i < 4; i++) c.mount_quat[i] = (float)(cfg.mount_quat[i] / qn);
  return c;
}

// what DepthArgs and LidarArgs both hold (two structs, not one base: each kernel keeps its parameter layout); ngeom = the handle's, 0 is
// passed on when the robot is not in the scene
template <class Args, class Cfg, class Bufs>
void fill_sensor_args(Args& a, const Cfg& c, const Bufs& b, const SceneTables& s, int num_envs, int ngeom, int force) {
  a.state = b.state; a.params = b.params; a.variant = b.variant; a.counter = b.counter;
  a.boxes = s.d_boxes; a.model = s.d_model; a.geoms = s.d_geoms;
  a.N = num_envs; a.T = s.T; a.B = s.B; a.ngeom = c.see_robot ? ngeom : 0;
  a.mount_body = c.mount_body; a.every = c.every; a.force = force ? 1 : 0;
  a.near_m = c.near; a.far_m = c.far;
  for (int i = 0; i < 3; i++) a.mpos[i] = c.mount_pos[i];
  for (int i = 0; i < 4; i++) a.mquat[i] = c.mount_quat[i];
  a.sigma = c.noise_sigma; a.dropout = c.dropout; a.seed = c.seed; a.env_off = c.env_id_offset;
}

// one tick: the kernel with the noise tail or the one without, one workgroup per env, and the counter's advance behind it
template <class Args>
int launch_sensor_tick(void (*with_noise)(Args), void (*without)(Args), const Args& a, hipStream_t st) {
  hipLaunchKernelGGL((a.sigma > 0.f || a.dropout > 0.f) ? with_noise : without, dim3(a.N), dim3(kLanes), 0, st, a);
  hipLaunchKernelGGL(sensor_advance_kernel, dim3(1), dim3(64), 0, st, a.counter);
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

}  // namespace
