// pgtt_lidar.hip — libpgtt_lidar.so: the scanning range sensor (include/pgtt_lidar.h), one workgroup per env.
//
// lidar_kernel, 256 lanes per env, the shape of depth_kernel (pgtt_depth.hip):
//   phase A  lanes 0..3 run the forward kinematics of one leg each (the formulas of mjcf.kinematics_np; only when the mount is not on the
//            torso or the robot is in the scene); every lane then forms the sensor basis from the mount body's pose.
//            Lane b < B moves box b of the env's variant into the SENSOR frame (the ray origin is the frame's origin) and tests its bounding
//            sphere against the sensor's reach: a scanner looks everywhere, so there is no cone, only |c| - r <= far.  Survivors are compacted
//            into LDS in box order with a ballot and prefix counts: no atomics, so the list is deterministic.  The posed robot geoms go the
//            same way.
//   phase B  rays over lanes, 256 per pass.  Ray r's unit direction in the sensor frame is one 16-byte row of the pattern table, the same for
//            every env (a coalesced read that L2 serves).  Every lane walks the same list (LDS broadcasts, wave-uniform trip count), takes
//            the minimum with the plane, clamps, adds the noise, stores the range coalesced and the world point as a 12-byte-per-lane run.
// A pattern direction may be exactly perpendicular to a box axis, and hit_box states that case.  (So may a camera ray: with an odd width or
// height the centre column or row of (u, v, 1) has u = 0 or v = 0.  The camera leaves it to rcp(0) = inf, which decides the slab the same way:
// inside it no constraint, outside it a miss; tests/test_gpu_raycast_edges.py holds both kernels to that.)
// A tick that the sensor period skips returns at once in every workgroup (the decision reads counter[0] on the device); sensor_advance_kernel,
// enqueued behind it, adds one to the counter.  Nothing is shared between envs: an env's scan does not depend on the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/pgtt_lidar.h"
#include "pgtt_sensor.hip.h"

namespace {

struct LidarArgs {
  const float* state;
  const float* params;
  const int32_t* variant;
  float* range;
  float* points;                        // or nullptr
  int64_t* counter;
  const float* boxes;                   // [T][B][kTabWords]
  const PgttModel* model;
  const PgttRenderGeom* geoms;
  const float4* dirs;                   // [R]: unit direction in the sensor frame, pad
  int N, T, B, ngeom;                   // ngeom = 0 when the robot is not in the scene
  int R, mount_body, every, force;
  float near_m, far_m;
  float mpos[3], mquat[4];
  float sigma, dropout;
  unsigned long long seed;
  long long env_off;
};

// the sensor: world vector -> sensor frame (its own x, y, z axes)
struct Sensor { V3 o, ax, ay, az; };
__device__ __forceinline__ V3 to_sensor(const Sensor& s, V3 w) { return v3(dot(s.ax, w), dot(s.ay, w), dot(s.az, w)); }

// May a ray from the origin, out to range far_m, touch the sphere (centre c in the sensor frame, radius r)?  A hit farther than far_m reads
// far_m like a miss.  The slack (that of the camera's sphere_in_view) covers the fp32 rounding of the centre and of the test itself.
__device__ __forceinline__ bool sphere_in_reach(V3 c, float r, float far_m) {
  const float n = sqrtf(dot(c, c));
  const float slack = 1e-3f * r + 1e-5f * (1.f + n);
  return n - r <= far_m + slack;
}

// slab test of the ray t * d against a box record (origin in the box frame, axes, half extents): t of the entry (a ray that starts inside the
// box does not see it).  A direction component that is exactly 0 along an axis: inside that slab the axis is no constraint, outside it is a miss.
__device__ __forceinline__ float hit_box(const float* __restrict__ r, V3 d) {
  float tn = -INFINITY, tf = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float dl = r[3 + 3 * k] * d.x + r[4 + 3 * k] * d.y + r[5 + 3 * k] * d.z;
    const float ol = r[k], h = r[12 + k];
    if (dl == 0.f) {
      if (fabsf(ol) > h) tf = -INFINITY;
    } else {
      const float inv = __builtin_amdgcn_rcpf(dl);
      const float t1 = (-h - ol) * inv, t2 = (h - ol) * inv;
      tn = fmaxf(tn, fminf(t1, t2));
      tf = fminf(tf, fmaxf(t1, t2));
    }
  }
  return (tn <= tf && tn > 0.f) ? tn : INFINITY;
}

template <bool NOISE>
__global__ void __launch_bounds__(kLanes) lidar_kernel(LidarArgs a) {
  __shared__ float sh_pose[PGTT_NBODY][8];                              // xpos[3], xquat[4]
  __shared__ __attribute__((aligned(16))) float sh_box[PGTT_MAX_BOX * kBoxWords];
  __shared__ __attribute__((aligned(16))) float sh_geom[PGTT_RENDER_MAX_GEOM * kGeomWords];
  __shared__ int sh_nbox[kWaves], sh_ngeom;
  const long long tick = a.counter[0];
  if (!a.force && (unsigned long long)tick % (unsigned)a.every != 0) return;       // the same decision in every workgroup
  const int e = blockIdx.x, tid = threadIdx.x, N = a.N;
  const int lane = tid & 63, wave = tid >> 6;

  // ---- phase A: kinematics (lanes 0..3: the base, then one leg each)
  const bool chain = a.mount_body != 0 || a.ngeom > 0;
  if (tid < PGTT_NLEG) {
    auto row = [&](int r) { return a.state[(size_t)r * N + e]; };
    const PgttModel* m = a.model;
    // this kernel's own statement of the chain, like the placement and the hit tests: see pgtt_raycast.hip.h
    V3 xp = v3(row(PGTT_S_QPOS + 0), row(PGTT_S_QPOS + 1), row(PGTT_S_QPOS + 2));
    Q4 xq;
    {
      const Q4 q = {row(PGTT_S_QPOS + 3), row(PGTT_S_QPOS + 4), row(PGTT_S_QPOS + 5), row(PGTT_S_QPOS + 6)};
      const float n = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
      xq = {q.w / n, q.x / n, q.y / n, q.z / n};
    }
    if (tid == 0) {
      sh_pose[0][0] = xp.x; sh_pose[0][1] = xp.y; sh_pose[0][2] = xp.z;
      sh_pose[0][3] = xq.w; sh_pose[0][4] = xq.x; sh_pose[0][5] = xq.y; sh_pose[0][6] = xq.z;
    }
    if (chain) {
      for (int k = 0; k < 3; k++) {                                     // hip, thigh, calf: each the child of the one before
        const int b = 1 + 3 * tid + k;
        xp = xp + qrot(xq, ld3(m->body_pos[b]));
        const Q4 quat = qmul(xq, Q4{m->body_quat[b][0], m->body_quat[b][1], m->body_quat[b][2], m->body_quat[b][3]});
        const float q0 = a.params ? a.params[(size_t)(PGTT_P_QPOS0 + b - 1) * N + e] : m->qpos0[7 + b - 1];
        const float ang = row(PGTT_S_QPOS + 7 + b - 1) - q0;
        float s, c; sincosf(0.5f * ang, &s, &c);
        xq = qmul(quat, Q4{c, m->jnt_axis[b - 1][0] * s, m->jnt_axis[b - 1][1] * s, m->jnt_axis[b - 1][2] * s});
        sh_pose[b][0] = xp.x; sh_pose[b][1] = xp.y; sh_pose[b][2] = xp.z;
        sh_pose[b][3] = xq.w; sh_pose[b][4] = xq.x; sh_pose[b][5] = xq.y; sh_pose[b][6] = xq.z;
      }
    }
  }
  __syncthreads();

  // ---- the sensor: body pose * mount pose
  Sensor sen;
  {
    const float* bp = sh_pose[a.mount_body];
    const Q4 bq = {bp[3], bp[4], bp[5], bp[6]};
    sen.o = ld3(bp) + qrot(bq, v3(a.mpos[0], a.mpos[1], a.mpos[2]));
    qaxes(qmul(bq, Q4{a.mquat[0], a.mquat[1], a.mquat[2], a.mquat[3]}), sen.ax, sen.ay, sen.az);
  }

  // ---- boxes of the env's variant -> sensor frame, culled, compacted in box order
  int nbox = 0, ngeom = 0;
  if (a.T > 0 || a.ngeom > 0) {                                          // the flat task without the robot: the plane alone, no list at all
    float rec[kBoxWords];
    bool keep = false;
    if (a.T > 0 && tid < a.B) {
      const int v = a.variant ? min(max(a.variant[e], 0), a.T - 1) : 0;
      const float4* src = reinterpret_cast<const float4*>(a.boxes + ((size_t)v * a.B + tid) * kTabWords);
      float w[kTabWords];
#pragma unroll
      for (int i = 0; i < kTabWords / 4; i++) { const float4 q = src[i]; w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w; }
      const V3 c = to_sensor(sen, ld3(w) - sen.o);
      const V3 h = ld3(w + 12);
      keep = sphere_in_reach(c, sqrtf(dot(h, h)), a.far_m);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const V3 r = to_sensor(sen, ld3(w + 3 + 3 * k));
        rec[3 + 3 * k] = r.x; rec[4 + 3 * k] = r.y; rec[5 + 3 * k] = r.z;
        rec[k] = -dot(r, c);                                             // the ray origin (the sensor) in the box frame
      }
      rec[12] = h.x; rec[13] = h.y; rec[14] = h.z; rec[15] = 0.f;
    }
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) sh_nbox[wave] = __popcll(kept);

    // ---- robot geoms (wave 0): posed, culled and compacted the same way
    if (wave == 0 && a.ngeom > 0) {
      float grec[kGeomWords];
      bool gkeep = false;
      if (tid < a.ngeom) {
        const PgttRenderGeom G = a.geoms[tid];
        const int b = min(max(G.body, 0), PGTT_NBODY - 1);
        const Q4 bq = {sh_pose[b][3], sh_pose[b][4], sh_pose[b][5], sh_pose[b][6]};
        const V3 c = to_sensor(sen, ld3(sh_pose[b]) + qrot(bq, ld3(G.pos)) - sen.o);
        V3 r[3]; qaxes(qmul(bq, Q4{G.quat[0], G.quat[1], G.quat[2], G.quat[3]}), r[0], r[1], r[2]);
        grec[0] = c.x; grec[1] = c.y; grec[2] = c.z;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const V3 rc = to_sensor(sen, r[k]);
          grec[3 + 3 * k] = rc.x; grec[4 + 3 * k] = rc.y; grec[5 + 3 * k] = rc.z;
        }
        grec[12] = G.size[0]; grec[13] = G.size[1]; grec[14] = G.size[2]; grec[15] = __int_as_float(G.type);
        const float rb = G.type == PGTT_RENDER_SPHERE ? G.size[0]
                         : (G.type == PGTT_RENDER_CAPSULE ? G.size[0] + G.size[1] : sqrtf(dot(ld3(G.size), ld3(G.size))));
        gkeep = sphere_in_reach(c, rb, a.far_m);
      }
      const unsigned long long gk = __ballot(gkeep);
      if (lane == 0) sh_ngeom = __popcll(gk);
      if (gkeep) {
        float* dst = sh_geom + __popcll(gk & ((1ull << lane) - 1ull)) * kGeomWords;
#pragma unroll
        for (int i = 0; i < kGeomWords; i++) dst[i] = grec[i];
      }
    }
    __syncthreads();
    int first = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) { first += w < wave ? sh_nbox[w] : 0; nbox += sh_nbox[w]; }
    if (a.ngeom > 0) ngeom = sh_ngeom;
    if (keep) {
      float4* dst = reinterpret_cast<float4*>(sh_box + (first + __popcll(kept & ((1ull << lane) - 1ull))) * kBoxWords);
#pragma unroll
      for (int i = 0; i < kBoxWords / 4; i++) dst[i] = make_float4(rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]);
    }
    __syncthreads();
  }

  // ---- phase B: rays over lanes
  const V3 pn = v3(sen.ax.z, sen.ay.z, sen.az.z);                       // the plane's normal (world +z) in the sensor frame
  const int R = a.R;
  float* out = a.range + (size_t)e * R;
  float* pts = a.points ? a.points + (size_t)e * R * 3 : nullptr;
  for (int r = tid; r < R; r += kLanes) {
    const float4 dv = a.dirs[r];
    const V3 d = v3(dv.x, dv.y, dv.z);
    float best = INFINITY;
    {
      const float den = dot(pn, d);
      if (den != 0.f) {
        const float t = -sen.o.z / den;
        if (t > 0.f) best = t;
      }
    }
    for (int k = 0; k < nbox; k++) best = fminf(best, hit_box(sh_box + k * kBoxWords, d));
    for (int g = 0; g < ngeom; g++) {
      const float* G = sh_geom + g * kGeomWords;
      const int type = __float_as_int(G[15]);
      const V3 c = ld3(G);
      float t;
      if (type == PGTT_RENDER_SPHERE) t = hit_sphere(-1.f * c, d, G[12]);
      else if (type == PGTT_RENDER_CAPSULE) t = hit_capsule(d, c, ld3(G + 9), G[12], G[13]);
      else {
        float rb[kBoxWords];
#pragma unroll
        for (int i = 3; i < 15; i++) rb[i] = G[i];
#pragma unroll
        for (int i = 0; i < 3; i++) rb[i] = -dot(ld3(G + 3 + 3 * i), c);
        t = hit_box(rb, d);
      }
      best = fminf(best, t);
    }
    float val = fminf(fmaxf(best, a.near_m), a.far_m);
    if (NOISE) val = noisy(val, a.seed, a.env_off, e, tick, PGTT_RS_LIDAR, r, a.sigma, a.dropout, a.near_m, a.far_m);
    out[r] = val;
    if (pts) {
      const float nanv = __uint_as_float(0x7fc00000u);
      V3 p = v3(nanv, nanv, nanv);
      if (val > a.near_m && val < a.far_m) p = sen.o + val * (d.x * sen.ax + d.y * sen.ay + d.z * sen.az);
      float* dst = pts + 3 * (size_t)r;
      dst[0] = p.x; dst[1] = p.y; dst[2] = p.z;
    }
  }
}

// the checks of the config and of the pattern; `who` prefixes the message
int resolve(const PgttLidarConfig* cfg, const float* dirs, int R, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (!cfg) return fail(PGTT_E_ARG, p + "null config");
  if (int rc = check_sensor_config(cfg, who)) return rc;
  if (R < 1 || R > PGTT_LIDAR_MAX_RAYS) return fail(PGTT_E_ARG, p + "R must be in [1, PGTT_LIDAR_MAX_RAYS]");
  if (!dirs) return fail(PGTT_E_ARG, p + "null pattern");
  for (int r = 0; r < R; r++) {
    double n = 0.0;
    for (int i = 0; i < 3; i++) n += (double)dirs[3 * r + i] * dirs[3 * r + i];
    if (!(n > 0.0) || !std::isfinite(n)) return fail(PGTT_E_ARG, p + "pattern row " + std::to_string(r) + " is zero or not finite");
  }
  return PGTT_OK;
}

}  // namespace

struct pgtt_lidar_scanner {
  int num_envs = 0;
  int ngeom = 0;
  int R = 0;
  PgttLidarConfig cfg{};
  PgttLidarBuffers buf{};
  bool bound = false;
  float4* d_dirs = nullptr;
  SceneTables scene;
};

extern "C" {

PGTT_SIDE_EXPORTS(lidar, LIDAR)
int pgtt_lidar_sizeof_config(void) { return (int)sizeof(PgttLidarConfig); }
int pgtt_lidar_sizeof_buffers(void) { return (int)sizeof(PgttLidarBuffers); }

int pgtt_lidar_check(const PgttLidarConfig* cfg, const float* dirs, int R) { return resolve(cfg, dirs, R, "pgtt_lidar_check"); }

int pgtt_lidar_create(const PgttModel* model, const PgttLidarConfig* cfg, const float* dirs, int R, const PgttRenderGeom* geoms, int ngeom,
                      int device, int num_envs, pgtt_lidar_handle* out) {
  if (!model || !cfg || !out || (ngeom > 0 && !geoms)) return fail(PGTT_E_ARG, "pgtt_lidar_create: null argument");
  *out = nullptr;
  if (num_envs < 1) return fail(PGTT_E_ARG, "pgtt_lidar_create: num_envs must be >= 1");
  if (int rc = resolve(cfg, dirs, R, "pgtt_lidar_create")) return rc;
  if (int rc = check_geoms(geoms, ngeom, "pgtt_lidar_create")) return rc;
  if (int rc = check_device(device, "pgtt_lidar_create")) return rc;
  pgtt_lidar_scanner* h = new pgtt_lidar_scanner();
  h->num_envs = num_envs; h->ngeom = ngeom; h->R = R; h->cfg = with_unit_mount(*cfg); h->scene.device = device;
  // the pattern: unit rows (normalised in double), padded to 16 bytes
  std::vector<float> tab((size_t)R * 4, 0.f);
  for (int r = 0; r < R; r++) {
    const double x = dirs[3 * r], y = dirs[3 * r + 1], z = dirs[3 * r + 2], n = std::sqrt(x * x + y * y + z * z);
    tab[4 * r] = (float)(x / n); tab[4 * r + 1] = (float)(y / n); tab[4 * r + 2] = (float)(z / n);
  }
  auto upload = [&]() -> int {
    if (int rc = h->scene.upload(model, geoms, ngeom)) return rc;
    HIP_TRY(hipMalloc(&h->d_dirs, tab.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(h->d_dirs, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    return PGTT_OK;
  };
  if (int rc = upload()) { pgtt_lidar_destroy(h); return rc; }
  *out = h;
  return PGTT_OK;
}

int pgtt_lidar_destroy(pgtt_lidar_handle h) {
  if (!h) return PGTT_OK;
  h->scene.release();
  if (h->d_dirs) hipFree(h->d_dirs);
  delete h;
  return PGTT_OK;
}

int pgtt_lidar_set_terrain(pgtt_lidar_handle h, const float* boxes, int T, int B) {
  if (!h) return fail(PGTT_E_ARG, "null handle");
  return h->scene.set_terrain(boxes, T, B, "pgtt_lidar_set_terrain");
}

int pgtt_lidar_bind(pgtt_lidar_handle h, const PgttLidarBuffers* bufs) {
  if (!h || !bufs) return fail(PGTT_E_ARG, "pgtt_lidar_bind: null argument");
  if (!bufs->state || !bufs->range || !bufs->counter) return fail(PGTT_E_ARG, "pgtt_lidar_bind: state, range and counter are required");
  h->buf = *bufs;
  h->bound = true;
  return PGTT_OK;
}

int pgtt_lidar(pgtt_lidar_handle h, int force, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_lidar: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_lidar: no buffers bound (pgtt_lidar_bind first)");
  HIP_TRY(hipSetDevice(h->scene.device));
  LidarArgs a{};
  fill_sensor_args(a, h->cfg, h->buf, h->scene, h->num_envs, h->ngeom, force);
  a.range = h->buf.range; a.points = h->buf.points; a.dirs = h->d_dirs; a.R = h->R;
  return launch_sensor_tick(lidar_kernel<true>, lidar_kernel<false>, a, (hipStream_t)stream);
}

}  // extern "C"
