// pgtt_depth.hip — libpgtt_depth.so: the onboard depth camera (include/pgtt_depth.h), one workgroup per env.
//
// depth_kernel, 256 lanes per env:
//   phase A  lanes 0..3 run the forward kinematics of one leg each (the formulas of mjcf.kinematics_np; only when the mount is not on the
//            torso or the robot is in the scene); every lane then forms the camera basis from the mount body's pose.
//            Lane b < B moves box b of the env's variant into the CAMERA frame (x right, y up, z along the optical axis; the ray origin is
//            the frame's origin) and tests its bounding sphere against the cone around the view frustum and against `far`.  Survivors are
//            compacted into LDS in box order with a ballot and prefix counts: no atomics, so the list is deterministic.  The posed robot
//            geoms go the same way.
//   phase B  pixels over lanes, 256 per pass.  The ray of pixel (i, j) in the camera frame is (u, v, 1) for every env; with that
//            un-normalised direction the slab parameter of a box IS the distance along the optical axis, and a record holds all that the
//            slab test needs (the origin in the box frame, the box's axes, the half extents).  Every lane walks the same list (LDS
//            broadcasts, wave-uniform trip count), takes the minimum with the plane, clamps, adds the noise and stores coalesced.
// A tick that the sensor period skips returns at once in every workgroup (the decision reads counter[0] on the device); sensor_advance_kernel,
// enqueued behind it, adds one to the counter.  Nothing is shared between envs: an env's image does not depend on the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pgtt_depth.h"
#include "pgtt_sensor.hip.h"

// experiment build (pgtt_side.mk, EXTRA=-DPGTT_DEPTH_NOCULL): every box and geom is kept; the figure DESIGN.md 14 compares against
#ifdef PGTT_DEPTH_NOCULL
#define PGTT_DEPTH_FLAVOR "nocull"
#endif

namespace {

struct DepthArgs {
  const float* state;
  const float* params;
  const int32_t* variant;
  float* depth;
  int64_t* counter;
  const float* boxes;                   // [T][B][kTabWords]
  const PgttModel* model;
  const PgttRenderGeom* geoms;
  int N, T, B, ngeom;                   // ngeom = 0 when the robot is not in the scene
  int W, H, mount_body, every, force;
  float tan_y, near_m, far_m;
  float mpos[3], mquat[4];
  float sigma, dropout;
  unsigned long long seed;
  long long env_off;
};

// the camera: world vector -> camera frame (x right, y up, z forward)
struct Cam { V3 o, right, up, fwd; };
__device__ __forceinline__ V3 to_cam(const Cam& c, V3 w) { return v3(dot(c.right, w), dot(c.up, w), dot(c.fwd, w)); }

// May a ray of the frustum, out to depth far_m, touch the sphere (centre c in the camera frame, radius r)?  Conservative: the frustum lies inside
// the cone of half angle atan(tan_c) about +z (tan_c = the corner ray's slope; sin_c, cos_c of that angle); for a centre at angle phi > the cone's
// from the axis, |c| sin(phi - cone) = rho cos - z sin is a lower bound of its distance to the cone.  A hit deeper than far_m reads far_m like a miss.
// The slack covers the fp32 rounding of the centre and of the test itself.
__device__ __forceinline__ bool sphere_in_view(V3 c, float r, float sin_c, float cos_c, float far_m) {
#ifdef PGTT_DEPTH_NOCULL
  return true;
#else
  const float rho = sqrtf(c.x * c.x + c.y * c.y);
  const float slack = 1e-3f * r + 1e-5f * (1.f + rho + fabsf(c.z));
  return rho * cos_c - c.z * sin_c <= r + slack && c.z - r <= far_m + slack;
#endif
}

// slab test of the ray t * (u, v, 1) against a box record (origin in the box frame, axes, half extents): t of the entry = depth along the axis
// (a ray that starts inside the box does not see it)
__device__ __forceinline__ float hit_box(const float* __restrict__ r, float u, float v) {
  float tn = -INFINITY, tf = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float dl = r[3 + 3 * k] * u + r[4 + 3 * k] * v + r[5 + 3 * k];
    const float inv = __builtin_amdgcn_rcpf(dl), ol = r[k], h = r[12 + k];
    const float t1 = (-h - ol) * inv, t2 = (h - ol) * inv;
    tn = fmaxf(tn, fminf(t1, t2));
    tf = fminf(tf, fmaxf(t1, t2));
  }
  return (tn <= tf && tn > 0.f) ? tn : INFINITY;
}

template <bool NOISE>
__global__ void __launch_bounds__(kLanes) depth_kernel(DepthArgs a) {
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

  // ---- the camera: body pose * mount pose; fwd = +x, up = +z, right = fwd x up
  Cam cam;
  {
    const float* bp = sh_pose[a.mount_body];
    const Q4 bq = {bp[3], bp[4], bp[5], bp[6]};
    cam.o = ld3(bp) + qrot(bq, v3(a.mpos[0], a.mpos[1], a.mpos[2]));
    V3 c1;
    qaxes(qmul(bq, Q4{a.mquat[0], a.mquat[1], a.mquat[2], a.mquat[3]}), cam.fwd, c1, cam.up);
    cam.right = cross(cam.fwd, cam.up);
  }
  const float tan_x = a.tan_y * ((float)a.W / (float)a.H);
  const float tan_c = sqrtf(tan_x * tan_x + a.tan_y * a.tan_y);
  const float cos_c = 1.f / sqrtf(1.f + tan_c * tan_c), sin_c = tan_c * cos_c;

  // ---- boxes of the env's variant -> camera frame, culled, compacted in box order
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
      const V3 c = to_cam(cam, ld3(w) - cam.o);
      const V3 h = ld3(w + 12);
      keep = sphere_in_view(c, sqrtf(dot(h, h)), sin_c, cos_c, a.far_m);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const V3 r = to_cam(cam, ld3(w + 3 + 3 * k));
        rec[3 + 3 * k] = r.x; rec[4 + 3 * k] = r.y; rec[5 + 3 * k] = r.z;
        rec[k] = -dot(r, c);                                             // the ray origin (the camera) in the box frame
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
        const V3 c = to_cam(cam, ld3(sh_pose[b]) + qrot(bq, ld3(G.pos)) - cam.o);
        V3 r[3]; qaxes(qmul(bq, Q4{G.quat[0], G.quat[1], G.quat[2], G.quat[3]}), r[0], r[1], r[2]);
        grec[0] = c.x; grec[1] = c.y; grec[2] = c.z;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const V3 rc = to_cam(cam, r[k]);
          grec[3 + 3 * k] = rc.x; grec[4 + 3 * k] = rc.y; grec[5 + 3 * k] = rc.z;
        }
        grec[12] = G.size[0]; grec[13] = G.size[1]; grec[14] = G.size[2]; grec[15] = __int_as_float(G.type);
        const float rb = G.type == PGTT_RENDER_SPHERE ? G.size[0]
                         : (G.type == PGTT_RENDER_CAPSULE ? G.size[0] + G.size[1] : sqrtf(dot(ld3(G.size), ld3(G.size))));
        gkeep = sphere_in_view(c, rb, sin_c, cos_c, a.far_m);
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

  // ---- phase B: pixels over lanes
  const V3 pn = v3(cam.right.z, cam.up.z, cam.fwd.z);                   // the plane's normal (world +z) in the camera frame
  const int npix = a.W * a.H;
  float* out = a.depth + (size_t)e * npix;
  for (int p = tid; p < npix; p += kLanes) {
    const int py = p / a.W, px = p - py * a.W;
    const float u = (2.f * ((float)px + 0.5f) / (float)a.W - 1.f) * tan_x;
    const float v = (1.f - 2.f * ((float)py + 0.5f) / (float)a.H) * a.tan_y;
    float best = INFINITY;
    {
      const float den = pn.x * u + pn.y * v + pn.z;
      if (den != 0.f) {
        const float t = -cam.o.z / den;
        if (t > 0.f) best = t;
      }
    }
    for (int k = 0; k < nbox; k++) best = fminf(best, hit_box(sh_box + k * kBoxWords, u, v));
    if (ngeom > 0) {
      const float dz = 1.f / sqrtf(u * u + v * v + 1.f);
      const V3 d = v3(u * dz, v * dz, dz);
      for (int g = 0; g < ngeom; g++) {
        const float* G = sh_geom + g * kGeomWords;
        const int type = __float_as_int(G[15]);
        const V3 c = ld3(G);
        float t;
        if (type == PGTT_RENDER_SPHERE) t = hit_sphere(-1.f * c, d, G[12]) * dz;
        else if (type == PGTT_RENDER_CAPSULE) t = hit_capsule(d, c, ld3(G + 9), G[12], G[13]) * dz;
        else {
          float r[kBoxWords];
#pragma unroll
          for (int i = 3; i < 15; i++) r[i] = G[i];
#pragma unroll
          for (int i = 0; i < 3; i++) r[i] = -dot(ld3(G + 3 + 3 * i), c);
          t = hit_box(r, u, v);
        }
        best = fminf(best, t);
      }
    }
    float val = fminf(fmaxf(best, a.near_m), a.far_m);
    if (NOISE) val = noisy(val, a.seed, a.env_off, e, tick, PGTT_RS_DEPTH, p, a.sigma, a.dropout, a.near_m, a.far_m);
    out[p] = val;
  }
}

}  // namespace

struct pgtt_depth_camera {
  int num_envs = 0;
  int ngeom = 0;
  PgttDepthConfig cfg{};
  PgttDepthBuffers buf{};
  bool bound = false;
  SceneTables scene;
};

extern "C" {

PGTT_SIDE_EXPORTS(depth, DEPTH)
int pgtt_depth_sizeof_config(void) { return (int)sizeof(PgttDepthConfig); }
int pgtt_depth_sizeof_buffers(void) { return (int)sizeof(PgttDepthBuffers); }

int pgtt_depth_create(const PgttModel* model, const PgttDepthConfig* cfg, const PgttRenderGeom* geoms, int ngeom, int device, int num_envs,
                      pgtt_depth_handle* out) {
  if (!model || !cfg || !out || (ngeom > 0 && !geoms)) return fail(PGTT_E_ARG, "pgtt_depth_create: null argument");
  *out = nullptr;
  if (num_envs < 1) return fail(PGTT_E_ARG, "pgtt_depth_create: num_envs must be >= 1");
  if (cfg->width < 1 || cfg->width > PGTT_DEPTH_MAX_DIM || cfg->height < 1 || cfg->height > PGTT_DEPTH_MAX_DIM)
    return fail(PGTT_E_ARG, "pgtt_depth_create: width and height must be in [1, PGTT_DEPTH_MAX_DIM]");
  if (!(cfg->fovy_deg > 0.f) || !(cfg->fovy_deg < 180.f)) return fail(PGTT_E_ARG, "pgtt_depth_create: fovy must be in (0, 180) degrees");
  if (int rc = check_sensor_config(cfg, "pgtt_depth_create")) return rc;
  if (int rc = check_geoms(geoms, ngeom, "pgtt_depth_create")) return rc;
  if (int rc = check_device(device, "pgtt_depth_create")) return rc;
  pgtt_depth_camera* h = new pgtt_depth_camera();
  h->num_envs = num_envs; h->ngeom = ngeom; h->cfg = with_unit_mount(*cfg); h->scene.device = device;
  if (int rc = h->scene.upload(model, geoms, ngeom)) { pgtt_depth_destroy(h); return rc; }
  *out = h;
  return PGTT_OK;
}

int pgtt_depth_destroy(pgtt_depth_handle h) {
  if (!h) return PGTT_OK;
  h->scene.release();
  delete h;
  return PGTT_OK;
}

int pgtt_depth_set_terrain(pgtt_depth_handle h, const float* boxes, int T, int B) {
  if (!h) return fail(PGTT_E_ARG, "null handle");
  return h->scene.set_terrain(boxes, T, B, "pgtt_depth_set_terrain");
}

int pgtt_depth_bind(pgtt_depth_handle h, const PgttDepthBuffers* bufs) {
  if (!h || !bufs) return fail(PGTT_E_ARG, "pgtt_depth_bind: null argument");
  if (!bufs->state || !bufs->depth || !bufs->counter) return fail(PGTT_E_ARG, "pgtt_depth_bind: state, depth and counter are required");
  h->buf = *bufs;
  h->bound = true;
  return PGTT_OK;
}

int pgtt_depth(pgtt_depth_handle h, int force, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_depth: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_depth: no buffers bound (pgtt_depth_bind first)");
  HIP_TRY(hipSetDevice(h->scene.device));
  const PgttDepthConfig& c = h->cfg;
  DepthArgs a{};
  fill_sensor_args(a, c, h->buf, h->scene, h->num_envs, h->ngeom, force);
  a.depth = h->buf.depth; a.W = c.width; a.H = c.height;
  a.tan_y = (float)std::tan(0.5 * (double)c.fovy_deg * 3.14159265358979323846 / 180.0);
  return launch_sensor_tick(depth_kernel<true>, depth_kernel<false>, a, (hipStream_t)stream);
}

}  // extern "C"
