// pgtt_render.hip — libpgtt_render.so: batched brute-force ray casting of env frames (include/pgtt_render.h).
//
// Two kernels per call, both on the caller's stream:
//   render_setup_kernel : one workgroup per view.  Lane 0 runs the forward kinematics of the 13 bodies from the env's qpos (the formulas
//                         of mjcf.kinematics_np) and builds the camera basis; lanes g < ngeom then place the robot primitives.  The result
//                         is one ViewRec per view in the caller's workspace.
//   render_pixel_kernel : grid (16x16 pixel tiles, views).  The prologue stages the view record, the env's terrain variant (ray-ready boxes)
//                         and the view's markers into LDS; every lane then walks the same primitive list (wave-uniform bounds, LDS
//                         broadcasts), takes the closest hit, casts one shadow ray toward the light and stores one packed RGBA dword.
//                         pgtt_render() launches render_pixel_kernel<false>.  pgtt_render_map() launches render_pixel_kernel<true, MapArgs>
//                         behind the same setup kernel: it also stages the env's window of elevation heights and walks the cell columns
//                         a ray crosses (hit_columns).
// Nothing is shared between views and nothing is atomic, so a view renders to the same bits whatever else is in the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/pgtt_render.h"
#include "pgtt_raycast.hip.h"
#include "pgtt_raycast_host.h"

namespace {

constexpr int kTile = 16;               // pixel tile edge: 256 lanes per workgroup
constexpr int kChunk = 64;              // views per setup launch (their cameras travel as launch arguments)
constexpr int kBoxWords = kTabWords;    // ray-ready box (pgtt_raycast_host.h): centre[3], local axes in world coordinates r0[3] r1[3] r2[3], half extents[3], pad
constexpr int kGeomWords = 20;          // placed geom: centre[3], local axes r0 r1 r2 [9], size[3], rgb[3], type, pad
constexpr int kHeadWords = 16;          // camera pos[3] fwd[3] right[3] up[3], tan(fovy / 2), env, variant, pad
constexpr int kViewWords = kHeadWords + PGTT_RENDER_MAX_GEOM * kGeomWords;

struct ViewArg {
  int32_t env;
  PgttRenderCamera cam;
};
struct SetupChunk {
  ViewArg v[kChunk];
};

// ---------------------------------------------------------------- setup: kinematics, camera, placed geoms
__global__ void __launch_bounds__(64) render_setup_kernel(SetupChunk chunk, int first_view, const float* __restrict__ state, const float* __restrict__ params,
                                                          const int32_t* __restrict__ variant, int N, int T, const PgttModel* __restrict__ m,
                                                          const PgttRenderGeom* __restrict__ geoms, int ngeom, float* __restrict__ ws,
                                                          float* __restrict__ body_pose) {
  __shared__ float sh_pose[PGTT_NBODY][8];      // xpos[3], xquat[4]
  const int lv = blockIdx.x, vi = first_view + lv;
  float* rec = ws + (size_t)vi * kViewWords;
  if (threadIdx.x == 0) {
    const int e = chunk.v[lv].env;
    const PgttRenderCamera cam = chunk.v[lv].cam;
    auto row = [&](int r) { return state[(size_t)r * N + e]; };
    // the body chain, serially on this lane (this kernel's own statement, like the placement and the hit tests below: see pgtt_raycast.hip.h)
    V3 xpos[PGTT_NBODY]; Q4 xq[PGTT_NBODY];
    xpos[0] = v3(row(PGTT_S_QPOS + 0), row(PGTT_S_QPOS + 1), row(PGTT_S_QPOS + 2));
    {
      Q4 q = {row(PGTT_S_QPOS + 3), row(PGTT_S_QPOS + 4), row(PGTT_S_QPOS + 5), row(PGTT_S_QPOS + 6)};
      const float n = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
      xq[0] = {q.w / n, q.x / n, q.y / n, q.z / n};
    }
#pragma unroll
    for (int b = 1; b < PGTT_NBODY; b++) {
      const int k = (b - 1) % 3, parent = k == 0 ? 0 : b - 1;
      const V3 pos = xpos[parent] + qrot(xq[parent], ld3(m->body_pos[b]));
      const Q4 quat = qmul(xq[parent], Q4{m->body_quat[b][0], m->body_quat[b][1], m->body_quat[b][2], m->body_quat[b][3]});
      const float q0 = params ? params[(size_t)(PGTT_P_QPOS0 + b - 1) * N + e] : m->qpos0[7 + b - 1];
      const float ang = row(PGTT_S_QPOS + 7 + b - 1) - q0;
      float s, c; sincosf(0.5f * ang, &s, &c);
      xq[b] = qmul(quat, Q4{c, m->jnt_axis[b - 1][0] * s, m->jnt_axis[b - 1][1] * s, m->jnt_axis[b - 1][2] * s});
      xpos[b] = pos;
    }
#pragma unroll
    for (int b = 0; b < PGTT_NBODY; b++) {
      sh_pose[b][0] = xpos[b].x; sh_pose[b][1] = xpos[b].y; sh_pose[b][2] = xpos[b].z;
      sh_pose[b][3] = xq[b].w; sh_pose[b][4] = xq[b].x; sh_pose[b][5] = xq[b].y; sh_pose[b][6] = xq[b].z;
    }
    // camera (MuJoCo free camera): fwd = (cos el cos az, cos el sin az, sin el), up = (-sin el cos az, -sin el sin az, cos el), right = fwd x up
    const float deg = 3.14159265358979323846f / 180.f;
    float az = cam.azimuth_deg;
    V3 look = ld3(cam.target);
    if (cam.mode != PGTT_CAM_FIXED) look = look + xpos[0];
    if (cam.mode == PGTT_CAM_TRACK_YAW) {
      const Q4 q = xq[0];
      az += atan2f(2.f * (q.w * q.z + q.x * q.y), 1.f - 2.f * (q.y * q.y + q.z * q.z)) / deg;
    }
    float sa, ca, se, ce;
    sincosf(az * deg, &sa, &ca); sincosf(cam.elevation_deg * deg, &se, &ce);
    const V3 fwd = v3(ce * ca, ce * sa, se), up = v3(-se * ca, -se * sa, ce), right = cross(fwd, up);
    const V3 pos = look - cam.distance * fwd;
    const float hd[kHeadWords] = {pos.x, pos.y, pos.z, fwd.x, fwd.y, fwd.z, right.x, right.y, right.z, up.x, up.y, up.z,
                                  tanf(0.5f * cam.fovy_deg * deg), __int_as_float(e),
                                  __int_as_float((T > 0 && variant) ? min(max(variant[e], 0), T - 1) : 0), 0.f};
#pragma unroll
    for (int i = 0; i < kHeadWords; i++) rec[i] = hd[i];
  }
  __syncthreads();
  if (body_pose)
    for (int i = threadIdx.x; i < PGTT_NBODY * 7; i += blockDim.x) body_pose[(size_t)vi * PGTT_NBODY * 7 + i] = sh_pose[i / 7][i % 7];
  const int g = threadIdx.x;
  if (g < ngeom) {
    const PgttRenderGeom G = geoms[g];
    const int b = min(max(G.body, 0), PGTT_NBODY - 1);
    const V3 bp = v3(sh_pose[b][0], sh_pose[b][1], sh_pose[b][2]);
    const Q4 bq = {sh_pose[b][3], sh_pose[b][4], sh_pose[b][5], sh_pose[b][6]};
    const V3 c = bp + qrot(bq, ld3(G.pos));
    V3 r0, r1, r2; qaxes(qmul(bq, Q4{G.quat[0], G.quat[1], G.quat[2], G.quat[3]}), r0, r1, r2);
    const float gw[kGeomWords] = {c.x, c.y, c.z, r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r2.x, r2.y, r2.z,
                                  G.size[0], G.size[1], G.size[2], G.rgb[0], G.rgb[1], G.rgb[2], __int_as_float(G.type), 0.f};
    float* dst = rec + kHeadWords + g * kGeomWords;
#pragma unroll
    for (int i = 0; i < kGeomWords; i++) dst[i] = gw[i];
  }
}

// ---------------------------------------------------------------- primitives (ray o + t d, |d| = 1; a hit needs t > 0)
// oriented box: slab test in the box frame; t = entry distance (a ray that starts inside the box does not see it)
__device__ __forceinline__ float hit_box(V3 o, V3 d, const float* __restrict__ bx, int& axis, float& sgn) {
  const V3 rel = o - ld3(bx);
  const V3 r0 = ld3(bx + 3), r1 = ld3(bx + 6), r2 = ld3(bx + 9);
  const float ol[3] = {dot(r0, rel), dot(r1, rel), dot(r2, rel)};
  const float dl[3] = {dot(r0, d), dot(r1, d), dot(r2, d)};
  float tn = -INFINITY, tf = INFINITY;
  axis = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float inv = 1.f / dl[a], h = bx[12 + a];
    const float t1 = (-h - ol[a]) * inv, t2 = (h - ol[a]) * inv;
    const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
    if (lo > tn) { tn = lo; axis = a; }
    tf = fminf(tf, hi);
  }
  sgn = dl[axis] < 0.f ? 1.f : -1.f;
  return (tn <= tf && tn > 0.f) ? tn : INFINITY;
}
__device__ __forceinline__ float hit_sphere(V3 o, V3 d, V3 c, float r) {
  const V3 oc = o - c;
  const float b = dot(oc, d), cc = dot(oc, oc) - r * r, disc = b * b - cc;
  if (disc < 0.f) return INFINITY;
  const float t = -b - sqrtf(disc);
  return t > 0.f ? t : INFINITY;
}
// capsule: segment c +- hl * ax, radius r (cylinder body, then the nearer end cap).  The cylinder's quadratic in its cross-product form;
// a <= 1e-12 baba, decided before h: the ray runs along the axis (see pgtt_raycast.hip.h)
__device__ __forceinline__ float hit_capsule(V3 o, V3 d, V3 c, V3 ax, float r, float hl) {
  const V3 pa = c - hl * ax, ba = (2.f * hl) * ax, oa = o - pa;
  const V3 bd = cross(ba, d), bo = cross(ba, oa);
  const float baba = dot(ba, ba), bard = dot(ba, d), baoa = dot(ba, oa);
  const float a = dot(bd, bd), b = dot(bd, bo), cc = dot(bo, bo) - r * r * baba;
  if (!(a > 1e-12f * baba)) return fminf(hit_sphere(o, d, pa, r), hit_sphere(o, d, pa + ba, r));
  const float h = b * b - a * cc;
  if (h < 0.f) return INFINITY;
  const float t = (-b - sqrtf(h)) / a, y = baoa + t * bard;
  if (y > 0.f && y < baba) return t > 0.f ? t : INFINITY;
  return hit_sphere(o, d, y <= 0.f ? pa : pa + ba, r);
}
__device__ __forceinline__ V3 capsule_normal(V3 p, V3 c, V3 ax, float r, float hl) {
  const float s = fminf(fmaxf(dot(p - c, ax), -hl), hl);
  return (1.f / r) * (p - (c + s * ax));
}
__device__ __forceinline__ float hit_geom(V3 o, V3 d, const float* __restrict__ g) {
  const int type = __float_as_int(g[18]);
  if (type == PGTT_RENDER_SPHERE) return hit_sphere(o, d, ld3(g), g[12]);
  if (type == PGTT_RENDER_CAPSULE) return hit_capsule(o, d, ld3(g), ld3(g + 9), g[12], g[13]);
  float bx[kBoxWords];
#pragma unroll
  for (int i = 0; i < 15; i++) bx[i] = g[i];
  int axis; float sgn;
  return hit_box(o, d, bx, axis, sgn);
}

// ---------------------------------------------------------------- the columns of a map call (include/pgtt_render.h, "Scene of a map call")
struct MapArgs {
  const float* map;
  const int32_t* origin;
  const float* tint;
  int G;
  float res, floor_z, lift, tint_lo, tint_hi;
  int terrain;
};

// Nearest column along the ray ol + t d, ol in WINDOW-LOCAL coordinates (cell (a, b) spans [a res, (a + 1) res] x [b res, (b + 1) res]; the
// window's corner lo res is subtracted once per lane, so the rounding of a far-away window is paid once and not per cell).  hm is the window of
// heights in window order, [G][G].  The ray is clipped to the window's box [0, G res]^2 x [floor_z, inf) and to t_stop (the best hit among the
// other primitives), then walks the cells it crosses in order - a 2-D grid traversal, at most 2 G - 1 cells - and tests each column with the slab
// rule in z against the cell's own xy crossing [t_in, t_out]: the first hit is the nearest.  The next border crossing is formed from the integer
// cell index at every step (one multiply and one fused multiply-add per axis), not summed up from a tDelta, so that its rounding does not grow
// with the number of steps either.  A direction component of magnitude below 1e-30 is a ray parallel to that axis: it crosses no border of it,
// and no division by it decides anything.  -> t (INFINITY: none), cell = a G + b, axis = the face's axis.
__device__ __forceinline__ float hit_columns(const float* __restrict__ hm, int G, float res, float floor_z, float lift, V3 ol, V3 d, float t_stop,
                                             int& cell, int& axis) {
  const float ext = (float)G * res;
  const bool mx = fabsf(d.x) > 1e-30f, my = fabsf(d.y) > 1e-30f, mz = fabsf(d.z) > 1e-30f;
  const float ivx = mx ? 1.f / d.x : 0.f, ivy = my ? 1.f / d.y : 0.f, ivz = mz ? 1.f / d.z : 0.f;
  float t0 = 0.f, t1 = t_stop;
  int ax = 2;                                    // the axis through which the ray entered the current cell; 2: it starts inside (or enters through the floor)
  if (mx) {
    const float ta = (0.f - ol.x) * ivx, tb = (ext - ol.x) * ivx;
    const float lo = fminf(ta, tb);
    if (lo > t0) { t0 = lo; ax = 0; }
    t1 = fminf(t1, fmaxf(ta, tb));
  } else if (ol.x < 0.f || ol.x > ext) return INFINITY;
  if (my) {
    const float ta = (0.f - ol.y) * ivy, tb = (ext - ol.y) * ivy;
    const float lo = fminf(ta, tb);
    if (lo > t0) { t0 = lo; ax = 1; }
    t1 = fminf(t1, fmaxf(ta, tb));
  } else if (ol.y < 0.f || ol.y > ext) return INFINITY;
  if (mz) {
    const float tf = (floor_z - ol.z) * ivz;
    if (d.z > 0.f) { if (tf > t0) { t0 = tf; ax = 2; } }
    else t1 = fminf(t1, tf);
  } else if (ol.z < floor_z) return INFINITY;
  if (!(t0 <= t1)) return INFINITY;
  const float inv_res = 1.f / res;
  int ix = min(max((int)floorf((ol.x + t0 * d.x) * inv_res), 0), G - 1);
  int iy = min(max((int)floorf((ol.y + t0 * d.y) * inv_res), 0), G - 1);
  const int sx = d.x > 0.f ? 1 : -1, sy = d.y > 0.f ? 1 : -1;
  const int fx = d.x > 0.f ? 1 : 0, fy = d.y > 0.f ? 1 : 0;
  float t_in = t0;
  for (int it = 0; it < 2 * G; it++) {
    const float tmx = mx ? ((float)(ix + fx) * res - ol.x) * ivx : INFINITY;
    const float tmy = my ? ((float)(iy + fy) * res - ol.y) * ivy : INFINITY;
    const float t_out = fminf(tmx, tmy);
    const float h = hm[ix * G + iy], top = h + lift;
    if (top > floor_z) {                         // false for NaN
      float lo, hi;
      if (mz) {
        const float ta = (floor_z - ol.z) * ivz, tb = (top - ol.z) * ivz;
        lo = fminf(ta, tb); hi = fmaxf(ta, tb);
      } else {
        lo = ol.z <= top ? -INFINITY : INFINITY; hi = INFINITY;
      }
      const float tn = fmaxf(t_in, lo), tf = fminf(t_out, hi);
      if (tn <= tf && tn > 0.f) {
        cell = ix * G + iy;
        axis = lo > t_in ? 2 : ax;
        return tn;
      }
    }
    if (t_out >= t1) break;                      // the next cell begins behind the window, behind the floor or behind a nearer primitive
    if (tmx < tmy) { ix += sx; ax = 0; if ((unsigned)ix >= (unsigned)G) break; }
    else { iy += sy; ax = 1; if ((unsigned)iy >= (unsigned)G) break; }
    t_in = t_out;
  }
  return INFINITY;
}

// ---------------------------------------------------------------- pixels
// One template for both pixel kernels.  <false> with an empty pack is pgtt_render()'s kernel: the same arguments and, instruction for instruction,
// the device code it had as a plain kernel (tools/side_isa_diff.py lists it under its new symbol; the bodies are equal).  <true, MapArgs> adds the
// map call's staging (the env's window of heights, un-toroidalised once into window order), the column walk behind the other primitives, the
// column's albedo (the tint layer is read from global memory once per pixel, at the hit cell) and the columns in the shadow ray.
// LDS of <true>: 2624 + 6400 + 2048 + 36864 = 47936 bytes, under the 64 KB a launch gets without an attribute.
__device__ __forceinline__ MapArgs map_args() { return MapArgs{}; }
__device__ __forceinline__ MapArgs map_args(MapArgs ma) { return ma; }

template <bool kMap, class... Map>
__global__ void __launch_bounds__(kTile * kTile) render_pixel_kernel(const float* __restrict__ ws, const float* __restrict__ boxes, int B,
                                                                     const float* __restrict__ markers, int M, int ngeom, int W, int H, int tiles_x,
                                                                     int shadows, uint32_t* __restrict__ rgba, float* __restrict__ depth,
                                                                     int32_t* __restrict__ seg, Map... map) {
  __shared__ float sh_view[kViewWords];
  __shared__ float sh_box[PGTT_MAX_BOX * kBoxWords];
  __shared__ float sh_mk[PGTT_RENDER_MAX_MARKER * 4];
  __shared__ float sh_map[kMap ? PGTT_RENDER_MAP_MAX_GRID * PGTT_RENDER_MAP_MAX_GRID : 1];
  const MapArgs ma = map_args(map...);
  const int vi = blockIdx.y, tid = threadIdx.x;
  const float* rec = ws + (size_t)vi * kViewWords;
  for (int i = tid; i < kHeadWords + ngeom * kGeomWords; i += blockDim.x) sh_view[i] = rec[i];
  if (B > 0) {
    const int v = __float_as_int(rec[14]);
    const float* src = boxes + (size_t)v * B * kBoxWords;
    for (int i = tid; i < B * kBoxWords; i += blockDim.x) sh_box[i] = src[i];
  }
  if (M > 0) {
    const float* src = markers + (size_t)vi * M * 4;
    for (int i = tid; i < M * 4; i += blockDim.x) sh_mk[i] = src[i];
  }
  // the map call: window cell (a, b) is world cell (lo + (a, b)) and lives at slot [(lo_x + a) mod G][(lo_y + b) mod G]
  int G = 0, slot_x0 = 0, slot_y0 = 0;
  size_t env_cells = 0;
  float win_x = 0.f, win_y = 0.f;
  if constexpr (kMap) {
    G = ma.G;
    const int e = __float_as_int(rec[13]);
    const int lim = 1 << 30;
    const int lo_x = min(max(ma.origin[2 * e], -lim), lim) - G / 2, lo_y = min(max(ma.origin[2 * e + 1], -lim), lim) - G / 2;
    slot_x0 = lo_x % G; if (slot_x0 < 0) slot_x0 += G;
    slot_y0 = lo_y % G; if (slot_y0 < 0) slot_y0 += G;
    env_cells = (size_t)e * G * G;
    win_x = (float)lo_x * ma.res; win_y = (float)lo_y * ma.res;
    const float* src = ma.map + env_cells;
    for (int i = tid; i < G * G; i += blockDim.x) {
      const int a = i / G, b = i - a * G;
      int sa = slot_x0 + a, sb = slot_y0 + b;
      if (sa >= G) sa -= G;
      if (sb >= G) sb -= G;
      sh_map[i] = src[sa * G + sb];
    }
  }
  __syncthreads();

  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int px = tx * kTile + (tid % kTile), py = ty * kTile + (tid / kTile);
  const V3 o = ld3(sh_view), fwd = ld3(sh_view + 3), right = ld3(sh_view + 6), up = ld3(sh_view + 9);
  const float tan_y = sh_view[12];
  const float u = (2.f * ((float)px + 0.5f) / (float)W - 1.f) * tan_y * ((float)W / (float)H);
  const float vv = (1.f - 2.f * ((float)py + 0.5f) / (float)H) * tan_y;
  V3 d = fwd + u * right + vv * up;
  d = (1.f / sqrtf(dot(d, d))) * d;

  // closest hit
  float best = INFINITY;
  int id = PGTT_SEG_SKY;
  V3 n = v3(0.f, 0.f, 1.f);
  if ((!kMap || ma.terrain) && d.z != 0.f) {
    const float t = -o.z / d.z;
    if (t > 0.f) { best = t; id = PGTT_SEG_PLANE; }
  }
  for (int b = 0; b < B; b++) {
    const float* bx = sh_box + b * kBoxWords;
    int axis; float sgn;
    const float t = hit_box(o, d, bx, axis, sgn);
    if (t < best) { best = t; id = PGTT_SEG_BOX + b; n = sgn * ld3(bx + 3 + 3 * axis); }
  }
  for (int g = 0; g < ngeom; g++) {
    const float* G = sh_view + kHeadWords + g * kGeomWords;
    const float t = hit_geom(o, d, G);
    if (t < best) { best = t; id = PGTT_SEG_GEOM + g; }
  }
  for (int k = 0; k < M; k++) {
    const float t = hit_sphere(o, d, ld3(sh_mk + 4 * k), sh_mk[4 * k + 3]);
    if (t < best) { best = t; id = PGTT_SEG_MARKER + k; }
  }
  if constexpr (kMap) {
    int cell, axis;
    const float t = hit_columns(sh_map, G, ma.res, ma.floor_z, ma.lift, v3(o.x - win_x, o.y - win_y, o.z), d, best, cell, axis);
    if (t < best) {
      best = t; id = PGTT_SEG_CELL + cell;
      const float c = axis == 0 ? d.x : axis == 1 ? d.y : d.z, sgn = c < 0.f ? 1.f : -1.f;
      n = v3(axis == 0 ? sgn : 0.f, axis == 1 ? sgn : 0.f, axis == 2 ? sgn : 0.f);
    }
  }

  V3 col;
  if (id == PGTT_SEG_SKY) {
    const float s = fmaxf(d.z, 0.f);
    col = v3(PGTT_RENDER_SKY_HORIZON_R + (PGTT_RENDER_SKY_ZENITH_R - PGTT_RENDER_SKY_HORIZON_R) * s,
             PGTT_RENDER_SKY_HORIZON_G + (PGTT_RENDER_SKY_ZENITH_G - PGTT_RENDER_SKY_HORIZON_G) * s,
             PGTT_RENDER_SKY_HORIZON_B + (PGTT_RENDER_SKY_ZENITH_B - PGTT_RENDER_SKY_HORIZON_B) * s);
  } else {
    const V3 p = o + best * d;
    V3 alb;
    if (id == PGTT_SEG_PLANE) {
      const int par = ((int)floorf(p.x / PGTT_RENDER_CHECKER) + (int)floorf(p.y / PGTT_RENDER_CHECKER)) & 1;
      alb = par ? v3(PGTT_RENDER_FLOOR_B_R, PGTT_RENDER_FLOOR_B_G, PGTT_RENDER_FLOOR_B_B) : v3(PGTT_RENDER_FLOOR_A_R, PGTT_RENDER_FLOOR_A_G, PGTT_RENDER_FLOOR_A_B);
    } else if (id < PGTT_SEG_GEOM) {
      alb = v3(PGTT_RENDER_BOX_R, PGTT_RENDER_BOX_G, PGTT_RENDER_BOX_B);
    } else if (id < PGTT_SEG_MARKER) {
      const float* G = sh_view + kHeadWords + (id - PGTT_SEG_GEOM) * kGeomWords;
      alb = ld3(G + 15);
      const int type = __float_as_int(G[18]);
      if (type == PGTT_RENDER_SPHERE) n = (1.f / G[12]) * (p - ld3(G));
      else if (type == PGTT_RENDER_CAPSULE) n = capsule_normal(p, ld3(G), ld3(G + 9), G[12], G[13]);
      else {
        float bx[kBoxWords];
#pragma unroll
        for (int i = 0; i < 15; i++) bx[i] = G[i];
        int axis; float sgn;
        hit_box(o, d, bx, axis, sgn);
        n = sgn * ld3(G + 3 + 3 * axis);
      }
    } else if (!kMap || id < PGTT_SEG_CELL) {
      const float* mk = sh_mk + 4 * (id - PGTT_SEG_MARKER);
      alb = v3(PGTT_RENDER_MARKER_R, PGTT_RENDER_MARKER_G, PGTT_RENDER_MARKER_B);
      n = (1.f / mk[3]) * (p - ld3(mk));
    } else {
      // a column: coloured by the tint layer at its slot, or by its own height
      const int cell = id - PGTT_SEG_CELL;
      float s = sh_map[cell];
      if (ma.tint) {
        const int a = cell / G, b = cell - a * G;
        int sa = slot_x0 + a, sb = slot_y0 + b;
        if (sa >= G) sa -= G;
        if (sb >= G) sb -= G;
        s = ma.tint[env_cells + sa * G + sb];
      }
      const float x = fminf(fmaxf((s - ma.tint_lo) / (ma.tint_hi - ma.tint_lo), 0.f), 1.f);
      alb = s != s ? v3(PGTT_RENDER_MAP_NOVALUE_R, PGTT_RENDER_MAP_NOVALUE_G, PGTT_RENDER_MAP_NOVALUE_B)
                   : v3(PGTT_RENDER_MAP_COLD_R + (PGTT_RENDER_MAP_HOT_R - PGTT_RENDER_MAP_COLD_R) * x,
                        PGTT_RENDER_MAP_COLD_G + (PGTT_RENDER_MAP_HOT_G - PGTT_RENDER_MAP_COLD_G) * x,
                        PGTT_RENDER_MAP_COLD_B + (PGTT_RENDER_MAP_HOT_B - PGTT_RENDER_MAP_COLD_B) * x);
    }
    if (dot(n, d) > 0.f) n = -1.f * n;
    V3 l = v3(PGTT_RENDER_LIGHT_X, PGTT_RENDER_LIGHT_Y, PGTT_RENDER_LIGHT_Z);
    l = (1.f / sqrtf(dot(l, l))) * l;
    const float ndl = fmaxf(dot(n, l), 0.f);
    float vis = 1.f;
    if (shadows && ndl > 0.f) {
      // any hit toward the light among the boxes and the robot geoms
      const V3 so = p + PGTT_RENDER_SHADOW_EPS * n;
      bool occ = false;
      for (int b = 0; b < B && !occ; b++) {
        int axis; float sgn;
        occ = hit_box(so, l, sh_box + b * kBoxWords, axis, sgn) < INFINITY;
      }
      for (int g = 0; g < ngeom && !occ; g++) occ = hit_geom(so, l, sh_view + kHeadWords + g * kGeomWords) < INFINITY;
      if constexpr (kMap) {
        // ... and the columns: the same walk, toward the light
        if (!occ) {
          int cell, axis;
          occ = hit_columns(sh_map, G, ma.res, ma.floor_z, ma.lift, v3(so.x - win_x, so.y - win_y, so.z), l, INFINITY, cell, axis) < INFINITY;
        }
      }
      vis = occ ? 0.f : 1.f;
    }
    const float s = PGTT_RENDER_AMBIENT + PGTT_RENDER_DIFFUSE * ndl * vis;
    col = v3(alb.x * s, alb.y * s, alb.z * s);
  }
  if (px < W && py < H) {
    const size_t idx = ((size_t)vi * H + py) * W + px;
    auto q8 = [](float c) { return (uint32_t)rintf(255.f * fminf(fmaxf(c, 0.f), 1.f)); };
    rgba[idx] = q8(col.x) | (q8(col.y) << 8) | (q8(col.z) << 16) | (255u << 24);
    if (depth) depth[idx] = id == PGTT_SEG_SKY ? INFINITY : best * dot(d, fwd);
    if (seg) seg[idx] = id;
  }
}

}  // namespace

struct pgtt_renderer {
  int ngeom = 0;
  SceneTables scene;
};

extern "C" {

PGTT_SIDE_EXPORTS(render, RENDER)
int pgtt_render_sizeof_geom(void) { return (int)sizeof(PgttRenderGeom); }
int pgtt_render_sizeof_camera(void) { return (int)sizeof(PgttRenderCamera); }
int pgtt_render_sizeof_views(void) { return (int)sizeof(PgttRenderViews); }
int pgtt_render_sizeof_map(void) { return (int)sizeof(PgttRenderMap); }

int64_t pgtt_render_workspace_bytes(int num_views) {
  if (num_views < 1 || num_views > PGTT_RENDER_MAX_VIEWS) return 0;
  return (int64_t)num_views * kViewWords * (int64_t)sizeof(float);
}

int pgtt_render_create(const PgttModel* model, const PgttRenderGeom* geoms, int ngeom, int device, pgtt_render_handle* out) {
  if (!model || !out || (ngeom > 0 && !geoms)) return fail(PGTT_E_ARG, "pgtt_render_create: null argument");
  *out = nullptr;
  if (int rc = check_geoms(geoms, ngeom, "pgtt_render_create")) return rc;
  if (int rc = check_device(device, "pgtt_render_create")) return rc;
  pgtt_renderer* h = new pgtt_renderer();
  h->ngeom = ngeom; h->scene.device = device;
  if (int rc = h->scene.upload(model, geoms, ngeom)) { pgtt_render_destroy(h); return rc; }
  *out = h;
  return PGTT_OK;
}

int pgtt_render_destroy(pgtt_render_handle h) {
  if (!h) return PGTT_OK;
  h->scene.release();
  delete h;
  return PGTT_OK;
}

int pgtt_render_set_terrain(pgtt_render_handle h, const float* boxes, int T, int B) {
  if (!h) return fail(PGTT_E_ARG, "null handle");
  return h->scene.set_terrain(boxes, T, B, "pgtt_render_set_terrain");
}

}  // extern "C"

namespace {

// what both render entries refuse; `who` is the entry's name
int check_views(pgtt_render_handle h, const PgttRenderViews* v, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (!h || !v) return fail(PGTT_E_ARG, p + "null argument");
  if (!v->state || !v->rgba || !v->workspace || !v->env_ids || !v->cameras) return fail(PGTT_E_ARG, p + "state, rgba, workspace, env_ids and cameras are required");
  if ((uintptr_t)v->workspace % 16 != 0) return fail(PGTT_E_ARG, p + "workspace must be 16-byte aligned");
  if (v->num_envs < 1) return fail(PGTT_E_ARG, p + "num_envs must be >= 1");
  if (v->num_views < 1 || v->num_views > PGTT_RENDER_MAX_VIEWS) return fail(PGTT_E_ARG, p + "num_views outside [1, PGTT_RENDER_MAX_VIEWS]");
  if (v->width < 1 || v->height < 1 || v->width > PGTT_RENDER_MAX_DIM || v->height > PGTT_RENDER_MAX_DIM)
    return fail(PGTT_E_ARG, p + "width and height must be in [1, PGTT_RENDER_MAX_DIM]");
  if (v->num_markers < 0 || v->num_markers > PGTT_RENDER_MAX_MARKER) return fail(PGTT_E_ARG, p + "num_markers outside [0, PGTT_RENDER_MAX_MARKER]");
  if (v->num_markers > 0 && !v->markers) return fail(PGTT_E_ARG, p + "num_markers > 0 needs a markers buffer");
  for (int i = 0; i < v->num_views; i++) {
    if (v->env_ids[i] < 0 || v->env_ids[i] >= v->num_envs) return fail(PGTT_E_ARG, p + "env id outside [0, num_envs)");
    const PgttRenderCamera& c = v->cameras[i];
    if (c.mode < PGTT_CAM_FIXED || c.mode > PGTT_CAM_TRACK_YAW) return fail(PGTT_E_ARG, p + "unknown camera mode");
    if (!(c.distance > 0.f) || !std::isfinite(c.distance)) return fail(PGTT_E_ARG, p + "camera distance must be positive");
    if (!(c.fovy_deg > 0.f) || !(c.fovy_deg < 180.f)) return fail(PGTT_E_ARG, p + "fovy must be in (0, 180) degrees");
    if (!std::isfinite(c.azimuth_deg) || !std::isfinite(c.elevation_deg) || !std::isfinite(c.target[0]) || !std::isfinite(c.target[1]) || !std::isfinite(c.target[2]))
      return fail(PGTT_E_ARG, p + "camera angles and target must be finite");
  }
  return PGTT_OK;
}

// both entries: the setup kernel over the views in chunks, then one pixel launch - the map call's when `m` is given
int launch_views(pgtt_render_handle h, const PgttRenderViews* v, const PgttRenderMap* m, void* stream) {
  HIP_TRY(hipSetDevice(h->scene.device));
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)v->workspace;
  for (int first = 0; first < v->num_views; first += kChunk) {
    const int nv = std::min(kChunk, v->num_views - first);
    SetupChunk chunk;
    std::memset(&chunk, 0, sizeof(chunk));
    for (int i = 0; i < nv; i++) { chunk.v[i].env = v->env_ids[first + i]; chunk.v[i].cam = v->cameras[first + i]; }
    hipLaunchKernelGGL(render_setup_kernel, dim3(nv), dim3(64), 0, st, chunk, first, v->state, v->params, v->variant, v->num_envs, h->scene.T,
                       h->scene.d_model, h->scene.d_geoms, h->ngeom, ws, v->body_pose);
  }
  const int tiles_x = (v->width + kTile - 1) / kTile, tiles_y = (v->height + kTile - 1) / kTile;
  const dim3 grid(tiles_x * tiles_y, v->num_views), block(kTile * kTile);
  const int shadows = (v->flags & PGTT_RENDER_SHADOWS) ? 1 : 0;
  if (!m) {
    hipLaunchKernelGGL((render_pixel_kernel<false>), grid, block, 0, st, ws, h->scene.d_boxes, h->scene.B, v->markers, v->num_markers, h->ngeom, v->width,
                       v->height, tiles_x, shadows, v->rgba, v->depth, v->segmentation);
  } else {
    const int terrain = (m->flags & PGTT_RENDER_MAP_TERRAIN) ? 1 : 0;
    const MapArgs ma = {m->map, m->origin, m->tint, m->grid, m->res, m->floor_z, m->lift, m->tint_lo, m->tint_hi, terrain};
    hipLaunchKernelGGL((render_pixel_kernel<true, MapArgs>), grid, block, 0, st, ws, h->scene.d_boxes, terrain ? h->scene.B : 0, v->markers, v->num_markers,
                       h->ngeom, v->width, v->height, tiles_x, shadows, v->rgba, v->depth, v->segmentation, ma);
  }
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

}  // namespace

extern "C" {

int pgtt_render(pgtt_render_handle h, const PgttRenderViews* v, void* stream) {
  if (int rc = check_views(h, v, "pgtt_render")) return rc;
  return launch_views(h, v, nullptr, stream);
}

int pgtt_render_map(pgtt_render_handle h, const PgttRenderViews* v, const PgttRenderMap* m, void* stream) {
  const std::string p = "pgtt_render_map: ";
  if (int rc = check_views(h, v, "pgtt_render_map")) return rc;
  if (!m) return fail(PGTT_E_ARG, p + "null PgttRenderMap");
  if (!m->map || !m->origin) return fail(PGTT_E_ARG, p + "map and origin are required");
  if (m->grid < 1 || m->grid > PGTT_RENDER_MAP_MAX_GRID) return fail(PGTT_E_ARG, p + "grid outside [1, PGTT_RENDER_MAP_MAX_GRID]");
  if (!(m->res > 0.f) || !std::isfinite(m->res)) return fail(PGTT_E_ARG, p + "res must be positive and finite");
  if (!std::isfinite(m->floor_z) || !std::isfinite(m->lift)) return fail(PGTT_E_ARG, p + "floor_z and lift must be finite");
  if (!std::isfinite(m->tint_lo) || !std::isfinite(m->tint_hi)) return fail(PGTT_E_ARG, p + "tint_lo and tint_hi must be finite");
  if (!(m->tint_lo < m->tint_hi)) return fail(PGTT_E_ARG, p + "tint_hi must be above tint_lo");
  if (m->flags & ~PGTT_RENDER_MAP_TERRAIN) return fail(PGTT_E_ARG, p + "unknown flag bits");
  return launch_views(h, v, m, stream);
}

}  // extern "C"
