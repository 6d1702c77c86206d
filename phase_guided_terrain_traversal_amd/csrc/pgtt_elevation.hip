// pgtt_elevation.hip — libpgtt_elevation.so: the elevation map fused from a depth image or from a point cloud (include/pgtt_elevation.h), one
// launch per call.
//
// elevation_kernel<POINTS>, one workgroup of four waves per env; a template on the source, so that the image instantiation (POINTS = false) holds
// no code of the other and is what it was before there were two.  LDS holds one word per map slot, `sh_m`: first the tick maximum as an
// order-preserving integer key (0 = no pixel fell into the slot), then, after the fuse, the slot's fused height, which the scan is sampled from.
//   phase A  lane 0 forms the base pose, the camera pose, the yaw's sine and cosine, the new origin and writes it; the other lanes zero sh_m.
//   phase B  lanes 0 .. 2G - 1 mark, per axis, the slot rows / columns whose world cell differs between the old and the new window.
//   phase C  every lane unprojects pixels (16-byte runs of the image when the pixel count allows) and raises sh_m[slot] with an LDS atomic maximum;
//            with POINTS every lane reads world points instead (the contiguous 12-byte-per-lane run) and there is no camera.
//   phase D  the persistent map streams through: 16-byte runs from HBM, stale slots to NaN, touched slots fused, the run written back only when
//            one of its slots changed; the fused value replaces the key in sh_m.
//   phase E  lanes 0 .. 116 sample the scan, the minimum over the known points is a wave reduction and one LDS exchange; est, known.
//   phase F  obs_out = obs with the scan rows replaced.
// The phases are separated by workgroup barriers.  No global atomics, no scratch; nothing is shared between envs.
// Written once, in front of the kernels ("what the kernels share"): phase A (stage_tick, from load_pose, stage_base, stage_camera, stage_yaw, cleared,
// window_of / stage_window), phase B (mark_stale), phase E (scan_min_and_write), phase F (assemble), stored_origin and scan_slot.  Phases C and D -
// the self filter, the window test, the unprojection, the image walk, the slot walk - are written out in every kernel that has them, and
// visibility_kernel holds its own phase A and clear predicate as well: which products the compiler fuses there depends on the code around them, and
// sharing these pieces moved outputs by an ulp.
//
// elevation_var_kernel<POINTS>, the variance tick (pgtt_elevation_var, pgtt_elevation_var_points): the same phases with a second pass over the pixels
// (integer band sums in a 64-bit LDS word per slot) and a Kalman update per slot while `map` and `var` stream through; described at the kernel.
// Phases A, B, E and F are the shared helpers'; phases C and D are its own.
//
// fill_kernel, the hole filling behind a tick: one workgroup of four waves per env again.  LDS holds the window in WINDOW order inside a border of one
// cell, one key word (key_of the value; kNoKey = a hole or the border) and one byte `D` per cell: 5 (G + 2)^2 bytes, 48020 at G = 96, under the
// 64 KB that need no launch attribute.  The border makes the window's edges edges and keeps every neighbour's index in range.
//   load     the map streams in as in phase D (16-byte runs, dwords for an odd G), every slot to its window cell; lane 0 stages the base
//            position, the yaw's sine and cosine (load_pose, stage_yaw) and the window of the stored origin (stored_origin, window_of).
//   pass p   every hole takes the minimum key over its neighbours with D < p, and D = p.  A cell written in this pass reads as a hole or as a key
//            with D = p or still 255, none of them a source, so one barrier per pass suffices and there are no atomics; a flag every lane reads
//            alike ends the loop after a pass that filled nothing.
//   sample   lanes 0 .. 116 read the key and D at the scan points (scan_slot); the minimum over the covered points is taken on the keys.
//   out      est, dist, obs_out (assemble), map_out and dist_out in the map's slot layout.
// It writes nothing the tick reads.
//
// Following a slower sensor (pgtt_elevation_follow): two launches, of which one does the work.  Both read the sensor's counter on the device and
// decide alike, in every workgroup, whether the call is fresh (fresh_call, the sensor's own rule one step later).
//   elevation_kernel<POINTS, true>  the gated instantiation: the tick above on a fresh call, returns at once on a hold call.
//   elevation_hold_kernel           returns at once on a fresh call.  On a hold call it leaves the map alone and samples the scan at the current
//            pose from the window the stored origin describes.  Two envs per workgroup, two waves per env; the map is not staged in LDS: a hold
//            needs 117 of its cells, gathered from global memory.  Lane 0 of each env stages the pose and the window (and writes the origin of a
//            cleared env); a cleared env's map goes out as NaN in 16-byte runs; the minimum, est and known are scan_min_and_write's and obs_out is
//            assemble's, both on the env's 128 lanes.  No atomics.
//
// Odometry drift (pgtt_elevation_odometry): odometry_kernel<POINTS> writes the estimated pose [7][N] the map may be bound to in place of `state`, and
// with POINTS the world points re-registered at it; odometry_advance_kernel behind it advances the draws' epoch.  Described at the kernel.  It reads
// and writes nothing of the handle's buffers, and no kernel above knows of it.
//
// Visibility clean-up (pgtt_elevation_visibility): visibility_kernel<POINTS>, a launch of its own in front of a tick.  The rays of the image or of the
// points lower a bound per slot in LDS, and a cell that stands above its bound by more than the margin is forgotten.  Described at the kernel.  It
// writes `map` (and `var`) and its own two outputs, and no kernel above knows of it.
//
// Sensor latency (pgtt_elevation_delayed): three launches.  latency_push_kernel stores the env's frame and its seven pose rows in slot `counter mod D`
// of a ring, draws a cleared env's latency and says whether the frame that is due exists; elevation_kernel<POINTS, false, true>, the STAMPED
// instantiation, is the tick with phase C under the pose of the due frame's capture and on that frame, everything else under the current pose;
// odometry_advance_kernel advances the counter behind both.  The four older instantiations hold none of this.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pgtt_elevation.h"
#include "pgtt_side_device.hip.h"
#include "pgtt_side_host.h"

namespace {

constexpr int kLanes = 256;                       // four waves per env
constexpr int kMaxG = PGTT_ELEVATION_MAX_GRID;
constexpr float kCellClamp = 1.0e9f;              // |cell index| stays below 2^30: a far-away or NaN coordinate cannot overflow the integer window test
static_assert(5 * (kMaxG + 2) * (kMaxG + 2) + 1024 <= 65536 && kMaxG - 1 < 255, "the fill's W and D with its staging stay under 64 KB of LDS; D fits a byte with 255 free");
static_assert(PGTT_NSCAN <= 128 && 2 * kMaxG <= kLanes && 4 * kMaxG * kMaxG <= 36864, "two waves sample the scan; one lane per slot row and column");

struct ElevArgs {
  const float* state; const float* depth; const float* obs; const float* done; const uint8_t* clear_mask;
  float* map; int32_t* origin; float* est; uint8_t* known; float* obs_out;
  int N, W, H, G, obs_dim, scan_row0, clear_all, use_done, self_on, vec_map, vec_img;
  float near_m, far_m, res, alpha, tu, tv, sdx, sdy;         // tu = tan(fovy / 2) W / H, tv = tan(fovy / 2)
  float mpos[3], mquat[4], self_half[3];
  const float* points; int P;                                // the points entry: [N][P][3] world points
  const int64_t* counter; int every, force;                  // the gated instantiations alone (pgtt_elevation_follow)
  // the stamped instantiations alone (pgtt_elevation_delayed): the ring the push kernel has filled, its counter as both kernels find it
  const float* ring_data; const float* ring_pose; const int32_t* lat; const uint8_t* fused; const int64_t* lat_counter; int D;
};

// what lane 0 stages for the workgroup
enum { P_CAM = 0, P_FWD = 3, P_RIGHT = 6, P_UP = 9, P_BASE = 12, P_RB = 15, P_SY = 24, P_CY = 25, P_N = 26 };
enum { P_CBASE = P_N, P_NS = P_N + 3 };           // the stamped tick: the base position at CAPTURE, next to the current one in P_BASE
enum { I_LOX = 0, I_LOY = 1, I_LMX = 2, I_LMY = 3, I_OLDX = 4, I_OLDY = 5, I_CLEAR = 6, I_FRAME = 7, I_N = 8 };   // I_FRAME: the stamped tick's ring slot, -1 = no frame

__device__ __forceinline__ int cell_of(float x, float res) { return (int)fminf(fmaxf(floorf(x / res), -kCellClamp), kCellClamp); }
// a value every lane holds alike, moved to a scalar register
__device__ __forceinline__ float uni(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ int floor_mod(int a, int g) { const int r = a % g; return r < 0 ? r + g : r; }
__device__ __forceinline__ int floor_mod64(long long a, int g) { const int r = (int)(a % g); return r < 0 ? r + g : r; }
// fp32 -> a key whose unsigned order is the order of the floats; no finite value maps to 0
__device__ __forceinline__ unsigned key_of(float z) { const unsigned b = __float_as_uint(z); return b ^ ((unsigned)((int)b >> 31) | 0x80000000u); }
__device__ __forceinline__ float value_of(unsigned k) { return __uint_as_float(k ^ (((k >> 31) - 1u) | 0x80000000u)); }

// ---------------------------------------------------------------- what the kernels share: every phase is stated once, here
// the seven pose rows of an env, S = its column of a [rows][N] array; NORMALISE: the quaternion divided by its norm
struct Pose { float bx, by, bz, qw, qx, qy, qz; };
template <bool NORMALISE = true>
__device__ __forceinline__ Pose load_pose(const float* S, long N) {
  const float bx = S[(PGTT_S_QPOS + 0) * N], by = S[(PGTT_S_QPOS + 1) * N], bz = S[(PGTT_S_QPOS + 2) * N];
  float qw = S[(PGTT_S_QPOS + 3) * N], qx = S[(PGTT_S_QPOS + 4) * N], qy = S[(PGTT_S_QPOS + 5) * N], qz = S[(PGTT_S_QPOS + 6) * N];
  if constexpr (NORMALISE) {
    const float qn = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= qn; qx /= qn; qy /= qn; qz /= qn;
  }
  return {bx, by, bz, qw, qx, qy, qz};
}
// the base position -> sh_p[base ..], the rows of the base rotation -> sh_p[P_RB ..]
struct Rot { float r00, r01, r02, r10, r11, r12, r20, r21, r22; };
__device__ __forceinline__ Rot stage_base(const Pose& p, int base, float* sh_p) {
  const float qw = p.qw, qx = p.qx, qy = p.qy, qz = p.qz;
  const float r00 = qw * qw + qx * qx - qy * qy - qz * qz, r01 = 2.f * (qx * qy - qw * qz), r02 = 2.f * (qx * qz + qw * qy);
  const float r10 = 2.f * (qx * qy + qw * qz), r11 = qw * qw - qx * qx + qy * qy - qz * qz, r12 = 2.f * (qy * qz - qw * qx);
  const float r20 = 2.f * (qx * qz - qw * qy), r21 = 2.f * (qy * qz + qw * qx), r22 = qw * qw - qx * qx - qy * qy + qz * qz;
  sh_p[base + 0] = p.bx; sh_p[base + 1] = p.by; sh_p[base + 2] = p.bz;
  sh_p[P_RB + 0] = r00; sh_p[P_RB + 1] = r01; sh_p[P_RB + 2] = r02; sh_p[P_RB + 3] = r10; sh_p[P_RB + 4] = r11; sh_p[P_RB + 5] = r12;
  sh_p[P_RB + 6] = r20; sh_p[P_RB + 7] = r21; sh_p[P_RB + 8] = r22;
  return {r00, r01, r02, r10, r11, r12, r20, r21, r22};
}
// the camera at mpos in the base frame -> sh_p[P_CAM ..]; camera = base * mount; fwd = its +x, up = its +z, right = fwd x up
__device__ __forceinline__ void stage_camera(const Pose& p, const Rot& R, const float* mpos, const float* mquat, float* sh_p) {
  sh_p[P_CAM + 0] = p.bx + R.r00 * mpos[0] + R.r01 * mpos[1] + R.r02 * mpos[2];
  sh_p[P_CAM + 1] = p.by + R.r10 * mpos[0] + R.r11 * mpos[1] + R.r12 * mpos[2];
  sh_p[P_CAM + 2] = p.bz + R.r20 * mpos[0] + R.r21 * mpos[1] + R.r22 * mpos[2];
  const float qw = p.qw, qx = p.qx, qy = p.qy, qz = p.qz;
  const float mw = mquat[0], mx = mquat[1], my = mquat[2], mz = mquat[3];
  const float cw = qw * mw - qx * mx - qy * my - qz * mz, cx = qw * mx + qx * mw + qy * mz - qz * my;
  const float cyq = qw * my - qx * mz + qy * mw + qz * mx, cz = qw * mz + qx * my - qy * mx + qz * mw;
  const float fx = cw * cw + cx * cx - cyq * cyq - cz * cz, fy = 2.f * (cx * cyq + cw * cz), fz = 2.f * (cx * cz - cw * cyq);
  const float ux = 2.f * (cx * cz + cw * cyq), uy = 2.f * (cyq * cz - cw * cx), uz = cw * cw - cx * cx - cyq * cyq + cz * cz;
  sh_p[P_FWD + 0] = fx; sh_p[P_FWD + 1] = fy; sh_p[P_FWD + 2] = fz;
  sh_p[P_UP + 0] = ux; sh_p[P_UP + 1] = uy; sh_p[P_UP + 2] = uz;
  sh_p[P_RIGHT + 0] = fy * uz - fz * uy; sh_p[P_RIGHT + 1] = fz * ux - fx * uz; sh_p[P_RIGHT + 2] = fx * uy - fy * ux;
}
// the sine and cosine of the yaw of a normalised base quaternion -> sh_p[P_SY], sh_p[P_CY]
__device__ __forceinline__ void stage_yaw(const Pose& p, float* sh_p) {
  const float yaw = atan2f(2.0f * (p.qw * p.qz + p.qx * p.qy), 1.0f - 2.0f * (p.qy * p.qy + p.qz * p.qz));
  float sy, cy;
  sincosf(yaw, &sy, &cy);
  sh_p[P_SY] = sy; sh_p[P_CY] = cy;
}
// does this call clear env e: the four fields every entry takes, in any of the argument structs
template <class A>
__device__ __forceinline__ bool cleared(const A& a, int e) {
  return a.clear_all || (a.clear_mask && a.clear_mask[e]) || (a.use_done && a.done && a.done[e] != 0.f);
}
// the origin as the last tick left it; one outside the tick's clamp (a map never ticked) is as far away as the clamp
__device__ __forceinline__ int2 stored_origin(const int32_t* origin, int e) {
  return make_int2(min(max(origin[2 * (long)e], -(1 << 30)), 1 << 30), min(max(origin[2 * (long)e + 1], -(1 << 30)), 1 << 30));
}
// the window of G x G cells around origin cell (ox, oy): its first cell and that cell's slot, per axis; sh_i[I_LOX .. I_LMY]
struct Window { int lox, loy, lmx, lmy; };
__device__ __forceinline__ Window window_of(int ox, int oy, int G) {
  const int lox = ox - G / 2, loy = oy - G / 2;
  return {lox, loy, floor_mod(lox, G), floor_mod(loy, G)};
}
__device__ __forceinline__ void stage_window(const Window& w, int* sh_i) { sh_i[I_LOX] = w.lox; sh_i[I_LOY] = w.loy; sh_i[I_LMX] = w.lmx; sh_i[I_LMY] = w.lmy; }
// the slot of the cell that contains scan point i = 9 r + c, or -1 outside the window.  pose: P_BASE, P_SY, P_CY; win: I_LOX .. I_LMY
__device__ __forceinline__ int scan_slot(int i, const float* pose, const int* win, float sdx, float sdy, float res, int G) {
  const int r = i / PGTT_SCAN_W, c = i - r * PGTT_SCAN_W;
  const float ox = ((float)(PGTT_SCAN_H - 1) * 0.5f - (float)r) * sdx, oy = ((float)(PGTT_SCAN_W - 1) * 0.5f - (float)c) * sdy;
  const float sy = pose[P_SY], cy = pose[P_CY];
  const float wx = pose[P_BASE + 0] + (ox * cy + oy * (-sy)), wy = pose[P_BASE + 1] + (ox * sy + oy * cy);
  const int relx = cell_of(wx, res) - win[I_LOX], rely = cell_of(wy, res) - win[I_LOY];
  int slot = -1;
  if ((unsigned)relx < (unsigned)G && (unsigned)rely < (unsigned)G) {
    int sx = relx + win[I_LMX], sy2 = rely + win[I_LMY];
    sx -= sx >= G ? G : 0; sy2 -= sy2 >= G ? G : 0;
    slot = sx * G + sy2;
  }
  return slot;
}
// phase B: lanes 0 .. 2G - 1 mark, per axis, the slots whose world cell moved.  Slot s holds world cell lo + ((s - lo) mod G) under the window that
// starts at lo.  sh_stale [0, G): slot rows (x), [G, 2G): slot columns (y)
__device__ __forceinline__ void mark_stale(const int* sh_i, unsigned char* sh_stale, int G, int tid) {
  if (tid < 2 * G) {
    const int ax = tid >= G, s = tid - ax * G;
    const int lo_new = sh_i[I_LOX + ax], lo_old = sh_i[I_OLDX + ax];
    unsigned char st = 1;
    if (!sh_i[I_CLEAR]) st = (lo_new + floor_mod(s - lo_new, G)) != (lo_old + floor_mod(s - lo_old, G));
    sh_stale[tid] = st;
  }
}
// phase E behind the lookup.  Lane lt of the env's LANES lanes holds z, the height at scan point lt, and kn, whether it is known (false in the lanes
// past the scan).  The minimum over the known points is a wave reduction and one exchange through sh_red[2], by the env's first two waves; est goes to
// sh_est and out, known out.  live = false: a half workgroup without an env, which only keeps the barrier
template <int LANES>
__device__ __forceinline__ void scan_min_and_write(float z, bool kn, bool live, int e, int lt, float* sh_red, float* sh_est, float* est, uint8_t* known) {
  float zmin = kn ? z : INFINITY;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) zmin = fminf(zmin, __shfl_xor(zmin, off, 64));
  if ((LANES == 128 || lt < 128) && (lt & 63) == 0) sh_red[lt >> 6] = zmin;
  __syncthreads();
  zmin = fminf(sh_red[0], sh_red[1]);
  if (live && lt < PGTT_NSCAN) {
    const float es = (kn && zmin < INFINITY) ? z - zmin : 0.f;
    sh_est[lt] = es;
    est[(long)e * PGTT_NSCAN + lt] = es;
    known[(long)e * PGTT_NSCAN + lt] = kn ? 1 : 0;
  }
}
// phase F: env e's row of obs_out = its row of obs with the scan rows replaced by est (LDS), by lane lt of the env's `lanes`
__device__ __forceinline__ void assemble(float* obs_out, const float* obs, const float* est, int e, int od, int row0, int lt, int lanes) {
  for (int k = lt; k < od; k += lanes) {
    const int j = k - row0;
    obs_out[(long)e * od + k] = (j >= 0 && j < PGTT_NSCAN) ? est[j] : obs[(long)e * od + k];
  }
}

// the sensor's rule, seen from behind the sensor's call, which has advanced the counter by one: every lane of every workgroup decides alike
__device__ __forceinline__ bool fresh_call(const int64_t* counter, int every, int force) {
  const long long c = counter[0] - 1;
  return force || (c >= 0 && (unsigned long long)c % (unsigned)every == 0);
}

// phase A of a tick, lane 0's: the sensor's pose (the base position to sh_p[P_SELF ..], the rotation, with an image the camera), then under the CURRENT
// pose the yaw, the clear, the old and the new window, and the new origin written.  STAMPED (pgtt_elevation_delayed): the sensor's pose is that of
// the due frame's capture, rows 0 .. 6 as the push kernel stored them in the ring (PGTT_S_QPOS = 0); without a frame the slot's rows are read all the
// same and what is made of them is not, phase C is skipped.  Both poses go through the same load_pose: the same operations on the same rows when the
// latency is 0, so the same bits
template <bool POINTS, bool STAMPED>
__device__ __forceinline__ void stage_tick(const ElevArgs& a, int e, float* sh_p, int* sh_i) {
  constexpr int P_SELF = STAMPED ? P_CBASE : P_BASE;
  const int G = a.G;
  const long N = a.N;
  const float* S = a.state + e;
  if constexpr (STAMPED) {
    const int frame = floor_mod64(a.lat_counter[0] - (long long)a.lat[e], a.D);
    sh_i[I_FRAME] = a.fused[e] ? frame : -1;
    S = a.ring_pose + (long)frame * 7 * N + e;
  }
  Pose p = load_pose(S, N);
  const Rot R = stage_base(p, P_SELF, sh_p);
  if constexpr (!POINTS) stage_camera(p, R, a.mpos, a.mquat, sh_p);
  if constexpr (STAMPED) {
    p = load_pose(a.state + e, N);
    sh_p[P_BASE + 0] = p.bx; sh_p[P_BASE + 1] = p.by; sh_p[P_BASE + 2] = p.bz;
  }
  stage_yaw(p, sh_p);
  const bool clear = cleared(a, e);
  const int ox = cell_of(p.bx, a.res), oy = cell_of(p.by, a.res);
  stage_window(window_of(ox, oy, G), sh_i);
  // an old origin outside the clamp (a map never ticked, garbage in the buffer) is as far away as the clamp: everything is stale
  const int px = a.origin[2 * (long)e], py = a.origin[2 * (long)e + 1];
  const bool sane = px >= -(1 << 30) && px <= (1 << 30) && py >= -(1 << 30) && py <= (1 << 30);
  sh_i[I_OLDX] = px - G / 2; sh_i[I_OLDY] = py - G / 2; sh_i[I_CLEAR] = (clear || !sane) ? 1 : 0;
  a.origin[2 * (long)e] = ox; a.origin[2 * (long)e + 1] = oy;
}

// STAMPED (pgtt_elevation_delayed): phase C works under the pose of the frame's CAPTURE, read from the ring - the camera, the self filter's rotation
// and, in P_CBASE, its base position - on the ring's frame; everything else (the clear, the window, the scan) under the current pose, as ever.
template <bool POINTS, bool GATED = false, bool STAMPED = false>
__global__ void __launch_bounds__(kLanes) elevation_kernel(ElevArgs a) {
  if constexpr (GATED) {
    if (!fresh_call(a.counter, a.every, a.force)) return;              // a hold call: elevation_hold_kernel's
  }
  extern __shared__ __attribute__((aligned(16))) unsigned sh_m[];      // [G * G]
  __shared__ float sh_p[STAMPED ? P_NS : P_N];
  constexpr int P_SELF = STAMPED ? P_CBASE : P_BASE;                   // the base position the self filter reads
  __shared__ int sh_i[I_N];
  __shared__ unsigned char sh_stale[2 * kMaxG];                        // [0, G): slot rows (x), [G, 2G): slot columns (y)
  __shared__ float sh_est[PGTT_NSCAN];
  __shared__ float sh_red[2];
  const int e = blockIdx.x, tid = threadIdx.x, G = a.G, GG = G * G;
  const long N = a.N;

  // ---- phase A: the poses (lane 0); the tick maximum starts empty
  if (tid == 0) stage_tick<POINTS, STAMPED>(a, e, sh_p, sh_i);
  for (int s = tid; s < GG; s += kLanes) sh_m[s] = 0u;
  __syncthreads();

  // ---- phase B: per axis, the slots whose world cell moved
  mark_stale(sh_i, sh_stale, G, tid);

  // ---- phase C: the tick maximum
  if constexpr (POINTS) {
    const float bpx = uni(sh_p[P_SELF + 0]), bpy = uni(sh_p[P_SELF + 1]), bpz = uni(sh_p[P_SELF + 2]);
    const float b00 = uni(sh_p[P_RB + 0]), b01 = uni(sh_p[P_RB + 1]), b02 = uni(sh_p[P_RB + 2]), b10 = uni(sh_p[P_RB + 3]), b11 = uni(sh_p[P_RB + 4]);
    const float b12 = uni(sh_p[P_RB + 5]), b20 = uni(sh_p[P_RB + 6]), b21 = uni(sh_p[P_RB + 7]), b22 = uni(sh_p[P_RB + 8]);
    const int lox = sh_i[I_LOX], loy = sh_i[I_LOY], lmx = sh_i[I_LMX], lmy = sh_i[I_LMY];
    const float* pts = a.points + (long)e * a.P * 3;
    int np = a.P;
    if constexpr (STAMPED) {                                           // the ring's frame, or none
      const int frame = sh_i[I_FRAME];
      pts = a.ring_data + ((long)max(frame, 0) * N + e) * a.P * 3;
      if (frame < 0) np = 0;
    }
    for (int k = tid; k < np; k += kLanes) {
      const float px = pts[3 * k], py = pts[3 * k + 1], pz = pts[3 * k + 2];
      if (!(fabsf(px) < INFINITY && fabsf(py) < INFINITY && fabsf(pz) < INFINITY)) continue;      // a NaN (no return) or a non-finite coordinate
      if (a.self_on) {
        const float dx = px - bpx, dy = py - bpy, dz = pz - bpz;             // R^T (p - base)
        const float lx = b00 * dx + b10 * dy + b20 * dz, ly = b01 * dx + b11 * dy + b21 * dz, lz = b02 * dx + b12 * dy + b22 * dz;
        if (fabsf(lx) <= a.self_half[0] && fabsf(ly) <= a.self_half[1] && fabsf(lz) <= a.self_half[2]) continue;
      }
      const int relx = cell_of(px, a.res) - lox, rely = cell_of(py, a.res) - loy;
      if ((unsigned)relx >= (unsigned)G || (unsigned)rely >= (unsigned)G) continue;
      int sx = relx + lmx, sy = rely + lmy;                            // (lo + rel) mod G
      sx -= sx >= G ? G : 0; sy -= sy >= G ? G : 0;
      atomicMax(&sh_m[sx * G + sy], key_of(pz));
    }
  } else {
    const float cpx = sh_p[P_CAM + 0], cpy = sh_p[P_CAM + 1], cpz = sh_p[P_CAM + 2];
    const float fx = sh_p[P_FWD + 0], fy = sh_p[P_FWD + 1], fz = sh_p[P_FWD + 2];
    const float rx = sh_p[P_RIGHT + 0], ry = sh_p[P_RIGHT + 1], rz = sh_p[P_RIGHT + 2];
    const float ux = sh_p[P_UP + 0], uy = sh_p[P_UP + 1], uz = sh_p[P_UP + 2];
    // the self filter's base position and rotation are read once, like the camera basis (the compiler cannot hoist LDS reads over the LDS atomics),
    // and kept in scalar registers: twelve more vector registers would cost the eighth wave per SIMD
    const float bpx = uni(sh_p[P_SELF + 0]), bpy = uni(sh_p[P_SELF + 1]), bpz = uni(sh_p[P_SELF + 2]);
    const float b00 = uni(sh_p[P_RB + 0]), b01 = uni(sh_p[P_RB + 1]), b02 = uni(sh_p[P_RB + 2]), b10 = uni(sh_p[P_RB + 3]), b11 = uni(sh_p[P_RB + 4]);
    const float b12 = uni(sh_p[P_RB + 5]), b20 = uni(sh_p[P_RB + 6]), b21 = uni(sh_p[P_RB + 7]), b22 = uni(sh_p[P_RB + 8]);
    const int lox = sh_i[I_LOX], loy = sh_i[I_LOY], lmx = sh_i[I_LMX], lmy = sh_i[I_LMY];
    const int W = a.W;
    int npix = a.W * a.H;
    const float* img = a.depth + (long)e * npix;
    if constexpr (STAMPED) {                                           // the ring's frame, or none
      const int frame = sh_i[I_FRAME];
      img = a.ring_data + ((long)max(frame, 0) * N + e) * npix;
      if (frame < 0) npix = 0;
    }
    auto pixel = [&](float d, int i, int j) {
      if (!(d > a.near_m && d < a.far_m)) return;                     // NaN, a miss, a dropout, below near
      const float u = (2.f * ((float)j + 0.5f) / (float)W - 1.f) * a.tu, v = (1.f - 2.f * ((float)i + 0.5f) / (float)a.H) * a.tv;
      const float px = cpx + d * (fx + u * rx + v * ux), py = cpy + d * (fy + u * ry + v * uy), pz = cpz + d * (fz + u * rz + v * uz);
      if (a.self_on) {
        const float dx = px - bpx, dy = py - bpy, dz = pz - bpz;             // R^T (p - base)
        const float lx = b00 * dx + b10 * dy + b20 * dz, ly = b01 * dx + b11 * dy + b21 * dz, lz = b02 * dx + b12 * dy + b22 * dz;
        if (fabsf(lx) <= a.self_half[0] && fabsf(ly) <= a.self_half[1] && fabsf(lz) <= a.self_half[2]) return;
      }
      const int relx = cell_of(px, a.res) - lox, rely = cell_of(py, a.res) - loy;
      if ((unsigned)relx >= (unsigned)G || (unsigned)rely >= (unsigned)G || !(pz == pz)) return;
      int sx = relx + lmx, sy = rely + lmy;                            // (lo + rel) mod G
      sx -= sx >= G ? G : 0; sy -= sy >= G ? G : 0;
      atomicMax(&sh_m[sx * G + sy], key_of(pz));
    };
    if (a.vec_img) {
      for (int p = 4 * tid; p < npix; p += 4 * kLanes) {
        const float4 d = *reinterpret_cast<const float4*>(img + p);
        int i = p / W, j = p - i * W;
        const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
          pixel(dv[k], i, j);
          j++;
          if (j == W) { j = 0; i++; }
        }
      }
    } else {
      for (int p = tid; p < npix; p += kLanes) { const int i = p / W; pixel(img[p], i, p - i * W); }
    }
  }
  __syncthreads();

  // ---- phase D: the map streams through; sh_m takes the fused heights
  {
    float* mp = a.map + (long)e * GG;
    const float alpha = a.alpha;
    const float nanv = __uint_as_float(0x7fc00000u);
    // one slot: -> the new height; `changed` when the stored value has to be written
    auto slot = [&](float h, unsigned key, int sx, int sy, bool& changed) {
      if (sh_stale[sx] | sh_stale[G + sy]) { h = nanv; changed = true; }
      if (key) {
        const float m = value_of(key);
        h = (h != h || alpha == 1.f) ? m : h + alpha * (m - h);       // alpha = 1 stores m itself: h + (m - h) would round
        changed = true;
      }
      return h;
    };
    if (a.vec_map) {
      for (int s = 4 * tid; s < GG; s += 4 * kLanes) {
        const float4 hv = *reinterpret_cast<const float4*>(mp + s);
        const uint4 kv = *reinterpret_cast<const uint4*>(sh_m + s);
        int sx = s / G, sy = s - sx * G;
        float h[4] = {hv.x, hv.y, hv.z, hv.w};
        const unsigned k4[4] = {kv.x, kv.y, kv.z, kv.w};
        bool changed = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          h[k] = slot(h[k], k4[k], sx, sy, changed);
          sy++;
          if (sy == G) { sy = 0; sx++; }
        }
        const float4 out = make_float4(h[0], h[1], h[2], h[3]);
        if (changed) *reinterpret_cast<float4*>(mp + s) = out;
        *reinterpret_cast<float4*>(sh_m + s) = out;
      }
    } else {
      for (int s = tid; s < GG; s += kLanes) {
        const int sx = s / G;
        bool changed = false;
        const float h = slot(mp[s], sh_m[s], sx, s - sx * G, changed);
        if (changed) mp[s] = h;
        sh_m[s] = __float_as_uint(h);
      }
    }
  }
  __syncthreads();

  // ---- phase E: the scan
  float z = 0.f;
  bool kn = false;
  if (tid < PGTT_NSCAN) {
    const int slot = scan_slot(tid, sh_p, sh_i, a.sdx, a.sdy, a.res, G);
    if (slot >= 0) {
      z = __uint_as_float(sh_m[slot]);
      kn = z == z;
    }
  }
  scan_min_and_write<kLanes>(z, kn, true, e, tid, sh_red, sh_est, a.est, a.known);

  // ---- phase F: obs_out = obs with the scan rows replaced
  if (a.obs_out) {
    __syncthreads();
    assemble(a.obs_out, a.obs, sh_est, e, a.obs_dim, a.scan_row0, tid, kLanes);
  }
}

// the variance tick: the plain tick's arguments (alpha is not read) and the variance layer's
struct VarArgs {
  ElevArgs a;
  float* var; float* est_var;
  float s0sq, srsq, process, gate2, band, var_max;           // sigma0^2, sigma_rel^2, gate^2
  int max_count;
};

constexpr int kCountShift = 40;                   // the (n, S) word: n above bit 40, S below.  n <= 65536 pixels, S < 65536 * 2^17 = 2^33
static_assert((double)PGTT_ELEVATION_MAX_BAND * PGTT_ELEVATION_BAND_SCALE <= 131072.0 && PGTT_ELEVATION_MAX_DIM * PGTT_ELEVATION_MAX_DIM <= 65536,
              "S stays below bit 40 for the image; a point cloud of P < 2^23 points does too");
static_assert(12 * PGTT_ELEVATION_VAR_MAX_GRID * PGTT_ELEVATION_VAR_MAX_GRID + 2048 <= 65536, "the variance tick's LDS needs no launch attribute");

// elevation_var_kernel<POINTS>: the variance tick (include/pgtt_elevation.h, "Variance-weighted fusion"), one workgroup of four waves per env.
// Dynamic LDS: sh_acc[G G], one 64-bit word (n << 40 | S) per slot, then sh_m[G G], the key word of elevation_kernel.  After phase D sh_m holds the
// fused heights and the low half of each sh_acc word the slot's variance.
//   phase A, B  stage_tick and mark_stale; the lanes zero both arrays.
//   phase C  two passes over the same pixels (or points) by ONE loop body, so that a point and its slot are the same bits in both: pass 0 raises
//            sh_m[slot] (ds_max_u32 on the key), pass 1 adds (1 << 40 | q) to sh_acc[slot] (ds_add_u64) for the pixels inside the band.  The point is
//            recomputed in pass 1: a lane holds up to 256 pixels of a 256 x 256 image, which no register file keeps.
//   phase D  `map` and `var` stream through in 16-byte runs (dwords for an odd G G): stale slots to NaN, predict, measurement and update per slot; a
//            run of either array is written back only when one of its slots changed there.
//   phase E, F  scan_min_and_write and assemble, with est_var next to est.
// Integer LDS atomics only; no global atomics, no scratch.
template <bool POINTS>
__global__ void __launch_bounds__(kLanes) elevation_var_kernel(VarArgs va) {
  const ElevArgs& a = va.a;
  extern __shared__ __attribute__((aligned(16))) unsigned long long sh_acc[];      // [G * G], then the keys
  __shared__ float sh_p[P_N];
  __shared__ int sh_i[I_N];
  __shared__ unsigned char sh_stale[2 * kMaxG];
  __shared__ float sh_est[PGTT_NSCAN];
  __shared__ float sh_red[2];
  const int e = blockIdx.x, tid = threadIdx.x, G = a.G, GG = G * G;
  const long N = a.N;
  unsigned* sh_m = reinterpret_cast<unsigned*>(sh_acc + GG);

  // ---- phase A: the poses (lane 0); the tick maximum and the sums start empty
  if (tid == 0) stage_tick<POINTS, false>(a, e, sh_p, sh_i);
  for (int s = tid; s < GG; s += kLanes) { sh_acc[s] = 0ull; sh_m[s] = 0u; }
  __syncthreads();

  // ---- phase B: per axis, the slots whose world cell moved
  mark_stale(sh_i, sh_stale, G, tid);

  // ---- phase C: pass 0 the tick maximum, pass 1 the band sums.  `admit` is what both do with a point that step 3 admits into `slot`
  const float bpx = uni(sh_p[P_BASE + 0]), bpy = uni(sh_p[P_BASE + 1]), bpz = uni(sh_p[P_BASE + 2]);
  const int lox = sh_i[I_LOX], loy = sh_i[I_LOY], lmx = sh_i[I_LMX], lmy = sh_i[I_LMY];
  {
    const float b00 = uni(sh_p[P_RB + 0]), b01 = uni(sh_p[P_RB + 1]), b02 = uni(sh_p[P_RB + 2]), b10 = uni(sh_p[P_RB + 3]), b11 = uni(sh_p[P_RB + 4]);
    const float b12 = uni(sh_p[P_RB + 5]), b20 = uni(sh_p[P_RB + 6]), b21 = uni(sh_p[P_RB + 7]), b22 = uni(sh_p[P_RB + 8]);
    const float band = va.band;
    auto admit = [&](int pass, int slot, float pz) {
      if (pass == 0) {
        atomicMax(&sh_m[slot], key_of(pz));
      } else {
        const float dz = value_of(sh_m[slot]) - pz;                   // >= 0: the maximum was taken over these bits
        if (dz <= band) atomicAdd(&sh_acc[slot], (1ull << kCountShift) | (unsigned long long)(unsigned)rintf(dz * PGTT_ELEVATION_BAND_SCALE));
      }
    };
    if constexpr (POINTS) {
      const float* pts = a.points + (long)e * a.P * 3;
#pragma nounroll
      for (int pass = 0; pass < 2; pass++) {
        for (int k = tid; k < a.P; k += kLanes) {
          const float px = pts[3 * k], py = pts[3 * k + 1], pz = pts[3 * k + 2];
          if (!(fabsf(px) < INFINITY && fabsf(py) < INFINITY && fabsf(pz) < INFINITY)) continue;
          if (a.self_on) {
            const float dx = px - bpx, dy = py - bpy, dz = pz - bpz;
            const float lx = b00 * dx + b10 * dy + b20 * dz, ly = b01 * dx + b11 * dy + b21 * dz, lz = b02 * dx + b12 * dy + b22 * dz;
            if (fabsf(lx) <= a.self_half[0] && fabsf(ly) <= a.self_half[1] && fabsf(lz) <= a.self_half[2]) continue;
          }
          const int relx = cell_of(px, a.res) - lox, rely = cell_of(py, a.res) - loy;
          if ((unsigned)relx >= (unsigned)G || (unsigned)rely >= (unsigned)G) continue;
          int sx = relx + lmx, sy = rely + lmy;
          sx -= sx >= G ? G : 0; sy -= sy >= G ? G : 0;
          admit(pass, sx * G + sy, pz);
        }
        __syncthreads();
      }
    } else {
      const float cpx = sh_p[P_CAM + 0], cpy = sh_p[P_CAM + 1], cpz = sh_p[P_CAM + 2];
      const float fx = sh_p[P_FWD + 0], fy = sh_p[P_FWD + 1], fz = sh_p[P_FWD + 2];
      const float rx = sh_p[P_RIGHT + 0], ry = sh_p[P_RIGHT + 1], rz = sh_p[P_RIGHT + 2];
      const float ux = sh_p[P_UP + 0], uy = sh_p[P_UP + 1], uz = sh_p[P_UP + 2];
      const int W = a.W, npix = a.W * a.H;
      const float* img = a.depth + (long)e * npix;
      auto pixel = [&](int pass, float d, int i, int j) {
        if (!(d > a.near_m && d < a.far_m)) return;
        const float u = (2.f * ((float)j + 0.5f) / (float)W - 1.f) * a.tu, v = (1.f - 2.f * ((float)i + 0.5f) / (float)a.H) * a.tv;
        const float px = cpx + d * (fx + u * rx + v * ux), py = cpy + d * (fy + u * ry + v * uy), pz = cpz + d * (fz + u * rz + v * uz);
        if (a.self_on) {
          const float dx = px - bpx, dy = py - bpy, dz = pz - bpz;
          const float lx = b00 * dx + b10 * dy + b20 * dz, ly = b01 * dx + b11 * dy + b21 * dz, lz = b02 * dx + b12 * dy + b22 * dz;
          if (fabsf(lx) <= a.self_half[0] && fabsf(ly) <= a.self_half[1] && fabsf(lz) <= a.self_half[2]) return;
        }
        const int relx = cell_of(px, a.res) - lox, rely = cell_of(py, a.res) - loy;
        if ((unsigned)relx >= (unsigned)G || (unsigned)rely >= (unsigned)G || !(pz == pz)) return;
        int sx = relx + lmx, sy = rely + lmy;
        sx -= sx >= G ? G : 0; sy -= sy >= G ? G : 0;
        admit(pass, sx * G + sy, pz);
      };
#pragma nounroll
      for (int pass = 0; pass < 2; pass++) {
        if (a.vec_img) {
          for (int p = 4 * tid; p < npix; p += 4 * kLanes) {
            const float4 d = *reinterpret_cast<const float4*>(img + p);
            int i = p / W, j = p - i * W;
            const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
              pixel(pass, dv[k], i, j);
              j++;
              if (j == W) { j = 0; i++; }
            }
          }
        } else {
          for (int p = tid; p < npix; p += kLanes) { const int i = p / W; pixel(pass, img[p], i, p - i * W); }
        }
        __syncthreads();
      }
    }
  }

  // ---- phase D: map and var stream through; sh_m takes the fused heights, the low half of sh_acc the variances
  {
    float* mp = a.map + (long)e * GG;
    float* vp = va.var + (long)e * GG;
    float* sh_v = reinterpret_cast<float*>(sh_acc);                    // slot s: sh_v[2 s]
    const float nanv = __uint_as_float(0x7fc00000u);
    const float res = a.res, process = va.process, var_max = va.var_max, gate2 = va.gate2, s0sq = va.s0sq, srsq = va.srsq;
    const int max_count = va.max_count;
    // one slot: h and v in and out; ch / cv when the stored height / variance has to be written
    auto slot = [&](float& h, float& v, unsigned key, unsigned long long acc, int sx, int sy, bool& ch, bool& cv) {
      if (sh_stale[sx] | sh_stale[G + sy]) { h = nanv; v = nanv; ch = true; cv = true; }
      if (h == h) {                                                    // predict
        const float v1 = fminf(v + process, var_max);
        cv |= __float_as_uint(v1) != __float_as_uint(v);
        v = v1;
      }
      if (!key) return;
      int n = (int)(acc >> kCountShift);
      const unsigned long long S = acc & ((1ull << kCountShift) - 1);
      const float zmax = value_of(key);
      float m = zmax;
      if (n < 1) n = 1;                                                // a non-finite maximum has no band: it stands alone
      else if (S) m = zmax - ((float)S / (float)n) * (1.0f / PGTT_ELEVATION_BAND_SCALE);
      int wa = sx - lmx, wb = sy - lmy;                                // the slot's world cell: lo + ((s - lo) mod G)
      wa += wa < 0 ? G : 0; wb += wb < 0 ? G : 0;
      const float dx = ((float)(lox + wa) + 0.5f) * res - bpx, dy = ((float)(loy + wb) + 0.5f) * res - bpy, dz = m - bpz;
      const float rho2 = dx * dx + dy * dy + dz * dz;
      const float r = (s0sq + srsq * rho2) / (float)min(n, max_count);
      if (h != h) {
        h = m; v = fminf(r, var_max); ch = true; cv = true;
      } else {
        const float d = m - h, den = v + r;
        if (d * d <= gate2 * den) {
          const float k = den > 0.f ? v / den : 0.f;
          h += k * d; v = den > 0.f ? v * r / den : 0.f; ch = true; cv = true;
        } else if (m > h) {
          h = m; v = fminf(r, var_max); ch = true; cv = true;
        }
      }
    };
    if (a.vec_map) {
      for (int s = 4 * tid; s < GG; s += 4 * kLanes) {
        const float4 hv = *reinterpret_cast<const float4*>(mp + s);
        const float4 vv = *reinterpret_cast<const float4*>(vp + s);
        const uint4 kv = *reinterpret_cast<const uint4*>(sh_m + s);
        const ulonglong2 a01 = *reinterpret_cast<const ulonglong2*>(sh_acc + s), a23 = *reinterpret_cast<const ulonglong2*>(sh_acc + s + 2);
        int sx = s / G, sy = s - sx * G;
        float h[4] = {hv.x, hv.y, hv.z, hv.w}, v[4] = {vv.x, vv.y, vv.z, vv.w};
        const unsigned k4[4] = {kv.x, kv.y, kv.z, kv.w};
        const unsigned long long a4[4] = {a01.x, a01.y, a23.x, a23.y};
        bool ch = false, cv = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          slot(h[k], v[k], k4[k], a4[k], sx, sy, ch, cv);
          sy++;
          if (sy == G) { sy = 0; sx++; }
        }
        const float4 out = make_float4(h[0], h[1], h[2], h[3]);
        if (ch) *reinterpret_cast<float4*>(mp + s) = out;
        if (cv) *reinterpret_cast<float4*>(vp + s) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(sh_m + s) = out;
#pragma unroll
        for (int k = 0; k < 4; k++) sh_v[2 * (s + k)] = v[k];
      }
    } else {
      for (int s = tid; s < GG; s += kLanes) {
        const int sx = s / G;
        bool ch = false, cv = false;
        float h = mp[s], v = vp[s];
        slot(h, v, sh_m[s], sh_acc[s], sx, s - sx * G, ch, cv);
        if (ch) mp[s] = h;
        if (cv) vp[s] = v;
        sh_m[s] = __float_as_uint(h);
        sh_v[2 * s] = v;
      }
    }
  }
  __syncthreads();

  // ---- phase E: the scan, with the variance of each point's cell
  float z = 0.f, zv = va.var_max;
  bool kn = false;
  if (tid < PGTT_NSCAN) {
    const int slot = scan_slot(tid, sh_p, sh_i, a.sdx, a.sdy, a.res, G);
    if (slot >= 0) {
      z = __uint_as_float(sh_m[slot]);
      kn = z == z;
      if (kn) zv = reinterpret_cast<const float*>(sh_acc)[2 * slot];
    }
  }
  scan_min_and_write<kLanes>(z, kn, true, e, tid, sh_red, sh_est, a.est, a.known);
  if (tid < PGTT_NSCAN) va.est_var[(long)e * PGTT_NSCAN + tid] = zv;

  // ---- phase F: obs_out = obs with the scan rows replaced
  if (a.obs_out) {
    __syncthreads();
    assemble(a.obs_out, a.obs, sh_est, e, a.obs_dim, a.scan_row0, tid, kLanes);
  }
}

struct HoldArgs {
  const float* state; const float* obs; const float* done; const uint8_t* clear_mask; const int64_t* counter;
  float* map; int32_t* origin; float* est; uint8_t* known; float* obs_out;
  int N, G, obs_dim, scan_row0, clear_all, use_done, vec_map, every, force;
  float res, sdx, sdy;
};

constexpr int kHoldLanes = 128;                   // two waves per env: phase E's reduction, lane for lane
constexpr int kHoldEnvs = kLanes / kHoldLanes;    // envs per workgroup

__global__ void __launch_bounds__(kLanes) elevation_hold_kernel(HoldArgs a) {
  __shared__ float sh_p[kHoldEnvs][P_N];
  __shared__ int sh_i[kHoldEnvs][I_N];
  __shared__ float sh_est[kHoldEnvs][PGTT_NSCAN];
  __shared__ float sh_red[kHoldEnvs][2];
  if (fresh_call(a.counter, a.every, a.force)) return;                 // a fresh call: the gated elevation_kernel's
  const int tid = threadIdx.x, half = tid / kHoldLanes, lt = tid - half * kHoldLanes, G = a.G, GG = G * G;
  const int e = blockIdx.x * kHoldEnvs + half;
  const long N = a.N;
  const bool live = e < a.N;                                           // the last workgroup of an odd N: its second half only keeps the barriers

  // ---- the pose, the clear and the window (lane 0 of the env)
  if (live && lt == 0) {
    const Pose p = load_pose(a.state + e, N);
    sh_p[half][P_BASE + 0] = p.bx; sh_p[half][P_BASE + 1] = p.by;
    stage_yaw(p, sh_p[half]);
    const bool clear = cleared(a, e);
    int2 o;
    if (clear) {
      // a cleared env takes the cell of its current base position, as a tick's clear does
      o = make_int2(cell_of(p.bx, a.res), cell_of(p.by, a.res));
      a.origin[2 * (long)e] = o.x; a.origin[2 * (long)e + 1] = o.y;
    } else {
      o = stored_origin(a.origin, e);                                  // as the last fresh call left it
    }
    stage_window(window_of(o.x, o.y, G), sh_i[half]);
    sh_i[half][I_CLEAR] = clear ? 1 : 0;
  }
  __syncthreads();

  // ---- a cleared env: the whole map becomes NaN and nothing is known; any other env: the scan's cells are gathered from the map as it stands
  float z = 0.f;
  bool kn = false;
  if (live) {
    float* mp = a.map + (long)e * GG;
    if (sh_i[half][I_CLEAR]) {
      const float nanv = __uint_as_float(0x7fc00000u);
      if (a.vec_map) {
        const float4 n4 = make_float4(nanv, nanv, nanv, nanv);
        for (int s = 4 * lt; s < GG; s += 4 * kHoldLanes) *reinterpret_cast<float4*>(mp + s) = n4;
      } else {
        for (int s = lt; s < GG; s += kHoldLanes) mp[s] = nanv;
      }
    } else if (lt < PGTT_NSCAN) {
      const int slot = scan_slot(lt, sh_p[half], sh_i[half], a.sdx, a.sdy, a.res, G);
      if (slot >= 0) {
        z = mp[slot];
        kn = z == z;
      }
    }
  }

  // ---- the minimum over the known points, est and known: phase E
  scan_min_and_write<kHoldLanes>(z, kn, live, e, lt, sh_red[half], sh_est[half], a.est, a.known);

  // ---- obs_out = obs with the scan rows replaced: phase F
  if (a.obs_out) {
    __syncthreads();
    if (live) assemble(a.obs_out, a.obs, sh_est[half], e, a.obs_dim, a.scan_row0, lt, kHoldLanes);
  }
}

struct FillArgs {
  const float* state; const float* obs; const float* map; const int32_t* origin;
  float* est; uint8_t* dist; float* obs_out; float* map_out; uint8_t* dist_out;
  int N, G, obs_dim, scan_row0, passes, vec_map, vec_out, vec_dist;
  float res, sdx, sdy;
};

constexpr unsigned kNoKey = 0xffffffffu;          // above the key of every value but a NaN's, and a NaN is never a source
constexpr int kUnknown = 255;

__global__ void __launch_bounds__(kLanes) fill_kernel(FillArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned sh_k[];      // [(G + 2)^2] keys in WINDOW order inside a border, then as many D bytes
  __shared__ float sh_p[P_N];
  __shared__ int sh_i[I_N];
  __shared__ float sh_est[PGTT_NSCAN];
  __shared__ unsigned sh_red[2];
  __shared__ int sh_any[3];                                            // pass p raises [p % 3] and lowers [(p + 1) % 3]: nobody still reads that one
  const int e = blockIdx.x, tid = threadIdx.x, G = a.G, GG = G * G, S = G + 2;
  const long N = a.N;
  unsigned char* sh_d = reinterpret_cast<unsigned char*>(sh_k + S * S);
  // the window of the origin as the tick left it.  Every lane forms it (two broadcast reads), so the load needs no barrier in front of it
  const int2 o = stored_origin(a.origin, e);
  const Window win = window_of(o.x, o.y, G);
  // slot (sx, sy) -> its place in the bordered window: row (sx - lmx) mod G, column (sy - lmy) mod G, both + 1
  auto place = [&](int sx, int sy) {
    int wa = sx - win.lmx, wb = sy - win.lmy;
    wa += wa < 0 ? G : 0; wb += wb < 0 ? G : 0;
    return (wa + 1) * S + wb + 1;
  };

  // ---- load: the pose (lane 0); the border, which is never a source and never filled; the keys and D of the map's slots
  if (tid == 0) {
    const Pose p = load_pose(a.state + e, N);
    sh_p[P_BASE + 0] = p.bx; sh_p[P_BASE + 1] = p.by;
    stage_yaw(p, sh_p);
    stage_window(win, sh_i);
    sh_any[0] = 0; sh_any[1] = 0; sh_any[2] = 0;
  }
  for (int i = tid; i < S; i += kLanes) {
    const int edge[4] = {i, (S - 1) * S + i, i * S, i * S + S - 1};
#pragma unroll
    for (int k = 0; k < 4; k++) { sh_k[edge[k]] = kNoKey; sh_d[edge[k]] = kUnknown; }
  }
  {
    const float* mp = a.map + (long)e * GG;
    auto put = [&](float h, int sx, int sy) {
      const int c = place(sx, sy);
      sh_k[c] = h != h ? kNoKey : key_of(h);
      sh_d[c] = h != h ? kUnknown : 0;
    };
    if (a.vec_map) {
      for (int s = 4 * tid; s < GG; s += 4 * kLanes) {
        const float4 hv = *reinterpret_cast<const float4*>(mp + s);
        int sx = s / G, sy = s - sx * G;
        const float h[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
          put(h[k], sx, sy);
          sy++;
          if (sy == G) { sy = 0; sx++; }
        }
      }
    } else {
      for (int s = tid; s < GG; s += kLanes) { const int sx = s / G; put(mp[s], sx, s - sx * G); }
    }
  }
  __syncthreads();

  // ---- the passes: eight rows of 32 lanes walk the window.  A hole reads its eight neighbours' keys; the border and the holes read kNoKey, so a
  // hole with nothing around it costs eight reads and no read of D.  A neighbour that holds a key is a source iff its D < p: one filled in this pass
  // reads D = p, or still 255, and is none either way - so W and D need one barrier per pass and no atomics.
  {
    const int tx = tid & 31, ty = tid >> 5;
    for (int p = 1; p <= a.passes; p++) {
      if (tid == 0) sh_any[(p + 1) % 3] = 0;
      bool filled = false;
      for (int wa = ty; wa < G; wa += kLanes / 32) {
        for (int wb = tx; wb < G; wb += 32) {
          const int c = (wa + 1) * S + wb + 1;                         // S + 1 <= c <= S * S - S - 2: every neighbour is inside [0, S * S)
          if (sh_k[c] != kNoKey) continue;
          const int nb[8] = {c - S - 1, c - S, c - S + 1, c - 1, c + 1, c + S - 1, c + S, c + S + 1};
          unsigned best = kNoKey;
#pragma unroll
          for (int k = 0; k < 8; k++) {
            const unsigned key = sh_k[nb[k]];
            if (key != kNoKey && (int)sh_d[nb[k]] < p) best = min(best, key);
          }
          if (best != kNoKey) {
            sh_d[c] = (unsigned char)p;
            sh_k[c] = best;
            filled = true;
          }
        }
      }
      if (filled) sh_any[p % 3] = 1;
      __syncthreads();
      if (!sh_any[p % 3]) break;                                       // every lane reads the same word: the branch is uniform
    }
  }

  // ---- sample: the scan on the filled window
  unsigned zk = kNoKey;
  int d = kUnknown;
  if (tid < PGTT_NSCAN) {
    const int slot = scan_slot(tid, sh_p, sh_i, a.sdx, a.sdy, a.res, G);
    if (slot >= 0) {
      const int sx = slot / G, c = place(sx, slot - sx * G);
      d = sh_d[c];
      zk = d != kUnknown ? sh_k[c] : kNoKey;
    }
  }
  unsigned kmin = zk;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, off, 64));
  if (tid < 128 && (tid & 63) == 0) sh_red[tid >> 6] = kmin;
  __syncthreads();
  kmin = min(sh_red[0], sh_red[1]);
  if (tid < PGTT_NSCAN) {
    const float zmin = kmin != kNoKey ? value_of(kmin) : 0.f;
    const float es = (d != kUnknown ? value_of(zk) : zmin) - zmin;
    sh_est[tid] = es;
    a.est[(long)e * PGTT_NSCAN + tid] = es;
    a.dist[(long)e * PGTT_NSCAN + tid] = (uint8_t)d;
  }

  // ---- out: the dense window in the map's slot layout; obs_out
  if (a.map_out || a.dist_out) {
    float* mo = a.map_out ? a.map_out + (long)e * GG : nullptr;
    uint8_t* dd = a.dist_out ? a.dist_out + (long)e * GG : nullptr;
    const unsigned nanv = 0x7fc00000u;
    if (a.vec_out && a.vec_dist) {
      for (int s = 4 * tid; s < GG; s += 4 * kLanes) {
        int sx = s / G, sy = s - sx * G;
        unsigned w[4], d4 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int c = place(sx, sy);
          const unsigned dk = sh_d[c];
          w[k] = dk != kUnknown ? __float_as_uint(value_of(sh_k[c])) : nanv;
          d4 |= dk << (8 * k);
          sy++;
          if (sy == G) { sy = 0; sx++; }
        }
        if (mo) *reinterpret_cast<uint4*>(mo + s) = make_uint4(w[0], w[1], w[2], w[3]);
        if (dd) *reinterpret_cast<unsigned*>(dd + s) = d4;
      }
    } else {
      for (int s = tid; s < GG; s += kLanes) {
        const int sx = s / G, c = place(sx, s - sx * G);
        const unsigned dk = sh_d[c];
        if (mo) mo[s] = __uint_as_float(dk != kUnknown ? __float_as_uint(value_of(sh_k[c])) : nanv);
        if (dd) dd[s] = (uint8_t)dk;
      }
    }
  }
  if (a.obs_out) {
    __syncthreads();
    assemble(a.obs_out, a.obs, sh_est, e, a.obs_dim, a.scan_row0, tid, kLanes);
  }
}

// ---------------------------------------------------------------- odometry drift (pgtt_elevation_odometry): the estimated pose the map is bound to
struct OdoArgs {
  const float* state; const float* done; const uint8_t* clear_mask; const float* points; float* points_est;
  float* pose_est; float* odo; const int64_t* counter;
  int N, P, clear_all, use_done;
  unsigned k0, k1, gid0;                                       // the Philox key (seed lo, seed hi); (uint32) env_id_offset
  float dt, sigma_xy, sigma_z, sigma_yaw, yaw_bias, scale;
};

// the transform of an env's points, T_est o T_true^-1: the cosine and sine of the new psi, the true base position, the new position error
enum { T_COS = 0, T_SIN = 1, T_B = 2, T_E = 5, T_N = 8 };
constexpr int kOdoTile = 3 * kLanes;                           // floats of one tile of points: one point per lane

// env e's update in the header's order: reads its rows of `state` and `odo`, writes `odo` and its column of pose_est, leaves the transform in t
__device__ __forceinline__ void odo_update(const OdoArgs& a, int e, float* t) {
  const long N = a.N;
  const Pose p = load_pose<false>(a.state + e, N);                      // the quaternion as it stands
  const float bx = p.bx, by = p.by, bz = p.bz, qw = p.qw, qx = p.qx, qy = p.qy, qz = p.qz;
  float* o = a.odo + (size_t)e * PGTT_ELEVATION_ODO_WORDS;
  const bool clear = cleared(a, e);
  unsigned w0 = a.gid0 + (unsigned)e, w1 = (unsigned)a.counter[0], w2 = PGTT_RS_ODOMETRY, w3 = clear ? 1u : 0u;
  philox4x32_10(a.k0, a.k1, w0, w1, w2, w3);
  const float k24 = 1.0f / 16777216.0f;
  const float u0 = (float)(w0 >> 8) * k24, u1 = (float)(w1 >> 8) * k24, u2 = (float)(w2 >> 8) * k24, u3 = (float)(w3 >> 8) * k24;
  float ex = 0.f, ey = 0.f, ez = 0.f, psi = 0.f, se, be;
  if (clear) {
    se = a.scale * (2.f * u0 - 1.f);
    be = a.yaw_bias * (2.f * u1 - 1.f);
  } else {
    ex = o[0]; ey = o[1]; ez = o[2]; psi = o[3]; se = o[7]; be = o[8];
    const float Dx = bx - o[4], Dy = by - o[5], Dz = bz - o[6];
    const float sl = sqrtf(sqrtf(Dx * Dx + Dy * Dy + Dz * Dz));
    // 2 pi u as half turns: 2 u is exact
    float s01, c01, s23, c23, sp, cp;
    sincospif(2.f * u1, &s01, &c01);
    sincospif(2.f * u3, &s23, &c23);
    const float r01 = sqrtf(-2.f * logf(1.f - u0)), r23 = sqrtf(-2.f * logf(1.f - u2));
    const float nx = r01 * c01, ny = r01 * s01, nz = r23 * c23, npsi = r23 * s23;
    sincosf(psi, &sp, &cp);                                    // the OLD psi
    const float g = 1.f + se, Px = g * Dx, Py = g * Dy, Pz = g * Dz;
    ex += ((cp * Px - sp * Py) - Dx) + (a.sigma_xy * sl) * nx;
    ey += ((sp * Px + cp * Py) - Dy) + (a.sigma_xy * sl) * ny;
    ez += (Pz - Dz) + (a.sigma_z * sl) * nz;
    psi += be * a.dt + (a.sigma_yaw * sqrtf(a.dt)) * npsi;
  }
  o[0] = ex; o[1] = ey; o[2] = ez; o[3] = psi; o[4] = bx; o[5] = by; o[6] = bz; o[7] = se; o[8] = be; o[9] = 0.f; o[10] = 0.f; o[11] = 0.f;
  float sh, ch;
  sincosf(0.5f * psi, &sh, &ch);
  float* E = a.pose_est + e;
  E[0 * N] = bx + ex; E[1 * N] = by + ey; E[2 * N] = bz + ez;
  // qz(psi) (x) q, qz = (ch, 0, 0, sh)
  E[3 * N] = ch * qw - sh * qz; E[4 * N] = ch * qx - sh * qy; E[5 * N] = ch * qy + sh * qx; E[6 * N] = ch * qz + sh * qw;
  sincosf(psi, &t[T_SIN], &t[T_COS]);                          // the NEW psi
  t[T_B + 0] = bx; t[T_B + 1] = by; t[T_B + 2] = bz; t[T_E + 0] = ex; t[T_E + 1] = ey; t[T_E + 2] = ez;
}

// POINTS = false: one lane per env; state, pose_est rows are read and written coalesced.
// POINTS = true: one workgroup per env.  Lane 0 makes the env's update once and leaves the transform in LDS; then the env's 3 P floats stream
// through in tiles of 256 points: coalesced dword loads into LDS, one point per lane there (12-byte rows: a stride of 3 banks, no conflict),
// coalesced dword stores.  Every lane loads and stores the same LDS words of a tile, so two barriers per tile order everything.  No atomics.
template <bool POINTS>
__global__ void __launch_bounds__(kLanes) odometry_kernel(OdoArgs a) {
  const int tid = threadIdx.x;
  if constexpr (!POINTS) {
    const long e = (long)blockIdx.x * kLanes + tid;
    float t[T_N];
    if (e < a.N) odo_update(a, (int)e, t);
  } else {
    __shared__ float sh_t[T_N];
    __shared__ float sh_pts[kOdoTile];
    const int e = blockIdx.x;
    if (tid == 0) odo_update(a, e, sh_t);
    __syncthreads();
    const float c = sh_t[T_COS], s = sh_t[T_SIN];
    const float bx = sh_t[T_B + 0], by = sh_t[T_B + 1], ex = sh_t[T_E + 0], ey = sh_t[T_E + 1], ez = sh_t[T_E + 2];
    const long F = 3L * a.P;
    const float* src = a.points + (size_t)e * (size_t)F;
    float* dst = a.points_est + (size_t)e * (size_t)F;
    for (long f0 = 0; f0 < F; f0 += kOdoTile) {
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const long i = f0 + j * kLanes + tid;
        if (i < F) sh_pts[j * kLanes + tid] = src[i];
      }
      __syncthreads();
      if (f0 + 3 * tid < F) {                                  // F is a multiple of 3: the lane's point is whole
        float* p = sh_pts + 3 * tid;
        const float x = p[0], y = p[1], z = p[2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
          const float rx = x - bx, ry = y - by;
          p[0] = (x + ((c * rx - s * ry) - rx)) + ex;
          p[1] = (y + ((s * rx + c * ry) - ry)) + ey;
          p[2] = z + ez;                                       // Rz leaves z alone: (Rz r - r).z is 0
        } else {
          p[0] = p[1] = p[2] = __uint_as_float(0x7fc00000u);
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const long i = f0 + j * kLanes + tid;
        if (i < F) dst[i] = sh_pts[j * kLanes + tid];
      }
    }
  }
}

// behind the update: the epoch of the next call's draws
__global__ void __launch_bounds__(64) odometry_advance_kernel(int64_t* counter) {
  if (threadIdx.x == 0 && blockIdx.x == 0) counter[0] = counter[0] + 1;
}

// ---------------------------------------------------------------- sensor latency (pgtt_elevation_delayed): the ring of frames and their poses
struct PushArgs {
  const float* state; const float* src; const float* done; const uint8_t* clear_mask; const int64_t* counter;
  float* ring_data; float* ring_pose; int32_t* lat; int32_t* age; uint8_t* fused;
  int N, D, F, vec, clear_all, use_done, lat_lo, lat_hi;       // F: floats of one env's frame (H W, or 3 P)
  unsigned k0, k1, gid0;                                       // the Philox key (seed lo, seed hi); (uint32) env_id_offset
};

// latency_push_kernel: in front of the stamped tick, one workgroup of four waves per env (include/pgtt_elevation.h, "Sensor latency", steps 1 - 3).
// Lane 0 makes the env's clear and draw, stores the seven pose rows in slot w = counter mod D, counts the frame and says whether the frame that is
// due exists; the lanes copy the env's frame into its part of slot w, in 16-byte runs when the host found that the frame's size and both addresses
// allow (vec, the vec_img convention) and in dwords otherwise.  One source serves the image and the points: a frame is F floats.  The counter is
// only read: odometry_advance_kernel advances it behind the stamped tick.  No atomics, no LDS.
__global__ void __launch_bounds__(kLanes) latency_push_kernel(PushArgs a) {
  const int e = blockIdx.x, tid = threadIdx.x;
  const long N = a.N;
  const long long c = a.counter[0];
  const int w = floor_mod64(c, a.D);
  if (tid == 0) {
    const bool clear = cleared(a, e);
    int L = a.lat[e], age = a.age[e];
    if (clear) {
      unsigned w0 = a.gid0 + (unsigned)e, w1 = (unsigned)c, w2 = PGTT_RS_LATENCY, w3 = 0u;
      philox4x32_10(a.k0, a.k1, w0, w1, w2, w3);
      L = a.lat_lo + (int)(((unsigned long long)w0 * (unsigned long long)(a.lat_hi - a.lat_lo + 1)) >> 32);      // integers alone
      age = 0;
      a.lat[e] = L;
    }
    age = min(age + 1, a.D);
    a.age[e] = age;
    a.fused[e] = L < age ? 1 : 0;                                 // else the frame that is due predates the episode
    const float* S = a.state + e;
    float* R = a.ring_pose + (long)w * 7 * N + e;
#pragma unroll
    for (int r = 0; r < 7; r++) R[r * N] = S[(PGTT_S_QPOS + r) * N];
  }
  const float* src = a.src + (long)e * a.F;
  float* dst = a.ring_data + ((long)w * N + e) * a.F;
  if (a.vec) {
    for (int i = 4 * tid; i < a.F; i += 4 * kLanes) *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
  } else {
    for (int i = tid; i < a.F; i += kLanes) dst[i] = src[i];
  }
}

// ---------------------------------------------------------------- visibility clean-up (pgtt_elevation_visibility): rays forget contradicted cells
struct VisArgs {
  const float* state; const float* depth; const float* done; const uint8_t* clear_mask; const float* points; const int32_t* origin;
  float* map; float* var; int32_t* cleared; float* bound_out;
  int N, W, H, G, P, stride, clear_all, use_done, self_on, vec_map, vec_out;
  float near_m, far_m, res, tu, tv, margin, end_guard, sigmas;
  float mpos[3], mquat[4], self_half[3], spos[3];
};

// visibility_kernel<POINTS>: one workgroup of four waves per env, in the phases of the tick.  Dynamic LDS: sh_b[G G], the bound of every slot as the
// tick's order-preserving key, kNoKey = no sample fell into the slot (above the key of every value a sample can have: a NaN z is not a sample).
//   skip     every lane reads the env's clear flags alike: an env the tick will clear writes cleared = 0 and a NaN bound_out, and returns before any
//            barrier.
//   phase A  lane 0 stages the base pose, the sensor position, the camera basis (the image) and the window of the stored origin; the others set the
//            keys to kNoKey.
//   phase B  a per-lane ray loop, ray r = tid + 256 n of the strided pixels in row-major order (or of the strided points): the 64 lanes of a wave
//            hold neighbours of one image row, whose rays are about as long as each other, so a wave's lanes leave the sample loop together; the four
//            waves take the image's rows in turn, so each gets far rows and near rows alike.  Per ray one reciprocal of Lh; per sample two FMAs for
//            x and y, one for z, the cell, the window test and one ds_min_u32.
//   phase C  `map` (and `var`) stream through in 16-byte runs (dwords when G G is no multiple of 4), a run is written back only when one of its
//            slots was forgotten; bound_out streams out; the count is a wave reduction and one LDS exchange.
// LDS integer atomics only; no global atomics, no scratch.
template <bool POINTS>
__global__ void __launch_bounds__(kLanes) visibility_kernel(VisArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned sh_b[];      // [G * G]
  __shared__ float sh_p[P_N];
  __shared__ int sh_i[I_N];
  __shared__ int sh_cnt[kLanes / 64];
  const int e = blockIdx.x, tid = threadIdx.x, G = a.G, GG = G * G;
  const long N = a.N;
  const float nanv = __uint_as_float(0x7fc00000u);

  // ---- skip: the tick behind this call will clear the env
  if (a.clear_all || (a.clear_mask && a.clear_mask[e]) || (a.use_done && a.done && a.done[e] != 0.f)) {      // cleared(a, e), written out: DESIGN.md 31
    if (tid == 0) a.cleared[e] = 0;
    if (a.bound_out) {
      float* bo = a.bound_out + (long)e * GG;
      for (int s = tid; s < GG; s += kLanes) bo[s] = nanv;
    }
    return;
  }

  // ---- phase A: the pose, the sensor and the window (lane 0); the bounds start empty
  if (tid == 0) {
    const float* S = a.state + e;
    const float bx = S[(PGTT_S_QPOS + 0) * N], by = S[(PGTT_S_QPOS + 1) * N], bz = S[(PGTT_S_QPOS + 2) * N];
    float qw = S[(PGTT_S_QPOS + 3) * N], qx = S[(PGTT_S_QPOS + 4) * N], qy = S[(PGTT_S_QPOS + 5) * N], qz = S[(PGTT_S_QPOS + 6) * N];
    const float qn = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= qn; qx /= qn; qy /= qn; qz /= qn;
    const float r00 = qw * qw + qx * qx - qy * qy - qz * qz, r01 = 2.f * (qx * qy - qw * qz), r02 = 2.f * (qx * qz + qw * qy);
    const float r10 = 2.f * (qx * qy + qw * qz), r11 = qw * qw - qx * qx + qy * qy - qz * qz, r12 = 2.f * (qy * qz - qw * qx);
    const float r20 = 2.f * (qx * qz - qw * qy), r21 = 2.f * (qy * qz + qw * qx), r22 = qw * qw - qx * qx - qy * qy + qz * qz;
    sh_p[P_BASE + 0] = bx; sh_p[P_BASE + 1] = by; sh_p[P_BASE + 2] = bz;
    sh_p[P_RB + 0] = r00; sh_p[P_RB + 1] = r01; sh_p[P_RB + 2] = r02; sh_p[P_RB + 3] = r10; sh_p[P_RB + 4] = r11; sh_p[P_RB + 5] = r12;
    sh_p[P_RB + 6] = r20; sh_p[P_RB + 7] = r21; sh_p[P_RB + 8] = r22;
    // the sensor: the tick's camera position, or the points' sensor_pos, both in the base frame
    const float* mp = POINTS ? a.spos : a.mpos;
    sh_p[P_CAM + 0] = bx + r00 * mp[0] + r01 * mp[1] + r02 * mp[2];
    sh_p[P_CAM + 1] = by + r10 * mp[0] + r11 * mp[1] + r12 * mp[2];
    sh_p[P_CAM + 2] = bz + r20 * mp[0] + r21 * mp[1] + r22 * mp[2];
    if constexpr (!POINTS) {
      const float mw = a.mquat[0], mx = a.mquat[1], my = a.mquat[2], mz = a.mquat[3];
      const float cw = qw * mw - qx * mx - qy * my - qz * mz, cx = qw * mx + qx * mw + qy * mz - qz * my;
      const float cyq = qw * my - qx * mz + qy * mw + qz * mx, cz = qw * mz + qx * my - qy * mx + qz * mw;
      const float fx = cw * cw + cx * cx - cyq * cyq - cz * cz, fy = 2.f * (cx * cyq + cw * cz), fz = 2.f * (cx * cz - cw * cyq);
      const float ux = 2.f * (cx * cz + cw * cyq), uy = 2.f * (cyq * cz - cw * cx), uz = cw * cw - cx * cx - cyq * cyq + cz * cz;
      sh_p[P_FWD + 0] = fx; sh_p[P_FWD + 1] = fy; sh_p[P_FWD + 2] = fz;
      sh_p[P_UP + 0] = ux; sh_p[P_UP + 1] = uy; sh_p[P_UP + 2] = uz;
      sh_p[P_RIGHT + 0] = fy * uz - fz * uy; sh_p[P_RIGHT + 1] = fz * ux - fx * uz; sh_p[P_RIGHT + 2] = fx * uy - fy * ux;
    }
    // the origin as the last tick left it; one outside the tick's clamp (a map never ticked) is as far away as the clamp (fill_kernel's rule)
    const int ox = min(max(a.origin[2 * (long)e], -(1 << 30)), 1 << 30), oy = min(max(a.origin[2 * (long)e + 1], -(1 << 30)), 1 << 30);
    const int lox = ox - G / 2, loy = oy - G / 2;
    sh_i[I_LOX] = lox; sh_i[I_LOY] = loy; sh_i[I_LMX] = floor_mod(lox, G); sh_i[I_LMY] = floor_mod(loy, G);
  }
  for (int s = tid; s < GG; s += kLanes) sh_b[s] = kNoKey;
  __syncthreads();

  // ---- phase B: the rays
  {
    const float sx = sh_p[P_CAM + 0], sy = sh_p[P_CAM + 1], sz = sh_p[P_CAM + 2];
    const float bpx = uni(sh_p[P_BASE + 0]), bpy = uni(sh_p[P_BASE + 1]), bpz = uni(sh_p[P_BASE + 2]);
    const float b00 = uni(sh_p[P_RB + 0]), b01 = uni(sh_p[P_RB + 1]), b02 = uni(sh_p[P_RB + 2]), b10 = uni(sh_p[P_RB + 3]), b11 = uni(sh_p[P_RB + 4]);
    const float b12 = uni(sh_p[P_RB + 5]), b20 = uni(sh_p[P_RB + 6]), b21 = uni(sh_p[P_RB + 7]), b22 = uni(sh_p[P_RB + 8]);
    const int lox = sh_i[I_LOX], loy = sh_i[I_LOY], lmx = sh_i[I_LMX], lmy = sh_i[I_LMY];
    const float res = a.res, ires = 1.0f / a.res, end_guard = a.end_guard;
    const int kmax = 2 * G;
    // one ray from the sensor to the admitted end point p
    auto ray = [&](float px, float py, float pz) {
      if (a.self_on) {
        const float dx = px - bpx, dy = py - bpy, dz = pz - bpz;             // R^T (p - base): the tick's self filter
        const float lx = b00 * dx + b10 * dy + b20 * dz, ly = b01 * dx + b11 * dy + b21 * dz, lz = b02 * dx + b12 * dy + b22 * dz;
        if (fabsf(lx) <= a.self_half[0] && fabsf(ly) <= a.self_half[1] && fabsf(lz) <= a.self_half[2]) return;
      }
      const float dx = px - sx, dy = py - sy;
      const float Lh = hypotf(dx, dy), lim = Lh - end_guard;
      if (!(0.5f * res <= lim)) return;                                 // no sample, no division: Lh == 0, a NaN, a ray shorter than the first sample
      const float inv = 1.0f / Lh;
      const float ux = dx * inv, uy = dy * inv, uz = (pz - sz) * inv;
      for (int k = 0; k < kmax; k++) {
        const float rk = ((float)k + 0.5f) * res;
        if (!(rk <= lim)) break;
        const float x = fmaf(rk, ux, sx), y = fmaf(rk, uy, sy), z = fmaf(rk, uz, sz);
        const int relx = (int)fminf(fmaxf(floorf(x * ires), -kCellClamp), kCellClamp) - lox;
        const int rely = (int)fminf(fmaxf(floorf(y * ires), -kCellClamp), kCellClamp) - loy;
        if ((unsigned)relx >= (unsigned)G || (unsigned)rely >= (unsigned)G || !(z == z)) continue;
        int cx = relx + lmx, cy = rely + lmy;                           // (lo + rel) mod G
        cx -= cx >= G ? G : 0; cy -= cy >= G ? G : 0;
        atomicMin(&sh_b[cx * G + cy], key_of(z));
      }
    };
    const int stride = a.stride;
    if constexpr (POINTS) {
      const float* pts = a.points + (long)e * a.P * 3;
      const int nray = (a.P + stride - 1) / stride;
      for (int r = tid; r < nray; r += kLanes) {
        const long k = (long)r * stride;
        const float px = pts[3 * k], py = pts[3 * k + 1], pz = pts[3 * k + 2];
        if (!(fabsf(px) < INFINITY && fabsf(py) < INFINITY && fabsf(pz) < INFINITY)) continue;      // the tick's validity test
        ray(px, py, pz);
      }
    } else {
      const float fx = sh_p[P_FWD + 0], fy = sh_p[P_FWD + 1], fz = sh_p[P_FWD + 2];
      const float rx = sh_p[P_RIGHT + 0], ry = sh_p[P_RIGHT + 1], rz = sh_p[P_RIGHT + 2];
      const float ux = sh_p[P_UP + 0], uy = sh_p[P_UP + 1], uz = sh_p[P_UP + 2];
      const int W = a.W, nw = (a.W + stride - 1) / stride, nray = nw * ((a.H + stride - 1) / stride);
      const float* img = a.depth + (long)e * a.W * a.H;
      for (int r = tid; r < nray; r += kLanes) {
        const int ri = r / nw, i = ri * stride, j = (r - ri * nw) * stride;
        const float d = img[i * W + j];
        if (!(d > a.near_m && d < a.far_m)) continue;                  // the tick's validity test and its unprojection
        const float u = (2.f * ((float)j + 0.5f) / (float)W - 1.f) * a.tu, v = (1.f - 2.f * ((float)i + 0.5f) / (float)a.H) * a.tv;
        ray(sx + d * (fx + u * rx + v * ux), sy + d * (fy + u * ry + v * uy), sz + d * (fz + u * rz + v * uz));
      }
    }
  }
  __syncthreads();

  // ---- phase C: the map (and the variance layer) stream through; the bound layer streams out
  int count = 0;
  {
    float* mp = a.map + (long)e * GG;
    float* vp = a.var ? a.var + (long)e * GG : nullptr;
    float* bo = a.bound_out ? a.bound_out + (long)e * GG : nullptr;
    const float margin = a.margin, sigmas = a.sigmas;
    // one slot: h (and v) in and out; -> true when the cell is forgotten
    auto slot = [&](float& h, float& v, unsigned key) {
      if (key == kNoKey || h != h) return false;
      const float t = vp ? h - sigmas * sqrtf(v) : h;
      if (!(t > value_of(key) + margin)) return false;
      h = nanv; v = nanv;
      return true;
    };
    if (a.vec_map) {
      for (int s = 4 * tid; s < GG; s += 4 * kLanes) {
        const float4 hv = *reinterpret_cast<const float4*>(mp + s);
        float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vp) vv = *reinterpret_cast<const float4*>(vp + s);
        const uint4 kv = *reinterpret_cast<const uint4*>(sh_b + s);
        float h[4] = {hv.x, hv.y, hv.z, hv.w}, v[4] = {vv.x, vv.y, vv.z, vv.w};
        const unsigned k4[4] = {kv.x, kv.y, kv.z, kv.w};
        int n = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) n += slot(h[k], v[k], k4[k]) ? 1 : 0;
        if (n) {
          *reinterpret_cast<float4*>(mp + s) = make_float4(h[0], h[1], h[2], h[3]);
          if (vp) *reinterpret_cast<float4*>(vp + s) = make_float4(v[0], v[1], v[2], v[3]);
          count += n;
        }
      }
    } else {
      for (int s = tid; s < GG; s += kLanes) {
        float h = mp[s], v = vp ? vp[s] : 0.f;
        if (slot(h, v, sh_b[s])) {
          mp[s] = h;
          if (vp) vp[s] = v;
          count++;
        }
      }
    }
    if (bo) {
      if (a.vec_out) {
        for (int s = 4 * tid; s < GG; s += 4 * kLanes) {
          const uint4 kv = *reinterpret_cast<const uint4*>(sh_b + s);
          *reinterpret_cast<float4*>(bo + s) = make_float4(kv.x == kNoKey ? nanv : value_of(kv.x), kv.y == kNoKey ? nanv : value_of(kv.y),
                                                            kv.z == kNoKey ? nanv : value_of(kv.z), kv.w == kNoKey ? nanv : value_of(kv.w));
        }
      } else {
        for (int s = tid; s < GG; s += kLanes) { const unsigned k = sh_b[s]; bo[s] = k == kNoKey ? nanv : value_of(k); }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
  if ((tid & 63) == 0) sh_cnt[tid >> 6] = count;
  __syncthreads();
  if (tid == 0) a.cleared[e] = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
}

// the config's checks; `who` prefixes the message
int resolve(const PgttElevationConfig* c, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (!c) return fail(PGTT_E_ARG, p + "null config");
  if (c->width < 1 || c->width > PGTT_ELEVATION_MAX_DIM || c->height < 1 || c->height > PGTT_ELEVATION_MAX_DIM)
    return fail(PGTT_E_ARG, p + "width and height must be in [1, PGTT_ELEVATION_MAX_DIM]");
  if (!(c->fovy_deg > 0.f && c->fovy_deg < 180.f)) return fail(PGTT_E_ARG, p + "fovy_deg must be in (0, 180)");
  if (!(c->near > 0.f) || !(c->near < c->far) || !std::isfinite(c->far)) return fail(PGTT_E_ARG, p + "need 0 < near < far, finite");
  if (c->mount_body != 0) return fail(PGTT_E_ARG, p + "only a camera on the torso is supported (mount_body == 0)");
  double qn = 0.0;
  for (int i = 0; i < 4; i++) qn += (double)c->mount_quat[i] * c->mount_quat[i];
  if (!(qn > 0.0) || !std::isfinite(qn)) return fail(PGTT_E_ARG, p + "mount_quat must be a non-zero quaternion");
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(c->mount_pos[i])) return fail(PGTT_E_ARG, p + "mount_pos must be finite");
  if (c->grid < PGTT_ELEVATION_MIN_GRID || c->grid > PGTT_ELEVATION_MAX_GRID) return fail(PGTT_E_ARG, p + "grid must be in [8, 96]");
  if (!(c->res > 0.f) || !std::isfinite(c->res)) return fail(PGTT_E_ARG, p + "res must be positive and finite");
  if (!(c->alpha > 0.f && c->alpha <= 1.f)) return fail(PGTT_E_ARG, p + "alpha must be in (0, 1]");
  for (int i = 0; i < 3; i++)
    if (!(c->self_half[i] >= 0.f) || !std::isfinite(c->self_half[i])) return fail(PGTT_E_ARG, p + "self_half must be >= 0 and finite");
  if (!std::isfinite(c->scan_dist_x) || !std::isfinite(c->scan_dist_y)) return fail(PGTT_E_ARG, p + "scan_dist_x and scan_dist_y must be finite");
  if (c->obs_dim < 1 || c->scan_row0 < 0 || (long)c->scan_row0 + PGTT_NSCAN > c->obs_dim) return fail(PGTT_E_ARG, p + "need 0 <= scan_row0 and scan_row0 + 117 <= obs_dim");
  return PGTT_OK;
}

}  // namespace

struct pgtt_elevation_map {
  int device = 0, num_envs = 0;
  PgttElevationConfig cfg{};
  PgttElevationBuffers buf{};
  bool bound = false;
  const float* points = nullptr;         // pgtt_elevation_bind_points; nullptr after pgtt_elevation_bind
  int P = 0;
  PgttElevationFill fill{};              // pgtt_elevation_bind_fill; kept by the other two binds
  int passes = 0;                        // 0 = no fill bound
  const int64_t* counter = nullptr;      // pgtt_elevation_bind_rate; kept by the other binds
  int every = 0;                         // 0 = no rate bound
  PgttElevationVar var{};                // pgtt_elevation_bind_var; kept by the other binds
  bool has_var = false;
  PgttElevationOdometry odo{};           // pgtt_elevation_bind_odometry; kept by the other binds
  bool has_odo = false;
  PgttElevationVisibility vis{};         // pgtt_elevation_bind_visibility; kept by the other binds
  bool has_vis = false;
  PgttElevationLatency lat{};            // pgtt_elevation_bind_latency; kept by the other binds
  bool has_lat = false;
};

namespace {

// what both bind calls ask of the buffers; need_depth: pgtt_elevation_bind's source, the depth image, is required with them
int check_buffers(const PgttElevationBuffers* bufs, const char* who, bool need_depth) {
  const std::string p = std::string(who) + ": ";
  if (!bufs->state || (need_depth && !bufs->depth) || !bufs->map || !bufs->origin || !bufs->est || !bufs->known)
    return fail(PGTT_E_ARG, p + (need_depth ? "state, depth, map, origin, est and known are required" : "state, map, origin, est and known are required"));
  if (bufs->obs_out && !bufs->obs) return fail(PGTT_E_ARG, p + "obs is required with obs_out");
  return PGTT_OK;
}

// may `count` floats per env stream in 16-byte runs: every env's block then starts on a 16-byte boundary of p0 (and p1); a NULL pointer counts as
// aligned, it is not streamed
bool runs16(long count, const void* p0, const void* p1 = nullptr) { return count % 4 == 0 && ((uintptr_t)p0 & 15) == 0 && ((uintptr_t)p1 & 15) == 0; }

// the config's camera and self filter as the kernels take them: ElevArgs and VisArgs, the same fields
template <class A>
void camera_args(const PgttElevationConfig& c, A& a) {
  a.W = c.width; a.H = c.height;
  a.self_on = (c.self_half[0] != 0.f || c.self_half[1] != 0.f || c.self_half[2] != 0.f) ? 1 : 0;
  const double th = std::tan(0.5 * (double)c.fovy_deg * 3.14159265358979323846 / 180.0);
  a.near_m = c.near; a.far_m = c.far; a.tu = (float)(th * c.width / c.height); a.tv = (float)th;
  for (int i = 0; i < 3; i++) { a.mpos[i] = c.mount_pos[i]; a.self_half[i] = c.self_half[i]; }
  for (int i = 0; i < 4; i++) a.mquat[i] = c.mount_quat[i];
}

// the kernel arguments of one tick on the handle's config and buffers
ElevArgs tick_args(const pgtt_elevation_map* h, const uint8_t* clear_mask, int clear_all, int use_done) {
  const PgttElevationConfig& c = h->cfg;
  const PgttElevationBuffers& b = h->buf;
  ElevArgs a{};
  a.state = b.state; a.depth = b.depth; a.obs = b.obs; a.done = b.done; a.clear_mask = clear_mask;
  a.map = b.map; a.origin = b.origin; a.est = b.est; a.known = b.known; a.obs_out = b.obs_out;
  a.N = h->num_envs; a.G = c.grid; a.obs_dim = c.obs_dim; a.scan_row0 = c.scan_row0;
  a.clear_all = clear_all ? 1 : 0; a.use_done = use_done ? 1 : 0;
  camera_args(c, a);
  a.vec_map = runs16(c.grid * c.grid, b.map) ? 1 : 0;
  a.vec_img = runs16(c.width * c.height, b.depth) ? 1 : 0;
  a.res = c.res; a.alpha = c.alpha; a.sdx = c.scan_dist_x; a.sdy = c.scan_dist_y;
  a.points = h->points; a.P = h->P;
  return a;
}

// one tick from the image (points = false) or from the bound points; follow: the gated tick and the hold behind the sensor's counter, `force` as
// the sensor's call was given
int launch(pgtt_elevation_map* h, bool points, const uint8_t* clear_mask, int clear_all, int use_done, void* stream, bool follow = false, int force = 0) {
  HIP_TRY(hipSetDevice(h->device));
  const PgttElevationConfig& c = h->cfg;
  const PgttElevationBuffers& b = h->buf;
  ElevArgs a = tick_args(h, clear_mask, clear_all, use_done);
  const size_t lds = (size_t)c.grid * c.grid * sizeof(unsigned);
  if (follow) {
    a.counter = h->counter; a.every = h->every; a.force = force ? 1 : 0;
    if (points) hipLaunchKernelGGL((elevation_kernel<true, true>), dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((elevation_kernel<false, true>), dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    HoldArgs o{};
    o.state = b.state; o.obs = b.obs; o.done = b.done; o.clear_mask = clear_mask; o.counter = h->counter;
    o.map = b.map; o.origin = b.origin; o.est = b.est; o.known = b.known; o.obs_out = b.obs_out;
    o.N = h->num_envs; o.G = c.grid; o.obs_dim = c.obs_dim; o.scan_row0 = c.scan_row0; o.clear_all = a.clear_all; o.use_done = a.use_done;
    o.vec_map = a.vec_map; o.every = h->every; o.force = a.force;
    o.res = c.res; o.sdx = c.scan_dist_x; o.sdy = c.scan_dist_y;
    hipLaunchKernelGGL(elevation_hold_kernel, dim3((h->num_envs + kHoldEnvs - 1) / kHoldEnvs), dim3(kLanes), 0, (hipStream_t)stream, o);
  } else if (points) {
    hipLaunchKernelGGL(elevation_kernel<true>, dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(elevation_kernel<false>, dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, a);
  }
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

// the variance settings' ranges; `who` prefixes the message
int resolve_var(const PgttElevationVar* v, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (!v) return fail(PGTT_E_ARG, p + "null settings");
  const float f[6] = {v->sigma0, v->sigma_rel, v->process, v->gate, v->band, v->var_max};
  for (int i = 0; i < 6; i++)
    if (!std::isfinite(f[i])) return fail(PGTT_E_ARG, p + "sigma0, sigma_rel, process, gate, band and var_max must be finite");
  if (!(v->sigma0 >= 0.f) || !(v->sigma_rel >= 0.f) || !(v->sigma0 + v->sigma_rel > 0.f))
    return fail(PGTT_E_ARG, p + "need sigma0 >= 0, sigma_rel >= 0 and sigma0 + sigma_rel > 0");
  if (!(v->process >= 0.f)) return fail(PGTT_E_ARG, p + "process must be >= 0");
  if (!(v->gate > 0.f)) return fail(PGTT_E_ARG, p + "gate must be > 0");
  if (!(v->band >= 0.f && v->band <= PGTT_ELEVATION_MAX_BAND)) return fail(PGTT_E_ARG, p + "band must be in [0, PGTT_ELEVATION_MAX_BAND = 0.5]");
  if (v->max_count < 1) return fail(PGTT_E_ARG, p + "max_count must be >= 1");
  if (!(v->var_max > 0.f)) return fail(PGTT_E_ARG, p + "var_max must be > 0");
  return PGTT_OK;
}

// one variance tick from the image (points = false) or from the bound points: one launch
int launch_var(pgtt_elevation_map* h, bool points, const uint8_t* clear_mask, int clear_all, int use_done, void* stream) {
  HIP_TRY(hipSetDevice(h->device));
  const PgttElevationConfig& c = h->cfg;
  const PgttElevationVar& v = h->var;
  VarArgs va{};
  va.a = tick_args(h, clear_mask, clear_all, use_done);
  va.a.vec_map = runs16(c.grid * c.grid, h->buf.map, v.var) ? 1 : 0;      // map and var stream together
  va.var = v.var; va.est_var = v.est_var;
  va.s0sq = (float)((double)v.sigma0 * v.sigma0); va.srsq = (float)((double)v.sigma_rel * v.sigma_rel); va.gate2 = (float)((double)v.gate * v.gate);
  va.process = v.process; va.band = v.band; va.var_max = v.var_max; va.max_count = v.max_count;
  const size_t lds = (size_t)c.grid * c.grid * (sizeof(unsigned long long) + sizeof(unsigned));
  if (points) hipLaunchKernelGGL(elevation_var_kernel<true>, dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, va);
  else hipLaunchKernelGGL(elevation_var_kernel<false>, dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, va);
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

// the odometry settings' ranges; `who` prefixes the message
int resolve_odometry(const PgttElevationOdometry* o, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (!o) return fail(PGTT_E_ARG, p + "null settings");
  const float f[6] = {o->dt, o->sigma_xy, o->sigma_z, o->sigma_yaw, o->yaw_bias, o->scale};
  for (int i = 0; i < 6; i++)
    if (!std::isfinite(f[i])) return fail(PGTT_E_ARG, p + "dt, sigma_xy, sigma_z, sigma_yaw, yaw_bias and scale must be finite");
  if (!(o->dt > 0.f)) return fail(PGTT_E_ARG, p + "dt must be > 0");
  if (!(o->sigma_xy >= 0.f) || !(o->sigma_z >= 0.f) || !(o->sigma_yaw >= 0.f) || !(o->yaw_bias >= 0.f))
    return fail(PGTT_E_ARG, p + "sigma_xy, sigma_z, sigma_yaw and yaw_bias must be >= 0");
  if (!(o->scale >= 0.f && o->scale < 1.f)) return fail(PGTT_E_ARG, p + "scale must be in [0, 1)");
  return PGTT_OK;
}

// the visibility settings' ranges; `who` prefixes the message
int resolve_visibility(const PgttElevationVisibility* v, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (!v) return fail(PGTT_E_ARG, p + "null settings");
  const float f[6] = {v->margin, v->end_guard, v->sigmas, v->sensor_pos[0], v->sensor_pos[1], v->sensor_pos[2]};
  for (int i = 0; i < 6; i++)
    if (!std::isfinite(f[i])) return fail(PGTT_E_ARG, p + "margin, end_guard, sigmas and sensor_pos must be finite");
  if (!(v->margin > 0.f)) return fail(PGTT_E_ARG, p + "margin must be > 0");
  if (!(v->end_guard >= 0.f)) return fail(PGTT_E_ARG, p + "end_guard must be >= 0");
  if (v->stride < 1) return fail(PGTT_E_ARG, p + "stride must be >= 1");
  if (!(v->sigmas >= 0.f)) return fail(PGTT_E_ARG, p + "sigmas must be >= 0");
  return PGTT_OK;
}

// the latency settings' ranges; `who` prefixes the message
int resolve_latency(const PgttElevationLatency* l, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (!l) return fail(PGTT_E_ARG, p + "null settings");
  if (l->lat_lo < 0 || l->lat_lo > l->lat_hi || l->lat_hi > PGTT_ELEVATION_MAX_LATENCY)
    return fail(PGTT_E_ARG, p + "need 0 <= lat_lo <= lat_hi <= PGTT_ELEVATION_MAX_LATENCY = 8");
  if (l->D < l->lat_hi + 1 || l->D > PGTT_ELEVATION_MAX_LATENCY + 1) return fail(PGTT_E_ARG, p + "D must be in [lat_hi + 1, PGTT_ELEVATION_MAX_LATENCY + 1]");
  return PGTT_OK;
}

}  // namespace

extern "C" {

int pgtt_elevation_sizeof_latency(void) { return (int)sizeof(PgttElevationLatency); }

int pgtt_elevation_check_latency(const PgttElevationLatency* l) { return resolve_latency(l, "pgtt_elevation_check_latency"); }

int pgtt_elevation_bind_latency(pgtt_elevation_handle h, const PgttElevationLatency* l) {
  if (!h || !l) return fail(PGTT_E_ARG, "pgtt_elevation_bind_latency: null argument");
  if (!l->ring_data || !l->ring_pose || !l->lat || !l->age || !l->fused || !l->counter)
    return fail(PGTT_E_ARG, "pgtt_elevation_bind_latency: ring_data, ring_pose, lat, age, fused and counter are required");
  if (int rc = resolve_latency(l, "pgtt_elevation_bind_latency")) return rc;
  h->lat = *l;
  h->has_lat = true;
  return PGTT_OK;
}

int pgtt_elevation_delayed(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation_delayed: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_elevation_delayed: no buffers bound (pgtt_elevation_bind or pgtt_elevation_bind_points first)");
  if (!h->has_lat) return fail(PGTT_E_STATE, "pgtt_elevation_delayed: no latency bound (pgtt_elevation_bind_latency first)");
  HIP_TRY(hipSetDevice(h->device));
  const PgttElevationConfig& c = h->cfg;
  const PgttElevationLatency& l = h->lat;
  const bool points = h->points != nullptr;                            // the source: whichever bind was made last
  ElevArgs a = tick_args(h, clear_mask, clear_all, use_done);
  PushArgs p{};
  p.state = h->buf.state; p.src = points ? h->points : h->buf.depth; p.done = h->buf.done; p.clear_mask = clear_mask; p.counter = l.counter;
  p.ring_data = l.ring_data; p.ring_pose = l.ring_pose; p.lat = l.lat; p.age = l.age; p.fused = l.fused;
  p.N = h->num_envs; p.D = l.D; p.F = points ? 3 * h->P : c.width * c.height;
  p.clear_all = a.clear_all; p.use_done = a.use_done; p.lat_lo = l.lat_lo; p.lat_hi = l.lat_hi;
  p.k0 = (unsigned)l.seed; p.k1 = (unsigned)(l.seed >> 32); p.gid0 = (unsigned)l.env_id_offset;
  const bool ring16 = runs16(p.F, l.ring_data);
  p.vec = (ring16 && ((uintptr_t)p.src & 15) == 0) ? 1 : 0;            // the frame's runs: in the ring and in the source
  hipLaunchKernelGGL(latency_push_kernel, dim3(h->num_envs), dim3(kLanes), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  a.ring_data = l.ring_data; a.ring_pose = l.ring_pose; a.lat = l.lat; a.fused = l.fused; a.lat_counter = l.counter; a.D = l.D;
  a.vec_img = ring16 ? 1 : 0;                                          // the image is the ring's now
  const size_t lds = (size_t)c.grid * c.grid * sizeof(unsigned);
  if (points) hipLaunchKernelGGL((elevation_kernel<true, false, true>), dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((elevation_kernel<false, false, true>), dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(odometry_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, l.counter);
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

PGTT_SIDE_EXPORTS(elevation, ELEVATION)
int pgtt_elevation_sizeof_visibility(void) { return (int)sizeof(PgttElevationVisibility); }

int pgtt_elevation_check_visibility(const PgttElevationVisibility* v) { return resolve_visibility(v, "pgtt_elevation_check_visibility"); }

int pgtt_elevation_bind_visibility(pgtt_elevation_handle h, const PgttElevationVisibility* v) {
  if (!h || !v) return fail(PGTT_E_ARG, "pgtt_elevation_bind_visibility: null argument");
  if (!v->cleared) return fail(PGTT_E_ARG, "pgtt_elevation_bind_visibility: cleared is required");
  if (int rc = resolve_visibility(v, "pgtt_elevation_bind_visibility")) return rc;
  h->vis = *v;
  h->has_vis = true;
  return PGTT_OK;
}

int pgtt_elevation_visibility(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation_visibility: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_elevation_visibility: no buffers bound (pgtt_elevation_bind or pgtt_elevation_bind_points first)");
  if (!h->has_vis) return fail(PGTT_E_STATE, "pgtt_elevation_visibility: no visibility bound (pgtt_elevation_bind_visibility first)");
  HIP_TRY(hipSetDevice(h->device));
  const PgttElevationConfig& c = h->cfg;
  const PgttElevationBuffers& b = h->buf;
  const PgttElevationVisibility& v = h->vis;
  const bool points = h->points != nullptr;                            // the source: whichever bind was made last
  VisArgs a{};
  a.state = b.state; a.depth = b.depth; a.done = b.done; a.clear_mask = clear_mask; a.points = h->points; a.origin = b.origin;
  a.map = b.map; a.var = h->has_var ? h->var.var : nullptr; a.cleared = v.cleared; a.bound_out = v.bound_out;
  a.N = h->num_envs; a.G = c.grid; a.P = h->P; a.stride = v.stride;
  a.clear_all = clear_all ? 1 : 0; a.use_done = use_done ? 1 : 0;
  camera_args(c, a);
  a.vec_map = runs16(c.grid * c.grid, b.map, a.var) ? 1 : 0;           // map and var stream together
  a.vec_out = runs16(c.grid * c.grid, v.bound_out) ? 1 : 0;
  a.res = c.res; a.margin = v.margin; a.end_guard = v.end_guard; a.sigmas = v.sigmas;
  for (int i = 0; i < 3; i++) a.spos[i] = v.sensor_pos[i];
  const size_t lds = (size_t)c.grid * c.grid * sizeof(unsigned);
  if (points) hipLaunchKernelGGL(visibility_kernel<true>, dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(visibility_kernel<false>, dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

int pgtt_elevation_sizeof_odometry(void) { return (int)sizeof(PgttElevationOdometry); }

int pgtt_elevation_check_odometry(const PgttElevationOdometry* o) { return resolve_odometry(o, "pgtt_elevation_check_odometry"); }

int pgtt_elevation_bind_odometry(pgtt_elevation_handle h, const PgttElevationOdometry* o) {
  if (!h || !o) return fail(PGTT_E_ARG, "pgtt_elevation_bind_odometry: null argument");
  if (!o->state || !o->pose_est || !o->odo || !o->counter) return fail(PGTT_E_ARG, "pgtt_elevation_bind_odometry: state, pose_est, odo and counter are required");
  if ((o->points != nullptr) != (o->points_est != nullptr)) return fail(PGTT_E_ARG, "pgtt_elevation_bind_odometry: points and points_est come together");
  if (o->points && o->P < 1) return fail(PGTT_E_ARG, "pgtt_elevation_bind_odometry: points need P >= 1");
  if (int rc = resolve_odometry(o, "pgtt_elevation_bind_odometry")) return rc;
  h->odo = *o;
  h->has_odo = true;
  return PGTT_OK;
}

int pgtt_elevation_odometry(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation_odometry: null handle");
  if (!h->has_odo) return fail(PGTT_E_STATE, "pgtt_elevation_odometry: no odometry bound (pgtt_elevation_bind_odometry first)");
  HIP_TRY(hipSetDevice(h->device));
  const PgttElevationOdometry& o = h->odo;
  OdoArgs a{};
  a.state = o.state; a.done = o.done; a.clear_mask = clear_mask; a.points = o.points; a.points_est = o.points_est;
  a.pose_est = o.pose_est; a.odo = o.odo; a.counter = o.counter;
  a.N = h->num_envs; a.P = o.P; a.clear_all = clear_all ? 1 : 0; a.use_done = use_done ? 1 : 0;
  a.k0 = (unsigned)o.seed; a.k1 = (unsigned)(o.seed >> 32); a.gid0 = (unsigned)o.env_id_offset;
  a.dt = o.dt; a.sigma_xy = o.sigma_xy; a.sigma_z = o.sigma_z; a.sigma_yaw = o.sigma_yaw; a.yaw_bias = o.yaw_bias; a.scale = o.scale;
  if (o.points) hipLaunchKernelGGL(odometry_kernel<true>, dim3(h->num_envs), dim3(kLanes), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(odometry_kernel<false>, dim3((h->num_envs + kLanes - 1) / kLanes), dim3(kLanes), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(odometry_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, o.counter);
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

int pgtt_elevation_sizeof_var(void) { return (int)sizeof(PgttElevationVar); }

int pgtt_elevation_check_var(const PgttElevationVar* v) { return resolve_var(v, "pgtt_elevation_check_var"); }

int pgtt_elevation_bind_var(pgtt_elevation_handle h, const PgttElevationVar* v) {
  if (!h || !v) return fail(PGTT_E_ARG, "pgtt_elevation_bind_var: null argument");
  if (!v->var || !v->est_var) return fail(PGTT_E_ARG, "pgtt_elevation_bind_var: var and est_var are required");
  if (int rc = resolve_var(v, "pgtt_elevation_bind_var")) return rc;
  if (h->cfg.grid > PGTT_ELEVATION_VAR_MAX_GRID)
    return fail(PGTT_E_ARG, "pgtt_elevation_bind_var: the variance tick supports grid <= PGTT_ELEVATION_VAR_MAX_GRID = 64 (12 bytes of LDS per slot)");
  h->var = *v;
  h->has_var = true;
  return PGTT_OK;
}

int pgtt_elevation_var(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation_var: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_elevation_var: no buffers bound (pgtt_elevation_bind first)");
  if (!h->buf.depth) return fail(PGTT_E_STATE, "pgtt_elevation_var: the handle was bound without a depth image (pgtt_elevation_bind_points with depth == NULL)");
  if (!h->has_var) return fail(PGTT_E_STATE, "pgtt_elevation_var: no variance bound (pgtt_elevation_bind_var first)");
  return launch_var(h, false, clear_mask, clear_all, use_done, stream);
}

int pgtt_elevation_var_points(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation_var_points: null handle");
  if (!h->points) return fail(PGTT_E_STATE, "pgtt_elevation_var_points: no points bound (pgtt_elevation_bind_points first)");
  if (!h->has_var) return fail(PGTT_E_STATE, "pgtt_elevation_var_points: no variance bound (pgtt_elevation_bind_var first)");
  return launch_var(h, true, clear_mask, clear_all, use_done, stream);
}
int pgtt_elevation_sizeof_config(void) { return (int)sizeof(PgttElevationConfig); }
int pgtt_elevation_sizeof_buffers(void) { return (int)sizeof(PgttElevationBuffers); }
int pgtt_elevation_sizeof_fill(void) { return (int)sizeof(PgttElevationFill); }

int pgtt_elevation_check(const PgttElevationConfig* cfg) { return resolve(cfg, "pgtt_elevation_check"); }

int pgtt_elevation_create(const PgttElevationConfig* cfg, int device, int num_envs, pgtt_elevation_handle* out) {
  if (!cfg || !out) return fail(PGTT_E_ARG, "pgtt_elevation_create: null argument");
  *out = nullptr;
  if (num_envs < 1) return fail(PGTT_E_ARG, "pgtt_elevation_create: num_envs must be >= 1");
  if (int rc = resolve(cfg, "pgtt_elevation_create")) return rc;
  if (int rc = check_device(device, "pgtt_elevation_create")) return rc;
  pgtt_elevation_map* h = new pgtt_elevation_map();
  h->device = device; h->num_envs = num_envs; h->cfg = *cfg;
  double qn = 0.0;
  for (int i = 0; i < 4; i++) qn += (double)cfg->mount_quat[i] * cfg->mount_quat[i];
  qn = std::sqrt(qn);
  for (int i = 0; i < 4; i++) h->cfg.mount_quat[i] = (float)(cfg->mount_quat[i] / qn);
  *out = h;
  return PGTT_OK;
}

int pgtt_elevation_destroy(pgtt_elevation_handle h) {
  delete h;
  return PGTT_OK;
}

int pgtt_elevation_bind(pgtt_elevation_handle h, const PgttElevationBuffers* bufs) {
  if (!h || !bufs) return fail(PGTT_E_ARG, "pgtt_elevation_bind: null argument");
  if (int rc = check_buffers(bufs, "pgtt_elevation_bind", true)) return rc;
  h->buf = *bufs;
  h->bound = true;
  h->points = nullptr; h->P = 0;
  return PGTT_OK;
}

int pgtt_elevation_bind_points(pgtt_elevation_handle h, const PgttElevationBuffers* bufs, const float* points, int P) {
  if (!h || !bufs) return fail(PGTT_E_ARG, "pgtt_elevation_bind_points: null argument");
  if (int rc = check_buffers(bufs, "pgtt_elevation_bind_points", false)) return rc;
  if (!points || P < 1) return fail(PGTT_E_ARG, "pgtt_elevation_bind_points: points is required, with P >= 1");
  h->buf = *bufs;
  h->bound = true;
  h->points = points; h->P = P;
  return PGTT_OK;
}

int pgtt_elevation(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_elevation: no buffers bound (pgtt_elevation_bind first)");
  if (!h->buf.depth) return fail(PGTT_E_STATE, "pgtt_elevation: the handle was bound without a depth image (pgtt_elevation_bind_points with depth == NULL)");
  return launch(h, false, clear_mask, clear_all, use_done, stream);
}

int pgtt_elevation_points(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation_points: null handle");
  if (!h->points) return fail(PGTT_E_STATE, "pgtt_elevation_points: no points bound (pgtt_elevation_bind_points first)");
  return launch(h, true, clear_mask, clear_all, use_done, stream);
}

int pgtt_elevation_bind_rate(pgtt_elevation_handle h, const int64_t* counter, int every) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation_bind_rate: null handle");
  if (!counter) return fail(PGTT_E_ARG, "pgtt_elevation_bind_rate: counter is required (the sensor's device counter)");
  if (every < 1) return fail(PGTT_E_ARG, "pgtt_elevation_bind_rate: every must be >= 1");
  h->counter = counter;
  h->every = every;
  return PGTT_OK;
}

int pgtt_elevation_follow(pgtt_elevation_handle h, const uint8_t* clear_mask, int clear_all, int use_done, int force, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation_follow: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_elevation_follow: no buffers bound (pgtt_elevation_bind or pgtt_elevation_bind_points first)");
  if (!h->every) return fail(PGTT_E_STATE, "pgtt_elevation_follow: no sensor rate bound (pgtt_elevation_bind_rate first)");
  return launch(h, h->points != nullptr, clear_mask, clear_all, use_done, stream, true, force);
}

int pgtt_elevation_bind_fill(pgtt_elevation_handle h, const PgttElevationFill* out, int passes) {
  if (!h || !out) return fail(PGTT_E_ARG, "pgtt_elevation_bind_fill: null argument");
  if (!out->est || !out->dist) return fail(PGTT_E_ARG, "pgtt_elevation_bind_fill: est and dist are required");
  if (passes < 1 || passes > PGTT_ELEVATION_MAX_GRID - 1) return fail(PGTT_E_ARG, "pgtt_elevation_bind_fill: passes must be in [1, 95]");
  h->fill = *out;
  h->passes = passes;
  return PGTT_OK;
}

int pgtt_elevation_fill(pgtt_elevation_handle h, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_elevation_fill: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_elevation_fill: no buffers bound (pgtt_elevation_bind or pgtt_elevation_bind_points first)");
  if (!h->passes) return fail(PGTT_E_STATE, "pgtt_elevation_fill: no outputs bound (pgtt_elevation_bind_fill first)");
  if (h->fill.obs_out && !h->buf.obs) return fail(PGTT_E_ARG, "pgtt_elevation_fill: obs is required with the fill's obs_out");
  HIP_TRY(hipSetDevice(h->device));
  const PgttElevationConfig& c = h->cfg;
  const PgttElevationFill& o = h->fill;
  FillArgs a{};
  a.state = h->buf.state; a.obs = h->buf.obs; a.map = h->buf.map; a.origin = h->buf.origin;
  a.est = o.est; a.dist = o.dist; a.obs_out = o.obs_out; a.map_out = o.map_out; a.dist_out = o.dist_out;
  a.N = h->num_envs; a.G = c.grid; a.obs_dim = c.obs_dim; a.scan_row0 = c.scan_row0; a.passes = h->passes;
  a.vec_map = runs16(c.grid * c.grid, a.map) ? 1 : 0;
  a.vec_out = runs16(c.grid * c.grid, o.map_out) ? 1 : 0;
  a.vec_dist = ((c.grid * c.grid) % 4 == 0 && ((uintptr_t)o.dist_out & 3) == 0) ? 1 : 0;            // dist_out's runs are 4 bytes; NULL counts as aligned
  a.res = c.res; a.sdx = c.scan_dist_x; a.sdy = c.scan_dist_y;
  const size_t lds = (size_t)(c.grid + 2) * (c.grid + 2) * (sizeof(unsigned) + 1);
  hipLaunchKernelGGL(fill_kernel, dim3(h->num_envs), dim3(kLanes), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

}  // extern "C"
