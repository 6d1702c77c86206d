/*
 * pgtt_depth.h — C ABI of libpgtt_depth.so: an onboard depth camera, one egocentric depth image per env per sensor tick.
 *
 * A separate library from libpgtt.so and libpgtt_render.so: it only READS the state rows an env keeps (include/pgtt.h) and writes the
 * caller's `depth` and `counter` buffers.  Unlike the renderer it is made to run next to the step: every env, every control step.
 *
 * Conventions (those of pgtt.h)
 *   - plain C; `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 or a negative PGTT_E_* code (pgtt.h); the message is available from pgtt_depth_last_error().
 *   - device buffers are CALLER-OWNED; pgtt_depth() enqueues its kernels on the caller's stream and neither allocates, synchronises nor
 *     reads anything back, so it can be captured in a HIP graph.
 *
 * Camera.  The camera is rigidly mounted on body `mount_body` (0 = the torso) with the pose (mount_pos, mount_quat) in that body's frame:
 *     camera pose = body pose * mount pose
 * The body pose comes from the env's qpos rows by the forward kinematics of the 13 bodies (the base quaternion normalised first, the
 * per-env hinge zero offsets PGTT_P_QPOS0 when `params` is bound), so the base's roll and pitch move the camera.
 * Optical axis fwd = the camera frame's +x, up = its +z, right = fwd x up (= its -y).
 * Image row 0 is the top; pixel (i, j) (row i, column j) is sampled at its centre:
 *     u = (2 (j + 0.5) / W - 1) * tan(fovy / 2) * W / H,   v = (1 - 2 (i + 0.5) / H) * tan(fovy / 2),   ray = normalise(fwd + u right + v up)
 * The value written is the hit's distance ALONG THE OPTICAL AXIS in metres, clamped to [near, far]; a miss writes `far`.
 *
 * Scene: the plane z = 0; the env's terrain variant (the boxes given to pgtt_depth_set_terrain, variant label clamped to [0, T) as the step
 * kernels clamp it); with see_robot the robot primitives (PgttRenderGeom, include/pgtt_render.h) posed by the same kinematics - the camera's
 * own body included, so the mount must sit outside that body's geoms.  A ray that starts inside a box does not see that box.
 *
 * Sensor rate: counter[0] is a device int64 that every pgtt_depth() call advances by one.  The image is recomputed when force != 0 or the
 * counter's value BEFORE the call is 0 modulo `every`; the decision is made on the device.  Otherwise `depth` is left untouched.
 *
 * Noise, applied only when noise_sigma > 0 or dropout > 0 (with both 0 no draw is made and the kernel is the one without noise code).
 * With d the clamped noise-free value of pixel p = i * W + j of local env e, c the counter's value before the call and
 *     u_k = uniform(seed, env_id_offset + e, (uint32) c, PGTT_RS_DEPTH, 4 p + k),  k = 0, 1, 2        (pgtt.h: the top 24 bits of word k of
 *           philox4x32_10(key = (seed_lo, seed_hi), counter = (global env id, epoch = (uint32) c, PGTT_RS_DEPTH, p)) * 2^-24)
 *     u_0 < dropout                    -> far
 *     otherwise z = sqrt(-2 ln(1 - u_1)) * cos(2 pi u_2)   (fp32)   and the value is clamp(d * (1 + noise_sigma * z), near, far)
 *
 * An env's image is a function of its own rows only: it is the same bits whatever else is in the batch and whatever N is.
 */
#ifndef PGTT_DEPTH_H_
#define PGTT_DEPTH_H_

#include <stdint.h>

#include "pgtt.h"
#include "pgtt_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGTT_DEPTH_MAX_DIM 256          /* width and height */
#define PGTT_RS_DEPTH 32                /* Philox stream id of the sensor noise (pgtt.h uses ids below 32) */

typedef struct PgttDepthConfig {
  int32_t width, height;                /* 1 .. PGTT_DEPTH_MAX_DIM each */
  float fovy_deg;                       /* vertical field of view, in (0, 180) */
  float near, far;                      /* 0 < near < far, metres along the optical axis */
  int32_t mount_body;                   /* 0 .. PGTT_NBODY - 1; 0 = the torso */
  float mount_pos[3];                   /* camera pose in the mount body's frame */
  float mount_quat[4];                  /* wxyz, non-zero; normalised by pgtt_depth_create */
  int32_t every;                        /* >= 1: the sensor period in pgtt_depth() calls (control steps) */
  int32_t see_robot;                    /* 0 / 1: the robot primitives are part of the scene */
  float noise_sigma;                    /* >= 0: relative standard deviation of the range noise */
  float dropout;                        /* in [0, 1): probability that a pixel reads `far` */
  uint64_t seed;                        /* key of the noise streams */
  int64_t env_id_offset;                /* global id of local env 0 (as pgtt_reset's) */
} PgttDepthConfig;

/* device pointers, all caller-owned, sized for N = num_envs given to pgtt_depth_create */
typedef struct PgttDepthBuffers {
  const float* state;                   /* [PGTT_NSTATE][N] (PgttBuffers.state), required */
  const float* params;                  /* [PGTT_NPARAM][N] or NULL (nominal qpos0) */
  const int32_t* variant;               /* [N] or NULL (= 0) */
  float* depth;                         /* [N][H][W], required */
  int64_t* counter;                     /* [1], required; the caller initialises it (0) */
} PgttDepthBuffers;

typedef struct pgtt_depth_camera* pgtt_depth_handle;

/* `model` gives the kinematic tree; `geoms` (host, ngeom <= PGTT_RENDER_MAX_GEOM) the robot primitives, used when cfg->see_robot is set.
 * Everything is copied.  PGTT_E_ARG for a config outside the ranges above. */
int pgtt_depth_create(const PgttModel* model, const PgttDepthConfig* cfg, const PgttRenderGeom* geoms, int ngeom, int device, int num_envs,
                      pgtt_depth_handle* out);
int pgtt_depth_destroy(pgtt_depth_handle h);
/* terrain: T variants x B (<= PGTT_MAX_BOX) boxes x [pos xyz, quat wxyz, half-size xyz] (the pgtt_set_terrain layout).  HOST pointer, copied
 * once into a resident device table.  T = 0 => plane only (the state after create).
 * The call frees the previous table and allocates a new one, and pgtt_depth() passes the table's address and T / B as launch arguments: a
 * pgtt_depth() captured in a HIP graph BEFORE this call still points at the freed table.  Capture again after every pgtt_depth_set_terrain;
 * never replay a graph captured before it.  (The same holds for pgtt_depth_bind and the buffers it names.) */
int pgtt_depth_set_terrain(pgtt_depth_handle h, const float* boxes_TxBx10, int T, int B);
/* PGTT_E_ARG when state, depth or counter is NULL */
int pgtt_depth_bind(pgtt_depth_handle h, const PgttDepthBuffers* bufs);
/* one sensor tick for all N envs: two launches (the image kernel, one workgroup per env; then the counter's increment).
 * PGTT_E_STATE before pgtt_depth_bind. */
int pgtt_depth(pgtt_depth_handle h, int force, void* stream);
int pgtt_depth_sizeof_config(void);
int pgtt_depth_sizeof_buffers(void);
/* "src=<SHA-256 of pgtt_depth.hip and this header>;flavor=product" */
const char* pgtt_depth_build_info(void);
const char* pgtt_depth_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PGTT_DEPTH_H_ */
