/*
 * pgtt_lidar.h — C ABI of libpgtt_lidar.so: a scanning range sensor, one range (and one world point) per ray per env per sensor tick.
 *
 * A separate library from libpgtt.so and the other side libraries: it only READS the state rows an env keeps (include/pgtt.h) and writes the
 * caller's `range`, `points` and `counter` buffers.  Like the depth camera (pgtt_depth.h) it is made to run next to the step.
 *
 * Conventions (those of pgtt.h)
 *   - plain C; `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 or a negative PGTT_E_* code (pgtt.h); the message is available from pgtt_lidar_last_error().
 *   - device buffers are CALLER-OWNED; pgtt_lidar() enqueues its kernels on the caller's stream and neither allocates, synchronises nor
 *     reads anything back, so it can be captured in a HIP graph.  The library reads no environment variable.
 *
 * Mount.  The sensor is rigidly mounted on body `mount_body` (0 = the torso, any of the PGTT_NBODY bodies) with the pose (mount_pos, mount_quat)
 * in that body's frame:
 *     sensor pose = body pose * mount pose
 * The body pose comes from the env's qpos rows by the forward kinematics of the 13 bodies, exactly as the depth camera's does (the base
 * quaternion normalised first, the per-env hinge zero offsets PGTT_P_QPOS0 when `params` is bound).
 *
 * Pattern.  A host table dirs[R][3] of ray directions in the SENSOR frame, 1 <= R <= PGTT_LIDAR_MAX_RAYS, the same for every env.  Each row is
 * normalised by pgtt_lidar_create (in double, then rounded to fp32); a zero or non-finite row is PGTT_E_ARG.  The table is copied to the device
 * once.  Ray r of an env starts at the sensor's origin o and runs along d_r = R_sensor dirs[r].
 *
 * Scene: the camera's.  The plane z = 0; the env's terrain variant (the boxes given to pgtt_lidar_set_terrain, variant label clamped to [0, T)
 * as the step kernels clamp it); with see_robot the robot primitives (PgttRenderGeom, include/pgtt_render.h) posed by the same kinematics - the
 * sensor's own body included, so the mount must sit outside that body's geoms.  A ray that starts inside a box does not see that box.
 * A direction may have a component that is exactly 0 in a box's frame: inside that slab the axis is no constraint, outside it the ray misses.
 *
 * Outputs.
 *   range[N][R]      the hit's distance ALONG THE RAY in metres, clamped to [near, far]; a miss reads `far`.
 *   points[N][R][3]  (optional, may be NULL) the WORLD point o + value * d_r where the written value satisfies near < value < far, otherwise
 *                    three NaNs.  World frame on purpose: a point is registered at the pose it was taken from.
 *
 * Sensor rate: counter[0] is a device int64 that every pgtt_lidar() call advances by one.  The scan is recomputed when force != 0 or the
 * counter's value BEFORE the call is 0 modulo `every`; the decision is made on the device.  Otherwise `range` and `points` are left untouched.
 *
 * Noise, applied only when noise_sigma > 0 or dropout > 0 (with both 0 no draw is made and the kernel is the one without noise code): the
 * camera's formulas.  With d the clamped noise-free range of ray r of local env e, c the counter's value before the call and
 *     u_k = uniform(seed, env_id_offset + e, (uint32) c, PGTT_RS_LIDAR, 4 r + k),  k = 0, 1, 2        (pgtt.h: the top 24 bits of word k of
 *           philox4x32_10(key = (seed_lo, seed_hi), counter = (global env id, epoch = (uint32) c, PGTT_RS_LIDAR, r)) * 2^-24)
 *     u_0 < dropout                    -> far (so the ray's point is NaN)
 *     otherwise z = sqrt(-2 ln(1 - u_1)) * cos(2 pi u_2)   (fp32)   and the value is clamp(d * (1 + noise_sigma * z), near, far)
 *
 * An env's outputs are functions of its own rows only: they are the same bits whatever else is in the batch and whatever N is.
 */
#ifndef PGTT_LIDAR_H_
#define PGTT_LIDAR_H_

#include <stdint.h>

#include "pgtt.h"
#include "pgtt_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGTT_LIDAR_MAX_RAYS 8192        /* rays of the pattern */
#define PGTT_RS_LIDAR 33                /* Philox stream id of the sensor noise (pgtt.h uses ids below 32, the depth camera 32) */

typedef struct PgttLidarConfig {
  float near, far;                      /* 0 < near < far, metres along the ray */
  int32_t mount_body;                   /* 0 .. PGTT_NBODY - 1; 0 = the torso */
  float mount_pos[3];                   /* sensor pose in the mount body's frame */
  float mount_quat[4];                  /* wxyz, non-zero; normalised by pgtt_lidar_create */
  int32_t every;                        /* >= 1: the sensor period in pgtt_lidar() calls (control steps) */
  int32_t see_robot;                    /* 0 / 1: the robot primitives are part of the scene */
  float noise_sigma;                    /* >= 0: relative standard deviation of the range noise */
  float dropout;                        /* in [0, 1): probability that a ray reads `far` */
  uint64_t seed;                        /* key of the noise streams */
  int64_t env_id_offset;                /* global id of local env 0 (as pgtt_reset's) */
} PgttLidarConfig;

/* device pointers, all caller-owned, sized for N = num_envs and R given to pgtt_lidar_create */
typedef struct PgttLidarBuffers {
  const float* state;                   /* [PGTT_NSTATE][N] (PgttBuffers.state), required */
  const float* params;                  /* [PGTT_NPARAM][N] or NULL (nominal qpos0) */
  const int32_t* variant;               /* [N] or NULL (= 0) */
  float* range;                         /* [N][R], required */
  float* points;                        /* [N][R][3] or NULL */
  int64_t* counter;                     /* [1], required; the caller initialises it (0) */
} PgttLidarBuffers;

typedef struct pgtt_lidar_scanner* pgtt_lidar_handle;

/* the checks of the config and of the pattern alone: host only, needs no GPU.  PGTT_E_ARG for a config outside the ranges above, R outside
 * [1, PGTT_LIDAR_MAX_RAYS], a NULL table, or a row that is zero or not finite. */
int pgtt_lidar_check(const PgttLidarConfig* cfg, const float* dirs_Rx3, int R);
/* `model` gives the kinematic tree; `dirs_Rx3` (host) the pattern; `geoms` (host, ngeom <= PGTT_RENDER_MAX_GEOM) the robot primitives, used
 * when cfg->see_robot is set.  Everything is copied.  PGTT_E_ARG for what pgtt_lidar_check refuses. */
int pgtt_lidar_create(const PgttModel* model, const PgttLidarConfig* cfg, const float* dirs_Rx3, int R, const PgttRenderGeom* geoms, int ngeom,
                      int device, int num_envs, pgtt_lidar_handle* out);
int pgtt_lidar_destroy(pgtt_lidar_handle h);
/* terrain: T variants x B (<= PGTT_MAX_BOX) boxes x [pos xyz, quat wxyz, half-size xyz] (the pgtt_set_terrain layout).  HOST pointer, copied
 * once into a resident device table.  T = 0 => plane only (the state after create).
 * The call frees the previous table and allocates a new one, and pgtt_lidar() passes the table's address and T / B as launch arguments: a
 * pgtt_lidar() captured in a HIP graph BEFORE this call still points at the freed table.  Capture again after every pgtt_lidar_set_terrain;
 * never replay a graph captured before it.  (The same holds for pgtt_lidar_bind and the buffers it names.) */
int pgtt_lidar_set_terrain(pgtt_lidar_handle h, const float* boxes_TxBx10, int T, int B);
/* PGTT_E_ARG when state, range or counter is NULL */
int pgtt_lidar_bind(pgtt_lidar_handle h, const PgttLidarBuffers* bufs);
/* one sensor tick for all N envs: two launches (the scan kernel, one workgroup per env; then the counter's increment).
 * PGTT_E_STATE before pgtt_lidar_bind. */
int pgtt_lidar(pgtt_lidar_handle h, int force, void* stream);
int pgtt_lidar_sizeof_config(void);
int pgtt_lidar_sizeof_buffers(void);
/* "src=<SHA-256 of pgtt_lidar.hip and the files it includes>;flavor=product" */
const char* pgtt_lidar_build_info(void);
const char* pgtt_lidar_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PGTT_LIDAR_H_ */
