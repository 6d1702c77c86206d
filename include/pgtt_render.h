/*
 * pgtt_render.h — C ABI of libpgtt_render.so: a batched ray-cast renderer for the env's state (frames, rollout videos).
 *
 * A separate library from libpgtt.so: it only READS the state rows an env keeps (include/pgtt.h) and writes images.
 * Nothing here is on the step path.
 *
 * Conventions (those of pgtt.h)
 *   - plain C; `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 or a negative PGTT_E_* code (pgtt.h); the message is available from pgtt_render_last_error().
 *   - device buffers are CALLER-OWNED; kernels are enqueued on the caller's stream; nothing allocates or synchronises inside pgtt_render().
 *
 * One call renders V views.  A view is one env id plus one camera; all views of a call share one resolution W x H.
 *   image row 0 is the top; pixel (i, j) is sampled at its centre (i + 0.5, j + 0.5); fovy is the vertical field of view;
 *   depth is the distance along the optical axis (+inf on a miss); segmentation ids are PGTT_SEG_*.
 * A view renders to the same bits whatever else is in the batch (nothing is shared between views, nothing is atomic).
 *
 * Scene: the plane z = 0, the env's terrain variant (the boxes given to pgtt_render_set_terrain, variant label clamped to [0, T) as the
 * step kernels clamp it), the robot primitives (PgttRenderGeom, posed by the forward kinematics of the 13 bodies from the env's qpos with
 * the per-env hinge zero offsets PGTT_P_QPOS0 when a params block is given) and optional marker spheres.
 * Shading: colour = albedo * (AMBIENT + DIFFUSE * max(0, n . l) * visible), n facing the ray, l = PGTT_RENDER_LIGHT normalised,
 * visible = 0 when a shadow ray from hit + PGTT_RENDER_SHADOW_EPS * n toward l hits a box or a robot geom (markers and the plane cast no
 * shadow), 1 otherwise or with shadows off.  A miss takes the sky colour SKY_HORIZON + (SKY_ZENITH - SKY_HORIZON) * max(0, d.z).
 * Stored as round(255 * clamp(c, 0, 1)) (round half to even, no gamma), packed r | g << 8 | b << 16 | 255 << 24.
 */
#ifndef PGTT_RENDER_H_
#define PGTT_RENDER_H_

#include <stdint.h>

#include "pgtt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- caps */
#define PGTT_RENDER_MAX_GEOM 32        /* robot primitives per handle */
#define PGTT_RENDER_MAX_MARKER 128     /* marker spheres per view (the 117 height-scan hits fit) */
#define PGTT_RENDER_MAX_DIM 4096       /* W and H */
#define PGTT_RENDER_MAX_VIEWS 16384     /* views per call (the pixel grid's second dimension) */

/* ---------------------------------------------------------------- shading constants (tests restate them) */
#define PGTT_RENDER_LIGHT_X 0.4f       /* direction TOWARD the light, normalised in the kernel */
#define PGTT_RENDER_LIGHT_Y 0.3f
#define PGTT_RENDER_LIGHT_Z 0.866f
#define PGTT_RENDER_AMBIENT 0.3f
#define PGTT_RENDER_DIFFUSE 0.7f
#define PGTT_RENDER_SHADOW_EPS 1e-3f   /* shadow-ray origin offset along the normal, metres */
#define PGTT_RENDER_CHECKER 0.5f       /* floor checker cell, metres: cell parity of (floor(x / c) + floor(y / c)) */
#define PGTT_RENDER_FLOOR_A_R 0.55f    /* even cells */
#define PGTT_RENDER_FLOOR_A_G 0.55f
#define PGTT_RENDER_FLOOR_A_B 0.60f
#define PGTT_RENDER_FLOOR_B_R 0.35f    /* odd cells */
#define PGTT_RENDER_FLOOR_B_G 0.35f
#define PGTT_RENDER_FLOOR_B_B 0.40f
#define PGTT_RENDER_BOX_R 0.80f        /* terrain boxes */
#define PGTT_RENDER_BOX_G 0.62f
#define PGTT_RENDER_BOX_B 0.40f
#define PGTT_RENDER_MARKER_R 0.10f     /* marker spheres */
#define PGTT_RENDER_MARKER_G 0.90f
#define PGTT_RENDER_MARKER_B 0.20f
#define PGTT_RENDER_SKY_HORIZON_R 0.75f
#define PGTT_RENDER_SKY_HORIZON_G 0.85f
#define PGTT_RENDER_SKY_HORIZON_B 0.95f
#define PGTT_RENDER_SKY_ZENITH_R 0.30f
#define PGTT_RENDER_SKY_ZENITH_G 0.50f
#define PGTT_RENDER_SKY_ZENITH_B 0.85f

/* ---------------------------------------------------------------- segmentation ids */
#define PGTT_SEG_SKY (-1)
#define PGTT_SEG_PLANE 0
#define PGTT_SEG_BOX 1                 /* + box index b (0 .. B-1) */
#define PGTT_SEG_GEOM 1000             /* + robot geom index g */
#define PGTT_SEG_MARKER 2000           /* + marker index k */

enum { PGTT_RENDER_SPHERE = 0, PGTT_RENDER_CAPSULE = 1, PGTT_RENDER_BOX = 2 };
/* FIXED: look-at = target (world).  TRACK: look-at = base position (qpos[0:3]) + target.  TRACK_YAW: as TRACK, and the azimuth is
 * azimuth_deg + the base yaw (atan2 of the normalised base quaternion, as the height scan takes it) in degrees. */
enum { PGTT_CAM_FIXED = 0, PGTT_CAM_TRACK = 1, PGTT_CAM_TRACK_YAW = 2 };
enum { PGTT_RENDER_SHADOWS = 1 };     /* PgttRenderViews.flags */

/* A robot primitive rigidly attached to body `body` (0 .. PGTT_NBODY-1), pose in that body's frame.
 * size: sphere (radius, -, -); capsule (radius, half-length along the local z axis, -); box (half extents x, y, z). */
typedef struct PgttRenderGeom {
  int32_t body;
  int32_t type;                        /* PGTT_RENDER_SPHERE / CAPSULE / BOX */
  float pos[3];
  float quat[4];                       /* wxyz */
  float size[3];
  float rgb[3];                        /* albedo */
} PgttRenderGeom;

/* MuJoCo's free-camera convention: fwd = (cos el cos az, cos el sin az, sin el), pos = lookat - distance * fwd, world +z up;
 * up = (-sin el cos az, -sin el sin az, cos el), right = fwd x up. */
typedef struct PgttRenderCamera {
  int32_t mode;                        /* PGTT_CAM_* */
  float target[3];
  float distance;                      /* > 0 */
  float azimuth_deg;
  float elevation_deg;
  float fovy_deg;                      /* in (0, 180) */
} PgttRenderCamera;

/* One render call.  HOST arrays: env_ids, cameras, markers' counts are read by pgtt_render itself (validated before any launch and
 * handed to the kernels as launch arguments); everything else is a DEVICE pointer. */
typedef struct PgttRenderViews {
  const float* state;                  /* device [PGTT_NSTATE][N] (PgttBuffers.state) */
  const float* params;                 /* device [PGTT_NPARAM][N] or NULL (nominal qpos0) */
  const int32_t* variant;              /* device [N] or NULL (= 0) */
  int32_t num_envs;                    /* N */
  int32_t num_views;                   /* V >= 1 */
  const int32_t* env_ids;              /* HOST [V], each in [0, N) */
  const PgttRenderCamera* cameras;     /* HOST [V] */
  const float* markers;                /* device [V][num_markers][4] (centre xyz, radius) or NULL */
  int32_t num_markers;                 /* 0 .. PGTT_RENDER_MAX_MARKER */
  int32_t width, height;               /* 1 .. PGTT_RENDER_MAX_DIM */
  int32_t flags;                       /* PGTT_RENDER_SHADOWS */
  uint32_t* rgba;                      /* device [V][H][W], required */
  float* depth;                        /* device [V][H][W] or NULL */
  int32_t* segmentation;               /* device [V][H][W] or NULL */
  float* body_pose;                    /* device [V][PGTT_NBODY][7] (world xyz, quat wxyz) or NULL: the setup kernel's kinematics (tests) */
  void* workspace;                     /* device, pgtt_render_workspace_bytes(V) bytes, 16-byte aligned */
} PgttRenderViews;

typedef struct pgtt_renderer* pgtt_render_handle;

/* `model` gives the kinematic tree (body_pos, body_quat, jnt_axis, qpos0); `geoms` (host, ngeom <= PGTT_RENDER_MAX_GEOM) the robot
 * primitives.  Both are copied. */
int pgtt_render_create(const PgttModel* model, const PgttRenderGeom* geoms, int ngeom, int device, pgtt_render_handle* out);
int pgtt_render_destroy(pgtt_render_handle h);
/* terrain: T variants x B (<= PGTT_MAX_BOX) boxes x [pos xyz, quat wxyz, half-size xyz] (the pgtt_set_terrain layout).  HOST pointer,
 * copied once into a resident device table.  T = 0 => plane only (the state after create). */
int pgtt_render_set_terrain(pgtt_render_handle h, const float* boxes_TxBx10, int T, int B);
/* bytes of the caller-owned workspace a call with `num_views` views needs (0 when num_views is out of range) */
int64_t pgtt_render_workspace_bytes(int num_views);
int pgtt_render(pgtt_render_handle h, const PgttRenderViews* v, void* stream);
int pgtt_render_sizeof_geom(void);
int pgtt_render_sizeof_camera(void);
int pgtt_render_sizeof_views(void);
/* "src=<SHA-256 of pgtt_render.hip and this header>;flavor=product" */
const char* pgtt_render_build_info(void);
const char* pgtt_render_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PGTT_RENDER_H_ */
