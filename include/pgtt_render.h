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
 *
 * The map call, pgtt_render_map(): the same views, with an env's elevation map drawn as a height field of cell columns.  This header does not
 * include the elevation library's; it restates the layout that header's "Map" paragraph gives.  `map` is [N][G][G] heights, NaN = not drawn.
 * For the view's env e, with lo = origin[e] - G/2 (integer division, G/2 rounded down; an origin outside +-2^30 is taken as +-2^30, as the
 * map's hole filling takes it): the WINDOW cell (a, b), 0 <= a, b < G, is world cell (lo_x + a, lo_y + b) and is stored at slot
 * [(lo_x + a) mod G][(lo_y + b) mod G] (floor-mod).  Any G from 1 to PGTT_RENDER_MAP_MAX_GRID is legal here.
 * Scene of a map call.  A window cell whose height h is not NaN and with h + lift > floor_z is a COLUMN: the axis-aligned box
 *     [(lo_x + a) res, (lo_x + a + 1) res] x [(lo_y + b) res, (lo_y + b + 1) res] x [floor_z, h + lift].
 * A pixel's ray takes the nearest hit over: all columns, each by the box rule above (entry distance, t > 0, a ray that starts inside a column
 * does not see it); the robot geoms; the markers; and, only with PGTT_RENDER_MAP_TERRAIN, the plane z = 0 and the env's terrain boxes.  That
 * brute-force statement is the contract; the kernel walks the cells a ray crosses instead.  Without the terrain flag a ray that hits nothing
 * takes the sky colour: a hole in the map shows sky.
 * Column normal: the face's axis, signed against the ray.  Column albedo: COLD + (HOT - COLD) x, x = clamp((s - tint_lo) / (tint_hi - tint_lo),
 * 0, 1), where s = tint[slot] when a tint layer is bound and the cell's height h (without lift) otherwise; NOVALUE when s is NaN.
 * Shading as above; with PGTT_RENDER_SHADOWS columns cast and receive shadows: the shadow ray is occluded by any column, any robot geom and,
 * with the terrain flag, any box.  Segmentation of a column: PGTT_SEG_CELL + a * G + b.  Depth as above.
 * A view renders to the same bits whatever else is in the batch; nothing but the images and the workspace is written.  With no column drawn
 * (all NaN, or every h + lift <= floor_z) and the terrain flag set, every output has the bits of pgtt_render() on the same views.
 * Refused (PGTT_E_ARG): everything pgtt_render() refuses; a NULL PgttRenderMap, map or origin; grid outside [1, PGTT_RENDER_MAP_MAX_GRID];
 * res not positive and finite; a non-finite floor_z, lift, tint_lo or tint_hi; tint_hi <= tint_lo; flag bits other than the one defined.
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
#define PGTT_RENDER_MAP_MAX_GRID 96    /* G of a map call: the window of heights is staged per pixel tile, 4 G G <= 36864 bytes */

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
#define PGTT_RENDER_MAP_COLD_R 0.15f   /* map columns: albedo at tint_lo and below */
#define PGTT_RENDER_MAP_COLD_G 0.35f
#define PGTT_RENDER_MAP_COLD_B 0.85f
#define PGTT_RENDER_MAP_HOT_R 0.95f    /* at tint_hi and above */
#define PGTT_RENDER_MAP_HOT_G 0.25f
#define PGTT_RENDER_MAP_HOT_B 0.10f
#define PGTT_RENDER_MAP_NOVALUE_R 0.45f /* where the tint layer is NaN */
#define PGTT_RENDER_MAP_NOVALUE_G 0.45f
#define PGTT_RENDER_MAP_NOVALUE_B 0.45f

/* ---------------------------------------------------------------- segmentation ids */
#define PGTT_SEG_SKY (-1)
#define PGTT_SEG_PLANE 0
#define PGTT_SEG_BOX 1                 /* + box index b (0 .. B-1) */
#define PGTT_SEG_GEOM 1000             /* + robot geom index g */
#define PGTT_SEG_MARKER 2000           /* + marker index k */
#define PGTT_SEG_CELL 10000            /* + a * G + b, the WINDOW cell (a, b) of a map call */

enum { PGTT_RENDER_SPHERE = 0, PGTT_RENDER_CAPSULE = 1, PGTT_RENDER_BOX = 2 };
/* FIXED: look-at = target (world).  TRACK: look-at = base position (qpos[0:3]) + target.  TRACK_YAW: as TRACK, and the azimuth is
 * azimuth_deg + the base yaw (atan2 of the normalised base quaternion, as the height scan takes it) in degrees. */
enum { PGTT_CAM_FIXED = 0, PGTT_CAM_TRACK = 1, PGTT_CAM_TRACK_YAW = 2 };
enum { PGTT_RENDER_SHADOWS = 1 };     /* PgttRenderViews.flags */
enum { PGTT_RENDER_MAP_TERRAIN = 1 }; /* PgttRenderMap.flags: draw the plane and the terrain boxes too */

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

/* The height field of a map call (layout and scene: the head of this file).  All three pointers are DEVICE pointers, only read. */
typedef struct PgttRenderMap {
  const float* map;                    /* device [N][G][G], required: heights, NaN = not drawn */
  const int32_t* origin;               /* device [N][2], required */
  const float* tint;                   /* device [N][G][G] in the same layout, or NULL: the colour is then taken from the height */
  int32_t grid;                        /* G, 1 .. PGTT_RENDER_MAP_MAX_GRID */
  float res;                           /* cell size, > 0, finite */
  float floor_z;                       /* finite: every column stands on this plane */
  float lift;                          /* finite: added to every height when drawn (0 in the belief view; a centimetre over the true terrain) */
  float tint_lo, tint_hi;              /* finite, tint_lo < tint_hi */
  int32_t flags;                       /* PGTT_RENDER_MAP_TERRAIN */
} PgttRenderMap;

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
/* the views of `v` with the height field `m` drawn as columns: the same setup kernel and workspace, a pixel kernel of its own */
int pgtt_render_map(pgtt_render_handle h, const PgttRenderViews* v, const PgttRenderMap* m, void* stream);
int pgtt_render_sizeof_geom(void);
int pgtt_render_sizeof_camera(void);
int pgtt_render_sizeof_views(void);
int pgtt_render_sizeof_map(void);
/* "src=<SHA-256 of pgtt_render.hip and this header>;flavor=product" */
const char* pgtt_render_build_info(void);
const char* pgtt_render_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PGTT_RENDER_H_ */
