// pgtt_common.hip.h — what every translation unit of libpgtt.so shares (gfx950, wave64): the resident terrain table entry, the kernel
// argument block, the Philox draws, the small vector / quaternion algebra and the DPP move.  Nothing here depends on the lane layout
// (PG_SUBS): the physics side (pgtt_physics.hip.h, pgtt_physics_quad.hip.h, pgtt_physics_inst.hip) adds that, the task side
// (pgtt_task.hip, pgtt_curriculum.hip) and the host code (pgtt_launch.h, pgtt_api.hip) include this header only.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/pgtt.h"

namespace pgtt {

#define PG_INL __device__ __forceinline__

struct TerrainBox {                 // resident terrain table entry (80 B), built once by pgtt_set_terrain
  float px, py, pz, rb;             // centre, bounding radius |half-size|
  float sx, sy, sz, m00;            // half-size, rotation matrix row-major
  float m01, m02, m10, m11;
  float m12, m20, m21, m22;
  float hx, hy, hz, pad;            // half-extents of the WORLD-axis-aligned bounding box (|R| size, rounded up)
};

// ------------------------------------------------------------------ small vector helpers
struct V3 { float x, y, z; };
PG_INL V3 v3(float x, float y, float z) { return V3{x, y, z}; }
PG_INL V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
PG_INL V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
PG_INL V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
PG_INL V3 operator*(float s, V3 a) { return v3(a.x * s, a.y * s, a.z * s); }
PG_INL float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PG_INL V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
PG_INL float norm(V3 a) { return sqrtf(dot(a, a)); }
struct Q4 { float w, x, y, z; };
PG_INL Q4 qmul(Q4 u, Q4 v) {
  return Q4{u.w * v.w - u.x * v.x - u.y * v.y - u.z * v.z, u.w * v.x + u.x * v.w + u.y * v.z - u.z * v.y,
            u.w * v.y - u.x * v.z + u.y * v.w + u.z * v.x, u.w * v.z + u.x * v.y - u.y * v.x + u.z * v.w};
}
struct M3 { float m[9]; };
PG_INL M3 qmat(Q4 q) {
  float q00 = q.w * q.w, q01 = q.w * q.x, q02 = q.w * q.y, q03 = q.w * q.z;
  float q11 = q.x * q.x, q12 = q.x * q.y, q13 = q.x * q.z, q22 = q.y * q.y, q23 = q.y * q.z, q33 = q.z * q.z;
  M3 r;
  r.m[0] = q00 + q11 - q22 - q33; r.m[1] = 2 * (q12 - q03); r.m[2] = 2 * (q13 + q02);
  r.m[3] = 2 * (q12 + q03); r.m[4] = q00 - q11 + q22 - q33; r.m[5] = 2 * (q23 - q01);
  r.m[6] = 2 * (q13 - q02); r.m[7] = 2 * (q23 + q01); r.m[8] = q00 - q11 - q22 + q33;
  return r;
}
PG_INL V3 qrot(V3 v, Q4 q) {        // mjx math.rotate
  V3 u = v3(q.x, q.y, q.z);
  float uv = dot(u, v), uu = dot(u, u);
  V3 c = cross(u, v);
  return 2.0f * (uv * u) + (q.w * q.w - uu) * v + (2.0f * q.w) * c;
}
PG_INL V3 mcol(const M3& a, int i) { return v3(a.m[i], a.m[3 + i], a.m[6 + i]); }
PG_INL V3 mtmul(const M3& a, V3 v) {   // a^T v
  return v3(a.m[0] * v.x + a.m[3] * v.y + a.m[6] * v.z, a.m[1] * v.x + a.m[4] * v.y + a.m[7] * v.z,
            a.m[2] * v.x + a.m[5] * v.y + a.m[8] * v.z);
}
PG_INL V3 mmul(const M3& a, V3 v) {
  return v3(a.m[0] * v.x + a.m[1] * v.y + a.m[2] * v.z, a.m[3] * v.x + a.m[4] * v.y + a.m[5] * v.z,
            a.m[6] * v.x + a.m[7] * v.y + a.m[8] * v.z);
}
// normalise with MJX's zero guard (allclose(x, 0, atol=1e-8) -> treated as zero, norm 0)
PG_INL float normalize3(V3& a) {
  bool z = fabsf(a.x) <= 1e-8f && fabsf(a.y) <= 1e-8f && fabsf(a.z) <= 1e-8f;
  if (z) a = v3(1.f, 1.f, 1.f);
  float n = norm(a);
  float d = n + (z ? 1.0f : 0.0f);
  a = v3(a.x / d, a.y / d, a.z / d);
  return z ? 0.0f : n;
}
PG_INL void normalize4(Q4& q) {
  bool z = fabsf(q.w) <= 1e-8f && fabsf(q.x) <= 1e-8f && fabsf(q.y) <= 1e-8f && fabsf(q.z) <= 1e-8f;
  if (z) q = Q4{1.f, 1.f, 1.f, 1.f};
  float n = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z) + (z ? 1.0f : 0.0f);
  q = Q4{q.w / n, q.x / n, q.y / n, q.z / n};
}
PG_INL void make_frame(V3 a, V3& n, V3& t1, V3& t2) {
  normalize3(a);
  V3 y = (a.y > -0.5f && a.y < 0.5f) ? v3(0, 1, 0) : v3(0, 0, 1);
  V3 b = y - a * dot(a, y);
  normalize3(b);
  n = a; t1 = b; t2 = cross(a, b);
}
PG_INL float sel4(int l, float a, float b, float c, float d) { return l == 0 ? a : (l == 1 ? b : (l == 2 ? c : d)); }

// one DPP move (VALU only): lane i takes x from the lane CTRL names (quad_perm, row_ror, ...); the layouts' reductions are built from it
template <int CTRL>
PG_INL float dpp_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
PG_INL int dpp_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true); }

constexpr int kGridG = 16;        // cells per side of the terrain grid (pgtt_set_terrain): 128-bit box mask per cell and variant

struct KArgs {
  const PgttModel* model;
  const PgttConfig* cfg;
  const TerrainBox* terrain;   // [T][B]
  const float4* cull;          // [T][B] (px, py, hx, hy) of the same boxes: the scan's cull reads 1.6 KB per variant instead of strided pieces of 8 KB
  const uint4* grid;           // [T][kGridG * kGridG]: boxes whose grown world AABB touches the cell (bit b of the 128 = box b)
  float grid_E, grid_inv;      // the grid covers [-E, E]^2, cell (ix, iy) = floor((x + E) * inv), clamped
  int T, B;
  PgttBuffers buf;
  int N;
  unsigned long long seed;
  long long env_off;
  const unsigned char* mask;
  float yaw_override;          // NaN = use the base yaw
  int write_qpos;              // MODE_FORWARD: store the (quaternion-normalised) qpos
  // test hooks (pgtt_set_test_overrides; both off in normal operation): with rng_fix != NaN every uniform draw returns rng_fix
  // (the reference-generated fixtures tests/golden/task_*.npz were produced with jax.random stubbed that way), and with
  // scan_preset != 0 the step's observe kernel takes the 117 scan heights from buf.scan_z instead of casting rays (the
  // fixtures hold scan values, not terrains)
  float rng_fix;
  int scan_preset;
  // Hand-over record of a control step, env-major [N][kHandover]: what the physics kernel computes and the observe kernel of the SAME
  // pgtt_step reads (qpos, qvel, motor targets, sensor frame).  The caller-visible rows stay the SoA [row][N] buffers, written as before;
  // but a wave that reads ITS env's 114 values out of them makes 114 requests for 128-byte lines, and the observe launch spends its first
  // ~5 us doing that (one request in ~23 ns per env, measured by leaving rows out).  From the record they are two coalesced loads.
  // handover_w: the physics launch writes it (every MODE_STEP launch does); handover_r: the observe launch may read it (pgtt_step only -
  // between pgtt_physics and pgtt_observe called on their own the caller may have edited the rows).
  float* handover_w;
  const float* handover_r;
};

// ------------------------------------------------------------------ Philox4x32-10 (independent of the oracle's C)
PG_INL void philox4x32_10(unsigned k0, unsigned k1, unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    unsigned n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
PG_INL float rng_uniform(unsigned long long seed, unsigned env, unsigned epoch, unsigned stream, int idx) {
  unsigned c0 = env, c1 = epoch, c2 = stream, c3 = (unsigned)(idx >> 2);
  philox4x32_10((unsigned)seed, (unsigned)(seed >> 32), c0, c1, c2, c3);
  unsigned w = (idx & 3) == 0 ? c0 : ((idx & 3) == 1 ? c1 : ((idx & 3) == 2 ? c2 : c3));
  return (float)(w >> 8) * (1.0f / 16777216.0f);
}
PG_INL float rng_uniform(unsigned long long seed, unsigned env, unsigned epoch, unsigned stream, int idx, float fix) {
  const float u = rng_uniform(seed, env, epoch, stream, idx);
  return fix == fix ? fix : u;
}
PG_INL int exp_timer(unsigned long long seed, unsigned env, unsigned epoch, unsigned stream, float ctrl_dt, float fix) {
  double u = (double)rng_uniform(seed, env, epoch, stream, 0, fix);
  double t = -log1p(-u) * 5.0;
  return (int)rint(t / (double)ctrl_dt);
}

// MODE_STEP_XFRC: MODE_STEP with PgttBuffers.xfrc bound (the torso wrench enters qfrc_smooth); a kernel of its own, so that the two step
// kernels without a wrench buffer are the code they were before it existed (same instructions, same roundings)
enum { MODE_STEP = 0, MODE_FORWARD = 1, MODE_STEP_XFRC = 2 };
constexpr int kHandover = 128;                 // floats per env (512 bytes: four lines)
enum { HO_QPOS = 0, HO_QVEL = 19, HO_MOTOR = 37, HO_FRAME = 49, HO_END = HO_FRAME + PGTT_NFRAME };
static_assert(HO_END <= kHandover, "hand-over record");
// OBS_STEP_OBS: the scan + observation half of a step (rewards / bookkeeping are done by task_kernel, one env per LANE)
enum { OBS_STEP = 0, OBS_SCAN_LIFT = 1, OBS_RESET = 2, OBS_SCAN_ONLY = 3, OBS_STEP_OBS = 4 };

// Workgroup i is dispatched to XCD i % 8 and every XCD has its own L2.  Rows of the SoA state are contiguous over envs,
// so neighbouring envs share 128-byte lines: give each XCD a CONTIGUOUS range of logical blocks (MI355X_MICROARCH.md,
// "XCD-aware launches").  Identity when the grid is not a multiple of 8.
PG_INL int xcd_block(int bid, int nblocks) {
  if (nblocks & 7) return bid;
  return (bid & 7) * (nblocks >> 3) + (bid >> 3);
}

}  // namespace pgtt
