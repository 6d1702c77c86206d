// pgtt_task.hip — the task-side kernels of libpgtt.so (gfx950): everything of a control step and of a reset that is not the physics.
// Host launchers at the end; pgtt_api.hip holds the entry points.
//
//   observe_kernel  : one env per WAVE.  13x9 height scan with the terrain variant's boxes read through
//                     wave-uniform addresses, quadrant statistics by wave reductions, the 171/215-dim
//                     observation rows assembled in LDS and stored coalesced, 21 rewards, bookkeeping,
//                     and (optionally) the Episode/AutoReset wrapper semantics.
//                     Reference: go2/joystick_pgtt.py:156-231, :238-370, go2/heightmap.py:25-67.
//   task_kernel     : the per-env scalar half of observe_kernel, one env per LANE (PgttConfig.observe_form = split).
//   reset_pose_kernel: pose / velocity sampling of Joystick.reset (go2/joystick_pgtt.py:51-70).
//   push_kernel     : the kick scheduler (pgtt_push).
//   interval_reduce_kernel, variant_range_kernel: the sums of pgtt_interval_reduce, pgtt_reset's check of the variant labels.
#include "pgtt_common.hip.h"

namespace pgtt {

// ------------------------------------------------------------------ reset: pose sampling (go2/joystick_pgtt.py:51-70)
__global__ __launch_bounds__(64) void reset_pose_kernel(KArgs a) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  const int N = a.N;
  if (e >= N) return;
  if (a.mask && !a.mask[e]) return;
  const PgttModel* __restrict__ m = a.model;
  float* __restrict__ S = a.buf.state;
  const unsigned id = (unsigned)(a.env_off + e);
  const unsigned ep = (unsigned)a.buf.istate[PGTT_I_RNG_CTR * (long)N + e];
  float qpos[19];
#pragma unroll
  for (int i = 0; i < 19; i++) qpos[i] = m->key_qpos[i];
  qpos[0] += rng_uniform(a.seed, id, ep, PGTT_RS_RESET_XY, 0, a.rng_fix) * 1.0f + -0.5f;
  qpos[1] += rng_uniform(a.seed, id, ep, PGTT_RS_RESET_XY, 1, a.rng_fix) * 1.0f + -0.5f;
  float yaw = rng_uniform(a.seed, id, ep, PGTT_RS_RESET_YAW, 0, a.rng_fix) * 6.28f + -3.14f;
  float sn, cs; sincosf(0.5f * yaw, &sn, &cs);
  Q4 q = qmul(Q4{qpos[3], qpos[4], qpos[5], qpos[6]}, Q4{cs, 0.f * sn, 0.f * sn, 1.f * sn});
  qpos[3] = q.w; qpos[4] = q.x; qpos[5] = q.y; qpos[6] = q.z;
#pragma unroll
  for (int i = 0; i < 19; i++) S[(PGTT_S_QPOS + i) * (long)N + e] = qpos[i];
#pragma unroll
  for (int i = 0; i < 18; i++) {
    S[(PGTT_S_QVEL + i) * (long)N + e] = i < 6 ? rng_uniform(a.seed, id, ep, PGTT_RS_RESET_VEL, i, a.rng_fix) * 0.2f + -0.1f : 0.f;
    S[(PGTT_S_QWARM + i) * (long)N + e] = 0.f;
  }
  if (a.buf.push_state && a.buf.xfrc && a.cfg->push_enable) {
    // the push scheduler of a reset env starts over (pgtt_push draws its wait), and the reset state carries no wrench
    a.buf.push_state[PGTT_PU_WAIT * (long)N + e] = -1.f;
    a.buf.push_state[PGTT_PU_STEP * (long)N + e] = -1.f;
#pragma unroll
    for (int r = 0; r < 6; r++) a.buf.xfrc[r * (long)N + e] = 0.f;
  }
}

// ------------------------------------------------------------------ push scheduler: one env per thread (pgtt_push; include/pgtt.h)
// MuJoCo Playground's Go2 joystick kicks (_maybe_apply_perturbation), recalled: wait, then a half-sine force pulse of the drawn duration whose
// integral is m_torso v / pi.  Runs before the step's physics launch and draws at the env's epoch of that step (streams PGTT_RS_PUSH_*).
// The affine maps of the draws are not contracted to an fma, so that a host replay in fp32 gets the same bits.
PG_INL float push_draw(const float* r, float u) {
#pragma clang fp contract(off)
  return u * (r[1] - r[0]) + r[0];
}
__global__ __launch_bounds__(64) void push_kernel(KArgs a) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  const int N = a.N;
  if (e >= N) return;
  const PgttConfig* __restrict__ cfg = a.cfg;
  float* __restrict__ P = a.buf.push_state;
  float* __restrict__ X = a.buf.xfrc;
  const unsigned id = (unsigned)(a.env_off + e);
  const unsigned ep = (unsigned)a.buf.istate[PGTT_I_RNG_CTR * (long)N + e];
  const float dt = cfg->ctrl_dt;
  float wait = P[PGTT_PU_WAIT * (long)N + e], kstep = P[PGTT_PU_STEP * (long)N + e], len = P[PGTT_PU_LEN * (long)N + e];
  float dur = P[PGTT_PU_DURATION * (long)N + e], vel = P[PGTT_PU_VELOCITY * (long)N + e];
  float dx = P[PGTT_PU_DIR_X * (long)N + e], dy = P[PGTT_PU_DIR_Y * (long)N + e];
  // a new wait after a reset (WAIT < 0), after a finished episode (done of the previous step) and after the last step of a kick
  const bool restart = wait < 0.f || a.buf.done[e] != 0.f;
  if (restart || (kstep >= 0.f && kstep >= len)) {
    wait = rintf(push_draw(cfg->push_wait_s, rng_uniform(a.seed, id, ep, PGTT_RS_PUSH_WAIT, 0, a.rng_fix)) / dt);
    kstep = -1.f;
  }
  if (kstep < 0.f) {
    if (wait > 0.f) {
      wait -= 1.f;
    } else {
      dur = push_draw(cfg->push_duration_s, rng_uniform(a.seed, id, ep, PGTT_RS_PUSH_KICK, 0, a.rng_fix));
      vel = push_draw(cfg->push_velocity, rng_uniform(a.seed, id, ep, PGTT_RS_PUSH_KICK, 1, a.rng_fix));
      const float ang = rng_uniform(a.seed, id, ep, PGTT_RS_PUSH_KICK, 2, a.rng_fix) * (float)(2.0 * M_PI);
      sincosf(ang, &dy, &dx);
      len = rintf(dur / dt);
      kstep = 0.f;
    }
  }
  float fx = 0.f, fy = 0.f;
  if (kstep >= 0.f) {
    const float mass = a.buf.params ? a.buf.params[PGTT_P_BODY_MASS * (long)N + e] : a.model->body_mass[0];
    const float u = 0.5f * sinf((float)M_PI * (kstep * dt) / dur);
    const float mag = u * mass * vel / dur;
    fx = mag * dx; fy = mag * dy;
    kstep += 1.f;
  }
  P[PGTT_PU_WAIT * (long)N + e] = wait; P[PGTT_PU_STEP * (long)N + e] = kstep; P[PGTT_PU_LEN * (long)N + e] = len;
  P[PGTT_PU_DURATION * (long)N + e] = dur; P[PGTT_PU_VELOCITY * (long)N + e] = vel;
  P[PGTT_PU_DIR_X * (long)N + e] = dx; P[PGTT_PU_DIR_Y * (long)N + e] = dy;
  X[0 * (long)N + e] = fx; X[1 * (long)N + e] = fy;
#pragma unroll
  for (int r = 2; r < 6; r++) X[r * (long)N + e] = 0.f;
}

// ------------------------------------------------------------------ observe: one env per wave
// sums over the 16 lanes of a DPP row / the 4 lanes of a quad, the same bits in every lane (symmetric butterflies, plain adds)
PG_INL float row16_sum(float x) {
#pragma clang fp contract(off)
  x = x + dpp_f<0xB1>(x); x = x + dpp_f<0x4E>(x); x = x + dpp_f<0x128>(x); x = x + dpp_f<0x124>(x);
  return x;
}
PG_INL float quad4_sum(float x) {
#pragma clang fp contract(off)
  x = x + dpp_f<0xB1>(x); x = x + dpp_f<0x4E>(x);
  return x;
}
PG_INL float quad4_min(float x) { x = fminf(x, dpp_f<0xB1>(x)); x = fminf(x, dpp_f<0x4E>(x)); return x; }
// max / min over the 16 lanes of a DPP row, the same bits in every lane of the row
PG_INL float row16_max(float x) { x = fmaxf(x, dpp_f<0xB1>(x)); x = fmaxf(x, dpp_f<0x4E>(x)); x = fmaxf(x, dpp_f<0x124>(x)); x = fmaxf(x, dpp_f<0x128>(x)); return x; }
PG_INL float row16_min(float x) { x = fminf(x, dpp_f<0xB1>(x)); x = fminf(x, dpp_f<0x4E>(x)); x = fminf(x, dpp_f<0x124>(x)); x = fminf(x, dpp_f<0x128>(x)); return x; }
// wave-wide max / min (all 64 lanes active): DPP butterflies inside the 16-lane rows, then the four row results through
// scalar registers - no LDS crossbar (ds_bpermute) round trips
PG_INL float wave_max(float v) {
  v = row16_max(v);
  const int i = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(i, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(i, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(i, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(i, 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
PG_INL float wave_min(float v) {
  v = row16_min(v);
  const int i = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(i, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(i, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(i, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(i, 48));
  return fminf(fminf(r0, r1), fminf(r2, r3));
}

// vertical ray (0,0,-1) from world point p against one terrain box; generic mjx _ray_box in the box frame.  The ray
// direction in the box frame lv = -R[2][:] is the same for every ray of a box: its reciprocals are formed once per box
// (v_rcp_f32, 1 ulp) and the six face parameters are (side - lp) * (1 / lv) instead of six divisions per ray; an
// axis-parallel component gives 1 / (+-0) = +-inf and the same +-inf / NaN face parameters as the division.
PG_INL float mul_unfused(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
struct RayBox { float il[3]; bool upright; };
PG_INL RayBox ray_box_prepare(const TerrainBox& tb) {
  // upright: the box z axis is along the world z axis (every shipped / generated terrain: boxes are only turned about z).  The ray
  // then runs along the box z axis: lv = (-0, -0, -m22), the four side faces get the parameters (side - lp) * rcp(-0) = +-inf / NaN
  // and hit points lp + x * (-0) = NaN, so they are never valid, while on the two z faces p0 = lp0 + x * (-0) = lp0 exactly - the generic
  // test reduces, bit for bit, to its two z faces.  m22 itself need not be 1: the tables hold float32 quaternions, and a box turned by
  // 90 degrees (0.70710677, 0, 0, 0.70710677) has m22 = w^2 + z^2 = 0.99999994 (half of the boxes of the level files).
  return RayBox{{__builtin_amdgcn_rcpf(-tb.m20), __builtin_amdgcn_rcpf(-tb.m21), __builtin_amdgcn_rcpf(-tb.m22)},
                tb.m20 == 0.f && tb.m21 == 0.f && tb.m22 != 0.f};
}
PG_INL float ray_box_down(const TerrainBox& tb, const RayBox& rb, V3 p) {
  V3 rel = p - v3(tb.px, tb.py, tb.pz);
  float lp[3] = {tb.m00 * rel.x + tb.m10 * rel.y + tb.m20 * rel.z, tb.m01 * rel.x + tb.m11 * rel.y + tb.m21 * rel.z,
                 tb.m02 * rel.x + tb.m12 * rel.y + tb.m22 * rel.z};
  float lv[3] = {-tb.m20, -tb.m21, -tb.m22};
  float sz[3] = {tb.sx, tb.sy, tb.sz};
  float best = INFINITY;
  if (rb.upright) {           // wave-uniform (the box record sits in scalar registers)
    const bool inside = (fabsf(lp[0]) <= sz[0]) & (fabsf(lp[1]) <= sz[1]);      // p0 = lp[0] + x * (-0) = lp[0], p1 likewise
    const float xt = (sz[2] - lp[2]) * rb.il[2], xb = (-sz[2] - lp[2]) * rb.il[2];
    best = (inside & (xt >= 0.f)) ? xt : best;
    best = (inside & (xb >= 0.f) & (xb < best)) ? xb : best;
    return best;
  }
#pragma unroll
  for (int f = 0; f < 6; f++) {
    const int ax = f % 3, i0 = ax == 0 ? 1 : 0, i1 = ax == 2 ? 1 : 2;
    float side = f < 3 ? sz[ax] : -sz[ax];
    float x = (side - lp[ax]) * rb.il[ax];
    float p0 = lp[i0] + x * lv[i0], p1 = lp[i1] + x * lv[i1];
    const bool valid = (fabsf(p0) <= sz[i0]) & (fabsf(p1) <= sz[i1]) & (x >= 0.f);     // `&`: selects, not branches
    best = (valid & (x < best)) ? x : best;
  }
  return best;
}

PG_INL float cubic_hermite(float t, float p0, float p1, float m0, float m1) {
  float t2 = t * t, t3 = t2 * t;
  return (2 * t3 - 3 * t2 + 1) * p0 + (t3 - 2 * t2 + t) * m0 + (-2 * t3 + 3 * t2) * p1 + (t3 - t2) * m1;
}
PG_INL float gait_get_z(float phi, float swing_height, float swing_min) {
  const float T_swing = (float)(2 * M_PI * (1 - 0.5) / 2), T_peak = (float)(2 * M_PI * (1 + 0.5) / 2), T_stance = (float)(2 * M_PI * 0.5);
  if (phi <= T_stance) return swing_min;
  if (phi <= T_peak) return cubic_hermite((phi - T_stance) / T_swing, swing_min, swing_height, T_swing * 0.f, T_swing * 0.f);
  return cubic_hermite((phi - T_peak) / T_swing, swing_height, swing_min, T_swing * 0.f, T_swing * 0.f);
}

// fmodf(x, y) for 0 <= x < 2 y - the phase clock: phase in [0, 2 pi) plus an increment below 2 pi.  There fmod is x or x - y, and x - y is exact
// (Sterbenz: y <= x <= 2 y), so the select returns fmodf's bits at 3 instructions instead of ~32 per foot; anything else takes the library call
PG_INL float fmod_once(float x, float y) {
  if (__builtin_expect(__ballot(!((x >= 0.f) & (x < 2.0f * y))) != 0ull, 0)) return fmodf(x, y);
  return x >= y ? x - y : x;
}

// Rewards, termination and bookkeeping of one control step (joystick_pgtt.py:193-227 / joystick.py): shared by the fused
// observe kernel (sh_* in LDS) and by task_kernel (sh_* = per-lane arrays, all indices compile-time constants).
struct TaskScalars {
  float cmd[3], phase[4], air[4], peak[4], hmax[4], hmin[4], last_contact[4], contact[4], first_contact[4];
  float gait_freq, phase_dt; int step_ctr, timer;
  bool done; float reward; float metrics[PGTT_NMETRIC];
};
// the values a step starts with, from the env's state rows and sensor frame: contact bookkeeping of joystick_pgtt.py:193-203.  H_max / H_min are
// the caller's: the fused form takes them from this scan's quadrant statistics, the split form from the state rows
PG_INL void task_foot_start(const float* st, const float* fr, float dt, int f, TaskScalars& t) {
  t.phase[f] = st[PGTT_S_PHASE + f];
  t.last_contact[f] = st[PGTT_S_LAST_CONTACT + f];
  t.contact[f] = fr[PGTT_F_CONTACT + f];
  const bool filt = (t.contact[f] != 0.f) || (t.last_contact[f] != 0.f);
  t.first_contact[f] = (st[PGTT_S_AIR_TIME + f] > 0.f ? 1.f : 0.f) * (filt ? 1.f : 0.f);
  t.air[f] = st[PGTT_S_AIR_TIME + f] + dt;
  t.peak[f] = fmaxf(st[PGTT_S_SWING_PEAK + f], fr[PGTT_F_FEET_POS + 3 * f + 2]);
}
// WAVE = true (fused observe kernel, one env per wave, every lane holds the same per-env scalars): the 12 joint terms and the
// 4 foot terms are evaluated by the lanes of a row / a quad in parallel (lane & 15 = joint, lane & 3 = foot) and summed
// with DPP butterflies - a fraction of the instructions of the serial loops and of the ~130 VGPRs their unrolled bodies keep
// alive.  WAVE = false (task_kernel, one env per lane): the serial loops.
template <bool WAVE>
PG_INL void task_rewards(const float* sh_st, const float* sh_fr, const float* sh_act, const PgttConfig* __restrict__ cfg,
                         const PgttModel* __restrict__ m, bool baseline, unsigned long long seed, unsigned id, unsigned ep, float dt,
                         float rng_fix, TaskScalars& t) {
  const float phase_dt = t.phase_dt;       // by value, read here: read inside the loop below, task_kernel compiles to other registers
  t.done = sh_fr[PGTT_F_UPVECTOR + 2] < 0.f;
  float rew[PGTT_NREW];
  const float cmd_norm = sqrtf(t.cmd[0] * t.cmd[0] + t.cmd[1] * t.cmd[1] + t.cmd[2] * t.cmd[2]);
  // the three exponentials (both tracking terms, feet_phase): WAVE = true evaluates them in ONE expf expansion, lanes 0 / 1 / 2
  float xlin, xang;
  {
    float e0 = t.cmd[0] - sh_fr[PGTT_F_LOCAL_LINVEL], e1 = t.cmd[1] - sh_fr[PGTT_F_LOCAL_LINVEL + 1];
    xlin = -(e0 * e0 + e1 * e1) / cfg->tracking_sigma;
    float ea = t.cmd[2] - sh_fr[PGTT_F_GYRO + 2];
    xang = -(ea * ea) / cfg->tracking_sigma;
  }
  rew[PGTT_R_LIN_VEL_Z] = sh_fr[PGTT_F_GLOBAL_LINVEL + 2] * sh_fr[PGTT_F_GLOBAL_LINVEL + 2];
  rew[PGTT_R_ANG_VEL_XY] = sh_fr[PGTT_F_GLOBAL_ANGVEL] * sh_fr[PGTT_F_GLOBAL_ANGVEL] + sh_fr[PGTT_F_GLOBAL_ANGVEL + 1] * sh_fr[PGTT_F_GLOBAL_ANGVEL + 1];
  rew[PGTT_R_ORIENTATION] = sh_fr[PGTT_F_UPVECTOR] * sh_fr[PGTT_F_UPVECTOR] + sh_fr[PGTT_F_UPVECTOR + 1] * sh_fr[PGTT_F_UPVECTOR + 1];
  {
    float sa = 0.f, lim = 0.f, pose = 0.f, s2 = 0.f, s1 = 0.f, en = 0.f, ar = 0.f;
    auto joint = [&](int i, float on) {
      float q = sh_st[PGTT_S_QPOS + 7 + i], dq = q - m->key_qpos[7 + i];
      sa += on * fabsf(dq);
      pose += on * ((dq * dq) * ((i % 3) == 0 ? 1.0f : 0.1f));
      // the reference holds the soft limits as float32 constants (go2/base.py:78-79): the product is ROUNDED before a joint is compared with it.
      // Contracted into q - range * factor it is not, and a joint exactly at its limit pays the product's rounding error instead of 0
      float lo = mul_unfused(m->jnt_range[i][0], cfg->soft_joint_pos_limit_factor), hi = mul_unfused(m->jnt_range[i][1], cfg->soft_joint_pos_limit_factor);
      lim += on * (-fminf(q - lo, 0.f) + fmaxf(q - hi, 0.f));
      float f = sh_fr[PGTT_F_ACT_FORCE + i];
      s2 += on * (f * f); s1 += on * fabsf(f);
      en += on * (fabsf(sh_st[PGTT_S_QVEL + 6 + i]) * fabsf(f));
      float da = sh_act[i] - sh_st[PGTT_S_LAST_ACT + i]; ar += on * (da * da);
    };
    if constexpr (WAVE) {
      const int j = (int)(threadIdx.x & 15);
      joint(j < 12 ? j : 0, j < 12 ? 1.0f : 0.0f);
      sa = row16_sum(sa); lim = row16_sum(lim); pose = row16_sum(pose); s2 = row16_sum(s2); s1 = row16_sum(s1); en = row16_sum(en); ar = row16_sum(ar);
    } else {
#pragma unroll
      for (int i = 0; i < 12; i++) joint(i, 1.0f);
    }
    rew[PGTT_R_STAND_STILL] = sa * (cmd_norm < 0.01f ? 1.f : 0.f);
    rew[PGTT_R_POSE] = pose; rew[PGTT_R_DOF_POS_LIMITS] = lim;
    rew[PGTT_R_TORQUES] = sqrtf(s2) + s1; rew[PGTT_R_ENERGY] = en; rew[PGTT_R_ACTION_RATE] = ar;
  }
  rew[PGTT_R_TERMINATION] = t.done ? 1.f : 0.f;
  {
    float slip = 0.f, clear = 0.f, perr = 0.f, swing = 0.f, airr = 0.f, con = 0.f, center = 0.f, fh = 0.f, minfoot = INFINITY;
    auto foot = [&](int f, float contact_f, float hmax_f, float phase_f, float air_f, float first_f, float peak_f) {
      float vx = sh_fr[PGTT_F_FEET_VEL + 3 * f], vy = sh_fr[PGTT_F_FEET_VEL + 3 * f + 1];
      float v2 = vx * vx + vy * vy;
      slip += v2 * contact_f;
      float px = sh_fr[PGTT_F_FEET_POS + 3 * f], py = sh_fr[PGTT_F_FEET_POS + 3 * f + 1], pz = sh_fr[PGTT_F_FEET_POS + 3 * f + 2];
      const float clr = baseline ? sh_fr[PGTT_F_FOOT_SITE_Z + f] - (hmax_f - cfg->base_feet_distance + cfg->swing_height)   // joystick.py:569-572
                                 : pz - (hmax_f + cfg->swing_height);                                                  // joystick_pgtt.py:576-578
      clear += fabsf(clr) * sqrtf(sqrtf(v2));
      float rz = gait_get_z(phase_f, hmax_f + cfg->swing_height, cfg->base_feet_distance);
      perr += (pz - rz) * (pz - rz);
      bool swing_mask = phase_f / (float)(2 * M_PI) >= 0.5f;
      swing += ((pz - cfg->swing_height) * (pz - cfg->swing_height)) * (swing_mask ? 1.f : 0.f);
      con += (swing_mask && contact_f != 0.f) ? 1.f : 0.f;
      airr += (air_f - (baseline ? 0.5f : 0.1f)) * first_f;        // joystick.py:591 / joystick_pgtt.py:597
      center += px * px + py * py;
      float er = peak_f / cfg->swing_height - 1.0f;
      fh += (er * er) * first_f;
      minfoot = fminf(minfoot, sh_fr[PGTT_F_FOOT_SITE_Z + f]);
    };
    if constexpr (WAVE) {
      const int f = (int)(threadIdx.x & 3);
      foot(f, sel4(f, t.contact[0], t.contact[1], t.contact[2], t.contact[3]), sel4(f, t.hmax[0], t.hmax[1], t.hmax[2], t.hmax[3]),
           sel4(f, t.phase[0], t.phase[1], t.phase[2], t.phase[3]), sel4(f, t.air[0], t.air[1], t.air[2], t.air[3]),
           sel4(f, t.first_contact[0], t.first_contact[1], t.first_contact[2], t.first_contact[3]), sel4(f, t.peak[0], t.peak[1], t.peak[2], t.peak[3]));
      slip = quad4_sum(slip); clear = quad4_sum(clear); perr = quad4_sum(perr); swing = quad4_sum(swing); airr = quad4_sum(airr);
      con = quad4_sum(con); center = quad4_sum(center); fh = quad4_sum(fh); minfoot = quad4_min(minfoot);
    } else {
#pragma unroll
      for (int f = 0; f < 4; f++) foot(f, t.contact[f], t.hmax[f], t.phase[f], t.air[f], t.first_contact[f], t.peak[f]);
    }
    float moving = cmd_norm > 0.01f ? 1.f : 0.f;
    rew[PGTT_R_FEET_SLIP] = slip * moving; rew[PGTT_R_FEET_CLEARANCE] = clear;
    const float xph = -perr / cfg->phase_sigma;
    if constexpr (WAVE) {
      const int ln = (int)(threadIdx.x & 63);
      const int ex = __float_as_int(expf(ln == 0 ? xlin : (ln == 1 ? xang : xph)));
      rew[PGTT_R_TRACKING_LIN_VEL] = __int_as_float(__builtin_amdgcn_readlane(ex, 0));
      rew[PGTT_R_TRACKING_ANG_VEL] = __int_as_float(__builtin_amdgcn_readlane(ex, 1));
      rew[PGTT_R_FEET_PHASE] = __int_as_float(__builtin_amdgcn_readlane(ex, 2));
    } else {
      rew[PGTT_R_TRACKING_LIN_VEL] = expf(xlin); rew[PGTT_R_TRACKING_ANG_VEL] = expf(xang); rew[PGTT_R_FEET_PHASE] = expf(xph);
    }
    rew[PGTT_R_FEET_SWING] = swing;
    rew[PGTT_R_FEET_AIR_TIME] = airr * moving; rew[PGTT_R_CONTACT] = -con; rew[PGTT_R_CENTER] = center;
    rew[PGTT_R_FEET_HEIGHT] = fh * moving;
    float bh = sh_st[PGTT_S_QPOS + 2] - minfoot - 0.27f;
    rew[PGTT_R_BODY_HEIGHT] = bh * bh;
  }
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < PGTT_NREW; k++) { t.metrics[k] = rew[k] * cfg->reward_scale[k]; sum += t.metrics[k]; }
  t.reward = fminf(fmaxf(sum * dt, 0.f), 10000.f);
  // bookkeeping (joystick_pgtt.py:205-227)
  t.step_ctr += 1;
#pragma unroll
  for (int f = 0; f < 4; f++) t.phase[f] = fmod_once(t.phase[f] + phase_dt, (float)(2 * M_PI));
  t.timer -= 1;
  if constexpr (WAVE) {
    // the waves that resample (1 - 2 % of a launch) are among the last to leave it: their four counter blocks (command y / z / w, timer)
    // in ONE Philox pass, lanes 0..3, instead of four - same words as rng_uniform(.., stream, i) = word i of block 0 of the stream
    if (t.done || t.timer <= 0) {
      const int ln = (int)(threadIdx.x & 63);
      unsigned c0 = id, c1 = ep, c2 = (unsigned)(ln == 0 ? PGTT_RS_CMD_Y : (ln == 1 ? PGTT_RS_CMD_Z : (ln == 2 ? PGTT_RS_CMD_W : PGTT_RS_TIMER))), c3 = 0u;
      philox4x32_10((unsigned)seed, (unsigned)(seed >> 32), c0, c1, c2, c3);
      auto uni = [&](unsigned w, int src) {
        const float u = (float)((unsigned)__builtin_amdgcn_readlane((int)w, src) >> 8) * (1.0f / 16777216.0f);
        return rng_fix == rng_fix ? rng_fix : u;
      };
      if (t.timer <= 0) {
        const unsigned w[3] = {c0, c1, c2};
#pragma unroll
        for (int i = 0; i < 3; i++) {
          float y = uni(w[i], 0) * (cfg->cmd_u_max[i] - cfg->cmd_u_min[i]) + cfg->cmd_u_min[i];
          float zb = uni(w[i], 1) < cfg->cmd_b[i] ? 1.f : 0.f;
          float wb = uni(w[i], 2) < 0.5f ? 1.f : 0.f;
          t.cmd[i] = t.cmd[i] - wb * (t.cmd[i] - y * zb);
        }
      }
      const double wait = -log1p(-(double)uni(c0, 3)) * 5.0;        // exp_timer
      t.timer = (int)rint(wait / (double)dt);
    }
  } else {
    if (t.timer <= 0) {
#pragma unroll
      for (int i = 0; i < 3; i++) {
        float y = rng_uniform(seed, id, ep, PGTT_RS_CMD_Y, i, rng_fix) * (cfg->cmd_u_max[i] - cfg->cmd_u_min[i]) + cfg->cmd_u_min[i];
        float zb = rng_uniform(seed, id, ep, PGTT_RS_CMD_Z, i, rng_fix) < cfg->cmd_b[i] ? 1.f : 0.f;
        float wb = rng_uniform(seed, id, ep, PGTT_RS_CMD_W, i, rng_fix) < 0.5f ? 1.f : 0.f;
        t.cmd[i] = t.cmd[i] - wb * (t.cmd[i] - y * zb);
      }
    }
    if (t.done || t.timer <= 0) t.timer = exp_timer(seed, id, ep, PGTT_RS_TIMER, dt, rng_fix);
  }
  float sp = 0.f;
#pragma unroll
  for (int f = 0; f < 4; f++) {
    float nc = t.contact[f] != 0.f ? 0.f : 1.f;
    t.air[f] *= nc; t.peak[f] *= nc; t.last_contact[f] = t.contact[f]; sp += t.peak[f];
  }
  t.metrics[PGTT_NREW] = sp / 4;
}

// ---- observation rows as a table.  Every row of the state observation is (source value [- zmin]) [+ noise] [- offset]; which source, which
// word of the noise draws, which noise scale and which offset is a function of the row number alone.  The kernel used to find them through a
// chain of row-range tests that every lane of every pass walked (the vector ALU is what the four waves of a SIMD share); now lane io reads
// descriptor io - byte offsets into ONE LDS array that holds the state rows, the sensor frame, the scan and the per-env scalars - and the
// pass is four LDS reads and ~20 vector instructions.  Layout of the array (floats):
enum { OL_ST = 0, OL_FR = OL_ST + PGTT_NSTATE, OL_SCAN = OL_FR + PGTT_NFRAME, OL_DRV = OL_SCAN + 128,
       OD_PHASE = 0 /* cos x4, sin x4 */, OD_GAIT = 8, OD_CMD = 9, OD_ZERO = 12, OD_LASTC = 13, OD_AIR = 17,
       OD_SCALE = 21 /* 0, gyro, gravity, joint pos, joint vel, scan */, OD_OFFS = 27 /* 0, key_qpos[7..18] */, OD_END = 40, OL_END = OL_DRV + OD_END };
constexpr int kObsRowSlots = 192, kPrivSlots = 64;
struct ObsRowTab { unsigned row[2][kObsRowSlots]; unsigned short priv[kPrivSlots]; unsigned short quad[64][4]; };
// descriptor: bits 0..10 byte offset of the source, 11..20 byte offset of the noise word in sh_rng, 21..25 byte offset of the scale in
// OD_SCALE (20 = scan: the row is taken relative to zmin), 26..31 byte offset of the offset in OD_OFFS
constexpr unsigned obs_row_desc(int i) {       // i = row in the PGTT layout (joystick_pgtt.py:336-349)
  unsigned src = 0, word = 0, scale = 0, offs = 0;
  if (i < 3) { src = OL_FR + PGTT_F_GYRO + i; word = i; scale = 1; }
  else if (i < 6) { src = OL_FR + PGTT_F_GRAVITY + i - 3; word = 4 + i - 3; scale = 2; }
  else if (i < 18) { src = OL_ST + PGTT_S_QPOS + 7 + i - 6; word = 8 + i - 6; scale = 3; offs = 1 + i - 6; }
  else if (i < 30) { src = OL_ST + PGTT_S_QVEL + 6 + i - 18; word = 20 + i - 18; scale = 4; }
  else if (i < 38) { src = OL_DRV + OD_PHASE + i - 30; }
  else if (i < 38 + PGTT_NSCAN) { src = OL_SCAN + i - 38; word = 32 + i - 38; scale = 5; }
  else if (i == 38 + PGTT_NSCAN) { src = OL_DRV + OD_GAIT; }
  else if (i < 39 + PGTT_NSCAN + 12) { src = OL_ST + PGTT_S_LAST_ACT + i - (39 + PGTT_NSCAN); }
  else if (i < 39 + PGTT_NSCAN + 15) { src = OL_DRV + OD_CMD + i - (51 + PGTT_NSCAN); }
  else { src = OL_DRV + OD_ZERO; }
  return (src * 4u) | ((word * 4u) << 11) | ((scale * 4u) << 21) | ((offs * 4u) << 26);
}
constexpr unsigned short obs_priv_src(int i) {    // the 44 privileged extras (joystick_pgtt.py:355-365)
  int src = OL_DRV + OD_ZERO;
  if (i < 3) src = OL_FR + PGTT_F_LOCAL_LINVEL + i;
  else if (i < 6) src = OL_FR + PGTT_F_ACCEL + i - 3;
  else if (i < 9) src = OL_FR + PGTT_F_GLOBAL_ANGVEL + i - 6;
  else if (i < 21) src = OL_FR + PGTT_F_ACT_FORCE + i - 9;
  else if (i < 25) src = OL_DRV + OD_LASTC + i - 21;
  else if (i < 37) src = OL_FR + PGTT_F_FEET_VEL + i - 25;
  else if (i < 41) src = OL_DRV + OD_AIR + i - 37;
  return (unsigned short)(src * 4);
}
// Quadrant statistics (joystick_pgtt.py:169-190, n = 6 on both axes of the 13 x 9 grid: top / back = rows 0..5 / 7..12, right / left =
// columns 7..8 / 0..5): the 16 lanes of row q of the wave cover quadrant q (0 top right, 1 top left, 2 back right, 3 back left), three
// cells each; a quadrant has 12 or 36 cells, the surplus slots repeat cells of the same quadrant (max and min do not mind).
constexpr unsigned short obs_quad_cell(int lane, int j) {
  const int q = lane >> 4, s = (lane & 15) + 16 * j;
  const bool left = (q & 1) != 0, back = (q & 2) != 0;
  const int ncol = left ? 6 : 2, ncell = 6 * ncol, k = s % ncell;
  const int r = (back ? 7 : 0) + k / ncol, c = (left ? 0 : 7) + k % ncol;
  return (unsigned short)((OL_SCAN + r * PGTT_SCAN_W + c) * 4);
}
constexpr ObsRowTab make_obs_row_tab() {
  ObsRowTab t{};
  for (int l = 0; l < 64; l++) for (int j = 0; j < 4; j++) t.quad[l][j] = obs_quad_cell(l, j < 3 ? j : 0);
  for (int io = 0; io < kObsRowSlots; io++) {
    t.row[0][io] = obs_row_desc(io);
    // the baseline layout (go2/joystick.py) drops rows 30..37 (phase) and 38 + NSCAN (gait_freq)
    t.row[1][io] = obs_row_desc(io < 30 ? io : (io < 30 + PGTT_NSCAN ? io + 8 : io + 9));
  }
  for (int i = 0; i < kPrivSlots; i++) t.priv[i] = obs_priv_src(i);
  return t;
}
static_assert(OL_END * 4 < 2048 && (8 + (PGTT_NSCAN + 3) / 4) * 16 <= 1024 && PGTT_OBS <= kObsRowSlots && PGTT_PRIV - PGTT_OBS <= kPrivSlots, "descriptor fields");
__device__ const ObsRowTab kObsRowTab = make_obs_row_tab();

// What the phases of observe_kernel pass on.  ObsPrefetch: what is requested from memory ahead of its use (see load_rows); ObsScan: the scan heights of
// this lane (cells lane and lane + 64) and the base height; ObsQuad: the quadrant statistics; ObsHist: lane < 24 holds one entry of each history.
struct ObsPrefetch { const TerrainBox* boxes; float4 brec[2]; unsigned rdesc[3], psrc; uint2 qcell; float epm_old, ivs_old; };
struct ObsScan { float bz, z[2]; };
struct ObsQuad { float max[4], min[4], zmin; };
struct ObsHist { float q, v; bool upd; };
// One wave's view of its env: what every phase needs - the launch arguments, the env, the lane, the wave's LDS arrays - and the phases themselves,
// in the order observe_kernel runs them.  Every phase is entered by all 64 lanes (the barriers inside count on it).
struct ObserveWave {
  const KArgs& a; const int e, lane, N;
  const PgttModel* __restrict__ m; const PgttConfig* __restrict__ cfg; float* __restrict__ S; int* __restrict__ I;
  float* sh_src; float* sh_st; float* sh_fr; float* sh_scan; float* sh_drv; float* sh_obs; float* sh_act;
  bool baseline;                        // set by load_rows
  int OBSD, PRIVD; unsigned id, ep; float dt;      // set by env_constants

  template <int OMODE, bool HAS_TERRAIN> PG_INL void load_rows(const float* __restrict__ action, ObsPrefetch& pf) {
    // The cull data of the env's variant do not depend on the state: lane j requests (centre x, y, world-AABB half extents x, y) of boxes j and
    // j + 64 BEFORE the state rows are waited for, so the two round trips overlap.  They come from the compact table (16 contiguous bytes per
    // box: 13 lines per variant) - the same four numbers out of the 80-byte records cost 160 line requests per wave, more than all its rows
    pf.boxes = nullptr;
    if (HAS_TERRAIN) {
      const int v = a.buf.variant ? min(max(a.buf.variant[e], 0), a.T - 1) : 0;      // clamped like in physics_kernel
      pf.boxes = a.terrain + (long)v * a.B;
#pragma unroll
      for (int h = 0; h < 2; h++) pf.brec[h] = a.cull[(long)v * a.B + min(lane + 64 * h, a.B - 1)];
    }
    if (OMODE == OBS_STEP && a.handover_r) {
      // this step's physics launch left qpos, qvel, the motor targets and the sensor frame env-major: two coalesced loads.  Of the other rows
      // the step reads PGTT_S_CMD .. PGTT_NSTATE - 1 without H_max / H_min (formed anew from this step's scan) and the older halves of the two
      // histories - not the warm start either
      const float* __restrict__ Hr = a.handover_r + (long)e * kHandover;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int j = lane + 64 * h;
        if (j < HO_END) {
          const float v = Hr[j];
          if (j < HO_MOTOR) sh_st[j] = v;                     // qpos, qvel: rows 0 .. 36 in the same order
          else if (j < HO_FRAME) sh_st[PGTT_S_MOTOR_TARGETS + j - HO_MOTOR] = v;
          else sh_fr[j - HO_FRAME] = v;
        }
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int r = PGTT_S_CMD + lane + 64 * h;
        const bool need = r < PGTT_NSTATE && !(r >= PGTT_S_HMAX && r < PGTT_S_HMIN + 4) && !(r >= PGTT_S_MOTOR_TARGETS && r < PGTT_S_MOTOR_TARGETS + 12) &&
                          !(r >= PGTT_S_QERR_HIST + 12 && r < PGTT_S_QERR_HIST + 24) && !(r >= PGTT_S_QVEL_HIST + 12 && r < PGTT_S_QVEL_HIST + 24);     // the older half of a history only ever leaves
        if (need) sh_st[r] = S[r * (long)N + e];
      }
    } else {
      for (int r = lane; r < PGTT_NSTATE; r += 64) sh_st[r] = S[r * (long)N + e];
      for (int r = lane; r < PGTT_NFRAME; r += 64) sh_fr[r] = a.buf.frame[r * (long)N + e];
    }
    if (OMODE == OBS_STEP && lane < 12) sh_act[lane] = action[(long)e * 12 + lane];
    // row descriptors of the three passes over the observation and of the privileged extras (constants: requested with the state rows)
    baseline = cfg->method == PGTT_METHOD_BASELINE;
#pragma unroll
    for (int it = 0; it < 3; it++) pf.rdesc[it] = kObsRowTab.row[baseline ? 1 : 0][lane + 64 * it];
    pf.psrc = kObsRowTab.priv[lane];
    pf.qcell = *reinterpret_cast<const uint2*>(kObsRowTab.quad[lane]);      // byte offsets of this lane's three scan cells
    // the running sums this step adds to (rows of this env, touched by this wave only) are requested here, a launch ahead of their use:
    // at the end of the wave nothing is left to hide a round trip behind
    pf.epm_old = 0.f; pf.ivs_old = 0.f;
    if (OMODE == OBS_STEP && lane < PGTT_NMETRIC + 2) {
      if (a.buf.ep_metrics) pf.epm_old = a.buf.ep_metrics[lane * (long)N + e];
      if (a.buf.interval_sums) pf.ivs_old = a.buf.interval_sums[lane * (long)N + e];
    }
    __syncthreads();
  }

  template <int OMODE, bool HAS_TERRAIN> PG_INL void height_scan(const ObsPrefetch& pf, ObsScan& sc) {
    // ---------------- height scan (heightmap.py:25-67)
    const float bx = sh_st[PGTT_S_QPOS + 0], by = sh_st[PGTT_S_QPOS + 1], bz = sh_st[PGTT_S_QPOS + 2];
    float yaw;
    if (OMODE == OBS_STEP || OMODE == OBS_STEP_OBS || (OMODE == OBS_SCAN_ONLY && a.yaw_override != a.yaw_override)) {
      float qw = sh_st[PGTT_S_QPOS + 3], qx = sh_st[PGTT_S_QPOS + 4], qy = sh_st[PGTT_S_QPOS + 5], qz = sh_st[PGTT_S_QPOS + 6];
      float qn = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
      qw /= qn; qx /= qn; qy /= qn; qz /= qn;
      yaw = atan2f(2.0f * (qw * qz + qx * qy), 1.0f - 2.0f * (qy * qy + qz * qz));
    } else if (OMODE == OBS_SCAN_ONLY) {
      yaw = a.yaw_override;
    } else {
      yaw = 0.f;
    }
    // ONE sincos evaluation for the yaw (lanes 8..63; every lane then takes it from lane 8) and for the eight phase rows of the observation
    // (lanes 0..7: cos x4, sin x4 of the phases the step starts with - parked in LDS until the rows are formed): the expansion is ~80 vector
    // instructions whatever the number of lanes that want it
    float sy, cy;
    if (OMODE == OBS_SCAN_ONLY || OMODE == OBS_SCAN_LIFT) sincosf(yaw, &sy, &cy);
    else {
      const int f = lane & 3;
      const float ph = OMODE == OBS_RESET ? ((f == 1 || f == 2) ? (float)M_PI : 0.f) : sh_st[PGTT_S_PHASE + f];
      float sn, cs; sincosf(lane < 8 ? ph : yaw, &sn, &cs);
      if (lane < 8) sh_drv[OD_PHASE + lane] = lane < 4 ? cs : sn;
      sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sn), 8)); cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cs), 8));
    }
    const float oz = bz + cfg->scan_z_offset;
    V3 org[2]; float hit[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      int idx = lane + 64 * h;
      int ii = idx < PGTT_NSCAN ? idx : 0;
      int r = ii / PGTT_SCAN_W, c = ii - r * PGTT_SCAN_W;
      float ox = ((float)(PGTT_SCAN_H - 1) * 0.5f - (float)r) * cfg->scan_dist_x;
      float oy = ((float)(PGTT_SCAN_W - 1) * 0.5f - (float)c) * cfg->scan_dist_y;
      float wx = ox * cy + oy * (-sy), wy = ox * sy + oy * cy;
      org[h] = v3(bx + wx, by + wy, oz);
      if (r == (PGTT_SCAN_H - 1) / 2 && c == (PGTT_SCAN_W - 1) / 2) org[h] = v3(bx, by, oz);
      // plane z=0 (normal +z): x = -pnt_z / vec_z = pnt_z, valid if x >= 0
      float x = oz;
      hit[h] = x >= 0.f ? x : INFINITY;
    }
    if (HAS_TERRAIN) {
      // cull, lane-parallel: lane j looks at boxes j and j + 64: world AABB of the box against the scan footprint, a
      // rectangle of half-sides (hx, hy) turned by the yaw - the four separating axes of a rectangle / AABB pair in the
      // plane, with 1 mm of slack (a vertical ray can only hit a box whose footprint contains it, so dropping the boxes
      // that do not overlap the rectangle changes no hit).  min() over the hits does not depend on the visiting order.
      const float hx = 0.5f * (PGTT_SCAN_H - 1) * fabsf(cfg->scan_dist_x) + 1e-3f, hy = 0.5f * (PGTT_SCAN_W - 1) * fabsf(cfg->scan_dist_y) + 1e-3f;
      const float acy = fabsf(cy), asy = fabsf(sy);
      // The survivors are COMPACTED into LDS (slot = number of surviving boxes before this one), prepared by the lane that owns them, and the ray
      // loop reads them from there through wave-uniform addresses, the next one requested while the current one is tested: no scalar-memory
      // round trip and no per-box arithmetic in the loop (a wave used to wait ~0.3 us for every 80-byte record; the slowest waves of a launch
      // are those that stand among many boxes).  kScanSlots survivors fit; further ones (never on the shipped terrains) are read from the table.
      constexpr int kScanSlots = 40;
      __shared__ float4 sh_box[kScanSlots * 3];
      unsigned long long todo[2];
      int nsurv = 0;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int b = lane + 64 * h;
        bool reach = false;
        if (b < a.B) {
          const float4 C = pf.brec[h];            // centre x, y; world-AABB half extents x, y
          const float dx = C.x - bx, dy = C.y - by;
          reach = (fabsf(dx) <= C.z + hx * acy + hy * asy) & (fabsf(dy) <= C.w + hx * asy + hy * acy) &
                  (fabsf(dx * cy + dy * sy) <= hx + C.z * acy + C.w * asy) & (fabsf(dy * cy - dx * sy) <= hy + C.z * asy + C.w * acy);
        }
        const unsigned long long mk = __ballot(reach);
        const int slot = nsurv + __popcll(mk & ((1ull << lane) - 1ull));
        if (reach && slot < kScanSlots) {
          // The lane that owns a surviving box prepares it for the ray loop - all survivors at once, one per lane.  A box turned about z only
          // (m20 = m21 = m02 = m12 = 0 exactly; every shipped / generated terrain) has lp2 = 0 * relx + 0 * rely + m22 * relz = round(m22 * relz)
          // with relz = oz - pz the same for every ray of the env: the parameters of its two z faces and their validity are properties of the
          // BOX (`hz` below, the value ray_box_down's two-face form returns for a ray inside the footprint); a ray only decides "inside or not".
          // Such a box goes to LDS as the 9 numbers that test needs; any other box as its index (the loop reads its record from the table).
          const float4 q0 = reinterpret_cast<const float4*>(pf.boxes + b)[0], q1 = reinterpret_cast<const float4*>(pf.boxes + b)[1], q2 = reinterpret_cast<const float4*>(pf.boxes + b)[2],
                       q3 = reinterpret_cast<const float4*>(pf.boxes + b)[3];
          const float m22 = q3.w;
          const bool fast = (q3.y == 0.f) & (q3.z == 0.f) & (m22 != 0.f) & (q2.y == 0.f) & (q3.x == 0.f);      // m20, m21, m22, m02, m12
          const float il2 = __builtin_amdgcn_rcpf(-m22);
          const float lp2 = mul_unfused(m22, oz - q0.z);       // a product on its own (the generic form adds it to two exact zeros): must not be fused into sz - lp2
          const float xt = (q1.z - lp2) * il2, xb = (-q1.z - lp2) * il2;
          float hz = xt >= 0.f ? xt : INFINITY;
          hz = ((xb >= 0.f) & (xb < hz)) ? xb : hz;
          sh_box[slot * 3 + 0] = make_float4(q0.x, q0.y, q1.w, q2.z);                    // px, py, m00, m10
          sh_box[slot * 3 + 1] = make_float4(q2.x, q2.w, q1.x, q1.y);                    // m01, m11, sx, sy
          sh_box[slot * 3 + 2] = make_float4(hz, fast ? 1.f : 0.f, __int_as_float(b), 0.f);
        }
        // boxes beyond the slots: the highest set bits of this half (slot order = bit order)
        int over = nsurv + __popcll(mk) - kScanSlots;
        unsigned long long rest = 0ull, t = mk;
        while (over > 0 && t != 0ull) { const int hb = 63 - __builtin_clzll(t); rest |= 1ull << hb; t &= ~(1ull << hb); over--; }
        todo[h] = rest;
        nsurv += __popcll(mk);
      }
      __syncthreads();
      const int nslot = min(nsurv, kScanSlots);
      auto load_slot = [&](int i, float4 (&r)[3]) {
#pragma unroll
        for (int q = 0; q < 3; q++) r[q] = sh_box[i * 3 + q];
      };
      auto test_box = [&](const float4 (&r)[3]) {
        if (__builtin_amdgcn_readfirstlane(__float_as_int(r[2].y)) != 0) {        // the record is the same in every lane: a scalar branch
          const float hz = r[2].x;
#pragma unroll
          for (int k = 0; k < 2; k++) {
            const float rx = org[k].x - r[0].x, ry = org[k].y - r[0].y;
            const float lp0 = r[0].z * rx + r[0].w * ry, lp1 = r[1].x * rx + r[1].y * ry;      // + m20 * relz = + (+-0): only the sign of a zero, and |lp| is what is tested
            const bool inside = (fabsf(lp0) <= r[1].z) & (fabsf(lp1) <= r[1].w);
            hit[k] = fminf(hit[k], inside ? hz : INFINITY);
          }
          return;
        }
        const TerrainBox tb = pf.boxes[__builtin_amdgcn_readfirstlane(__float_as_int(r[2].z))];
        const RayBox rb = ray_box_prepare(tb);
#pragma unroll
        for (int k = 0; k < 2; k++) hit[k] = fminf(hit[k], ray_box_down(tb, rb, org[k]));
      };
      float4 cur[3], nxt[3];
      if (nslot > 0) load_slot(0, cur);
      for (int i = 0; i < nslot; i++) {
        if (i + 1 < nslot) load_slot(i + 1, nxt);
        test_box(cur);
#pragma unroll
        for (int q = 0; q < 3; q++) cur[q] = nxt[q];
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        unsigned long long mk = todo[h];
        while (mk != 0ull) {
          const int b = 64 * h + __builtin_ctzll(mk);
          mk &= mk - 1ull;
          TerrainBox tb = pf.boxes[b];
          const RayBox rb = ray_box_prepare(tb);
#pragma unroll
          for (int k = 0; k < 2; k++) hit[k] = fminf(hit[k], ray_box_down(tb, rb, org[k]));
        }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
      float dist = hit[h] == INFINITY ? -1.0f : hit[h];
      sc.z[h] = org[h].z + (-1.0f) * dist;
      int idx = lane + 64 * h;
      if ((OMODE == OBS_STEP || OMODE == OBS_STEP_OBS) && a.scan_preset != 0) sc.z[h] = a.buf.scan_z[(long)e * PGTT_NSCAN + (idx < PGTT_NSCAN ? idx : 0)];   // test hook
      if (idx < PGTT_NSCAN) { sh_scan[idx] = sc.z[h]; a.buf.scan_z[(long)e * PGTT_NSCAN + idx] = sc.z[h]; }
    }
    sc.bz = bz;
  }

  // OBS_SCAN_LIFT: the base is set down on the highest scan point
  PG_INL void lift_base(const ObsScan& sc) {
    const bool v1 = lane + 64 < PGTT_NSCAN;
    const float zmax = wave_max(fmaxf(sc.z[0], v1 ? sc.z[1] : -INFINITY));
    if (lane == 0) S[(PGTT_S_QPOS + 2) * (long)N + e] = sc.bz + zmax;
  }

  PG_INL void quadrant_stats(uint2 cells, const ObsScan& sc, ObsQuad& q) {
    // ---------------- quadrant statistics (joystick_pgtt.py:169-190): n = 6 on both axes of the 13x9 grid
    {
      __syncthreads();                     // the scan is in LDS
      const char* const srcb = reinterpret_cast<const char*>(sh_src);
      const float c0 = *reinterpret_cast<const float*>(srcb + (cells.x & 0xffffu)), c1 = *reinterpret_cast<const float*>(srcb + (cells.x >> 16)),
                  c2 = *reinterpret_cast<const float*>(srcb + (cells.y & 0xffffu));
      float mx = fmaxf(fmaxf(c0, c1), c2), mn = fminf(fminf(c0, c1), c2);
      mx = row16_max(mx); mn = row16_min(mn);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        q.max[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mx), 16 * k));
        q.min[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mn), 16 * k));
      }
    }
    const bool v1 = lane + 64 < PGTT_NSCAN;
    q.zmin = wave_min(fminf(sc.z[0], v1 ? sc.z[1] : INFINITY));
  }

  PG_INL void env_constants() {
    // ---------------- per-env scalars (computed redundantly by every lane from LDS)
    // method 1 = the baseline task go2/joystick.py: no phase / gait_freq rows in the observation (162 / 206 instead of
    // 171 / 215), H_max = quadrant max, world-frame clearance target, 0.5 s air-time threshold
    OBSD = baseline ? PGTT_OBS_BASELINE : PGTT_OBS; PRIVD = OBSD + (PGTT_PRIV - PGTT_OBS);
    id = (unsigned)(a.env_off + e);
    ep = (unsigned)I[PGTT_I_RNG_CTR * (long)N + e];
    dt = cfg->ctrl_dt;
  }

  // the scalars of a reset env (Joystick.reset, joystick_pgtt.py:72-139) and the info arrays of its row image
  PG_INL void reset_scalars(TaskScalars& t) {
#pragma unroll
    for (int i = 0; i < 3; i++)
      t.cmd[i] = rng_uniform(a.seed, id, ep, PGTT_RS_RESET_CMD, i, a.rng_fix) * (cfg->cmd_u_max[i] - cfg->cmd_u_min[i]) + cfg->cmd_u_min[i];
    t.gait_freq = rng_uniform(a.seed, id, ep, PGTT_RS_RESET_FREQ, 0, a.rng_fix) * (cfg->gait_freq[1] - cfg->gait_freq[0]) + cfg->gait_freq[0];
    t.phase_dt = (float)(2 * M_PI) * dt * t.gait_freq;
    t.phase[0] = 0.f; t.phase[1] = (float)M_PI; t.phase[2] = (float)M_PI; t.phase[3] = 0.f;
#pragma unroll
    for (int f = 0; f < 4; f++) { t.air[f] = 0.f; t.peak[f] = 0.f; t.hmax[f] = 0.1f; t.hmin[f] = 0.f; t.last_contact[f] = 0.f; t.contact[f] = 0.f; t.first_contact[f] = 0.f; }
    t.timer = exp_timer(a.seed, id, ep, PGTT_RS_RESET_TIMER, dt, a.rng_fix);
    t.step_ctr = 0;
    __syncthreads();
    // info arrays that _get_obs reads
    if (lane < 12) { sh_st[PGTT_S_LAST_ACT + lane] = 0.f; sh_st[PGTT_S_LAST_LAST_ACT + lane] = 0.f; sh_st[PGTT_S_MOTOR_TARGETS + lane] = 0.f; }
    if (lane < 24) { sh_st[PGTT_S_QERR_HIST + lane] = 0.f; sh_st[PGTT_S_QVEL_HIST + lane] = 0.f; }
    __syncthreads();
  }

  // the scalars a step starts with; H_max / H_min from this scan
  PG_INL void step_scalars(const ObsQuad& q, TaskScalars& t) {
    t.step_ctr = I[PGTT_I_STEP * (long)N + e];
    t.timer = I[PGTT_I_STEPS_UNTIL_CMD * (long)N + e];
#pragma unroll
    for (int i = 0; i < 3; i++) t.cmd[i] = sh_st[PGTT_S_CMD + i];
    t.gait_freq = sh_st[PGTT_S_GAIT_FREQ]; t.phase_dt = sh_st[PGTT_S_PHASE_DT];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      task_foot_start(sh_st, sh_fr, dt, f, t);
      t.hmax[f] = baseline ? q.max[f] : q.max[f] - q.min[f]; t.hmin[f] = q.min[f];     // joystick.py:186 vs joystick_pgtt.py:189
    }
  }

  template <int OMODE> PG_INL void observation_rows(const ObsPrefetch& pf, const TaskScalars& t, float zmin, ObsHist& hs) {
    // ---------------- observation rows in LDS (joystick_pgtt.py:336-365)
    const float lvl = cfg->noise_level;
    // The noise draws of all rows in ONE Philox pass: the 147 noisy rows need 38 counter blocks (gyro 1, gravity 1, joint
    // positions 3, joint velocities 3, scan 30; rng_uniform(.., stream, idx) is word idx & 3 of block idx >> 2), lane j forms
    // block j and parks its four words in LDS - same draws as one rng_uniform call per row, a third of the multiplies.
    __shared__ unsigned sh_rng[64 * 4];
    static_assert(8 + (PGTT_NSCAN + 3) / 4 <= 64, "one lane per Philox block");
    {
      const int stream = lane == 0 ? PGTT_RS_GYRO : (lane == 1 ? PGTT_RS_GRAVITY : (lane < 5 ? PGTT_RS_QPOS : (lane < 8 ? PGTT_RS_QVEL : PGTT_RS_SCAN)));
      const int blk = lane < 2 ? 0 : (lane < 5 ? lane - 2 : (lane < 8 ? lane - 5 : lane - 8));
      unsigned c0 = id, c1 = ep, c2 = (unsigned)stream, c3 = (unsigned)blk;
      philox4x32_10((unsigned)a.seed, (unsigned)(a.seed >> 32), c0, c1, c2, c3);
      sh_rng[4 * lane + 0] = c0; sh_rng[4 * lane + 1] = c1; sh_rng[4 * lane + 2] = c2; sh_rng[4 * lane + 3] = c3;
    }
    // the per-env scalars the rows draw on, next to the rows' other sources (the phase rows are there since the yaw was formed): gait frequency, command, last contact, air time, the five noise scales and the twelve joint offsets
    if (lane < 12) sh_drv[OD_OFFS + 1 + lane] = m->key_qpos[7 + lane];
    if (lane == 0) {
      sh_drv[OD_GAIT] = t.gait_freq; sh_drv[OD_ZERO] = 0.f; sh_drv[OD_OFFS] = 0.f;
#pragma unroll
      for (int k = 0; k < 3; k++) sh_drv[OD_CMD + k] = t.cmd[k];
#pragma unroll
      for (int f = 0; f < 4; f++) { sh_drv[OD_LASTC + f] = t.last_contact[f]; sh_drv[OD_AIR + f] = t.air[f]; }
      sh_drv[OD_SCALE + 0] = 0.f; sh_drv[OD_SCALE + 1] = cfg->noise_gyro; sh_drv[OD_SCALE + 2] = cfg->noise_gravity;
      sh_drv[OD_SCALE + 3] = cfg->noise_joint_pos; sh_drv[OD_SCALE + 4] = cfg->noise_joint_vel; sh_drv[OD_SCALE + 5] = cfg->noise_heightscan;
    }
    __syncthreads();
    const char* const srcb = reinterpret_cast<const char*>(sh_src);
#pragma unroll
    for (int it = 0; it < 3; it++) {
      const int io = lane + 64 * it;
      if (io >= OBSD) continue;
      // every row is (base + noise) - offset with noise = (2u - 1) * level * scale (rows without noise read a word too, with scale 0; rows
      // without an offset subtract the table's zero: x - 0 is x)
      const unsigned d = pf.rdesc[it], so = (d >> 21) & 0x1fu;
      const float base0 = *reinterpret_cast<const float*>(srcb + (d & 0x7ffu));
      const unsigned word = *reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(sh_rng) + ((d >> 11) & 0x3ffu));
      const float scale = *reinterpret_cast<const float*>(srcb + (OL_DRV + OD_SCALE) * 4 + so);
      const float offs = *reinterpret_cast<const float*>(srcb + (OL_DRV + OD_OFFS) * 4 + (d >> 26));
      const float base = base0 - (so == 20u ? zmin : 0.f);              // scan rows are heights above the lowest scan point
      const float uw = (float)(word >> 8) * (1.0f / 16777216.0f);
      const float u = a.rng_fix == a.rng_fix ? a.rng_fix : uw;
      const float noisy = scale != 0.f ? base + (2.f * u - 1.f) * lvl * scale : base;
      sh_obs[io] = noisy - offs;
    }
    if (lane < PGTT_PRIV - PGTT_OBS) sh_obs[OBSD + OBSD + lane] = *reinterpret_cast<const float*>(srcb + pf.psrc);
    // privileged extras 41..43: the force on the torso during this step (xfrc_applied[torso, :3], joystick_pgtt.py:364); 0 without a wrench buffer
    // and in the observation of a reset
    if ((OMODE == OBS_STEP || OMODE == OBS_STEP_OBS) && a.buf.xfrc && lane >= 41 && lane < 44) sh_obs[OBSD + OBSD + lane] = a.buf.xfrc[(lane - 41) * (long)N + e];
    // history buffers (joystick_pgtt.py:319-334): motor_targets in sh_st was written by the physics kernel
    hs.q = 0.f; hs.v = 0.f; hs.upd = (t.step_ctr % cfg->history_update_steps) == 0;
    if (lane < 24) {
      if (hs.upd) {
        hs.v = lane < 12 ? sh_st[PGTT_S_QVEL + 6 + lane] : sh_st[PGTT_S_QVEL_HIST + lane - 12];
        hs.q = lane < 12 ? sh_st[PGTT_S_QPOS + 7 + lane] - sh_st[PGTT_S_MOTOR_TARGETS + lane] : sh_st[PGTT_S_QERR_HIST + lane - 12];
      } else { hs.v = sh_st[PGTT_S_QVEL_HIST + lane]; hs.q = sh_st[PGTT_S_QERR_HIST + lane]; }
    }
    __syncthreads();
    for (int i = lane; i < OBSD; i += 64) sh_obs[OBSD + i] = sh_obs[i];     // privileged = state || extras
    __syncthreads();
  }

  PG_INL void store_split(const TaskScalars& t) {
    // scan + observation half: H_max / H_min of this scan for task_kernel, the observation rows (a finished episode's
    // rows are replaced by task_kernel), nothing else
    if (lane < 4) {
      S[(PGTT_S_HMAX + lane) * (long)N + e] = sel4(lane, t.hmax[0], t.hmax[1], t.hmax[2], t.hmax[3]);
      S[(PGTT_S_HMIN + lane) * (long)N + e] = sel4(lane, t.hmin[0], t.hmin[1], t.hmin[2], t.hmin[3]);
    }
    for (int i = lane; i < OBSD; i += 64) a.buf.obs_state[(long)e * OBSD + i] = sh_obs[i];
    for (int i = lane; i < PRIVD; i += 64) a.buf.obs_priv[(long)e * PRIVD + i] = sh_obs[OBSD + i];
  }

  template <int OMODE> PG_INL void wrap_and_store(const ObsPrefetch& pf, const TaskScalars& t, const ObsHist& hs, int ep_steps, bool prev_done) {
    // ---------------- Episode / AutoReset wrapper semantics (UPSTREAM-RECALL)
    float act_i = 0.f;
    if (OMODE == OBS_STEP && lane < 12) act_i = sh_act[lane];
    bool wdone = t.done;
    if (OMODE == OBS_STEP && cfg->autoreset) {
      ep_steps += 1;
      if (ep_steps >= cfg->episode_length) wdone = true;
    }
    // Every value below is the same in all lanes (a per-env scalar in a vector register).  Lane 0 parks them in LDS - the new values of the
    // env's state rows in their slots of the row image sh_st, the metrics with (reward, 1) behind them - and the wave then stores ROW RANGES
    // with one address per lane; picking "my row's value" out of registers costs a compare + select per candidate (22 for a metric) and a
    // 64-bit address per store site, in a kernel whose four waves per SIMD share the vector ALU.
    // AutoReset of a finished episode: the first state and its observation are requested HERE, all at once (the copy loops at the end of the
    // wave were eight dependent round trips - each store could alias the next load - and the few waves with a finished episode were the last
    // of the launch to leave)
    const bool restore = OMODE == OBS_STEP && cfg->autoreset && wdone && a.buf.first_state && a.buf.first_obs;
    constexpr int kFirstObsPasses = (PGTT_OBS + PGTT_PRIV + 63) / 64;
    float first_st = 0.f, first_ob[kFirstObsPasses];
    if (restore) {
      if (lane < PGTT_S_CMD) first_st = a.buf.first_state[lane * (long)N + e];
      const float* __restrict__ fo = a.buf.first_obs + (long)e * (OBSD + PRIVD);
#pragma unroll
      for (int i = 0; i < kFirstObsPasses; i++) first_ob[i] = lane + 64 * i < OBSD + PRIVD ? fo[lane + 64 * i] : 0.f;
    }
    __shared__ float sh_met[PGTT_NMETRIC + 2];
    __syncthreads();                       // the row image has been read for the last time (rewards, history)
    if (lane < 12) {
      const float prev = sh_st[PGTT_S_LAST_ACT + lane];
      sh_st[PGTT_S_LAST_LAST_ACT + lane] = OMODE == OBS_STEP ? prev : 0.f;
      sh_st[PGTT_S_LAST_ACT + lane] = OMODE == OBS_STEP ? act_i : 0.f;
      if (OMODE != OBS_STEP) sh_st[PGTT_S_MOTOR_TARGETS + lane] = 0.f;
    }
    if (lane < 24) { sh_st[PGTT_S_QVEL_HIST + lane] = hs.v; sh_st[PGTT_S_QERR_HIST + lane] = hs.q; }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 3; i++) sh_st[PGTT_S_CMD + i] = t.cmd[i];
#pragma unroll
      for (int f = 0; f < 4; f++) {
        sh_st[PGTT_S_PHASE + f] = t.phase[f]; sh_st[PGTT_S_AIR_TIME + f] = t.air[f]; sh_st[PGTT_S_SWING_PEAK + f] = t.peak[f];
        sh_st[PGTT_S_HMAX + f] = t.hmax[f]; sh_st[PGTT_S_HMIN + f] = t.hmin[f]; sh_st[PGTT_S_LAST_CONTACT + f] = t.last_contact[f];
      }
      sh_st[PGTT_S_PHASE_DT] = t.phase_dt; sh_st[PGTT_S_GAIT_FREQ] = t.gait_freq;
#pragma unroll
      for (int k = 0; k < PGTT_NMETRIC; k++) sh_met[k] = t.metrics[k];
      sh_met[PGTT_NMETRIC] = t.reward; sh_met[PGTT_NMETRIC + 1] = 1.0f;
    }
    __syncthreads();
    if (OMODE == OBS_STEP && cfg->autoreset && a.buf.ep_metrics && lane < PGTT_NMETRIC + 2)
      a.buf.ep_metrics[lane * (long)N + e] = (pf.epm_old + sh_met[lane]) * (prev_done ? 0.f : 1.f);

    // ---------------- stores: rows PGTT_S_CMD .. PGTT_NSTATE - 1 of the image (the step leaves the motor targets, which are the physics kernel's, alone)
    static_assert(PGTT_NSTATE - PGTT_S_CMD <= 128 && PGTT_NMETRIC + 2 <= 64, "two passes over the rows, one over the t.metrics");
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int r = PGTT_S_CMD + lane + 64 * h;
      // the step leaves the histories alone except on the steps that shift them (1 in history_update_steps)
      const bool mine = r < PGTT_NSTATE && (OMODE != OBS_STEP || r < PGTT_S_MOTOR_TARGETS || r >= PGTT_S_LAST_CONTACT || (hs.upd && r >= PGTT_S_QERR_HIST));
      if (mine) S[r * (long)N + e] = sh_st[r];
    }
    if (lane == 0) {
      I[PGTT_I_STEP * (long)N + e] = t.step_ctr; I[PGTT_I_STEPS_UNTIL_CMD * (long)N + e] = t.timer;
      I[PGTT_I_RNG_CTR * (long)N + e] = (int)(ep + 1u); I[PGTT_I_EP_STEPS * (long)N + e] = ep_steps;
      a.buf.reward[e] = t.reward; a.buf.done[e] = wdone ? 1.f : 0.f;
    }
    if (lane < PGTT_NMETRIC) {
      const float v = sh_met[lane];
      a.buf.metrics[lane * (long)N + e] = v;
    }
    if (OMODE == OBS_STEP && a.buf.interval_sums && lane < PGTT_NMETRIC + 2)
      a.buf.interval_sums[lane * (long)N + e] = pf.ivs_old + (lane < PGTT_NMETRIC ? sh_met[lane] : (lane == PGTT_NMETRIC ? t.reward : (wdone ? 1.f : 0.f)));
    if (restore) {                         // the first observation takes the place of this step's in LDS (same layout: state rows, then privileged rows)
      static_assert(PGTT_S_CMD <= 64, "one lane per restored state row");
      if (lane < PGTT_S_CMD) S[lane * (long)N + e] = first_st;
#pragma unroll
      for (int i = 0; i < kFirstObsPasses; i++) if (lane + 64 * i < OBSD + PRIVD) sh_obs[lane + 64 * i] = first_ob[i];
      __syncthreads();
    }
    for (int i = lane; i < OBSD; i += 64) a.buf.obs_state[(long)e * OBSD + i] = sh_obs[i];
    for (int i = lane; i < PRIVD; i += 64) a.buf.obs_priv[(long)e * PRIVD + i] = sh_obs[OBSD + i];
    if (OMODE == OBS_RESET) {
      if (a.buf.first_state) for (int r = lane; r < PGTT_S_CMD; r += 64) a.buf.first_state[r * (long)N + e] = sh_st[r];
      if (a.buf.first_obs) for (int i = lane; i < OBSD + PRIVD; i += 64) a.buf.first_obs[(long)e * (OBSD + PRIVD) + i] = sh_obs[i];
      if (a.buf.ep_metrics) for (int k = lane; k < PGTT_NMETRIC + 2; k += 64) a.buf.ep_metrics[k * (long)N + e] = 0.f;
    }
  }
};

template <int OMODE, bool HAS_TERRAIN>
// four waves per SIMD (128 VGPRs): the kernel is latency-bound, a launch lasts as long as the resident waves of a SIMD take in turn
__global__ __launch_bounds__(64, 4) void observe_kernel(KArgs a, const float* __restrict__ action) {
  const int e = xcd_block(blockIdx.x, gridDim.x), lane = threadIdx.x, N = a.N;
  if (OMODE != OBS_STEP && OMODE != OBS_STEP_OBS && a.mask && !a.mask[e]) return;

  __shared__ float sh_src[OL_END];
  __shared__ float sh_obs[PGTT_OBS + PGTT_PRIV + 2];
  __shared__ float sh_act[12];
  ObserveWave w{a, e, lane, N, a.model, a.cfg, a.buf.state, a.buf.istate, sh_src, sh_src + OL_ST, sh_src + OL_FR, sh_src + OL_SCAN, sh_src + OL_DRV, sh_obs, sh_act};
  ObsPrefetch pf; ObsScan sc;
  w.template load_rows<OMODE, HAS_TERRAIN>(action, pf);              // every mode: the row image, the prefetches
  w.template height_scan<OMODE, HAS_TERRAIN>(pf, sc);                // every mode: yaw, cull, rays; scan_z
  if (OMODE == OBS_SCAN_ONLY) return;
  if (OMODE == OBS_SCAN_LIFT) { w.lift_base(sc); return; }
  // OBS_STEP, OBS_STEP_OBS, OBS_RESET: the observation
  ObsQuad q; ObsHist hs; TaskScalars t;
  w.quadrant_stats(pf.qcell, sc, q);
  w.env_constants();
  int ep_steps = 0; bool prev_done = false;       // Episode / AutoReset wrapper state
  if (OMODE == OBS_RESET) w.reset_scalars(t);
  else {
    ep_steps = w.I[PGTT_I_EP_STEPS * (long)N + e];
    prev_done = w.cfg->autoreset && a.buf.done[e] != 0.f;
    if (prev_done) ep_steps = 0;
    w.step_scalars(q, t);
  }
  w.template observation_rows<OMODE>(pf, t, q.zmin, hs);
  if (OMODE == OBS_STEP_OBS) { w.store_split(t); return; }         // the split form ends here: task_kernel does the rest
  // OBS_STEP: rewards, termination, bookkeeping; OBS_RESET: none
  t.reward = 0.f; t.done = false;
#pragma unroll
  for (int k = 0; k < PGTT_NMETRIC; k++) t.metrics[k] = 0.f;
  if (OMODE == OBS_STEP) task_rewards<true>(w.sh_st, w.sh_fr, w.sh_act, w.cfg, w.m, w.baseline, a.seed, w.id, w.ep, w.dt, a.rng_fix, t);
  w.template wrap_and_store<OMODE>(pf, t, hs, ep_steps, prev_done);    // OBS_STEP, OBS_RESET
}


// ------------------------------------------------------------------ interval reduction: one block per row of interval_sums
// out[k] (+)= sum over the envs of row k, and the row is cleared: read, zero and reduce in one pass (a GEMV, a fill and an add otherwise);
// block `rows` only hands the caller's env-step count over
__global__ __launch_bounds__(256) void interval_reduce_kernel(float* __restrict__ sums, int N, int rows, float* __restrict__ acc, float env_steps, int accumulate) {
  if ((int)blockIdx.x == rows) { if (threadIdx.x == 0) acc[rows] = (accumulate ? acc[rows] : 0.f) + env_steps; return; }
  float* __restrict__ row = sums + (long)blockIdx.x * N;
  float s = 0.f;
  if ((N & 3) == 0) {
    float4* __restrict__ row4 = reinterpret_cast<float4*>(row);
    for (int i = threadIdx.x; i < (N >> 2); i += 256) { const float4 v = row4[i]; row4[i] = make_float4(0.f, 0.f, 0.f, 0.f); s += (v.x + v.y) + (v.z + v.w); }
  } else {
    for (int i = threadIdx.x; i < N; i += 256) { s += row[i]; row[i] = 0.f; }
  }
  s = row16_sum(s);                                      // the 16 lanes of a DPP row, then the rows and the waves through LDS
  __shared__ float part[16];
  if ((threadIdx.x & 15) == 0) part[threadIdx.x >> 4] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) t += part[i];
    acc[blockIdx.x] = (accumulate ? acc[blockIdx.x] : 0.f) + t;
  }
}

// ------------------------------------------------------------------ task: one env per LANE (coalesced SoA rows)
// The per-env scalar half of a control step: contact bookkeeping, the 21 rewards, termination, command resampling,
// history buffers, Episode / AutoReset wrapper semantics.  In the fused observe kernel every wave repeats this ~2.5 k
// instruction stream for ONE env; here a wave does it for 64.  Runs after observe_kernel<OBS_STEP_OBS>, which left
// H_max / H_min of the current scan in the state rows and wrote the observation rows.
__global__ __launch_bounds__(64) void task_kernel(KArgs a, const float* __restrict__ action) {
  const int N = a.N;
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= N) return;
  const PgttModel* __restrict__ m = a.model;
  const PgttConfig* __restrict__ cfg = a.cfg;
  float* __restrict__ S = a.buf.state;
  int* __restrict__ I = a.buf.istate;
  const float* __restrict__ Fr = a.buf.frame;
  // rows this half reads, as per-lane arrays with compile-time indices (registers)
  float st[PGTT_NSTATE], fr[PGTT_NFRAME], act[12];
#pragma unroll
  for (int r = 0; r < PGTT_S_QWARM; r++) st[r] = S[r * (long)N + e];                      // qpos, qvel
#pragma unroll
  for (int r = PGTT_S_CMD; r < PGTT_NSTATE; r++) st[r] = S[r * (long)N + e];              // task rows
#pragma unroll
  for (int r = 0; r < PGTT_NFRAME; r++) fr[r] = Fr[r * (long)N + e];
#pragma unroll
  for (int i = 0; i < 12; i++) act[i] = action[(long)e * 12 + i];
  const bool baseline = cfg->method == PGTT_METHOD_BASELINE;
  const int OBSD = baseline ? PGTT_OBS_BASELINE : PGTT_OBS, PRIVD = OBSD + (PGTT_PRIV - PGTT_OBS);
  const unsigned id = (unsigned)(a.env_off + e);
  const unsigned ep = (unsigned)I[PGTT_I_RNG_CTR * (long)N + e];
  int ep_steps = I[PGTT_I_EP_STEPS * (long)N + e];
  const float dt = cfg->ctrl_dt;
  const bool prev_done = cfg->autoreset && a.buf.done[e] != 0.f;
  if (prev_done) ep_steps = 0;
  TaskScalars t;
  t.step_ctr = I[PGTT_I_STEP * (long)N + e]; t.timer = I[PGTT_I_STEPS_UNTIL_CMD * (long)N + e];
#pragma unroll
  for (int i = 0; i < 3; i++) t.cmd[i] = st[PGTT_S_CMD + i];
  t.phase_dt = st[PGTT_S_PHASE_DT];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    task_foot_start(st, fr, dt, f, t);
    t.hmax[f] = st[PGTT_S_HMAX + f];                                                     // of the current scan
  }
  // history buffers (joystick_pgtt.py:319-334) use the step counter BEFORE it advances
  float hist_q[24], hist_v[24];
  const bool upd = (t.step_ctr % cfg->history_update_steps) == 0;
#pragma unroll
  for (int i = 0; i < 24; i++) {
    const float nv = i < 12 ? st[PGTT_S_QVEL + 6 + (i < 12 ? i : 0)] : st[PGTT_S_QVEL_HIST + (i >= 12 ? i - 12 : 0)];
    const float nq = i < 12 ? st[PGTT_S_QPOS + 7 + (i < 12 ? i : 0)] - st[PGTT_S_MOTOR_TARGETS + (i < 12 ? i : 0)] : st[PGTT_S_QERR_HIST + (i >= 12 ? i - 12 : 0)];
    hist_v[i] = upd ? nv : st[PGTT_S_QVEL_HIST + i];
    hist_q[i] = upd ? nq : st[PGTT_S_QERR_HIST + i];
  }
  task_rewards<false>(st, fr, act, cfg, m, baseline, a.seed, id, ep, dt, a.rng_fix, t);
  // Episode / AutoReset wrapper semantics
  bool wdone = t.done;
  if (cfg->autoreset) {
    ep_steps += 1;
    if (ep_steps >= cfg->episode_length) wdone = true;
    if (a.buf.ep_metrics) {
      const float keep = prev_done ? 0.f : 1.f;
#pragma unroll
      for (int k = 0; k < PGTT_NMETRIC + 2; k++) {
        const float add = k < PGTT_NMETRIC ? t.metrics[k < PGTT_NMETRIC ? k : 0] : (k == PGTT_NMETRIC ? t.reward : 1.0f);
        float* p = a.buf.ep_metrics + k * (long)N + e;
        *p = (*p + add) * keep;
      }
    }
  }
  // stores
#pragma unroll
  for (int i = 0; i < 3; i++) S[(PGTT_S_CMD + i) * (long)N + e] = t.cmd[i];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    S[(PGTT_S_PHASE + f) * (long)N + e] = t.phase[f];
    S[(PGTT_S_AIR_TIME + f) * (long)N + e] = t.air[f];
    S[(PGTT_S_SWING_PEAK + f) * (long)N + e] = t.peak[f];
    S[(PGTT_S_LAST_CONTACT + f) * (long)N + e] = t.last_contact[f];
  }
#pragma unroll
  for (int i = 0; i < 24; i++) { S[(PGTT_S_QVEL_HIST + i) * (long)N + e] = hist_v[i]; S[(PGTT_S_QERR_HIST + i) * (long)N + e] = hist_q[i]; }
#pragma unroll
  for (int i = 0; i < 12; i++) { S[(PGTT_S_LAST_LAST_ACT + i) * (long)N + e] = st[PGTT_S_LAST_ACT + i]; S[(PGTT_S_LAST_ACT + i) * (long)N + e] = act[i]; }
  I[PGTT_I_STEP * (long)N + e] = t.step_ctr; I[PGTT_I_STEPS_UNTIL_CMD * (long)N + e] = t.timer;
  I[PGTT_I_RNG_CTR * (long)N + e] = (int)(ep + 1u); I[PGTT_I_EP_STEPS * (long)N + e] = ep_steps;
  a.buf.reward[e] = t.reward; a.buf.done[e] = wdone ? 1.f : 0.f;
#pragma unroll
  for (int k = 0; k < PGTT_NMETRIC; k++) a.buf.metrics[k * (long)N + e] = t.metrics[k];
  if (a.buf.interval_sums) {
#pragma unroll
    for (int k = 0; k < PGTT_NMETRIC; k++) a.buf.interval_sums[k * (long)N + e] += t.metrics[k];
    a.buf.interval_sums[PGTT_NMETRIC * (long)N + e] += t.reward;
    a.buf.interval_sums[(PGTT_NMETRIC + 1) * (long)N + e] += wdone ? 1.f : 0.f;
  }
  // AutoReset: a finished episode continues from the env's first state and first observation
  if (cfg->autoreset && wdone && a.buf.first_state && a.buf.first_obs) {
    for (int r = 0; r < PGTT_S_CMD; r++) S[r * (long)N + e] = a.buf.first_state[r * (long)N + e];
    const float* fo = a.buf.first_obs + (long)e * (OBSD + PRIVD);
    for (int i = 0; i < OBSD; i++) a.buf.obs_state[(long)e * OBSD + i] = fo[i];
    for (int i = 0; i < PRIVD; i++) a.buf.obs_priv[(long)e * PRIVD + i] = fo[OBSD + i];
  }
}

// number of labels outside [0, T): the step kernels clamp such a label (no out-of-bounds read), pgtt_reset reports it
__global__ void variant_range_kernel(const int32_t* __restrict__ variant, int N, int T, int* __restrict__ bad) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const bool out = e < N && (variant[e] < 0 || variant[e] >= T);
  const unsigned long long b = __ballot(out);
  if (b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(bad, __popcll(b));
}
}  // namespace pgtt

template <int OMODE>
static void launch_observe(hipStream_t st, const pgtt::KArgs& a, const float* action) {
  dim3 grid(a.N), block(64);
  if (a.T > 0) hipLaunchKernelGGL((pgtt::observe_kernel<OMODE, true>), grid, block, 0, st, a, action);
  else hipLaunchKernelGGL((pgtt::observe_kernel<OMODE, false>), grid, block, 0, st, a, action);
}
void pgtt_launch_observe(int omode, hipStream_t st, const pgtt::KArgs& a, const float* action) {
  switch (omode) {
    case pgtt::OBS_STEP: return launch_observe<pgtt::OBS_STEP>(st, a, action);
    case pgtt::OBS_SCAN_LIFT: return launch_observe<pgtt::OBS_SCAN_LIFT>(st, a, action);
    case pgtt::OBS_RESET: return launch_observe<pgtt::OBS_RESET>(st, a, action);
    case pgtt::OBS_SCAN_ONLY: return launch_observe<pgtt::OBS_SCAN_ONLY>(st, a, action);
    case pgtt::OBS_STEP_OBS: return launch_observe<pgtt::OBS_STEP_OBS>(st, a, action);
  }
}
void pgtt_launch_task(hipStream_t st, const pgtt::KArgs& a, const float* action) {
  hipLaunchKernelGGL(pgtt::task_kernel, dim3((a.N + 63) / 64), dim3(64), 0, st, a, action);
}
void pgtt_launch_reset_pose(hipStream_t st, const pgtt::KArgs& a) {
  hipLaunchKernelGGL(pgtt::reset_pose_kernel, dim3((a.N + 63) / 64), dim3(64), 0, st, a);
}
void pgtt_launch_push(hipStream_t st, const pgtt::KArgs& a) {
  hipLaunchKernelGGL(pgtt::push_kernel, dim3((a.N + 63) / 64), dim3(64), 0, st, a);
}
void pgtt_launch_interval_reduce(hipStream_t st, float* sums, int N, int rows, float* acc, float env_steps, int accumulate) {
  hipLaunchKernelGGL(pgtt::interval_reduce_kernel, dim3(rows + 1), dim3(256), 0, st, sums, N, rows, acc, env_steps, accumulate);
}
void pgtt_launch_variant_range(hipStream_t st, const int32_t* variant, int N, int T, int* bad) {
  hipLaunchKernelGGL(pgtt::variant_range_kernel, dim3((N + 63) / 64), dim3(64), 0, st, variant, N, T, bad);
}
