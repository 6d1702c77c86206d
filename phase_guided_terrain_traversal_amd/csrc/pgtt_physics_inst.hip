// One physics_kernel instantiation per translation unit (-DPG_MODE, -DPG_DR, -DPG_TERRAIN, -DPG_SUBS: csrc/flags.mk) so that the
// variants compile in parallel; each exports a plain host launcher that pgtt_api.hip finds through the generated variant list.
//
//   physics_kernel  : one env per 4, 8 or 16 lanes (lane = leg [x sub-lane]; 16, 8 or 4 envs per 64-thread block, see
//                     pgtt_physics_quad.hip.h), DPP reductions.  MODE_STEP = mjx_env.step (n_substeps x
//                     {forward, Euler}) + sensor frame + contact flags; MODE_FORWARD = one mjx.forward
//                     (reset path).  Reference: go2/joystick_pgtt.py:146-148, :72, :78.
#include "pgtt_physics_quad.hip.h"

namespace pgtt {

// ------------------------------------------------------------------ physics: one env per 4 * SUBS lanes (layouts: see pgtt_physics_quad.hip.h)
// SUBS is part of the kernel's name only (the layout itself is the translation unit's PG_SUBS).
template <int MODE, bool HAS_DR, bool HAS_TERRAIN, int SUBS>
__global__ __launch_bounds__(64) void physics_kernel(KArgs a, const float* __restrict__ action) {
  static_assert(SUBS == kSubs, "one lane layout per translation unit");
  constexpr bool kStep = MODE != MODE_FORWARD;         // MODE_STEP or MODE_STEP_XFRC
  const int N = a.N;
  const int l = lane_leg();                            // leg FL,FR,RL,RR
  const int blk = xcd_block(blockIdx.x, gridDim.x);
  int e = blk * kEnvsPerWave + lane_env();
  bool valid = e < N;
  if (!valid) e = N - 1;                               // keep whole quads running (DPP), suppress the stores
  if (!kStep && a.mask && !a.mask[e]) valid = false;
  // Hex layout: the model constants (sizeof(PgttModel) = 2.5 KB, read ~100 times per substep through uniform or per-leg addresses) are staged
  // in LDS once per launch: with one wave per SIMD every wait for a vector-memory round trip is exposed, and an LDS read returns in about
  // half the time of an L1 hit (80 global loads of the step kernel became LDS reads: bit-identical, level4 168.0 -> 166.7 us, flat 118.1 ->
  // 115.9 us at 4096 envs).  Not in the oct layout, where the change costs 52 B of scratch per lane and 0.5 - 0.8 %.
  // Order of the prologue: the variant index first (two dependent round trips hang on it: index -> box records), then every other load of
  // the launch - model image, per-env model, state rows, action - and ONE barrier behind all the staging stores; the prologue reads the
  // model through its global pointer (gm), everything after the barrier through `m`.
  __shared__ unsigned sh_model[kSubs == 4 ? (sizeof(PgttModel) + 3) / 4 : 1];
  const PgttModel* __restrict__ gm = a.model;
  // a label outside [0, T) would index past the terrain tables: clamped (v_med3, identity for a valid label; pgtt_reset reports such labels as PGTT_E_ARG)
  const int variant = (HAS_TERRAIN && a.buf.variant) ? min(max(a.buf.variant[e], 0), a.T - 1) : 0;
  constexpr int kModelWords = (int)((sizeof(PgttModel) + 3) / 4), kModelTrips = (kModelWords + 63) / 64;
  unsigned mw[kSubs == 4 ? kModelTrips : 1];
  if (kSubs == 4) {
#pragma unroll
    for (int t = 0; t < kModelTrips; t++) { const int i = t * 64 + (int)threadIdx.x; mw[t] = reinterpret_cast<const unsigned*>(a.model)[i < kModelWords ? i : 0]; }
  }
  const PgttConfig* __restrict__ cfg = a.cfg;
  float* __restrict__ S = a.buf.state;
  // Base-body rows are stored by ALL four lanes of the quad (same address, bit-identical value): the kernel has no
  // region in which only part of a quad is active while replicated state is live ("quad invariants").
  const bool lead = valid;

  QEnvModel em;
  qload_env_model<HAS_DR>(gm, a.buf.params, N, e, l, em);
  QSim s;
#pragma unroll
  for (int i = 0; i < 7; i++) s.qb[i] = PG_ROW(S, PGTT_S_QPOS + i, N, e);
#pragma unroll
  for (int i = 0; i < 6; i++) { s.vb[i] = PG_ROW(S, PGTT_S_QVEL + i, N, e); s.wb[i] = PG_ROW(S, PGTT_S_QWARM + i, N, e); }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int j = 3 * l + k, ac = 3 * (l ^ 1) + k;     // joint index, actuator index driving it
    s.ql[k] = PG_ROW(S, PGTT_S_QPOS + 7 + j, N, e);
    s.vl[k] = PG_ROW(S, PGTT_S_QVEL + 6 + j, N, e);
    s.wl[k] = PG_ROW(S, PGTT_S_QWARM + 6 + j, N, e);
    if (kStep) s.ctrl[k] = gm->key_qpos[7 + ac] + PG_REC(action, e, 12, ac) * cfg->action_scale;
    else s.ctrl[k] = PG_ROW(S, PGTT_S_QPOS + 7 + ac, N, e);          // mjx_env.init(ctrl = qpos[7:])
  }
  const TerrainBox* boxes = nullptr;
  const uint4* grid_v = nullptr;
  unsigned box0 = 0u, cell0 = 0u;       // PG_ADDR32: first box / grid cell of the env's variant as 32-bit element indices from the tables' bases
  int nbox = 0;
  // LDS staging of the env's terrain variant: centre + bounding radius of its <=100 boxes (read 2 x 4 substeps
  // by the broad phase), and a per-lane column for the broad-phase keys of the own foot
  __shared__ float4 sh_box[HAS_TERRAIN && kBoxLds ? PGTT_MAX_BOX * kEnvsPerWave : 1];      // (cx, cy, cz, hx)
  __shared__ float2 sh_box2[HAS_TERRAIN && kBoxLds ? PGTT_MAX_BOX * kEnvsPerWave : 1];     // (hy, hz)
  __shared__ float sh_con[HAS_TERRAIN ? kMaxB * kSlotFields * kSlotCols : 1];
  const int quad = lane_env();                         // env within the wave
  const BoxSlots slots{sh_con, lane_col()};
  if (HAS_TERRAIN) {
#if PG_ADDR32
    boxes = a.terrain; grid_v = a.grid;
    box0 = (unsigned)variant * (unsigned)a.B; cell0 = (unsigned)variant * (unsigned)(kGridG * kGridG);
#else
    boxes = a.terrain + (long)variant * a.B;
    grid_v = a.grid + (long)variant * (kGridG * kGridG);
#endif
    nbox = a.B;
    for (int b = lane_in_env(); kBoxLds && b < nbox; b += 4 * kSubs) {
      const TerrainBox* tb = PG_ADDR32 ? &pg_at(boxes, box0 + (unsigned)b) : boxes + b;
      sh_box[b * kEnvsPerWave + quad] = make_float4(tb->px, tb->py, tb->pz, tb->hx);
      sh_box2[b * kEnvsPerWave + quad] = make_float2(tb->hy, tb->hz);
    }
    slots.clear_all();
  }
  const PgttModel* __restrict__ m = gm;
  if (kSubs == 4) {
#pragma unroll
    for (int t = 0; t < kModelTrips; t++) { const int i = t * 64 + (int)threadIdx.x; if (i < kModelWords) sh_model[i] = mw[t]; }
    m = reinterpret_cast<const PgttModel*>(sh_model);
  }
  if (HAS_TERRAIN || kSubs == 4) __syncthreads();
  s.niter = 0; s.niter_max = 0; s.pen_overflow = false;
  QPhysics ph(m, em, s, l);
  QSolver sol(m, s, slots);
  sol.lds_slots = HAS_TERRAIN && nbox > 0;
  const int nsub = kStep ? cfg->n_substeps : 1;
  const float dt = m->timestep;
  for (int sub = 0; sub < nsub; sub++) {
    ph.kinematics();
    if (HAS_TERRAIN) ph.collide(boxes, box0, nbox, sh_box, sh_box2, slots, quad, grid_v, cell0, a.grid_E, a.grid_inv); else s.nbox = 0;
    ph.inertia();
    ph.velocity_stage<MODE == MODE_STEP_XFRC>(a.buf.xfrc, N, e);      // the reset's forward pass applies no wrench
    ph.constraint_stage(HAS_TERRAIN && boxes != nullptr && nbox > 0, a.buf.box_friction, N, e, slots);
    // ---- sensors of the last forward (pre-integration state), written BEFORE the solve; the accelerometer is an affine map of
    //      qacc[0:6]: its constant part is kept across the solve (3 values), the 3 x 6 matrix is formed after it from frames that are
    //      still live (R0, cdr, imu, com) - 18 registers less across the Newton loop of a kernel that spills to scratch
    float acc0[3];
    const bool last = sub == nsub - 1;
    if (last) {
      float* __restrict__ Fr = a.buf.frame;
      int ee = e; asm volatile("" : "+v"(ee));     // re-form the row addresses here (see the final stores)
      V3 w = s.cvel0.a, vl = s.cvel0.l;
      V3 dif = s.imu - s.com;
      V3 gyro = mtmul(s.R0, w);
      V3 glin = vl - cross(dif, w);
      V3 llin = mtmul(s.R0, glin);
      S6 cacc{v3(0, 0, 0), v3(-m->gravity[0], -m->gravity[1], -m->gravity[2])};
#pragma unroll
      for (int k = 0; k < 3; k++) cacc = cacc + s.cddr[k] * s.vb[3 + k];
      V3 a0 = mtmul(s.R0, cacc.l - cross(dif, cacc.a)) + cross(gyro, llin);
      acc0[0] = a0.x; acc0[1] = a0.y; acc0[2] = a0.z;
      float* __restrict__ Ho = &PG_REC(a.handover_w, ee, kHandover, HO_FRAME);      // MODE_STEP: the same values, env-major, for this step's observe launch
      auto put1 = [&](int row, float v) { PG_ROW(Fr, row, N, ee) = v; if (kStep) Ho[row] = v; };
      auto put3 = [&](int row, V3 v) { put1(row, v.x); put1(row + 1, v.y); put1(row + 2, v.z); };
      if (lead) {
        put3(PGTT_F_GYRO, gyro); put3(PGTT_F_GLOBAL_LINVEL, glin); put3(PGTT_F_GLOBAL_ANGVEL, w); put3(PGTT_F_LOCAL_LINVEL, llin);
        put3(PGTT_F_UPVECTOR, v3(s.R0.m[2], s.R0.m[5], s.R0.m[8]));
        put3(PGTT_F_GRAVITY, v3(-s.R0.m[6], -s.R0.m[7], -s.R0.m[8]));
      }
      // own foot: sensor order FR,FL,RR,RL = leg ^ 1
      const int f = l ^ 1;
      bool touching = s.con0.dist < 0.f;
      if (HAS_TERRAIN) {
#pragma unroll
        for (int k = 0; k < kMaxB; k++) touching |= (k < s.nbox) & (slots.at(k, 0) < 0.f);
      }
      // box-contact slot numbering of the debug record: own contacts follow those of the lower legs
      const int n0 = quad_bcast<0>(s.nbox), n1 = quad_bcast<1>(s.nbox), n2 = quad_bcast<2>(s.nbox), n3 = quad_bcast<3>(s.nbox);
      const int off = l == 0 ? 0 : (l == 1 ? n0 : (l == 2 ? n0 + n1 : n0 + n1 + n2)), total = n0 + n1 + n2 + n3;
      if (valid) {
        put3(PGTT_F_FEET_POS + 3 * f, mtmul(s.R0, s.sitef - s.imu));
        S6 cv = s.cvell[2];
        put3(PGTT_F_FEET_VEL + 3 * f, cv.l - cross(s.sitef - s.com, cv.a));
        put1(PGTT_F_CONTACT + f, touching ? 1.0f : 0.0f);
        put1(PGTT_F_FOOT_SITE_Z + f, s.sitef.z);
#pragma unroll
        for (int k = 0; k < 3; k++) put1(PGTT_F_ACT_FORCE + 3 * f + k, s.act_force[k]);
        if (a.buf.dbg_contact && a.buf.dbg_dist) {
          int* dc = a.buf.dbg_contact + (long)ee * 16; float* dd = a.buf.dbg_dist + (long)ee * 8;
          dc[2 * l] = l; dc[2 * l + 1] = -1; dd[l] = s.con0.dist;
          if (HAS_TERRAIN) {
#pragma unroll
            for (int k = 0; k < kMaxB; k++) if (k < s.nbox && off + k < 4) {
              dc[2 * (4 + off + k)] = l; dc[2 * (4 + off + k) + 1] = __float_as_int(slots.at(k, 20)); dd[4 + off + k] = slots.at(k, 0); }
          }
#pragma unroll
          for (int k = 0; k < 4; k++) if (k >= total) { dc[2 * (4 + k)] = -1; dc[2 * (4 + k) + 1] = -2; dd[4 + k] = 1.0f; }
        }
      }
    }
    sol.solve();
    const int pen_ovf = last ? quad_sum_i(sub_sum_i(s.pen_overflow ? 1 : 0)) : 0;      // over the lanes of the env, all lanes active
    if (last && lead) {
      float* __restrict__ Fr = a.buf.frame;
      int ee = e; asm volatile("" : "+v"(ee));
      float accA[3][6];
      const V3 dif = s.imu - s.com;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        V3 ct = mtmul(s.R0, v3(k == 0, k == 1, k == 2));
        V3 cr = mtmul(s.R0, s.cdr[k].l - cross(dif, s.cdr[k].a));
        accA[0][k] = ct.x; accA[1][k] = ct.y; accA[2][k] = ct.z;
        accA[0][3 + k] = cr.x; accA[1][3 + k] = cr.y; accA[2][3 + k] = cr.z;
      }
#pragma unroll
      for (int r = 0; r < 3; r++) {
        float v = acc0[r];
#pragma unroll
        for (int k = 0; k < 6; k++) v += accA[r][k] * s.qacc_b[k];
        PG_ROW(Fr, PGTT_F_ACCEL + r, N, ee) = v;
        if (kStep) PG_REC(a.handover_w, ee, kHandover, HO_FRAME + PGTT_F_ACCEL + r) = v;
      }
      if (a.buf.dbg_niter) a.buf.dbg_niter[ee] = s.niter_max | (pen_ovf > 0 ? PGTT_DBG_PEN_OVERFLOW : 0);
    }
    if (kStep) {
      // ---- semi-implicit Euler (eulerdamp disabled)
#pragma unroll
      for (int i = 0; i < 6; i++) s.vb[i] = s.vb[i] + s.qacc_b[i] * dt;
#pragma unroll
      for (int k = 0; k < 3; k++) s.vl[k] = s.vl[k] + s.qacc_l[k] * dt;
#pragma unroll
      for (int i = 0; i < 3; i++) s.qb[i] = s.qb[i] + dt * s.vb[i];
      V3 wv = v3(s.vb[3], s.vb[4], s.vb[5]);
      float nn = normalize3(wv);
      float sn, cs; sincosf(0.5f * (dt * nn), &sn, &cs);
      Q4 q2 = qmul(Q4{s.qb[3], s.qb[4], s.qb[5], s.qb[6]}, Q4{cs, wv.x * sn, wv.y * sn, wv.z * sn});
      normalize4(q2);
      s.qb[3] = q2.w; s.qb[4] = q2.x; s.qb[5] = q2.y; s.qb[6] = q2.z;
#pragma unroll
      for (int k = 0; k < 3; k++) s.ql[k] = s.ql[k] + dt * s.vl[k];
    }
  }
  if (!valid) return;
  // The compiler would otherwise keep the ~50 row addresses formed for the loads at the top alive (spilled to scratch)
  // until these stores: an opaque copy of the env index makes it re-form them here (one mad each).
  asm volatile("" : "+v"(e));
#if PG_ADDR32
  int lq = l; asm volatile("" : "+v"(lq));      // ... and of the leg index: the per-leg row offsets (3 l + k) N + e are formed again as well
#else
  const int lq = l;
#endif
  if (kStep || a.write_qpos) {
#pragma unroll
    for (int i = 0; i < 7; i++) PG_ROW(S, PGTT_S_QPOS + i, N, e) = s.qb[i];
#pragma unroll
    for (int k = 0; k < 3; k++) PG_ROW(S, PGTT_S_QPOS + 7 + 3 * lq + k, N, e) = s.ql[k];
  }
  if (kStep) {
#pragma unroll
    for (int i = 0; i < 6; i++) PG_ROW(S, PGTT_S_QVEL + i, N, e) = s.vb[i];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      PG_ROW(S, PGTT_S_QVEL + 6 + 3 * lq + k, N, e) = s.vl[k];
      PG_ROW(S, PGTT_S_MOTOR_TARGETS + 3 * (lq ^ 1) + k, N, e) = s.ctrl[k];
    }
    float* __restrict__ Ho = &PG_REC(a.handover_w, e, kHandover, 0);
#pragma unroll
    for (int i = 0; i < 7; i++) Ho[HO_QPOS + i] = s.qb[i];
#pragma unroll
    for (int i = 0; i < 6; i++) Ho[HO_QVEL + i] = s.vb[i];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      Ho[HO_QPOS + 7 + 3 * lq + k] = s.ql[k]; Ho[HO_QVEL + 6 + 3 * lq + k] = s.vl[k]; Ho[HO_MOTOR + 3 * (lq ^ 1) + k] = s.ctrl[k];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) PG_ROW(S, PGTT_S_QWARM + i, N, e) = s.wb[i];
#pragma unroll
  for (int k = 0; k < 3; k++) PG_ROW(S, PGTT_S_QWARM + 6 + 3 * lq + k, N, e) = s.wl[k];
}

}  // namespace pgtt

#define PG_CAT_(a, s, b, c, d) a##s##_##b##_##c##_##d
#define PG_CAT(a, s, b, c, d) PG_CAT_(a, s, b, c, d)

void PG_CAT(pgtt_launch_physics_s, PG_SUBS, PG_MODE, PG_DR, PG_TERRAIN)(int nblocks, hipStream_t st, const pgtt::KArgs& a, const float* action) {
  hipLaunchKernelGGL((pgtt::physics_kernel<PG_MODE, (PG_DR != 0), (PG_TERRAIN != 0), PG_SUBS>), dim3(nblocks), dim3(64), 0, st, a, action);
}
