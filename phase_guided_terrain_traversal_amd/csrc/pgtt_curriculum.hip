// pgtt_curriculum.hip — the terrain curriculum's kernels (pgtt_curriculum; include/pgtt.h).  A translation unit of its own: the step kernels
// and the file they live in stay as they are.  Host launchers at the end; pgtt_api.hip holds the entry point and the masked reset that follows.
#include "pgtt_common.hip.h"

namespace pgtt {

// rows of the library-owned record that keeps a finished env's step outputs across its restart (the reset's observe pass clears them)
enum { CUR_SAVE_REWARD = PGTT_NMETRIC, CUR_SAVE_DONE = PGTT_NMETRIC + 1, CUR_NSAVE = PGTT_NMETRIC + 2 };

// episode mean of the unscaled tracking_lin_vel term.  The metric rows hold term * scale (no dt) and the length row counts the steps the sums
// hold.  Not contracted, correctly rounded division (csrc/Makefile compiles this file without the 1-ulp switch in every build): curriculum.replay
// computes the same bits in numpy fp32.
PG_INL float cur_tracking(float sum, float len, float scale) {
#pragma clang fp contract(off)
  const float den = len * scale;
  return (len > 0.f && scale != 0.f) ? sum / den : 0.f;
}
PG_INL int cur_pick(float u, int T) {
#pragma clang fp contract(off)
  const int k = (int)(u * (float)T);
  return k < T - 1 ? k : T - 1;
}

// one env per thread, in the plain form of push_kernel.  Caller-visible writes: level, variant, stats.  The settings travel by value
// (PgttCurriculum, 96 bytes).  Library-owned: the reset mask (a byte for EVERY env) and the step-output record of the finished ones.
__global__ __launch_bounds__(64) void curriculum_kernel(KArgs a, PgttCurriculum c, unsigned char* __restrict__ mask, float* __restrict__ save) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  const int N = a.N;
  const PgttConfig* __restrict__ cfg = a.cfg;
  const int L = c.levels;
  const bool fin = e < N && a.buf.done[e] != 0.f;
  int lvl = -1;
  bool up = false, down = false;
  if (fin) {
    lvl = min(max(c.level[e], 0), L - 1);
    const int steps = a.buf.istate[PGTT_I_EP_STEPS * (long)N + e];
    const bool truncated = steps >= cfg->episode_length;              // the wrapper's own test (observe_kernel)
    const float trk = cur_tracking(a.buf.ep_metrics[PGTT_R_TRACKING_LIN_VEL * (long)N + e], a.buf.ep_metrics[(PGTT_NMETRIC + 1) * (long)N + e],
                                   cfg->reward_scale[PGTT_R_TRACKING_LIN_VEL]);
    up = truncated && trk >= c.promote_tracking;
    down = !truncated && (float)steps < c.demote_length * (float)cfg->episode_length;
    const int nl = up ? min(lvl + 1, L - 1) : (down ? max(lvl - 1, 0) : lvl);
    up = nl > lvl; down = nl < lvl;                                   // the totals count moves, not clamped attempts
    const int v0 = c.level_start[nl], Tl = c.level_start[nl + 1] - v0;
    const unsigned id = (unsigned)(a.env_off + e);
    const unsigned ep = (unsigned)a.buf.istate[PGTT_I_RNG_CTR * (long)N + e];     // as the step left it
    const float u = rng_uniform(a.seed, id, ep, PGTT_RS_CURRICULUM, 0, a.rng_fix);
    c.level[e] = nl;
    a.buf.variant[e] = v0 + cur_pick(u, Tl);
#pragma unroll
    for (int k = 0; k < PGTT_NMETRIC; k++) save[k * (long)N + e] = a.buf.metrics[k * (long)N + e];
    save[CUR_SAVE_REWARD * (long)N + e] = a.buf.reward[e];
    save[CUR_SAVE_DONE * (long)N + e] = a.buf.done[e];
  }
  if (e < N) mask[e] = fin ? 1 : 0;
  int* __restrict__ stats = c.stats;
  if (stats) {
    // per-wave counts by ballot, then one integer atomic per wave and non-zero counter: the sums do not depend on the order of the adds
    const bool lead = (threadIdx.x & 63) == 0;
    const int nfin = __popcll(__ballot(fin));
    if (nfin == 0) return;                                            // wave-uniform
    for (int k = 0; k < L; k++) {
      const int cnt = __popcll(__ballot(fin && lvl == k));
      if (cnt != 0 && lead) atomicAdd(stats + k, cnt);
    }
    const int cu = __popcll(__ballot(up)), cd = __popcll(__ballot(down));
    if (lead) {
      if (cu != 0) atomicAdd(stats + PGTT_CS_PROMOTED, cu);
      if (cd != 0) atomicAdd(stats + PGTT_CS_DEMOTED, cd);
      atomicAdd(stats + PGTT_CS_FINISHED, nfin);
    }
  }
}

// after the masked reset: reward, done and metrics of the finished envs as the step wrote them
__global__ __launch_bounds__(64) void curriculum_restore_kernel(KArgs a, const unsigned char* __restrict__ mask, const float* __restrict__ save) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  const int N = a.N;
  if (e >= N || !mask[e]) return;
#pragma unroll
  for (int k = 0; k < PGTT_NMETRIC; k++) a.buf.metrics[k * (long)N + e] = save[k * (long)N + e];
  a.buf.reward[e] = save[CUR_SAVE_REWARD * (long)N + e];
  a.buf.done[e] = save[CUR_SAVE_DONE * (long)N + e];
}

// number of envs whose level is outside [0, L) or whose variant is outside its level's range (pgtt_reset's one-off check of the caller's labels)
__global__ __launch_bounds__(64) void curriculum_check_kernel(KArgs a, PgttCurriculum c, int* __restrict__ bad) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  bool out = false;
  if (e < a.N) {
    const int l = c.level[e], v = a.buf.variant[e];
    out = l < 0 || l >= c.levels;
    if (!out) out = v < c.level_start[l] || v >= c.level_start[l + 1];
  }
  const unsigned long long b = __ballot(out);
  if (b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(bad, __popcll(b));
}

}  // namespace pgtt

int pgtt_curriculum_save_rows() { return pgtt::CUR_NSAVE; }
void pgtt_launch_curriculum(hipStream_t st, const pgtt::KArgs& a, const PgttCurriculum& c, unsigned char* mask, float* save) {
  hipLaunchKernelGGL(pgtt::curriculum_kernel, dim3((a.N + 63) / 64), dim3(64), 0, st, a, c, mask, save);
}
void pgtt_launch_curriculum_restore(hipStream_t st, const pgtt::KArgs& a, const unsigned char* mask, const float* save) {
  hipLaunchKernelGGL(pgtt::curriculum_restore_kernel, dim3((a.N + 63) / 64), dim3(64), 0, st, a, mask, save);
}
void pgtt_launch_curriculum_check(hipStream_t st, const pgtt::KArgs& a, const PgttCurriculum& c, int* bad) {
  hipLaunchKernelGGL(pgtt::curriculum_check_kernel, dim3((a.N + 63) / 64), dim3(64), 0, st, a, c, bad);
}
