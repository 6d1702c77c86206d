/*
 * pgtt_learn.h - libpgtt_learn.so: the pieces of one PPO minibatch update that pgtt_train.h does not have, so that the whole update of
 * phase_guided_terrain_traversal_amd/learn.py::NativeLearner is hand-written HIP (gfx950) on ONE stream: the minibatch gather with the
 * observation and advantage normalisation, the Linear layers forward (bias, SiLU) and their data gradient on fp32 MFMA, the value loss,
 * the global-norm clip with Adam over one flat parameter buffer, and generalised advantage estimation; and, for the policy distillation of
 * distill.py, which composes the same pieces, the imitation loss between two policy heads and a gather of (observation, label) rows.  The policy loss and the weight /
 * bias gradients stay pgtt_ppo_policy_loss / pgtt_ppo_linear_backward of libpgtt.so (pgtt_train.h).  Like pgtt_train.h these replace no
 * entry point of the reference (its PPO is Brax's, configured at training/train.py:135-161); the arithmetic they restate is that of
 * phase_guided_terrain_traversal_amd/ppo.py, held to the fp64 statement in tests/ppo_reference.py.
 *
 * Conventions as in pgtt_train.h: plain C, device pointers (float32 unless said otherwise), every kernel enqueued on the caller's stream,
 * nothing synchronises and nothing allocates (every call can be captured in a HIP graph), 0 or a negative PGTT_E_* code with the message
 * in pgtt_learn_last_error().  Every entry refuses a NULL pointer (where NULL is not named as allowed) or a non-positive size with
 * PGTT_E_ARG and writes nothing.  Weights are torch's [out][in] layout as they are; nothing is packed.  Sums have a fixed order: two calls
 * on equal inputs give equal bits.
 */
#ifndef PGTT_LEARN_H_
#define PGTT_LEARN_H_
#include "pgtt.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One minibatch out of the flat [rows] batch: for i < B, r = idx[i] (clamped into [0, rows): an index outside reads no foreign memory),
 *   x_s[i][:] = (obs[r][:] - mean_s) / std_s,   x_p[i][:] = (priv[r][:] - mean_p) / std_p   (one subtraction, one correctly rounded division),
 *   u_out[i][:] = u[r][:],  logp_out[i] = logp[r],  ret_out[i] = ret[r]   (copies, equal bits),
 *   adv_out[i] = (a_i - mean a) / (sqrt(mean (a - mean a)^2) + 1e-8),  a_i = adv[r]   (population standard deviation, two passes).
 * Two launches: one workgroup per row, then a single workgroup that forms the two sums over B in a fixed order and normalises adv_out in place. */
typedef struct PgttLearnGatherArgs {
  const int64_t* idx;          /* [B] rows of the batch */
  const float* obs;            /* [rows][obs_dim] */
  const float* priv;           /* [rows][priv_dim] */
  const float* u;              /* [rows][act_dim] */
  const float* logp;           /* [rows] */
  const float* adv;            /* [rows] raw advantages */
  const float* ret;            /* [rows] value targets */
  const float* mean_s;         /* [obs_dim] */
  const float* std_s;          /* [obs_dim] */
  const float* mean_p;         /* [priv_dim] */
  const float* std_p;          /* [priv_dim] */
  float* x_s;                  /* [B][obs_dim] */
  float* x_p;                  /* [B][priv_dim] */
  float* u_out;                /* [B][act_dim] */
  float* logp_out;             /* [B] */
  float* adv_out;              /* [B] normalised */
  float* ret_out;              /* [B] */
  int32_t B, rows, obs_dim, priv_dim, act_dim;
} PgttLearnGatherArgs;
int pgtt_learn_gather(const PgttLearnGatherArgs* args, void* stream);

/* Z = X W^T + b,  Y = act ? silu(Z) : Z   with X [K][M], W [N][M], b [N], Y and Z [K][N]; silu(z) = z / (1 + expf(-z)).
 * fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 sums), the contraction runs over m in ascending blocks of 16.  Any K, M, N >= 1:
 * the tails are masked in the kernel.  z_KxN receives the pre-activation for the backward pass; NULL is allowed when act == 0 (refused when act != 0).
 * One launch. */
int pgtt_learn_linear_forward(const float* x_KxM, const float* w_NxM, const float* b_N, int K, int M, int N, int act,
                              float* y_KxN, float* z_KxN, void* stream);

/* dX = (dY W) * silu'(Zprev)  with dY [K][N], W [N][M], Zprev and dX [K][M]; Zprev is the pre-activation that produced this layer's input,
 * NULL = no factor.  silu'(z) = s (1 + z (1 - s)), s = 1 / (1 + exp(-z)), is evaluated in fp64 and rounded once: it has a root at z = -1.278
 * where an fp32 evaluation loses every digit to cancellation.  fp32 MFMA as above, any K, M, N >= 1.  One launch. */
int pgtt_learn_linear_backward_data(const float* dy_KxN, const float* w_NxM, const float* zprev_KxM, int K, int M, int N,
                                    float* dx_KxM, void* stream);

/* loss_1[0] = 0.25 mean((ret - v)^2),  dv[i] = 0.5 (v[i] - ret[i]) / B: one launch of a single workgroup, fixed order. */
int pgtt_learn_value_loss(const float* v_B, const float* ret_B, int B, float* loss_1, float* dv_B, void* stream);

/* Global-norm clip and Adam over ONE flat buffer of P floats, two launches:
 *   1. g <- grad_scale g (when grad_scale != 1), per-workgroup partial sums of g^2 into `partial`, *t <- *t + 1;
 *   2. every workgroup adds the partials in the same fixed order: norm = sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)), then with c = coef g
 *      m <- beta1 m + (1 - beta1) c,  v <- beta2 v + (1 - beta2) c^2,  p <- p - lr (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps);
 *      the two bias corrections are formed in fp64 from the fp64 betas and rounded once.  *norm_1 receives the UNCLIPPED norm (of grad_scale g).
 * g keeps grad_scale g (not coef g).  partial holds pgtt_learn_adam_partials(P) floats of scratch (at most 1024). */
typedef struct PgttLearnAdamArgs {
  float* p;                    /* [P] parameters */
  float* g;                    /* [P] gradients */
  float* m;                    /* [P] first moments */
  float* v;                    /* [P] second moments */
  int64_t* t;                  /* device int64[1]: the step counter, advanced by one per call */
  float* partial;              /* [pgtt_learn_adam_partials(P)] scratch */
  float* norm_1;               /* device float[1]: the unclipped gradient norm */
  int64_t P;
  double lr, beta1, beta2, eps;
  float max_norm, grad_scale;
} PgttLearnAdamArgs;
int pgtt_learn_clip_adam(const PgttLearnAdamArgs* args, void* stream);
int pgtt_learn_adam_partials(int64_t P);

/* Generalised advantage estimation as Brax's compute_gae (phase_guided_terrain_traversal_amd/ppo.py::compute_gae), rows [T][N], boot [N]:
 *   term = done (1 - trunc);  delta_t = (r_t + gamma (1 - term_t) V_{t+1} - V_t)(1 - trunc_t),  V_T = boot;
 *   acc_t = delta_t + gamma lambda (1 - term_t)(1 - trunc_t) acc_{t+1},  acc_T = 0;   vs_t = acc_t + V_t;
 *   adv_t = (r_t + gamma (1 - term_t) vs_{t+1} - V_t)(1 - trunc_t),  vs_T = boot.
 * One lane per env, one backward loop over T, one launch. */
int pgtt_learn_gae(const float* trunc_TxN, const float* done_TxN, const float* rew_TxN, const float* val_TxN, const float* boot_N,
                   int T, int N, float lambda, float gamma, float* adv_TxN, float* vs_TxN, void* stream);

/* Policy distillation (phase_guided_terrain_traversal_amd/distill.py): the imitation loss between two heads and its gradient, held to the fp64
 * statement in tests/distill_reference.py.  Both heads are in the trainer's layout (loc | raw), [B][2A], sigma = softplus(raw) + 1e-3 with
 * softplus(r) = max(r, 0) + log1p(exp(-|r|)) (finite for every finite r).  Per row i and dimension a, with d = loc_t - loc_s and
 * q = (sigma_t^2 + d^2) / sigma_s^2:
 *   KL = log(sigma_s / sigma_t) + 0.5 (q - 1)            KL(teacher || student) of the two diagonal Gaussians of the pre-tanh variable,
 *   dL/dloc_s = -d / sigma_s^2 / B,   dL/draw_s = (1 - q) / sigma_s * sigmoid(raw_s) / B,
 *   loss_2[0] = (1 / B) sum_i sum_a KL,   loss_2[1] = (1 / (B A)) sum_i sum_a (tanh loc_s - tanh loc_t)^2   (the error of the deterministic action:
 *   logged, no gradient),   grad = d loss_2[0] / d student head, [B][2A] in the layout of the head.
 * Every division is correctly rounded and 1 - q is formed before the division by sigma_s: a student head that has the teacher's bits gives
 * loss_2 = (0, 0) and an all-zero gradient exactly.  Two launches: one lane per row in workgroups of 64, the two sums of a workgroup added in lane
 * order into partial[2 block], partial[2 block + 1]; then one wave adds the partials in block order.  partial holds 2 ceil(B / 64) floats (the layout of
 * pgtt_ppo_policy_loss).  Any A >= 1. */
int pgtt_learn_distill_loss(const float* student_Bx2A, const float* teacher_Bx2A, int B, int A, float* partial_2xceilB64, float* loss_2,
                            float* grad_Bx2A, void* stream);

/* One minibatch of (observation, label) pairs out of [rows]: for i < B, r = idx[i] (clamped into [0, rows): an index outside reads no foreign memory),
 *   x[i][:] = (obs[r][:] - mean) / std   (one subtraction, one correctly rounded division: the bits of x_s above),
 *   y[i][:] = target[r][:]               (a copy, equal bits; tgt_dim wide).
 * One launch, one workgroup per row. */
int pgtt_learn_gather_rows(const int64_t* idx_B, const float* obs, const float* target, const float* mean, const float* std,
                           int B, int rows, int obs_dim, int tgt_dim, float* x, float* y, void* stream);

/* The recurrent policy (phase_guided_terrain_traversal_amd/recurrent_policy.py): the policy MLP with a GRU memory of R values per env
 * between its last hidden layer and its head, held to the fp64 statement in tests/recurrent_policy_reference.py.  R = `memory` is a multiple of 16 in
 * [16, PGTT_LEARN_MAX_MEMORY]; every entry below refuses another R with PGTT_E_ARG.  Per env e, all in fp32:
 *   x  = (obs - mean) / std                                  one subtraction, one correctly rounded division
 *   h1 = silu(W0 x + b0) (h1 values);  h2 = silu(W1 h1 + b1) (h2);  h3 = silu(W2 h2 + b2) (h3)       as pgtt_learn_linear_forward states them
 *   m0 = cleared(e) ? 0 : mem[e]                             cleared(e): clear_all != 0, or clear_mask[e] != 0, or use_done != 0 and done[e] != 0
 *   gi = W_ih h3 + b_ih  (3R values: r | u | n)              torch.nn.GRUCell's weight_ih [3R][h3] and bias_ih, gate order r, z, n (z is called u here)
 *   gh = W_hh m0 + b_hh  (3R values)                         weight_hh [3R][R], bias_hh
 *   r  = sigmoid(gi_r + gh_r);  u = sigmoid(gi_u + gh_u);  n = tanh(gi_n + r * gh_n)
 *   m1 = (1 - u) * n + u * m0;   mem[e] = m1
 *   head = W3 h3 + b3 + W_m m1   (24 values: loc | raw, W_m [24][R] has no bias);   action = tanh(loc)   (12 values)
 * sigmoid(v) = 1 / (1 + t) for v >= 0 and t / (1 + t) for v < 0 with t = exp(-|v|);  tanh(v) = sign(v) (1 - t) / (1 + t) with t = exp(-2 |v|): no
 * overflow at any v, +-100 included (the forms of pgtt_perceive.h).  u = 1 keeps m0: (1 - 1) * n + 1 * m0.  With done == NULL, use_done clears
 * nothing; with clear_mask == NULL the mask clears nothing.  A cleared env never reads mem[e]: it may hold anything, NaN included.  The use_done and
 * auto-reset semantics are those of pgtt_perceive.h: the acting step runs before the env's step, so it sees the `done` of the step before, and with
 * auto-reset the observation is then already the new episode's first.
 *
 * The acting step.  Five launches: a normalising copy (one workgroup per env; it also writes the store_obs row), three launches of the
 * linear-forward kernel (the trunk, into `work`), and ONE launch for everything from h3 on - one workgroup of four waves per 16 envs: the two gate
 * products on fp32 MFMA (v_mfma_f32_16x16x4_f32), the gates lane-local in the accumulators' layout, m1, the head product over h3 and m1, the tanh,
 * the clear and the stores.  Sums, per output element, each ONE chain of fp32 MFMA accumulation that starts at zero: a part over K values runs in
 * blocks of 16 k ascending, inside a block k = 16 kb + 4 g + s with s the outer and g the inner index (s, g in 0..3).
 *   gi_r + gh_r: first the h3 products of W_ih's row with h3, then the R products of W_hh's row with m0, then + b_ih, then + b_hh;  gi_u + gh_u likewise;
 *   gi_n: the h3 products, then + b_ih;   gh_n: the R products, then + b_hh;
 *   head: first the h3 products of W3's row with h3, then the R products of W_m's row with m1, then + b3.
 * An env's action, head, mem and stored rows are functions of its own observation, memory and clear flags only: the same bits in any batch, at any
 * position.  With store pointers given, row t (0 <= t < store_rows, PGTT_E_ARG otherwise) receives: store_obs[t][e][:] = obs[e][:] (what the policy
 * saw, the same bits), store_mem0[t][e][:] = m0 (the memory the step started from, after clearing), store_clear[t][e] = cleared(e) as 0 / 1.
 * h3 must be a multiple of 16.  `work` holds pgtt_learn_recurrent_act_work_floats(num_envs, obs_dim, h1, h2, h3) floats of scratch; after the call it
 * holds, in this order, x [N][obs_dim], h1 [N][h1], h2 [N][h2], h3 [N][h3] and N max(h1, h2, h3) floats of pre-activations. */
#define PGTT_LEARN_MAX_MEMORY 256
typedef struct PgttLearnRecurrentActArgs {
  const float* obs;            /* [N][obs_dim] */
  const float* mean;           /* [obs_dim] */
  const float* std;            /* [obs_dim] */
  const float* w0;             /* [h1][obs_dim] */
  const float* w1;             /* [h2][h1] */
  const float* w2;             /* [h3][h2] */
  const float* w3;             /* [24][h3] */
  const float* b0;             /* [h1] */
  const float* b1;             /* [h2] */
  const float* b2;             /* [h3] */
  const float* b3;             /* [24] */
  const float* w_ih;           /* [3R][h3] */
  const float* w_hh;           /* [3R][R] */
  const float* b_ih;           /* [3R] */
  const float* b_hh;           /* [3R] */
  const float* w_m;            /* [24][R] */
  const float* done;           /* [N] 0 / 1 (PgttBuffers.done) or NULL */
  const uint8_t* clear_mask;   /* [N] or NULL */
  float* mem;                  /* [N][R], read and written */
  float* action;               /* [N][12] */
  float* head;                 /* [N][24] or NULL */
  float* store_obs;            /* [store_rows][N][obs_dim] or NULL */
  float* store_mem0;           /* [store_rows][N][R] or NULL */
  uint8_t* store_clear;        /* [store_rows][N] or NULL */
  float* work;                 /* scratch, see above */
  int32_t num_envs, obs_dim, h1, h2, h3, memory, t, store_rows, clear_all, use_done;
} PgttLearnRecurrentActArgs;
int pgtt_learn_recurrent_act(const PgttLearnRecurrentActArgs* args, void* stream);
int64_t pgtt_learn_recurrent_act_work_floats(int num_envs, int obs_dim, int h1, int h2, int h3);

/* The sampled acting step: the step above with the tanh-normal head of pgtt_policy_act (pgtt_train.h) behind it, still five launches - the sampling is
 * the end of the fifth.  head, mem, store_obs, store_mem0 and store_clear are those of pgtt_learn_recurrent_act, bit for bit: the sample does not feed
 * the memory.  Per env e and actuator j < 12, with loc = head[j], raw = head[12 + j], all in fp32 and in exactly the forms of policy_act_kernel:
 *   sc   = softplus_t(raw) + 1e-3f                        softplus_t(x) = x > 20 ? x : log1pf(expf(x))   (torch's threshold 20)
 *   eps  = eps[e][j] when eps is given, else the in-kernel draw of pgtt_train.h: actuators 2k and 2k + 1 share ONE Philox4x32-10 block, key
 *          (seed & 0xffffffff, seed >> 32), counter ((uint32)(env_id_offset + e), draw & 0xffffffff, (draw >> 32) ^ 0x50475454, k) with
 *          draw = counters[1] (0 when counters == NULL; counters[0] is not read: the storage row is act.t), words w0 .. w3 (w2, w3 unused);
 *          u1 = ((float)(w0 >> 8) + 0.5f) 2^-24,  u2 = (float)(w1 >> 8) 2^-24,  r = sqrtf(-2 logf(u1)),  theta = 6.28318530717958648f * u2,
 *          eps = r cosf(theta) for even j, r sinf(theta) for odd j
 *   u    = deterministic ? loc : loc + sc * eps           the pre-tanh sample
 *   z    = (u - loc) / sc
 *   lp_j = -0.5f z z - logf(sc) - 0.91893853320467274f - 2.0f (0.69314718055994531f - u - softplus_t(-2.0f u))
 *   act.action[e][j] = tanh(u)                            the overflow-free form above: deterministic != 0 gives pgtt_learn_recurrent_act's action bits
 *   logp[e] = ((..(0 + lp_0) + lp_1) + ..) + lp_11        one lane per env adds the 12 terms out of LDS, j ascending from 0
 * With store pointers given, row act.t (0 <= t < store_rows, PGTT_E_ARG otherwise) receives store_u[t][e][:] = u and store_logp[t][e] = logp[e].
 * Rows past num_envs are neither drawn for nor stored.  An env's u, logp and action depend on its own row and on its global id env_id_offset + e only:
 * the same bits in any batch, at any position.  No atomics, no scratch; on top of the two memory tiles the kernel holds 2304 bytes of static LDS (the
 * [16][24] head values of its 16 envs and their [16][12] terms lp_j).  Refused with PGTT_E_ARG, nothing written: a NULL args, everything
 * pgtt_learn_recurrent_act refuses of `act`, and store_u or store_logp given with store_rows <= 0 or t outside [0, store_rows). */
typedef struct PgttLearnRecurrentSampleArgs {
  PgttLearnRecurrentActArgs act;  /* every field with the meaning it has above; act.action receives tanh(u) */
  const float* eps;               /* [N][12] standard-normal draws, or NULL: drawn in the kernel */
  const int64_t* counters;        /* device int64[2] or NULL: draw = counters[1] (0 when NULL); counters[0] is not read, the row is act.t */
  float* store_u;                 /* [store_rows][N][12] or NULL: the pre-tanh sample, row act.t */
  float* store_logp;              /* [store_rows][N] or NULL */
  uint64_t seed;
  int64_t env_id_offset;
  int32_t deterministic;          /* non-zero: u = loc */
} PgttLearnRecurrentSampleArgs;
int pgtt_learn_recurrent_act_sample(const PgttLearnRecurrentSampleArgs* args, void* stream);

/* The point-wise pieces of back-propagation through time over the same cell; the products around them are pgtt_learn_linear_forward (act = 0, a zero
 * bias where none exists), pgtt_learn_linear_backward_data and pgtt_ppo_linear_backward.  Rows [B][.], gates in the order r | u | n, clear flags uint8.
 *   clear_rows:    m0[i][:] = clear[i] ? 0 : m[i][:]          (a cleared row of m is not read).  One launch.
 *   cell_forward:  from gi [B][3R], gh [B][3R] (= W_hh m0 + b_hh) and m0 [B][R]: gates [B][3R] = (r | u | n) and m1 [B][R] as above; when m0_next is
 *                  given, m0_next[i][:] = clear_next[i] ? 0 : m1[i][:]  (clear_next == NULL: a copy), the next step's m0.  One launch.
 *   cell_backward: with dm1 = dm1_head + (dm0_next given and not clear_next[i] ? dm0_next : 0)  - dL/dm1 from the head and dL/dm0 of the step after,
 *                  which is zero where that step was cleared and absent at the last step (dm0_next == NULL) - and the SAVED gates (nothing is recomputed):
 *                    dn = dm1 (1 - u),  du = dm1 (m0 - n),  dpre_n = dn (1 - n^2),  dpre_u = du u (1 - u),  dr = gh_n dpre_n,  dpre_r = dr r (1 - r),
 *                    dgi = (dpre_r | dpre_u | dpre_n),   dgh = (dpre_r | dpre_u | r dpre_n),   dm0_direct = u dm1;
 *                  dL/dm0 of this step is dm0_direct + dgh W_hh (pgtt_learn_linear_backward_data, then pgtt_learn_add_rows).  One launch.
 *   add_rows:      out[i] = a[i] + b[i] over n floats; out may be a or b.  One launch.
 * One lane per (row, memory value); nothing is summed across lanes. */
int pgtt_learn_gru_clear_rows(const float* m_BxR, const uint8_t* clear_B, int B, int R, float* m0_BxR, void* stream);
int pgtt_learn_gru_cell_forward(const float* gi_Bx3R, const float* gh_Bx3R, const float* m0_BxR, const uint8_t* clear_next_B, int B, int R,
                                float* gates_Bx3R, float* m1_BxR, float* m0_next_BxR, void* stream);
int pgtt_learn_gru_cell_backward(const float* gates_Bx3R, const float* gh_Bx3R, const float* m0_BxR, const float* dm1_head_BxR,
                                 const float* dm0_next_BxR, const uint8_t* clear_next_B, int B, int R, float* dgi_Bx3R, float* dgh_Bx3R,
                                 float* dm0_direct_BxR, void* stream);
int pgtt_learn_add_rows(const float* a_n, const float* b_n, int64_t n, float* out_n, void* stream);

int pgtt_learn_sizeof_recurrent_act_args(void);
int pgtt_learn_sizeof_recurrent_sample_args(void);
int pgtt_learn_sizeof_gather_args(void);
int pgtt_learn_sizeof_adam_args(void);
const char* pgtt_learn_build_info(void);      /* "src=<srchash.side_sha256("learn")>;flavor=product" */
const char* pgtt_learn_last_error(void);
#ifdef __cplusplus
}
#endif
#endif /* PGTT_LEARN_H_ */
