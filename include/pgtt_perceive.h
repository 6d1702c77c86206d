/*
 * pgtt_perceive.h — C ABI of libpgtt_perceive.so: the student perception module.  A small conv net that estimates the 117 height-scan rows of
 * the observation from the onboard depth image (include/pgtt_depth.h) and proprioceptive rows of the observation, so that a policy trained on the
 * privileged scan can act on what a robot senses.  Forward only; training differentiates the same function in torch (perceive.ScanEstimator).
 *
 * A separate library from libpgtt.so, libpgtt_render.so and libpgtt_depth.so: it READS the caller's `depth` and `obs` and writes `latent`, `est`
 * and `obs_out`.
 *
 * Conventions (those of pgtt.h)
 *   - plain C; `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 or a negative PGTT_E_* code (pgtt.h); the message is available from pgtt_perceive_last_error().
 *   - device buffers are CALLER-OWNED; pgtt_perceive() enqueues two kernels on the caller's stream and neither allocates, synchronises nor
 *     reads anything back, so it can be captured in a HIP graph.  The library reads no environment variable.
 *
 * The function, per env e, all in fp32 and in THIS order:
 *   1. x[0][i][j] = (min(max(d, near), far) - near) / (far - near) - 0.5 with d = depth[e][i][j]; a NaN d reads as `far`.
 *   2. n_conv times: y[o][i][j] = silu(b[o] + sum_{c, di, dj} w[o][c][di][dj] * x[c][i * stride + di][j * stride + dj]),   silu(v) = v / (1 + exp(-v))
 *      no padding, no dilation: H_out = (H_in - kernel) / stride + 1 (integer division), W_out likewise.
 *   3. latent[e][(o * H_out + i) * W_out + j] = y[o][i][j] of the last conv: the flatten is in [C][H][W] order, F = C * H_out * W_out values.
 *   4. z = latent[e] followed by obs[e][prop_rows[0 .. n_prop - 1]]:  F + n_prop values.
 *   5. h = silu(W1 z + b1) (hidden values);  est[e] = W2 h + b2 (PGTT_NSCAN = 117 values, no activation).
 *   obs_out[e] (when bound) is obs[e] with rows [scan_row0, scan_row0 + 117) replaced by est[e]; every other row is copied bit for bit.
 * The sums run on fp32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered chain of fp32 fma, one rounding per product), in a fixed order per output element:
 *   conv: k = (c * kernel + di) * kernel + dj ascending;   linear: blocks of 16 k ascending, inside a block k = 16 kb + 4 g + s with s the outer and g the
 *   inner index (s, g in 0..3).  The bias is added after the sum.
 * An env's `latent`, `est` and `obs_out` rows are functions of its own depth image and observation only: the same bits in any batch, at any position.
 *
 * The recurrent form (PgttPerceiveMemory, pgtt_perceive_recurrent): a GRU cell between the hidden layer and the scan rows, with a memory of R values
 * per env, R a multiple of 16 in [16, PGTT_PERCEIVE_MAX_MEMORY].  Steps 1 - 4 and h = silu(W1 z + b1) are the ones above; then, all in fp32:
 *   m0   = cleared(e) ? 0 : mem[e]                     cleared(e): clear_all != 0, or clear_mask[e] != 0, or use_done != 0 and done[e] != 0
 *   gi   = W_ih h + b_ih     (3R values: r | u | n)    torch.nn.GRUCell's weight_ih [3R][hidden] and bias_ih, gate order r, z, n (z is called u here)
 *   gh   = W_hh m0 + b_hh    (3R values)               weight_hh [3R][R], bias_hh
 *   r    = sigmoid(gi_r + gh_r);  u = sigmoid(gi_u + gh_u);  n = tanh(gi_n + r * gh_n)
 *   m1   = (1 - u) * n + u * m0;   mem[e] = m1
 *   est[e] = W_out m1 + b_out  (117 values, no activation);  obs_out as above.
 * With done == NULL, use_done clears nothing.  A cleared env never reads mem[e]: it may hold anything, NaN included.
 * Sums, per output element: gi_r + gh_r is ONE chain, first the `hidden` products of W_ih's row with h, then the R products of W_hh's row with m0,
 * each part in the linear order above (blocks of 16 k ascending, k = 16 kb + 4 g + s, s outer, g inner), then + b_ih, then + b_hh; gi_u + gh_u
 * likewise.  gi_n and gh_n are a chain each, over `hidden` and over R products, the bias (b_ih, b_hh) added after the sum.  est is one chain over
 * the R products, then + b_out.  sigmoid(v) = 1 / (1 + t) for v >= 0 and t / (1 + t) for v < 0 with t = exp(-|v|);  tanh(v) = sign(v) (1 - t) / (1 + t)
 * with t = exp(-2 |v|): no overflow at any v, +-100 included.  u = 1 keeps m0: (1 - 1) * n + 1 * m0.
 * An env's `latent`, `mem`, `est` and `obs_out` rows are functions of its own depth image, observation, memory and clear flags only: the same bits
 * in any batch, at any position.
 * use_done and auto-reset.  With PgttConfig.autoreset = 1 the step that finishes an episode leaves done[e] = 1 AND has already restored the env's
 * first state, and the camera has rendered it, so a call with use_done after the step starts the new episode from m0 = 0 on the new episode's
 * first image.  With autoreset = 0 done[e] stays as the step's termination test gives it: use_done then restarts the memory at every call while
 * done[e] != 0, until the caller resets the env (pgtt_reset with a mask) and passes the same mask as clear_mask.
 *
 * Packed layouts (perceive.ScanEstimator.pack() produces them; zero wherever an index is past the matrix):
 *   conv layer, weight [O][C][k][k] read as the matrix W[O][K], K = C k k, Kp = K rounded up to a multiple of 4:
 *       packed[((mt * (Kp / 4) + ks) * 64 + 16 g + i)] = W[16 mt + i][4 ks + g]         O / 16 * Kp * 16 floats;  bias: [O]
 *   linear layer, weight [out][in], out_p / in_p rounded up to multiples of 16 (pgtt_train.h's order):
 *       packed[(((t * (in_p / 16) + kb) * 64 + 16 g + i) * 4 + s] = W[16 t + i][16 kb + 4 g + s]     out_p * in_p floats;  bias: [out_p]
 *
 * LDS budget.  One workgroup per env keeps the preprocessed image and every conv output but the last in LDS, alternating between two buffers.  With
 * a_0 = H * W and a_l = out_ch[l] * H_l * W_l floats for l = 1 .. n_conv - 1 (the last conv's output goes to `latent`, not to LDS), a config is accepted when
 *       4 * (max(a_0, a_2) + a_1) <= PGTT_PERCEIVE_LDS_BYTES         (a_l = 0 for a layer that is not there)
 * The default net (48 x 64 -> 16 ch k5 s2 -> 32 ch k3 s2 -> 32 ch k3 s2) has a = 3072, 10560, 4480: 4 * (4480 + 10560) = 60160 bytes.
 */
#ifndef PGTT_PERCEIVE_H_
#define PGTT_PERCEIVE_H_

#include <stdint.h>

#include "pgtt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGTT_PERCEIVE_MAX_CONV 3
#define PGTT_PERCEIVE_MAX_CH 64
#define PGTT_PERCEIVE_MAX_PROP 64
#define PGTT_PERCEIVE_MAX_HIDDEN 512
#define PGTT_PERCEIVE_MAX_DIM 256         /* width and height (pgtt_depth.h's limit) */
#define PGTT_PERCEIVE_LDS_BYTES 61440     /* activations of one env, see above: 60 KB, which leaves room for the kernel's offset table in 64 KB */
#define PGTT_PERCEIVE_NLAYER 5            /* packed layers: 0..2 the convs, 3 Linear(F + n_prop -> hidden), 4 Linear(hidden -> 117) */
#define PGTT_PERCEIVE_MAX_MEMORY 256       /* R of the recurrent form: a multiple of 16 in [16, 256] */

typedef struct PgttPerceiveConfig {
  int32_t height, width;                  /* the depth image, 1 .. PGTT_PERCEIVE_MAX_DIM each */
  float near, far;                        /* near < far, finite */
  int32_t n_conv;                         /* 1 .. 3 */
  int32_t out_ch[PGTT_PERCEIVE_MAX_CONV]; /* a multiple of 16, at most 64 */
  int32_t kernel[PGTT_PERCEIVE_MAX_CONV]; /* 3 or 5 */
  int32_t stride[PGTT_PERCEIVE_MAX_CONV]; /* 1 or 2 */
  int32_t n_prop;                         /* 0 .. 64 */
  int32_t prop_rows[PGTT_PERCEIVE_MAX_PROP];      /* indices into the observation row, each in [0, obs_dim) */
  int32_t hidden;                         /* a multiple of 16, at most 512 */
  int32_t obs_dim;                        /* width of obs / obs_out */
  int32_t scan_row0;                      /* first scan row of the observation: 38 (PGTT_METHOD_PGTT), 30 (baseline); scan_row0 + 117 <= obs_dim */
} PgttPerceiveConfig;

/* device pointers, all caller-owned, sized for N = num_envs given to pgtt_perceive_create.  obs_out must not overlap obs. */
typedef struct PgttPerceiveBuffers {
  const float* depth;                     /* [N][H][W], required */
  const float* obs;                       /* [N][obs_dim], required */
  const float* w[PGTT_PERCEIVE_NLAYER];   /* packed weights, pgtt_perceive_packed_floats(cfg, l) floats; required for l < n_conv and l = 3, 4 */
  const float* b[PGTT_PERCEIVE_NLAYER];   /* biases: out_ch[l], hidden, 128 floats; required like w */
  float* latent;                          /* [N][F], required */
  float* est;                             /* [N][117], required */
  float* obs_out;                         /* [N][obs_dim] or NULL */
} PgttPerceiveBuffers;

/* the recurrent form: device pointers, all caller-owned.  The packed weights are in the linear tile order above with rows padded to 16 (3R and R are
 * multiples of 16 already) and w_out to 128 rows; gate q (0 = r, 1 = u, 2 = n) of memory value j is row q R + j of w_ih, w_hh, b_ih and b_hh.
 * w_ih, w_hh, w_out and b_out are read 16 bytes at a time and must be 16-byte aligned (PGTT_E_ARG otherwise); b_ih, b_hh, done, mem and the
 * clear_mask of a call are read and written as single values and need no alignment beyond their type's. */
typedef struct PgttPerceiveMemory {
  int32_t memory;                         /* R: a multiple of 16 in [16, PGTT_PERCEIVE_MAX_MEMORY] */
  const float* w_ih;                      /* packed [3R][hidden], required */
  const float* w_hh;                      /* packed [3R][R], required */
  const float* w_out;                     /* packed [128][R] (rows 117 .. 127 zero), required */
  const float* b_ih;                      /* [3R], required */
  const float* b_hh;                      /* [3R], required */
  const float* b_out;                     /* [128], required */
  const float* done;                      /* [N] 0 / 1 (PgttBuffers.done) or NULL: use_done then clears nothing */
  float* mem;                             /* [N][R], required: read and written by every recurrent call */
} PgttPerceiveMemory;

typedef struct pgtt_perceive_net* pgtt_perceive_handle;

/* host only: PGTT_OK, or PGTT_E_ARG for a config outside the ranges above - a channel count or `hidden` that is not a multiple of 16 or too large,
 * a layer whose output would be empty, a prop_rows entry outside [0, obs_dim), scan_row0 + 117 > obs_dim, activations past the LDS budget */
int pgtt_perceive_check(const PgttPerceiveConfig* cfg);
/* F of a config (>= 1), or PGTT_E_ARG */
int pgtt_perceive_latent_dim(const PgttPerceiveConfig* cfg);
/* floats of packed layer l (0 for a conv that is not there), or PGTT_E_ARG */
int pgtt_perceive_packed_floats(const PgttPerceiveConfig* cfg, int layer);
/* the refusals of pgtt_perceive_check; the config is copied */
int pgtt_perceive_create(const PgttPerceiveConfig* cfg, int device, int num_envs, pgtt_perceive_handle* out);
int pgtt_perceive_destroy(pgtt_perceive_handle h);
/* PGTT_E_ARG (the handle keeps what was bound before) when a required pointer is NULL.  A pgtt_perceive() captured in a HIP graph keeps the
 * addresses bound when it was captured. */
int pgtt_perceive_bind(pgtt_perceive_handle h, const PgttPerceiveBuffers* bufs);
/* one estimate for all N envs: two launches (the conv trunk, one workgroup per env; the head and the obs_out assembly, one workgroup per 16 envs).
 * PGTT_E_STATE before pgtt_perceive_bind. */
int pgtt_perceive(pgtt_perceive_handle h, void* stream);
/* host only: the refusals of pgtt_perceive_check, and PGTT_E_ARG for a `memory` that is no multiple of 16 in [16, PGTT_PERCEIVE_MAX_MEMORY] */
int pgtt_perceive_memory_check(const PgttPerceiveConfig* cfg, int memory);
/* host only: floats of a packed matrix of the recurrent form, which = 0 w_ih (3R * hidden), 1 w_hh (3R * R), 2 w_out (128 * R); or PGTT_E_ARG */
int pgtt_perceive_memory_packed_floats(const PgttPerceiveConfig* cfg, int memory, int which);
/* after pgtt_perceive_bind (PGTT_E_STATE before it): the recurrent form's weights and state, copied; NULL takes them away again.  PGTT_E_ARG for a
 * NULL required pointer or a bad `memory`; the handle then keeps what it had.  A captured recurrent call keeps the addresses set at capture. */
int pgtt_perceive_set_memory(pgtt_perceive_handle h, const PgttPerceiveMemory* mem_or_null);
/* one recurrent estimate for all N envs: two launches (the conv trunk of pgtt_perceive; the recurrent head - hidden layer, GRU cell, scan rows and the
 * obs_out assembly - one workgroup per 16 envs).  clear_mask: device uint8 [N] or NULL.  Reads the bound depth, obs, w[0 .. 3], b[0 .. 3] and writes
 * latent, est, obs_out and mem.  It never reads w[4] / b[4]: a recurrent caller binds any zero buffer of the right size there.
 * PGTT_E_STATE before pgtt_perceive_bind or before pgtt_perceive_set_memory. */
int pgtt_perceive_recurrent(pgtt_perceive_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream);
int pgtt_perceive_sizeof_memory(void);
int pgtt_perceive_sizeof_config(void);
int pgtt_perceive_sizeof_buffers(void);
/* "src=<SHA-256 of the library's sources, srchash.side_sha256("perceive")>;flavor=product" */
const char* pgtt_perceive_build_info(void);
const char* pgtt_perceive_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PGTT_PERCEIVE_H_ */
