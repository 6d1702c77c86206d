// pgtt_learn.hip — libpgtt_learn.so (include/pgtt_learn.h, gfx950): what one PPO minibatch update needs next to the two kernels of
// pgtt_ppo.hip, so that learn.py::NativeLearner runs the whole update as ~40 hand-written launches on one stream.
//
//   gather_kernel / adv_normalise_kernel     one workgroup per minibatch row (normalised observations, copies, the raw advantage), then ONE
//                                            workgroup: mean and population std of the advantages in a fixed order, normalised in place
//   linear_forward_kernel                    Z = X W^T + b, Y = silu(Z): fp32 MFMA 16x16x4 with blocked summation, four waves per workgroup, a 32x32 (or 32x16)
//                                            block of the output per wave, both operands straight from global memory as 16-byte runs along the
//                                            contraction index (lane (i, g) holds m = m0 + 4 g + s for the s-th of four MFMAs), next run prefetched
//   linear_backward_data_kernel              dX = (dY W) silu'(Zprev): the same blocking; W is walked by rows here (four dwords per lane)
//   value_loss_kernel                        one workgroup
//   adam_norm_kernel / adam_apply_kernel     partial sums of g^2 (and t + 1), then clip coefficient + Adam in every workgroup alike
//   gae_kernel                               one lane per env, one backward loop over T
//   distill_loss_kernel / distill_loss_finish   policy distillation (distill.py): one lane per row, KL(teacher || student) of the two heads with its gradient
//                                            and the error of the deterministic action, summed per workgroup in lane order, then in block order
//   gather_rows_kernel                       one workgroup per minibatch row: the normalised observation and its label row
//   normalise_kernel / recurrent_tail_kernel the recurrent policy's acting step (recurrent_policy.py): the normalising copy in front of three linear_forward
//                                            launches, then per 16 envs the GRU cell on MFMA (gates lane-local), m1, the head over h3 and m1, tanh, stores;
//                                            recurrent_tail_kernel<true> (pgtt_learn_recurrent_act_sample) ends in the tanh-normal head of policy_act_kernel
//                                            instead: the 16 x 24 head values through LDS, one lane per (env, actuator), Philox draws, u, logp, tanh(u)
//   gru_clear_rows / gru_cell_forward / gru_cell_backward / add_rows    the point-wise pieces of BPTT over that cell, one lane per (row, memory value)
// No atomics, no scratch, no LDS beyond the reductions' 16 words, recurrent_tail_kernel's two [16][R + 4] memory tiles and, in its sampled form, 2304 static
// bytes (the [16][24] head tile and the [16][12] log-probability terms); nothing allocates or synchronises.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pgtt_learn.h"
#include "pgtt_side_device.hip.h"
#include "pgtt_side_host.h"

namespace {

int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PGTT_OK : fail(PGTT_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
// four consecutive floats behind a pointer that is only 4-byte aligned (rows of 171 or 215 floats): one global_load_dwordx4
struct __attribute__((packed, aligned(4))) F4 { float x, y, z, w; };
__device__ __forceinline__ F4 ld4(const float* p) { return *reinterpret_cast<const F4*>(p); }

constexpr int kRed = 1024;          // lanes of the single-workgroup reductions

// sum over the workgroup, the same bits in every lane: xor butterfly inside a wave, then the waves' sums in wave order
__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();                                            // sh may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  const int nw = blockDim.x >> 6;
  for (int w = 0; w < nw; w++) s += sh[w];
  return s;
}

// ------------------------------------------------------------------ gather
__global__ __launch_bounds__(256) void gather_kernel(PgttLearnGatherArgs a) {
  const int i = blockIdx.x, tid = threadIdx.x;
  long r = a.idx[i];
  r = r < 0 ? 0 : (r >= a.rows ? (long)a.rows - 1 : r);
  for (int k = tid; k < a.obs_dim; k += 256) a.x_s[(long)i * a.obs_dim + k] = (a.obs[r * a.obs_dim + k] - a.mean_s[k]) / a.std_s[k];
  for (int k = tid; k < a.priv_dim; k += 256) a.x_p[(long)i * a.priv_dim + k] = (a.priv[r * a.priv_dim + k] - a.mean_p[k]) / a.std_p[k];
  for (int k = tid; k < a.act_dim; k += 256) a.u_out[(long)i * a.act_dim + k] = a.u[r * a.act_dim + k];
  if (tid == 64) a.logp_out[i] = a.logp[r];
  if (tid == 128) a.ret_out[i] = a.ret[r];
  if (tid == 192) a.adv_out[i] = a.adv[r];
}

__global__ __launch_bounds__(kRed) void adv_normalise_kernel(float* __restrict__ adv, int B) {
  __shared__ float sh[kRed / 64];
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += kRed) s += adv[i];
  const float mean = block_sum(s, sh) / (float)B;
  float q = 0.f;
  for (int i = threadIdx.x; i < B; i += kRed) { const float d = adv[i] - mean; q += d * d; }
  const float sd = sqrtf(block_sum(q, sh) / (float)B);
  for (int i = threadIdx.x; i < B; i += kRed) adv[i] = (adv[i] - mean) / (sd + 1e-8f);
}

// ------------------------------------------------------------------ the two GEMMs
// A workgroup is four waves, WR x WC of them over the output; a wave owns 32 rows x (16 NCT) columns: 2 x NCT accumulators of the 16x16x4 form.
// C/D map of that form: register r of lane l is row 4 (l >> 4) + r, column l & 15.
// One round = 16 terms of the contraction.  The round's products are summed in accumulators of their own that start at zero, and only the round's
// sum is added to the running total (blocked summation): the long chain has one link per 16 terms instead of four, which halves the rounding error
// of a 512-term row against one accumulator chained through every MFMA - at the price of 8 NCT vector adds per 8 NCT MFMAs.
template <int NCT>
__device__ __forceinline__ void mfma_round(const F4 (&a)[2], const F4 (&b)[NCT], f32x4 (&acc)[2][NCT]) {
  f32x4 blk[2][NCT];
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int c = 0; c < NCT; c++) blk[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, b[c].x, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int c = 0; c < NCT; c++) blk[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, b[c].y, blk[t][c], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int c = 0; c < NCT; c++) blk[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, b[c].z, blk[t][c], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int c = 0; c < NCT; c++) blk[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, b[c].w, blk[t][c], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int c = 0; c < NCT; c++) acc[t][c] += blk[t][c];
}

__device__ __forceinline__ float silu_f(float z) { return z / (1.0f + expf(-z)); }
// fp64, rounded once: silu' passes through 0 at z = -1.2785, where s and s z (1 - s) cancel
__device__ __forceinline__ float dsilu_f(float zf) {
  const double z = (double)zf, s = 1.0 / (1.0 + exp(-z));
  return (float)(s * (1.0 + z * (1.0 - s)));
}

template <int WC, int NCT>
__global__ __launch_bounds__(256) void linear_forward_kernel(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                                             int K, int M, int N, int act, float* __restrict__ Y, float* __restrict__ Z) {
  constexpr int WR = 4 / WC;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
  const long r0 = (long)blockIdx.x * (WR * 32) + (wave / WC) * 32;
  const int c0 = blockIdx.y * (WC * NCT * 16) + (wave % WC) * (NCT * 16);
  if (r0 >= K || c0 >= N) return;                        // wave-uniform; the kernel has no barrier
  // operand rows of this lane, clamped: a row or column past the edge repeats the last one and is not stored
  const float* xa[2];
  const float* wb[NCT];
#pragma unroll
  for (int t = 0; t < 2; t++) { const long r = r0 + 16 * t + li; xa[t] = X + (r < K ? r : (long)K - 1) * M + 4 * g; }
#pragma unroll
  for (int c = 0; c < NCT; c++) { const int n = c0 + 16 * c + li; wb[c] = W + (long)(n < N ? n : N - 1) * M + 4 * g; }
  f32x4 acc[2][NCT];
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int c = 0; c < NCT; c++) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  F4 a[2], b[NCT];
  const int nfull = M / 16;
  if (nfull > 0) {
#pragma unroll
    for (int t = 0; t < 2; t++) a[t] = ld4(xa[t]);
#pragma unroll
    for (int c = 0; c < NCT; c++) b[c] = ld4(wb[c]);
    for (int i = 0; i < nfull; i++) {
      const int nx = (i + 1 < nfull ? i + 1 : i) * 16;   // the last trip loads its own run again instead of branching
      F4 an[2], bn[NCT];
#pragma unroll
      for (int t = 0; t < 2; t++) an[t] = ld4(xa[t] + nx);
#pragma unroll
      for (int c = 0; c < NCT; c++) bn[c] = ld4(wb[c] + nx);
      mfma_round<NCT>(a, b, acc);
#pragma unroll
      for (int t = 0; t < 2; t++) a[t] = an[t];
#pragma unroll
      for (int c = 0; c < NCT; c++) b[c] = bn[c];
    }
  }
  const int m0 = nfull * 16;
  if (m0 < M) {                                          // the last 1 .. 15 terms: element by element, zeros past the end (nothing is read there)
    const int mq = m0 + 4 * g;
    const bool o0 = mq < M, o1 = mq + 1 < M, o2 = mq + 2 < M, o3 = mq + 3 < M;
#pragma unroll
    for (int t = 0; t < 2; t++) { const float* p = xa[t] + m0; a[t] = F4{o0 ? p[0] : 0.f, o1 ? p[1] : 0.f, o2 ? p[2] : 0.f, o3 ? p[3] : 0.f}; }
#pragma unroll
    for (int c = 0; c < NCT; c++) { const float* p = wb[c] + m0; b[c] = F4{o0 ? p[0] : 0.f, o1 ? p[1] : 0.f, o2 ? p[2] : 0.f, o3 ? p[3] : 0.f}; }
    mfma_round<NCT>(a, b, acc);
  }
#pragma unroll
  for (int c = 0; c < NCT; c++) {
    const int n = c0 + 16 * c + li;
    if (n >= N) continue;
    const float bn = bias[n];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const long row = r0 + 16 * t + 4 * g + r;
        if (row >= K) continue;
        const float z = acc[t][c][r] + bn;
        if (Z) Z[row * N + n] = z;
        Y[row * N + n] = act ? silu_f(z) : z;
      }
  }
}

template <int WC, int NCT>
__global__ __launch_bounds__(256) void linear_backward_data_kernel(const float* __restrict__ dY, const float* __restrict__ W, const float* __restrict__ Zp,
                                                                   int K, int M, int N, float* __restrict__ dX) {
  constexpr int WR = 4 / WC;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
  const long r0 = (long)blockIdx.x * (WR * 32) + (wave / WC) * 32;
  const int c0 = blockIdx.y * (WC * NCT * 16) + (wave % WC) * (NCT * 16);
  if (r0 >= K || c0 >= M) return;
  const float* ya[2];
  const float* wb[NCT];                                  // column m of W, at row 4 g: the lane's four rows are M floats apart
#pragma unroll
  for (int t = 0; t < 2; t++) { const long r = r0 + 16 * t + li; ya[t] = dY + (r < K ? r : (long)K - 1) * N + 4 * g; }
#pragma unroll
  for (int c = 0; c < NCT; c++) { const int m = c0 + 16 * c + li; wb[c] = W + (long)(4 * g) * M + (m < M ? m : M - 1); }
  f32x4 acc[2][NCT];
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int c = 0; c < NCT; c++) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  F4 a[2], b[NCT];
  const int nfull = N / 16;
  const long M1 = M, M2 = 2L * M, M3 = 3L * M;
  if (nfull > 0) {
#pragma unroll
    for (int t = 0; t < 2; t++) a[t] = ld4(ya[t]);
#pragma unroll
    for (int c = 0; c < NCT; c++) b[c] = F4{wb[c][0], wb[c][M1], wb[c][M2], wb[c][M3]};
    for (int i = 0; i < nfull; i++) {
      const int nx = (i + 1 < nfull ? i + 1 : i) * 16;
      F4 an[2], bn[NCT];
#pragma unroll
      for (int t = 0; t < 2; t++) an[t] = ld4(ya[t] + nx);
#pragma unroll
      for (int c = 0; c < NCT; c++) { const float* p = wb[c] + (long)nx * M; bn[c] = F4{p[0], p[M1], p[M2], p[M3]}; }
      mfma_round<NCT>(a, b, acc);
#pragma unroll
      for (int t = 0; t < 2; t++) a[t] = an[t];
#pragma unroll
      for (int c = 0; c < NCT; c++) b[c] = bn[c];
    }
  }
  const int n0 = nfull * 16;
  if (n0 < N) {
    const int nq = n0 + 4 * g;
    const bool o0 = nq < N, o1 = nq + 1 < N, o2 = nq + 2 < N, o3 = nq + 3 < N;
#pragma unroll
    for (int t = 0; t < 2; t++) { const float* p = ya[t] + n0; a[t] = F4{o0 ? p[0] : 0.f, o1 ? p[1] : 0.f, o2 ? p[2] : 0.f, o3 ? p[3] : 0.f}; }
#pragma unroll
    for (int c = 0; c < NCT; c++) { const float* p = wb[c] + (long)n0 * M; b[c] = F4{o0 ? p[0] : 0.f, o1 ? p[M1] : 0.f, o2 ? p[M2] : 0.f, o3 ? p[M3] : 0.f}; }
    mfma_round<NCT>(a, b, acc);
  }
#pragma unroll
  for (int c = 0; c < NCT; c++) {
    const int m = c0 + 16 * c + li;
    if (m >= M) continue;
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const long row = r0 + 16 * t + 4 * g + r;
        if (row >= K) continue;
        const float d = acc[t][c][r];
        dX[row * M + m] = Zp ? d * dsilu_f(Zp[row * M + m]) : d;
      }
  }
}

// cols: the width of the output.  Wide outputs take 64 x 64 per workgroup, narrow ones (the heads: 24, 1) stack the four waves over the rows
template <typename F>
int launch_gemm(int K, int cols, const char* who, F&& go) {
  const int wc = cols > 32 ? 2 : 1, nct = cols > 16 ? 2 : 1;
  const long gx = ((long)K + (4 / wc) * 32 - 1) / ((4 / wc) * 32), gy = ((long)cols + wc * nct * 16 - 1) / (wc * nct * 16);
  if (gy > 65535) return fail(PGTT_E_ARG, std::string(who) + ": more than 65535 column blocks");
  go(wc, nct, dim3((unsigned)gx, (unsigned)gy));
  return launched(who);
}

// ------------------------------------------------------------------ value loss
__global__ __launch_bounds__(kRed) void value_loss_kernel(const float* __restrict__ v, const float* __restrict__ ret, int B, float* __restrict__ loss,
                                                          float* __restrict__ dv) {
  __shared__ float sh[kRed / 64];
  const float fB = (float)B;
  float q = 0.f;
  for (int i = threadIdx.x; i < B; i += kRed) {
    const float d = v[i] - ret[i];
    q += d * d;
    dv[i] = 0.5f * d / fB;
  }
  q = block_sum(q, sh);
  if (threadIdx.x == 0) loss[0] = 0.25f * (q / fB);
}

// ------------------------------------------------------------------ clip + Adam
__global__ __launch_bounds__(256) void adam_norm_kernel(float* __restrict__ g, long P, float grad_scale, float* __restrict__ partial, int64_t* __restrict__ t) {
  __shared__ float sh[4];
  float q = 0.f;
  const long stride = (long)gridDim.x * 256;
  if (grad_scale != 1.0f) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += stride) { const float x = g[i] * grad_scale; g[i] = x; q += x * x; }
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += stride) { const float x = g[i]; q += x * x; }
  }
  q = block_sum(q, sh);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = q;
    if (blockIdx.x == 0) t[0] = t[0] + 1;
  }
}

struct AdamK {
  float* p; const float* g; float* m; float* v; const int64_t* t; const float* partial; float* norm;
  long P; int nb; double lr, b1, b2, eps; float max_norm;
};

__global__ __launch_bounds__(256) void adam_apply_kernel(AdamK a) {
  __shared__ float sh[4];
  __shared__ float bc[2];
  float q = 0.f;
  for (int i = threadIdx.x; i < a.nb; i += 256) q += a.partial[i];
  q = block_sum(q, sh);                                   // every workgroup: the same partials in the same order
  if (threadIdx.x == 0) {
    const double t = (double)a.t[0];
    bc[0] = (float)(1.0 - pow(a.b1, t));
    bc[1] = (float)(1.0 - pow(a.b2, t));
  }
  __syncthreads();
  const float norm = sqrtf(q), coef = fminf(1.0f, a.max_norm / (norm + 1e-6f));
  if (blockIdx.x == 0 && threadIdx.x == 0) a.norm[0] = norm;
  const float b1 = (float)a.b1, b2 = (float)a.b2, c1 = (float)(1.0 - a.b1), c2 = (float)(1.0 - a.b2), lr = (float)a.lr, eps = (float)a.eps;
  const float bc1 = bc[0], bc2 = bc[1];
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.P; i += stride) {
    const float c = coef * a.g[i];
    const float m = b1 * a.m[i] + c1 * c, v = b2 * a.v[i] + c2 * (c * c);
    a.m[i] = m; a.v[i] = v;
    a.p[i] = a.p[i] - lr * (m / bc1) / (sqrtf(v / bc2) + eps);
  }
}

// workgroups of the first pass = partial sums (2048 elements each, at most 1024), and of the second pass (1024 elements each, at most 2048)
int adam_blocks(long P) { const long nb = (P + 2047) / 2048; return (int)(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb)); }
int adam_apply_blocks(long P) { const long nb = (P + 1023) / 1024; return (int)(nb < 1 ? 1 : (nb > 2048 ? 2048 : nb)); }

// ------------------------------------------------------------------ GAE
__global__ __launch_bounds__(256) void gae_kernel(const float* __restrict__ trunc, const float* __restrict__ done, const float* __restrict__ rew,
                                                  const float* __restrict__ val, const float* __restrict__ boot, int T, int N, float lam, float gamma,
                                                  float* __restrict__ adv, float* __restrict__ vs) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  const float gl = gamma * lam;
  float acc = 0.f, v_next = boot[e], vs_next = v_next;
  for (int t = T - 1; t >= 0; t--) {
    const long k = (long)t * N + e;
    const float tr = trunc[k], mask = 1.0f - tr, nonterm = 1.0f - done[k] * mask, r = rew[k], v = val[k];
    const float delta = (r + gamma * nonterm * v_next - v) * mask;
    acc = delta + gl * nonterm * mask * acc;
    adv[k] = (r + gamma * nonterm * vs_next - v) * mask;
    vs_next = acc + v;
    vs[k] = vs_next;
    v_next = v;
  }
}

// ------------------------------------------------------------------ distillation: KL(teacher || student) of two heads, its gradient; the row gather
// finite for every finite r: exp never sees a positive argument
__device__ __forceinline__ float softplus_stable(float r) { return fmaxf(r, 0.f) + log1pf(expf(-fabsf(r))); }
__device__ __forceinline__ float sigmoid_stable(float r) {
  const float e = expf(-fabsf(r));
  return r >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// the sum of v over the wave in lane order 0, 1, .. 63, the same bits in every lane
__device__ __forceinline__ float lane_order_sum(float v) {
  float s = 0.f;
  for (int l = 0; l < 64; l++) s += __shfl(v, l);
  return s;
}

__global__ __launch_bounds__(64) void distill_loss_kernel(const float* __restrict__ student, const float* __restrict__ teacher, int B, int A,
                                                          float* __restrict__ partial, float* __restrict__ grad) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  const bool on = i < B;
  const float fB = (float)B;
  float kl = 0.f, act = 0.f;
  if (on) {
    const float* s = student + i * 2 * A;
    const float* t = teacher + i * 2 * A;
    float* g = grad + i * 2 * A;
    for (int a = 0; a < A; a++) {
      const float ls = s[a], rs = s[A + a], lt = t[a], rt = t[A + a];
      const float ss = softplus_stable(rs) + 1e-3f, st = softplus_stable(rt) + 1e-3f;
      const float e = ls - lt;                               // -d
      const float ss2 = ss * ss;
      const float q = (st * st + e * e) / ss2;               // exactly 1 where the student has the teacher's bits
      kl += logf(ss / st) + 0.5f * (q - 1.0f);
      const float dt = tanhf(ls) - tanhf(lt);
      act += dt * dt;
      g[a] = e / ss2 / fB;
      g[A + a] = (1.0f - q) / ss * sigmoid_stable(rs) / fB;
    }
  }
  const float v0 = lane_order_sum(kl), v1 = lane_order_sum(act);
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = v0; partial[2 * blockIdx.x + 1] = v1; }
}

// one wave: 64 partials at a time, each run added in block order onto the running sums
__global__ __launch_bounds__(64) void distill_loss_finish(const float* __restrict__ partial, int nblocks, int B, int A, float* __restrict__ loss) {
  float v0 = 0.f, v1 = 0.f;
  for (int b0 = 0; b0 < nblocks; b0 += 64) {
    const int b = b0 + threadIdx.x;
    const float p0 = b < nblocks ? partial[2 * b] : 0.f, p1 = b < nblocks ? partial[2 * b + 1] : 0.f;
    const int n = nblocks - b0 < 64 ? nblocks - b0 : 64;
    for (int l = 0; l < n; l++) { v0 += __shfl(p0, l); v1 += __shfl(p1, l); }
  }
  if (threadIdx.x == 0) { loss[0] = v0 / (float)B; loss[1] = v1 / ((float)B * (float)A); }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const int64_t* __restrict__ idx, const float* __restrict__ obs, const float* __restrict__ target,
                                                          const float* __restrict__ mean, const float* __restrict__ std, int rows, int obs_dim, int tgt_dim,
                                                          float* __restrict__ x, float* __restrict__ y) {
  const int i = blockIdx.x, tid = threadIdx.x;
  long r = idx[i];
  r = r < 0 ? 0 : (r >= rows ? (long)rows - 1 : r);
  for (int k = tid; k < obs_dim; k += 256) x[(long)i * obs_dim + k] = (obs[r * obs_dim + k] - mean[k]) / std[k];
  for (int k = tid; k < tgt_dim; k += 256) y[(long)i * tgt_dim + k] = target[r * tgt_dim + k];
}

// ------------------------------------------------------------------ the recurrent policy: the acting step from h3 on, and the point-wise pieces of BPTT
// no overflow at any v: exp never sees a positive argument
__device__ __forceinline__ float tanh_stable(float v) {
  const float t = expf(-2.0f * fabsf(v));
  return copysignf((1.0f - t) / (1.0f + t), v);
}

__global__ __launch_bounds__(256) void normalise_kernel(const float* __restrict__ obs, const float* __restrict__ mean, const float* __restrict__ std, int od,
                                                        float* __restrict__ x, float* __restrict__ store_obs) {
  const long e = blockIdx.x;
  for (int k = threadIdx.x; k < od; k += 256) {
    const float o = obs[e * od + k];
    x[e * od + k] = (o - mean[k]) / std[k];
    if (store_obs) store_obs[e * od + k] = o;
  }
}

// one step of a chain over 16 k: s outer (the four MFMAs), g inner (the four k of one MFMA)
__device__ __forceinline__ f32x4 mfma16(const F4& a, const F4& b, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

struct RecurrentK {
  const float *h3, *w_ih, *w_hh, *b_ih, *b_hh, *w3, *b3, *w_m, *done;
  const uint8_t* clear_mask;
  float *mem, *action, *head, *store_mem0;         // the two store pointers are those of row t
  uint8_t* store_clear;
  int N, H, R, clear_all, use_done;
};

// what the sampled tail needs on top: the tanh-normal head of policy_act_kernel (pgtt_policy.hip), its forms and its draws
struct SampleK {
  const float* eps;
  const int64_t* counters;
  float *store_u, *store_logp;                     // those of row t
  unsigned long long seed;
  long env_id_offset;
  int deterministic;
};
template <bool SAMPLE> struct TailK : RecurrentK { SampleK s; };
template <> struct TailK<false> : RecurrentK {};

__device__ __forceinline__ float softplus_t(float x) { return x > 20.f ? x : log1pf(expf(x)); }      // torch F.softplus (threshold 20)

constexpr int kHead = 24, kAct = 12;

// the sampled tail's static LDS, 1536 + 768 bytes; only the kernel that calls these owns them.  With scl's 64 bytes the statics stay a multiple of 16, so
// the dynamic memory tiles behind them keep their 16-byte alignment (their rows are read as 128-bit runs)
__device__ __forceinline__ float* sampled_head_tile() { __shared__ float t[16 * kHead]; return t; }
__device__ __forceinline__ float* sampled_logp_tile() { __shared__ float t[16 * kAct]; return t; }

// One workgroup of four waves per 16 envs.  LDS: m0 and m1 of the 16 envs, [16][R + 4] floats each (the rows 16 bytes apart from a multiple of the
// 32 banks).  A wave owns the memory values 16 ct .. 16 ct + 15 for ct = wave, wave + 4, ..: four accumulators (r, u, gi_n, gh_n) in the C layout of the
// 16x16x4 form - register q of lane l is env 4 (l >> 4) + q, memory value 16 ct + (l & 15) - so the gates and m1 are lane-local.  Then the head:
// waves 0 and 1 take its columns 0..15 and 16..23.  Rows past N repeat env N - 1's h3, count as cleared and are not stored.
// SAMPLE: loc[j] and raw[j] of an actuator sit in different lanes (and, for j >= 4, waves), so waves 0 and 1 leave the 16 x 24 head values in a static
// LDS tile (1536 bytes) and, after one barrier, lane tid < 16 * 12 takes one (env, actuator): scale, the draw, u, its log-probability term (into a
// second static tile, 768 bytes: 2304 bytes in all), tanh(u); after a second barrier one lane per env adds the 12 terms, j ascending.  Rows past N
// are neither drawn for nor stored.
template <bool SAMPLE>
__global__ __launch_bounds__(256) void recurrent_tail_kernel(TailK<SAMPLE> a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int scl[16];
  const int R = a.R, H = a.H, LS = R + 4;
  float* sm0 = lds;
  float* sm1 = lds + 16 * LS;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const long e0 = (long)blockIdx.x * 16;
  float *shead = nullptr, *slp = nullptr;
  if constexpr (SAMPLE) { shead = sampled_head_tile(); slp = sampled_logp_tile(); }
  if (tid < 16) {
    const long e = e0 + tid;
    int c = 1;
    if (e < a.N) {
      c = a.clear_all != 0 || (a.clear_mask && a.clear_mask[e] != 0) || (a.use_done && a.done && a.done[e] != 0.f);
      if (a.store_clear) a.store_clear[e] = (uint8_t)c;
    }
    scl[tid] = c;
  }
  __syncthreads();
  for (int k = tid; k < 16 * R; k += 256) {
    const int i = k / R, j = k - i * R;
    const long e = e0 + i;
    const float v = scl[i] ? 0.f : a.mem[e * R + j];          // a cleared env's row is not read
    sm0[i * LS + j] = v;
    if (a.store_mem0 && e < a.N) a.store_mem0[e * R + j] = v;
  }
  __syncthreads();
  const long er = e0 + li < a.N ? e0 + li : (long)a.N - 1;
  const float* xa = a.h3 + er * H + 4 * g;
  const float* ma = sm0 + li * LS + 4 * g;
  for (int ct = wave; ct < R / 16; ct += 4) {
    const int j = ct * 16 + li;
    f32x4 ar = {0.f, 0.f, 0.f, 0.f}, au = ar, an = ar, ahn = ar;
    const float* wr = a.w_ih + (long)j * H + 4 * g;
    const float* wu = wr + (long)R * H;
    const float* wn = wu + (long)R * H;
    for (int kb = 0; kb < H; kb += 16) {
      const F4 x = ld4(xa + kb);
      ar = mfma16(x, ld4(wr + kb), ar);
      au = mfma16(x, ld4(wu + kb), au);
      an = mfma16(x, ld4(wn + kb), an);
    }
    const float* vr = a.w_hh + (long)j * R + 4 * g;
    const float* vu = vr + (long)R * R;
    const float* vn = vu + (long)R * R;
    for (int kb = 0; kb < R; kb += 16) {
      const F4 x = ld4(ma + kb);
      ar = mfma16(x, ld4(vr + kb), ar);
      au = mfma16(x, ld4(vu + kb), au);
      ahn = mfma16(x, ld4(vn + kb), ahn);
    }
    const float bir = a.b_ih[j], biu = a.b_ih[R + j], bin = a.b_ih[2 * R + j];
    const float bhr = a.b_hh[j], bhu = a.b_hh[R + j], bhn = a.b_hh[2 * R + j];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = 4 * g + q;
      const float r = sigmoid_stable((ar[q] + bir) + bhr), u = sigmoid_stable((au[q] + biu) + bhu);
      const float n = tanh_stable((an[q] + bin) + r * (ahn[q] + bhn));
      const float m1 = (1.0f - u) * n + u * sm0[i * LS + j];
      sm1[i * LS + j] = m1;
      if (e0 + i < a.N) a.mem[(e0 + i) * R + j] = m1;
    }
  }
  __syncthreads();
  if (wave < 2) {
    const int c = wave * 16 + li, cr = c < kHead ? c : kHead - 1;        // a column past the head repeats the last one and is not stored
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* w3 = a.w3 + (long)cr * H + 4 * g;
    for (int kb = 0; kb < H; kb += 16) acc = mfma16(ld4(xa + kb), ld4(w3 + kb), acc);
    const float* wm = a.w_m + (long)cr * R + 4 * g;
    const float* mb = sm1 + li * LS + 4 * g;
    for (int kb = 0; kb < R; kb += 16) acc = mfma16(ld4(mb + kb), ld4(wm + kb), acc);
    if (c < kHead) {
      const float b = a.b3[c];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const long e = e0 + 4 * g + q;
        if constexpr (SAMPLE) shead[(4 * g + q) * kHead + c] = acc[q] + b;      // rows past N too: finite, and nobody reads them
        if (e >= a.N) continue;
        const float v = acc[q] + b;
        if (a.head) a.head[e * kHead + c] = v;
        if constexpr (!SAMPLE) {
          if (c < kAct) a.action[e * kAct + c] = tanh_stable(v);
        }
      }
    }
  }
  if constexpr (SAMPLE) {
    __syncthreads();
    if (tid < 16 * kAct) {
      const int env = tid / kAct, j = tid - env * kAct;
      const long e = e0 + env;
      float lp = 0.f;
      if (e < a.N) {
        const float loc = shead[env * kHead + j], raw = shead[env * kHead + kAct + j];
        const float sc = softplus_t(raw) + 1e-3f;
        float eps;
        if (a.s.eps) eps = a.s.eps[e * kAct + j];
        else {
          // one Philox block per (env, draw, actuator pair): Box-Muller on two of its four words (pgtt_train.h)
          const unsigned long long draw = a.s.counters ? (unsigned long long)a.s.counters[1] : 0ull;
          unsigned c0 = (unsigned)(a.s.env_id_offset + e), c1 = (unsigned)draw, c2 = (unsigned)(draw >> 32) ^ 0x50475454u, c3 = (unsigned)(j >> 1);
          philox4x32_10((unsigned)a.s.seed, (unsigned)(a.s.seed >> 32), c0, c1, c2, c3);
          const float u1 = ((float)(c0 >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = (float)(c1 >> 8) * (1.0f / 16777216.0f);
          const float r = sqrtf(-2.0f * logf(u1));
          float sn, cs; sincosf(6.28318530717958648f * u2, &sn, &cs);
          eps = (j & 1) ? r * sn : r * cs;
        }
        const float u = a.s.deterministic ? loc : loc + sc * eps;
        const float z = (u - loc) / sc;
        const float kHalfLog2Pi = 0.91893853320467274f, kLog2 = 0.69314718055994531f;
        lp = -0.5f * z * z - logf(sc) - kHalfLog2Pi - 2.0f * (kLog2 - u - softplus_t(-2.0f * u));
        a.action[e * kAct + j] = tanh_stable(u);
        if (a.s.store_u) a.s.store_u[e * kAct + j] = u;
      }
      slp[tid] = lp;
    }
    __syncthreads();
    if (tid < 16 && e0 + tid < a.N && a.s.store_logp) {
      float lp = 0.f;
#pragma unroll
      for (int j = 0; j < kAct; j++) lp += slp[tid * kAct + j];
      a.s.store_logp[e0 + tid] = lp;
    }
  }
}

__global__ __launch_bounds__(256) void gru_clear_rows_kernel(const float* __restrict__ m, const uint8_t* __restrict__ clear, long n, int R, float* __restrict__ m0) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  m0[k] = clear[k / R] ? 0.f : m[k];
}

__global__ __launch_bounds__(256) void gru_cell_forward_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ m0,
                                                               const uint8_t* __restrict__ clear_next, long n, int R, float* __restrict__ gates,
                                                               float* __restrict__ m1, float* __restrict__ m0_next) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const long i = k / R, b = i * 3 * R + (k - i * R);
  const float r = sigmoid_stable(gi[b] + gh[b]), u = sigmoid_stable(gi[b + R] + gh[b + R]);
  const float nn = tanh_stable(gi[b + 2 * R] + r * gh[b + 2 * R]);
  const float v = (1.0f - u) * nn + u * m0[k];
  gates[b] = r; gates[b + R] = u; gates[b + 2 * R] = nn;
  m1[k] = v;
  if (m0_next) m0_next[k] = (clear_next && clear_next[i]) ? 0.f : v;
}

__global__ __launch_bounds__(256) void gru_cell_backward_kernel(const float* __restrict__ gates, const float* __restrict__ gh, const float* __restrict__ m0,
                                                                const float* __restrict__ dm1_head, const float* __restrict__ dm0_next,
                                                                const uint8_t* __restrict__ clear_next, long n, int R, float* __restrict__ dgi,
                                                                float* __restrict__ dgh, float* __restrict__ dm0_direct) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const long i = k / R, b = i * 3 * R + (k - i * R);
  float dm1 = dm1_head[k];
  if (dm0_next && !(clear_next && clear_next[i])) dm1 += dm0_next[k];
  const float r = gates[b], u = gates[b + R], nn = gates[b + 2 * R];
  const float dn = dm1 * (1.0f - u), du = dm1 * (m0[k] - nn);
  const float dpn = dn * (1.0f - nn * nn), dpu = du * (u * (1.0f - u));
  const float dr = gh[b + 2 * R] * dpn, dpr = dr * (r * (1.0f - r));
  dgi[b] = dpr; dgi[b + R] = dpu; dgi[b + 2 * R] = dpn;
  dgh[b] = dpr; dgh[b + R] = dpu; dgh[b + 2 * R] = r * dpn;
  dm0_direct[k] = u * dm1;
}

__global__ __launch_bounds__(256) void add_rows_kernel(const float* a, const float* b, long n, float* out) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k < n) out[k] = a[k] + b[k];
}

bool memory_ok(int R) { return R >= 16 && R <= PGTT_LEARN_MAX_MEMORY && R % 16 == 0; }
unsigned blocks256(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

PGTT_SIDE_EXPORTS(learn, LEARN)
int pgtt_learn_sizeof_gather_args(void) { return (int)sizeof(PgttLearnGatherArgs); }
int pgtt_learn_sizeof_adam_args(void) { return (int)sizeof(PgttLearnAdamArgs); }
int pgtt_learn_adam_partials(int64_t P) { return P > 0 ? adam_blocks((long)P) : 0; }

int pgtt_learn_gather(const PgttLearnGatherArgs* a, void* stream) {
  if (!a) return fail(PGTT_E_ARG, "pgtt_learn_gather: null args");
  if (!a->idx || !a->obs || !a->priv || !a->u || !a->logp || !a->adv || !a->ret || !a->mean_s || !a->std_s || !a->mean_p || !a->std_p || !a->x_s ||
      !a->x_p || !a->u_out || !a->logp_out || !a->adv_out || !a->ret_out)
    return fail(PGTT_E_ARG, "pgtt_learn_gather: null pointer");
  if (a->B <= 0 || a->rows <= 0 || a->obs_dim <= 0 || a->priv_dim <= 0 || a->act_dim <= 0) return fail(PGTT_E_ARG, "pgtt_learn_gather: B, rows, obs_dim, priv_dim and act_dim must be positive");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gather_kernel, dim3(a->B), dim3(256), 0, st, *a);
  hipLaunchKernelGGL(adv_normalise_kernel, dim3(1), dim3(kRed), 0, st, a->adv_out, a->B);
  return launched("pgtt_learn_gather");
}

int pgtt_learn_linear_forward(const float* x, const float* w, const float* b, int K, int M, int N, int act, float* y, float* z, void* stream) {
  if (!x || !w || !b || !y) return fail(PGTT_E_ARG, "pgtt_learn_linear_forward: null pointer");
  if (act && !z) return fail(PGTT_E_ARG, "pgtt_learn_linear_forward: act != 0 needs z (the backward pass reads the pre-activation)");
  if (K <= 0 || M <= 0 || N <= 0) return fail(PGTT_E_ARG, "pgtt_learn_linear_forward: K, M and N must be positive");
  hipStream_t st = (hipStream_t)stream;
  return launch_gemm(K, N, "pgtt_learn_linear_forward", [&](int wc, int nct, dim3 grid) {
    if (wc == 2) hipLaunchKernelGGL((linear_forward_kernel<2, 2>), grid, dim3(256), 0, st, x, w, b, K, M, N, act, y, z);
    else if (nct == 2) hipLaunchKernelGGL((linear_forward_kernel<1, 2>), grid, dim3(256), 0, st, x, w, b, K, M, N, act, y, z);
    else hipLaunchKernelGGL((linear_forward_kernel<1, 1>), grid, dim3(256), 0, st, x, w, b, K, M, N, act, y, z);
  });
}

int pgtt_learn_linear_backward_data(const float* dy, const float* w, const float* zprev, int K, int M, int N, float* dx, void* stream) {
  if (!dy || !w || !dx) return fail(PGTT_E_ARG, "pgtt_learn_linear_backward_data: null pointer");
  if (K <= 0 || M <= 0 || N <= 0) return fail(PGTT_E_ARG, "pgtt_learn_linear_backward_data: K, M and N must be positive");
  hipStream_t st = (hipStream_t)stream;
  return launch_gemm(K, M, "pgtt_learn_linear_backward_data", [&](int wc, int nct, dim3 grid) {
    if (wc == 2) hipLaunchKernelGGL((linear_backward_data_kernel<2, 2>), grid, dim3(256), 0, st, dy, w, zprev, K, M, N, dx);
    else if (nct == 2) hipLaunchKernelGGL((linear_backward_data_kernel<1, 2>), grid, dim3(256), 0, st, dy, w, zprev, K, M, N, dx);
    else hipLaunchKernelGGL((linear_backward_data_kernel<1, 1>), grid, dim3(256), 0, st, dy, w, zprev, K, M, N, dx);
  });
}

int pgtt_learn_value_loss(const float* v, const float* ret, int B, float* loss, float* dv, void* stream) {
  if (!v || !ret || !loss || !dv) return fail(PGTT_E_ARG, "pgtt_learn_value_loss: null pointer");
  if (B <= 0) return fail(PGTT_E_ARG, "pgtt_learn_value_loss: B must be positive");
  hipLaunchKernelGGL(value_loss_kernel, dim3(1), dim3(kRed), 0, (hipStream_t)stream, v, ret, B, loss, dv);
  return launched("pgtt_learn_value_loss");
}

int pgtt_learn_clip_adam(const PgttLearnAdamArgs* a, void* stream) {
  if (!a) return fail(PGTT_E_ARG, "pgtt_learn_clip_adam: null args");
  if (!a->p || !a->g || !a->m || !a->v || !a->t || !a->partial || !a->norm_1) return fail(PGTT_E_ARG, "pgtt_learn_clip_adam: null pointer");
  if (a->P <= 0) return fail(PGTT_E_ARG, "pgtt_learn_clip_adam: P must be positive");
  const int nb = adam_blocks((long)a->P);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_norm_kernel, dim3(nb), dim3(256), 0, st, a->g, (long)a->P, a->grad_scale, a->partial, a->t);
  AdamK k{a->p, a->g, a->m, a->v, a->t, a->partial, a->norm_1, (long)a->P, nb, a->lr, a->beta1, a->beta2, a->eps, a->max_norm};
  hipLaunchKernelGGL(adam_apply_kernel, dim3(adam_apply_blocks((long)a->P)), dim3(256), 0, st, k);
  return launched("pgtt_learn_clip_adam");
}

int pgtt_learn_gae(const float* trunc, const float* done, const float* rew, const float* val, const float* boot, int T, int N, float lambda, float gamma,
                   float* adv, float* vs, void* stream) {
  if (!trunc || !done || !rew || !val || !boot || !adv || !vs) return fail(PGTT_E_ARG, "pgtt_learn_gae: null pointer");
  if (T <= 0 || N <= 0) return fail(PGTT_E_ARG, "pgtt_learn_gae: T and N must be positive");
  hipLaunchKernelGGL(gae_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, trunc, done, rew, val, boot, T, N, lambda, gamma, adv, vs);
  return launched("pgtt_learn_gae");
}

int pgtt_learn_distill_loss(const float* student, const float* teacher, int B, int A, float* partial, float* loss, float* grad, void* stream) {
  if (!student || !teacher || !partial || !loss || !grad) return fail(PGTT_E_ARG, "pgtt_learn_distill_loss: null pointer");
  if (B <= 0 || A <= 0) return fail(PGTT_E_ARG, "pgtt_learn_distill_loss: B and A must be positive");
  const int nb = (B + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(distill_loss_kernel, dim3(nb), dim3(64), 0, st, student, teacher, B, A, partial, grad);
  hipLaunchKernelGGL(distill_loss_finish, dim3(1), dim3(64), 0, st, partial, nb, B, A, loss);
  return launched("pgtt_learn_distill_loss");
}

int pgtt_learn_gather_rows(const int64_t* idx, const float* obs, const float* target, const float* mean, const float* std, int B, int rows, int obs_dim,
                           int tgt_dim, float* x, float* y, void* stream) {
  if (!idx || !obs || !target || !mean || !std || !x || !y) return fail(PGTT_E_ARG, "pgtt_learn_gather_rows: null pointer");
  if (B <= 0 || rows <= 0 || obs_dim <= 0 || tgt_dim <= 0) return fail(PGTT_E_ARG, "pgtt_learn_gather_rows: B, rows, obs_dim and tgt_dim must be positive");
  hipLaunchKernelGGL(gather_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, idx, obs, target, mean, std, rows, obs_dim, tgt_dim, x, y);
  return launched("pgtt_learn_gather_rows");
}

int pgtt_learn_sizeof_recurrent_act_args(void) { return (int)sizeof(PgttLearnRecurrentActArgs); }

int64_t pgtt_learn_recurrent_act_work_floats(int N, int od, int h1, int h2, int h3) {
  if (N <= 0 || od <= 0 || h1 <= 0 || h2 <= 0 || h3 <= 0) return 0;
  const int64_t hz = h1 > h2 ? (h1 > h3 ? h1 : h3) : (h2 > h3 ? h2 : h3);
  return (int64_t)N * ((int64_t)od + h1 + h2 + h3 + hz);
}

}  // extern "C"

namespace {

// both acting entries: every check, then the five launches; `s` given = the sampled tail
int recurrent_act(const PgttLearnRecurrentActArgs* a, const PgttLearnRecurrentSampleArgs* s, void* stream, const char* who) {
  if (!a->obs || !a->mean || !a->std || !a->w0 || !a->w1 || !a->w2 || !a->w3 || !a->b0 || !a->b1 || !a->b2 || !a->b3 || !a->w_ih || !a->w_hh ||
      !a->b_ih || !a->b_hh || !a->w_m || !a->mem || !a->action || !a->work)
    return fail(PGTT_E_ARG, std::string(who) + ": null pointer");
  if (a->num_envs <= 0 || a->obs_dim <= 0 || a->h1 <= 0 || a->h2 <= 0 || a->h3 <= 0)
    return fail(PGTT_E_ARG, std::string(who) + ": num_envs, obs_dim, h1, h2 and h3 must be positive");
  if (a->h3 % 16 != 0) return fail(PGTT_E_ARG, std::string(who) + ": h3 must be a multiple of 16");
  if (!memory_ok(a->memory)) return fail(PGTT_E_ARG, std::string(who) + ": memory must be a multiple of 16 in [16, 256]");
  const bool stores = a->store_obs || a->store_mem0 || a->store_clear;
  if (stores && (a->store_rows <= 0 || a->t < 0 || a->t >= a->store_rows))
    return fail(PGTT_E_ARG, std::string(who) + ": the storage row t must be in [0, store_rows)");
  if (s && (s->store_u || s->store_logp) && (a->store_rows <= 0 || a->t < 0 || a->t >= a->store_rows))
    return fail(PGTT_E_ARG, std::string(who) + ": the storage row t of store_u / store_logp must be in [0, store_rows)");
  hipStream_t st = (hipStream_t)stream;
  const long N = a->num_envs, od = a->obs_dim, R = a->memory;
  float* x = a->work;
  float* y1 = x + N * od;
  float* y2 = y1 + N * a->h1;
  float* y3 = y2 + N * a->h2;
  float* z = y3 + N * a->h3;                                  // the pre-activations: nobody reads them here
  const long row = (long)a->t * N;
  hipLaunchKernelGGL(normalise_kernel, dim3((unsigned)N), dim3(256), 0, st, a->obs, a->mean, a->std, (int)od, x,
                     a->store_obs ? a->store_obs + row * od : nullptr);
  int rc = pgtt_learn_linear_forward(x, a->w0, a->b0, (int)N, (int)od, a->h1, 1, y1, z, stream);
  if (rc == PGTT_OK) rc = pgtt_learn_linear_forward(y1, a->w1, a->b1, (int)N, a->h1, a->h2, 1, y2, z, stream);
  if (rc == PGTT_OK) rc = pgtt_learn_linear_forward(y2, a->w2, a->b2, (int)N, a->h2, a->h3, 1, y3, z, stream);
  if (rc != PGTT_OK) return rc;
  RecurrentK k{y3, a->w_ih, a->w_hh, a->b_ih, a->b_hh, a->w3, a->b3, a->w_m, a->done, a->clear_mask, a->mem, a->action, a->head,
               a->store_mem0 ? a->store_mem0 + row * R : nullptr, a->store_clear ? a->store_clear + row : nullptr,
               (int)N, a->h3, (int)R, a->clear_all, a->use_done};
  const dim3 grid((unsigned)((N + 15) / 16));
  const size_t lds = (size_t)(2 * 16 * (R + 4)) * sizeof(float);
  if (!s) {
    TailK<false> kd;
    static_cast<RecurrentK&>(kd) = k;
    hipLaunchKernelGGL(recurrent_tail_kernel<false>, grid, dim3(256), lds, st, kd);
  } else {
    TailK<true> ks;
    static_cast<RecurrentK&>(ks) = k;
    ks.s = SampleK{s->eps, s->counters, s->store_u ? s->store_u + row * kAct : nullptr, s->store_logp ? s->store_logp + row : nullptr,
                   (unsigned long long)s->seed, (long)s->env_id_offset, s->deterministic};
    hipLaunchKernelGGL(recurrent_tail_kernel<true>, grid, dim3(256), lds, st, ks);
  }
  return launched(who);
}

}  // namespace

extern "C" {

int pgtt_learn_sizeof_recurrent_sample_args(void) { return (int)sizeof(PgttLearnRecurrentSampleArgs); }

int pgtt_learn_recurrent_act(const PgttLearnRecurrentActArgs* a, void* stream) {
  if (!a) return fail(PGTT_E_ARG, "pgtt_learn_recurrent_act: null args");
  return recurrent_act(a, nullptr, stream, "pgtt_learn_recurrent_act");
}

int pgtt_learn_recurrent_act_sample(const PgttLearnRecurrentSampleArgs* s, void* stream) {
  if (!s) return fail(PGTT_E_ARG, "pgtt_learn_recurrent_act_sample: null args");
  return recurrent_act(&s->act, s, stream, "pgtt_learn_recurrent_act_sample");
}

int pgtt_learn_gru_clear_rows(const float* m, const uint8_t* clear, int B, int R, float* m0, void* stream) {
  if (!m || !clear || !m0) return fail(PGTT_E_ARG, "pgtt_learn_gru_clear_rows: null pointer");
  if (B <= 0) return fail(PGTT_E_ARG, "pgtt_learn_gru_clear_rows: B must be positive");
  if (!memory_ok(R)) return fail(PGTT_E_ARG, "pgtt_learn_gru_clear_rows: R must be a multiple of 16 in [16, 256]");
  const long n = (long)B * R;
  hipLaunchKernelGGL(gru_clear_rows_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, m, clear, n, R, m0);
  return launched("pgtt_learn_gru_clear_rows");
}

int pgtt_learn_gru_cell_forward(const float* gi, const float* gh, const float* m0, const uint8_t* clear_next, int B, int R, float* gates, float* m1,
                                float* m0_next, void* stream) {
  if (!gi || !gh || !m0 || !gates || !m1) return fail(PGTT_E_ARG, "pgtt_learn_gru_cell_forward: null pointer");
  if (B <= 0) return fail(PGTT_E_ARG, "pgtt_learn_gru_cell_forward: B must be positive");
  if (!memory_ok(R)) return fail(PGTT_E_ARG, "pgtt_learn_gru_cell_forward: R must be a multiple of 16 in [16, 256]");
  const long n = (long)B * R;
  hipLaunchKernelGGL(gru_cell_forward_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, gi, gh, m0, clear_next, n, R, gates, m1, m0_next);
  return launched("pgtt_learn_gru_cell_forward");
}

int pgtt_learn_gru_cell_backward(const float* gates, const float* gh, const float* m0, const float* dm1_head, const float* dm0_next,
                                 const uint8_t* clear_next, int B, int R, float* dgi, float* dgh, float* dm0_direct, void* stream) {
  if (!gates || !gh || !m0 || !dm1_head || !dgi || !dgh || !dm0_direct) return fail(PGTT_E_ARG, "pgtt_learn_gru_cell_backward: null pointer");
  if (B <= 0) return fail(PGTT_E_ARG, "pgtt_learn_gru_cell_backward: B must be positive");
  if (!memory_ok(R)) return fail(PGTT_E_ARG, "pgtt_learn_gru_cell_backward: R must be a multiple of 16 in [16, 256]");
  const long n = (long)B * R;
  hipLaunchKernelGGL(gru_cell_backward_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, gates, gh, m0, dm1_head, dm0_next, clear_next, n, R,
                     dgi, dgh, dm0_direct);
  return launched("pgtt_learn_gru_cell_backward");
}

int pgtt_learn_add_rows(const float* a, const float* b, int64_t n, float* out, void* stream) {
  if (!a || !b || !out) return fail(PGTT_E_ARG, "pgtt_learn_add_rows: null pointer");
  if (n <= 0) return fail(PGTT_E_ARG, "pgtt_learn_add_rows: n must be positive");
  hipLaunchKernelGGL(add_rows_kernel, dim3(blocks256((long)n)), dim3(256), 0, (hipStream_t)stream, a, b, (long)n, out);
  return launched("pgtt_learn_add_rows");
}

}  // extern "C"
