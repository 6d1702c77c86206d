// pgtt_perceive.hip — libpgtt_perceive.so: the student perception module (include/pgtt_perceive.h), two launches per call.
//
// perceive_trunk_kernel, one workgroup of four waves per env:
//   the depth image is preprocessed into LDS; the activations alternate between two LDS buffers and never go to HBM between layers.  A conv is
//   an implicit GEMM on v_mfma_f32_16x16x4_f32: M = a tile of 16 output channels, N = 16 output pixels, K = in_ch * k * k (zero-padded to a multiple
//   of 4).  A wave owns (pixel tile, channel tile) units, round robin.  Per MFMA a lane (i = lane & 15, g = lane >> 4) needs W[16 mt + i][4 ks + g],
//   one coalesced dword of the packed weights (they are the same for every env and stay in L2), and the input pixel of (k = 4 ks + g, pixel i): an LDS
//   read at `pixel base + offset of k`, the offsets of a layer's k in a small LDS table.  The pad k of the table points at the pixel's own base and meets a
//   zero weight.  The last conv writes `latent` ([C][H][W] order) straight from the accumulators.
// perceive_head_kernel, one workgroup of eight waves per 16 envs (pgtt_policy.hip's shape: the env is the MFMA's column):
//   z = [latent | obs[prop_rows]] is staged into LDS 256 k at a time, every wave keeps up to four 16-neuron tiles of the hidden layer in accumulators, so
//   the (F + n_prop) x hidden matrix is read once per 16 envs; then hidden -> 117 (eight tiles, one per wave), `est`, and the obs_out assembly.
// perceive_recurrent_head_kernel, the same shape (pgtt_perceive_recurrent): z -> hidden as above; the 16 envs' memory m0 is staged into sh_x (zeros for a
//   cleared env); wave w owns the 16-neuron tiles w and w + 8 of the memory and keeps four accumulator groups per tile - gi_r + gh_r and gi_u + gh_u
//   (one chain over hidden + R each), gi_n, gh_n - so with D[neuron = 16 tile + 4 g + r][env = i] the gates and the blend with m0 are lane-local;
//   m1 goes to `mem` and back into sh_x, then R -> 117 in eight tiles and the same assembly.  One fused launch: h and m1 never leave LDS.
// Nothing is shared between envs but the weights: a column of an MFMA does not see the other columns, so an env's rows do not depend on the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pgtt_perceive.h"
#include "pgtt_side_host.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTrunkLanes = 256;                  // four waves per env
constexpr int kTrunkWaves = kTrunkLanes / 64;
constexpr int kMaxK = PGTT_PERCEIVE_MAX_CH * 25;  // the deepest K: 64 input channels, 5 x 5
constexpr int kEnvs = 16;                         // envs per workgroup of the head = the N of the MFMA
constexpr int kHeadWaves = 8;
constexpr int kHeadLanes = 64 * kHeadWaves;
constexpr int kChunk = 256;                       // k staged per pass of the head
constexpr int kXS = kChunk + 4;                   // row strides: K + 4 floats, the sixteen 128-bit reads of a quarter-wave in sixteen bank quadruples
constexpr int kHS = PGTT_PERCEIVE_MAX_HIDDEN + 4;
constexpr int kOutPad = 128;                      // 117 scan rows in eight tiles
constexpr int kES = kOutPad + 4;
static_assert(kHeadWaves * 4 * 16 >= PGTT_PERCEIVE_MAX_HIDDEN && kHeadWaves * 16 == kOutPad && kOutPad >= PGTT_NSCAN, "tiles per wave");
static_assert(kEnvs * kES <= kEnvs * kXS, "the estimate reuses the staging buffer");
static_assert(PGTT_PERCEIVE_MAX_MEMORY + 4 <= kXS && 2 * kHeadWaves * 16 >= PGTT_PERCEIVE_MAX_MEMORY, "the memory reuses the staging buffer; two tiles per wave");
static_assert(kES <= kHS, "the recurrent estimate reuses the hidden buffer");

__device__ __forceinline__ float silu(float x) { return x / (1.0f + expf(-x)); }
// t = exp(-|x|) <= 1: no overflow at any x
__device__ __forceinline__ float sigmoidf(float x) { const float t = expf(-fabsf(x)), s = 1.0f / (1.0f + t); return x >= 0.f ? s : t * s; }
__device__ __forceinline__ float tanh_of(float x) { const float t = expf(-2.0f * fabsf(x)); return copysignf((1.0f - t) / (1.0f + t), x); }

struct ConvLayer { int cin, hin, win, cout, hout, wout, k, s, K, Kp; };

struct Net {                                      // what a config comes to
  ConvLayer L[PGTT_PERCEIVE_MAX_CONV];
  int n_conv, F, Kin, KB, off_b, lds_floats;      // KB = k-blocks of 16 of the first linear layer; off_b = start of the second LDS buffer, in floats
};

struct TrunkArgs {
  const float* depth;
  const float* w[PGTT_PERCEIVE_MAX_CONV];
  const float* b[PGTT_PERCEIVE_MAX_CONV];
  float* latent;
  ConvLayer L[PGTT_PERCEIVE_MAX_CONV];
  int n_conv, H, W, F, off_b;
  float near_m, far_m;
};

struct HeadArgs {
  const float* latent;
  const float* obs;
  const int32_t* prop;                            // [n_prop], device
  const float4* w1; const float* b1;
  const float4* w2; const float* b2;
  float* est;
  float* obs_out;
  int N, F, Kin, KB, hidden, obs_dim, scan_row0;
};

struct CellArgs {                                 // the recurrent head's own: PgttPerceiveMemory and the clear flags
  const float4* w_ih; const float4* w_hh; const float4* w_out;
  const float* b_ih; const float* b_hh; const float* b_out;
  const float* done;
  const uint8_t* clear_mask;
  float* mem;
  int R, clear_all, use_done;
};

__global__ void __launch_bounds__(kTrunkLanes) perceive_trunk_kernel(TrunkArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sh_act[];
  __shared__ unsigned short sh_koff[kMaxK];             // offsets of a layer's k inside its input: below 2^14 floats by the LDS budget
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  // ---- the image: clamp, scale to [-0.5, 0.5]; a NaN reads as far
  {
    const int npix = a.H * a.W;
    const float* src = a.depth + (size_t)e * npix;
    const float span = a.far_m - a.near_m;
    for (int p = tid; p < npix; p += kTrunkLanes) {
      float d = src[p];
      d = d != d ? a.far_m : d;
      sh_act[p] = (fminf(fmaxf(d, a.near_m), a.far_m) - a.near_m) / span - 0.5f;
    }
  }
  int in_off = 0, out_off = a.off_b;
#pragma unroll
  for (int l = 0; l < PGTT_PERCEIVE_MAX_CONV; l++) {
    if (l < a.n_conv) {
      const ConvLayer L = a.L[l];
      const int kk = L.k * L.k, plane = L.hin * L.win;
      for (int k = tid; k < L.Kp; k += kTrunkLanes) {
        int off = 0;
        if (k < L.K) {
          const int c = k / kk, r = k - c * kk, dy = r / L.k, dx = r - dy * L.k;
          off = c * plane + dy * L.win + dx;
        }
        sh_koff[k] = (unsigned short)off;
      }
      __syncthreads();                             // the table and the layer's input are in LDS
      const float* in = sh_act + in_off;
      float* out = sh_act + out_off;
      const int P = L.hout * L.wout, nmt = L.cout >> 4, units = ((P + 15) >> 4) * nmt, nks = L.Kp >> 2;
      const bool last = l == a.n_conv - 1;
      for (int u = wave; u < units; u += kTrunkWaves) {
        const int pt = u / nmt, mt = u - pt * nmt;
        const int p = 16 * pt + i, pc = min(p, P - 1);          // a lane past the last pixel computes the last pixel again and stores nothing
        const int oy = pc / L.wout, ox = pc - oy * L.wout;
        const float* px = in + oy * L.s * L.win + ox * L.s;
        const float* wl = a.w[l] + (size_t)mt * nks * 64 + lane;
        const unsigned short* ko = sh_koff + g;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < nks; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[ks * 64], px[ko[4 * ks]], acc, 0, 0, 0);
        if (p < P) {
          const int ch = 16 * mt + 4 * g;
          const float4 bv = *reinterpret_cast<const float4*>(a.b[l] + ch);
          const float v0 = silu(acc[0] + bv.x), v1 = silu(acc[1] + bv.y), v2 = silu(acc[2] + bv.z), v3 = silu(acc[3] + bv.w);
          if (last) {
            float* dst = a.latent + (size_t)e * a.F + (size_t)ch * P + p;
            dst[0] = v0; dst[P] = v1; dst[2 * P] = v2; dst[3 * P] = v3;
          } else {
            float* dst = out + ch * P + p;
            dst[0] = v0; dst[P] = v1; dst[2 * P] = v2; dst[3 * P] = v3;
          }
        }
      }
      __syncthreads();                             // the output is complete, the table free
      const int t = in_off; in_off = out_off; out_off = t;
    }
  }
}

// Its z -> hidden phase and its est / obs_out phase have twins below, hidden_layer() and emit() of the recurrent head: a fix to one is a fix to both.
__global__ void __launch_bounds__(kHeadLanes) perceive_head_kernel(HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float sh_x[kEnvs * kXS];        // the staged chunk of z; later the estimate [env][kES]
  __shared__ __attribute__((aligned(16))) float sh_h[kEnvs * kHS];        // the hidden layer
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int N = a.N, F = a.F, od = a.obs_dim, nt = a.hidden >> 4;
  const long e0 = (long)blockIdx.x * kEnvs;
  // ---- z -> hidden: tiles wave, wave + 8, wave + 16, wave + 24
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < a.KB; kc += kChunk / 16) {
    const int nkb = min(kChunk / 16, a.KB - kc);
    __syncthreads();                               // the chunk before this one has been consumed
    {
      const int env = tid >> 5, k0 = tid & 31;      // 32 lanes walk the k of one env
      const long e = e0 + env;
#pragma unroll
      for (int j = 0; j < kChunk / 32; j++) {
        const int k = k0 + 32 * j, gk = 16 * kc + k;
        float v = 0.f;
        if (e < N && k < 16 * nkb) {
          if (gk < F) v = a.latent[e * F + gk];
          else if (gk < a.Kin) v = a.obs[e * od + a.prop[gk - F]];
        }
        sh_x[env * kXS + k] = v;
      }
    }
    __syncthreads();
    const float* xrow = sh_x + i * kXS + 4 * g;
    for (int kb = 0; kb < nkb; kb++) {
      const float4 b = *reinterpret_cast<const float4*>(xrow + 16 * kb);
      float4 w[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int tile = wave + kHeadWaves * t;
        w[t] = tile < nt ? a.w1[((long)tile * a.KB + kc + kb) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      // consecutive MFMAs go to different accumulators
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t].x, b.x, acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t].y, b.y, acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t].z, b.z, acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t].w, b.w, acc[t], 0, 0, 0);
    }
  }
  // bias + SiLU, D[neuron = 16 tile + 4 g + r][env = i] -> sh_h[env][neuron]
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int tile = wave + kHeadWaves * t;
    if (tile < nt) {
      const int n = 16 * tile + 4 * g;
      const float4 bv = *reinterpret_cast<const float4*>(a.b1 + n);
      *reinterpret_cast<float4*>(sh_h + i * kHS + n) = make_float4(silu(acc[t][0] + bv.x), silu(acc[t][1] + bv.y), silu(acc[t][2] + bv.z), silu(acc[t][3] + bv.w));
    }
  }
  __syncthreads();                                 // the hidden layer is complete; sh_x is free
  // ---- hidden -> 117 (128): tile = wave
  {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    const float* hrow = sh_h + i * kHS + 4 * g;
    const float4* wl = a.w2 + (long)wave * nt * 64 + lane;
    for (int kb = 0; kb < nt; kb++) {
      const float4 b = *reinterpret_cast<const float4*>(hrow + 16 * kb);
      const float4 w = wl[kb * 64];
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, b.x, o, 0, 0, 0); o = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, b.y, o, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, b.z, o, 0, 0, 0); o = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, b.w, o, 0, 0, 0);
    }
    const int n = 16 * wave + 4 * g;
    const float4 bv = *reinterpret_cast<const float4*>(a.b2 + n);
    *reinterpret_cast<float4*>(sh_x + i * kES + n) = make_float4(o[0] + bv.x, o[1] + bv.y, o[2] + bv.z, o[3] + bv.w);
  }
  __syncthreads();
  // ---- est, and obs_out = obs with the scan rows replaced
  for (int idx = tid; idx < kEnvs * PGTT_NSCAN; idx += kHeadLanes) {
    const int env = idx / PGTT_NSCAN, j = idx - env * PGTT_NSCAN;
    if (e0 + env < N) a.est[(e0 + env) * PGTT_NSCAN + j] = sh_x[env * kES + j];
  }
  if (a.obs_out) {
    for (int idx = tid; idx < kEnvs * od; idx += kHeadLanes) {
      const int env = idx / od, k = idx - env * od, j = k - a.scan_row0;
      if (e0 + env < N) a.obs_out[(e0 + env) * od + k] = (j >= 0 && j < PGTT_NSCAN) ? sh_x[env * kES + j] : a.obs[(e0 + env) * od + k];
    }
  }
}

// The recurrent head.  Its first and last phases are perceive_head_kernel's, statement for statement; that kernel stays as it is so that pgtt_perceive()
// keeps its code object.
// z -> hidden of the 16 envs from e0 on, into sh_h[env][neuron]; sh_x is the staging buffer.  Ends before the barrier that completes sh_h.
__device__ __forceinline__ void hidden_layer(const HeadArgs& a, float* sh_x, float* sh_h, const long e0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int N = a.N, F = a.F, od = a.obs_dim, nt = a.hidden >> 4;
  // ---- z -> hidden: tiles wave, wave + 8, wave + 16, wave + 24
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < a.KB; kc += kChunk / 16) {
    const int nkb = min(kChunk / 16, a.KB - kc);
    __syncthreads();                               // the chunk before this one has been consumed
    {
      const int env = tid >> 5, k0 = tid & 31;      // 32 lanes walk the k of one env
      const long e = e0 + env;
#pragma unroll
      for (int j = 0; j < kChunk / 32; j++) {
        const int k = k0 + 32 * j, gk = 16 * kc + k;
        float v = 0.f;
        if (e < N && k < 16 * nkb) {
          if (gk < F) v = a.latent[e * F + gk];
          else if (gk < a.Kin) v = a.obs[e * od + a.prop[gk - F]];
        }
        sh_x[env * kXS + k] = v;
      }
    }
    __syncthreads();
    const float* xrow = sh_x + i * kXS + 4 * g;
    for (int kb = 0; kb < nkb; kb++) {
      const float4 b = *reinterpret_cast<const float4*>(xrow + 16 * kb);
      float4 w[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int tile = wave + kHeadWaves * t;
        w[t] = tile < nt ? a.w1[((long)tile * a.KB + kc + kb) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      // consecutive MFMAs go to different accumulators
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t].x, b.x, acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t].y, b.y, acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t].z, b.z, acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t].w, b.w, acc[t], 0, 0, 0);
    }
  }
  // bias + SiLU, D[neuron = 16 tile + 4 g + r][env = i] -> sh_h[env][neuron]
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int tile = wave + kHeadWaves * t;
    if (tile < nt) {
      const int n = 16 * tile + 4 * g;
      const float4 bv = *reinterpret_cast<const float4*>(a.b1 + n);
      *reinterpret_cast<float4*>(sh_h + i * kHS + n) = make_float4(silu(acc[t][0] + bv.x), silu(acc[t][1] + bv.y), silu(acc[t][2] + bv.z), silu(acc[t][3] + bv.w));
    }
  }
}

// est and obs_out of the 16 envs from e0 on, from the estimate sh_e[env][kES]
__device__ __forceinline__ void emit(const HeadArgs& a, const float* sh_e, const long e0) {
  const int tid = threadIdx.x, N = a.N, od = a.obs_dim;
  // ---- est, and obs_out = obs with the scan rows replaced
  for (int idx = tid; idx < kEnvs * PGTT_NSCAN; idx += kHeadLanes) {
    const int env = idx / PGTT_NSCAN, j = idx - env * PGTT_NSCAN;
    if (e0 + env < N) a.est[(e0 + env) * PGTT_NSCAN + j] = sh_e[env * kES + j];
  }
  if (a.obs_out) {
    for (int idx = tid; idx < kEnvs * od; idx += kHeadLanes) {
      const int env = idx / od, k = idx - env * od, j = k - a.scan_row0;
      if (e0 + env < N) a.obs_out[(e0 + env) * od + k] = (j >= 0 && j < PGTT_NSCAN) ? sh_e[env * kES + j] : a.obs[(e0 + env) * od + k];
    }
  }
}

// the GRU cell of NT neuron tiles per wave (tiles wave, wave + 8): m0 in sh_x[env][kXS], h in sh_h; m1 to `mem` and to sh_x.  Two barriers inside.
template <int NT>
__device__ __forceinline__ void gru_cell(const HeadArgs& a, const CellArgs& c, float* sh_x, const float* sh_h, const long e0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int R = c.R, nrt = R >> 4, nht = a.hidden >> 4;
  f32x4 acc[NT][4];                                // per tile: gi_r + gh_r, gi_u + gh_u, gi_n, gh_n
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int q = 0; q < 4; q++) acc[t][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  // W_ih h: the chains of r, u and gi_n.  Row tile of gate q and neuron tile `tile` is q * nrt + tile.
  {
    const float* hrow = sh_h + i * kHS + 4 * g;
    for (int kb = 0; kb < nht; kb++) {
      const float4 b = *reinterpret_cast<const float4*>(hrow + 16 * kb);
      float4 w[NT][3];
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int tile = wave + kHeadWaves * t;
#pragma unroll
        for (int q = 0; q < 3; q++) w[t][q] = tile < nrt ? c.w_ih[((long)(q * nrt + tile) * nht + kb) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 3; q++) acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][q].x, b.x, acc[t][q], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 3; q++) acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][q].y, b.y, acc[t][q], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 3; q++) acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][q].z, b.z, acc[t][q], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 3; q++) acc[t][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][q].w, b.w, acc[t][q], 0, 0, 0);
    }
  }
  // W_hh m0: r and u go on in their chains, gh_n is a chain of its own (accumulator 3)
  {
    const float* mrow = sh_x + i * kXS + 4 * g;
    for (int kb = 0; kb < nrt; kb++) {
      const float4 b = *reinterpret_cast<const float4*>(mrow + 16 * kb);
      float4 w[NT][3];
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int tile = wave + kHeadWaves * t;
#pragma unroll
        for (int q = 0; q < 3; q++) w[t][q] = tile < nrt ? c.w_hh[((long)(q * nrt + tile) * nrt + kb) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 3; q++) { const int d = q == 2 ? 3 : q; acc[t][d] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][q].x, b.x, acc[t][d], 0, 0, 0); }
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 3; q++) { const int d = q == 2 ? 3 : q; acc[t][d] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][q].y, b.y, acc[t][d], 0, 0, 0); }
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 3; q++) { const int d = q == 2 ? 3 : q; acc[t][d] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][q].z, b.z, acc[t][d], 0, 0, 0); }
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 3; q++) { const int d = q == 2 ? 3 : q; acc[t][d] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t][q].w, b.w, acc[t][d], 0, 0, 0); }
    }
  }
  // gates and blend, lane-local: this lane holds neurons 16 tile + 4 g + 0..3 of env i
  float4 m1[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int tile = wave + kHeadWaves * t;
    m1[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tile < nrt) {
      const int n = 16 * tile + 4 * g;
      const float4 m0 = *reinterpret_cast<const float4*>(sh_x + i * kXS + n);
      const float m0v[4] = {m0.x, m0.y, m0.z, m0.w};
      float out[4];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float gr = sigmoidf(acc[t][0][r] + c.b_ih[n + r] + c.b_hh[n + r]);
        const float gu = sigmoidf(acc[t][1][r] + c.b_ih[R + n + r] + c.b_hh[R + n + r]);
        const float gn = tanh_of((acc[t][2][r] + c.b_ih[2 * R + n + r]) + gr * (acc[t][3][r] + c.b_hh[2 * R + n + r]));
        out[r] = (1.0f - gu) * gn + gu * m0v[r];
      }
      m1[t] = make_float4(out[0], out[1], out[2], out[3]);
    }
  }
  __syncthreads();                                 // every wave has read m0 and h
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int tile = wave + kHeadWaves * t;
    if (tile < nrt) {
      const int n = 16 * tile + 4 * g;
      *reinterpret_cast<float4*>(sh_x + i * kXS + n) = m1[t];
      if (e0 + i < a.N) {
        float* dst = c.mem + (e0 + i) * R + n;      // dwords: `mem` need not be 16-byte aligned
        dst[0] = m1[t].x; dst[1] = m1[t].y; dst[2] = m1[t].z; dst[3] = m1[t].w;
      }
    }
  }
  __syncthreads();                                 // m1 is complete in sh_x
}

__global__ void __launch_bounds__(kHeadLanes) perceive_recurrent_head_kernel(HeadArgs a, CellArgs c) {
  __shared__ __attribute__((aligned(16))) float sh_x[kEnvs * kXS];        // the staged chunk of z; then m0, then m1 [env][kXS]
  __shared__ __attribute__((aligned(16))) float sh_h[kEnvs * kHS];        // the hidden layer; later the estimate [env][kES]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
  const int R = c.R, nrt = R >> 4;
  const long e0 = (long)blockIdx.x * kEnvs;
  hidden_layer(a, sh_x, sh_h, e0);
  __syncthreads();                                 // the hidden layer is complete; sh_x is free
  // ---- m0: zeros for a cleared env and for an env past N
  {
    const int env = tid >> 5, k0 = tid & 31;
    const long e = e0 + env;
    bool live = e < a.N && !c.clear_all;
    if (live && c.clear_mask) live = c.clear_mask[e] == 0;
    if (live && c.use_done && c.done) live = c.done[e] == 0.f;
    for (int k = k0; k < R; k += 32) sh_x[env * kXS + k] = live ? c.mem[e * R + k] : 0.f;
  }
  __syncthreads();
  if (nrt > kHeadWaves) gru_cell<2>(a, c, sh_x, sh_h, e0);
  else gru_cell<1>(a, c, sh_x, sh_h, e0);
  // ---- memory -> 117 (128): tile = wave; the estimate goes where the hidden layer was (gru_cell's first barrier freed it)
  {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    const float* mrow = sh_x + i * kXS + 4 * g;
    const float4* wl = c.w_out + (long)wave * nrt * 64 + lane;
    for (int kb = 0; kb < nrt; kb++) {
      const float4 b = *reinterpret_cast<const float4*>(mrow + 16 * kb);
      const float4 w = wl[kb * 64];
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, b.x, o, 0, 0, 0); o = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, b.y, o, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, b.z, o, 0, 0, 0); o = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, b.w, o, 0, 0, 0);
    }
    const int n = 16 * wave + 4 * g;
    const float4 bv = *reinterpret_cast<const float4*>(c.b_out + n);
    *reinterpret_cast<float4*>(sh_h + i * kES + n) = make_float4(o[0] + bv.x, o[1] + bv.y, o[2] + bv.z, o[3] + bv.w);
  }
  __syncthreads();
  emit(a, sh_h, e0);
}

// the config's checks and what it comes to; `who` prefixes the message
int resolve(const PgttPerceiveConfig* c, Net* net, const char* who) {
  const std::string p = std::string(who) + ": ";
  if (!c) return fail(PGTT_E_ARG, p + "null config");
  if (c->height < 1 || c->height > PGTT_PERCEIVE_MAX_DIM || c->width < 1 || c->width > PGTT_PERCEIVE_MAX_DIM)
    return fail(PGTT_E_ARG, p + "height and width must be in [1, PGTT_PERCEIVE_MAX_DIM]");
  if (!(c->near < c->far) || !std::isfinite(c->near) || !std::isfinite(c->far)) return fail(PGTT_E_ARG, p + "need near < far, finite");
  if (c->n_conv < 1 || c->n_conv > PGTT_PERCEIVE_MAX_CONV) return fail(PGTT_E_ARG, p + "n_conv must be in [1, 3]");
  if (c->hidden < 16 || c->hidden > PGTT_PERCEIVE_MAX_HIDDEN || c->hidden % 16) return fail(PGTT_E_ARG, p + "hidden must be a multiple of 16 in [16, 512]");
  if (c->obs_dim < 1 || c->scan_row0 < 0 || (long)c->scan_row0 + PGTT_NSCAN > c->obs_dim) return fail(PGTT_E_ARG, p + "need 0 <= scan_row0 and scan_row0 + 117 <= obs_dim");
  if (c->n_prop < 0 || c->n_prop > PGTT_PERCEIVE_MAX_PROP) return fail(PGTT_E_ARG, p + "n_prop must be in [0, 64]");
  for (int j = 0; j < c->n_prop; j++)
    if (c->prop_rows[j] < 0 || c->prop_rows[j] >= c->obs_dim) return fail(PGTT_E_ARG, p + "prop_rows entry outside [0, obs_dim)");
  Net n{};
  n.n_conv = c->n_conv;
  int cin = 1, hin = c->height, win = c->width;
  long act[PGTT_PERCEIVE_MAX_CONV + 1] = {(long)hin * win, 0, 0, 0};
  for (int l = 0; l < c->n_conv; l++) {
    const int co = c->out_ch[l], k = c->kernel[l], s = c->stride[l];
    if (co < 16 || co > PGTT_PERCEIVE_MAX_CH || co % 16) return fail(PGTT_E_ARG, p + "out_ch must be a multiple of 16 in [16, 64]");
    if (k != 3 && k != 5) return fail(PGTT_E_ARG, p + "kernel must be 3 or 5");
    if (s != 1 && s != 2) return fail(PGTT_E_ARG, p + "stride must be 1 or 2");
    if (hin < k || win < k) return fail(PGTT_E_ARG, p + "a conv layer's output would be empty");
    ConvLayer& L = n.L[l];
    L.cin = cin; L.hin = hin; L.win = win; L.cout = co; L.k = k; L.s = s;
    L.hout = (hin - k) / s + 1; L.wout = (win - k) / s + 1;
    L.K = cin * k * k; L.Kp = (L.K + 3) & ~3;
    cin = co; hin = L.hout; win = L.wout;
    act[l + 1] = (long)co * hin * win;
  }
  n.F = (int)act[c->n_conv];
  act[c->n_conv] = 0;                              // the last conv's output goes to `latent`
  const long a02 = act[0] > act[2] ? act[0] : act[2];
  if (4 * (a02 + act[1]) > PGTT_PERCEIVE_LDS_BYTES) return fail(PGTT_E_ARG, p + "the activations do not fit the LDS budget (pgtt_perceive.h)");
  n.off_b = (int)((a02 + 3) & ~3L);
  n.lds_floats = n.off_b + (int)act[1];
  n.Kin = n.F + c->n_prop;
  n.KB = (n.Kin + 15) >> 4;
  if (net) *net = n;
  return PGTT_OK;
}

int check_memory(int memory, const char* who) {
  if (memory < 16 || memory > PGTT_PERCEIVE_MAX_MEMORY || memory % 16) return fail(PGTT_E_ARG, std::string(who) + ": memory must be a multiple of 16 in [16, 256]");
  return PGTT_OK;
}

}  // namespace

struct pgtt_perceive_net {
  int device = 0, num_envs = 0;
  PgttPerceiveConfig cfg{};
  Net net{};
  PgttPerceiveBuffers buf{};
  bool bound = false;
  int32_t* d_prop = nullptr;
  PgttPerceiveMemory mem{};                        // the recurrent form; has_mem after pgtt_perceive_set_memory
  bool has_mem = false;
};

extern "C" {

PGTT_SIDE_EXPORTS(perceive, PERCEIVE)
int pgtt_perceive_sizeof_config(void) { return (int)sizeof(PgttPerceiveConfig); }
int pgtt_perceive_sizeof_buffers(void) { return (int)sizeof(PgttPerceiveBuffers); }
int pgtt_perceive_sizeof_memory(void) { return (int)sizeof(PgttPerceiveMemory); }

int pgtt_perceive_check(const PgttPerceiveConfig* cfg) { return resolve(cfg, nullptr, "pgtt_perceive_check"); }

int pgtt_perceive_latent_dim(const PgttPerceiveConfig* cfg) {
  Net n;
  if (int rc = resolve(cfg, &n, "pgtt_perceive_latent_dim")) return rc;
  return n.F;
}

int pgtt_perceive_packed_floats(const PgttPerceiveConfig* cfg, int layer) {
  Net n;
  if (int rc = resolve(cfg, &n, "pgtt_perceive_packed_floats")) return rc;
  if (layer < 0 || layer >= PGTT_PERCEIVE_NLAYER) return fail(PGTT_E_ARG, "pgtt_perceive_packed_floats: layer must be in [0, 5)");
  if (layer < PGTT_PERCEIVE_MAX_CONV) return layer < n.n_conv ? n.L[layer].cout * n.L[layer].Kp : 0;
  if (layer == 3) return cfg->hidden * n.KB * 16;
  return kOutPad * cfg->hidden;
}

int pgtt_perceive_create(const PgttPerceiveConfig* cfg, int device, int num_envs, pgtt_perceive_handle* out) {
  if (!cfg || !out) return fail(PGTT_E_ARG, "pgtt_perceive_create: null argument");
  *out = nullptr;
  if (num_envs < 1) return fail(PGTT_E_ARG, "pgtt_perceive_create: num_envs must be >= 1");
  Net n;
  if (int rc = resolve(cfg, &n, "pgtt_perceive_create")) return rc;
  if (int rc = check_device(device, "pgtt_perceive_create")) return rc;
  pgtt_perceive_net* h = new pgtt_perceive_net();
  h->device = device; h->num_envs = num_envs; h->cfg = *cfg; h->net = n;
  auto upload = [&]() -> int {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(&h->d_prop, PGTT_PERCEIVE_MAX_PROP * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(h->d_prop, cfg->prop_rows, PGTT_PERCEIVE_MAX_PROP * sizeof(int32_t), hipMemcpyHostToDevice));
    return PGTT_OK;
  };
  if (int rc = upload()) { pgtt_perceive_destroy(h); return rc; }
  *out = h;
  return PGTT_OK;
}

int pgtt_perceive_destroy(pgtt_perceive_handle h) {
  if (!h) return PGTT_OK;
  if (h->d_prop) { hipSetDevice(h->device); hipFree(h->d_prop); }
  delete h;
  return PGTT_OK;
}

int pgtt_perceive_bind(pgtt_perceive_handle h, const PgttPerceiveBuffers* bufs) {
  if (!h || !bufs) return fail(PGTT_E_ARG, "pgtt_perceive_bind: null argument");
  if (!bufs->depth || !bufs->obs || !bufs->latent || !bufs->est) return fail(PGTT_E_ARG, "pgtt_perceive_bind: depth, obs, latent and est are required");
  for (int l = 0; l < PGTT_PERCEIVE_NLAYER; l++)
    if ((l >= PGTT_PERCEIVE_MAX_CONV || l < h->cfg.n_conv) && (!bufs->w[l] || !bufs->b[l]))
      return fail(PGTT_E_ARG, "pgtt_perceive_bind: the weights and biases of every layer of the net are required");
  h->buf = *bufs;
  h->bound = true;
  return PGTT_OK;
}

// the arguments of the two launches from what is bound
static void launch_args(const pgtt_perceive_net* h, TrunkArgs* tp, HeadArgs* ap) {
  const PgttPerceiveConfig& c = h->cfg;
  const Net& n = h->net;
  TrunkArgs t{};
  t.depth = h->buf.depth; t.latent = h->buf.latent;
  for (int l = 0; l < PGTT_PERCEIVE_MAX_CONV; l++) { t.w[l] = h->buf.w[l]; t.b[l] = h->buf.b[l]; t.L[l] = n.L[l]; }
  t.n_conv = n.n_conv; t.H = c.height; t.W = c.width; t.F = n.F; t.off_b = n.off_b; t.near_m = c.near; t.far_m = c.far;
  HeadArgs a{};
  a.latent = h->buf.latent; a.obs = h->buf.obs; a.prop = h->d_prop;
  a.w1 = reinterpret_cast<const float4*>(h->buf.w[3]); a.b1 = h->buf.b[3];
  a.w2 = reinterpret_cast<const float4*>(h->buf.w[4]); a.b2 = h->buf.b[4];
  a.est = h->buf.est; a.obs_out = h->buf.obs_out;
  a.N = h->num_envs; a.F = n.F; a.Kin = n.Kin; a.KB = n.KB; a.hidden = c.hidden; a.obs_dim = c.obs_dim; a.scan_row0 = c.scan_row0;
  *tp = t; *ap = a;
}

int pgtt_perceive(pgtt_perceive_handle h, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_perceive: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_perceive: no buffers bound (pgtt_perceive_bind first)");
  HIP_TRY(hipSetDevice(h->device));
  TrunkArgs t; HeadArgs a;
  launch_args(h, &t, &a);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(perceive_trunk_kernel, dim3(h->num_envs), dim3(kTrunkLanes), (size_t)h->net.lds_floats * sizeof(float), st, t);
  hipLaunchKernelGGL(perceive_head_kernel, dim3((h->num_envs + kEnvs - 1) / kEnvs), dim3(kHeadLanes), 0, st, a);
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

int pgtt_perceive_memory_check(const PgttPerceiveConfig* cfg, int memory) {
  if (int rc = resolve(cfg, nullptr, "pgtt_perceive_memory_check")) return rc;
  return check_memory(memory, "pgtt_perceive_memory_check");
}

int pgtt_perceive_memory_packed_floats(const PgttPerceiveConfig* cfg, int memory, int which) {
  if (int rc = resolve(cfg, nullptr, "pgtt_perceive_memory_packed_floats")) return rc;
  if (int rc = check_memory(memory, "pgtt_perceive_memory_packed_floats")) return rc;
  if (which == 0) return 3 * memory * cfg->hidden;
  if (which == 1) return 3 * memory * memory;
  if (which == 2) return kOutPad * memory;
  return fail(PGTT_E_ARG, "pgtt_perceive_memory_packed_floats: which must be 0 (w_ih), 1 (w_hh) or 2 (w_out)");
}

int pgtt_perceive_set_memory(pgtt_perceive_handle h, const PgttPerceiveMemory* m) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_perceive_set_memory: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_perceive_set_memory: no buffers bound (pgtt_perceive_bind first)");
  if (!m) { h->mem = PgttPerceiveMemory{}; h->has_mem = false; return PGTT_OK; }
  if (int rc = check_memory(m->memory, "pgtt_perceive_set_memory")) return rc;
  if (!m->w_ih || !m->w_hh || !m->w_out || !m->b_ih || !m->b_hh || !m->b_out || !m->mem)
    return fail(PGTT_E_ARG, "pgtt_perceive_set_memory: w_ih, w_hh, w_out, b_ih, b_hh, b_out and mem are required");
  for (const float* p : {m->w_ih, m->w_hh, m->w_out, m->b_out})      // read as float4
    if (reinterpret_cast<uintptr_t>(p) % 16) return fail(PGTT_E_ARG, "pgtt_perceive_set_memory: w_ih, w_hh, w_out and b_out must be 16-byte aligned");
  h->mem = *m;
  h->has_mem = true;
  return PGTT_OK;
}

int pgtt_perceive_recurrent(pgtt_perceive_handle h, const uint8_t* clear_mask, int clear_all, int use_done, void* stream) {
  if (!h) return fail(PGTT_E_ARG, "pgtt_perceive_recurrent: null handle");
  if (!h->bound) return fail(PGTT_E_STATE, "pgtt_perceive_recurrent: no buffers bound (pgtt_perceive_bind first)");
  if (!h->has_mem) return fail(PGTT_E_STATE, "pgtt_perceive_recurrent: no memory set (pgtt_perceive_set_memory first)");
  HIP_TRY(hipSetDevice(h->device));
  TrunkArgs t; HeadArgs a;
  launch_args(h, &t, &a);
  const PgttPerceiveMemory& m = h->mem;
  CellArgs c{};
  c.w_ih = reinterpret_cast<const float4*>(m.w_ih); c.w_hh = reinterpret_cast<const float4*>(m.w_hh); c.w_out = reinterpret_cast<const float4*>(m.w_out);
  c.b_ih = m.b_ih; c.b_hh = m.b_hh; c.b_out = m.b_out; c.done = m.done; c.clear_mask = clear_mask; c.mem = m.mem;
  c.R = m.memory; c.clear_all = clear_all != 0; c.use_done = use_done != 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(perceive_trunk_kernel, dim3(h->num_envs), dim3(kTrunkLanes), (size_t)h->net.lds_floats * sizeof(float), st, t);
  hipLaunchKernelGGL(perceive_recurrent_head_kernel, dim3((h->num_envs + kEnvs - 1) / kEnvs), dim3(kHeadLanes), 0, st, a, c);
  HIP_TRY(hipGetLastError());
  return PGTT_OK;
}

}  // extern "C"
