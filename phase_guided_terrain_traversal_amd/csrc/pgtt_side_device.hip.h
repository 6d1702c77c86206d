// pgtt_side_device.hip.h — the device-side counterpart of pgtt_side_host.h: what the kernels of several side libraries state in common.  Today that
// is the env's generator alone.  Included by pgtt_depth.hip and pgtt_lidar.hip (through pgtt_sensor.hip.h), pgtt_elevation.hip and pgtt_learn.hip,
// and listed for those four in srchash.SIDE_SOURCES; the renderer and the student perception kernels draw nothing and do not include it.
// Two more statements of Philox stand outside the side libraries and stay: pgtt_common.hip.h's, which is inside the physics source hash, and
// pgtt_policy.hip's, which is `inline`, not __forceinline__, and part of libpgtt.so, whose device code tools/side_isa_diff.py cannot compare.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// Philox4x32-10, the env's generator (pgtt.h)
__device__ __forceinline__ void philox4x32_10(unsigned k0, unsigned k1, unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    const unsigned n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
    c0 = n0; c1 = l1; c2 = n2; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

}  // namespace
