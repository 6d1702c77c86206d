// pgtt_raycast.hip.h — the device-side algebra that libpgtt_render.so (pgtt_render.hip), libpgtt_depth.so (pgtt_depth.hip) and libpgtt_lidar.so
// (pgtt_lidar.hip) share: V3 / Q4, qmul, qaxes, qrot(q, v).  The host side of the same three libraries is pgtt_raycast_host.h.
// NOT here, although the kernels state them: the forward kinematics of the body chain (the formulas of mjcf.kinematics_np), the placement of
// a PgttRenderGeom on its body, and the sphere / capsule tests.  Moved into shared helpers with their expressions unchanged, they make the
// compiler pair and contract the fp32 products of the kernels differently.  Measured on an MI355X against the build before: a shared chain
// moved body poses by one ulp (6e-8) and with them 0.2 % of the renderer's and 10 % of a thigh-mounted depth camera's pixels
// (profiles/r10_ab_raycast_chain.txt); a shared placement and shared hit tests, the depth camera calling the renderer's forms with the ray
// origin at zero, moved 1.5 % of the pixels of a thigh-mounted camera that sees the robot by up to 7e-6 m (profiles/r10_ab_raycast_hits.txt).
// So each kernel keeps its own statement of these (the LiDAR's, the third, likewise), and tests/test_gpu_render.py, tests/test_gpu_depth.py and
// tests/test_gpu_lidar.py hold them against fp64 references on whole scenes; tests/test_gpu_raycast_edges.py holds hit_box, hit_sphere and
// hit_capsule to fp64 at their edges, on crafted cases.
// What the three statements of hit_capsule have in common (pa, ba = the segment's start and vector, oa = origin - pa, |d| = 1):
//   the cylinder's quadratic a t^2 + 2 b t + cc = 0 in its cross-product form (Lagrange's identity),
//     a = baba - bard^2 = |ba x d|^2,   b = baba rdoa - baoa bard = (ba x d).(ba x oa),   cc = baba oaoa - baoa^2 - r^2 baba = |ba x oa|^2 - r^2 baba.
//   The dot-product form cancels to rounding noise for a ray within 1e-3 rad of the axis (misses, and hits 2 hl too deep); this one does not.
//   a <= 1e-12 baba, i.e. the ray within 1e-6 rad of the axis: the ray drifts less than 1e-6 of the capsule's length off the axis over it and
//   can only meet a cap, so both caps are tried.  Below that scale a is rounding noise: a component of ba x d carries an error of about
//   6e-8 |ba| (one rounded product), which gives an a of about 1e-14 baba for a ray exactly along the axis, so the threshold has a margin of 100.
//   It is decided BEFORE h = b^2 - a cc is looked at: the compiler may form ba x d twice, contracted differently, and multiply the two, so
//   that an a at noise level, and with it h, comes out negative for a ray that meets the capsule.
// The two onboard sensors, depth_kernel and lidar_kernel, are one shape, and what they state in common was tried piece by piece with hipcc for gfx950
// and tools/side_isa_diff.py against the build before:
//   moved into a shared header, text unchanged                              device code of depth_kernel<*>, lidar_kernel<*>
//   Philox, hit_sphere, hit_capsule, the counter's advance kernel           identical, all four
//   + the noise tail as a function                                          <false> identical; <true> one s_nop fewer and one select in its short
//                                                                           encoding, every other opcode count equal; every buffer bit-identical
//                                                                           on an MI355X (profiles/r34_ab_raycast.txt)
//   + the body chain as a function (the args by reference, or plain         all four differ: 18 fewer fused multiply-adds, a 12-byte load split in
//     pointers and scalars)                                                 two - bits would move
//   + the placement of boxes and geoms with the compaction                  all four differ: another mix of packed fma / mul / add - bits would move
// What was a __device__ function already moves freely; what stands inline in a kernel does not.  So pgtt_sensor.hip.h is the home of the pair's
// common tests (hit_sphere, hit_capsule: the ray from the origin, a unit d), of the noise tail and of their common host code, and the chain, the
// placement, hit_box (whose two forms differ on purpose), the culls and the loops keep their text in both kernels.
// Included by those three translation units only (the sensors' through pgtt_sensor.hip.h).  It does not include pgtt_common.hip.h (whose qrot(v, q)
// is the physics kernels' form): that file is inside the physics source hash (srchash.py), and this one is inside the three side hashes only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pgtt_render.h"

namespace {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 ld3(const float* p) { return {p[0], p[1], p[2]}; }

struct Q4 { float w, x, y, z; };
__device__ __forceinline__ Q4 qmul(Q4 a, Q4 b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
// columns of the rotation matrix of q: the frame's local axes in the parent's coordinates
__device__ __forceinline__ void qaxes(Q4 q, V3& c0, V3& c1, V3& c2) {
  const float w = q.w, x = q.x, y = q.y, z = q.z;
  c0 = v3(w * w + x * x - y * y - z * z, 2.f * (x * y + w * z), 2.f * (x * z - w * y));
  c1 = v3(2.f * (x * y - w * z), w * w - x * x + y * y - z * z, 2.f * (y * z + w * x));
  c2 = v3(2.f * (x * z + w * y), 2.f * (y * z - w * x), w * w - x * x - y * y + z * z);
}
__device__ __forceinline__ V3 qrot(Q4 q, V3 v) {
  V3 c0, c1, c2; qaxes(q, c0, c1, c2);
  return v.x * c0 + v.y * c1 + v.z * c2;
}

}  // namespace
