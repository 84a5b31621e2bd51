// What the resampling kernels of the animation modes share (warp.hip: the affine 2D warp; warp3d.hip: the perspective warp by a depth map):
// the border rule of one tap index and the Keys cubic weights, so that the two kernels bring a tap into the frame and weigh it in the same way,
// to the bit.
#pragma once
#include <hip/hip_runtime.h>

constexpr int WARP_THREADS = 256;
constexpr double WARP_MAX_COORD = 1073741824.0;  // 2^30: floor - 1 .. floor + 2 of anything inside stays an int

// border rule of one tap index (|i| <= 2^30 + 2) on an extent n (1 <= n < 2^31)
template <int BORDER>
__device__ __forceinline__ int warp_index(int i, int n) {
  if (BORDER == 2) return i < 0 ? 0 : (i >= n ? n - 1 : i);
  if ((unsigned)i < (unsigned)n) return i;  // inside: the common case
  if (BORDER == 0) {
    const unsigned un = (unsigned)n;
    if (i >= 0) return (int)((unsigned)i % un);
    const unsigned r = (0u - (unsigned)i) % un;
    return r ? (int)(un - r) : 0;
  }
  if (n == 1) return 0;
  const unsigned p = 2u * (unsigned)(n - 1);  // < 2^32
  unsigned r = (i >= 0 ? (unsigned)i : 0u - (unsigned)i) % p;  // the reflection is even about 0
  if (r >= (unsigned)n) r = p - r;
  return (int)r;
}

// Keys cubic weights (a = -0.75) of the taps at distances t + 1, t, 1 - t, 2 - t; exactly (0, 1, 0, 0) at t = 0
__device__ __forceinline__ void cubic_weights(float t, float& w0, float& w1, float& w2, float& w3) {
  const float A = -0.75f;
  const float u = 1.f - t, t1 = t + 1.f, u1 = u + 1.f;
  w0 = ((A * t1 - 5.f * A) * t1 + 8.f * A) * t1 - 4.f * A;
  w1 = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w2 = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w3 = ((A * u1 - 5.f * A) * u1 + 8.f * A) * u1 - 4.f * A;
}
