// Weight rows of ResizeRight's separable cubic resize (antialiased, pad_mode='constant') for an extent n resized to m, with exact integer
// geometry: the routines csrc/cutresize.hip (cutouts) and csrc/ilvr.hip (low-pass refinement) build their LDS weight rows with, and the
// host entry cgd_resize_weights.  The geometry is stated at the head of cutresize.hip.
#pragma once

__host__ __device__ inline long floor_div(long a, long b) {  // b > 0
  const long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ inline long ceil_div(long a, long b) { return -floor_div(-a, b); }  // b > 0

// number of taps of an n -> m resize
__host__ __device__ inline int resize_taps(int n, int m) { return m >= n ? 4 : (int)ceil_div(4L * n, m); }

// cubic(d) in product form (no cancellation between large terms): (|d|-1)(1.5 d^2 - |d| - 1) on [0,1], 0.5 t^2 (t-1), t = 2-|d|, on (1,2]
__host__ __device__ inline float resize_cubic(float d) {
#pragma clang fp contract(off)
  const float a = d < 0.f ? -d : d;
  if (a <= 1.f) return (a - 1.f) * ((1.5f * a - 1.f) * a - 1.f);
  if (a <= 2.f) {
    const float t = 2.f - a;
    return 0.5f * t * t * (t - 1.f);
  }
  return 0.f;
}

// first tap of output o; the tap distances c_o - j are (num - 2 m j) / (2m) with num = (2o+1) n - m
__host__ __device__ inline int resize_left(int n, int m, int o) {
  const long num = (2L * o + 1) * n - m;
  return (int)ceil_div(num - 4L * (m >= n ? m : n), 2L * m);
}

// un-normalised kernel value of tap j of output o (the factor s of the antialiasing kernel cancels in the normalisation)
__host__ __device__ inline float resize_k(int n, int m, int o, int j) {
#pragma clang fp contract(off)
  const long numer = (2L * o + 1) * n - m - 2L * m * j;
  return resize_cubic((float)numer / (float)(2L * (m >= n ? m : n)));  // d for s >= 1, s d = numer / (2n) for s < 1
}

// weights of output o into w[0 .. T-1] (stride 1), returns left_o.  T = resize_taps(n, m)
__host__ __device__ inline int resize_row(int n, int m, int o, int T, float* w) {
#pragma clang fp contract(off)
  const int left = resize_left(n, m, o);
  float sum = 0.f;
  for (int t = 0; t < T; ++t) {
    const float k = resize_k(n, m, o, left + t);
    w[t] = k;
    sum += k;
  }
  const float inv = 1.f / (sum == 0.f ? 1.f : sum);
  for (int t = 0; t < T; ++t) w[t] *= inv;
  return left;
}

// outputs o of an n -> m resize whose taps include input x: [lo, hi] clamped to [0, m-1] (left_o is non-decreasing in o)
__device__ inline void resize_inverse_range(int n, int m, int T, int x, int& lo, int& hi) {
  const long K = 4L * (m >= n ? m : n);
  // left_o <= x              <=>  (2o+1) n <= 2 m x + m + K
  const long q_hi = floor_div(2L * m * x + m + K, n);
  // left_o + T - 1 >= x      <=>  (2o+1) n >  2 m (x - T) + m + K
  const long q_lo = floor_div(2L * m * (x - T) + m + K, n) + 1;
  const long h_ = floor_div(q_hi - 1, 2), l_ = floor_div(q_lo, 2);
  hi = (int)(h_ < m - 1 ? h_ : m - 1);
  lo = (int)(l_ > 0 ? l_ : 0);
}
