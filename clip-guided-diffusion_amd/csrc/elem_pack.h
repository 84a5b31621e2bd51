// Shared by the elementwise per-plane kernels (dpm.hip, mask.hip, invert.hip; threshold.hip uses load / store / aligned16): a plane is walked
// in units of V floats, V = 4 (one 16-byte access; needs HW % 4 == 0 and 16-byte aligned pointers, so that a unit never straddles two
// planes) or V = 1 (any 4-byte aligned pointer, any HW).  plane_walk is the host side of the walk (V and the grid); the kernels keep the
// device side, two explicit loops (planes, then units): lambda-taking helpers changed their machine code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace elem_pack {

template <int V>
struct Pack;
template <>
struct Pack<1> {
  typedef float type;
};
template <>
struct Pack<4> {
  typedef float4 type;
};

template <int V>
__device__ __forceinline__ void load(const float* p, float (&v)[V]) {
  const typename Pack<V>::type t = *reinterpret_cast<const typename Pack<V>::type*>(p);
  const float* f = reinterpret_cast<const float*>(&t);
#pragma unroll
  for (int e = 0; e < V; ++e) v[e] = f[e];
}

template <int V>
__device__ __forceinline__ void store(float* p, const float (&v)[V]) {
  typename Pack<V>::type t;
  float* f = reinterpret_cast<float*>(&t);
#pragma unroll
  for (int e = 0; e < V; ++e) f[e] = v[e];
  *reinterpret_cast<typename Pack<V>::type*>(p) = t;
}

// a null pointer (an optional buffer that is absent) counts as aligned
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Host side: V = 4 when HW % 4 == 0 and every pointer of `ptrs` is 16-byte aligned, else 1; grid.x covers a plane's units (256 per
// workgroup, at most 1024 workgroups), grid.y the planes (at most 65535).  Calls launch(std::integral_constant<int, V>, grid).
template <class Launch, class... P>
inline void plane_walk(int HW, int planes, Launch&& launch, const P*... ptrs) {
  const bool vec = HW % 4 == 0 && (aligned16(ptrs) && ...);
  const dim3 grid(std::min(cdiv(vec ? HW / 4 : HW, 256), 1024), std::min(planes, 65535));
  if (vec)
    launch(std::integral_constant<int, 4>(), grid);
  else
    launch(std::integral_constant<int, 1>(), grid);
}

}  // namespace elem_pack
