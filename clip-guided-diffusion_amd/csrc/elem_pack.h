// Shared by the elementwise per-plane kernels (mask.hip, invert.hip): a plane is walked in units of V floats, V = 4 (one 16-byte access; needs
// HW % 4 == 0 and 16-byte aligned pointers, so that a unit never straddles two planes) or V = 1 (any 4-byte aligned pointer, any HW).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

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

}  // namespace elem_pack
