// Device-side staging primitives of the MFMA kernels (gfx950 only): the vector types, the bf16 hi / lo splits, buffer loads, non-temporal accesses, the
// fused GroupNorm + SiLU and the timeline stamps, each defined once.  Internal header for the kernel files; the host-only translation units
// (unet, vit, text; net.h, kernels.h, common.h) do not include it.  Everything here is force-inlined: the kernels are sensitive to the form of these
// helpers (hconv.hip, SPLITQ), so a change here is checked with benchmarks/isa_diff.py against the build before it.
#pragma once
#include <hip/hip_runtime.h>

typedef float cgd_f32x2 __attribute__((ext_vector_type(2)));
typedef float cgd_f32x4 __attribute__((ext_vector_type(4)));  // native vector: value selects stay in registers
typedef float cgd_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 cgd_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 cgd_bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 cgd_bf16x8 __attribute__((ext_vector_type(8)));
typedef int cgd_i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned cgd_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned cgd_u32x4 __attribute__((ext_vector_type(4)));

// ---- bf16 hi / lo split --------------------------------------------------------------------------------------------------------------------------
// element-wise: hi = bf16(v), residual = v - float(hi) (its bf16 is the lo operand of the bf16x3 products)
__device__ __forceinline__ cgd_bf16x4 cgd_to_bf16x4(const cgd_f32x4 v) {
  cgd_bf16x4 r;
  r[0] = (__bf16)v.x;
  r[1] = (__bf16)v.y;
  r[2] = (__bf16)v.z;
  r[3] = (__bf16)v.w;
  return r;
}
__device__ __forceinline__ cgd_f32x4 cgd_residual4(const cgd_f32x4 v, const cgd_bf16x4 hi) {
  return cgd_f32x4{v.x - (float)hi[0], v.y - (float)hi[1], v.z - (float)hi[2], v.w - (float)hi[3]};
}

// fp32 quad -> bf16 hi quad + bf16 lo quad (lo = bf16(v - float(hi)): the operands of the bf16x3 products), in the instruction sequence the staging loops
// want (round 6): per PAIR one v_cvt_pk_bf16_f32 for hi, the two hi values back as floats with one shift and one mask of that packed word, one packed
// subtract, one v_cvt_pk_bf16_f32 for lo — 10 vector-ALU instructions per quad.  Written element by element (`(__bf16)v.x`, `v.x - (float)hi[0]`) the
// compiler converts the first pair of every quad three times (packed for the store, each element again for its residual): 13 per quad.  Same values.
__device__ __forceinline__ void cgd_split_pair(const cgd_f32x2 v, unsigned& hi, unsigned& lo) {
  hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, cgd_bf16x2));
  const cgd_f32x2 hf = cgd_f32x2{__builtin_bit_cast(float, hi << 16), __builtin_bit_cast(float, hi & 0xffff0000u)};
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(v - hf, cgd_bf16x2));
}
__device__ __forceinline__ void cgd_split_quad(const cgd_f32x4 v, cgd_bf16x4& hi, cgd_bf16x4& lo) {
  cgd_u32x2 h, l;
  unsigned a, b;
  cgd_split_pair(cgd_f32x2{v.x, v.y}, a, b);
  h.x = a; l.x = b;
  cgd_split_pair(cgd_f32x2{v.z, v.w}, a, b);
  h.y = a; l.y = b;
  hi = __builtin_bit_cast(cgd_bf16x4, h);
  lo = __builtin_bit_cast(cgd_bf16x4, l);
}
__device__ __forceinline__ void cgd_split_oct(const float (&v)[8], cgd_bf16x8& hi, cgd_bf16x8& lo) {
  cgd_u32x4 h, l;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned a, b;
    cgd_split_pair(cgd_f32x2{v[2 * p], v[2 * p + 1]}, a, b);
    h[p] = a;
    l[p] = b;
  }
  hi = __builtin_bit_cast(cgd_bf16x8, h);
  lo = __builtin_bit_cast(cgd_bf16x8, l);
}

// ---- buffer loads --------------------------------------------------------------------------------------------------------------------------------
// Raw buffer resource, stride 0; gfx9 resource word 3 = 0x00020000 (DATA_FORMAT 32).  A lane whose voffset is >= `records` (bytes) reads zeros and touches
// no memory: padding pixels and rows beyond M carry the offset CGD_OOB, and a resource of zero records puts every lane out of range.  `base` and
// `records` are wave-uniform.
constexpr int CGD_OOB = (int)0x80000000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t cgd_buf_rsrc(const void* base, unsigned records) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)records, 0x00020000);
}
// neg = a wave-uniform integer: < 0 -> the loads are wanted (`records` as given), >= 0 -> they are past the end of the slice (zero records).  The sign
// bit is spread by a scalar shift in inline asm: plain C++ is re-written into a compare + select by the optimiser, and a select is lowered through
// v_cndmask, which puts the resource into vector registers, i.e. a readfirstlane loop around every load.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t cgd_buf_rsrc(const void* base, unsigned records, int neg) {
  int num;
  asm("s_ashr_i32 %0, %1, 31" : "=s"(num) : "s"(neg) : "scc");
  return cgd_buf_rsrc(base, (unsigned)num & records);
}
// 16 bytes at base + voffset (per lane) + soffset (wave-uniform)
__device__ __forceinline__ cgd_i32x4 cgd_buf_load16(const __amdgpu_buffer_rsrc_t r, int voffset, int soffset) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, voffset, soffset, 0);
}
// the resource made at the load (after its offsets, the order the staging loops were scheduled with); _if: the resource masked by `neg`
__device__ __forceinline__ cgd_i32x4 cgd_buf_load16(const void* base, unsigned records, int voffset, int soffset) {
  return cgd_buf_load16(cgd_buf_rsrc(base, records), voffset, soffset);
}
__device__ __forceinline__ cgd_i32x4 cgd_buf_load16_if(const void* base, unsigned records, int neg, int voffset, int soffset) {
  return cgd_buf_load16(cgd_buf_rsrc(base, records, neg), voffset, soffset);
}

// ---- non-temporal 16-byte accesses ---------------------------------------------------------------------------------------------------------------
// the "nt" cache policy: the line is not kept for a reuse that never comes (MI355X_MICROARCH.md "nt-weights")
template <typename V>
__device__ __forceinline__ V cgd_ld16_nt(const void* p) {
  static_assert(sizeof(V) == 16, "a 16-byte vector type");
  return __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
}
template <typename V>
__device__ __forceinline__ void cgd_st16_nt(void* p, const V v) {
  static_assert(sizeof(V) == 16, "a 16-byte vector type");
  __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
}
// for packed weights that exactly ONE workgroup reads once per pass (the 8x8-level convs, the few-row GEMMs, the embedding GEMV; A/B knob CGD_NT)
__device__ __forceinline__ uint4 cgd_load_nt(const uint4* p) {
  const cgd_u32x4 v = cgd_ld16_nt<cgd_u32x4>(p);
  return uint4{v.x, v.y, v.z, v.w};
}

// ---- fused GroupNorm + SiLU of the 3x3 conv kernels' patch staging -----------------------------------------------------------------------------------
// 1 / (1 + exp(-u)) on v_rcp_f32 (1 ulp) instead of the 10-instruction IEEE division
__device__ __forceinline__ float cgd_sigmoid_rcp(float u) { return __builtin_amdgcn_rcpf(1.f + __expf(-u)); }
// silu(x * a + b), {a, b} = the norm's folded per-(sample, channel) pair.  The operands are taken by reference so that they are read where the expression
// uses them, as in the macros this replaces: taken by value, kconv_kernel's GN instantiations are scheduled differently (WR = 3: 4190 instructions and
// 244 registers for 4211 and 242)
__device__ __forceinline__ float cgd_silu_affine(const float& x, const float& a, const float& b) {
  const float u = x * a + b;
  return u * cgd_sigmoid_rcp(u);
}

// ---- per-wavefront timeline stamps (benchmarks/ubench/*_stamps.hip) ----------------------------------------------------------------------------------
// REC: unsigned long long records [workgroup][wavefront 0..3][32].  Lane 0 of wavefront WAVE of workgroup WG stores into entry I: CGD_STAMP wall_clock64()
// (100 MHz), CGD_STAMP_HW_ID the wavefront's XCC_ID | HW_ID.  The kernel files wrap these in macros of their own, which are CGD_NO_STAMP in the library build.
#define CGD_STAMP_VALUE(REC, WG, WAVE, I, V)                                        \
  do {                                                                              \
    if ((threadIdx.x & 63) == 0) (REC)[((long)(WG) * 4 + (WAVE)) * 32 + (I)] = (V); \
  } while (0)
#define CGD_STAMP(REC, WG, WAVE, I) CGD_STAMP_VALUE(REC, WG, WAVE, I, wall_clock64())
#define CGD_STAMP_HW_ID(REC, WG, WAVE, I) \
  CGD_STAMP_VALUE(REC, WG, WAVE, I, ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4))
#define CGD_NO_STAMP \
  do {               \
  } while (0)
