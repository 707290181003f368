// Shared device/host helpers for the Daft-Exprt gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define DX_OK 0
#define DX_ERR_ARG 1
#define DX_ERR_LAUNCH 2

#ifdef __cplusplus
extern "C" {
#endif
void dx_set_error(const char* fmt, ...);
#ifdef __cplusplus
}
#endif

#define DX_REQUIRE(cond, ...)              \
  do {                                     \
    if (!(cond)) {                         \
      dx_set_error(__VA_ARGS__);           \
      return DX_ERR_ARG;                   \
    }                                      \
  } while (0)

#define DX_LAUNCH_CHECK(name)                                         \
  do {                                                                \
    hipError_t e_ = hipGetLastError();                                \
    if (e_ != hipSuccess) {                                           \
      dx_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
      return DX_ERR_LAUNCH;                                           \
    }                                                                 \
  } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
// The 16-bit operand / storage type of the reduced-precision paths.  dx_gemm.hip, dx_ffpair.hip, dx_attention.hip and dx_rows.hip are
// compiled TWICE: as they stand (bf16: BASELINE.json config 2) and with -DDX_F16 (IEEE fp16: config 5), where every exported name
// gets the suffix _f16 (dx_f16_names.h) and every "bf16" flag / argument of the C ABI means "fp16".  Same kernels, same layouts,
// v_mfma_f32_16x16x32_f16 instead of _bf16.  (The vector typedefs keep their historic names.)
#ifdef DX_F16
typedef _Float16 dx_h16;
#define DX_MFMA_H16(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_f16((A), (B), (C), 0, 0, 0)
#include "dx_f16_names.h"
#else
typedef __bf16 dx_h16;
#define DX_MFMA_H16(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_bf16((A), (B), (C), 0, 0, 0)
#endif
#include "../../include/daft_exprt_hip.h"   // after the renames: the prototypes, DxWgradJob, the launch-plan record (DX_PLAN_*, DX_K_*)
typedef dx_h16 bf16x8 __attribute__((ext_vector_type(8)));
typedef dx_h16 bf16x4 __attribute__((ext_vector_type(4)));

static inline int dx_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int dx_roundup(int a, int b) { return dx_cdiv(a, b) * b; }
static inline bool dx_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the six fields every launch plan has (include/daft_exprt_hip.h); the family's own fields start at zero
static inline void dx_plan_set(int* p, int kernel, int tok, int gx, int gy, int gz, int threads) {
  for (int i = 0; i < DX_PLAN_INTS; ++i) p[i] = 0;
  p[DX_PLAN_KERNEL] = kernel; p[DX_PLAN_TOK] = tok; p[DX_PLAN_GRID_X] = gx; p[DX_PLAN_GRID_Y] = gy; p[DX_PLAN_GRID_Z] = gz; p[DX_PLAN_THREADS] = threads;
}

#ifdef __HIPCC__
// ---- split-bf16 operands (C ABI operand mode 2, bf16 build) ---------------------------------------------------------------------
// x = hi + lo with hi = bf16_rne(x), lo = bf16_rne(x - hi) (v_cvt_pk_bf16_f32); lo = 0 where hi is not finite, so an inf / NaN operand
// makes exactly the sums non-finite that it makes non-finite in exact f32 (an inf may become NaN: inf * lo, lo = 0 where the other
// operand is exact in bf16).  A product is hi_a*lo_b + lo_a*hi_b + hi_a*hi_b, the two small cross terms
// first, fp32 accumulate: ~16 mantissa bits for 3 bf16 MFMAs where the exact-f32 form needs 8 K=4 ones.
typedef __bf16 dx_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 dx_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_bf16x2(float x0, float x1, unsigned& hi, unsigned& lo) {
  dx_bf16x2 h, l;
  h[0] = (__bf16)x0; h[1] = (__bf16)x1;
  const float h0 = (float)h[0], h1 = (float)h[1];
  l[0] = (__bf16)(__builtin_isfinite(h0) ? x0 - h0 : 0.f);
  l[1] = (__bf16)(__builtin_isfinite(h1) ? x1 - h1 : 0.f);
  hi = __builtin_bit_cast(unsigned, h); lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ void split_bf16x4(const f32x4& v, uint2& hi, uint2& lo) {
  split_bf16x2(v[0], v[1], hi.x, lo.x);
  split_bf16x2(v[2], v[3], hi.y, lo.y);
}
// two 4-element groups -> one 8-element hi / lo MFMA operand (a first, then b)
__device__ __forceinline__ void split_bf16x8(const f32x4& a, const f32x4& b, dx_bf16x8& hi, dx_bf16x8& lo) {
  uint2 ha, la, hb, lb;
  split_bf16x4(a, ha, la);
  split_bf16x4(b, hb, lb);
  hi = __builtin_bit_cast(dx_bf16x8, make_uint4(ha.x, ha.y, hb.x, hb.y));
  lo = __builtin_bit_cast(dx_bf16x8, make_uint4(la.x, la.y, lb.x, lb.y));
}
__device__ __forceinline__ f32x4 dx_mma_split3(const dx_bf16x8& ah, const dx_bf16x8& al, const dx_bf16x8& bh, const dx_bf16x8& bl, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
  return c;
}

// ---- exact-f32 / bf16 operand modes of the kernels whose storage is fp32 ---------------------------------------------------------
// One 16-wide k step in exact f32: four chained v_mfma_f32_16x16x4_f32; a / b hold the lane's 4 consecutive k (k = 4 (lane / 16) + e)
// of row / column (lane % 16).  A and B use the same k map, so any permutation inside a step cancels.
__device__ __forceinline__ f32x4 dx_mma_f32_k16(f32x4 a, f32x4 b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c, 0, 0, 0);
  return c;
}
// T: the LDS / pack element; KS: k per step; VEC: k per lane and step (one 16-byte fragment); PAD: LDS row padding in elements.
// Always bf16 (never dx_h16): these kernels have no fp16 twin.
template <bool BF> struct DxMmaOp;
template <> struct DxMmaOp<false> {
  typedef float T;
  static constexpr int KS = 16, VEC = 4, PAD = 4;
  __device__ static __forceinline__ T cvt(float v) { return v; }
  __device__ static __forceinline__ f32x4 mma(const uint4& a, const uint4& b, f32x4 c) {
    return dx_mma_f32_k16(__builtin_bit_cast(f32x4, a), __builtin_bit_cast(f32x4, b), c);
  }
};
template <> struct DxMmaOp<true> {
  typedef __bf16 T;
  static constexpr int KS = 32, VEC = 8, PAD = 8;
  __device__ static __forceinline__ T cvt(float v) { return (__bf16)v; }
  __device__ static __forceinline__ f32x4 mma(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dx_bf16x8, a), __builtin_bit_cast(dx_bf16x8, b), c, 0, 0, 0);
  }
};

// The same trait by C ABI operand mode (0 exact f32, 1 bf16, 2 split bf16), for the kernels that take all three.  An operand is IMG
// images of T, a lane's fragment one uint4 per image: modes 0 and 1 are DxMmaOp as it stands with one image; mode 2 keeps a hi and
// a lo bf16 image with bf16's k map (KS, VEC, PAD), so its operand bytes are the f32 mode's.
//   put / put4(d, los, v): write fp32 values as operand elements at d (mode 2: the lo image los elements further on);
//   mma(a, b, c): a and b the fragments of every image ([0] hi, [1] lo).
template <int MODE> struct DxMmaMode : DxMmaOp<MODE != 0> {
  typedef DxMmaOp<MODE != 0> Base;
  typedef typename Base::T T;
  static constexpr int IMG = 1;
  __device__ static __forceinline__ void put(T* d, int, float v) { *d = Base::cvt(v); }
  __device__ static __forceinline__ void put4(T* d, int, const float4& v) {
    d[0] = Base::cvt(v.x); d[1] = Base::cvt(v.y); d[2] = Base::cvt(v.z); d[3] = Base::cvt(v.w);
  }
  __device__ static __forceinline__ f32x4 mma(const uint4 (&a)[1], const uint4 (&b)[1], f32x4 c) { return Base::mma(a[0], b[0], c); }
};
template <> struct DxMmaMode<2> {
  typedef __bf16 T;
  static constexpr int KS = 32, VEC = 8, PAD = 8, IMG = 2;
  __device__ static __forceinline__ void put(T* d, int los, float v) {
    unsigned h, l;
    split_bf16x2(v, 0.f, h, l);
    *reinterpret_cast<unsigned short*>(d) = (unsigned short)h;
    *reinterpret_cast<unsigned short*>(d + los) = (unsigned short)l;
  }
  __device__ static __forceinline__ void put4(T* d, int los, const float4& v) {      // d 8-byte aligned, los % 4 == 0
    uint2 h, l;
    split_bf16x4(f32x4{v.x, v.y, v.z, v.w}, h, l);
    *reinterpret_cast<uint2*>(d) = h;
    *reinterpret_cast<uint2*>(d + los) = l;
  }
  __device__ static __forceinline__ f32x4 mma(const uint4 (&a)[2], const uint4 (&b)[2], f32x4 c) {
    return dx_mma_split3(__builtin_bit_cast(dx_bf16x8, a[0]), __builtin_bit_cast(dx_bf16x8, a[1]), __builtin_bit_cast(dx_bf16x8, b[0]),
                         __builtin_bit_cast(dx_bf16x8, b[1]), c);
  }
};

// ---- wave64 reductions -------------------------------------------------------------------------
__device__ __forceinline__ float dx_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float dx_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// ---- counter-based dropout RNG -----------------------------------------------------------------
// Counter-based draw for (seed, index): 64 random bits = four 16-bit keep/drop decisions.  The same (seed, index) is
// evaluated again in the backward kernels, so no mask tensor is stored.  The attention kernels are VALU-bound with dropout on
// (a wave64 vector instruction takes 4 cycles; ~40 % of their instructions were this function), so the mixer is as short as the
// statistics allow: the high halves of index and seed are folded in by one multiply (loop-invariant in every caller: hoisted), the
// low word is a two-round multiply-xorshift finaliser (the "lowbias32" constants), the high word one more multiply-xorshift of the
// low one: 3 multiplies in the loop instead of 6, ~13 instructions instead of ~22.  Keep rate per field, cross-field, lag-1 along
// keys / rows / consecutive indices, seed vs seed + 1 correlations and byte uniformity of the keep mask are all at noise level on
// 4 M attention-shaped and 4 M consecutive indices (tests/test_host_glue_cpu.py restates the function in numpy and checks them).
__device__ __forceinline__ uint64_t dx_rand64(uint64_t seed, uint64_t idx) {
  uint32_t x = (uint32_t)idx ^ (uint32_t)seed;
  const uint32_t hi = (uint32_t)(idx >> 32) ^ (uint32_t)(seed >> 32);
  x ^= hi * 0x9E3779B1u;
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  uint32_t y = (x ^ 0x85EBCA6Bu) * 0xC2B2AE35u; y ^= y >> 15;
  return ((uint64_t)y << 32) | x;
}
__device__ __forceinline__ float dx_dropout_scale(uint64_t seed, uint64_t elem, uint32_t thresh16, float inv_keep) {
  uint64_t r = dx_rand64(seed, elem >> 2);
  uint32_t bits = (uint32_t)(r >> (16 * (elem & 3))) & 0xFFFFu;
  return bits >= thresh16 ? inv_keep : 0.0f;
}
// Keep/drop selection without unpacking the draw: the 16-bit field is compared IN PLACE (SDWA word select) and the value is
// selected by the resulting mask -- one v_cmp + one v_cndmask per element instead of shift, mask, compare, select, multiply.
// The 1/(1-p) factor is not applied here: callers fold it into an operand or an epilogue scale (it is the same for all kept elements).
// result = (field >= thresh) ? x : alt, field = low (dx_keep_lo) or high (dx_keep_hi) half of w.  thresh < 65536.
// HAZARD RULE: x and alt must be results of ordinary VALU instructions, never MFMA accumulators -- the compiler's hazard recogniser
// does not look inside inline asm, and an asm that reads an accumulator too early reads stale data (callers subtract or copy first).
__device__ __forceinline__ float dx_keep_lo(uint32_t w, uint32_t thresh, float x, float alt) {
  float y;
  asm("v_cmp_ge_u16_sdwa vcc, %1, %2 src0_sel:WORD_0 src1_sel:WORD_0\n\tv_cndmask_b32_e32 %0, %4, %3, vcc" : "=v"(y) : "v"(w), "v"(thresh), "v"(x), "v"(alt) : "vcc");
  return y;
}
__device__ __forceinline__ float dx_keep_hi(uint32_t w, uint32_t thresh, float x, float alt) {
  float y;
  asm("v_cmp_ge_u16_sdwa vcc, %1, %2 src0_sel:WORD_1 src1_sel:WORD_0\n\tv_cndmask_b32_e32 %0, %4, %3, vcc" : "=v"(y) : "v"(w), "v"(thresh), "v"(x), "v"(alt) : "vcc");
  return y;
}
// two values under the same decision (field already isolated in `bits`): x <- kept ? x : 0, y <- kept ? y : alt
__device__ __forceinline__ void dx_keep2(uint32_t bits, uint32_t thresh, float& x, float& y, float alt) {
  asm("v_cmp_ge_u32_e32 vcc, %2, %3\n\tv_cndmask_b32_e32 %0, 0, %0, vcc\n\tv_cndmask_b32_e32 %1, %4, %1, vcc" : "+v"(x), "+v"(y) : "v"(bits), "v"(thresh), "v"(alt) : "vcc");
}
// x[i] <- kept(i) ? x[i] : alt for the four consecutive elements of one draw
__device__ __forceinline__ void dx_keep4(uint64_t r, uint32_t thresh, float x[4], float alt) {
  const uint32_t lo = (uint32_t)r, hi = (uint32_t)(r >> 32);
  x[0] = dx_keep_lo(lo, thresh, x[0], alt); x[1] = dx_keep_hi(lo, thresh, x[1], alt);
  x[2] = dx_keep_lo(hi, thresh, x[2], alt); x[3] = dx_keep_hi(hi, thresh, x[3], alt);
}
// four consecutive elements (elem0 % 4 == 0)
__device__ __forceinline__ void dx_dropout_scale4(uint64_t seed, uint64_t elem0, uint32_t thresh16, float inv_keep, float out[4]) {
  uint64_t r = dx_rand64(seed, elem0 >> 2);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = ((uint32_t)(r >> (16 * i)) & 0xFFFFu) >= thresh16 ? inv_keep : 0.0f;
}
#endif
