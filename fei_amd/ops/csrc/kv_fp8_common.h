// Device helpers shared by the contiguous (kv_fp8.hip) and the paged
// (kv_fp8_paged.hip) fp8 KV kernels. They live here, and nowhere twice, so
// that every append path writes identical bytes and both decode kernels
// reduce in the same order. Storage format: see the header of kv_fp8.hip
// (fei_amd/ops/reference.py::quant_kv_fp8 is the definition).
#pragma once
#include "fei_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef unsigned char u8;

// Quantise one row held as (x1, x2) = elements (i, i + half) per lane and
// store codes + scale. Must be called by ALL 64 lanes of one wave; lanes
// with i >= half pass act = false (they join the absmax reduction with 0
// and store nothing). D/2 active lanes: one wave at D=128, half at D=64.
__device__ __forceinline__ void kv8_quant_store(float x1, float x2, bool act,
                                                int i, int half,
                                                u8* __restrict__ dst,
                                                float* __restrict__ sdst) {
  float amax = act ? fmaxf(fabsf(x1), fabsf(x2)) : 0.f;
  amax = wave_reduce_max(amax);
  const float scale = amax > 0.f ? amax / 448.f : 1.f;
  if (act) {
    dst[i] = e4m3_encode(x1 / scale);
    dst[i + half] = e4m3_encode(x2 / scale);
    if (i == 0) *sdst = scale;
  }
}

// RoPE + quantise + append of ONE token's k/v row for one kv-head. Every
// append path (decode form, prefill form, the fused decode-attention form,
// contiguous or paged) goes through here, so all of them write identical
// bytes. kp/vp: the raw bf16 rows; cs: cos/sin row of the token's position
// ([D/2][2] f32); `row`: flat row index, ((b*Hkv + hkv)*max_seq + p) in a
// contiguous cache and ((blk*Hkv + hkv)*BS + (p & (BS-1))) in a paged pool —
// it addresses data (x D) and scale alike. All 64 lanes of one wave call it
// with lane = 0..63.
__device__ __forceinline__ void kv8_rope_append(
    const u16* __restrict__ kp, const u16* __restrict__ vp,
    const float* __restrict__ cs, int D, long row, int lane,
    u8* __restrict__ kd, float* __restrict__ ks,
    u8* __restrict__ vd, float* __restrict__ vs) {
  const int half = D / 2;
  const bool act = lane < half;
  float k1 = 0.f, k2 = 0.f, v1 = 0.f, v2 = 0.f;
  if (act) {
    const float c = cs[lane * 2 + 0];
    const float sn = cs[lane * 2 + 1];
    const float x1 = bf2f(kp[lane]), x2 = bf2f(kp[lane + half]);
    // rounded to bf16 exactly as the bf16 cache stores it, then quantised
    k1 = bf2f(f2bf(x1 * c - x2 * sn));
    k2 = bf2f(f2bf(x2 * c + x1 * sn));
    v1 = bf2f(vp[lane]);
    v2 = bf2f(vp[lane + half]);
  }
  kv8_quant_store(k1, k2, act, lane, half, kd + row * D, ks + row);
  kv8_quant_store(v1, v2, act, lane, half, vd + row * D, vs + row);
}

#define DEC8_TILE 256
#define DEC8_DMAX 128
#define DEC8_GMAX 8

// Reduce G values at once, one barrier pair for all heads (the bf16 decode
// kernel's block_reduce_vec, which is local to fei_kernels.hip).
template <int OP, int G>  // OP: 0 = max, 1 = sum
__device__ __forceinline__ void block_reduce_vec8(float* v,
                                                  float red[DEC8_GMAX][4]) {
  const int nw = blockDim.x >> 6;
  const int wid = threadIdx.x >> 6;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float x = v[g];
#pragma unroll
    for (int off = 32; off; off >>= 1)
      x = OP == 0 ? fmaxf(x, __shfl_xor(x, off)) : x + __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) red[g][wid] = x;
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float x = red[g][0];
    for (int i = 1; i < nw; ++i)
      x = OP == 0 ? fmaxf(x, red[g][i]) : x + red[g][i];
    v[g] = x;
  }
  __syncthreads();
}

// 8 codes -> 8 bf16 of f32(code) * sc (the prefill kernels' tile staging)
__device__ __forceinline__ s16x8 kv8_dequant8(u32x2 c8, float sc) {
  s16x8 r;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(c8[w], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(c8[w], true);
    r[w * 4 + 0] = (short)f2bf(lo[0] * sc);
    r[w * 4 + 1] = (short)f2bf(lo[1] * sc);
    r[w * 4 + 2] = (short)f2bf(hi[0] * sc);
    r[w * 4 + 3] = (short)f2bf(hi[1] * sc);
  }
  return r;
}

}  // namespace
