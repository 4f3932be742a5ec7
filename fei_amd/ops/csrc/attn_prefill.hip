// Causal GQA prefill attention over a contiguous bf16 cache for gfx950.
// Semantics: fei_amd/ops/reference.py::attn_prefill — q [B,S,Hq,D] (roped),
// caches [B,Hkv,max_seq,D] already hold the roped K and V for positions
// [0, pos0+S); q token s attends cache [0, pos0+s] (causal) or [0, kv_len)
// (bidirectional, used by the bge encoder path).
//
// The tiles, swizzles, MFMA chains, softmax and epilogue are the shared tile
// core's (attn_prefill_core.h, which also has the structure notes and the
// fragment maps). Particular to this kernel: grid (ceil(S/64), Hq, B), the
// run-time `causal` flag, and a K/V slot that is 8 contiguous bf16 of cache
// row kk.
#include "attn_prefill_core.h"

namespace {

template <int D>
__global__ void __launch_bounds__(256)
k_attn_prefill(const u16* __restrict__ q, const u16* __restrict__ kc,
               const u16* __restrict__ vc, u16* __restrict__ out,
               const int* __restrict__ pos0, const int* __restrict__ kv_len,
               int B, int S, int Hq, int Hkv, int max_seq, float scale,
               int causal, long q_ts) {
  using namespace prefill;
  const int qt = blockIdx.x;       // 64-row q tile
  const int hq = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x;
  const int p0 = pos0[b];
  const int q_hi = min(qt * 64 + 64, S);           // exclusive rel row bound
  const int kv_end = causal ? (p0 + q_hi) : kv_len[b];

  __shared__ Tiles<D> T;
  Wave<D> st;
  wave_init<D>(st, q, (long)b * S, qt, S, hq, q_ts);

  const u16* kbase = kc + ((long)b * Hkv + hkv) * max_seq * D;
  const u16* vbase = vc + ((long)b * Hkv + hkv) * max_seq * D;

  const int ntiles = (kv_end + KV - 1) / KV;
  for (int t = 0; t < ntiles; ++t) {
    // ---- stage K/V tile (KV keys x D), zero-padded past kv_end ----------
    __syncthreads();                                // vt/kt reuse protection
    for (int i = tid; i < KV * D / 8; i += 256) {   // vec8 slots in a tile
      const int key = i / (D / 8);
      const int col8 = i % (D / 8);
      const int kk = t * KV + key;
      s16x8 k8 = {0, 0, 0, 0, 0, 0, 0, 0};
      s16x8 v8 = k8;
      if (kk < kv_end) {
        k8 = *(const s16x8*)(kbase + (long)kk * D + col8 * 8);
        v8 = *(const s16x8*)(vbase + (long)kk * D + col8 * 8);
      }
      store_slot<D>(T, key, col8, k8, v8);
    }
    __syncthreads();
    tile_compute<D>(st, T, t, kv_end, p0, qt, scale, causal);
  }
  epilogue<D>(st, out, (long)b * S, qt, S, hq, Hq);
}

}  // namespace

extern "C" {

void fei_attn_prefill(const void* q, const void* k_cache, const void* v_cache,
                      void* out, const int* pos0, const int* kv_len,
                      int B, int S, int Hq, int Hkv, int D, int max_seq,
                      float scale, int causal, long q_ts, hipStream_t stream) {
  dim3 grid((S + 63) / 64, Hq, B);
  if (D == 128) {
    hipLaunchKernelGGL(k_attn_prefill<128>, grid, dim3(256), 0, stream,
                       (const u16*)q, (const u16*)k_cache, (const u16*)v_cache,
                       (u16*)out, pos0, kv_len, B, S, Hq, Hkv, max_seq, scale,
                       causal, q_ts);
  } else if (D == 64) {
    hipLaunchKernelGGL(k_attn_prefill<64>, grid, dim3(256), 0, stream,
                       (const u16*)q, (const u16*)k_cache, (const u16*)v_cache,
                       (u16*)out, pos0, kv_len, B, S, Hq, Hkv, max_seq, scale,
                       causal, q_ts);
  }
}

// ---------------------------------------------------------------------------
// MFMA layout probe: C[16x16] = A[16x32] @ B[32x16] with the fragment maps
// of attn_prefill_core.h, all matrices row-major bf16 in global memory. Lets
// the GPU test falsify the assumed lane mappings with asymmetric inputs
// (guide §3).
// ---------------------------------------------------------------------------
__global__ void k_mfma_probe(const u16* __restrict__ A,
                             const u16* __restrict__ Bm,
                             float* __restrict__ C) {
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15;
  const int lg = lane >> 4;
  s16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = (short)A[l15 * 32 + 8 * lg + j];
    b[j] = (short)Bm[(8 * lg + j) * 16 + l15];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) C[(4 * lg + r) * 16 + l15] = acc[r];
}

void fei_mfma_probe(const void* A, const void* B, float* C,
                    hipStream_t stream) {
  hipLaunchKernelGGL(k_mfma_probe, dim3(1), dim3(64), 0, stream,
                     (const u16*)A, (const u16*)B, C);
}

}  // extern "C"
