// Fused score + top-k over an embedding corpus (gfx950): the scan behind
// memdir semantic search. One pass over emb [N, C] scores every eligible row
// against up to 8 f32 queries and keeps a running top-k per query; the
// N-float score vector is never written and no selection launch runs.
//
//   k_score_topk_partial<T, Q, NT, NTL>   grid WG x 256 threads
//     Workgroup g owns the contiguous slab [g*N/WG, (g+1)*N/WG), cut once
//     more into four contiguous wave ranges. A wave walks its range 64 rows
//     at a time: each lane reads one mask byte (rows at or past the range end
//     are not read), a ballot turns the 64 bytes into a wave-uniform bit set,
//     and the wave pops TWO set bits per step, so two eligible rows' loads
//     are in flight whatever the mask density and a masked-out row is never
//     loaded. Loads are 16 B per lane (4 f32 or 8 f16), all NT chunks of both
//     rows issued before the first dot; NTL selects nontemporal loads
//     (k_gemv's rule: the corpus is past L3). Each lane's slice of the Q
//     query rows lives in registers (NT * 16/sizeof(T) * Q floats) for the
//     whole slab. Dots accumulate in f32; one wave reduction per (row, query).
//
//     Running top-k, per wave and query: k <= 64, so one candidate (score,
//     row) per lane, lanes >= k parked on a better-than-anything sentinel.
//     The current minimum and its lane are wave-uniform; a new score is
//     compared against it (uniform branch), replaces the minimum's lane on
//     insert, and the minimum is recomputed with one wave reduction.
//     At slab end the four waves' candidates meet in LDS and every candidate
//     counts how many others beat it: rank < k is its slot in the
//     workgroup's sorted partial list [Q, WG, k]; empty slots are (-inf, -1).
//
//   k_score_topk_final                    grid Q x 1024 threads
//     Workgroup q streams its WG*k partials through the same per-wave
//     running top-k (a ballot picks the lanes that beat the wave's minimum)
//     and the same LDS rank merge, and writes the final k, sorted.
//
// Order: everywhere (score descending, then row ascending), a total order on
// real candidates, so the result is a function of the inputs alone: not of
// WG, the slab cut or which wave saw a row. A NaN score counts as -inf.
//
// No kernel reads emb or mask at or past row N: row indices come from set
// bits of ballots guarded by row < range end, chunk indices clamp to the
// row's last 16 B (the clamped lanes' query registers are 0).
#include "fei_common.h"

#include <limits.h>
#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

#define ST_EMPTY_ROW INT_MAX          // empty slot inside the kernels

// a wave-uniform value, moved to a scalar register so branches on it are scalar
__device__ __forceinline__ float st_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// a strictly before b in the order (score desc, row asc)
__device__ __forceinline__ bool st_better(float as, int ai, float bs, int bi) {
  return as > bs || (as == bs && ai < bi);
}

// One wave's running top-k for one query. cs/ci: this lane's candidate.
// ms/mi/ml: the wave's worst candidate and its lane, wave-uniform.
struct WaveTopK {
  float cs;
  int ci;
  float ms;
  int mi;
  int ml;

  __device__ __forceinline__ void init(int lane, int k) {
    const bool live = lane < k;
    cs = live ? -INFINITY : INFINITY;       // lanes >= k: never the minimum
    ci = live ? ST_EMPTY_ROW : -1;
    ms = -INFINITY;
    mi = ST_EMPTY_ROW;
    ml = 0;
  }

  // s, r wave-uniform
  __device__ __forceinline__ void insert(float s, int r, int lane) {
    if (!st_better(s, r, ms, mi)) return;
    if (lane == ml) { cs = s; ci = r; }
    float ws = cs;
    int wi = ci;
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      const float os = __shfl_xor(ws, off);
      const int oi = __shfl_xor(wi, off);
      if (st_better(ws, wi, os, oi)) { ws = os; wi = oi; }
    }
    ms = st_uniform(ws);
    mi = __builtin_amdgcn_readfirstlane(wi);
    ml = __builtin_ctzll(__ballot(cs == ms && ci == mi));
  }
};

// Merge the NW waves' candidates of one query (already in LDS, row -1 =
// none) into the sorted best k at out_s/out_i. Every thread of the block
// calls it; tid indexes the candidate it ranks.
template <int NW>
__device__ __forceinline__ void st_merge(const float* __restrict__ ls,
                                         const int* __restrict__ li,
                                         float* __restrict__ out_s,
                                         int* __restrict__ out_i,
                                         int tid, int k) {
  const float s = ls[tid];
  const int i = li[tid];
  int rank = 0, nreal = 0;
  for (int w = 0; w < NW; ++w) {
    for (int l = 0; l < k; ++l) {
      const float os = ls[w * 64 + l];
      const int oi = li[w * 64 + l];
      if (oi >= 0) {
        ++nreal;
        rank += st_better(os, oi, s, i) ? 1 : 0;
      }
    }
  }
  if (i >= 0 && rank < k) {
    out_s[rank] = s;
    out_i[rank] = i;
  }
  if (tid < k && tid >= nreal) {
    out_s[tid] = -INFINITY;
    out_i[tid] = -1;
  }
}

template <typename T> struct StVec;
template <> struct StVec<float> {
  typedef f32x4 V;
  static constexpr int E = 4;
};
template <> struct StVec<_Float16> {
  typedef f16x8 V;
  static constexpr int E = 8;
};

template <typename V, bool NTL>
__device__ __forceinline__ V st_load(const V* p) {
  return NTL ? __builtin_nontemporal_load(p) : *p;
}

template <typename T, int Q, int NT, bool NTL>
__global__ void __launch_bounds__(256)
k_score_topk_partial(const T* __restrict__ emb, const float* __restrict__ q,
                     const unsigned char* __restrict__ mask,
                     float* __restrict__ part_s, int* __restrict__ part_i,
                     int N, int C, int nq, int k) {
  typedef typename StVec<T>::V V;
  constexpr int E = StVec<T>::E;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int WG = gridDim.x;
  const long lo = (long)blockIdx.x * N / WG;
  const long hi = (long)(blockIdx.x + 1) * N / WG;
  const int wlo = (int)(lo + (hi - lo) * wid / 4);
  const int whi = (int)(lo + (hi - lo) * (wid + 1) / 4);
  const int nv = C / E;                       // 16 B chunks per row, >= 1

  // this lane's slice of the queries; 0 past the row and for padding queries
  float qr[NT][Q][E];
  int cidx[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = t * 64 + lane;
    cidx[t] = min(c, nv - 1);
#pragma unroll
    for (int u = 0; u < Q; ++u) {
      const bool live = c < nv && u < nq;
      const f32x4* src = (const f32x4*)(q + (long)(live ? u : 0) * C +
                                        (long)cidx[t] * E);
#pragma unroll
      for (int h = 0; h < E / 4; ++h) {
        const f32x4 v = src[h];
#pragma unroll
        for (int j = 0; j < 4; ++j) qr[t][u][h * 4 + j] = live ? v[j] : 0.f;
      }
    }
  }

  WaveTopK tk[Q];
#pragma unroll
  for (int u = 0; u < Q; ++u) tk[u].init(lane, k);

  for (int base = wlo; base < whi; base += 64) {
    const int r = base + lane;
    bool el = r < whi;
    if (el && mask) el = mask[r] != 0;
    u64 bits = __ballot(el);
    while (bits) {
      const int r0 = base + __builtin_ctzll(bits);
      bits &= bits - 1;
      const bool two = bits != 0;
      const int r1 = two ? base + __builtin_ctzll(bits) : r0;
      bits &= bits - 1;                       // 0 stays 0
      const V* p0 = (const V*)(emb + (long)r0 * C);
      const V* p1 = (const V*)(emb + (long)r1 * C);
      V v0[NT], v1[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v0[t] = st_load<V, NTL>(&p0[cidx[t]]);
#pragma unroll
      for (int t = 0; t < NT; ++t) v1[t] = st_load<V, NTL>(&p1[cidx[t]]);
      float a0[Q], a1[Q];
#pragma unroll
      for (int u = 0; u < Q; ++u) { a0[u] = 0.f; a1[u] = 0.f; }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
          const float e0 = (float)v0[t][j];
          const float e1 = (float)v1[t][j];
#pragma unroll
          for (int u = 0; u < Q; ++u) {
            a0[u] = fmaf(e0, qr[t][u][j], a0[u]);
            a1[u] = fmaf(e1, qr[t][u][j], a1[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < Q; ++u) {
        float s0 = st_uniform(wave_reduce_sum(a0[u]));
        float s1 = st_uniform(wave_reduce_sum(a1[u]));
        if (u < nq) {
          s0 = s0 != s0 ? -INFINITY : s0;
          s1 = s1 != s1 ? -INFINITY : s1;
          tk[u].insert(s0, r0, lane);
          if (two) tk[u].insert(s1, r1, lane);
        }
      }
    }
  }

  __shared__ float ls[Q][256];
  __shared__ int li[Q][256];
#pragma unroll
  for (int u = 0; u < Q; ++u) {
    const bool real = lane < k && tk[u].ci != ST_EMPTY_ROW;
    ls[u][tid] = tk[u].cs;
    li[u][tid] = real ? tk[u].ci : -1;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < Q; ++u) {
    if (u < nq) {
      const long o = ((long)u * WG + blockIdx.x) * k;
      st_merge<4>(ls[u], li[u], part_s + o, part_i + o, tid, k);
    }
  }
}

#define ST_FINAL_WAVES 16

__global__ void __launch_bounds__(ST_FINAL_WAVES * 64)
k_score_topk_final(const float* __restrict__ part_s,
                   const int* __restrict__ part_i,
                   float* __restrict__ out_s, int* __restrict__ out_i,
                   int M, int k) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const float* ps = part_s + (long)blockIdx.x * M;
  const int* pi = part_i + (long)blockIdx.x * M;

  WaveTopK tk;
  tk.init(lane, k);
  for (int base = wid * 64; base < M; base += ST_FINAL_WAVES * 64) {
    const int j = base + lane;
    float s = -INFINITY;
    int i = -1;
    if (j < M) { s = ps[j]; i = pi[j]; }
    u64 bits = __ballot(i >= 0 && st_better(s, i, tk.ms, tk.mi));
    while (bits) {
      const int b = __builtin_ctzll(bits);
      bits &= bits - 1;
      tk.insert(st_uniform(__shfl(s, b)),
                __builtin_amdgcn_readfirstlane(__shfl(i, b)), lane);
    }
  }

  __shared__ float ls[ST_FINAL_WAVES * 64];
  __shared__ int li[ST_FINAL_WAVES * 64];
  const bool real = lane < k && tk.ci != ST_EMPTY_ROW;
  ls[tid] = tk.cs;
  li[tid] = real ? tk.ci : -1;
  __syncthreads();
  st_merge<ST_FINAL_WAVES>(ls, li, out_s + (long)blockIdx.x * k,
                           out_i + (long)blockIdx.x * k, tid, k);
}

template <typename T, int Q, int NT>
void st_launch(const void* emb, const void* q, const void* mask, void* part_s,
               void* part_i, int N, int C, int nq, int k, int WG,
               int nontemporal, hipStream_t stream) {
  if (nontemporal)
    hipLaunchKernelGGL((k_score_topk_partial<T, Q, NT, true>), dim3(WG),
                       dim3(256), 0, stream, (const T*)emb, (const float*)q,
                       (const unsigned char*)mask, (float*)part_s,
                       (int*)part_i, N, C, nq, k);
  else
    hipLaunchKernelGGL((k_score_topk_partial<T, Q, NT, false>), dim3(WG),
                       dim3(256), 0, stream, (const T*)emb, (const float*)q,
                       (const unsigned char*)mask, (float*)part_s,
                       (int*)part_i, N, C, nq, k);
}

template <typename T, int Q>
void st_launch_nt(int nt, const void* emb, const void* q, const void* mask,
                  void* part_s, void* part_i, int N, int C, int nq, int k,
                  int WG, int nontemporal, hipStream_t stream) {
#define ST_ARGS emb, q, mask, part_s, part_i, N, C, nq, k, WG, nontemporal, stream
  if (nt <= 1) st_launch<T, Q, 1>(ST_ARGS);
  else if (nt <= 2) st_launch<T, Q, 2>(ST_ARGS);
  else if (nt <= 4) st_launch<T, Q, 4>(ST_ARGS);
  else if constexpr (sizeof(T) == 4) st_launch<T, Q, 8>(ST_ARGS);
#undef ST_ARGS
}

template <typename T>
void st_launch_q(int nt, const void* emb, const void* q, const void* mask,
                 void* part_s, void* part_i, int N, int C, int nq, int k,
                 int WG, int nontemporal, hipStream_t stream) {
#define ST_ARGS nt, emb, q, mask, part_s, part_i, N, C, nq, k, WG, nontemporal, stream
  if (nq <= 1) st_launch_nt<T, 1>(ST_ARGS);
  else if (nq <= 2) st_launch_nt<T, 2>(ST_ARGS);
  else if (nq <= 4) st_launch_nt<T, 4>(ST_ARGS);
  else st_launch_nt<T, 8>(ST_ARGS);
#undef ST_ARGS
}

}  // namespace

extern "C" {

// scores [Q, k] f32 and rows [Q, k] i32 of the k best eligible rows of
// emb [N, C] (f32, or f16 with is_f16) per query of q [Q, C] f32, sorted by
// (score desc, row asc), the tail (-inf, -1) when fewer than k rows are
// eligible. mask: u8 [N], non-zero = eligible, or null for every row.
// part_s / part_i: workspace [Q, WG, k] f32 / i32.
// Returns 0, or a negative code with nothing launched and nothing written:
// -1 a null pointer, -2 k outside 1..64, -3 Q outside 1..8, -4 C not a
// multiple of 8 in 8..2048, -5 N < 1, -6 WG outside 1..min(N, 65536), -7 emb or q not
// 16 B aligned.
int fei_score_topk(const void* emb, const void* q, const void* mask,
                   void* part_s, void* part_i, void* out_s, void* out_i,
                   int N, int C, int Q, int k, int WG, int is_f16,
                   int nontemporal, hipStream_t stream) {
  if (!emb || !q || !part_s || !part_i || !out_s || !out_i) return -1;
  if (k < 1 || k > 64) return -2;
  if (Q < 1 || Q > 8) return -3;
  if (C < 8 || C > 2048 || C % 8 != 0) return -4;
  if (N < 1) return -5;
  if (WG < 1 || WG > N || WG > 65536) return -6;
  if (((uintptr_t)emb | (uintptr_t)q) & 15) return -7;
  const int nv = C / (is_f16 ? 8 : 4);
  const int nt = (nv + 63) / 64;              // <= 8 (f32) or 4 (f16)
  if (is_f16)
    st_launch_q<_Float16>(nt, emb, q, mask, part_s, part_i, N, C, Q, k, WG,
                          nontemporal, stream);
  else
    st_launch_q<float>(nt, emb, q, mask, part_s, part_i, N, C, Q, k, WG,
                       nontemporal, stream);
  hipLaunchKernelGGL(k_score_topk_final, dim3(Q), dim3(ST_FINAL_WAVES * 64),
                     0, stream, (const float*)part_s, (const int*)part_i,
                     (float*)out_s, (int*)out_i, WG * k, k);
  return 0;
}

}  // extern "C"
