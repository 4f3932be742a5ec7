// The top-k / top-p filtered sampler's per-row body, shared by
// k_sample_filtered (sample_filtered.hip: scalar parameters, one `step`) and
// k_sample_filtered_rows (sample_rows.hip: every parameter per row), so the
// two kernels agree bit for bit by construction.
//
// One 1024-thread workgroup per logits row. Logits are bf16, so a row has at
// most 65 536 distinct values: the filter threshold is found EXACTLY by
// two-level selection over the 16-bit order-preserving key (no sort):
//   level 1: 4096 bins on key>>4  (LDS histogram: u32 count, u64 mass)
//   level 2:   16 bins on key&15  inside the one level-1 bin that holds the
//              threshold (each level-2 bin is ONE bf16 value, so its mass is
//              count x mass(value) -- counts only).
// Semantics = ops/reference.py filter_keep: top-k first (k-th largest counting
// multiplicity, ties kept), then top-p over the top-k set on the RAW logits
// (a value group is kept iff the mass strictly above it is < p); temperature
// applies only at the draw.
//
// Determinism: mass is accumulated as u64 fixed point (40 fractional bits of
// exp(x - rowmax); <= 2^18 terms fit) with integer LDS atomics, so the sums do
// not depend on arrival order. There are no floating-point atomics.
//
// Passes over the row (re-read from L2; a 128 256-wide row is 256 KB):
//   P1 max/min key + level-1 counts            always
//   P2 level-2 counts of the top-k bin and/or level-1 mass of the top-k set
//   P3 level-2 counts of the top-p bin          only if it is not the top-k bin
//   draw: argmax over {key >= thr} of x*invT + Gumbel(hash)   -- same hash,
//         formula and lowest-index tie-break as k_sample_onepass, so filtered
//         and unfiltered sampling share one noise stream.
#pragma once
#include "fei_common.h"

namespace {

constexpr int NT = 1024;            // threads per workgroup
constexpr int NW = NT / 64;         // waves
constexpr int NB1 = 4096;           // level-1 bins (key >> 4)
constexpr int NB2 = 16;             // level-2 bins (key & 15)
constexpr float FX_ONE = 1099511627776.f;   // 2^40

// bf16 bits -> u16 key with the same order as the value (-0 folded into +0 so
// that equal values share a key).
__device__ __forceinline__ u32 bf_key(u16 u) {
  if (u == 0x8000u) u = 0;
  return (u & 0x8000u) ? (u32)(u16)~u : (u32)(u | 0x8000u);
}
__device__ __forceinline__ u16 key_bf(u32 k) {
  return (k & 0x8000u) ? (u16)(k & 0x7fffu) : (u16)~k;
}
// fixed-point mass of one element: a pure function of (key, rowmax)
__device__ __forceinline__ u64 fx_mass(u32 key, float vmax) {
  return (u64)(__expf(bf2f(key_bf(key)) - vmax) * FX_ONE);
}

// Visit every element of a row once: f(idx, bf16 bits). 16-byte vector loads
// over the aligned body; scalar head/tail cover rows that do not start on a
// 16-byte boundary (vocab % 8 != 0, b > 0) and vocab % 8 leftovers.
template <class F>
__device__ __forceinline__ void for_each_elem(const u16* __restrict__ row,
                                              int vocab, F f) {
  const int tid = threadIdx.x;
  int head = (int)(((16u - (u32)((uintptr_t)row & 15u)) & 15u) >> 1);
  if (head > vocab) head = vocab;
  if (tid < head) f(tid, row[tid]);
  const s16x8* body = (const s16x8*)(row + head);
  const int nv = (vocab - head) >> 3;
  for (int i = tid; i < nv; i += NT) {
    const s16x8 v8 = body[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) f(head + i * 8 + j, (u16)v8[j]);
  }
  const int t0 = head + nv * 8;            // < 8 elements left
  if (t0 + tid < vocab) f(t0 + tid, row[t0 + tid]);
}

// Sum of v over all threads with a HIGHER thread index (exclusive suffix
// sum), plus the block total. `red` is LDS with NW entries.
template <class T>
__device__ __forceinline__ T block_suffix_excl(T v, T* red, T* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  T s = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_down(s, off);
    if (lane + off < 64) s += o;
  }
  if (lane == 0) red[wid] = s;
  __syncthreads();
  T hi = 0, tot = 0;
  for (int w = 0; w < NW; ++w) {
    const T x = red[w];
    tot += x;
    if (w > wid) hi += x;
  }
  __syncthreads();
  *total = tot;
  return s - v + hi;
}

// What sample_filtered_row hands back; meaningful in thread 0 only.
struct RowDraw {
  int token;      // drawn index
  u32 thr;        // key of the smallest kept value
  u32 kept;       // size of the keep set
};

// Filter + draw for ONE row by the whole 1024-thread workgroup. Every
// argument is workgroup-uniform. `st` is the draw's step and `hash_row` the
// row id mixed into the noise hash (k_sample_filtered passes blockIdx.x,
// k_sample_filtered_rows passes 0: a row's noise then depends on its own
// seed and step only). The LDS below is the kernel's whole LDS footprint.
__device__ __forceinline__ RowDraw sample_filtered_row(
    const u16* __restrict__ row, int vocab, int top_k, float top_p,
    float temperature, u64 seed, u64 st, u64 hash_row) {
  __shared__ u64 mass1[NB1];
  __shared__ u32 cnt1[NB1];
  __shared__ u32 cnt2[NB2];
  __shared__ u64 red64[NW];
  __shared__ u32 red32[NW];
  __shared__ u64 sh_mass;
  __shared__ int sh_bin;
  __shared__ u32 sh_a, sh_b;
  __shared__ float rv[NW];
  __shared__ int ri[NW];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;

  for (int i = tid; i < NB1; i += NT) { cnt1[i] = 0; mass1[i] = 0; }
  if (tid < NB2) cnt2[tid] = 0;
  if (tid == 0) { sh_bin = 0; sh_a = 0; sh_b = 0; sh_mass = 0; }
  __syncthreads();

  // ---- P1: key range + level-1 counts --------------------------------
  u32 kmax = 0, kmin = 0xffffu;
  for_each_elem(row, vocab, [&](int, u16 u) {
    const u32 k = bf_key(u);
    kmax = max(kmax, k);
    kmin = min(kmin, k);
    atomicAdd(&cnt1[k >> 4], 1u);
  });
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    kmax = max(kmax, (u32)__shfl_xor((int)kmax, off));
    kmin = min(kmin, (u32)__shfl_xor((int)kmin, off));
  }
  if (lane == 0) { red32[wid] = kmax; ((u32*)red64)[wid] = kmin; }
  __syncthreads();                       // also publishes cnt1
  for (int w = 0; w < NW; ++w) {
    kmax = max(kmax, red32[w]);
    kmin = min(kmin, ((u32*)red64)[w]);
  }
  __syncthreads();
  const float vmax = bf2f(key_bf(kmax));

  const bool k_on = top_k > 0 && top_k < vocab;
  const bool p_on = top_p < 1.f;
  u32 thr = kmin;                        // smallest kept key
  u32 kept = (u32)vocab;

  u32 c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = cnt1[tid * 4 + j];

  // top-k set K = {bin > hb_k} U {bin == hb_k, key&15 >= lo_k}
  int hb_k = -1;
  u32 lo_k = 0;
  if (k_on) {
    // level 1: the highest bin whose inclusive suffix count reaches k
    const u32 tsum = c[0] + c[1] + c[2] + c[3];
    u32 tot;
    u32 above = block_suffix_excl<u32>(tsum, red32, &tot);
    const u32 k = (u32)top_k;
    if (above < k && above + tsum >= k) {
      for (int j = 3; j >= 0; --j) {
        if (above + c[j] >= k) { sh_bin = tid * 4 + j; sh_a = above; break; }
        above += c[j];
      }
    }
    __syncthreads();
    hb_k = sh_bin;
  }

  if (k_on || p_on) {
    // ---- P2: level-2 counts of bin hb_k; level-1 mass of bins above it ---
    for_each_elem(row, vocab, [&](int, u16 u) {
      const u32 k = bf_key(u);
      const int bin = (int)(k >> 4);
      if (bin == hb_k) atomicAdd(&cnt2[k & 15u], 1u);
      else if (p_on && bin > hb_k)
        atomicAdd((unsigned long long*)&mass1[bin], fx_mass(k, vmax));
    });
    __syncthreads();
  }

  if (k_on) {
    if (tid == 0) {
      // level 2: the k-th largest value itself (ties across it are kept)
      const u32 need = (u32)top_k - sh_a;
      u32 cum = 0;
      int lo = NB2 - 1;
      for (;; --lo) {
        cum += cnt2[lo];
        if (cum >= need || lo == 0) break;
      }
      sh_b = (u32)lo;
      sh_a += cum;                       // |K|
      if (p_on) {
        u64 m = 0;                       // mass of K inside bin hb_k
        for (int l = lo; l < NB2; ++l)
          m += (u64)cnt2[l] * fx_mass(((u32)hb_k << 4) | (u32)l, vmax);
        mass1[hb_k] = m;
      }
    }
    __syncthreads();
    lo_k = sh_b;
    kept = sh_a;
    thr = ((u32)hb_k << 4) | lo_k;
    __syncthreads();
  }

  if (p_on) {
    // level 1: lowest non-empty bin of K whose mass strictly above is < p*sum
    u64 m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = mass1[tid * 4 + j];
    u64 total;
    const u64 above = block_suffix_excl<u64>(m[0] + m[1] + m[2] + m[3],
                                             red64, &total);
    const double target = (double)top_p * (double)total;
    if (tid == 0) sh_bin = NB1;
    __syncthreads();
    u64 a = above, a_cand = 0;
    int cand = -1;
    for (int j = 3; j >= 0; --j) {
      const int bin = tid * 4 + j;
      if (bin >= hb_k && c[j] > 0 && (double)a < target) { cand = bin; a_cand = a; }
      a += m[j];
    }
    if (cand >= 0) atomicMin(&sh_bin, cand);
    __syncthreads();
    // (no candidate only if the row holds NaN/inf: keep the max group)
    const int hb_p = sh_bin < NB1 ? sh_bin : (int)(kmax >> 4);
    if (cand == hb_p) sh_mass = a_cand;  // exactly one thread owns that bin
    u32 cnt_hi = 0;                      // elements in bins above hb_p
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (tid * 4 + j > hb_p) cnt_hi += c[j];
    u32 cnt_above;
    block_suffix_excl<u32>(cnt_hi, red32, &cnt_above);

    u32 lo_floor = lo_k;
    if (hb_p != hb_k) {
      // ---- P3: level-2 counts of bin hb_p --------------------------------
      lo_floor = 0;
      if (tid < NB2) cnt2[tid] = 0;
      __syncthreads();
      for_each_elem(row, vocab, [&](int, u16 u) {
        const u32 k = bf_key(u);
        if ((int)(k >> 4) == hb_p) atomicAdd(&cnt2[k & 15u], 1u);
      });
      __syncthreads();
    }
    if (tid == 0) {
      u64 a2 = sh_mass;
      u32 in_bin = 0, lo_thr = NB2 - 1;
      for (int lo = NB2 - 1; lo >= (int)lo_floor; --lo) {
        const u32 n = cnt2[lo];
        if (!n) continue;
        if (!((double)a2 < target)) break;
        lo_thr = (u32)lo;
        in_bin += n;
        a2 += (u64)n * fx_mass(((u32)hb_p << 4) | (u32)lo, vmax);
      }
      sh_a = cnt_above + in_bin;
      sh_b = ((u32)hb_p << 4) | lo_thr;
    }
    __syncthreads();
    kept = sh_a;
    thr = sh_b;
  }

  // ---- draw: identical arithmetic to k_sample_onepass over the kept set --
  const float invT = temperature > 0.f ? 1.f / temperature : 1.f;
  float best = -1.0f / 0.0f;
  int besti = 0x7fffffff;
  for_each_elem(row, vocab, [&](int idx, u16 u) {
    if (bf_key(u) < thr) return;
    float v = bf2f(u) * invT;
    if (temperature > 0.f) {
      float r = hash_uniform(seed ^ (st * 0x51ed27f1ull) ^ (hash_row << 40) ^ (u64)idx);
      v += -__logf(-__logf(r));
    }
    if (v > best || (v == best && idx < besti)) { best = v; besti = idx; }
  });
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const int oi = __shfl_xor(besti, off);
    if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
  }
  if (lane == 0) { rv[wid] = best; ri[wid] = besti; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < NW; ++i)
      if (rv[i] > best || (rv[i] == best && ri[i] < besti)) {
        best = rv[i]; besti = ri[i];
      }
  }
  return RowDraw{besti, thr, kept};
}

}  // namespace
