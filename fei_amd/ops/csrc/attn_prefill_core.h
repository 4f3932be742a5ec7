// Tile core of the flash-style MFMA prefill attention kernels for gfx950
// (mfma_f32_16x16x32_bf16, LDS-staged K/V tiles, online softmax). ONE
// definition of the tiles, the swizzles, the per-wave state, the slot store,
// the tile compute, the epilogue and the block-table stage, used by
//   k_attn_prefill              attn_prefill.hip         contiguous bf16
//   k_attn_prefill_paged_ragged attn_prefill_ragged.hip  paged bf16, packed
// A kernel keeps only what is its own: where b / qt / S and the q/out row
// base come from, and how a slot's 8 K and 8 V values are fetched.
//
// NOT on the core, each still a full copy of this text that has to be kept in
// step with it by hand (the cross-kernel bit-equality GPU tests check it):
//   k_attn_prefill_paged        attn_prefill_paged.hip   paged bf16
//   k_attn_prefill_kv8          kv_fp8.hip               contiguous fp8
//   k_attn_prefill_paged_kv8    kv_fp8_paged.hip         paged fp8
// On the core these three had the same registers, LDS and results, but
// measured 0.8 % to 2.5 % slower than their copies in at least one head size
// (profiles/prefill_core.md), so they stay as they were.
//
// Structure: block 256 = 4 waves; a workgroup owns one 64-row q tile of one
// head, wave w its rows [qt*64 + 16w, +16). K/V tiles of 64 keys are staged
// in LDS and shared by the 4 waves. Per tile: QK^T = D/32 MFMAs per 16-key
// chunk, per-row online softmax in registers (16-lane shfl groups), P staged
// through LDS to re-shape C-layout -> A-layout, PV = 2 MFMAs per 16 columns.
//
// Fragment maps (verified on hardware by k_mfma_probe / test_ops_gpu):
//   A[16x32]: lane l -> A[l&15][8*(l>>4)+j], j=0..7
//   B[32x16]: lane l -> B[8*(l>>4)+j][l&15]
//   C[16x16]: lane l, reg r -> C[4*(l>>4)+r][l&15]
//
// Everything here is force-inlined into the calling kernel: the tiles are a
// __shared__ object of the kernel, passed by reference.
#pragma once
#include "fei_common.h"

namespace prefill {

constexpr int KV = 64;          // keys per LDS tile (one barrier per 64)
constexpr int NC = KV / 16;     // 16-key score chunks per tile
constexpr int KA = KV / 32;     // P A-fragments per tile (K=32 each)
template <int D> constexpr int DC = D / 16;   // d-chunks (8 for D=128)
template <int D> constexpr int KS = D / 32;   // K steps per QK^T mfma chain
// waves per SIMD the registers allow; the ragged kernel states it as its
// target (minimum and maximum, like k_attn_prefill_paged)
template <int D> constexpr int WAVES_PER_SIMD = D == 128 ? 3 : 4;

// K tile: row-major with a T2 XOR swizzle (guide Guideline 4): read
// column-slice-wise with ds_read_b128, swizzling the 16-byte slot index by
// (row&7) spreads each 16-lane group over 8 slots.
// V tile: stored TRANSPOSED [col][key] in 8-key blocks so the PV B-fragment
// (8 consecutive keys of one column) is ONE 16-byte vector read — the r02
// ablation (experimental/prefill_ablate.hip) measured the per-element PV
// gather at 56% of the kernel. The 8-key block index is XOR-swizzled by
// (col&7) to break the 128-byte column stride's bank pattern (<=2-way). The
// transpose cost moves to the staging scatter: 8 ds_write_b16 per global
// vec8 — 4x fewer LDS ops than the per-element PV reads they replace.
// p_lds[w] is private to wave w.
template <int D>
struct Tiles {
  u16 kt[KV][D];
  u16 vtT[D][KV];
  u16 p_lds[4][16][KV];
};

// 16-byte slot of (row, col8) within a kt row
__device__ __forceinline__ constexpr int swz16(int row, int col8) {
  return col8 ^ (row & 7);
}
// u16 offset of (col, key) within vtT
__device__ __forceinline__ constexpr int vt_off(int col, int key) {
  return col * 64 + (((key >> 3) ^ (col & 7) ^ ((col >> 3) & 7)) << 3) +
         (key & 7);
}

// Per-wave state: the Q A-fragments and the online-softmax state per C row r
// (replicated across the 16-lane group).
template <int D>
struct Wave {
  s16x8 a_q[KS<D>];
  float m_row[4], l_row[4];
  f32x4 o_acc[DC<D>];
};

// Reset the softmax state and load the Q fragments (row = l&15 within this
// wave's 16-row block). row0 = first q/out row of the sequence: b * S, or
// cu[b] in a packed batch. Rows past S are clamped to the sequence's last.
template <int D>
__device__ __forceinline__ void wave_init(Wave<D>& st,
                                          const u16* __restrict__ q, long row0,
                                          int qt, int S, int hq, long q_ts) {
  const int w = threadIdx.x >> 6, l15 = threadIdx.x & 15;
  const int lg = (threadIdx.x & 63) >> 4;
  const int qrow_rel = qt * 64 + w * 16 + l15;     // A-fragment row
  const int qrow_ld = min(qrow_rel, S - 1);        // clamp for tail
  const u16* qp = q + (row0 + qrow_ld) * q_ts + (long)hq * D + 8 * lg;
#pragma unroll
  for (int ks = 0; ks < KS<D>; ++ks)
    st.a_q[ks] = *(const s16x8*)(qp + ks * 32);
#pragma unroll
  for (int r = 0; r < 4; ++r) { st.m_row[r] = -1.0f / 0.0f; st.l_row[r] = 0.f; }
#pragma unroll
  for (int dc = 0; dc < DC<D>; ++dc) st.o_acc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Store slot (key, col8) of the tile: 8 K values into the swizzled kt slot, 8
// V values scattered into the transposed vtT. The caller passes zeros for a
// key >= kv_end.
template <int D>
__device__ __forceinline__ void store_slot(Tiles<D>& T, int key, int col8,
                                           s16x8 k8, s16x8 v8) {
  ((s16x8*)T.kt)[key * (D / 8) + swz16(key, col8)] = k8;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    ((u16*)T.vtT)[vt_off(col8 * 8 + j, key)] = (u16)v8[j];
}

// One staged tile t: QK^T, mask + online softmax, O rescale, P reshape, PV.
// Keys >= kv_end are masked; with `causal` also keys past the row's own
// position p0 + row. Call between the staging barrier and the next tile's.
template <int D>
__device__ __forceinline__ void tile_compute(Wave<D>& st, Tiles<D>& T, int t,
                                             int kv_end, int p0, int qt,
                                             float scale, int causal) {
  const int w = threadIdx.x >> 6, l15 = threadIdx.x & 15;
  const int lg = (threadIdx.x & 63) >> 4;

  // ---- QK^T: NC 16-key chunks -----------------------------------------
  f32x4 sfrag[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS<D>; ++ks) {
      const int krow = c * 16 + l15;
      const int kcol8 = swz16(krow, ks * 4 + lg);
      const s16x8 b_k = ((const s16x8*)T.kt)[krow * (D / 8) + kcol8];
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(st.a_q[ks], b_k, acc, 0, 0,
                                                    0);
    }
    sfrag[c] = acc;
  }

  // ---- mask + online softmax ------------------------------------------
  float p_val[NC][4];
  float alpha[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow_abs = p0 + qt * 64 + w * 16 + 4 * lg + r;
    float sv[NC];
    float mx = -1.0f / 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      sv[c] = sfrag[c][r] * scale;
      const int key = t * KV + c * 16 + l15;
      if (key >= kv_end || (causal && key > qrow_abs)) sv[c] = -1.0f / 0.0f;
      mx = fmaxf(mx, sv[c]);
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float m_new = fmaxf(st.m_row[r], mx);
    alpha[r] = __expf(st.m_row[r] - m_new);        // 0 on first tile
    st.m_row[r] = m_new;
    float psum = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      p_val[c][r] = (sv[c] == -1.0f / 0.0f) ? 0.f : __expf(sv[c] - m_new);
      psum += p_val[c][r];
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) psum += __shfl_xor(psum, off);
    st.l_row[r] = st.l_row[r] * alpha[r] + psum;
  }

  // ---- rescale O, stage P (C-layout -> A-layout via LDS) ---------------
#pragma unroll
  for (int dc = 0; dc < DC<D>; ++dc)
#pragma unroll
    for (int r = 0; r < 4; ++r) st.o_acc[dc][r] *= alpha[r];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      T.p_lds[w][4 * lg + r][c * 16 + l15] = f2bf(p_val[c][r]);
  // same-wave LDS RAW: compiler inserts lgkmcnt waits; no barrier needed
  // (p_lds[w] is private to wave w).

  // ---- PV: KA P-fragments of K=32 each ---------------------------------
  s16x8 a_p[KA];
#pragma unroll
  for (int ka = 0; ka < KA; ++ka)
    a_p[ka] = *(const s16x8*)(&T.p_lds[w][l15][ka * 32 + 8 * lg]);
#pragma unroll
  for (int dc = 0; dc < DC<D>; ++dc) {
    const int col = dc * 16 + l15;
#pragma unroll
    for (int ka = 0; ka < KA; ++ka) {
      // 8 consecutive keys of this column = one 16-byte read
      const s16x8 b_v = *(const s16x8*)(
          &((const u16*)T.vtT)[vt_off(col, ka * 32 + 8 * lg)]);
      st.o_acc[dc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_p[ka], b_v, st.o_acc[dc], 0, 0, 0);
    }
  }
}

// Epilogue: O / l, bf16 store of the rows below S. out is [rows, Hq, D]
// contiguous; row0 as in wave_init.
template <int D>
__device__ __forceinline__ void epilogue(const Wave<D>& st,
                                         u16* __restrict__ out, long row0,
                                         int qt, int S, int hq, int Hq) {
  const int w = threadIdx.x >> 6, l15 = threadIdx.x & 15;
  const int lg = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int srow = qt * 64 + w * 16 + 4 * lg + r;
    if (srow >= S) continue;
    const float inv_l = st.l_row[r] > 0.f ? 1.f / st.l_row[r] : 0.f;
    u16* orow = out + ((row0 + srow) * Hq + hq) * D;
#pragma unroll
    for (int dc = 0; dc < DC<D>; ++dc)
      orow[dc * 16 + l15] = f2bf(st.o_acc[dc][r] * inv_l);
  }
}

// ---------------------------------------------------------------------------
// Block-table stage of a paged kernel. Table entries reach the staging
// loop through a 64-int LDS array (bts, one physical block per key of the
// tile, 256 B): thread (tid & 63) loads the entry of key t*64 + (tid & 63)
// ONE TILE AHEAD into a register with table_load, right after the staging
// barrier, so the table -> row dependent load is in flight during the
// previous tile's MFMA work; wave 0 drops the registers into bts with
// table_publish in front of the next tile's first barrier, and the staging
// loop reads bts[key]. A key >= kv_end has no block: its table entry is never
// read, and neither is its bts slot (past the last tile that is every key).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int table_load(const int* __restrict__ bt, int t,
                                          int kv_end, int bs_log) {
  const int kk = t * KV + (threadIdx.x & 63);
  return kk < kv_end ? bt[kk >> bs_log] : 0;
}
__device__ __forceinline__ void table_publish(int* bts, int blk_next) {
  if (threadIdx.x < KV) bts[threadIdx.x] = blk_next;
}

}  // namespace prefill
