// Prefill over a PAGED KV pool for gfx950: the RoPE + append and the causal
// MFMA attention of attn_prefill.hip / fei_kernels.hip with ONE difference —
// a K/V row is addressed through a block table instead of a contiguous
// [B,Hkv,max_seq,D] cache.
//
// Conventions (k_attn_decode_paged's): pools [num_blocks, Hkv, BS, D], BS a
// power of two; block_table [B, max_blocks] int32; row p of sequence b lives
// at pool[bt[b][p >> bs_log], hkv, p & (BS-1), :].
//
// Only entries of logical blocks below ceil(kv_end / BS) are ever read
// (kv_end = pos0 + rows of this q tile), and of the last such block only the
// rows below kv_end: production tables pad with -1, and pool rows past a
// sequence's length belong to nobody.
//
// Bit identity with the contiguous kernels is the contract
// (tests/test_prefill_paged_gpu.py): k_attn_prefill_paged<D> keeps
// k_attn_prefill<D>'s grid, wave -> row ownership, 64-key LDS tiles, both
// swizzles, zero padding, MFMA chains, online softmax, P reshape and
// epilogue expression for expression. That text now lives in
// attn_prefill_core.h (k_attn_prefill and the ragged kernel are built on it);
// this kernel keeps its own copy because on the core it measured slower
// (profiles/prefill_core.md). When the core changes, change this copy.
#include "fei_common.h"

namespace {

// ---------------------------------------------------------------------------
// RoPE (prefill) + paged KV append for S tokens. q [B,S,Hq,D] roped in place;
// k [B,S,Hkv,D] roped + appended with v at logical row pos0[b]+s.
// Grid: (S, Hq+Hkv, B); block D/2. Same expressions as k_rope_kv_prefill.
// ---------------------------------------------------------------------------
__global__ void k_rope_kv_prefill_paged(
    u16* __restrict__ q, const u16* __restrict__ k, const u16* __restrict__ v,
    u16* __restrict__ kp, u16* __restrict__ vp,
    const int* __restrict__ block_table, const float* __restrict__ cos_sin,
    const int* __restrict__ pos0, int B, int S, int Hq, int Hkv, int D,
    int bs_log, int max_blocks, long q_ts, long kv_ts) {
  const int s_idx = blockIdx.x;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int i = threadIdx.x;
  const int p = pos0[b] + s_idx;
  const long tok = (long)b * S + s_idx;
  const float c = cos_sin[((long)p * (D / 2) + i) * 2 + 0];
  const float sn = cos_sin[((long)p * (D / 2) + i) * 2 + 1];
  if (h < Hq) {
    u16* qp = q + tok * q_ts + (long)h * D;
    float x1 = bf2f(qp[i]), x2 = bf2f(qp[i + D / 2]);
    qp[i] = f2bf(x1 * c - x2 * sn);
    qp[i + D / 2] = f2bf(x2 * c + x1 * sn);
  } else {
    const int hk = h - Hq;
    const u16* kin = k + tok * kv_ts + (long)hk * D;
    const u16* vin = v + tok * kv_ts + (long)hk * D;
    const int BS = 1 << bs_log;
    const int blk = block_table[(long)b * max_blocks + (p >> bs_log)];
    const long row = (((long)blk * Hkv + hk) * BS + (p & (BS - 1))) * D;
    u16* kcp = kp + row;
    u16* vcp = vp + row;
    float x1 = bf2f(kin[i]), x2 = bf2f(kin[i + D / 2]);
    kcp[i] = f2bf(x1 * c - x2 * sn);
    kcp[i + D / 2] = f2bf(x2 * c + x1 * sn);
    vcp[i] = vin[i];
    vcp[i + D / 2] = vin[i + D / 2];
  }
}

// ---------------------------------------------------------------------------
// Causal GQA prefill attention over the pool. grid (ceil(S/64), Hq, B), block
// 256 = 4 waves; see attn_prefill.hip for the structure and fragment maps.
//
// Table entries reach the staging loop through a 64-int LDS stage (bts, one
// physical block per key of the tile, 256 B): thread (tid & 63) loads the
// entry of key t*64 + (tid & 63) ONE TILE AHEAD into a register, right after
// the staging barrier, so the table -> row dependent load is in flight during
// the previous tile's MFMA work; wave 0 drops the registers into bts in front
// of the next tile's first barrier, and the staging loop reads bts[key].
//
// Resources: 40 KB + 256 B of LDS at D=128 still fits 3 workgroups per CU,
// which is what k_attn_prefill<128>'s registers allow (4 at D=64). The
// 64-bit row offsets cost a few VGPRs over the contiguous kernel, just past
// its occupancy step, so the waves-per-SIMD target is stated: the compiler
// meets it without scratch (profiles/paged_prefill.md has the numbers). The
// staging loop runs one trip at a time, as the compiler leaves
// k_attn_prefill's.
// ---------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 4, D == 128 ? 3 : 4)))
k_attn_prefill_paged(const u16* __restrict__ q, const u16* __restrict__ kp,
                     const u16* __restrict__ vp,
                     const int* __restrict__ block_table,
                     u16* __restrict__ out, const int* __restrict__ pos0,
                     int B, int S, int Hq, int Hkv, int bs_log,
                     int max_blocks, float scale, long q_ts) {
  constexpr int DC = D / 16;       // d-chunks (8 for D=128)
  constexpr int KS = D / 32;       // K-dim steps per QK^T mfma chain
  constexpr int KV = 64;           // keys per LDS tile (one barrier per 64)
  constexpr int NC = KV / 16;      // 16-key score chunks per tile
  constexpr int KA = KV / 32;      // P A-fragments per tile (K=32 each)
  constexpr int NIT = KV * D / 8 / 256;   // staging trips per thread
  const int qt = blockIdx.x;       // 64-row q tile
  const int hq = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x;
  const int w = tid >> 6;          // wave 0..3
  const int lane = tid & 63;
  const int l15 = lane & 15;
  const int lg = lane >> 4;        // 16-lane group 0..3

  // same tiles and swizzles as k_attn_prefill (attn_prefill.hip)
  __shared__ u16 kt[64][D];
  __shared__ u16 vtT[D][64];
  __shared__ u16 p_lds[4][16][64];
#define SWZ16(row, col8) ((col8) ^ ((row) & 7))
#define VT_OFF(col, key) \
  ((col) * 64 + \
   ((((key) >> 3) ^ ((col) & 7) ^ (((col) >> 3) & 7)) << 3) + ((key) & 7))

  const int p0 = pos0[b];
  const int q_hi = min(qt * 64 + 64, S);           // exclusive rel row bound
  const int kv_end = p0 + q_hi;

  // ---- load Q fragments (row = l&15 within this wave's 16-row block) ----
  const int qrow_rel = qt * 64 + w * 16 + l15;     // A-fragment row
  const int qrow_ld = min(qrow_rel, S - 1);        // clamp for tail
  s16x8 a_q[KS];
  {
    const u16* qp = q + ((long)b * S + qrow_ld) * q_ts + (long)hq * D + 8 * lg;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      a_q[ks] = *(const s16x8*)(qp + ks * 32);
  }

  // online-softmax state per C row r (replicated across the 16-lane group)
  float m_row[4], l_row[4];
  f32x4 o_acc[DC];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_row[r] = -1.0f / 0.0f; l_row[r] = 0.f; }
#pragma unroll
  for (int dc = 0; dc < DC; ++dc) o_acc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int BS = 1 << bs_log;
  const int* bt = block_table + (long)b * max_blocks;

  // physical block of key t*KV + (tid & 63); a key >= kv_end has none (its
  // table entry is never read, and neither is its bts slot)
  __shared__ int bts[KV];
  int blk_next;
  auto load_block = [&](int t) {
    const int kk = t * KV + (tid & 63);
    blk_next = kk < kv_end ? bt[kk >> bs_log] : 0;
  };
  load_block(0);

  const int ntiles = (kv_end + KV - 1) / KV;
  for (int t = 0; t < ntiles; ++t) {
    // ---- stage K/V tile (KV keys x D), zero-padded past kv_end ----------
    if (tid < KV) bts[tid] = blk_next;              // read after the barrier
    __syncthreads();                                // vt/kt reuse protection
    {
#pragma unroll 1
      for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * 256;
        const int key = i / (D / 8);
        const int col8 = i % (D / 8);
        const int kk = t * KV + key;
        const int dst = key * (D / 8) + SWZ16(key, col8);
        s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        s16x8 v8 = z;
        if (kk < kv_end) {
          const long row =
              (((long)bts[key] * Hkv + hkv) * BS + (kk & (BS - 1))) * D;
          ((s16x8*)kt)[dst] = *(const s16x8*)(kp + row + col8 * 8);
          v8 = *(const s16x8*)(vp + row + col8 * 8);
        } else {
          ((s16x8*)kt)[dst] = z;
        }
        // V transposed scatter (VT_OFF block swizzle)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          ((u16*)vtT)[VT_OFF(col8 * 8 + j, key)] = (u16)v8[j];
      }
    }
    __syncthreads();
    load_block(t + 1);             // past the last tile every key >= kv_end

    // ---- QK^T: NC 16-key chunks ---------------------------------------
    f32x4 sfrag[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int krow = c * 16 + l15;
        const int kcol8 = SWZ16(krow, ks * 4 + lg);
        const s16x8 b_k = *(const s16x8*)(&((s16x8*)kt)[krow * (D / 8) + kcol8]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_q[ks], b_k, acc, 0, 0, 0);
      }
      sfrag[c] = acc;
    }

    // ---- mask + online softmax ----------------------------------------
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
        if (key >= kv_end || key > qrow_abs) sv[c] = -1.0f / 0.0f;
        mx = fmaxf(mx, sv[c]);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      const float m_new = fmaxf(m_row[r], mx);
      alpha[r] = __expf(m_row[r] - m_new);          // 0 on first tile
      m_row[r] = m_new;
      float psum = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        p_val[c][r] = (sv[c] == -1.0f / 0.0f) ? 0.f : __expf(sv[c] - m_new);
        psum += p_val[c][r];
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) psum += __shfl_xor(psum, off);
      l_row[r] = l_row[r] * alpha[r] + psum;
    }

    // ---- rescale O, stage P (C-layout -> A-layout via LDS) -------------
#pragma unroll
    for (int dc = 0; dc < DC; ++dc)
#pragma unroll
      for (int r = 0; r < 4; ++r) o_acc[dc][r] *= alpha[r];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p_lds[w][4 * lg + r][c * 16 + l15] = f2bf(p_val[c][r]);
    // same-wave LDS RAW: compiler inserts lgkmcnt waits; no barrier needed
    // (p_lds[w] is private to wave w).

    // ---- PV: KA P-fragments of K=32 each -------------------------------
    s16x8 a_p[KA];
#pragma unroll
    for (int ka = 0; ka < KA; ++ka)
      a_p[ka] = *(const s16x8*)(&p_lds[w][l15][ka * 32 + 8 * lg]);
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
      const int col = dc * 16 + l15;
#pragma unroll
      for (int ka = 0; ka < KA; ++ka) {
        // 8 consecutive keys of this column = one 16-byte read
        const s16x8 b_v = *(const s16x8*)(
            &((u16*)vtT)[VT_OFF(col, ka * 32 + 8 * lg)]);
        o_acc[dc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_p[ka], b_v,
                                                            o_acc[dc], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: O / l, store ------------------------------------------
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int srow = qt * 64 + w * 16 + 4 * lg + r;
    if (srow >= S) continue;
    const float inv_l = l_row[r] > 0.f ? 1.f / l_row[r] : 0.f;
    u16* orow = out + (((long)b * S + srow) * Hq + hq) * D;
#pragma unroll
    for (int dc = 0; dc < DC; ++dc)
      orow[dc * 16 + l15] = f2bf(o_acc[dc][r] * inv_l);
  }
#undef SWZ16
#undef VT_OFF
}

// log2 of a power-of-two block size, -1 for anything else
int block_size_log2(int block_size) {
  if (block_size <= 0 || (block_size & (block_size - 1)) != 0) return -1;
  int bs_log = 0;
  while ((1 << bs_log) < block_size) ++bs_log;
  return bs_log;
}

}  // namespace

extern "C" {

// Both return 0 when launched and non-zero when they refuse (nothing is
// launched then): 1 = empty problem (B, S <= 0), 2 = head counts, 3 = head
// size without a kernel instance, 4 = block size not a power of two.

int fei_rope_kv_prefill_paged(void* q, const void* k, const void* v,
                              void* k_pool, void* v_pool,
                              const int* block_table, const float* cos_sin,
                              const int* pos0, int B, int S, int Hq, int Hkv,
                              int D, int block_size, int max_blocks,
                              long q_ts, long kv_ts, hipStream_t stream) {
  if (B <= 0 || S <= 0 || max_blocks <= 0) return 1;
  if (Hq <= 0 || Hkv <= 0) return 2;
  if (D != 64 && D != 128) return 3;
  const int bs_log = block_size_log2(block_size);
  if (bs_log < 0) return 4;
  hipLaunchKernelGGL(k_rope_kv_prefill_paged, dim3(S, Hq + Hkv, B),
                     dim3(D / 2), 0, stream, (u16*)q, (const u16*)k,
                     (const u16*)v, (u16*)k_pool, (u16*)v_pool, block_table,
                     cos_sin, pos0, B, S, Hq, Hkv, D, bs_log, max_blocks,
                     q_ts, kv_ts);
  return 0;
}

int fei_attn_prefill_paged(const void* q, const void* k_pool,
                           const void* v_pool, const int* block_table,
                           void* out, const int* pos0, int B, int S, int Hq,
                           int Hkv, int D, int block_size, int max_blocks,
                           float scale, long q_ts, hipStream_t stream) {
  if (B <= 0 || S <= 0 || max_blocks <= 0) return 1;
  if (Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0) return 2;
  if (D != 64 && D != 128) return 3;
  const int bs_log = block_size_log2(block_size);
  if (bs_log < 0) return 4;
  dim3 grid((S + 63) / 64, Hq, B);
  if (D == 128) {
    hipLaunchKernelGGL(k_attn_prefill_paged<128>, grid, dim3(256), 0, stream,
                       (const u16*)q, (const u16*)k_pool, (const u16*)v_pool,
                       block_table, (u16*)out, pos0, B, S, Hq, Hkv, bs_log,
                       max_blocks, scale, q_ts);
  } else {
    hipLaunchKernelGGL(k_attn_prefill_paged<64>, grid, dim3(256), 0, stream,
                       (const u16*)q, (const u16*)k_pool, (const u16*)v_pool,
                       block_table, (u16*)out, pos0, B, S, Hq, Hkv, bs_log,
                       max_blocks, scale, q_ts);
  }
  return 0;
}

}  // extern "C"
