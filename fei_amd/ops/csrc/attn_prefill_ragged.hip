// RAGGED prefill over a paged KV pool for gfx950: the RoPE + append and the
// causal MFMA attention of attn_prefill_paged.hip for a PACKED batch of
// sequences of unequal length, in one launch each.
//
// Layout: the tokens of all B sequences are packed back to back. q is
// [T, Hq, D] with token stride q_ts, k and v are [T, Hkv, D] with token stride
// kv_ts, out is [T, Hq, D] contiguous; T = sum(len_b). Sequence b owns the
// packed rows [cu[b], cu[b+1]); its row s is logical KV row pos0[b] + s,
// reached through row b of block_table [B, max_blocks]. Pools as in
// attn_prefill_paged.hip: [num_blocks, Hkv, BS, D], BS a power of two.
//
// Work list instead of a (q tile, head, batch) grid: blockIdx.x indexes a
// host-built tile map of (sequence, q tile) int32 pairs, n_tiles =
// sum(ceil(len_b / 64)), q tiles counted from the sequence's OWN start, so
// no workgroup is launched for rows nobody owns. The append finds a token's
// sequence in a per-token int32 map (tok_seq [T]), also host-built.
//
// For sequence b only table entries of logical blocks below
// ceil((pos0[b] + len_b) / BS) are read, and of the pool only rows below
// pos0[b] + len_b; q rows are clamped to the sequence's last row and out
// rows are guarded by len_b, so a tail tile neither reads nor writes a
// neighbouring sequence's packed rows.
//
// Bit identity with the uniform paged kernels is the contract
// (tests/test_prefill_ragged_gpu.py): per sequence the rows are bit-equal to
// k_rope_kv_prefill_paged / k_attn_prefill_paged<D> run with B = 1 on that
// sequence alone. k_attn_prefill_paged_ragged<D> is k_attn_prefill_paged<D>
// with S := len_b and the q/out base := cu[b]; its tiles, swizzles, table
// stage, MFMA chains, softmax and epilogue are the shared tile core
// (attn_prefill_core.h), of which k_attn_prefill_paged<D> keeps a copy. When
// the core or the staging loop below changes, change attn_prefill_paged.hip.
#include "attn_prefill_core.h"

namespace {

// ---------------------------------------------------------------------------
// RoPE (prefill) + paged KV append for T packed tokens. q [T,Hq,D] roped in
// place; k [T,Hkv,D] roped + appended with v at logical row pos0[b] + s of
// sequence b = tok_seq[token], s = token - cu[b].
// Grid: (T, Hq+Hkv); block D/2. Same expressions as k_rope_kv_prefill_paged.
// ---------------------------------------------------------------------------
__global__ void k_rope_kv_prefill_paged_ragged(
    u16* __restrict__ q, const u16* __restrict__ k, const u16* __restrict__ v,
    u16* __restrict__ kp, u16* __restrict__ vp,
    const int* __restrict__ block_table, const float* __restrict__ cos_sin,
    const int* __restrict__ pos0, const int* __restrict__ cu,
    const int* __restrict__ tok_seq, int Hq, int Hkv, int D, int bs_log,
    int max_blocks, long q_ts, long kv_ts) {
  const long tok = blockIdx.x;
  const int h = blockIdx.y;
  const int b = tok_seq[tok];
  const int i = threadIdx.x;
  const int p = pos0[b] + ((int)tok - cu[b]);
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
// Causal GQA prefill attention over the pool for a packed batch. grid
// (n_tiles, Hq), block 256 = 4 waves; tile_map[2*i] = sequence, [2*i+1] = q
// tile of work item i. Tiles, table stage, compute and epilogue are the tile
// core's (attn_prefill_core.h); the slot fetch is k_attn_prefill_paged's.
// The staging loop runs one trip at a time, as the compiler leaves
// k_attn_prefill's.
//
// Resources: as k_attn_prefill_paged<D> (40 KB + 256 B of LDS at D=128, 3
// workgroups per CU; 4 at D=64); the sequence's bounds and bases are
// workgroup-uniform and live in SGPRs. The waves-per-SIMD target is stated
// as there (profiles/ragged_prefill.md has the numbers).
// ---------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(prefill::WAVES_PER_SIMD<D>,
                                   prefill::WAVES_PER_SIMD<D>)))
k_attn_prefill_paged_ragged(const u16* __restrict__ q,
                            const u16* __restrict__ kp,
                            const u16* __restrict__ vp,
                            const int* __restrict__ block_table,
                            u16* __restrict__ out,
                            const int* __restrict__ pos0,
                            const int* __restrict__ cu,
                            const int* __restrict__ tile_map, int Hq, int Hkv,
                            int bs_log, int max_blocks, float scale,
                            long q_ts) {
  using namespace prefill;
  constexpr int NIT = KV * D / 8 / 256;            // staging trips per thread
  const int b = tile_map[2 * blockIdx.x];          // sequence
  const int qt = tile_map[2 * blockIdx.x + 1];     // its 64-row q tile
  const int hq = blockIdx.y;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x;
  const long tok0 = cu[b];                         // first packed row
  const int S = cu[b + 1] - (int)tok0;             // len_b
  const int p0 = pos0[b];
  const int kv_end = p0 + min(qt * 64 + 64, S);    // exclusive key bound
  const int BS = 1 << bs_log;
  const int* bt = block_table + (long)b * max_blocks;

  __shared__ Tiles<D> T;
  __shared__ int bts[KV];
  Wave<D> st;
  wave_init<D>(st, q, tok0, qt, S, hq, q_ts);
  int blk_next = table_load(bt, 0, kv_end, bs_log);

  const int ntiles = (kv_end + KV - 1) / KV;
  for (int t = 0; t < ntiles; ++t) {
    // ---- stage K/V tile (KV keys x D), zero-padded past kv_end ----------
    table_publish(bts, blk_next);                   // read after the barrier
    __syncthreads();                                // vt/kt reuse protection
#pragma unroll 1
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256;
      const int key = i / (D / 8);
      const int col8 = i % (D / 8);
      const int kk = t * KV + key;
      s16x8 k8 = {0, 0, 0, 0, 0, 0, 0, 0};
      s16x8 v8 = k8;
      if (kk < kv_end) {
        const long row =
            (((long)bts[key] * Hkv + hkv) * BS + (kk & (BS - 1))) * D;
        k8 = *(const s16x8*)(kp + row + col8 * 8);
        v8 = *(const s16x8*)(vp + row + col8 * 8);
      }
      store_slot<D>(T, key, col8, k8, v8);
    }
    __syncthreads();
    blk_next = table_load(bt, t + 1, kv_end, bs_log);
    tile_compute<D>(st, T, t, kv_end, p0, qt, scale, 1);
  }
  epilogue<D>(st, out, tok0, qt, S, hq, Hq);
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
// launched then), with fei_attn_prefill_paged's codes: 1 = empty problem
// (T, B, n_tiles <= 0), 2 = head counts, 3 = head size without a kernel
// instance, 4 = block size not a power of two.

int fei_rope_kv_prefill_paged_ragged(
    void* q, const void* k, const void* v, void* k_pool, void* v_pool,
    const int* block_table, const float* cos_sin, const int* pos0,
    const int* cu, const int* tok_seq, int T, int B, int Hq, int Hkv, int D,
    int block_size, int max_blocks, long q_ts, long kv_ts,
    hipStream_t stream) {
  if (T <= 0 || B <= 0 || max_blocks <= 0) return 1;
  if (Hq <= 0 || Hkv <= 0) return 2;
  if (D != 64 && D != 128) return 3;
  const int bs_log = block_size_log2(block_size);
  if (bs_log < 0) return 4;
  hipLaunchKernelGGL(k_rope_kv_prefill_paged_ragged, dim3(T, Hq + Hkv),
                     dim3(D / 2), 0, stream, (u16*)q, (const u16*)k,
                     (const u16*)v, (u16*)k_pool, (u16*)v_pool, block_table,
                     cos_sin, pos0, cu, tok_seq, Hq, Hkv, D, bs_log,
                     max_blocks, q_ts, kv_ts);
  return 0;
}

int fei_attn_prefill_paged_ragged(
    const void* q, const void* k_pool, const void* v_pool,
    const int* block_table, void* out, const int* pos0, const int* cu,
    const int* tile_map, int n_tiles, int T, int B, int Hq, int Hkv, int D,
    int block_size, int max_blocks, float scale, long q_ts,
    hipStream_t stream) {
  if (T <= 0 || B <= 0 || n_tiles <= 0 || max_blocks <= 0) return 1;
  if (Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0) return 2;
  if (D != 64 && D != 128) return 3;
  const int bs_log = block_size_log2(block_size);
  if (bs_log < 0) return 4;
  dim3 grid(n_tiles, Hq);
  if (D == 128) {
    hipLaunchKernelGGL(k_attn_prefill_paged_ragged<128>, grid, dim3(256), 0,
                       stream, (const u16*)q, (const u16*)k_pool,
                       (const u16*)v_pool, block_table, (u16*)out, pos0, cu,
                       tile_map, Hq, Hkv, bs_log, max_blocks, scale, q_ts);
  } else {
    hipLaunchKernelGGL(k_attn_prefill_paged_ragged<64>, grid, dim3(256), 0,
                       stream, (const u16*)q, (const u16*)k_pool,
                       (const u16*)v_pool, block_table, (u16*)out, pos0, cu,
                       tile_map, Hq, Hkv, bs_log, max_blocks, scale, q_ts);
  }
  return 0;
}

}  // extern "C"
