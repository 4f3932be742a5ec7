// FP8 (OCP e4m3fn) KV cache for gfx950: append, split-K decode attention and
// MFMA prefill attention over a quantised cache.
//
// Storage format (fei_amd/ops/reference.py::quant_kv_fp8 is the definition):
// each cached row — the D elements of one (batch, kv-head, position) — is D
// e4m3fn codes plus one f32 scale:
//   data  u8  [B, Hkv, max_seq, D]       scale f32 [B, Hkv, max_seq]
//   scale = amax / 448 (1 when amax == 0), code = e4m3fn(x / scale) with an
//   IEEE f32 division (no fast-math flag in build.py: `/` is correctly
//   rounded), round-to-nearest-even, saturating.
// x is what the bf16 cache would have stored: K roped in f32 and rounded to
// bf16 first, V as given.
//
// The attention kernels are the fp8 counterparts of k_attn_decode
// (fei_kernels.hip) and k_attn_prefill (attn_prefill.hip): same grids, same
// LDS layouts, same f32 partials — so k_attn_decode_combine reduces the
// decode partials unchanged. Codes are dequantised with the hardware
// converter (v_cvt_pk_f32_fp8); the per-key scale is applied ONCE per key:
// to the finished K score, and folded into the probability staged for the
// P*V pass (the running sum l uses the unscaled probability).
// No kernel reads data or scales at positions >= its valid length.
// The row quantise/append helper, the G-wide block reduce and the staging
// dequantiser are shared with the paged kernels: kv_fp8_common.h.
#include "kv_fp8_common.h"

namespace {

// ---------------------------------------------------------------------------
// Append, decode form. Grid (Hq+Hkv, B), block 64 (one wave): q heads are
// roped in place, kv heads are roped + quantised + appended at pos[b].
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_rope_kv8_decode(u16* __restrict__ q, const u16* __restrict__ k,
                  const u16* __restrict__ v, u8* __restrict__ kd,
                  float* __restrict__ ks, u8* __restrict__ vd,
                  float* __restrict__ vs, const float* __restrict__ cos_sin,
                  const int* __restrict__ pos, int Hq, int Hkv, int D,
                  int max_seq, long q_bs, long kv_bs) {
  const int h = blockIdx.x;
  const int b = blockIdx.y;
  const int i = threadIdx.x;
  const int half = D / 2;
  const int p = pos[b];
  const float* cs = cos_sin + (long)p * half * 2;
  if (h < Hq) {
    if (i < half) {
      u16* qp = q + (long)b * q_bs + (long)h * D;
      const float c = cs[i * 2], s = cs[i * 2 + 1];
      const float x1 = bf2f(qp[i]), x2 = bf2f(qp[i + half]);
      qp[i] = f2bf(x1 * c - x2 * s);
      qp[i + half] = f2bf(x2 * c + x1 * s);
    }
  } else {
    const int hk = h - Hq;
    kv8_rope_append(k + (long)b * kv_bs + (long)hk * D,
                    v + (long)b * kv_bs + (long)hk * D, cs, D,
                    ((long)b * Hkv + hk) * max_seq + p, i, kd, ks, vd, vs);
  }
}

// Append, prefill form: S tokens at pos0[b]+s. Grid (S, Hq+Hkv, B), block 64.
__global__ void __launch_bounds__(64)
k_rope_kv8_prefill(u16* __restrict__ q, const u16* __restrict__ k,
                   const u16* __restrict__ v, u8* __restrict__ kd,
                   float* __restrict__ ks, u8* __restrict__ vd,
                   float* __restrict__ vs, const float* __restrict__ cos_sin,
                   const int* __restrict__ pos0, int S, int Hq, int Hkv, int D,
                   int max_seq, long q_ts, long kv_ts) {
  const int s_idx = blockIdx.x;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int i = threadIdx.x;
  const int half = D / 2;
  const int p = pos0[b] + s_idx;
  const long tok = (long)b * S + s_idx;
  const float* cs = cos_sin + (long)p * half * 2;
  if (h < Hq) {
    if (i < half) {
      u16* qp = q + tok * q_ts + (long)h * D;
      const float c = cs[i * 2], sn = cs[i * 2 + 1];
      const float x1 = bf2f(qp[i]), x2 = bf2f(qp[i + half]);
      qp[i] = f2bf(x1 * c - x2 * sn);
      qp[i + half] = f2bf(x2 * c + x1 * sn);
    }
  } else {
    const int hk = h - Hq;
    kv8_rope_append(k + tok * kv_ts + (long)hk * D,
                    v + tok * kv_ts + (long)hk * D, cs, D,
                    ((long)b * Hkv + hk) * max_seq + p, i, kd, ks, vd, vs);
  }
}

// ---------------------------------------------------------------------------
// Split-K decode attention over the fp8 cache. Grid (splits, Hkv, B), block
// 256; the length n = pos[b]+1 is read on the device. Structure and LDS are
// those of k_attn_decode; what differs:
//   phase A: a key row is D bytes (D/16 16-byte loads); the raw score is
//            multiplied once by k_scale[key].
//   phase B: ONE V lane map for every chunk length — 8 codes (8 B) per lane,
//            D/8 lanes per row, and the tile's keys INTERLEAVED over the
//            256/(D/8) key-groups (key j*kgroups + kg). A wave's four
//            key-groups then read four adjacent rows (512 contiguous bytes),
//            and every key-group has work as soon as the chunk holds
//            `kgroups` keys (16 at D=128), so the bf16 kernel's separate
//            short-chunk pair map (needed there because its blocked key
//            assignment idles 15 of 16 groups on a 16-key chunk) has no job
//            left. p staged in LDS carries v_scale[key].
// ROPE=true fuses the step's RoPE + KV-append: wave 0 of the split that owns
// key n-1 quantises and writes the row before the block barrier, then every
// thread reads it back like any other key (same-workgroup visibility).
// Always followed by the separate k_attn_decode_combine launch.
// ---------------------------------------------------------------------------
template <int G, bool ROPE>
__global__ void __launch_bounds__(256)
k_attn_decode_kv8(const u16* __restrict__ q, u8* __restrict__ kd,
                  float* __restrict__ ksc, u8* __restrict__ vd,
                  float* __restrict__ vsc, float* __restrict__ part_o,
                  float* __restrict__ part_ml, const int* __restrict__ pos,
                  int Hq, int Hkv, int D, int max_seq, int splits,
                  float scale, long q_bs, const u16* __restrict__ kin,
                  const u16* __restrict__ vin,
                  const float* __restrict__ cos_sin, long kv_bs) {
  const int split = blockIdx.x;
  const int hkv = blockIdx.y;
  const int b = blockIdx.z;
  const int tid = threadIdx.x;

  __shared__ float qs[DEC8_GMAX][DEC8_DMAX];
  __shared__ float pl[DEC8_GMAX][DEC8_TILE];
  __shared__ float red[DEC8_GMAX][4];
  __shared__ float osh[DEC8_TILE][8];

  const int n = pos[b] + 1;
  const int chunk = (n + splits - 1) / splits;
  const int start = split * chunk;
  const int end = min(start + chunk, n);

  if (start >= end) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int hq = hkv * G + g;
      float* po = part_o + (((long)b * Hq + hq) * splits + split) * D;
      float* pml = part_ml + (((long)b * Hq + hq) * splits + split) * 2;
      for (int d = tid; d < D; d += blockDim.x) po[d] = 0.f;
      if (tid == 0) { pml[0] = -1.0f / 0.0f; pml[1] = 0.f; }
    }
    return;
  }

  const int half = D / 2;
  const int p_new = n - 1;
  const long row0 = ((long)b * Hkv + hkv) * max_seq;
  if (ROPE) {
    const float* cs = cos_sin + (long)p_new * half * 2;
    for (int i = tid; i < G * half; i += blockDim.x) {
      const int g = i / half, d = i % half;
      const float c = cs[d * 2 + 0];
      const float sn = cs[d * 2 + 1];
      const u16* qp = q + (long)b * q_bs + (long)(hkv * G + g) * D;
      const float x1 = bf2f(qp[d]);
      const float x2 = bf2f(qp[d + half]);
      qs[g][d] = (x1 * c - x2 * sn) * scale;
      qs[g][d + half] = (x2 * c + x1 * sn) * scale;
    }
    // no other split's [start, end) range touches key p_new
    if (p_new >= start && p_new < end && tid < 64)
      kv8_rope_append(kin + (long)b * kv_bs + (long)hkv * D,
                      vin + (long)b * kv_bs + (long)hkv * D, cs, D,
                      row0 + p_new, tid, kd, ksc, vd, vsc);
  } else {
    for (int i = tid; i < G * D; i += blockDim.x) {
      const int g = i / D, d = i % D;
      qs[g][d] = bf2f(q[(long)b * q_bs + (long)(hkv * G + g) * D + d]) * scale;
    }
  }
  __syncthreads();

  const u8* kbase = kd + row0 * D;
  const u8* vbase = vd + row0 * D;
  const float* ksb = ksc + row0;
  const float* vsb = vsc + row0;

  const int dvecs = D / 8;                        // lanes per V row
  const int kgroups = blockDim.x / dvecs;         // 16 at D=128, 32 at D=64
  const int dv = tid % dvecs;
  const int kg = tid / dvecs;

  float m[DEC8_GMAX], l[DEC8_GMAX], sc[DEC8_GMAX];
  float oa[DEC8_GMAX][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -1.0f / 0.0f; l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) oa[g][e] = 0.f;
  }

  for (int tile = start; tile < end; tile += DEC8_TILE) {
    const int kk = tile + tid;
    float vscale = 0.f;
    if (kk < end) {
      const u32x4* krow = (const u32x4*)(kbase + (long)kk * D);
      const float kscale = ksb[kk];
      vscale = vsb[kk];
#pragma unroll
      for (int g = 0; g < G; ++g) sc[g] = 0.f;
      for (int i = 0; i < D / 16; ++i) {
        const u32x4 k16 = krow[i];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(k16[w], false);
          const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(k16[w], true);
          const int d0 = i * 16 + w * 4;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            sc[g] = fmaf(qs[g][d0 + 0], lo[0], sc[g]);
            sc[g] = fmaf(qs[g][d0 + 1], lo[1], sc[g]);
            sc[g] = fmaf(qs[g][d0 + 2], hi[0], sc[g]);
            sc[g] = fmaf(qs[g][d0 + 3], hi[1], sc[g]);
          }
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) sc[g] *= kscale;
    } else {
#pragma unroll
      for (int g = 0; g < G; ++g) sc[g] = -1.0f / 0.0f;
    }
    float tile_m[DEC8_GMAX];
#pragma unroll
    for (int g = 0; g < G; ++g) tile_m[g] = sc[g];
    block_reduce_vec8<0, G>(tile_m, red);
    float alpha[DEC8_GMAX], pv[DEC8_GMAX];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float m_new = fmaxf(m[g], tile_m[g]);
      alpha[g] = __expf(m[g] - m_new);             // 0 on first tile
      pv[g] = (kk < end) ? __expf(sc[g] - m_new) : 0.f;
      pl[g][tid] = pv[g] * vscale;                 // v_scale folded into p
      m[g] = m_new;
    }
    float tile_sum[DEC8_GMAX];
#pragma unroll
    for (int g = 0; g < G; ++g) tile_sum[g] = pv[g];   // l: unscaled p
    block_reduce_vec8<1, G>(tile_sum, red);        // also makes pl visible
#pragma unroll
    for (int g = 0; g < G; ++g) {
      l[g] = l[g] * alpha[g] + tile_sum[g];
#pragma unroll
      for (int e = 0; e < 8; ++e) oa[g][e] *= alpha[g];
    }

    // P*V: break-free trip count (keys kg, kg + kgroups, ... < kmax)
    const int kmax = min(DEC8_TILE, end - tile);
    const int iters = kg < kmax ? (kmax - kg + kgroups - 1) / kgroups : 0;
#pragma unroll 2
    for (int j = 0; j < iters; ++j) {
      const int kl = j * kgroups + kg;
      const u32x2 v8 =
          *((const u32x2*)(vbase + (long)(tile + kl) * D) + dv);
      float vf[8];
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(v8[w], false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(v8[w], true);
        vf[w * 4 + 0] = lo[0]; vf[w * 4 + 1] = lo[1];
        vf[w * 4 + 2] = hi[0]; vf[w * 4 + 3] = hi[1];
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float p = pl[g][kl];
#pragma unroll
        for (int e = 0; e < 8; ++e) oa[g][e] = fmaf(p, vf[e], oa[g][e]);
      }
    }
    __syncthreads();                               // pl reuse next tile
  }

  // each key-group writes its own LDS slot (kg * dvecs + dv == tid); ONE
  // barrier, then key-group 0 sums
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int hq = hkv * G + g;
    float* po = part_o + (((long)b * Hq + hq) * splits + split) * D;
    float* pml = part_ml + (((long)b * Hq + hq) * splits + split) * 2;
#pragma unroll
    for (int e = 0; e < 8; ++e) osh[tid][e] = oa[g][e];
    __syncthreads();
    if (kg == 0) {
      float s[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = osh[dv][e];
      for (int gg = 1; gg < kgroups; ++gg) {
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += osh[gg * dvecs + dv][e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) po[dv * 8 + e] = s[e];
    }
    if (tid == 0) { pml[0] = m[g]; pml[1] = l[g]; }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Causal MFMA prefill attention over the fp8 cache: k_attn_prefill<D> with
// the tile staging changed — 8 codes per slot, dequantised with the key's
// scale, rounded to bf16 and written to the same swizzled kt / transposed
// vtT LDS tiles. QK^T / PV MFMA chains and the softmax are the bf16 kernel's.
// Slots past kv_end are zero-padded without touching data or scales.
// Everything below the staging block is a copy of the tile core that
// k_attn_prefill is built on (attn_prefill_core.h), kept because this kernel
// measured slower on the core (profiles/prefill_core.md): a fix to the
// softmax, the swizzles or the epilogue there belongs here too.
// Fragment maps (attn_prefill_core.h header, verified by k_mfma_probe):
//   A[16x32]: lane l -> A[l&15][8*(l>>4)+j], j=0..7
//   B[32x16]: lane l -> B[8*(l>>4)+j][l&15]
//   C[16x16]: lane l, reg r -> C[4*(l>>4)+r][l&15]
// ---------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256)
k_attn_prefill_kv8(const u16* __restrict__ q, const u8* __restrict__ kd,
                   const float* __restrict__ ksc, const u8* __restrict__ vd,
                   const float* __restrict__ vsc, u16* __restrict__ out,
                   const int* __restrict__ pos0, int S, int Hq, int Hkv,
                   int max_seq, float scale, long q_ts) {
  constexpr int DC = D / 16;
  constexpr int KS = D / 32;
  constexpr int KV = 64;
  constexpr int NC = KV / 16;
  constexpr int KA = KV / 32;
  const int qt = blockIdx.x;
  const int hq = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int lane = tid & 63;
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  // K tile: row-major, 16-byte slot index XOR-swizzled by (row&7) so the
  // column-slice ds_read_b128 of a 16-lane group spreads over 8 slots.
  // V tile: TRANSPOSED [col][key] in 8-key blocks, so the PV B-fragment (8
  // consecutive keys of one column) is one 16-byte read; the 8-key block
  // index is XOR-swizzled by (col&7) against the 128-byte column stride's
  // bank pattern. The transpose is paid in the staging scatter below.
  __shared__ u16 kt[64][D];
  __shared__ u16 vtT[D][64];
  __shared__ u16 p_lds[4][16][64];
#define SWZ16(row, col8) ((col8) ^ ((row) & 7))
#define VT_OFF(col, key) \
  ((col) * 64 + \
   ((((key) >> 3) ^ ((col) & 7) ^ (((col) >> 3) & 7)) << 3) + ((key) & 7))

  const int p0 = pos0[b];
  const int q_hi = min(qt * 64 + 64, S);
  const int kv_end = p0 + q_hi;

  const int qrow_rel = qt * 64 + w * 16 + l15;
  const int qrow_ld = min(qrow_rel, S - 1);
  s16x8 a_q[KS];
  {
    const u16* qp = q + ((long)b * S + qrow_ld) * q_ts + (long)hq * D + 8 * lg;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      a_q[ks] = *(const s16x8*)(qp + ks * 32);
  }

  float m_row[4], l_row[4];
  f32x4 o_acc[DC];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_row[r] = -1.0f / 0.0f; l_row[r] = 0.f; }
#pragma unroll
  for (int dc = 0; dc < DC; ++dc) o_acc[dc] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long row0 = ((long)b * Hkv + hkv) * max_seq;
  const u8* kbase = kd + row0 * D;
  const u8* vbase = vd + row0 * D;
  const float* ksb = ksc + row0;
  const float* vsb = vsc + row0;

  const int ntiles = (kv_end + KV - 1) / KV;
  for (int t = 0; t < ntiles; ++t) {
    // ---- stage K/V tile: 8 codes per slot -> dequant -> bf16; slots past
    // kv_end are zero and load neither codes nor scales -----------------
    __syncthreads();                                // vt/kt reuse protection
    {
      const int nv8 = KV * D / 8;
      for (int i = tid; i < nv8; i += 256) {
        const int key = i / (D / 8);
        const int col8 = i % (D / 8);
        const int kk = t * KV + key;
        const int dst = key * (D / 8) + SWZ16(key, col8);
        s16x8 k8 = {0, 0, 0, 0, 0, 0, 0, 0};
        s16x8 v8 = k8;
        if (kk < kv_end) {
          k8 = kv8_dequant8(
              *(const u32x2*)(kbase + (long)kk * D + col8 * 8), ksb[kk]);
          v8 = kv8_dequant8(
              *(const u32x2*)(vbase + (long)kk * D + col8 * 8), vsb[kk]);
        }
        ((s16x8*)kt)[dst] = k8;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          ((u16*)vtT)[VT_OFF(col8 * 8 + j, key)] = (u16)v8[j];
      }
    }
    __syncthreads();

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

    // ---- causal mask + online softmax (per C row, 16-lane shfl groups) --
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
      alpha[r] = __expf(m_row[r] - m_new);
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

#pragma unroll
    for (int dc = 0; dc < DC; ++dc)
#pragma unroll
      for (int r = 0; r < 4; ++r) o_acc[dc][r] *= alpha[r];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p_lds[w][4 * lg + r][c * 16 + l15] = f2bf(p_val[c][r]);
    // same-wave LDS RAW: the compiler inserts the lgkmcnt waits; no barrier
    // needed (p_lds[w] is private to wave w)

    // ---- PV: KA P-fragments of K=32 each ------------------------------
    s16x8 a_p[KA];
#pragma unroll
    for (int ka = 0; ka < KA; ++ka)
      a_p[ka] = *(const s16x8*)(&p_lds[w][l15][ka * 32 + 8 * lg]);
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
      const int col = dc * 16 + l15;
#pragma unroll
      for (int ka = 0; ka < KA; ++ka) {
        const s16x8 b_v = *(const s16x8*)(
            &((u16*)vtT)[VT_OFF(col, ka * 32 + 8 * lg)]);
        o_acc[dc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_p[ka], b_v,
                                                            o_acc[dc], 0, 0, 0);
      }
    }
  }

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

}  // namespace

extern "C" {

void fei_rope_kv8_decode(void* q, const void* k, const void* v, void* kd,
                         float* ks, void* vd, float* vs, const float* cos_sin,
                         const int* pos, int B, int Hq, int Hkv, int D,
                         int max_seq, long q_bs, long kv_bs,
                         hipStream_t stream) {
  hipLaunchKernelGGL(k_rope_kv8_decode, dim3(Hq + Hkv, B), dim3(64), 0, stream,
                     (u16*)q, (const u16*)k, (const u16*)v, (u8*)kd, ks,
                     (u8*)vd, vs, cos_sin, pos, Hq, Hkv, D, max_seq, q_bs,
                     kv_bs);
}

void fei_rope_kv8_prefill(void* q, const void* k, const void* v, void* kd,
                          float* ks, void* vd, float* vs,
                          const float* cos_sin, const int* pos0, int B, int S,
                          int Hq, int Hkv, int D, int max_seq, long q_ts,
                          long kv_ts, hipStream_t stream) {
  hipLaunchKernelGGL(k_rope_kv8_prefill, dim3(S, Hq + Hkv, B), dim3(64), 0,
                     stream, (u16*)q, (const u16*)k, (const u16*)v, (u8*)kd,
                     ks, (u8*)vd, vs, cos_sin, pos0, S, Hq, Hkv, D, max_seq,
                     q_ts, kv_ts);
}

// returns 0, or -1 for an unsupported group size (the wrapper raises)
int fei_attn_decode_kv8(const void* q, void* kd, float* ks, void* vd,
                        float* vs, float* part_o, float* part_ml,
                        const int* pos, int B, int Hq, int Hkv, int D,
                        int max_seq, int splits, float scale, long q_bs,
                        const void* kin, const void* vin,
                        const float* cos_sin, long kv_bs,
                        hipStream_t stream) {
  const int G = Hq / Hkv;
  dim3 grid(splits, Hkv, B);
  const int rope = cos_sin != nullptr;
#define LAUNCH_DEC8(GV, RV) \
  hipLaunchKernelGGL((k_attn_decode_kv8<GV, RV>), grid, dim3(256), 0, stream, \
                     (const u16*)q, (u8*)kd, ks, (u8*)vd, vs, part_o, \
                     part_ml, pos, Hq, Hkv, D, max_seq, splits, scale, q_bs, \
                     (const u16*)kin, (const u16*)vin, cos_sin, kv_bs)
#define LAUNCH_DEC8_R(GV) do { \
    if (rope) LAUNCH_DEC8(GV, true); else LAUNCH_DEC8(GV, false); } while (0)
  switch (G) {
    case 1: LAUNCH_DEC8_R(1); break;
    case 2: LAUNCH_DEC8_R(2); break;
    case 4: LAUNCH_DEC8_R(4); break;
    case 8: LAUNCH_DEC8_R(8); break;
    default: return -1;
  }
#undef LAUNCH_DEC8_R
#undef LAUNCH_DEC8
  return 0;
}

int fei_attn_prefill_kv8(const void* q, const void* kd, const float* ks,
                         const void* vd, const float* vs, void* out,
                         const int* pos0, int B, int S, int Hq, int Hkv,
                         int D, int max_seq, float scale, long q_ts,
                         hipStream_t stream) {
  dim3 grid((S + 63) / 64, Hq, B);
#define LAUNCH_PF8(DV) \
  hipLaunchKernelGGL(k_attn_prefill_kv8<DV>, grid, dim3(256), 0, stream, \
                     (const u16*)q, (const u8*)kd, ks, (const u8*)vd, vs, \
                     (u16*)out, pos0, S, Hq, Hkv, max_seq, scale, q_ts)
  if (D == 128) LAUNCH_PF8(128);
  else if (D == 64) LAUNCH_PF8(64);
  else return -1;
#undef LAUNCH_PF8
  return 0;
}

}  // extern "C"
