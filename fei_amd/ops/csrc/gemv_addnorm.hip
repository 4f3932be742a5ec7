// Residual add + RMSNorm folded into the consuming batch-1 GEMV (gfx950).
//
//   h_out = bf16(h_in + delta)
//   x     = bf16(h_out * inv * wn),  inv = rsqrt(mean(h_out^2) + eps)
//   out   = x @ W^T                  (k_gemv_addnorm)
//   out   = silu(x @ Wg^T) * (x @ Wu^T)   (k_gemv_swiglu_addnorm)
//
// Replaces the k_add_rmsnorm launch in front of the qkv and gate/up GEMVs
// of the plain decode chain. Bit-identical to k_add_rmsnorm followed by
// k_gemv / k_gemv_swiglu: the prologue below uses k_add_rmsnorm's
// expressions, per-thread element order and block reduction, and the dot
// keeps k_gemv's per-lane accumulation order.
//
// Where the norm goes: a GEMV's weight addresses do not depend on x, so
// each wave first has its whole weight row slice (up to PRE loop iterations
// per row) in flight and only then computes the norm — once per workgroup,
// every workgroup redundantly from the L2-hot 3 x K bf16 operands — while
// the weights travel from HBM. The memory counter retires loads in issue
// order, so the prologue's own operand loads are issued AHEAD of the
// weight loads: the wait for them then leaves every weight load in flight.
// Normalised x lives in LDS only; the new residual is written by workgroup
// 0 alone, to a buffer other than h_in (every other workgroup is still
// reading h_in).
#include "fei_common.h"

namespace {

constexpr int PRE = 8;   // weight loop iterations preloaded per row (K=4096: all)
constexpr int PRO = 2;   // prologue iterations with preloaded operands (K=4096: all)

template <bool NT>
__device__ __forceinline__ s16x8 ldw(const s16x8* p) {
  return NT ? __builtin_nontemporal_load(p) : *p;
}

// Issue PRE iterations of one row's loads. Indices past the row clamp to its
// last vec8 (an in-bounds duplicate, never accumulated): no branch sits
// between the loads, so they leave back to back.
template <bool NT>
__device__ __forceinline__ void preload_row(s16x8 (&wv)[PRE],
                                            const s16x8* __restrict__ wrow,
                                            int nv, int lane) {
#pragma unroll
  for (int u = 0; u < PRE; ++u)
    wv[u] = ldw<NT>(&wrow[min(lane + u * 64, nv - 1)]);
}

struct AddnormIn { s16x8 d[PRO], h[PRO], w[PRO]; };

__device__ __forceinline__ void addnorm_issue(AddnormIn& in,
                                              const s16x8* __restrict__ dr,
                                              const s16x8* __restrict__ hr,
                                              const s16x8* __restrict__ wr,
                                              int nv, int tid) {
#pragma unroll
  for (int u = 0; u < PRO; ++u) {
    const int i = min(tid + u * 256, nv - 1);
    in.d[u] = dr[i];
    in.h[u] = hr[i];
    in.w[u] = wr[i];
  }
}

// k_add_rmsnorm's first pass over one vec8: new residual + running sumsq of
// the bf16-ROUNDED sum.
__device__ __forceinline__ float addnorm_sumsq8(s16x8 rv, s16x8 xv, s16x8& nr,
                                                float ss) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f = bf2f((u16)rv[j]) + bf2f((u16)xv[j]);
    u16 b = f2bf(f);
    nr[j] = (short)b;
    f = bf2f(b);
    ss = fmaf(f, f, ss);
  }
  return ss;
}

// k_add_rmsnorm's second pass over one vec8.
__device__ __forceinline__ s16x8 addnorm_scale8(s16x8 rv, s16x8 wvv,
                                                float inv) {
  s16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    o[j] = (short)f2bf(bf2f((u16)rv[j]) * inv * bf2f((u16)wvv[j]));
  return o;
}

// Thread t owns vec8 t, t+256, ... in both passes (k_add_rmsnorm's loop
// shape), so a thread only ever re-reads LDS slots it wrote itself and the
// single barrier at the end is the only one the x row needs. `ho` is null
// in every workgroup but the one that writes the new residual.
__device__ __forceinline__ void addnorm_finish(const AddnormIn& in,
                                               s16x8* xs, float* red,
                                               const s16x8* __restrict__ dr,
                                               const s16x8* __restrict__ hr,
                                               const s16x8* __restrict__ wr,
                                               s16x8* __restrict__ ho,
                                               int nv, int K, float eps,
                                               int tid) {
  float ss = 0.f;
  s16x8 nr[PRO];
#pragma unroll
  for (int u = 0; u < PRO; ++u) {
    // computed on every thread (idle ones on the clamped duplicate) and
    // selected: a branch here lets hipcc sink the operand loads into it,
    // behind the weight loads
    const int i = tid + u * 256;
    const float s2 = addnorm_sumsq8(in.h[u], in.d[u], nr[u], ss);
    ss = i < nv ? s2 : ss;
    if (ho && i < nv) ho[i] = nr[u];
  }
  for (int i = tid + PRO * 256; i < nv; i += 256) {   // K > 4096
    s16x8 n;
    ss = addnorm_sumsq8(hr[i], dr[i], n, ss);
    xs[i] = n;
    if (ho) ho[i] = n;
  }
  ss = block_reduce_sum(ss, red);
  const float inv = rsqrtf(ss / (float)K + eps);
#pragma unroll
  for (int u = 0; u < PRO; ++u) {
    const int i = tid + u * 256;
    const s16x8 o = addnorm_scale8(nr[u], in.w[u], inv);
    if (i < nv) xs[i] = o;
  }
  for (int i = tid + PRO * 256; i < nv; i += 256)
    xs[i] = addnorm_scale8(xs[i], wr[i], inv);
  __syncthreads();
}

// Dot of two weight rows with the LDS x row, k_gemv's order per lane:
// acc += dot8 over ascending i — the preloaded registers, then the tail.
template <bool NT>
__device__ __forceinline__ void dot_rows(float& acc0, float& acc1,
                                         const s16x8 (&wv0)[PRE],
                                         const s16x8 (&wv1)[PRE],
                                         const s16x8* __restrict__ wrow0,
                                         const s16x8* __restrict__ wrow1,
                                         const s16x8* xs, int nv, int lane) {
#pragma unroll
  for (int u = 0; u < PRE; ++u) {
    const int i = lane + u * 64;
    const s16x8 xv = xs[min(i, nv - 1)];
    const float d0 = dot8_bf16(xv, wv0[u]);
    const float d1 = dot8_bf16(xv, wv1[u]);
    acc0 = i < nv ? acc0 + d0 : acc0;      // select, not a branch per load
    acc1 = i < nv ? acc1 + d1 : acc1;
    // one iteration at a time: left free, the scheduler reads all PRE x
    // vectors and widens them to f32 up front (234 VGPRs instead of 151)
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int i = lane + PRE * 64; i < nv; i += 64) {     // K > 4096
    const s16x8 a = ldw<NT>(&wrow0[i]);
    const s16x8 b = ldw<NT>(&wrow1[i]);
    const s16x8 xv = xs[i];
    acc0 += dot8_bf16(xv, a);
    acc1 += dot8_bf16(xv, b);
  }
}

// LDS: K bf16 of x, then the 4 floats of the block reduction — one array
// (a second __shared__ object can make hipcc drain the weight loads before
// the first LDS read).
#define ADDNORM_LDS(K) ((size_t)(K) * 2 + 4 * sizeof(float))

// A workgroup owns `rg` consecutive groups of 8 rows (2 per wave, k_gemv's
// mapping inside a group). The first group's weights fly during the
// prologue; later groups amortise it. Waves past N keep a clamped, valid
// row pointer, reach every barrier and store nothing.
template <int M, bool NT>
__global__ void __launch_bounds__(256)
k_gemv_addnorm(u16* __restrict__ out, const u16* __restrict__ delta,
               const u16* __restrict__ h_in, u16* __restrict__ h_out,
               const u16* __restrict__ wn, const u16* __restrict__ w,
               int N, int K, float eps, int rg) {
  static_assert(M == 1, "the add+norm prologue is batch-1 only");
  extern __shared__ s16x8 lds_x[];
  s16x8* xs = lds_x;
  float* red = (float*)(lds_x + (K >> 3));
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int nv = K >> 3;
  int n0 = blockIdx.x * rg * 8 + wid * 2;

  bool active = n0 < N;
  bool two = (n0 + 1) < N;
  const s16x8* wrow0 = (const s16x8*)(w + (long)(active ? n0 : 0) * K);
  const s16x8* wrow1 =
      (const s16x8*)(w + (long)(active ? n0 + (two ? 1 : 0) : 0) * K);

  const s16x8* dr = (const s16x8*)delta;
  const s16x8* hr = (const s16x8*)h_in;
  const s16x8* wr = (const s16x8*)wn;
  AddnormIn in;
  addnorm_issue(in, dr, hr, wr, nv, tid);
  s16x8 wv0[PRE], wv1[PRE];
  preload_row<NT>(wv0, wrow0, nv, lane);
  preload_row<NT>(wv1, wrow1, nv, lane);
  addnorm_finish(in, xs, red, dr, hr, wr,
                 blockIdx.x == 0 ? (s16x8*)h_out : nullptr, nv, K, eps, tid);

  for (int g = 0;;) {
    float acc0 = 0.f, acc1 = 0.f;
    dot_rows<NT>(acc0, acc1, wv0, wv1, wrow0, wrow1, xs, nv, lane);
    const float v0 = wave_reduce_sum(acc0);
    const float v1 = wave_reduce_sum(acc1);
    if (lane == 0 && active) {
      out[n0] = f2bf(v0);
      if (two) out[n0 + 1] = f2bf(v1);
    }
    if (++g >= rg) break;
    n0 += 8;
    active = n0 < N;
    two = (n0 + 1) < N;
    wrow0 = (const s16x8*)(w + (long)(active ? n0 : 0) * K);
    wrow1 = (const s16x8*)(w + (long)(active ? n0 + (two ? 1 : 0) : 0) * K);
    preload_row<NT>(wv0, wrow0, nv, lane);
    preload_row<NT>(wv1, wrow1, nv, lane);
  }
}

// Same prologue in front of k_gemv_swiglu's body: wave -> gate row n and up
// row n + N, 4 rows per group.
template <int M, bool NT>
__global__ void __launch_bounds__(256)
k_gemv_swiglu_addnorm(u16* __restrict__ out, const u16* __restrict__ delta,
                      const u16* __restrict__ h_in, u16* __restrict__ h_out,
                      const u16* __restrict__ wn, const u16* __restrict__ w,
                      int N, int K, float eps, int rg) {
  static_assert(M == 1, "the add+norm prologue is batch-1 only");
  extern __shared__ s16x8 lds_x[];
  s16x8* xs = lds_x;
  float* red = (float*)(lds_x + (K >> 3));
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int nv = K >> 3;
  int n = blockIdx.x * rg * 4 + wid;

  bool active = n < N;
  const s16x8* grow = (const s16x8*)(w + (long)(active ? n : 0) * K);
  const s16x8* urow = (const s16x8*)(w + (long)((active ? n : 0) + N) * K);

  const s16x8* dr = (const s16x8*)delta;
  const s16x8* hr = (const s16x8*)h_in;
  const s16x8* wr = (const s16x8*)wn;
  AddnormIn in;
  addnorm_issue(in, dr, hr, wr, nv, tid);
  s16x8 gv[PRE], uv[PRE];
  preload_row<NT>(gv, grow, nv, lane);
  preload_row<NT>(uv, urow, nv, lane);
  addnorm_finish(in, xs, red, dr, hr, wr,
                 blockIdx.x == 0 ? (s16x8*)h_out : nullptr, nv, K, eps, tid);

  for (int g = 0;;) {
    float accg = 0.f, accu = 0.f;
    dot_rows<NT>(accg, accu, gv, uv, grow, urow, xs, nv, lane);
    const float gs = wave_reduce_sum(accg);
    const float us = wave_reduce_sum(accu);
    if (lane == 0 && active) {
      const float silu = gs / (1.f + __expf(-gs));
      out[n] = f2bf(silu * us);
    }
    if (++g >= rg) break;
    n += 4;
    active = n < N;
    grow = (const s16x8*)(w + (long)(active ? n : 0) * K);
    urow = (const s16x8*)(w + (long)((active ? n : 0) + N) * K);
    preload_row<NT>(gv, grow, nv, lane);
    preload_row<NT>(uv, urow, nv, lane);
  }
}

// ---------------------------------------------------------------------------
// Ring schedule (K <= 4096, the preload is the whole row slice): the weight
// stream stays full across row groups. Once slot u of group g has been
// dotted it is reloaded with slot u of the same wave's group g + 1
// (k_gemv_deep's scheme), so the wave reduction, the epilogue and the store
// of group g run with the next group's 16 loads per lane in flight; only a
// workgroup's last group drains. Groups are dealt grid-stride, group =
// blockIdx.x + g * gridDim.x, so one resident round of workgroups covers
// every group with trip counts at most one apart. The G trips are a template
// parameter and the kernel is straight-line code: as a runtime loop the ring
// becomes loop-carried and hipcc copies it (profiles/gemv_deep.md). Groups
// past N keep a clamped, valid row pointer; their loads are issued and
// nothing is stored. Per lane the chain is still acc += dot8_bf16(x_i, w_i)
// over ascending i from +0.f: only the moment a load is issued changes.
// ---------------------------------------------------------------------------

constexpr int RING_MAX_TRIPS = 8;

// The first group's loads in the order the dots consume them (slot by slot,
// both rows), so every group waits with the same 14 loads behind it.
template <bool NT>
__device__ __forceinline__ void preload_rows(s16x8 (&wv0)[PRE],
                                             s16x8 (&wv1)[PRE],
                                             const s16x8* __restrict__ wrow0,
                                             const s16x8* __restrict__ wrow1,
                                             int nv, int lane) {
#pragma unroll
  for (int u = 0; u < PRE; ++u) {
    const int j = min(lane + u * 64, nv - 1);
    wv0[u] = ldw<NT>(&wrow0[j]);
    wv1[u] = ldw<NT>(&wrow1[j]);
  }
}

template <bool NT, bool REFILL>
__device__ __forceinline__ void dot_rows_ring(float& acc0, float& acc1,
                                              s16x8 (&wv0)[PRE],
                                              s16x8 (&wv1)[PRE],
                                              const s16x8* __restrict__ next0,
                                              const s16x8* __restrict__ next1,
                                              const s16x8* xs, int nv,
                                              int lane) {
#pragma unroll
  for (int u = 0; u < PRE; ++u) {
    const int i = lane + u * 64;
    const int j = min(i, nv - 1);
    const s16x8 xv = xs[j];
    const float d0 = dot8_bf16(xv, wv0[u]);
    const float d1 = dot8_bf16(xv, wv1[u]);
    acc0 = i < nv ? acc0 + d0 : acc0;      // select, not a branch per load
    acc1 = i < nv ? acc1 + d1 : acc1;
    if (REFILL) {
      // The refill's index is made to depend on this slot's sums: left
      // independent, hipcc hoists every refill above the first dot (32
      // loads in flight, 256 VGPRs, occupancy 1).
      int jr = j;
      asm volatile("" : "+v"(jr), "+v"(acc0), "+v"(acc1));
      wv0[u] = ldw<NT>(&next0[jr]);
      wv1[u] = ldw<NT>(&next1[jr]);
    }
    // one slot at a time: keeps the refill right behind its dot and stops
    // the scheduler widening every slot to f32 up front
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <bool NT, int G>
__global__ void __launch_bounds__(256)
k_gemv_addnorm_ring(u16* __restrict__ out, const u16* __restrict__ delta,
                    const u16* __restrict__ h_in, u16* __restrict__ h_out,
                    const u16* __restrict__ wn, const u16* __restrict__ w,
                    int N, int K, float eps) {
  extern __shared__ s16x8 lds_x[];
  s16x8* xs = lds_x;
  float* red = (float*)(lds_x + (K >> 3));
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int nv = K >> 3;                   // <= PRE * 64
  const long stride = (long)gridDim.x * 8;
  long n0 = (long)blockIdx.x * 8 + wid * 2;

  bool active = n0 < N;
  bool two = (n0 + 1) < N;
  const s16x8* wrow0 = (const s16x8*)(w + (active ? n0 : 0) * K);
  const s16x8* wrow1 = (const s16x8*)(w + (active ? n0 + (two ? 1 : 0) : 0) * K);

  const s16x8* dr = (const s16x8*)delta;
  const s16x8* hr = (const s16x8*)h_in;
  const s16x8* wr = (const s16x8*)wn;
  AddnormIn in;
  addnorm_issue(in, dr, hr, wr, nv, tid);
  s16x8 wv0[PRE], wv1[PRE];
  preload_rows<NT>(wv0, wv1, wrow0, wrow1, nv, lane);
  addnorm_finish(in, xs, red, dr, hr, wr,
                 blockIdx.x == 0 ? (s16x8*)h_out : nullptr, nv, K, eps, tid);

#pragma unroll
  for (int g = 0; g < G; ++g) {
    float acc0 = 0.f, acc1 = 0.f;
    const long nn = n0 + stride;
    const bool nactive = nn < N;
    const bool ntwo = (nn + 1) < N;
    if (g + 1 < G) {
      wrow0 = (const s16x8*)(w + (nactive ? nn : 0) * K);
      wrow1 = (const s16x8*)(w + (nactive ? nn + (ntwo ? 1 : 0) : 0) * K);
      dot_rows_ring<NT, true>(acc0, acc1, wv0, wv1, wrow0, wrow1, xs, nv,
                              lane);
    } else {
      dot_rows_ring<NT, false>(acc0, acc1, wv0, wv1, wrow0, wrow1, xs, nv,
                               lane);
    }
    const float v0 = wave_reduce_sum(acc0);
    const float v1 = wave_reduce_sum(acc1);
    if (lane == 0 && active) {
      out[n0] = f2bf(v0);
      if (two) out[n0 + 1] = f2bf(v1);
    }
    n0 = nn;
    active = nactive;
    two = ntwo;
  }
}

template <bool NT, int G>
__global__ void __launch_bounds__(256)
k_gemv_swiglu_addnorm_ring(u16* __restrict__ out,
                           const u16* __restrict__ delta,
                           const u16* __restrict__ h_in,
                           u16* __restrict__ h_out,
                           const u16* __restrict__ wn,
                           const u16* __restrict__ w, int N, int K,
                           float eps) {
  extern __shared__ s16x8 lds_x[];
  s16x8* xs = lds_x;
  float* red = (float*)(lds_x + (K >> 3));
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int nv = K >> 3;                   // <= PRE * 64
  const long stride = (long)gridDim.x * 4;
  long n = (long)blockIdx.x * 4 + wid;

  bool active = n < N;
  const long up = (long)N * nv;            // gate row n -> up row n + N, in vec8
  const s16x8* grow = (const s16x8*)(w + (active ? n : 0) * K);
  const s16x8* urow = grow + up;

  const s16x8* dr = (const s16x8*)delta;
  const s16x8* hr = (const s16x8*)h_in;
  const s16x8* wr = (const s16x8*)wn;
  AddnormIn in;
  addnorm_issue(in, dr, hr, wr, nv, tid);
  s16x8 gv[PRE], uv[PRE];
  preload_rows<NT>(gv, uv, grow, urow, nv, lane);
  addnorm_finish(in, xs, red, dr, hr, wr,
                 blockIdx.x == 0 ? (s16x8*)h_out : nullptr, nv, K, eps, tid);

#pragma unroll
  for (int g = 0; g < G; ++g) {
    float accg = 0.f, accu = 0.f;
    const long nn = n + stride;
    const bool nactive = nn < N;
    if (g + 1 < G) {
      grow = (const s16x8*)(w + (nactive ? nn : 0) * K);
      urow = grow + up;
      dot_rows_ring<NT, true>(accg, accu, gv, uv, grow, urow, xs, nv, lane);
    } else {
      dot_rows_ring<NT, false>(accg, accu, gv, uv, grow, urow, xs, nv, lane);
    }
    const float gs = wave_reduce_sum(accg);
    const float us = wave_reduce_sum(accu);
    if (lane == 0 && active) {
      const float silu = gs / (1.f + __expf(-gs));
      out[n] = f2bf(silu * us);
    }
    n = nn;
    active = nactive;
  }
}

// Kernel instance for (swiglu, nontemporal, trips): one table for the launch
// and for the occupancy query.
template <int G>
const void* ring_instance(bool swiglu, bool nt) {
  if (swiglu)
    return nt ? (const void*)k_gemv_swiglu_addnorm_ring<true, G>
              : (const void*)k_gemv_swiglu_addnorm_ring<false, G>;
  return nt ? (const void*)k_gemv_addnorm_ring<true, G>
            : (const void*)k_gemv_addnorm_ring<false, G>;
}

const void* ring_kernel(bool swiglu, bool nt, int trips) {
  switch (trips) {
    case 1: return ring_instance<1>(swiglu, nt);
    case 2: return ring_instance<2>(swiglu, nt);
    case 3: return ring_instance<3>(swiglu, nt);
    case 4: return ring_instance<4>(swiglu, nt);
    case 5: return ring_instance<5>(swiglu, nt);
    case 6: return ring_instance<6>(swiglu, nt);
    case 7: return ring_instance<7>(swiglu, nt);
    case 8: return ring_instance<8>(swiglu, nt);
    default: return nullptr;
  }
}

// Shapes the ring kernels take: the whole row slice fits the preload.
bool ring_shape_ok(int K) {
  return K > 0 && K % 8 == 0 && (K >> 3) <= PRE * 64;
}

int ring_launch(bool swiglu, void* out, const void* delta, const void* h_in,
                void* h_out, const void* wn, const void* w, int M, int N,
                int K, float eps, int nontemporal, int grid, int trips,
                hipStream_t stream) {
  if (M != 1) return -1;
  if (!ring_shape_ok(K) || N < 1) return -2;
  if (h_in == h_out) return -3;
  const long groups = swiglu ? ((long)N + 3) / 4 : ((long)N + 7) / 8;
  const void* fn = ring_kernel(swiglu, nontemporal != 0, trips);
  // every group must be walked: a short plan would leave rows unwritten
  if (!fn || grid < 1 || (long)grid * trips < groups) return -4;
  void* args[] = {&out, &delta, &h_in, &h_out, &wn, &w, &N, &K, &eps};
  if (hipLaunchKernel(fn, dim3(grid), dim3(256), args, ADDNORM_LDS(K),
                      stream) != hipSuccess)
    return -5;
  return 0;
}

}  // namespace

extern "C" {

// Most trips a ring kernel instance walks.
int fei_gemv_addnorm_ring_max_trips(void) { return RING_MAX_TRIPS; }

// Workgroups of one ring kernel instance a CU holds at once (the HIP
// occupancy query for its registers and its dynamic LDS at this K), times
// the CU count of the current device: the slots of one resident round.
// Returns a negative code for a shape or trip count without an instance (-2,
// -4) or a failed query (-5). Enqueues nothing; callers cache the value.
int fei_gemv_addnorm_ring_slots(int swiglu, int nontemporal, int trips,
                                int K) {
  if (!ring_shape_ok(K)) return -2;
  const void* fn = ring_kernel(swiglu != 0, nontemporal != 0, trips);
  if (!fn) return -4;
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &per_cu, fn, 256, ADDNORM_LDS(K)) != hipSuccess)
    return -5;
  if (per_cu < 1 || cus < 1) return -5;
  return per_cu * cus;
}

// The ring schedule: `grid` workgroups, each walking `trips` groups
// grid-stride (grid * trips must cover every group). Other arguments and
// codes as below; -4 for a plan without a kernel instance or one that does
// not cover N, -5 for a failed launch.
int fei_gemv_addnorm_ring(void* out, const void* delta, const void* h_in,
                          void* h_out, const void* wn, const void* w, int M,
                          int N, int K, float eps, int nontemporal, int grid,
                          int trips, hipStream_t stream) {
  return ring_launch(false, out, delta, h_in, h_out, wn, w, M, N, K, eps,
                     nontemporal, grid, trips, stream);
}

int fei_gemv_swiglu_addnorm_ring(void* out, const void* delta,
                                 const void* h_in, void* h_out,
                                 const void* wn, const void* w, int M, int N,
                                 int K, float eps, int nontemporal, int grid,
                                 int trips, hipStream_t stream) {
  return ring_launch(true, out, delta, h_in, h_out, wn, w, M, N, K, eps,
                     nontemporal, grid, trips, stream);
}

// The drain-between-groups schedule (contiguous groups; every K the LDS row
// holds). Arguments follow fei_gemv_norm. `row_groups` (>= 1): row groups walked per
// workgroup. Returns 0, or a negative code with nothing launched: -1 for a
// batch other than 1, -2 for a shape outside the kernel (K not a positive
// multiple of 8, x row over the 32 KB LDS cap, N < 1), -3 for an aliased
// residual pair.
int fei_gemv_addnorm(void* out, const void* delta, const void* h_in,
                     void* h_out, const void* wn, const void* w, int M, int N,
                     int K, float eps, int nontemporal, int row_groups,
                     hipStream_t stream) {
  if (M != 1) return -1;
  if (K <= 0 || K % 8 != 0 || (size_t)K * 2 > 32 * 1024 || N < 1) return -2;
  if (h_in == h_out) return -3;
  const int rg = row_groups < 1 ? 1 : row_groups;
  const int groups = (N + 7) / 8;
  dim3 grid((groups + rg - 1) / rg);
#define LA(NTV) hipLaunchKernelGGL((k_gemv_addnorm<1, NTV>), grid, dim3(256), \
    ADDNORM_LDS(K), stream, (u16*)out, (const u16*)delta, (const u16*)h_in, \
    (u16*)h_out, (const u16*)wn, (const u16*)w, N, K, eps, rg)
  if (nontemporal) LA(true); else LA(false);
#undef LA
  return 0;
}

int fei_gemv_swiglu_addnorm(void* out, const void* delta, const void* h_in,
                            void* h_out, const void* wn, const void* w, int M,
                            int N, int K, float eps, int nontemporal,
                            int row_groups, hipStream_t stream) {
  if (M != 1) return -1;
  if (K <= 0 || K % 8 != 0 || (size_t)K * 2 > 32 * 1024 || N < 1) return -2;
  if (h_in == h_out) return -3;
  const int rg = row_groups < 1 ? 1 : row_groups;
  const int groups = (N + 3) / 4;
  dim3 grid((groups + rg - 1) / rg);
#define LA(NTV) hipLaunchKernelGGL((k_gemv_swiglu_addnorm<1, NTV>), grid, \
    dim3(256), ADDNORM_LDS(K), stream, (u16*)out, (const u16*)delta, \
    (const u16*)h_in, (u16*)h_out, (const u16*)wn, (const u16*)w, N, K, eps, rg)
  if (nontemporal) LA(true); else LA(false);
#undef LA
  return 0;
}

}  // extern "C"
