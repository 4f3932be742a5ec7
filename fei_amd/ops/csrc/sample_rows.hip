// Per-row top-k / top-p filtered sampler for continuous batching,
// hipGraph-capturable.
//
// The same per-row body as k_sample_filtered (sample_filtered_body.h), but
// every row is its own request: top_k, top_p, temperature, seed and step are
// device arrays of length B, read once per workgroup (they are
// workgroup-uniform, so they stay in SGPRs). The noise hash mixes in row id 0
// whatever blockIdx.x is, so a row's draw depends only on its own (logits,
// parameters, seed, step) and not on where it sits in the batch: row b's
// token and info are bit-equal to k_sample_filtered run with B = 1 on that
// row with that row's scalars.
//
// The kernel writes token and info only. The caller advances `step`
// (step.add_(1)); nothing but the sizes is a kernel argument, so a captured
// launch follows in-place changes of a request's parameters.
#include "sample_filtered_body.h"

extern "C" {

__global__ void __launch_bounds__(1024)
k_sample_filtered_rows(const u16* __restrict__ logits, int* __restrict__ token,
                       float* __restrict__ info,
                       const int* __restrict__ top_k,
                       const float* __restrict__ top_p,
                       const float* __restrict__ temperature,
                       const u64* __restrict__ seed,
                       const int* __restrict__ step, int B, int vocab) {
  const int b = blockIdx.x;
  const RowDraw d = sample_filtered_row(logits + (long)b * vocab, vocab,
                                        top_k[b], top_p[b], temperature[b],
                                        seed[b], (u64)step[b], 0ull);
  if (threadIdx.x == 0) {
    token[b] = d.token;
    info[b * 2] = bf2f(key_bf(d.thr));
    ((int*)info)[b * 2 + 1] = (int)d.kept;
  }
}

// Returns 0 when it launched; non-zero (and launches nothing) for an empty
// batch or vocabulary.
int fei_sample_filtered_rows(const void* logits, int* token, float* info,
                             const int* top_k, const float* top_p,
                             const float* temperature, const u64* seed,
                             const int* step, int B, int vocab,
                             hipStream_t stream) {
  if (B <= 0 || vocab <= 0) return 1;
  hipLaunchKernelGGL(k_sample_filtered_rows, dim3(B), dim3(1024), 0, stream,
                     (const u16*)logits, token, info, top_k, top_p,
                     temperature, seed, step, B, vocab);
  return 0;
}

}  // extern "C"
