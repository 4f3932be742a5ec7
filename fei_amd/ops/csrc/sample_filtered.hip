// Top-k / top-p (nucleus) filtered sampler, hipGraph-capturable.
//
// One 1024-thread workgroup per logits row, any B; the filter parameters,
// temperature and seed are kernel arguments and all rows share one device
// `step`. The algorithm (two-level selection over the bf16 key, fixed-point
// mass, Gumbel-max draw) lives in sample_filtered_body.h, which
// k_sample_filtered_rows (sample_rows.hip) shares.
#include "sample_filtered_body.h"

extern "C" {

__global__ void __launch_bounds__(1024)
k_sample_filtered(const u16* __restrict__ logits, int* __restrict__ token,
                  int* __restrict__ out_tokens, const int* __restrict__ step,
                  float* __restrict__ info, int B, int vocab, int top_k,
                  float top_p, float temperature, u64 seed, int max_new) {
  const int b = blockIdx.x;
  const u64 st = (u64)(*step);
  const RowDraw d = sample_filtered_row(logits + (long)b * vocab, vocab, top_k,
                                        top_p, temperature, seed, st, (u64)b);
  if (threadIdx.x == 0) {
    token[b] = d.token;
    if (out_tokens && (int)st < max_new)
      out_tokens[(long)b * max_new + (int)st] = d.token;
    info[b * 2] = bf2f(key_bf(d.thr));
    ((int*)info)[b * 2 + 1] = (int)d.kept;
  }
}

void fei_sample_filtered(const void* logits, int* token, int* out_tokens,
                         const int* step, float* info, int B, int vocab,
                         int top_k, float top_p, float temperature, u64 seed,
                         int max_new, hipStream_t stream) {
  hipLaunchKernelGGL(k_sample_filtered, dim3(B), dim3(1024), 0, stream,
                     (const u16*)logits, token, out_tokens, step, info, B,
                     vocab, top_k, top_p, temperature, seed, max_new);
}

}  // extern "C"
