"""Filtered (top-k / top-p) sampler: kernel time and end-to-end decode rate.

1. Kernel: fei_sample_filtered next to the plain sampler (k_sample_onepass
   at B <= 8) on the same bf16 logits, device-event timed over many
   launches, twice: on one buffer (row stays in L2) and rotating through a
   pool larger than the 256 MiB Infinity Cache (fresh rows from HBM). In a
   decode step the row was just written by the lm_head GEMV, so the hot
   figure is the closer one.
2. End to end (one engine, B=1): generate() with the filter on the graph
   path (a), the legacy eager generate_sampled() (b), and unfiltered
   generate() (c); wall time of the whole call ending in a device
   synchronise, arms alternated, median of --reps.

Run on an MI355X:
    timeout 900 python scripts/bench_sampler.py [--model llama3-8b]
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fei_amd import ops

DEV = "cuda:0"
FILTERS = ((50, 1.0), (0, 0.9), (50, 0.9))


def time_launches(fn, n_buf, iters, warmup):
    """us per call. The launches are captured into one hipGraph (one node
    per buffer) and the replays are timed with device events, so host
    launch overhead does not bound a kernel of a few microseconds."""
    n = n_buf if n_buf > 1 else 256
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(min(warmup, n)):
            fn(i % n_buf)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            fn(i % n_buf)
    reps = max(2, iters // n)
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * n) * 1000.0


def bench_kernel(B, V, iters, warmup):
    g = torch.Generator().manual_seed(1)
    # pool > 256 MiB so that rotating through it defeats L2 and the LLC
    n_pool = (320 << 20) // (B * V * 2) + 1
    pool = torch.empty(n_pool, B, V, dtype=torch.bfloat16, device=DEV)
    base = (torch.randn(B, V, generator=g) * 3.0).to(torch.bfloat16).to(DEV)
    pool.copy_(base.unsqueeze(0))
    token = torch.zeros(B, dtype=torch.int32, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    info = torch.zeros(B, 2, dtype=torch.float32, device=DEV)
    ws = torch.zeros(B, 128, dtype=torch.float32, device=DEV)

    def plain(i):
        ops.sample(pool[i], token, step, ws, temperature=0.8, seed=3)

    rows = []
    for label, n_buf in (("hot_l2", 1), ("fresh", n_pool)):
        t_plain = time_launches(plain, n_buf, iters, warmup)
        rows.append({"bench": "kernel", "B": B, "V": V, "logits": label,
                     "kernel": "sample_onepass" if B <= 8 else "sample",
                     "us": round(t_plain, 2)})
        for k, p in FILTERS:
            def filt(i, k=k, p=p):
                ops.sample_filtered(pool[i], token, step, info,
                                    temperature=0.8, seed=3, top_k=k, top_p=p)
            t = time_launches(filt, n_buf, iters, warmup)
            rows.append({"bench": "kernel", "B": B, "V": V, "logits": label,
                         "kernel": "sample_filtered", "top_k": k, "top_p": p,
                         "us": round(t, 2),
                         "ratio_vs_plain": round(t / t_plain, 2)})
    for r in rows:
        print(json.dumps(r), flush=True)
    del pool
    torch.cuda.empty_cache()


def bench_e2e(model, new_tokens, reps):
    from fei_amd.engine.engine import LocalEngine
    eng = LocalEngine.create(model, max_seq_len=1024, seed=7,
                             use_hip_graph=True)
    rng = torch.Generator().manual_seed(99)
    prompt = torch.randint(4, 260, (64,), generator=rng).tolist()

    def a():
        return eng.generate(prompt, max_new_tokens=new_tokens,
                            temperature=0.8, top_k=50, top_p=0.9,
                            stop_on_eos=False)

    def b():
        # the eager path is unchanged by the filter kernel; reset the
        # engine's graph-path filter so its prefill samples as it always did
        eng.top_k, eng.top_p = 0, 1.0
        return eng.generate_sampled(prompt, max_new_tokens=new_tokens,
                                    temperature=0.8, top_k=50, top_p=0.9)

    def c():
        return eng.generate(prompt, max_new_tokens=new_tokens,
                            temperature=0.8, stop_on_eos=False)

    arms = {"a_filtered_graph": a, "b_eager_generate_sampled": b,
            "c_unfiltered_graph": c}
    wall = {n: [] for n in arms}
    rate = {n: [] for n in arms}
    for rep in range(reps + 1):                  # rep 0 = warm-up (captures)
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                wall[name].append(dt)
                if "decode_tok_s" in out:
                    rate[name].append(out["decode_tok_s"])
    res = {"bench": "e2e", "model": model, "new_tokens": new_tokens,
           "reps": reps}
    for name in arms:
        res[name] = {"wall_s_median": round(statistics.median(wall[name]), 4),
                     "wall_s_all": [round(x, 4) for x in wall[name]]}
        if rate[name]:
            res[name]["decode_tok_s_median"] = round(
                statistics.median(rate[name]), 2)
    wa, wb, wc = (res[n]["wall_s_median"] for n in arms)
    res["speedup_a_over_b_wall"] = round(wb / wa, 3)
    res["a_over_c_decode_rate"] = round(
        res["a_filtered_graph"]["decode_tok_s_median"] /
        res["c_unfiltered_graph"]["decode_tok_s_median"], 4)
    print(json.dumps(res), flush=True)
    eng.shutdown()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama3-8b")
    p.add_argument("--vocab", type=int, default=128256)
    p.add_argument("--iters", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--new-tokens", type=int, default=256)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--skip-e2e", action="store_true")
    p.add_argument("--skip-kernel", action="store_true")
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_sampler.py needs a GPU"
    ops.require_lib()
    if not args.skip_kernel:
        for B in (1, 8):
            bench_kernel(B, args.vocab, args.iters, args.warmup)
    if not args.skip_e2e:
        bench_e2e(args.model, args.new_tokens, args.reps)


if __name__ == "__main__":
    main()
