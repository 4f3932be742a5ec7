"""Per-row sampler (k_sample_filtered_rows): kernel time next to
k_sample_filtered, and session decode ms/step with sampled sessions.

1. Kernel: both kernels on the same bf16 logits [B, V] with the same
   (uniform) parameters, scalars for the one and device arrays for the
   other. 256 launches are captured into one hipGraph and whole replays are
   timed with device events (scripts/bench_sampler.py's method, "hot L2");
   the arms alternate for --reps rounds and the figure is the median round,
   the spread its min .. max. --other-lib times fei_sample_filtered of
   another build of the kernel library as a third arm.
2. Sessions: N sessions on --model through PagedSessionManager.step_chunk,
   all greedy / mixed (every other session sampled) / all sampled, in one
   process, alternating, median ms/step of --reps rounds.

Run on an MI355X:
    timeout 900 python scripts/bench_sample_rows.py [--skip-sessions]
Prints one JSON line per measurement.
"""
import argparse
import ctypes
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
T, SEED = 0.8, 3


def graph_of(fn, n=256):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(8):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g, n


def time_graph(g, n, replays):
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (replays * n) * 1000.0


def bench_kernel(B, V, reps, replays, other):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(B, V, generator=g) * 3.0).to(torch.bfloat16).to(DEV)
    token = torch.zeros(B, dtype=torch.int32, device=DEV)
    info = torch.zeros(B, 2, dtype=torch.float32, device=DEV)
    step1 = torch.zeros(1, dtype=torch.int32, device=DEV)
    stepB = torch.zeros(B, dtype=torch.int32, device=DEV)
    for k, p in FILTERS:
        rows = dict(
            top_k=torch.full((B,), k, dtype=torch.int32, device=DEV),
            top_p=torch.full((B,), p, dtype=torch.float32, device=DEV),
            temperature=torch.full((B,), T, dtype=torch.float32, device=DEV),
            seed=torch.full((B,), SEED, dtype=torch.int64, device=DEV))

        def scalar():
            ops.sample_filtered(x, token, step1, info, temperature=T,
                                seed=SEED, top_k=k, top_p=p)

        def per_row():
            ops.sample_rows(x, token, stepB, info, **rows)

        arms = {"sample_filtered": scalar, "sample_rows": per_row}
        if other is not None:
            def other_scalar():
                other.fei_sample_filtered(
                    x.data_ptr(), token.data_ptr(), None, step1.data_ptr(),
                    info.data_ptr(), B, V, k, p, T, SEED, 0,
                    torch.cuda.current_stream().cuda_stream)
            arms["sample_filtered_other_lib"] = other_scalar
        graphs = {name: graph_of(fn) for name, fn in arms.items()}
        us = {name: [] for name in arms}
        for _ in range(reps):
            for name, (gr, n) in graphs.items():
                us[name].append(time_graph(gr, n, replays))
        res = {"bench": "kernel", "B": B, "V": V, "top_k": k, "top_p": p,
               "temperature": T, "launches_per_round": 256 * replays,
               "rounds": reps}
        for name, v in us.items():
            res[name + "_us"] = round(statistics.median(v), 2)
            res[name + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        print(json.dumps(res), flush=True)


def session_round(mgr_cls, eng, n, new, sampled_rows, chunk=8):
    """ms per decode step of n sessions; sampled_rows: which sessions
    sample. One warm chunk before the clock starts."""
    mgr = mgr_cls(eng)
    rng = torch.Generator().manual_seed(5)
    hi = min(16000, eng.spec.vocab_size - 2)
    sids = []
    for i in range(n):
        ids = torch.randint(4, hi, (64 + 48 * i,), generator=rng).tolist()
        kw = dict(temperature=0.8, top_k=50, top_p=0.9, seed=100 + i) \
            if i in sampled_rows else {}
        sids.append(mgr.open(ids, max_new_tokens=new + 2 * chunk, **kw))
    mgr.eos = -1                        # every session decodes every step
    mgr.step_chunk(chunk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 0
    while steps < new:
        mgr.step_chunk(chunk)
        steps += chunk
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert len(mgr.active) == n
    for s in sids:
        mgr.close(s)
    return dt / steps * 1e3


def bench_sessions(model, n, new, reps, extra_arms=None):
    from fei_amd.engine.engine import LocalEngine
    from fei_amd.engine.sessions import PagedSessionManager
    eng = LocalEngine.create(model, max_seq_len=4096, seed=7,
                             use_hip_graph=False)
    arms = {"all_greedy": (PagedSessionManager, ()),
            "mixed": (PagedSessionManager, tuple(range(0, n, 2))),
            "all_sampled": (PagedSessionManager, tuple(range(n)))}
    arms.update(extra_arms or {})
    ms = {name: [] for name in arms}
    for rep in range(reps + 1):                     # round 0 = warm-up
        for name, (cls, rows) in arms.items():
            v = session_round(cls, eng, n, new, rows)
            if rep:
                ms[name].append(v)
    res = {"bench": "sessions decode ms/step", "model": model, "sessions": n,
           "steps": new, "rounds": reps}
    for name, v in ms.items():
        res[name + "_ms"] = round(statistics.median(v), 3)
        res[name + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
    print(json.dumps(res), flush=True)
    eng.shutdown()


def load_other(path):
    lib = ctypes.CDLL(path)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.fei_sample_filtered.argtypes = [vp, vp, vp, vp, vp, i, i, i, f, f,
                                        ctypes.c_ulonglong, i, vp]
    return lib


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama3-8b")
    p.add_argument("--vocab", type=int, default=128256)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--replays", type=int, default=8)
    p.add_argument("--sessions", type=int, default=8)
    p.add_argument("--new-tokens", type=int, default=128)
    p.add_argument("--other-lib", default=None)
    p.add_argument("--skip-kernel", action="store_true")
    p.add_argument("--skip-sessions", action="store_true")
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_sample_rows.py needs a GPU"
    ops.require_lib()
    other = load_other(args.other_lib) if args.other_lib else None
    if not args.skip_kernel:
        for B in (8, 32):
            bench_kernel(B, args.vocab, args.reps, args.replays, other)
    if not args.skip_sessions:
        bench_sessions(args.model, args.sessions, args.new_tokens,
                       max(3, args.reps // 2))


if __name__ == "__main__":
    main()
