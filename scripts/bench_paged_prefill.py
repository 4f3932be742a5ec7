#!/usr/bin/env python
"""Paged prefill microbenchmark (profiles/paged_prefill.md).

1. Kernel: ops.attn_prefill_paged against ops.attn_prefill on the same rows
   at the llama3-8b attention shape (Hq 32, Hkv 8, D 128, block size 16):
   S = 2048 at pos0 = 0 and S = 128 at pos0 = 4096. The pool's physical
   blocks are a seeded permutation. The two outputs must be bit-equal before
   anything is timed. Each round times N back-to-back launches of one kernel
   between two device events, then N of the other; the figure is the median
   round, the spread its min .. max.
2. Admission: PagedSessionManager.open() of a 2048-token prompt on
   llama3-8b, against the scratch-cache + slice-copy admission it replaced
   (kept here, as open_scatter, for this comparison only). Host clock around
   a call that ends in a device synchronise; the two alternate.
3. Ragged (profiles/ragged_prefill.md): ONE ops.attn_prefill_paged_ragged
   launch over B packed sequences against B separate ops.attn_prefill_paged
   launches on the same sequences, pool and tables: 8 x 256 tokens, and a
   ragged mix. Bit-equal per sequence before anything is timed; timed as in 1.

Needs a GPU: there is no CPU fallback for a timing.

    python scripts/bench_paged_prefill.py [--skip-open] [--ragged-only]
                                          [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fei_amd import ops  # noqa: E402

HQ, HKV, D, BS = 32, 8, 128, 16
KERNEL_SHAPES = [(2048, 0, 100), (128, 4096, 400)]      # (S, pos0, launches)


def bench_kernel(S: int, pos0: int, launches: int, rounds: int) -> dict:
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(S + pos0)
    n = pos0 + S
    nb = -(-n // BS)
    kc = torch.randn(1, HKV, n, D, generator=g).to(torch.bfloat16).to(dev)
    vc = torch.randn(1, HKV, n, D, generator=g).to(torch.bfloat16).to(dev)
    q = torch.randn(1, S, HQ, D, generator=g).to(torch.bfloat16).to(dev)
    perm = torch.randperm(nb + 8, generator=g)[:nb]
    pad = nb * BS - n
    kp = torch.zeros(nb + 8, HKV, BS, D, dtype=torch.bfloat16, device=dev)
    vp = torch.zeros_like(kp)
    for pool, cache in ((kp, kc), (vp, vc)):
        rows = torch.nn.functional.pad(cache[0], (0, 0, 0, pad))
        pool[perm.to(dev)] = rows.view(HKV, nb, BS, D).transpose(0, 1)
    table = perm.to(torch.int32).view(1, nb).to(dev)
    p0 = torch.full((1,), pos0, dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(D)
    out_c = torch.empty_like(q)
    out_p = torch.empty_like(q)

    def contig():
        ops.attn_prefill(q, kc, vc, p0, scale=scale, out=out_c)

    def paged():
        ops.attn_prefill_paged(q, kp, vp, table, p0, scale=scale, out=out_p)

    for _ in range(10):
        contig()
        paged()
    torch.cuda.synchronize()
    if not torch.equal(out_c.view(torch.int16), out_p.view(torch.int16)):
        raise SystemExit(f"S={S} pos0={pos0}: paged output differs")

    def timed(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / launches            # us per launch

    tc, tp = [], []
    for _ in range(rounds):
        tc.append(timed(contig))
        tp.append(timed(paged))
    flops = 0.0
    for s in range(S):                                      # causal QK^T + PV
        flops += 4.0 * (pos0 + s + 1) * D * HQ
    mc, mp = statistics.median(tc), statistics.median(tp)
    return {"what": "attn_prefill_paged vs attn_prefill", "S": S,
            "pos0": pos0, "launches_per_round": launches, "rounds": rounds,
            "contig_us": round(mc, 2), "contig_us_min_max":
            [round(min(tc), 2), round(max(tc), 2)],
            "paged_us": round(mp, 2), "paged_us_min_max":
            [round(min(tp), 2), round(max(tp), 2)],
            "paged_over_contig": round(mp / mc, 4),
            "contig_tflops": round(flops / mc / 1e6, 1),
            "paged_tflops": round(flops / mp / 1e6, 1)}


RAGGED_SHAPES = [([256] * 8, [0] * 8, 100),
                 ([40, 1500, 256, 64, 700, 128, 40, 300], [0] * 8, 50),
                 ([40, 17, 256, 64, 3, 128, 40, 300],
                  [1500, 700, 0, 2048, 300, 64, 40, 1000], 100)]


def bench_ragged(lens, pos0, launches: int, rounds: int) -> dict:
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(sum(lens) + sum(pos0))
    B, T = len(lens), sum(lens)
    need = [-(-(p + n) // BS) for n, p in zip(lens, pos0)]
    nb = sum(need)
    perm = torch.randperm(nb + 8, generator=g)[:nb]
    kp = torch.randn(nb + 8, HKV, BS, D, generator=g).to(torch.bfloat16) \
        .to(dev)
    vp = torch.randn(nb + 8, HKV, BS, D, generator=g).to(torch.bfloat16) \
        .to(dev)
    table = torch.full((B, max(need)), -1, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = perm[at:at + n].to(torch.int32)
        at += n
    table = table.to(dev)
    q = torch.randn(T, HQ, D, generator=g).to(torch.bfloat16).to(dev)
    batch = ops.RaggedBatch(lens, pos0, table, dev, block_size=BS)
    scale = 1.0 / math.sqrt(D)
    out_r = torch.empty_like(q)
    out_s = torch.empty_like(q)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    parts = [(q[cu[b]:cu[b + 1]].unsqueeze(0),
              out_s[cu[b]:cu[b + 1]].unsqueeze(0), table[b:b + 1].contiguous(),
              torch.full((1,), pos0[b], dtype=torch.int32, device=dev))
             for b in range(B)]

    def ragged():
        ops.attn_prefill_paged_ragged(q, kp, vp, batch, scale=scale,
                                      out=out_r)

    def serial():
        for qb, ob, tb, pb in parts:
            ops.attn_prefill_paged(qb, kp, vp, tb, pb, scale=scale, out=ob)

    for _ in range(5):
        ragged()
        serial()
    torch.cuda.synchronize()
    if not torch.equal(out_r.view(torch.int16), out_s.view(torch.int16)):
        raise SystemExit(f"lens={lens} pos0={pos0}: ragged output differs")

    def timed(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / launches   # us per call (B launches
                                                    # for the serial form)

    ts, tr = [], []
    for _ in range(rounds):
        ts.append(timed(serial))
        tr.append(timed(ragged))
    flops = 0.0
    for n, p in zip(lens, pos0):
        flops += 4.0 * D * HQ * (n * p + n * (n + 1) / 2)
    ms, mr = statistics.median(ts), statistics.median(tr)
    return {"what": "attn_prefill_paged_ragged vs B x attn_prefill_paged",
            "lens": lens, "pos0": pos0, "tiles": batch.n_tiles,
            "launches_per_round": launches, "rounds": rounds,
            "serial_us": round(ms, 2), "serial_us_min_max":
            [round(min(ts), 2), round(max(ts), 2)],
            "ragged_us": round(mr, 2), "ragged_us_min_max":
            [round(min(tr), 2), round(max(tr), 2)],
            "ragged_over_serial": round(mr / ms, 4),
            "serial_tflops": round(flops / ms / 1e6, 1),
            "ragged_tflops": round(flops / mr / 1e6, 1)}


def open_scatter(mgr, ids) -> int:
    """The admission open() used before the paged prefill kernels: prefill
    into a contiguous scratch cache per layer, then copy it into the
    session's blocks slice by slice."""
    from fei_amd.engine.sessions import Session
    m, dev = mgr.model, mgr.model.device
    S = len(ids)
    sid = mgr.pool.new_sequence()
    mgr.pool.ensure_capacity(sid, S + 1)
    k_tmp = [torch.zeros(1, m.hkv_l, S, m.D, device=dev, dtype=m.dtype)
             for _ in range(m.spec.num_layers)]
    v_tmp = [torch.zeros_like(k_tmp[0]) for _ in range(m.spec.num_layers)]
    tokens = torch.tensor([ids], dtype=torch.int64, device=dev)
    pos0 = torch.zeros(1, dtype=torch.int32, device=dev)
    logits = m.forward_prefill(tokens, pos0, k_tmp, v_tmp)
    bs = mgr.pool.block_size
    blocks = mgr.pool.table(sid).blocks
    for li in range(m.spec.num_layers):
        for j in range(0, S, bs):
            blk = blocks[j // bs]
            n = min(bs, S - j)
            mgr.pool.k[li][blk, :, :n, :] = k_tmp[li][0, :, j:j + n, :]
            mgr.pool.v[li][blk, :, :n, :] = v_tmp[li][0, :, j:j + n, :]
    first = int(logits[0].argmax())
    mgr.sessions[sid] = Session(sid=sid, prompt_ids=ids, generated=[first],
                                pos=S, context_ids=list(ids))
    return sid


def bench_open(S: int, rounds: int) -> dict:
    from fei_amd.engine.engine import LocalEngine
    from fei_amd.engine.sessions import PagedSessionManager
    eng = LocalEngine.create("llama3-8b", max_seq_len=S + 512,
                             use_hip_graph=False)
    mgr = PagedSessionManager(eng, block_size=BS, num_blocks=S // BS * 2 + 8)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, eng.spec.vocab_size, (S,), generator=g).tolist()

    def run(fn) -> tuple:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sid = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        first = mgr.sessions[sid].generated[0]
        mgr.close(sid)
        return dt, first

    paged = lambda: mgr.open(ids, max_new_tokens=4)      # noqa: E731
    scatter = lambda: open_scatter(mgr, ids)             # noqa: E731
    for _ in range(2):
        _, f_s = run(scatter)
        _, f_p = run(paged)
    if f_s != f_p:
        raise SystemExit("open(): first token differs between the two paths")
    ts, tp = [], []
    for _ in range(rounds):
        ts.append(run(scatter)[0])
        tp.append(run(paged)[0])
    ms, mp = statistics.median(ts), statistics.median(tp)
    eng.shutdown()
    return {"what": "PagedSessionManager.open, llama3-8b", "S": S,
            "rounds": rounds, "scatter_ms": round(ms, 2),
            "scatter_ms_min_max": [round(min(ts), 2), round(max(ts), 2)],
            "paged_ms": round(mp, 2),
            "paged_ms_min_max": [round(min(tp), 2), round(max(tp), 2)],
            "paged_over_scatter": round(mp / ms, 4)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--open-rounds", type=int, default=5)
    ap.add_argument("--skip-open", action="store_true")
    ap.add_argument("--ragged-only", action="store_true",
                    help="only the ragged section")
    ap.add_argument("--out", default=None, help="also append the JSON lines "
                    "to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_prefill needs a GPU")
    ops.require_lib()
    results = []
    if not args.ragged_only:
        results += [bench_kernel(S, p0, n, args.rounds)
                    for S, p0, n in KERNEL_SHAPES]
    results += [bench_ragged(lens, p0, n, args.rounds)
                for lens, p0, n in RAGGED_SHAPES]
    if not args.skip_open and not args.ragged_only:
        results.append(bench_open(2048, args.open_rounds))
    for r in results:
        line = json.dumps(r)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                        exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
