#!/usr/bin/env python
"""Time ops.score_topk (k_score_topk_partial + k_score_topk_final) against the
expression it replaces in EmbeddingIndex: ``emb @ q`` + torch.topk, eight
such calls at Q = 8, and for a scoped search score-all + masked_fill + topk.

Points: N x C corpus, f32 and f16, Q = 1 and 8, no mask / 1 % / 50 % mask.
Per point: the median of per-call device-event times over --iters calls
after --warmup calls, the bytes the scan has to read (eligible rows plus the
mask) over that time, and the ratio baseline / fused. The baseline always
reads the f32 matrix: that is what the index holds without the f16 copy.
Needs a GPU; prints one JSON line per point and a markdown table."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fei_amd import ops  # noqa: E402


def timed(fn, warmup: int, iters: int) -> float:
    """Median seconds per call of fn, device events around each call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(times)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sweep", action="store_true",
                    help="also time the unmasked points over grid sizes")
    ap.add_argument("--out", default=None, help="write the table here too")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_score_topk needs a GPU", file=sys.stderr)
        return 2
    ops.require_lib()
    dev = torch.device("cuda:0")
    N, C, k = args.rows, args.dim, args.topk
    g = torch.Generator(device=dev).manual_seed(1)
    emb32 = torch.nn.functional.normalize(
        torch.randn(N, C, device=dev, generator=g), dim=1)
    emb16 = emb32.to(torch.float16)
    q8 = torch.nn.functional.normalize(
        torch.randn(8, C, device=dev, generator=g), dim=1)
    masks = {"none": None}
    for name, p in (("1%", 0.01), ("50%", 0.5)):
        masks[name] = (torch.rand(N, device=dev, generator=g) < p).to(
            torch.uint8)

    # same rows as the parent's expression, at this size (distinct scores)
    want = torch.topk(emb32 @ q8[0], k).indices.sort().values
    got = ops.score_topk(emb32, q8[0], k)[1].long().sort().values
    assert torch.equal(want, got), "fused top-k differs from torch.topk"
    m = masks["1%"]
    want = torch.topk((emb32 @ q8[0]).masked_fill(m == 0, float("-inf")),
                      k).indices.sort().values
    got = ops.score_topk(emb32, q8[0], k, m)[1].long().sort().values
    assert torch.equal(want, got), "masked fused top-k differs"

    def baseline(Q, mask):
        keep = None if mask is None else mask == 0

        def run():
            for u in range(Q):
                s = emb32 @ q8[u]
                if keep is not None:
                    s = s.masked_fill(keep, float("-inf"))
                torch.topk(s, k)
        return run

    rows = []
    base_t = {}
    for Q in (1, 8):
        for mname, mask in masks.items():
            base_t[(Q, mname)] = timed(baseline(Q, mask), args.warmup,
                                       args.iters)
    for dname, emb in (("f32", emb32), ("f16", emb16)):
        for Q in (1, 8):
            q = q8[:Q].contiguous()
            for mname, mask in masks.items():
                t = timed(lambda: ops.score_topk(emb, q, k, mask),
                          args.warmup, args.iters)
                elig = N if mask is None else int(mask.sum())
                nbytes = elig * C * emb.element_size() + \
                    (0 if mask is None else N)
                tb = base_t[(Q, mname)]
                row = {"dtype": dname, "Q": Q, "mask": mname, "N": N, "C": C,
                       "k": k, "fused_us": round(t * 1e6, 1),
                       "baseline_us": round(tb * 1e6, 1),
                       "fused_TBps": round(nbytes / t / 1e12, 3),
                       "ratio": round(tb / t, 2)}
                rows.append(row)
                print(json.dumps(row), flush=True)

    sweep = []
    if args.sweep:
        for dname, emb in (("f32", emb32), ("f16", emb16)):
            for Q in (1, 8):
                q = q8[:Q].contiguous()
                for wg in (256, 512, 1024, 2048, 4096):
                    t = timed(lambda: ops.score_topk(emb, q, k,
                                                     workgroups=wg),
                              args.warmup, args.iters)
                    row = {"sweep": True, "dtype": dname, "Q": Q,
                           "workgroups": wg, "fused_us": round(t * 1e6, 1)}
                    sweep.append(row)
                    print(json.dumps(row), flush=True)

    lines = ["| dtype | Q | mask | fused us | baseline us | fused TB/s | "
             "baseline / fused |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['dtype']} | {r['Q']} | {r['mask']} | "
                     f"{r['fused_us']} | {r['baseline_us']} | "
                     f"{r['fused_TBps']} | {r['ratio']} |")
    if sweep:
        lines += ["", "| dtype | Q | workgroups | fused us |", "|---|---|---|---|"]
        for r in sweep:
            lines.append(f"| {r['dtype']} | {r['Q']} | {r['workgroups']} | "
                         f"{r['fused_us']} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
