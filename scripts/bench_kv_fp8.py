"""fp8 KV cache measurements (profiles/kv_fp8.md is produced from these).

  python scripts/bench_kv_fp8.py decode    # ms/step, bf16 vs fp8 KV, 8B
  python scripts/bench_kv_fp8.py trace --kv {bf16,fp8}
        # 64 graph replays at 16k context; run under
        # rocprofv3 --kernel-trace --stats -- python ... for kernel times
  python scripts/bench_kv_fp8.py quality   # attention rel-L2 + 8B greedy
                                           # token agreement, fp8 vs bf16 KV

Long contexts are not prefilled token by token: the graph is captured on a
short real prompt, then cache rows [0, ctx) are filled with random content
of the cache's own format and pos is set to ctx. Decode time does not
depend on the values, only on the bytes read.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MODEL = "llama3-8b"


def _engine(kv, batch, max_seq):
    from fei_amd.engine.engine import LocalEngine
    return LocalEngine.create(MODEL, batch_size=batch, max_seq_len=max_seq,
                              seed=7, kv_quant=(None if kv == "bf16" else kv))


def _fake_context(eng, ctx):
    """rows [0, ctx) <- random content; pos <- ctx."""
    from fei_amd import ops
    for c in (*eng.k_caches, *eng.v_caches):
        if isinstance(c, ops.QuantKV):
            d = c.data[:, :, :ctx]
            d.random_(0, 256)
            d[(d & 0x7F) == 0x7F] = 0           # no NaN codes
            c.scale[:, :, :ctx] = 0.01
        else:
            c[:, :, :ctx].normal_(0.0, 0.5)
    eng.pos.fill_(ctx)
    torch.cuda.synchronize()


def _ms_per_step(eng, ctx, warm=16, windows=5, steps=48):
    _fake_context(eng, ctx)
    for _ in range(warm):
        eng._graph.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(steps):
            eng._graph.replay()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / steps)
    return round(statistics.median(out), 4), round(max(out) - min(out), 4)


def cmd_decode(args):
    """ms/step medians. The bf16 case is measured twice (first and last) so
    the run-to-run spread is on the page."""
    res = {}
    prompt = list(range(4, 36))
    for batch, ctxs, max_seq in ((1, [512, 4096, 16384, 65536], 66560),
                                 (8, [4096], 5120)):
        for tag, kv in (("bf16", "bf16"), ("fp8", "fp8"), ("bf16_again", "bf16")):
            eng = _engine(kv, batch, max_seq)
            if batch == 1:
                eng.prefill(prompt)
            else:
                eng.prefill_ragged([prompt] * batch)
            for ctx in ctxs:
                med, spread = _ms_per_step(eng, ctx)
                res[f"B{batch}_ctx{ctx}_{tag}"] = {"ms_per_step": med,
                                                   "window_spread_ms": spread}
                print(f"B={batch} ctx={ctx} kv={tag}: {med} ms/step "
                      f"(spread of windows {spread})", flush=True)
            eng.shutdown()
            del eng
            torch.cuda.empty_cache()
    print(json.dumps(res))


def cmd_trace(args):
    eng = _engine(args.kv, 1, 17408)
    eng.prefill(list(range(4, 36)))
    _fake_context(eng, 16384)
    for _ in range(64):
        eng._graph.replay()
    torch.cuda.synchronize()
    print(f"kv={args.kv}: 64 replays at ctx 16384 done")
    eng.shutdown()


def cmd_quality(args):
    from fei_amd import ops
    from fei_amd.ops import reference as ref
    dev = "cuda:0"
    B, Hq, Hkv, D, MS = 2, 8, 2, 128, 1024
    res = {"attn_rel_l2": {}}
    for n in (1, 17, 300, 1000):
        g = torch.Generator().manual_seed(n)
        q = torch.randn(B, Hq, D, generator=g).to(torch.bfloat16)
        k = torch.randn(B, Hkv, MS, D, generator=g)
        v = torch.randn(B, Hkv, MS, D, generator=g)
        k[..., 5] *= 8.0                         # one outlier channel
        v[..., 9] *= 8.0
        k, v = k.to(torch.bfloat16), v.to(torch.bfloat16)
        pos = torch.full((B,), n - 1, dtype=torch.int32, device=dev)
        o16 = ops.attn_decode(q.to(dev), k.to(dev), v.to(dev), pos).float()
        k8 = ops.QuantKV(*(t.to(dev) for t in ref.quant_kv_fp8(k)))
        v8 = ops.QuantKV(*(t.to(dev) for t in ref.quant_kv_fp8(v)))
        o8 = ops.attn_decode(q.to(dev), k8, v8, pos).float()
        res["attn_rel_l2"][n] = round(
            ((o8 - o16).norm() / o16.norm()).item(), 5)
    prompt = torch.randint(4, 16000, (200,),
                           generator=torch.Generator().manual_seed(9)).tolist()
    toks = {}
    for kv in ("bf16", "fp8"):
        eng = _engine(kv, 1, 512)
        toks[kv] = eng.generate(prompt, max_new_tokens=64,
                                stop_on_eos=False)["token_ids"]
        eng.shutdown()
        del eng
        torch.cuda.empty_cache()
    same = [a == b for a, b in zip(toks["bf16"], toks["fp8"])]
    res["greedy_tokens_equal_of_64"] = sum(same)
    res["greedy_common_prefix"] = (same.index(False) if False in same
                                   else len(same))
    print(json.dumps(res))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_kv_fp8.py measures on the GPU; none found")
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("decode")
    t = sub.add_parser("trace")
    t.add_argument("--kv", choices=("bf16", "fp8"), required=True)
    sub.add_parser("quality")
    a = ap.parse_args()
    {"decode": cmd_decode, "trace": cmd_trace, "quality": cmd_quality}[a.cmd](a)
