"""Continuous-batching serving throughput: N concurrent sessions with
staggered prompt lengths through PagedSessionManager (block-table
attention, per-step admission/retire) — the serving-path counterpart of
bench.py --batch (which measures the static-batch engine loop).
--kv-quant fp8 serves the sessions out of an fp8 KV pool.

--admit serial|batch|both measures ADMISSION instead (profiles/
ragged_prefill.md): N sessions of L tokens (default 8 x 256) and a ragged
mix, admitted by open() in a loop (serial) and by one open_many() (batch),
in the same process, alternating, --rounds times after two warm-up rounds.
Host clock around calls that end in a device synchronise; the figure is the
median round, the spread its min .. max. One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fei_amd.engine.engine import LocalEngine
from fei_amd.engine.sessions import PagedSessionManager

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--kv-quant", choices=["none", "fp8"], default="none",
                help="KV pool format (default: the unquantised pool)")
ap.add_argument("--admit", choices=["serial", "batch", "both"], default=None,
                help="measure admission (open() in a loop and/or open_many) "
                "instead of decode throughput")
ap.add_argument("--admit-n", type=int, default=8, help="sessions per round")
ap.add_argument("--admit-len", type=int, default=256,
                help="prompt tokens per session of the uniform shape")
ap.add_argument("--rounds", type=int, default=7,
                help="measured admission rounds per mode (at least 7)")
args = ap.parse_args()
KVQ = None if args.kv_quant == "none" else args.kv_quant
N = int(os.environ.get("SESS_N", "8"))
NEW = int(os.environ.get("SESS_NEW", "256"))
MODEL = os.environ.get("SESS_MODEL", "llama3-8b")
# a 40-token tool result next to a 1500-token first prompt: 3028 tokens, two
# forwards at the default max_batch_tokens
RAGGED_MIX = [40, 1500, 256, 64, 700, 128, 40, 300]


def bench_admission() -> None:
    eng = LocalEngine.create(MODEL, max_seq_len=4096, seed=7,
                             use_hip_graph=False)
    mgr = PagedSessionManager(eng, kv_quant=KVQ)
    rng = torch.Generator().manual_seed(5)
    hi = min(16000, eng.spec.vocab_size - 2)
    sync = torch.cuda.synchronize if torch.cuda.is_available() \
        else (lambda: None)
    modes = ["serial", "batch"] if args.admit == "both" else [args.admit]
    rounds = max(7, args.rounds)

    def admit(mode, prompts):
        sync()
        t0 = time.perf_counter()
        if mode == "serial":
            sids = [mgr.open(p, max_new_tokens=NEW) for p in prompts]
        else:
            sids = mgr.open_many(prompts, max_new_tokens=NEW)
        sync()
        dt = (time.perf_counter() - t0) * 1e3
        firsts = [mgr.sessions[s].generated[0] for s in sids]
        for s in sids:
            mgr.close(s)
        return dt, firsts

    shapes = [("uniform", [args.admit_len] * args.admit_n),
              ("ragged mix", RAGGED_MIX)]
    for name, lens in shapes:
        prompts = [torch.randint(4, hi, (n,), generator=rng).tolist()
                   for n in lens]
        firsts = {}
        for _ in range(2):                          # warm-up, both modes
            for mode in modes:
                firsts[mode] = admit(mode, prompts)[1]
        times = {mode: [] for mode in modes}
        for _ in range(rounds):                     # alternating
            for mode in modes:
                times[mode].append(admit(mode, prompts)[0])
        res = {"metric": "session admission ms (paged prefill)",
               "shape": name, "lens": lens, "tokens": sum(lens),
               "rounds": rounds, "model": MODEL,
               "kv_dtype": mgr.pool.kv_dtype, "data": "synthetic"}
        for mode in modes:
            t = times[mode]
            res[f"{mode}_ms"] = round(statistics.median(t), 2)
            res[f"{mode}_ms_min_max"] = [round(min(t), 2), round(max(t), 2)]
        if len(modes) == 2:
            res["batch_over_serial"] = round(
                res["batch_ms"] / res["serial_ms"], 4)
            # bf16 GEMMs of different M: a near tie may pick another token
            res["first_tokens_equal"] = sum(
                a == b for a, b in zip(firsts["serial"], firsts["batch"]))
        print(json.dumps(res), flush=True)
    eng.shutdown()


if args.admit:
    bench_admission()
    sys.exit(0)
eng = LocalEngine.create(MODEL, max_seq_len=4096, seed=7)
# the engine (and so the memory left for the pool) is the same in both modes:
# only the pool's format changes
mgr = PagedSessionManager(eng, kv_quant=KVQ)
rng = torch.Generator().manual_seed(5)
sids = []
for i in range(N):
    plen = 64 + 48 * i                      # staggered contexts
    hi = min(16000, eng.spec.vocab_size - 2)
    ids = torch.randint(4, hi, (plen,), generator=rng).tolist()
    sids.append(mgr.open(ids, max_new_tokens=NEW))
if torch.cuda.is_available():
    torch.cuda.synchronize()
t0 = time.perf_counter()
steps = 0
CH = int(os.environ.get("SESS_CHUNK", "8"))
while mgr.active and steps < NEW + 8:
    k = min(CH, NEW + 8 - steps)
    mgr.step_chunk(k)
    steps += k
if torch.cuda.is_available():
    torch.cuda.synchronize()
dt = time.perf_counter() - t0
toks = sum(len(mgr.result(s)["token_ids"]) for s in sids)
print(json.dumps({
    "metric": "serving aggregate tok/s (continuous batching, paged KV)",
    "value": round(toks / dt, 1), "unit": "tok/s", "sessions": N,
    "new_tokens_per_session": NEW, "steps": steps,
    "ms_per_step": round(dt / steps * 1000, 3), "model": MODEL,
    "kv_dtype": mgr.pool.kv_dtype, "pool_blocks": mgr.pool.num_blocks,
    "data": "synthetic"}))
