"""Masters, pools and case runners of the fp8 paged KV path
(csrc/kv_fp8_paged.hip: k_rope_kv8_prefill_paged, k_attn_decode_paged_kv8,
k_attn_prefill_paged_kv8), shared by test_kv_fp8_paged_gpu.py (device
"cuda:0": the HIP kernels) and test_kv_fp8_paged_cpu.py (device "cpu": the
reference dispatch of fei_amd.ops).

The criterion is equality, not a bound: a paged fp8 kernel differs from its
contiguous twin (csrc/kv_fp8.hip) in row addressing alone, so whatever the
contiguous op gives over a QuantKV cache, the paged op must give — bit for
bit — over a QuantKV pool that holds the same rows behind a scrambled block
table (paged_prefill_cases.Paged).

Masters are quantised on the CPU with reference.quant_kv_fp8. Rows get very
different magnitudes (base 1/8; some positions x8, others /64, in different
patterns for K and V, as in test_kv_fp8_gpu.py), so a swapped or mis-indexed
scale is far from a rounding error. Every pool row no valid table entry leads
to — the poison block that padding entries point at included — holds code
0x7F (e4m3fn NaN) and scale inf, or a sentinel in the append tests: a wrong
read shows as NaN, a wrong write as a changed sentinel. Padding entries point
at the poison block on the GPU (never out of range) and are -1 on the CPU.
"""

import functools
import math

import torch

from fei_amd import ops
from fei_amd.ops import reference as ref

import paged_prefill_cases as pc
from decode_shape_cases import bf16r, bits, put

INF = float("inf")
POISON_CODE, POISON_SCALE = 0x7F, INF
SENT_CODE, SENT_SCALE = 0x55, -3.0

B, HQ = pc.B, pc.HQ                      # prefill cases: 2 sequences, 4 q heads
DEC_HQ, DEC_HKV = 8, 2                   # decode cases

# decode attention: (n, splits, D, BS, pos); pos None = [n-1, max(n//2-1, 0)]
DECODE_CASES = (
    [(n, sp, 128, bs, None) for bs in (16, 64)
     for n, sp in ((1, 1), (7, 4), (20, 32), (300, 16))]
    # one sequence with chunks >= 64 keys, the other short, in one launch
    + [(2100, 32, 128, bs, (2099, 700)) for bs in (16, 64)]
    + [(300, 32, 64, 16, None),          # D = 64
       (300, 16, 128, 1, None)])         # one table entry per key
FUSED_CASES = [(n, sp) for n in (1, 20, 300) for sp in (4, 32)]


def decode_id(c):
    n, sp, D, bs, pos = c
    return f"n{n}-splits{sp}-D{D}-BS{bs}" + ("-mixed" if pos else "")


def _pad(device):
    return "poison" if device != "cpu" else "minus1"


@functools.lru_cache(maxsize=None)
def quant_master(nb, hkv, MS, D, seed, which):
    """(codes u8 [nb,hkv,MS,D], scales f32 [nb,hkv,MS]) of a random cache
    with rows of widely differing magnitudes, quantised on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = bf16r(torch.randn(nb, hkv, MS, D, generator=g) / 8)
    p = torch.arange(MS)
    up, down = ((p % 7 == 1, p % 5 == 2) if which == "k"
                else (p % 6 == 3, p % 4 == 1))
    x[:, :, up] *= 8.0
    x[:, :, down] /= 64.0
    return ref.quant_kv_fp8(x.to(torch.bfloat16))


def contiguous(master, n_rows, device):
    """QuantKV cache holding the first n_rows[b] rows; poison behind them."""
    codes, scales = (t.clone() for t in master)
    for b, n in enumerate(n_rows):
        codes[b, :, n:] = POISON_CODE
        scales[b, :, n:] = POISON_SCALE
    return ops.QuantKV(codes.to(device), scales.to(device))


def pool_of(pg, master, n_rows, device, code=POISON_CODE, scale=POISON_SCALE):
    """QuantKV pool behind pg's table holding the first n_rows[b] rows of
    the master; every other row of every block is (code, scale)."""
    codes, scales = master
    hkv, D = codes.shape[1], codes.shape[3]
    data = torch.full((pg.num_blocks, hkv, pg.BS, D), code, dtype=torch.uint8)
    sc = torch.full((pg.num_blocks, hkv, pg.BS), scale, dtype=torch.float32)
    for b, n in enumerate(n_rows):
        blk, off = pg.index(b, 0, n)
        data[blk, :, off] = codes[b, :, :n].transpose(0, 1)
        sc[blk, :, off] = scales[b, :, :n].transpose(0, 1)
    return ops.QuantKV(data.to(device), sc.to(device))


def clone8(c):
    return ops.QuantKV(c.data.clone(), c.scale.clone())


def gather8(pg, pool, b, lo, hi):
    """(codes [Hkv, hi-lo, D], scales [Hkv, hi-lo]) of logical rows lo..hi-1."""
    blk, off = pg.index(b, lo, hi)
    blk, off = blk.to(pool.data.device), off.to(pool.data.device)
    return (pool.data[blk, :, off].transpose(0, 1),
            pool.scale[blk, :, off].transpose(0, 1))


def same_bytes(a, b):
    """QuantKV a and b hold the same bytes (scales compared as bits: inf and
    negative sentinels included)."""
    return torch.equal(a.data, b.data) and \
        torch.equal(bits(a.scale), bits(b.scale))


# -- prefill attention ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _prefill_q(D):
    g = torch.Generator().manual_seed(4100 + D)
    return bf16r(2.0 * torch.randn(B, 129, HQ, D, generator=g))


def _prefill_masters(hkv, D):
    return (quant_master(B, hkv, pc.MS, D, 4200 + 10 * hkv + D, "k"),
            quant_master(B, hkv, pc.MS, D, 4300 + 10 * hkv + D, "v"))


@functools.lru_cache(maxsize=None)
def attn_reference(G, D, S, pos0, device):
    """(q, pos0 tensor, scale, contiguous-path output): once per case,
    shared by every block size."""
    K, V = _prefill_masters(HQ // G, D)
    n_rows = [p + S for p in pos0]
    qd = put(_prefill_q(D)[:, :S], device)
    p0 = torch.tensor(pos0, dtype=torch.int32, device=device)
    scale = 1.0 / math.sqrt(D)
    want = ops.attn_prefill(qd, contiguous(K, n_rows, device),
                            contiguous(V, n_rows, device), p0, scale=scale)
    assert not bool(torch.isnan(want.float()).any())
    return qd, p0, scale, want


def run_attn_case(G, D, S, pos0, BS, device):
    what = f"attn_prefill_paged fp8 G{G} D{D} S{S} pos0{pos0} BS{BS}"
    K, V = _prefill_masters(HQ // G, D)
    qd, p0, scale, want = attn_reference(G, D, S, pos0, device)
    n_rows = [p + S for p in pos0]
    pg = pc.Paged(n_rows, BS, seed=S * 131 + BS, pad=_pad(device))
    kp, vp = (pool_of(pg, m, n_rows, device) for m in (K, V))
    q_before = qd.clone()
    out = ops.attn_prefill_paged(qd, kp, vp, pg.table.to(device), p0,
                                 scale=scale)
    assert tuple(out.shape) == (B, S, HQ, D), what
    assert not bool(torch.isnan(out.float()).any()), f"{what}: NaN read"
    assert torch.equal(bits(out), bits(want)), \
        f"{what}: differs from attn_prefill over the contiguous QuantKV"
    assert torch.equal(bits(qd), bits(q_before)), f"{what}: q written"


# -- prefill append ---------------------------------------------------------------

def _sentinel8(shape, device):
    return ops.QuantKV(
        torch.full(shape, SENT_CODE, dtype=torch.uint8, device=device),
        torch.full(shape[:-1], SENT_SCALE, dtype=torch.float32, device=device))


def run_append_case(hkv, D, S, pos0, BS, device):
    what = f"rope_kv_prefill_paged fp8 Hkv{hkv} D{D} S{S} pos0{pos0} BS{BS}"
    g = torch.Generator().manual_seed(D + 7 * hkv + 13 * S)
    q = bf16r(torch.randn(B, S, HQ, D, generator=g))
    k = bf16r(torch.randn(B, S, hkv, D, generator=g))
    v = bf16r(torch.randn(B, S, hkv, D, generator=g))
    # token rows of very different magnitudes, K and V in different patterns
    s = torch.arange(S)
    k[:, s % 3 == 1] *= 8.0
    k[:, s % 5 == 2] /= 64.0
    v[:, s % 4 == 3] *= 8.0
    v[:, s % 3 == 0] /= 64.0
    tab = ref.rope_table(pc.MS, D).to(device)
    p0 = torch.tensor(pos0, dtype=torch.int32, device=device)
    # contiguous path
    q1 = put(q, device)
    Kc, Vc = (_sentinel8((B, hkv, pc.MS, D), device) for _ in range(2))
    ops.rope_kv_prefill(q1, put(k, device), put(v, device), Kc, Vc, p0, tab)
    # paged path: sentinel everywhere, the poison block included
    pg = pc.Paged([p + S for p in pos0], BS, seed=S * 17 + BS,
                  pad=_pad(device))
    shape = (pg.num_blocks, hkv, BS, D)
    kp, vp = _sentinel8(shape, device), _sentinel8(shape, device)
    before = (clone8(kp), clone8(vp))
    q2 = put(q, device)
    ret = ops.rope_kv_prefill_paged(q2, put(k, device), put(v, device), kp,
                                    vp, pg.table.to(device), p0, tab)
    assert ret.data_ptr() == q2.data_ptr(), f"{what}: q is roped in place"
    assert torch.equal(bits(q2), bits(q1)), f"{what}: roped q"
    for pool, old, cache, name in ((kp, before[0], Kc, "K"),
                                   (vp, before[1], Vc, "V")):
        want = clone8(old)
        for b in range(B):
            lo, hi = pos0[b], pos0[b] + S
            codes, scales = gather8(pg, pool, b, lo, hi)
            assert torch.equal(codes, cache.data[b, :, lo:hi]), \
                f"{what}: appended {name} codes of sequence {b}"
            assert torch.equal(bits(scales), bits(cache.scale[b, :, lo:hi])), \
                f"{what}: appended {name} scales of sequence {b}"
            assert not bool((scales == SENT_SCALE).any()), \
                f"{what}: a {name} scale was not written"
            blk, off = pg.index(b, lo, hi)
            blk, off = blk.to(device), off.to(device)
            want.data[blk, :, off] = cache.data[b, :, lo:hi].transpose(0, 1)
            want.scale[blk, :, off] = cache.scale[b, :, lo:hi].transpose(0, 1)
        assert same_bytes(pool, want), \
            f"{what}: {name} pool written outside the appended rows"


# -- decode attention ---------------------------------------------------------------

def _decode_setup(n, D, pos, device):
    MS = 4096 if n > 1024 else 1024
    if pos is None:
        pos = (n - 1, max(n // 2 - 1, 0))
    g = torch.Generator().manual_seed(20 + n + D)
    q = bf16r(2.0 * torch.randn(2, DEC_HQ, D, generator=g))
    K = quant_master(2, DEC_HKV, MS, D, 21 + n, "k")
    V = quant_master(2, DEC_HKV, MS, D, 22 + n, "v")
    return q, K, V, list(pos)


def run_decode_case(n, splits, D, BS, pos, device):
    what = f"attn_decode_paged fp8 n{n} splits{splits} D{D} BS{BS}"
    q, K, V, pos = _decode_setup(n, D, pos, device)
    n_rows = [p + 1 for p in pos]
    posd = torch.tensor(pos, dtype=torch.int32, device=device)
    want = ops.attn_decode(put(q, device), contiguous(K, n_rows, device),
                           contiguous(V, n_rows, device), posd, splits=splits)
    pg = pc.Paged(n_rows, BS, seed=n * 31 + BS, pad=_pad(device))
    out = ops.attn_decode_paged(put(q, device),
                                pool_of(pg, K, n_rows, device),
                                pool_of(pg, V, n_rows, device),
                                pg.table.to(device), posd, splits=splits)
    assert not bool(torch.isnan(want.float()).any()), what
    assert not bool(torch.isnan(out.float()).any()), f"{what}: NaN read"
    assert torch.equal(out, want), \
        f"{what}: differs from attn_decode over the contiguous QuantKV"


def run_fused_case(n, splits, device, D=128, BS=16):
    """The k=, v=, table= form: RoPE + quantised append of key n-1 inside the
    attention call. Rows [0, pos[b]) are valid, row pos[b] is poison until
    the call writes it."""
    what = f"attn_decode_paged fp8 fused n{n} splits{splits}"
    q, K, V, pos = _decode_setup(n, D, None, device)
    g = torch.Generator().manual_seed(900 + n)
    kin = bf16r(0.5 * torch.randn(2, DEC_HKV, D, generator=g))
    vin = bf16r(0.125 * torch.randn(2, DEC_HKV, D, generator=g))
    tab = ref.rope_table(1024, D).to(device)
    posd = torch.tensor(pos, dtype=torch.int32, device=device)
    kc, vc = contiguous(K, pos, device), contiguous(V, pos, device)
    want = ops.attn_decode(put(q, device), kc, vc, posd, splits=splits,
                           k=put(kin, device), v=put(vin, device), table=tab)
    pg = pc.Paged([p + 1 for p in pos], BS, seed=n * 37 + splits,
                  pad=_pad(device))
    kp, vp = pool_of(pg, K, pos, device), pool_of(pg, V, pos, device)
    before = (clone8(kp), clone8(vp))
    out = ops.attn_decode_paged(put(q, device), kp, vp, pg.table.to(device),
                                posd, splits=splits, k=put(kin, device),
                                v=put(vin, device), table=tab)
    assert not bool(torch.isnan(out.float()).any()), f"{what}: NaN"
    assert torch.equal(out, want), f"{what}: output"
    for pool, old, cache, name in ((kp, before[0], kc, "K"),
                                   (vp, before[1], vc, "V")):
        want_pool = clone8(old)
        for b, p in enumerate(pos):
            codes, scales = gather8(pg, pool, b, p, p + 1)
            assert torch.equal(codes, cache.data[b, :, p:p + 1]), \
                f"{what}: written {name} codes"
            assert torch.equal(bits(scales), bits(cache.scale[b, :, p:p + 1])), \
                f"{what}: written {name} scale"
            assert bool(torch.isfinite(scales).all()), \
                f"{what}: {name} scale not written"
            blk, off = pg.index(b, p, p + 1)
            blk, off = blk.to(device), off.to(device)
            want_pool.data[blk, :, off] = cache.data[b, :, p:p + 1].transpose(0, 1)
            want_pool.scale[blk, :, off] = \
                cache.scale[b, :, p:p + 1].transpose(0, 1)
        assert same_bytes(pool, want_pool), \
            f"{what}: {name} pool written outside the appended row"


# -- model ---------------------------------------------------------------------------

def gather_blocks(t, blocks, n, BS):
    """Logical rows 0..n-1 of a pool tensor ([nb,Hkv,BS,D] or [nb,Hkv,BS])
    behind a plain block list -> [Hkv, n, ...]."""
    p = torch.arange(n, device=t.device)
    blk = torch.tensor(blocks, device=t.device)[p // BS]
    return t[blk, :, p % BS].transpose(0, 1)


def run_forward_prefill_paged(model, device):
    """Two slices (40 tokens at 0, 23 at 40) by both paths: the logits and
    every layer's codes and scales are bit-equal."""
    m = model
    BS, n_blocks = 16, 9
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, m.spec.vocab_size, (1, 63), generator=g).to(device)
    kc, vc = m.new_kv_cache(1, 128, kv_quant="fp8")
    shape = (n_blocks, m.hkv_l, BS, m.D)

    def poison():
        return ops.QuantKV(
            torch.full(shape, POISON_CODE, dtype=torch.uint8, device=device),
            torch.full(shape[:-1], POISON_SCALE, dtype=torch.float32,
                       device=device))

    kp, vp = [poison() for _ in kc], [poison() for _ in kc]
    blocks = [5, 2, 7, 0]                   # 64 rows; block 8 is the poison
    pad = 8 if device != "cpu" else -1
    table = torch.tensor([blocks + [pad, pad]], dtype=torch.int32,
                         device=device)
    for lo, hi in ((0, 40), (40, 63)):
        p0 = torch.full((1,), lo, dtype=torch.int32, device=device)
        want = m.forward_prefill(ids[:, lo:hi], p0, kc, vc)
        got = m.forward_prefill_paged(ids[:, lo:hi], p0, kp, vp, table)
        assert got.shape == want.shape
        assert not bool(torch.isnan(got.float()).any())
        assert torch.equal(bits(got), bits(want)), f"logits of slice {lo}:{hi}"
    for li in range(len(kc)):
        for pool, cache in ((kp[li], kc[li]), (vp[li], vc[li])):
            assert torch.equal(gather_blocks(pool.data, blocks, 63, BS),
                               cache.data[0, :, :63]), f"layer {li} codes"
            assert torch.equal(gather_blocks(pool.scale, blocks, 63, BS),
                               cache.scale[0, :, :63]), f"layer {li} scales"
