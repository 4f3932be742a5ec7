"""Case tables and runners of the ragged paged prefill path
(k_rope_kv_prefill_paged_ragged, k_attn_prefill_paged_ragged<D>), shared by
test_prefill_ragged_gpu.py (device "cuda:0": the HIP kernels) and
test_prefill_ragged_cpu.py (device "cpu": the fp32 reference dispatch).

The criterion is equality, not a bound: for every sequence b the packed rows
[cu[b], cu[b+1]) of the ragged op must be bit-equal to what the UNIFORM
paged op (ops.attn_prefill_paged / ops.rope_kv_prefill_paged) gives with
B = 1 on that sequence alone, over the same pool and its own table row. The
ragged kernels differ from the uniform ones in where a workgroup finds its
sequence, nothing else.

Pools and tables are paged_prefill_cases.Paged's: scrambled physical blocks,
spare blocks, NaN (attention) or a sentinel (append) in every row that may
not be touched; on the GPU the padding table entries point at an in-range
NaN poison block, on the CPU they are -1. q is a strided view (token stride
wider than Hq * D, as the model's fused qkv output is); the out buffer has
sentinel rows past T that must survive.
"""

import functools
import math

import torch

from fei_amd import ops
from fei_amd.ops import reference as ref

from decode_shape_cases import NAN, bf16r, bits, put
from paged_prefill_cases import Paged, sentinel

HQ, MS = 4, 320
GD_PAIRS = [(g, d) for g in (1, 4) for d in (64, 128)]
# (lengths, pos0), the smallest at which packing can go wrong; len + pos0 <=
# MS everywhere.
CASES = [
    # a one-row sequence in front; sequence starts off the 64-row packed grid
    ((1, 65, 17), (37, 0, 64)),
    # a full tile, a tail, three q tiles over five key tiles, a key-tile edge
    # on the diagonal
    ((64, 3, 129, 64), (1, 63, 130, 63)),
    # B = 1: the uniform op's own problem
    ((129,), (1,)),
    # nine sequences inside one 64-row packed span
    (tuple(range(1, 10)), (0,) * 9),
]
BLOCK_SIZES = (16, 64, 128)
BS1_CASE = CASES[0]                # block size 1: one table entry per key
BMAX = max(len(c[0]) for c in CASES)
OUT_GUARD = 3                      # sentinel rows behind the packed output
Q_PAD = 24                         # extra elements per token row of q


def case_id(c):
    return "len" + "_".join(map(str, c[0])) + "-pos0_" + \
        "_".join(map(str, c[1]))


def cu_of(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def strided_rows(t, device, pad=Q_PAD):
    """[T, H, D] master -> a test tensor that is a view into a wider buffer:
    token stride H*D + pad, as the fused qkv output's views have."""
    T, H, D = t.shape
    buf = torch.zeros(T, H * D + pad)
    buf[:, :H * D] = t.reshape(T, H * D)
    buf = put(buf, device)
    return buf.as_strided((T, H, D), (H * D + pad, D, 1))


@functools.lru_cache(maxsize=None)
def _masters(hkv, D):
    g = torch.Generator().manual_seed(7000 + 10 * hkv + D)
    K = bf16r(torch.randn(BMAX, hkv, MS, D, generator=g))
    V = bf16r(torch.randn(BMAX, hkv, MS, D, generator=g))
    q = bf16r(2.0 * torch.randn(MS, HQ, D, generator=g))
    return K, V, q


def _paged(lens, pos0, BS, seed, device):
    return Paged([p + n for n, p in zip(lens, pos0)], BS, seed=seed,
                 pad="poison" if device != "cpu" else "minus1")


def run_attn_case(G, D, lens, pos0, BS, device):
    what = f"attn_prefill_paged_ragged G{G} D{D} len{lens} pos0{pos0} BS{BS}"
    hkv = HQ // G
    B, cu = len(lens), cu_of(lens)
    T = cu[-1]
    K, V, qm = _masters(hkv, D)
    pg = _paged(lens, pos0, BS, sum(lens) * 131 + BS, device)
    kp = put(pg.pool(K[:B], NAN), device)
    vp = put(pg.pool(V[:B], NAN), device)
    table = pg.table.to(device)
    q = strided_rows(qm[:T], device)
    q_before = q.clone()
    scale = 1.0 / math.sqrt(D)
    guard = put(sentinel((T + OUT_GUARD, HQ, D)), device)
    out = guard.clone()
    batch = ops.RaggedBatch(list(lens), list(pos0), table, device,
                            block_size=BS)
    ret = ops.attn_prefill_paged_ragged(q, kp, vp, batch, scale=scale,
                                        out=out)
    assert ret.data_ptr() == out.data_ptr(), f"{what}: out not used"
    assert torch.equal(bits(out[T:]), bits(guard[T:])), \
        f"{what}: rows past T written"
    assert not bool(torch.isnan(out.float()).any()), f"{what}: NaN read"
    for b in range(B):
        r = slice(cu[b], cu[b + 1])
        p0 = torch.tensor([pos0[b]], dtype=torch.int32, device=device)
        want = ops.attn_prefill_paged(q[r].unsqueeze(0), kp, vp,
                                      table[b:b + 1], p0, scale=scale)
        assert not bool(torch.isnan(want.float()).any())
        assert torch.equal(bits(out[r]), bits(want[0])), \
            f"{what}: sequence {b} differs from attn_prefill_paged alone"
    assert torch.equal(bits(q.contiguous()), bits(q_before.contiguous())), \
        f"{what}: q written"
    # without out=: a fresh [T, Hq, D] with the same bits
    fresh = ops.attn_prefill_paged_ragged(q, kp, vp, batch, scale=scale)
    assert tuple(fresh.shape) == (T, HQ, D), what
    assert torch.equal(bits(fresh), bits(out[:T])), f"{what}: out= differs"


def run_append_case(hkv, D, lens, pos0, BS, device):
    what = f"rope_kv_prefill_paged_ragged Hkv{hkv} D{D} len{lens} " \
           f"pos0{pos0} BS{BS}"
    B, cu = len(lens), cu_of(lens)
    T = cu[-1]
    g = torch.Generator().manual_seed(D + 7 * hkv + 13 * T)
    qm = bf16r(torch.randn(T, HQ, D, generator=g))
    km = bf16r(torch.randn(T, hkv, D, generator=g))
    vm = bf16r(torch.randn(T, hkv, D, generator=g))
    tab = ref.rope_table(MS, D).to(device)
    pg = _paged(lens, pos0, BS, sum(lens) * 17 + BS, device)
    table = pg.table.to(device)
    shape = (pg.num_blocks, hkv, BS, D)
    before = (put(sentinel(shape), device), put(-sentinel(shape), device))
    k, v = strided_rows(km, device, 8), strided_rows(vm, device, 8)
    # the uniform op, one sequence at a time, into its own pools
    q1 = strided_rows(qm, device)
    kp1, vp1 = before[0].clone(), before[1].clone()
    for b in range(B):
        r = slice(cu[b], cu[b + 1])
        p0 = torch.tensor([pos0[b]], dtype=torch.int32, device=device)
        ops.rope_kv_prefill_paged(q1[r].unsqueeze(0), k[r].unsqueeze(0),
                                  v[r].unsqueeze(0), kp1, vp1,
                                  table[b:b + 1], p0, tab)
    # the ragged op, once
    q2 = strided_rows(qm, device)
    kp2, vp2 = before[0].clone(), before[1].clone()
    batch = ops.RaggedBatch(list(lens), list(pos0), table, device)
    ret = ops.rope_kv_prefill_paged_ragged(q2, k, v, kp2, vp2, batch, tab)
    assert ret.data_ptr() == q2.data_ptr(), f"{what}: q is roped in place"
    assert torch.equal(bits(q2.contiguous()), bits(q1.contiguous())), \
        f"{what}: roped q"
    for got, one, old, name in ((kp2, kp1, before[0], "K"),
                                (vp2, vp1, before[1], "V")):
        want = old.clone()            # the sentinel, but for the rows appended
        for b in range(B):
            lo, hi = pos0[b], pos0[b] + lens[b]
            assert torch.equal(bits(pg.gather(got, b, lo, hi)),
                               bits(pg.gather(one, b, lo, hi))), \
                f"{what}: appended {name} rows of sequence {b}"
            blk, off = pg.index(b, lo, hi)
            blk, off = blk.to(device), off.to(device)
            want[blk, :, off] = one[blk, :, off]
        assert torch.equal(bits(got), bits(want)), \
            f"{what}: {name} pool written outside the appended rows"


def tiny_args(D, BS, device, dtype, S=4, Hq=4, Hkv=2, width=4):
    """One 4-token sequence at pos0 0 over zeroed pools: the refusal tests'
    arguments (q, kv, pool, table)."""
    q = torch.zeros(S, Hq, D, dtype=dtype, device=device)
    kv = torch.zeros(S, Hkv, D, dtype=dtype, device=device)
    pool = torch.zeros(4, Hkv, BS, D, dtype=dtype, device=device)
    table = torch.zeros(1, width, dtype=torch.int32, device=device)
    return q, kv, pool, table
