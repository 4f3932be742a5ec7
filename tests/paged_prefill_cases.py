"""Case tables and pool builders of the paged prefill path
(k_rope_kv_prefill_paged, k_attn_prefill_paged<D>), shared by
test_prefill_paged_gpu.py (device "cuda:0": the HIP kernels, bit equality
with the contiguous kernels) and test_prefill_paged_cpu.py (device "cpu":
the fp32 reference dispatch, exact equality with the contiguous reference).

The criterion is equality, not a bound: the paged kernels differ from the
contiguous ones in row addressing alone, so whatever the contiguous path
gives for a cache, the paged path must give for a pool that holds the same
rows behind a scrambled block table.

Every pool row no table entry may lead to is NaN (attention) or a sentinel
(append): a wrong read shows as NaN, a wrong write as a changed sentinel.
On the GPU the table entries beyond a sequence's last needed block point at
a NaN "poison" block, never out of range; on the CPU they are -1.
"""

import functools
import math

import torch

from fei_amd import ops
from fei_amd.ops import reference as ref

from decode_shape_cases import NAN, bf16r, bits, put

B, HQ, MS = 2, 4, 320
GD_PAIRS = [(g, d) for g in (1, 4) for d in (64, 128)]
# (S, (pos0 of sequence 0, of sequence 1)), from prefill_shape_cases.py's
# CAUSAL_CASES: one row; a key-tile edge on the diagonal; a second wave; a
# full q tile; a second workgroup; three q tiles over five key tiles.
# For the append with BS = 16: (17, (64, 15)) writes rows 15..31 — it
# crosses the block edge at 16 and ends exactly on the one at 32; with
# BS = 64, (64, (1, 63)) crosses 64 and (65, (64, 15)) starts on it.
CASES = [
    (1, (0, 37)),
    (3, (1, 63)),
    (17, (64, 15)),
    (64, (1, 63)),
    (65, (64, 15)),
    (129, (130, 1)),
]
# smaller than, equal to and larger than the 64-key tile
BLOCK_SIZES = (16, 64, 128)
BS1_CASE = (65, (64, 15))          # block size 1: one table entry per key
SPARE_BLOCKS = 3
TABLE_PAD = 2                      # padding entries per table row


def case_id(c):
    return f"S{c[0]}-pos0_{c[1][0]}_{c[1][1]}"


def sentinel(shape):
    """bf16-exact, position-dependent and never a value randn rounds to
    often: a changed element shows in a bit compare."""
    n = math.prod(shape)
    return (((torch.arange(n) % 251).float() - 125.0) / 8.0).view(shape)


class Paged:
    """A scrambled block table for B sequences of n_rows[b] rows, and pools
    built behind it. Physical blocks are a seeded random permutation; the
    pool holds SPARE_BLOCKS unused blocks and one poison block."""

    def __init__(self, n_rows, BS, seed, pad="poison"):
        self.BS, self.n_rows = BS, list(n_rows)
        need = [-(-n // BS) for n in n_rows]
        total = sum(need)
        self.num_blocks = total + SPARE_BLOCKS + 1
        g = torch.Generator().manual_seed(seed)
        perm = torch.randperm(self.num_blocks, generator=g).tolist()
        self.poison = perm[-1]
        width = max(need) + TABLE_PAD
        fill = self.poison if pad == "poison" else -1
        self.table = torch.full((len(n_rows), width), fill, dtype=torch.int32)
        at = 0
        for b, nb in enumerate(need):
            self.table[b, :nb] = torch.tensor(perm[at:at + nb],
                                              dtype=torch.int32)
            at += nb

    def index(self, b, lo, hi):
        """(physical block, row within the block) of logical rows lo..hi-1."""
        p = torch.arange(lo, hi)
        return self.table[b, p // self.BS].long(), p % self.BS

    def pool(self, master, fill):
        """CPU f32 pool [num_blocks, Hkv, BS, D] holding the first n_rows[b]
        rows of master [B, Hkv, MS, D]; every other row is ``fill`` (a value
        or a full-shape tensor)."""
        hkv, D = master.shape[1], master.shape[3]
        shape = (self.num_blocks, hkv, self.BS, D)
        pool = fill.clone() if torch.is_tensor(fill) else torch.full(shape, fill)
        for b, n in enumerate(self.n_rows):
            blk, off = self.index(b, 0, n)
            pool[blk, :, off] = master[b, :, :n].transpose(0, 1)
        return pool

    def gather(self, pool, b, lo, hi):
        """[Hkv, hi-lo, D] logical rows lo..hi-1 of sequence b."""
        blk, off = self.index(b, lo, hi)
        return pool[blk.to(pool.device), :, off.to(pool.device)].transpose(0, 1)


@functools.lru_cache(maxsize=None)
def _masters(hkv, D):
    g = torch.Generator().manual_seed(4000 + 10 * hkv + D)
    K = bf16r(torch.randn(B, hkv, MS, D, generator=g))
    V = bf16r(torch.randn(B, hkv, MS, D, generator=g))
    q = bf16r(2.0 * torch.randn(B, 129, HQ, D, generator=g))
    return K, V, q


@functools.lru_cache(maxsize=None)
def attn_reference(G, D, S, pos0, device):
    """(q, pos0 tensor, scale, contiguous-path output), computed once per
    case and shared by every block size. The contiguous caches are NaN past
    pos0 + S, like the pools."""
    hkv = HQ // G
    K, V, q = _masters(hkv, D)
    caches = []
    for m in (K, V):
        t = torch.full_like(m, NAN)
        for b in range(B):
            n = pos0[b] + S
            t[b, :, :n] = m[b, :, :n]
        caches.append(put(t, device))
    qd = put(q[:, :S], device)
    p0 = torch.tensor(pos0, dtype=torch.int32, device=device)
    scale = 1.0 / math.sqrt(D)
    want = ops.attn_prefill(qd, caches[0], caches[1], p0, scale=scale)
    assert not bool(torch.isnan(want.float()).any())
    return qd, p0, scale, want


def run_attn_case(G, D, S, pos0, BS, device):
    what = f"attn_prefill_paged G{G} D{D} S{S} pos0{pos0} BS{BS}"
    hkv = HQ // G
    K, V, _ = _masters(hkv, D)
    qd, p0, scale, want = attn_reference(G, D, S, pos0, device)
    pg = Paged([p + S for p in pos0], BS, seed=S * 131 + BS,
               pad="poison" if device != "cpu" else "minus1")
    kp, vp = put(pg.pool(K, NAN), device), put(pg.pool(V, NAN), device)
    q_before = qd.clone()
    out = ops.attn_prefill_paged(qd, kp, vp, pg.table.to(device), p0,
                                 scale=scale)
    assert tuple(out.shape) == (B, S, HQ, D), what
    assert not bool(torch.isnan(out.float()).any()), f"{what}: NaN read"
    assert torch.equal(bits(out), bits(want)), \
        f"{what}: differs from attn_prefill on the same rows"
    assert torch.equal(bits(qd), bits(q_before)), f"{what}: q written"


def run_append_case(hkv, D, S, pos0, BS, device):
    what = f"rope_kv_prefill_paged Hkv{hkv} D{D} S{S} pos0{pos0} BS{BS}"
    g = torch.Generator().manual_seed(D + 7 * hkv + 13 * S)
    q = bf16r(torch.randn(B, S, HQ, D, generator=g))
    k = bf16r(torch.randn(B, S, hkv, D, generator=g))
    v = bf16r(torch.randn(B, S, hkv, D, generator=g))
    tab = ref.rope_table(MS, D).to(device)
    p0 = torch.tensor(pos0, dtype=torch.int32, device=device)
    # contiguous path
    q1 = put(q, device)
    Kc = put(sentinel((B, hkv, MS, D)), device)
    Vc = Kc.clone()
    ops.rope_kv_prefill(q1, put(k, device), put(v, device), Kc, Vc, p0, tab)
    # paged path: sentinel everywhere, the poison block included
    pg = Paged([p + S for p in pos0], BS, seed=S * 17 + BS,
               pad="poison" if device != "cpu" else "minus1")
    shape = (pg.num_blocks, hkv, BS, D)
    kp = put(sentinel(shape), device)
    vp = put(-sentinel(shape), device)
    before = (kp.clone(), vp.clone())
    q2 = put(q, device)
    ret = ops.rope_kv_prefill_paged(q2, put(k, device), put(v, device), kp,
                                    vp, pg.table.to(device), p0, tab)
    assert ret.data_ptr() == q2.data_ptr(), f"{what}: q is roped in place"
    assert torch.equal(bits(q2), bits(q1)), f"{what}: roped q"
    for pool, old, cache, name in ((kp, before[0], Kc, "K"),
                                   (vp, before[1], Vc, "V")):
        want = old.clone()
        for b in range(B):
            lo, hi = pos0[b], pos0[b] + S
            got = pg.gather(pool, b, lo, hi)
            assert torch.equal(bits(got), bits(cache[b, :, lo:hi])), \
                f"{what}: appended {name} rows of sequence {b}"
            blk, off = pg.index(b, lo, hi)
            want[blk.to(device), :, off.to(device)] = \
                cache[b, :, lo:hi].transpose(0, 1)
        assert torch.equal(bits(pool), bits(want)), \
            f"{what}: {name} pool written outside the appended rows"
