"""Paged prefill on the GPU: k_attn_prefill_paged<D> and
k_rope_kv_prefill_paged must be BIT-equal to k_attn_prefill<D> and
k_rope_kv_prefill on the same rows (the kernels differ in row addressing
alone), through the ops, LlamaModel.forward_prefill_paged and
PagedSessionManager.extend. bf16 tensors are compared as int16.

Pools and tables come from paged_prefill_cases.py: scrambled physical
blocks, spare blocks, NaN (or a sentinel) in every row the kernels may not
touch, padding table entries that point at a NaN poison block — never out of
range, so a wrong read is a NaN and not a fault."""

import pytest
import torch

from fei_amd import ops

import paged_prefill_cases as pc
from decode_shape_cases import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("BS", pc.BLOCK_SIZES)
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
@pytest.mark.parametrize("G,D", pc.GD_PAIRS)
def test_attn_prefill_paged_bit_equal(G, D, case, BS):
    S, pos0 = case
    pc.run_attn_case(G, D, S, pos0, BS, DEV)


@pytest.mark.parametrize("G,D", pc.GD_PAIRS)
def test_attn_prefill_paged_block_size_1(G, D):
    S, pos0 = pc.BS1_CASE
    pc.run_attn_case(G, D, S, pos0, 1, DEV)


@pytest.mark.parametrize("BS", pc.BLOCK_SIZES)
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
@pytest.mark.parametrize("G,D", pc.GD_PAIRS)
def test_rope_kv_prefill_paged_bit_equal(G, D, case, BS):
    S, pos0 = case
    pc.run_append_case(pc.HQ // G, D, S, pos0, BS, DEV)


def test_rope_kv_prefill_paged_block_size_1():
    S, pos0 = pc.BS1_CASE
    pc.run_append_case(2, 128, S, pos0, 1, DEV)


# -- model and sessions --------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    from fei_amd.engine.engine import LocalEngine
    return LocalEngine.create("llama3-tiny", max_seq_len=256, seed=7,
                              use_hip_graph=False)


def _gather(pool, blocks, n, BS):
    p = torch.arange(n, device=pool.device)
    blk = torch.tensor(blocks, device=pool.device)[p // BS]
    return pool[blk, :, p % BS].transpose(0, 1)            # [Hkv, n, D]


def test_forward_prefill_paged_bit_equal(engine):
    """Two slices (40 tokens at 0, 23 at 40) by both paths: identical GEMM
    shapes, so the logits and every layer's KV rows are bit-equal."""
    m = engine.model
    assert m.dtype == torch.bfloat16
    BS, n_blocks = 16, 9
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, m.spec.vocab_size, (1, 63), generator=g).to(DEV)
    kc, vc = m.new_kv_cache(1, 128)
    shape = (n_blocks, m.hkv_l, BS, m.D)
    nan = float("nan")
    kp = [torch.full(shape, nan, dtype=m.dtype, device=DEV) for _ in kc]
    vp = [torch.full(shape, nan, dtype=m.dtype, device=DEV) for _ in kc]
    blocks = [5, 2, 7, 0]                   # 64 rows; block 8 is the poison
    table = torch.tensor([blocks + [8, 8]], dtype=torch.int32, device=DEV)
    for lo, hi in ((0, 40), (40, 63)):
        p0 = torch.full((1,), lo, dtype=torch.int32, device=DEV)
        want = m.forward_prefill(ids[:, lo:hi], p0, kc, vc)
        got = m.forward_prefill_paged(ids[:, lo:hi], p0, kp, vp, table)
        assert got.shape == want.shape
        assert torch.equal(bits(got), bits(want)), f"logits of slice {lo}:{hi}"
    for li in range(len(kc)):
        for pool, cache in ((kp[li], kc[li]), (vp[li], vc[li])):
            assert torch.equal(bits(_gather(pool, blocks, 63, BS)),
                               bits(cache[0, :, :63])), f"layer {li}"


def test_session_extend_gpu(engine):
    """open -> run -> extend -> run: the turn's first token is the argmax of
    forward_prefill over a contiguous gather of the session's pool rows."""
    from fei_amd.engine.sessions import PagedSessionManager
    m = engine.model
    V = m.spec.vocab_size
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=32)
    free0 = mgr.pool.free_blocks()
    sid = mgr.open("paged session, first turn", max_new_tokens=6)
    mgr.run()
    s = mgr.sessions[sid]
    assert s.done
    turn1 = mgr.result(sid)["token_ids"]
    pos, last = s.pos, s.generated[-1]
    blocks = list(mgr.pool.table(sid).blocks)
    ids2 = [3, 141, 59, 26, 5, 358, 97, 93, 23, 84, 62, 64, 33, 83, 27, 95, 2]
    # contiguous copies of the rows the session holds, before the extend
    kc, vc = m.new_kv_cache(1, 256)
    for li in range(len(kc)):
        kc[li][0, :, :pos] = _gather(mgr.pool.k[li], blocks, pos, 16)
        vc[li][0, :, :pos] = _gather(mgr.pool.v[li], blocks, pos, 16)
    tokens = torch.tensor([[last] + ids2], dtype=torch.int64, device=DEV)
    p0 = torch.full((1,), pos, dtype=torch.int32, device=DEV)
    want = int(m.forward_prefill(tokens, p0, kc, vc)[0].argmax())

    first = mgr.extend(sid, ids2, max_new_tokens=6)
    assert first == want
    assert mgr.sessions[sid].pos == pos + 1 + len(ids2)
    assert mgr.result(sid)["turn"] == 1
    mgr.run()
    res = mgr.result(sid)
    assert res["done"] and res["token_ids"][0] == first
    assert 1 <= len(res["token_ids"]) <= 6
    assert all(0 <= t < V for t in turn1 + res["token_ids"])
    mgr.close(sid)
    assert mgr.pool.free_blocks() == free0


# -- refusals --------------------------------------------------------------------

def _args(D, BS, S=4):
    bf = torch.bfloat16
    q = torch.zeros(1, S, 4, D, dtype=bf, device=DEV)
    kv = torch.zeros(1, S, 2, D, dtype=bf, device=DEV)
    pool = torch.zeros(4, 2, BS, D, dtype=bf, device=DEV)
    table = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    pos0 = torch.zeros(1, dtype=torch.int32, device=DEV)
    return q, kv, pool, table, pos0


@pytest.mark.parametrize("D,BS", [(96, 16), (64, 12), (128, 48)])
def test_refusals_launch_nothing(D, BS):
    q, kv, pool, table, pos0 = _args(D, BS)
    out = torch.full_like(q, 7.0)
    kp, vp = pool.clone(), pool.clone()
    rope = ops.ref.rope_table(64, D).to(DEV)
    with pytest.raises(ValueError):
        ops.attn_prefill_paged(q, kp, vp, table, pos0, out=out)
    with pytest.raises(ValueError):
        ops.rope_kv_prefill_paged(q, kv, kv.clone(), kp, vp, table, pos0, rope)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(kp.any()) \
        and not bool(vp.any()) and not bool(q.any())


def test_entry_points_refuse():
    """The C entry points themselves return non-zero (and launch nothing)
    for what the Python checks stop first."""
    lib = ops.require_lib()
    q, kv, pool, table, pos0 = _args(64, 16)
    out = torch.full_like(q, 7.0)
    vpool = pool.clone()
    st = torch.cuda.current_stream().cuda_stream
    rope = ops.ref.rope_table(64, 64).to(DEV)

    def attn(B=1, S=4, D=64, BS=16):
        return lib.fei_attn_prefill_paged(
            q.data_ptr(), pool.data_ptr(), vpool.data_ptr(), table.data_ptr(),
            out.data_ptr(), pos0.data_ptr(), B, S, 4, 2, D, BS, 4, 0.125,
            q.stride(1), st)

    def append(B=1, S=4, D=64, BS=16):
        return lib.fei_rope_kv_prefill_paged(
            q.data_ptr(), kv.data_ptr(), kv.data_ptr(), pool.data_ptr(),
            vpool.data_ptr(), table.data_ptr(), rope.data_ptr(),
            pos0.data_ptr(), B, S, 4, 2, D, BS, 4, q.stride(1), kv.stride(1),
            st)

    for fn in (attn, append):
        assert fn(D=96) != 0 and fn(BS=12) != 0 and fn(BS=0) != 0
        assert fn(S=0) != 0 and fn(B=0) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(pool.any()) \
        and not bool(vpool.any())
    assert attn() == 0 and append() == 0
    torch.cuda.synchronize()
