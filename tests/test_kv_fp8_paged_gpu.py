"""The fp8 paged KV path on the GPU: k_attn_prefill_paged_kv8<D>,
k_rope_kv8_prefill_paged and k_attn_decode_paged_kv8<G, ROPE>
(csrc/kv_fp8_paged.hip) must be BIT-equal to k_attn_prefill_kv8<D>,
k_rope_kv8_prefill and k_attn_decode_kv8<G, ROPE> (csrc/kv_fp8.hip) on the
same rows — the kernels differ in row addressing alone — through the ops,
LlamaModel.forward_prefill_paged and PagedSessionManager.

Pools and tables come from kv_fp8_paged_cases.py: scrambled physical blocks,
spare blocks, code 0x7F / scale inf (or a sentinel) in every row the kernels
may not touch, padding table entries that point at a poison block — never
out of range, so a wrong read is a NaN and not a fault."""

import pytest
import torch

from fei_amd import ops

import kv_fp8_paged_cases as kc
import paged_prefill_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("BS", pc.BLOCK_SIZES)
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
@pytest.mark.parametrize("G,D", pc.GD_PAIRS)
def test_attn_prefill_paged_fp8_bit_equal(G, D, case, BS):
    S, pos0 = case
    kc.run_attn_case(G, D, S, pos0, BS, DEV)


@pytest.mark.parametrize("G,D", pc.GD_PAIRS)
def test_attn_prefill_paged_fp8_block_size_1(G, D):
    S, pos0 = pc.BS1_CASE
    kc.run_attn_case(G, D, S, pos0, 1, DEV)


@pytest.mark.parametrize("BS", pc.BLOCK_SIZES)
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
@pytest.mark.parametrize("G,D", pc.GD_PAIRS)
def test_rope_kv_prefill_paged_fp8_bit_equal(G, D, case, BS):
    S, pos0 = case
    kc.run_append_case(pc.HQ // G, D, S, pos0, BS, DEV)


@pytest.mark.parametrize("G,D", pc.GD_PAIRS)
def test_rope_kv_prefill_paged_fp8_block_size_1(G, D):
    S, pos0 = pc.BS1_CASE
    kc.run_append_case(pc.HQ // G, D, S, pos0, 1, DEV)


@pytest.mark.parametrize("case", kc.DECODE_CASES, ids=kc.decode_id)
def test_attn_decode_paged_fp8_bit_equal(case):
    kc.run_decode_case(*case, DEV)


@pytest.mark.parametrize("n,splits", kc.FUSED_CASES)
def test_attn_decode_paged_fp8_rope_append_fused(n, splits):
    kc.run_fused_case(n, splits, DEV)


# -- model and sessions --------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    from fei_amd.engine.engine import LocalEngine
    return LocalEngine.create("llama3-tiny", max_seq_len=256, seed=7,
                              use_hip_graph=False, kv_quant="fp8")


def test_forward_prefill_paged_fp8_bit_equal(engine):
    assert engine.model.dtype == torch.bfloat16
    kc.run_forward_prefill_paged(engine.model, DEV)


def test_session_fp8_extend_gpu(engine):
    """open -> run -> extend -> run on an fp8 engine: the pool is fp8, and
    the turn's first token is the argmax of forward_prefill over a contiguous
    QuantKV gathered from the session's pool rows."""
    from fei_amd.engine.sessions import PagedSessionManager
    m = engine.model
    V = m.spec.vocab_size
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=32)
    assert mgr.pool.kv_dtype == "fp8"
    assert all(isinstance(c, ops.QuantKV) for c in mgr.pool.k + mgr.pool.v)
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
    kcs, vcs = m.new_kv_cache(1, 256, kv_quant="fp8")
    for li in range(len(kcs)):
        for cache, pool in ((kcs[li], mgr.pool.k[li]), (vcs[li], mgr.pool.v[li])):
            cache.data[0, :, :pos] = kc.gather_blocks(pool.data, blocks, pos, 16)
            cache.scale[0, :, :pos] = kc.gather_blocks(pool.scale, blocks,
                                                       pos, 16)
    tokens = torch.tensor([[last] + ids2], dtype=torch.int64, device=DEV)
    p0 = torch.full((1,), pos, dtype=torch.int32, device=DEV)
    want = int(m.forward_prefill(tokens, p0, kcs, vcs)[0].argmax())

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

def _args(D, BS, S=4, Hq=4, Hkv=2, splits=4):
    bf = torch.bfloat16
    q = torch.zeros(1, S, Hq, D, dtype=bf, device=DEV)
    kv = torch.zeros(1, S, Hkv, D, dtype=bf, device=DEV)
    kp, vp = (ops.QuantKV.zeros((4, Hkv, BS, D), DEV) for _ in range(2))
    table = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    pos0 = torch.zeros(1, dtype=torch.int32, device=DEV)
    return q, kv, kp, vp, table, pos0


def _untouched(*pools):
    return all(not bool(p.data.any()) and bool((p.scale == 1.0).all())
               for p in pools)


@pytest.mark.parametrize("D,BS,splits", [(96, 16, 4), (64, 12, 4),
                                         (64, 16, 33), (128, 16, 65)],
                         ids=["D96", "BS12", "splits33-D64", "splits65-D128"])
def test_refusals_launch_nothing(D, BS, splits):
    q, kv, kp, vp, table, pos0 = _args(D, BS)
    out = torch.full_like(q, 7.0)
    out1 = torch.full_like(q[:, 0], 7.0)
    rope = ops.ref.rope_table(64, D).to(DEV)
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q[:, 0], kp, vp, table, pos0, splits=splits,
                              out=out1)
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q[:, 0], kp, vp, table, pos0, splits=splits,
                              out=out1, k=kv[:, 0], v=kv[:, 0].clone(),
                              table=rope)
    if splits == 4:                 # the split limit is the decode op's alone
        with pytest.raises(ValueError):
            ops.attn_prefill_paged(q, kp, vp, table, pos0, out=out)
        with pytest.raises(ValueError):
            ops.rope_kv_prefill_paged(q, kv, kv.clone(), kp, vp, table, pos0,
                                      rope)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((out1 == 7.0).all())
    assert _untouched(kp, vp) and not bool(q.any())


def test_mixed_pools_refused():
    q, kv, kp, vp, table, pos0 = _args(64, 16)
    tensor_pool = torch.zeros(4, 2, 16, 64, dtype=torch.bfloat16, device=DEV)
    out = torch.full_like(q, 7.0)
    rope = ops.ref.rope_table(64, 64).to(DEV)
    with pytest.raises(TypeError):
        ops.attn_decode_paged(q[:, 0], kp, tensor_pool, table, pos0, splits=4)
    with pytest.raises(TypeError):
        ops.attn_prefill_paged(q, kp, tensor_pool, table, pos0, out=out)
    with pytest.raises(TypeError):
        ops.rope_kv_prefill_paged(q, kv, kv.clone(), kp, tensor_pool, table,
                                  pos0, rope)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and _untouched(kp)
    assert not bool(tensor_pool.any()) and not bool(q.any())


def test_entry_points_refuse():
    """The C entry points themselves return non-zero (and launch nothing)
    for what the Python checks stop first, then 0 for a valid call."""
    lib = ops.require_lib()
    q, kv, kp, vp, table, pos0 = _args(64, 16)
    out = torch.full_like(q, 7.0)
    splits = 4
    part_o = torch.full((1, 4, splits, 64), 7.0, device=DEV)
    part_ml = torch.full((1, 4, splits, 2), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    rope = ops.ref.rope_table(64, 64).to(DEV)
    pools = (kp.data.data_ptr(), kp.scale.data_ptr(), vp.data.data_ptr(),
             vp.scale.data_ptr())

    def attn(B=1, S=4, D=64, BS=16, Hq=4):
        return lib.fei_attn_prefill_paged_kv8(
            q.data_ptr(), *pools, table.data_ptr(), out.data_ptr(),
            pos0.data_ptr(), B, S, Hq, 2, D, BS, 4, 0.125, q.stride(1), st)

    def append(B=1, S=4, D=64, BS=16, Hq=4):
        return lib.fei_rope_kv8_prefill_paged(
            q.data_ptr(), kv.data_ptr(), kv.data_ptr(), *pools,
            table.data_ptr(), rope.data_ptr(), pos0.data_ptr(), B, S, Hq, 2,
            D, BS, 4, q.stride(1), kv.stride(1), st)

    def decode(B=1, S=1, D=64, BS=16, Hq=4):
        # S stands for the split count here: <= 0 is an empty problem too
        return lib.fei_attn_decode_paged_kv8(
            q.data_ptr(), *pools, table.data_ptr(), part_o.data_ptr(),
            part_ml.data_ptr(), pos0.data_ptr(), B, Hq, 2, D, BS, 4,
            splits if S > 0 else 0, 0.125, q.stride(1), None, None, None, 0,
            st)

    for fn in (attn, append, decode):
        assert fn(D=96) != 0 and fn(BS=12) != 0 and fn(BS=0) != 0
        assert fn(S=0) != 0 and fn(B=0) != 0
    assert decode(Hq=6) != 0 and decode(Hq=32) != 0       # GQA group 3, 16
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((part_o == 7.0).all())
    assert bool((part_ml == 7.0).all()) and _untouched(kp, vp)
    assert attn() == 0 and append() == 0 and decode() == 0
    torch.cuda.synchronize()
    assert not bool((part_ml == 7.0).all())
