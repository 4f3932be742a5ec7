"""Ragged paged prefill on the GPU: k_attn_prefill_paged_ragged<D> and
k_rope_kv_prefill_paged_ragged must be BIT-equal, sequence by sequence, to
k_attn_prefill_paged<D> and k_rope_kv_prefill_paged run with B = 1 on that
sequence alone (the kernels differ in where a workgroup finds its sequence,
nothing else) — through the ops, LlamaModel.forward_prefill_paged_ragged and
PagedSessionManager.open_many / extend_many. bf16 tensors are compared as
int16.

Pools and tables come from ragged_prefill_cases.py: scrambled physical
blocks, spare blocks, NaN (or a sentinel) in every row the kernels may not
touch, padding table entries that point at a NaN poison block — never out of
range, so a wrong read is a NaN and not a fault."""

import pytest
import torch

from fei_amd import ops

import ragged_prefill_cases as rc
from decode_shape_cases import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


@pytest.mark.parametrize("BS", rc.BLOCK_SIZES)
@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
@pytest.mark.parametrize("G,D", rc.GD_PAIRS)
def test_attn_prefill_paged_ragged_bit_equal(G, D, case, BS):
    lens, pos0 = case
    rc.run_attn_case(G, D, lens, pos0, BS, DEV)


@pytest.mark.parametrize("G,D", rc.GD_PAIRS)
def test_attn_prefill_paged_ragged_block_size_1(G, D):
    lens, pos0 = rc.BS1_CASE
    rc.run_attn_case(G, D, lens, pos0, 1, DEV)


@pytest.mark.parametrize("BS", rc.BLOCK_SIZES)
@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
@pytest.mark.parametrize("G,D", rc.GD_PAIRS)
def test_rope_kv_prefill_paged_ragged_bit_equal(G, D, case, BS):
    lens, pos0 = case
    rc.run_append_case(rc.HQ // G, D, lens, pos0, BS, DEV)


@pytest.mark.parametrize("G,D", rc.GD_PAIRS)
def test_rope_kv_prefill_paged_ragged_block_size_1(G, D):
    lens, pos0 = rc.BS1_CASE
    rc.run_append_case(rc.HQ // G, D, lens, pos0, 1, DEV)


# -- refusals --------------------------------------------------------------------

@pytest.mark.parametrize("D,BS", [(96, 16), (64, 12), (128, 48)])
def test_refusals_launch_nothing(D, BS):
    q, kv, pool, table = rc.tiny_args(D, BS, DEV, BF)
    out = torch.full_like(q, 7.0)
    kp, vp = pool.clone(), pool.clone()
    rope = ops.ref.rope_table(64, D).to(DEV)
    batch = ops.RaggedBatch([4], [0], table, DEV)
    with pytest.raises(ValueError):
        ops.attn_prefill_paged_ragged(q, kp, vp, batch, out=out)
    with pytest.raises(ValueError):
        ops.rope_kv_prefill_paged_ragged(q, kv, kv.clone(), kp, vp, batch,
                                         rope)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(kp.any()) \
        and not bool(vp.any()) and not bool(q.any())


def test_entry_points_refuse():
    """The C entry points themselves return non-zero (and launch nothing)
    for what the Python checks stop first, and for an empty problem."""
    lib = ops.require_lib()
    q, kv, pool, table = rc.tiny_args(64, 16, DEV, BF)
    out = torch.full_like(q, 7.0)
    vpool = pool.clone()
    st = torch.cuda.current_stream().cuda_stream
    rope = ops.ref.rope_table(64, 64).to(DEV)
    bt = ops.RaggedBatch([4], [0], table, DEV)

    def attn(T=4, B=1, n_tiles=1, D=64, BS=16):
        return lib.fei_attn_prefill_paged_ragged(
            q.data_ptr(), pool.data_ptr(), vpool.data_ptr(),
            bt.block_table.data_ptr(), out.data_ptr(), bt.pos0.data_ptr(),
            bt.cu_seqlens.data_ptr(), bt.tile_map.data_ptr(), n_tiles, T, B,
            4, 2, D, BS, 4, 0.125, q.stride(0), st)

    def append(T=4, B=1, D=64, BS=16):
        return lib.fei_rope_kv_prefill_paged_ragged(
            q.data_ptr(), kv.data_ptr(), kv.data_ptr(), pool.data_ptr(),
            vpool.data_ptr(), bt.block_table.data_ptr(), rope.data_ptr(),
            bt.pos0.data_ptr(), bt.cu_seqlens.data_ptr(),
            bt.tok_seq.data_ptr(), T, B, 4, 2, D, BS, 4, q.stride(0),
            kv.stride(0), st)

    for fn in (attn, append):
        assert fn(D=96) == 3 and fn(BS=12) == 4 and fn(BS=48) == 4
        assert fn(BS=0) == 4
        assert fn(T=0) == 1 and fn(B=0) == 1
    assert attn(n_tiles=0) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(pool.any()) \
        and not bool(vpool.any())
    assert attn() == 0 and append() == 0
    torch.cuda.synchronize()


def test_fp8_pool_has_no_ragged_kernel():
    q, kv, pool, table = rc.tiny_args(64, 16, DEV, BF)
    kp = ops.QuantKV.zeros(tuple(pool.shape), DEV)
    vp = ops.QuantKV.zeros(tuple(pool.shape), DEV)
    rope = ops.ref.rope_table(64, 64).to(DEV)
    batch = ops.RaggedBatch([4], [0], table, DEV)
    with pytest.raises(NotImplementedError):
        ops.attn_prefill_paged_ragged(q, kp, vp, batch)
    with pytest.raises(NotImplementedError):
        ops.rope_kv_prefill_paged_ragged(q, kv, kv.clone(), kp, vp, batch,
                                         rope)
    torch.cuda.synchronize()
    assert not bool(kp.data.any()) and not bool(vp.data.any())


# -- model ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    from fei_amd.engine.engine import LocalEngine
    return LocalEngine.create("llama3-tiny", max_seq_len=256, seed=7,
                              use_hip_graph=False)


def _gather(pool, blocks, lo, hi, BS):
    p = torch.arange(lo, hi, device=pool.device)
    blk = torch.tensor(blocks, device=pool.device)[p // BS]
    return pool[blk, :, p % BS].transpose(0, 1)            # [Hkv, n, D]


def _nan_pools(m, n_blocks, BS, device, dtype):
    shape = (n_blocks, m.hkv_l, BS, m.D)
    mk = lambda: [torch.full(shape, float("nan"), dtype=dtype, device=device)
                  for _ in m.layers]
    return mk(), mk()


def test_forward_ragged_single_sequence_bit_equal(engine):
    """Two slices (40 tokens at 0, 23 at 40) of ONE sequence by both paths:
    identical GEMM shapes, so the logits and every layer's KV rows are
    bit-equal to forward_prefill_paged."""
    m = engine.model
    assert m.dtype == BF
    BS, n_blocks = 16, 9
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, m.spec.vocab_size, (1, 63), generator=g).to(DEV)
    kp1, vp1 = _nan_pools(m, n_blocks, BS, DEV, BF)
    kp2, vp2 = _nan_pools(m, n_blocks, BS, DEV, BF)
    blocks = [5, 2, 7, 0]                   # 64 rows; block 8 is the poison
    table = torch.tensor([blocks + [8, 8]], dtype=torch.int32, device=DEV)
    for lo, hi in ((0, 40), (40, 63)):
        p0 = torch.full((1,), lo, dtype=torch.int32, device=DEV)
        want = m.forward_prefill_paged(ids[:, lo:hi], p0, kp1, vp1, table)
        batch = ops.RaggedBatch([hi - lo], [lo], table, DEV, block_size=BS)
        got = m.forward_prefill_paged_ragged(ids[0, lo:hi], batch, kp2, vp2)
        assert got.shape == want.shape
        assert torch.equal(bits(got), bits(want)), f"logits of slice {lo}:{hi}"
    for li in range(len(kp1)):
        for a, b in ((kp2[li], kp1[li]), (vp2[li], vp1[li])):
            assert torch.equal(bits(_gather(a, blocks, 0, 63, BS)),
                               bits(_gather(b, blocks, 0, 63, BS))), \
                f"layer {li}"


def _fp32_twin(m):
    """A CPU fp32 LlamaModel with m's (bf16) weights: its forwards go
    through the ops' reference dispatch."""
    from fei_amd.models.llama import LlamaModel
    t = LlamaModel(m.spec, torch.device("cpu"), dtype=torch.float32,
                   max_seq_len=m.max_seq_len)
    up = lambda w: w.detach().float().cpu()
    t.emb, t.norm_f, t.lm_head = up(m.emb), up(m.norm_f), up(m.lm_head)
    for lt, lm in zip(t.layers, m.layers):
        for name in ("norm_attn", "wqkv", "wo", "norm_mlp", "wgu", "wdown"):
            setattr(lt, name, up(getattr(lm, name)))
    return t


def test_forward_ragged_several_sequences_vs_fp32(engine):
    """Three sequences in one forward, then a second ragged forward that
    continues each at its own pos0. The GEMM M differs from the serial
    path's, so bits may differ: per sequence the ragged logits must be no
    further from an fp32 run of the same weights (CPU reference dispatch)
    than TWICE the serial paged path's own distance — both are bf16 chains
    that differ only in GEMM blocking."""
    m = engine.model
    twin = _fp32_twin(m)
    BS, n_blocks = 16, 16
    stages = [((40, 7, 70), (0, 0, 0)), ((5, 20, 3), (40, 7, 70))]
    rows = [[3, 9, 1], [12, 7], [6, 0, 14, 4, 10]]         # 15 = poison
    W = 6
    table = torch.full((3, W), 15, dtype=torch.int32)
    for b, blk in enumerate(rows):
        table[b, :len(blk)] = torch.tensor(blk, dtype=torch.int32)
    table_d = table.to(DEV)
    kpr, vpr = _nan_pools(m, n_blocks, BS, DEV, BF)         # ragged
    kps, vps = _nan_pools(m, n_blocks, BS, DEV, BF)         # serial
    kpf, vpf = _nan_pools(twin, n_blocks, BS, "cpu", torch.float32)
    g = torch.Generator().manual_seed(23)
    for lens, pos0 in stages:
        ids = [torch.randint(0, m.spec.vocab_size, (n,), generator=g)
               for n in lens]
        batch = ops.RaggedBatch(list(lens), list(pos0), table_d, DEV,
                                block_size=BS)
        got = m.forward_prefill_paged_ragged(torch.cat(ids).to(DEV), batch,
                                             kpr, vpr)
        assert tuple(got.shape) == (3, m.spec.vocab_size)
        got = got.float().cpu()
        assert bool(torch.isfinite(got).all())
        for b in range(3):
            p0 = torch.tensor([pos0[b]], dtype=torch.int32)
            serial = m.forward_prefill_paged(
                ids[b][None].to(DEV), p0.to(DEV), kps, vps,
                table_d[b:b + 1])[0].float().cpu()
            exact = twin.forward_prefill_paged(ids[b][None], p0, kpf, vpf,
                                               table[b:b + 1])[0]
            d_ragged = float((got[b] - exact).abs().max())
            d_serial = float((serial - exact).abs().max())
            assert d_ragged <= 2.0 * d_serial, \
                f"lens {lens} pos0 {pos0} sequence {b}: ragged is " \
                f"{d_ragged:.6g} from fp32, serial {d_serial:.6g}"


# -- sessions ---------------------------------------------------------------------

def test_open_many_extend_many_gpu(engine):
    from fei_amd.engine.sessions import PagedSessionManager
    V = engine.model.spec.vocab_size
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=48)
    free0 = mgr.pool.free_blocks()
    prompts = [[(17 * i + 3) % V for i in range(70)],
               [5, 9, 2],
               [(7 * i + 1) % V for i in range(23)]]
    sids = mgr.open_many(prompts, max_new_tokens=6)
    assert len(sids) == 3 and len(set(sids)) == 3
    for sid, p in zip(sids, prompts):
        s = mgr.sessions[sid]
        assert s.pos == len(p) and s.turn == 0 and len(s.generated) == 1
        assert s.prompt_ids == p and 0 <= s.generated[0] < V
    # one prompt alone: what open() gives
    solo_mgr = PagedSessionManager(engine, block_size=16, num_blocks=16)
    a = solo_mgr.open(prompts[0], max_new_tokens=6)
    b = solo_mgr.open_many([prompts[0]], max_new_tokens=6)[0]
    assert solo_mgr.sessions[a].generated == solo_mgr.sessions[b].generated
    mgr.run()
    turn1 = {}
    for sid in sids:
        res = mgr.result(sid)
        assert res["done"] and res["turn"] == 0
        assert 1 <= len(res["token_ids"]) <= 6
        assert all(0 <= t < V for t in res["token_ids"])
        turn1[sid] = (mgr.sessions[sid].pos, res["token_ids"])
    exts = [[3, 141, 59], [(11 * i + 5) % V for i in range(40)], [8]]
    firsts = mgr.extend_many(list(zip(sids, exts)), max_new_tokens=5)
    for sid, ext, first in zip(sids, exts, firsts):
        s = mgr.sessions[sid]
        assert s.pos == turn1[sid][0] + 1 + len(ext)
        assert s.turn == 1 and s.generated == [first] and 0 <= first < V
        assert s.context_ids[-len(ext):] == ext
    mgr.run()
    for sid, first in zip(sids, firsts):
        res = mgr.result(sid)
        assert res["done"] and res["turn"] == 1
        assert res["token_ids"][0] == first
        assert 1 <= len(res["token_ids"]) <= 5
        assert all(0 <= t < V for t in res["token_ids"])
    for sid in sids:
        mgr.close(sid)
    assert mgr.pool.free_blocks() == free0
