"""The fp8 paged KV path without a GPU.

Ops: on CPU tensors fei_amd.ops.attn_prefill_paged / rope_kv_prefill_paged /
attn_decode_paged gather the logical rows of a QuantKV pool, dequantise them
and run the contiguous fp8 reference, so they must equal the contiguous fp8
ops exactly over scrambled tables whose padding entries are -1.

Engine layers: PagedKVPool(kv_quant="fp8"), PagedSessionManager's
inheritance of the engine's kv_quant, and the multi-turn contract on an fp8
pool: a paged session that is opened, run, extended and run again emits in
every turn exactly what LocalEngine(kv_quant="fp8").generate emits for the
whole context, greedy, on the CPU llama3-tiny; after open() the session's
codes and scales equal the solo engine's cache rows bit for bit."""

import pytest
import torch

from fei_amd import ops
from fei_amd.engine.engine import LocalEngine
from fei_amd.engine.kv_cache import PagedKVPool
from fei_amd.engine.sessions import PagedSessionManager

import kv_fp8_paged_cases as kc
import paged_prefill_cases as pc

CPU = torch.device("cpu")


# -- ops -----------------------------------------------------------------------

@pytest.mark.parametrize("BS", pc.BLOCK_SIZES + (1,))
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_attn_prefill_paged_fp8_equals_reference(case, BS):
    S, pos0 = case
    for G, D in ((1, 64), (4, 128)):
        kc.run_attn_case(G, D, S, pos0, BS, "cpu")


@pytest.mark.parametrize("BS", pc.BLOCK_SIZES + (1,))
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_rope_kv_prefill_paged_fp8_equals_reference(case, BS):
    S, pos0 = case
    for hkv, D in ((4, 64), (1, 128)):
        kc.run_append_case(hkv, D, S, pos0, BS, "cpu")


@pytest.mark.parametrize("case", kc.DECODE_CASES, ids=kc.decode_id)
def test_attn_decode_paged_fp8_equals_reference(case):
    kc.run_decode_case(*case, "cpu")


@pytest.mark.parametrize("n,splits", kc.FUSED_CASES)
def test_attn_decode_paged_fp8_fused_equals_reference(n, splits):
    kc.run_fused_case(n, splits, "cpu")


def test_attn_prefill_paged_fp8_bf16_rounding():
    """With a bf16 q the dequantised rows are rounded to bf16 first, as
    attn_prefill does (the kernel stages bf16(f32(code) * scale))."""
    S, pos0, D, BS = 17, (64, 15), 64, 16
    K = kc.quant_master(2, 2, pc.MS, D, 1, "k")
    V = kc.quant_master(2, 2, pc.MS, D, 2, "v")
    n_rows = [p + S for p in pos0]
    g = torch.Generator().manual_seed(3)
    q = torch.randn(2, S, 4, D, generator=g).to(torch.bfloat16)
    p0 = torch.tensor(pos0, dtype=torch.int32)
    want = ops.attn_prefill(q, kc.contiguous(K, n_rows, "cpu"),
                            kc.contiguous(V, n_rows, "cpu"), p0)
    pg = pc.Paged(n_rows, BS, seed=5, pad="minus1")
    got = ops.attn_prefill_paged(q, kc.pool_of(pg, K, n_rows, "cpu"),
                                 kc.pool_of(pg, V, n_rows, "cpu"), pg.table, p0)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)


def test_mixed_pools_refused():
    kp = ops.QuantKV.zeros((4, 2, 16, 64), CPU)
    vp = torch.zeros(4, 2, 16, 64)
    q = torch.zeros(1, 4, 4, 64)
    kv = torch.zeros(1, 4, 2, 64)
    table = torch.zeros(1, 2, dtype=torch.int32)
    pos0 = torch.zeros(1, dtype=torch.int32)
    rope = ops.ref.rope_table(64, 64)
    with pytest.raises(TypeError):
        ops.attn_decode_paged(q[:, 0], kp, vp, table, pos0)
    with pytest.raises(TypeError):
        ops.attn_prefill_paged(q, kp, vp, table, pos0)
    with pytest.raises(TypeError):
        ops.rope_kv_prefill_paged(q, kv, kv.clone(), vp, kp, table, pos0, rope)
    assert not bool(kp.data.any()) and not bool(vp.any())


def test_block_size_not_a_power_of_two():
    kp, vp = (ops.QuantKV.zeros((4, 2, 12, 64), CPU) for _ in range(2))
    q = torch.zeros(1, 4, 4, 64)
    table = torch.zeros(1, 2, dtype=torch.int32)
    pos0 = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q[:, 0], kp, vp, table, pos0)
    with pytest.raises(ValueError):
        ops.attn_prefill_paged(q, kp, vp, table, pos0)


# -- PagedKVPool(kv_quant="fp8") --------------------------------------------------

def _pool(n=8, bs=4, **kw):
    return PagedKVPool(num_layers=2, num_kv_heads=3, head_dim=8, block_size=bs,
                       num_blocks=n, device=CPU, dtype=torch.float32, **kw)


def test_pool_layers():
    pool = _pool(kv_quant="fp8")
    assert pool.kv_dtype == "fp8" and pool.kv_quant == "fp8"
    assert len(pool.k) == 2 and len(pool.v) == 2
    for c in pool.k + pool.v:
        assert isinstance(c, ops.QuantKV)
        assert c.data.dtype == torch.uint8 and c.data.shape == (8, 3, 4, 8)
        assert c.scale.dtype == torch.float32 and c.scale.shape == (8, 3, 4)
    assert len({c.data.data_ptr() for c in pool.k + pool.v}) == 4


def test_pool_kv_dtype_of_plain_pools():
    assert _pool().kv_dtype == "fp32" and _pool().kv_quant is None
    assert isinstance(_pool().k[0], torch.Tensor)
    bf = PagedKVPool(1, 1, 8, block_size=4, num_blocks=2, device=CPU,
                     dtype=torch.bfloat16)
    assert bf.kv_dtype == "bf16"


@pytest.mark.parametrize("L,Hkv,D,BS", [(2, 2, 64, 16), (3, 1, 128, 32)])
def test_pool_default_block_count(L, Hkv, D, BS):
    """CPU budget 1 << 28 bytes; an fp8 block is 2*L*Hkv*BS*(D+4) bytes."""
    pool = PagedKVPool(L, Hkv, D, block_size=BS, device=CPU, kv_quant="fp8")
    assert pool.num_blocks == (1 << 28) // (2 * L * Hkv * BS * (D + 4))
    assert pool.free_blocks() == pool.num_blocks


def test_pool_fork_copies_codes_and_scales():
    pool = _pool(kv_quant="fp8")
    a = pool.new_sequence()
    blocks = list(pool.ensure_capacity(a, 10))              # 3 blocks
    g = torch.Generator().manual_seed(1)
    for c in pool.k + pool.v:
        c.data.copy_(torch.randint(0, 0x7F, c.data.shape, generator=g,
                                   dtype=torch.uint8))
        c.scale.copy_(torch.rand(c.scale.shape, generator=g) + 0.5)
    b = pool.fork(a)
    forked = pool.table(b).blocks
    assert len(forked) == 3 and not set(forked) & set(blocks)
    assert pool.table(b).length == 10 and pool.free_blocks() == 2
    for c in pool.k + pool.v:
        assert torch.equal(c.data[forked], c.data[blocks])
        assert torch.equal(c.scale[forked], c.scale[blocks])


def test_pool_truncate_and_release_unchanged():
    pool = _pool(kv_quant="fp8")
    sid = pool.new_sequence()
    blocks = list(pool.ensure_capacity(sid, 10))
    assert len(blocks) == 3 and pool.free_blocks() == 5
    free = list(pool._free)
    pool.ensure_capacity(sid, 19)
    pool.truncate(sid, 10)
    assert pool._free == free and pool.table(sid).blocks == blocks
    assert pool.truncate(sid, 4) == blocks[:1] and pool.free_blocks() == 7
    with pytest.raises(ValueError):
        pool.truncate(sid, 9)
    pool.release(sid)
    assert pool.free_blocks() == 8


@pytest.mark.parametrize("bad", ["int8", "bf16", "FP8", ""])
def test_pool_bad_kv_quant(bad):
    with pytest.raises(ValueError, match="kv_quant"):
        _pool(kv_quant=bad)


# -- PagedSessionManager inheritance -------------------------------------------------

@pytest.fixture(scope="module")
def engine8():
    return LocalEngine.create("llama3-tiny", device=CPU, kv_quant="fp8")


@pytest.fixture(scope="module")
def plain_engine():
    return LocalEngine.create("llama3-tiny", device=CPU)


def test_manager_inherits_fp8(engine8):
    mgr = PagedSessionManager(engine8, num_blocks=8)
    assert mgr.pool.kv_dtype == "fp8"
    assert all(isinstance(c, ops.QuantKV) for c in mgr.pool.k + mgr.pool.v)


def test_manager_explicit_kv_quant_overrides(engine8, plain_engine):
    mgr = PagedSessionManager(plain_engine, num_blocks=8, kv_quant="fp8")
    assert mgr.pool.kv_dtype == "fp8" and isinstance(mgr.pool.k[0], ops.QuantKV)
    mgr = PagedSessionManager(engine8, num_blocks=8, kv_quant="none")
    assert mgr.pool.kv_dtype == "fp32"
    assert isinstance(mgr.pool.k[0], torch.Tensor)
    with pytest.raises(ValueError, match="kv_quant"):
        PagedSessionManager(plain_engine, num_blocks=8, kv_quant="int4")


def test_plain_engine_keeps_a_tensor_pool(plain_engine):
    mgr = PagedSessionManager(plain_engine, num_blocks=8)
    assert mgr.pool.kv_quant is None and mgr.pool.kv_dtype == "fp32"
    assert all(isinstance(c, torch.Tensor) for c in mgr.pool.k + mgr.pool.v)


# -- sessions on an fp8 pool -----------------------------------------------------------

P1 = "def add(a, b):\n    return"
P2 = [(53 * i + 7) % 500 for i in range(70)]      # crosses the 64-key tile
IDS2 = [7, 300, 41, 12, 255, 9]
IDS3 = [(37 * i + 11) % 500 for i in range(23)]   # crosses block edges


def solo(engine, ctx, n):
    return engine.generate(list(ctx), max_new_tokens=n,
                           stop_on_eos=False)["token_ids"]


def check_turn(engine, mgr, sid, ctx, n):
    """The session's current turn equals the solo run over ctx up to the
    turn's own stop, and it stopped for a reason: EOS or the budget."""
    res = mgr.result(sid)
    got = res["token_ids"]
    assert res["done"] and got
    assert got == solo(engine, ctx, n)[:len(got)]
    assert got[-1] == mgr.eos or len(got) == n
    return got


def test_open_rows_equal_the_solo_cache(engine8):
    """After open() the session's gathered codes and scales are the solo
    engine's cache rows, bit for bit, in every layer."""
    mgr = PagedSessionManager(engine8, block_size=16, num_blocks=32)
    for ids in (engine8.tokenizer.encode(P1), P2):
        sid = mgr.open(ids, max_new_tokens=4)
        blocks, S = mgr.pool.table(sid).blocks, len(ids)
        solo(engine8, ids, 1)                   # prefills rows [0, S)
        for li in range(len(mgr.pool.k)):
            for pool, cache in ((mgr.pool.k[li], engine8.k_caches[li]),
                                (mgr.pool.v[li], engine8.v_caches[li])):
                assert torch.equal(kc.gather_blocks(pool.data, blocks, S, 16),
                                   cache.data[0, :, :S]), f"layer {li} codes"
                assert torch.equal(kc.gather_blocks(pool.scale, blocks, S, 16),
                                   cache.scale[0, :, :S]), f"layer {li} scales"


def test_sessions_match_the_solo_fp8_engine(engine8):
    """open -> run -> extend -> run, two sessions of different lengths
    decoding together: every turn equals the solo fp8 engine's tokens over
    the same whole context."""
    p1 = engine8.tokenizer.encode(P1)
    mgr = PagedSessionManager(engine8, block_size=16, num_blocks=64)
    a = mgr.open(P1, max_new_tokens=5)
    b = mgr.open(P2, max_new_tokens=9)
    mgr.run(chunk=3)
    ta = check_turn(engine8, mgr, a, p1, 5)
    tb = check_turn(engine8, mgr, b, P2, 9)
    mgr.extend(a, IDS3, max_new_tokens=7)
    mgr.extend(b, IDS2, max_new_tokens=6)
    mgr.run()
    check_turn(engine8, mgr, a, p1 + ta + IDS3, 7)
    check_turn(engine8, mgr, b, P2 + tb + IDS2, 6)
    assert mgr.result(a)["turn"] == 1 and mgr.result(b)["turn"] == 1
    for sid in (a, b):
        mgr.close(sid)
    assert mgr.pool.free_blocks() == 64


def test_cpu_decode_step_goes_through_the_op(engine8, monkeypatch):
    """On an fp8 pool the CPU branch of _forward_paged never writes pool rows
    itself: the append is ops.attn_decode_paged's k=, v=, table= form."""
    calls = []
    real = ops.attn_decode_paged

    def spy(*a, **kw):
        calls.append(kw.get("table") is not None and kw.get("k") is not None)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "attn_decode_paged", spy)
    mgr = PagedSessionManager(engine8, block_size=16, num_blocks=16)
    mgr.eos = -1
    sid = mgr.open(P1, max_new_tokens=3)
    mgr.step()
    assert calls and all(calls)
    assert len(mgr.sessions[sid].generated) == 2


# -- serve -------------------------------------------------------------------------------

def test_create_app_fp8_sessions():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from fei_amd.serve.api import create_app
    app = create_app(model="llama3-tiny", device=CPU, kv_quant="fp8",
                     session_blocks=16)
    c = TestClient(app)
    assert app.state.engine.kv_dtype == "fp8"
    r = c.post("/v1/sessions", json={"prompt": "abcdefgh" * 3,
                                     "max_tokens": 3})
    assert r.status_code == 200
    mgr = app.state.session_manager()
    assert mgr.pool.kv_dtype == "fp8"
    assert isinstance(mgr.pool.k[0], ops.QuantKV)
    st = c.post("/v1/sessions/step?n=4").json()
    assert st["kv_dtype"] == "fp8"
    assert c.get(f"/v1/sessions/{r.json()['session_id']}").json()["token_ids"]
