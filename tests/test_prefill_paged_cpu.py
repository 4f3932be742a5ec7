"""Paged prefill and multi-turn continuation without a GPU.

Ops: on CPU tensors fei_amd.ops.attn_prefill_paged / rope_kv_prefill_paged
gather the logical rows and run the contiguous fp32 reference, so they must
equal it exactly over scrambled tables whose padding entries are -1.

Contract: a paged session that is opened, run, extended and run again emits
in every turn exactly what LocalEngine.generate emits for the whole context
(prompt + earlier turns + extensions), greedy, on the CPU llama3-tiny."""

import pytest
import torch

from fei_amd import ops
from fei_amd.engine.engine import LocalEngine
from fei_amd.engine.kv_cache import PagedKVPool
from fei_amd.engine.sessions import PagedSessionManager

import paged_prefill_cases as pc


# -- ops -----------------------------------------------------------------------

@pytest.mark.parametrize("BS", pc.BLOCK_SIZES + (1,))
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_attn_prefill_paged_equals_reference(case, BS):
    S, pos0 = case
    for G, D in ((1, 64), (4, 128)):
        pc.run_attn_case(G, D, S, pos0, BS, "cpu")


@pytest.mark.parametrize("BS", pc.BLOCK_SIZES + (1,))
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_rope_kv_prefill_paged_equals_reference(case, BS):
    S, pos0 = case
    for hkv, D in ((4, 64), (1, 128)):
        pc.run_append_case(hkv, D, S, pos0, BS, "cpu")


def _cpu_args(Hq=4, Hkv=2, D=64, BS=16, S=4, width=2, p0=0):
    q = torch.zeros(1, S, Hq, D)
    kv = torch.zeros(1, S, Hkv, D)
    pool = torch.zeros(4, Hkv, BS, D)
    table = torch.zeros(1, width, dtype=torch.int32)
    pos0 = torch.full((1,), p0, dtype=torch.int32)
    return q, kv, pool, table, pos0


@pytest.mark.parametrize("kw", [
    dict(Hq=6, Hkv=4),                 # Hq % Hkv != 0
    dict(BS=12),                       # block size not a power of two
    dict(S=4, width=2, p0=29),         # 2 * 16 rows < 29 + 4
], ids=["gqa", "block_size", "table_too_short"])
def test_value_errors(kw):
    q, kv, pool, table, pos0 = _cpu_args(**kw)
    rope = ops.ref.rope_table(64, q.shape[-1])
    with pytest.raises(ValueError):
        ops.attn_prefill_paged(q, pool, pool.clone(), table, pos0)
    with pytest.raises(ValueError):
        ops.rope_kv_prefill_paged(q, kv, kv.clone(), pool, pool.clone(),
                                  table, pos0, rope)
    assert not bool(pool.any())


def test_table_exactly_long_enough():
    q, kv, pool, table, pos0 = _cpu_args(S=4, width=2, p0=28)   # 32 rows
    table[0, 1] = 3
    out = ops.attn_prefill_paged(q, pool, pool.clone(), table, pos0)
    assert tuple(out.shape) == tuple(q.shape)


# -- PagedKVPool.truncate --------------------------------------------------------

def _pool(n=8, bs=4):
    return PagedKVPool(num_layers=1, num_kv_heads=1, head_dim=8, block_size=bs,
                       num_blocks=n, device=torch.device("cpu"),
                       dtype=torch.float32)


def test_truncate():
    pool = _pool()
    sid = pool.new_sequence()
    blocks = list(pool.ensure_capacity(sid, 10))            # 3 blocks
    assert len(blocks) == 3 and pool.free_blocks() == 5
    assert pool.truncate(sid, 5) == blocks[:2]
    assert pool.table(sid).length == 5 and pool.free_blocks() == 6
    assert pool.truncate(sid, 5) == blocks[:2]              # idempotent
    assert pool.truncate(sid, 4) == blocks[:1]              # exactly one block
    assert pool.truncate(sid, 0) == [] and pool.free_blocks() == 8
    assert pool.table(sid).length == 0
    with pytest.raises(ValueError):
        pool.truncate(sid, 1)                               # cannot grow
    with pytest.raises(ValueError):
        pool.truncate(sid, -1)
    with pytest.raises(KeyError):
        pool.truncate(99, 0)


def test_truncate_undoes_a_growth_exactly():
    pool = _pool()
    a = pool.new_sequence()
    pool.ensure_capacity(a, 6)
    free, blocks = list(pool._free), list(pool.table(a).blocks)
    pool.ensure_capacity(a, 19)                             # + 3 blocks
    pool.truncate(a, 6)
    assert pool._free == free and pool.table(a).blocks == blocks
    assert pool.table(a).length == 6
    b = pool.new_sequence()                 # the next taker gets the same block
    assert pool.ensure_capacity(b, 1) == [free[-1]]


# -- the multi-turn contract -----------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    return LocalEngine.create("llama3-tiny")


P1 = "def add(a, b):\n    return"
P2 = "The quick brown fox"
P3 = "x = [1, 2,"
IDS2 = [7, 300, 41, 12, 255, 9]
IDS3 = [100, 101, 5]


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


def _stop_token(tokens, lo, hi):
    """(index, token) of a token inside tokens[lo:hi] that does not occur
    before its index: setting mgr.eos to it stops the turn exactly there."""
    for j in range(lo, hi):
        if tokens[j] not in tokens[:j]:
            return j, tokens[j]
    raise AssertionError("no usable stop token; change the prompt")


def test_extend_after_eos_inside_a_chunk(engine):
    """Turn 1 ends at an EOS in the middle of a step_chunk(8): the chunk's
    remaining steps left garbage rows past pos, which the extension
    overwrites. Then a third turn."""
    p1 = engine.tokenizer.encode(P1)
    t1 = solo(engine, p1, 12)
    j, eos = _stop_token(t1, 2, 6)
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    mgr.eos = eos
    sid = mgr.open(P1, max_new_tokens=12)
    mgr.step_chunk(8)
    s = mgr.sessions[sid]
    assert s.done and mgr.result(sid)["token_ids"] == t1[:j + 1]
    assert s.pos == len(p1) + j and mgr.result(sid)["turn"] == 0
    # the pool really holds rows past pos (written by the rest of the chunk)
    assert mgr.pool.table(sid).length >= len(p1) + 8

    first = mgr.extend(sid, IDS2, max_new_tokens=7)
    ctx2 = p1 + t1[:j + 1] + IDS2
    assert s.context_ids == ctx2 and s.turn == 1
    assert s.pos == len(ctx2) and s.generated == [first]
    mgr.run()
    t2 = check_turn(engine, mgr, sid, ctx2, 7)
    assert t2[0] == first and mgr.result(sid)["turn"] == 1

    first3 = mgr.extend(sid, IDS3, max_new_tokens=5)
    ctx3 = ctx2 + t2 + IDS3
    assert s.context_ids == ctx3 and s.turn == 2
    mgr.run()
    t3 = check_turn(engine, mgr, sid, ctx3, 5)
    assert t3[0] == first3
    mgr.close(sid)
    assert mgr.pool.free_blocks() == 64


def test_extend_after_budget_stop(engine):
    p1 = engine.tokenizer.encode(P2)
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    sid = mgr.open(P2, max_new_tokens=5)
    mgr.run()
    t1 = check_turn(engine, mgr, sid, p1, 5)
    if mgr.eos not in t1:
        assert len(t1) == 5
    mgr.extend(sid, IDS2, max_new_tokens=6)
    mgr.run()
    check_turn(engine, mgr, sid, p1 + t1 + IDS2, 6)


def test_extend_with_a_string_prompt(engine):
    p1 = engine.tokenizer.encode(P3)
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    sid = mgr.open(P3, max_new_tokens=4)
    mgr.run()
    t1 = mgr.result(sid)["token_ids"]
    text = "\ntool: 42\n"
    mgr.extend(sid, text, max_new_tokens=4)
    mgr.run()
    check_turn(engine, mgr, sid, p1 + t1 + engine.tokenizer.encode(text), 4)


def test_extension_crosses_block_boundaries(engine):
    """pos = 13 after turn 1 (block size 16): a 40-token extension runs over
    the block edges at 16, 32 and 48, in blocks reserved by the extend."""
    p1 = list(range(20, 30))
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    sid = mgr.open(p1, max_new_tokens=4)
    mgr.run(chunk=3)
    t1 = check_turn(engine, mgr, sid, p1, 4)
    if len(t1) == 4:
        assert mgr.sessions[sid].pos == 13
    held = len(mgr.pool.table(sid).blocks)
    ext = [(37 * i + 11) % 500 for i in range(40)]
    mgr.extend(sid, ext, max_new_tokens=6)
    assert len(mgr.pool.table(sid).blocks) > held
    mgr.run()
    check_turn(engine, mgr, sid, p1 + t1 + ext, 6)


def test_extends_interleaved_with_decoding(engine):
    """Two sessions extended at different times while a third keeps
    decoding: each still matches its solo run."""
    ids = {p: engine.tokenizer.encode(p) for p in (P1, P2, P3)}
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    a = mgr.open(P1, max_new_tokens=3)
    b = mgr.open(P2, max_new_tokens=4)
    c = mgr.open(P3, max_new_tokens=30)
    while not (mgr.sessions[a].done and mgr.sessions[b].done):
        mgr.step_chunk(2)
    ta = check_turn(engine, mgr, a, ids[P1], 3)
    tb = check_turn(engine, mgr, b, ids[P2], 4)
    assert not mgr.sessions[c].done or mgr.eos in mgr.sessions[c].generated
    mgr.extend(a, IDS2, max_new_tokens=9)
    mgr.step_chunk(3)
    mgr.extend(b, IDS3, max_new_tokens=6)
    mgr.run(chunk=4)
    check_turn(engine, mgr, a, ids[P1] + ta + IDS2, 9)
    check_turn(engine, mgr, b, ids[P2] + tb + IDS3, 6)
    check_turn(engine, mgr, c, ids[P3], 30)
    for sid in (a, b, c):
        mgr.close(sid)
    assert mgr.pool.free_blocks() == 64


# -- open() regression -------------------------------------------------------------

def test_open_longer_than_a_key_tile(engine):
    ids = [(53 * i + 7) % 500 for i in range(150)]          # three 64-key tiles
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    sid = mgr.open(ids, max_new_tokens=6)
    mgr.run()
    check_turn(engine, mgr, sid, ids, 6)


def test_open_and_extend_in_prefill_chunks(engine, monkeypatch):
    monkeypatch.setattr(LocalEngine, "PREFILL_CHUNK", 16)
    ids = [(29 * i + 3) % 500 for i in range(53)]           # 16+16+16+5
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    sid = mgr.open(ids, max_new_tokens=5)
    mgr.run()
    t1 = check_turn(engine, mgr, sid, ids, 5)
    ext = [(31 * i + 1) % 500 for i in range(37)]           # 1+37 = 16+16+6
    mgr.extend(sid, ext, max_new_tokens=5)
    mgr.run()
    check_turn(engine, mgr, sid, ids + t1 + ext, 5)


# -- errors --------------------------------------------------------------------------

def test_extend_errors(engine):
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    with pytest.raises(KeyError):
        mgr.extend(12345, IDS2)
    mgr.eos = -1                                  # nothing ends this turn early
    sid = mgr.open(list(range(40, 52)), max_new_tokens=40)
    with pytest.raises(ValueError, match="active"):
        mgr.extend(sid, IDS2)
    mgr.close(sid)
    mgr.eos = engine.tokenizer.eos_id
    sid = mgr.open(list(range(40, 52)), max_new_tokens=3)
    mgr.run()
    s = mgr.sessions[sid]
    snap = (s.pos, list(s.generated), s.turn, list(s.context_ids),
            list(mgr.pool.table(sid).blocks), mgr.pool.free_blocks())
    limit = engine.model.max_seq_len
    with pytest.raises(ValueError, match="max_seq_len"):
        mgr.extend(sid, IDS2, max_new_tokens=limit)
    with pytest.raises(ValueError, match="max_seq_len"):
        mgr.extend(sid, IDS2,
                   max_new_tokens=limit - s.pos - 1 - len(IDS2) + 1)
    assert snap == (s.pos, list(s.generated), s.turn, list(s.context_ids),
                    list(mgr.pool.table(sid).blocks), mgr.pool.free_blocks())
    # the largest budget that fits: pos + 1 + new + budget == max_seq_len
    mgr.extend(sid, IDS2, max_new_tokens=limit - s.pos - 1 - len(IDS2))


def test_extend_pool_exhaustion_leaves_the_session_as_it_was(engine):
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=5)
    a = mgr.open(list(range(60, 80)), max_new_tokens=3)      # 20 rows
    b = mgr.open(list(range(90, 100)), max_new_tokens=3)     # 10 rows
    mgr.run()
    sa = mgr.sessions[a]
    assert sa.done and mgr.sessions[b].done
    assert mgr.pool.free_blocks() == 1            # a partial growth is undone
    t = mgr.pool.table(a)
    snap = (sa.pos, list(sa.generated), sa.done, sa.turn,
            list(sa.context_ids), sa.max_new_tokens, list(t.blocks), t.length,
            list(mgr.pool._free))
    res = mgr.result(a)
    ext = [(41 * i + 2) % 500 for i in range(30)]  # needs 2 more blocks
    with pytest.raises(MemoryError):
        mgr.extend(a, ext, max_new_tokens=4)
    assert snap == (sa.pos, list(sa.generated), sa.done, sa.turn,
                    list(sa.context_ids), sa.max_new_tokens, list(t.blocks),
                    t.length, list(mgr.pool._free))
    assert mgr.result(a) == res
    mgr.close(b)                                   # evict -> the same extend fits
    ctx = list(range(60, 80)) + res["token_ids"] + ext
    mgr.extend(a, ext, max_new_tokens=4)
    mgr.run()
    check_turn(engine, mgr, a, ctx, 4)


# -- HTTP -----------------------------------------------------------------------------

def _client(engine, blocks):
    from fastapi.testclient import TestClient
    from fei_amd.serve.api import create_app
    return TestClient(create_app(engine=engine, session_blocks=blocks))


def _finish(c, sid):
    for _ in range(64):
        if c.get(f"/v1/sessions/{sid}").json()["done"]:
            return
        c.post("/v1/sessions/step?n=4")
    raise AssertionError("session did not finish")


def test_http_extend(engine):
    c = _client(engine, 64)
    sid = c.post("/v1/sessions", json={"prompt": "abc abc",
                                       "max_tokens": 4}).json()["session_id"]
    # still decoding: 409 (unless the very first token was EOS)
    if not c.get(f"/v1/sessions/{sid}").json()["done"]:
        r = c.post(f"/v1/sessions/{sid}/extend", json={"prompt": "more"})
        assert r.status_code == 409
    _finish(c, sid)
    turn1 = c.get(f"/v1/sessions/{sid}").json()
    assert turn1["turn"] == 0
    assert c.post("/v1/sessions/9999/extend",
                  json={"prompt": "x"}).status_code == 404
    r = c.post(f"/v1/sessions/{sid}/extend",
               json={"prompt": "x", "max_tokens": 100000})
    assert r.status_code == 400
    r = c.post(f"/v1/sessions/{sid}/extend",
               json={"prompt": " and then", "max_tokens": 5})
    assert r.status_code == 200
    body = r.json()
    assert body["session_id"] == sid
    _finish(c, sid)
    turn2 = c.get(f"/v1/sessions/{sid}").json()
    assert turn2["turn"] == 1 and turn2["token_ids"][0] == body["first_token"]
    ctx = (engine.tokenizer.encode("abc abc") + turn1["token_ids"]
           + engine.tokenizer.encode(" and then"))
    got = turn2["token_ids"]
    assert got == solo(engine, ctx, 5)[:len(got)]
    c.delete(f"/v1/sessions/{sid}")


def test_http_extend_503_on_pool_exhaustion(engine):
    c = _client(engine, 3)
    n1 = len(engine.tokenizer.encode("abcdefgh" * 3))
    big = "ijklmnop" * 6
    # 3 blocks = 48 rows: turn 1 and a short extension fit, the big one
    # (pos + 1 + new + 1 rows, pos = n1 + 1) does not
    assert n1 + 8 <= 48 < n1 + 3 + len(engine.tokenizer.encode(big)), \
        "prompt sizes no longer straddle the 3-block pool"
    sid = c.post("/v1/sessions", json={"prompt": "abcdefgh" * 3,
                                       "max_tokens": 2}).json()["session_id"]
    for _ in range(8):
        if c.get(f"/v1/sessions/{sid}").json()["done"]:
            break
        c.post("/v1/sessions/step?n=1")
    before = c.get(f"/v1/sessions/{sid}").json()
    assert before["done"]
    r = c.post(f"/v1/sessions/{sid}/extend",
               json={"prompt": big, "max_tokens": 2})
    assert r.status_code == 503
    assert c.get(f"/v1/sessions/{sid}").json() == before
    r = c.post(f"/v1/sessions/{sid}/extend",
               json={"prompt": "ok", "max_tokens": 2})
    assert r.status_code == 200
