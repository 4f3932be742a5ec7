"""Ragged paged prefill and batched session admission without a GPU.

Ops: on CPU tensors ops.attn_prefill_paged_ragged /
rope_kv_prefill_paged_ragged run the uniform paged ops' fp32 reference
sequence by sequence, so per sequence they must equal those ops exactly,
over scrambled tables whose padding entries are -1.

Contract: every session admitted by open_many / extend_many emits, turn
after turn, exactly what LocalEngine.generate emits for its whole context
(greedy, CPU llama3-tiny), and a batch that does not fit changes nothing."""

import copy

import pytest
import torch

from fei_amd import ops
from fei_amd.engine.engine import LocalEngine
from fei_amd.engine.sessions import PagedSessionManager

import ragged_prefill_cases as rc

CPU = torch.device("cpu")


# -- ops -----------------------------------------------------------------------

@pytest.mark.parametrize("BS", rc.BLOCK_SIZES + (1,))
@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_attn_prefill_paged_ragged_equals_uniform(case, BS):
    lens, pos0 = case
    for G, D in ((1, 64), (4, 128)):
        rc.run_attn_case(G, D, lens, pos0, BS, "cpu")


@pytest.mark.parametrize("BS", rc.BLOCK_SIZES + (1,))
@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_rope_kv_prefill_paged_ragged_equals_uniform(case, BS):
    lens, pos0 = case
    for hkv, D in ((4, 64), (1, 128)):
        rc.run_append_case(hkv, D, lens, pos0, BS, "cpu")


def test_ragged_batch_layout():
    lens, pos0 = rc.CASES[0]                                # (1, 65, 17)
    table = torch.zeros(3, 8, dtype=torch.int32)
    b = ops.RaggedBatch(list(lens), list(pos0), table, "cpu", block_size=16)
    assert (b.B, b.T, b.n_tiles, b.max_blocks) == (3, 83, 4, 8)
    assert b.cu_seqlens.dtype == torch.int32
    assert b.cu_seqlens.tolist() == [0, 1, 66, 83]
    assert b.tile_map.dtype == torch.int32
    assert b.tile_map.tolist() == [[0, 0], [1, 0], [1, 1], [2, 0]]
    assert b.tok_seq.tolist() == [0] + [1] * 65 + [2] * 17
    assert b.pos0.tolist() == list(pos0)
    assert b.last_index.tolist() == [0, 65, 82]
    assert b.block_table.dtype == torch.int32
    assert tuple(b.block_table.shape) == (3, 8)


def _table(B=2, W=4, dtype=torch.int32):
    return torch.zeros(B, W, dtype=dtype)


@pytest.mark.parametrize("args", [
    ([4, 0], [0, 0], _table()),                    # a length below 1
    ([4, -2], [0, 0], _table()),
    ([], [], _table(0)),                           # nothing to do
    ([4, 4], [0], _table()),                       # mismatched lists
    ([4, 4], [0, 0], _table(dtype=torch.int64)),   # not int32
    ([4, 4], [0, 0], _table(3)),                   # not [B, W]
    ([4, 4], [0, 0], torch.zeros(8, dtype=torch.int32)),
    ([4, 4], [0, 0], [[0, 1], [2, 3]]),            # not a tensor
], ids=["len0", "len_neg", "empty", "mismatch", "int64", "rows", "1d",
        "list"])
def test_ragged_batch_value_errors(args):
    with pytest.raises(ValueError):
        ops.RaggedBatch(*args, "cpu")


def test_ragged_batch_table_too_narrow():
    # sequence 1 reaches row 61 + 4 = 65: five 16-row blocks, the table has 4
    with pytest.raises(ValueError, match="needs 5"):
        ops.RaggedBatch([4, 4], [0, 61], _table(), "cpu", block_size=16)
    ops.RaggedBatch([4, 4], [0, 60], _table(), "cpu", block_size=16)
    # without a block size the ops check it against their pool
    batch = ops.RaggedBatch([4, 4], [0, 61], _table(), "cpu")
    q = torch.zeros(8, 4, 64)
    kv = torch.zeros(8, 2, 64)
    pool = torch.zeros(6, 2, 16, 64)
    rope = ops.ref.rope_table(128, 64)
    with pytest.raises(ValueError, match="needs 5"):
        ops.attn_prefill_paged_ragged(q, pool, pool.clone(), batch)
    with pytest.raises(ValueError, match="needs 5"):
        ops.rope_kv_prefill_paged_ragged(q, kv, kv.clone(), pool,
                                         pool.clone(), batch, rope)
    assert not bool(pool.any())


@pytest.mark.parametrize("kw", [dict(Hq=6, Hkv=4), dict(BS=12), dict(BS=48)],
                         ids=["gqa", "bs12", "bs48"])
def test_op_value_errors(kw):
    BS = kw.pop("BS", 16)
    q, kv, pool, table = rc.tiny_args(64, BS, "cpu", torch.float32, **kw)
    rope = ops.ref.rope_table(64, 64)
    batch = ops.RaggedBatch([4], [0], table, "cpu")
    with pytest.raises(ValueError):
        ops.attn_prefill_paged_ragged(q, pool, pool.clone(), batch)
    with pytest.raises(ValueError):
        ops.rope_kv_prefill_paged_ragged(q, kv, kv.clone(), pool,
                                         pool.clone(), batch, rope)
    with pytest.raises(ValueError):                 # q is not [T, Hq, D]
        ops.attn_prefill_paged_ragged(q[:3], pool, pool.clone(), batch)
    assert not bool(pool.any())


def test_fp8_pool_on_the_cpu_path():
    """An fp8 pool is accepted on the CPU path: per sequence it is the
    uniform fp8 reference."""
    lens, pos0, BS, hkv, D = (5, 19, 2), (3, 0, 30), 16, 2, 64
    g = torch.Generator().manual_seed(5)
    T = sum(lens)
    q = torch.randn(T, 4, D, generator=g)
    k = torch.randn(T, hkv, D, generator=g)
    v = torch.randn(T, hkv, D, generator=g)
    rope = ops.ref.rope_table(64, D)
    table = torch.tensor([[4, -1], [1, 6], [0, 3]], dtype=torch.int32)
    shape = (7, hkv, BS, D)
    pools = [ops.QuantKV.zeros(shape, "cpu") for _ in range(4)]
    # sequences 0 and 2 continue: give them earlier rows, in both pool pairs
    for b, n in ((0, 3), (2, 30)):
        kk = torch.randn(1, n, hkv, D, generator=g)
        p0 = torch.zeros(1, dtype=torch.int32)
        for kp, vp in (pools[:2], pools[2:]):
            ops.rope_kv_prefill_paged(torch.zeros(1, n, 4, D), kk, kk.clone(),
                                      kp, vp, table[b:b + 1], p0, rope)
    batch = ops.RaggedBatch(list(lens), list(pos0), table, "cpu",
                            block_size=BS)
    q1, q2 = q.clone(), q.clone()
    ops.rope_kv_prefill_paged_ragged(q1, k, v, pools[0], pools[1], batch,
                                     rope)
    out = ops.attn_prefill_paged_ragged(q1, pools[0], pools[1], batch)
    cu = rc.cu_of(lens)
    for b in range(3):
        r = slice(cu[b], cu[b + 1])
        p0 = torch.tensor([pos0[b]], dtype=torch.int32)
        ops.rope_kv_prefill_paged(q2[r][None], k[r][None], v[r][None],
                                  pools[2], pools[3], table[b:b + 1], p0,
                                  rope)
        want = ops.attn_prefill_paged(q2[r][None], pools[2], pools[3],
                                      table[b:b + 1], p0)
        assert torch.equal(out[r], want[0]), f"sequence {b}"
    assert torch.equal(q1, q2)
    for a, b_ in ((pools[0], pools[2]), (pools[1], pools[3])):
        assert torch.equal(a.data, b_.data) and torch.equal(a.scale, b_.scale)


# -- the model --------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    return LocalEngine.create("llama3-tiny", device=CPU)


def test_forward_ragged_equals_forward_paged_per_sequence(engine):
    """fp32 reference: the packed forward's logits and pool rows are those
    of forward_prefill_paged on each sequence alone (row-wise GEMMs)."""
    m = engine.model
    BS, lens, pos0 = 16, (21, 3, 40), (0, 0, 0)
    table = torch.tensor([[3, 9, -1], [12, -1, -1], [6, 0, 14]],
                         dtype=torch.int32)
    shape = (16, m.hkv_l, BS, m.D)
    mk = lambda: [torch.zeros(shape) for _ in m.layers]
    kp1, vp1, kp2, vp2 = mk(), mk(), mk(), mk()
    g = torch.Generator().manual_seed(3)
    ids = [torch.randint(0, m.spec.vocab_size, (n,), generator=g)
           for n in lens]
    batch = ops.RaggedBatch(list(lens), list(pos0), table, "cpu",
                            block_size=BS)
    got = m.forward_prefill_paged_ragged(torch.cat(ids), batch, kp1, vp1)
    assert tuple(got.shape) == (3, m.spec.vocab_size)
    for b in range(3):
        p0 = torch.tensor([pos0[b]], dtype=torch.int32)
        want = m.forward_prefill_paged(ids[b][None], p0, kp2, vp2,
                                       table[b:b + 1])
        torch.testing.assert_close(got[b], want[0], rtol=1e-4, atol=1e-5)
        assert int(got[b].argmax()) == int(want[0].argmax())
    for a, b_ in zip(kp1 + vp1, kp2 + vp2):
        torch.testing.assert_close(a, b_, rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError):
        m.forward_prefill_paged_ragged(torch.cat(ids)[None], batch, kp1, vp1)


# -- the admission contract ------------------------------------------------------

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


def _ids(n, a, c):
    return [(a * i + c) % 500 for i in range(n)]


PROMPTS = [_ids(5, 37, 11), _ids(150, 53, 7), _ids(23, 29, 3), [9]]
EXTS = [_ids(40, 41, 2), [100, 101, 5], [], _ids(70, 31, 1)]


def snapshot(mgr):
    """Everything an admission may not touch when it fails."""
    return copy.deepcopy((
        {sid: vars(s) for sid, s in mgr.sessions.items()},
        {sid: (t.blocks, t.length) for sid, t in mgr.pool._tables.items()},
        mgr.pool._free))


def _two_turns(engine, mgr, n1=5, n2=6, **kw):
    """open_many(PROMPTS) -> run -> extend_many(EXTS) -> run, every turn
    checked against the solo run over the whole context."""
    sids = mgr.open_many(PROMPTS, max_new_tokens=n1, **kw)
    assert len(sids) == len(PROMPTS) == len(set(sids))
    for sid, p in zip(sids, PROMPTS):
        s = mgr.sessions[sid]
        assert (s.pos, s.turn, s.prompt_ids) == (len(p), 0, p)
    mgr.run()
    ctxs = []
    for sid, p in zip(sids, PROMPTS):
        ctxs.append(p + check_turn(engine, mgr, sid, p, n1))
    firsts = mgr.extend_many(list(zip(sids, EXTS)), max_new_tokens=n2, **kw)
    for i, (sid, ext) in enumerate(zip(sids, EXTS)):
        s = mgr.sessions[sid]
        ctxs[i] = ctxs[i] + ext
        assert s.context_ids == ctxs[i] and s.pos == len(ctxs[i])
        assert s.turn == 1 and s.generated == [firsts[i]]
    mgr.run()
    for i, sid in enumerate(sids):
        t2 = check_turn(engine, mgr, sid, ctxs[i], n2)
        assert t2[0] == firsts[i]
    for sid in sids:
        mgr.close(sid)
    assert mgr.pool.free_blocks() == mgr.pool.num_blocks


def test_open_many_extend_many_token_identity(engine):
    """Unequal lengths, one prompt longer than two key tiles, a one-token
    prompt, an empty extension."""
    _two_turns(engine, PagedSessionManager(engine, block_size=16,
                                           num_blocks=96))


def test_pieces_span_several_forwards(engine, monkeypatch):
    """PREFILL_CHUNK = 16: the 150-token prompt is ten pieces in ten
    forwards, next to the others' first pieces."""
    monkeypatch.setattr(LocalEngine, "PREFILL_CHUNK", 16)
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=96)
    seen = []
    fwd = mgr.model.forward_prefill_paged_ragged

    def spy(tokens, batch, k, v):
        seen.append((list(batch.seq_lens), list(batch.pos0_host)))
        return fwd(tokens, batch, k, v)

    monkeypatch.setattr(mgr.model, "forward_prefill_paged_ragged", spy)
    sids = mgr.open_many(PROMPTS, max_new_tokens=4, max_batch_tokens=40)
    # forward 0: 5 + 16 + 16 fit in 40, then the one-token prompt (38);
    # forward 1: the second pieces of the two long prompts (16 + 7)
    assert seen[0] == ([5, 16, 16, 1], [0, 0, 0, 0])
    assert seen[1] == ([16, 7], [16, 16])
    assert seen[2:] == [([n], [p]) for n, p in
                        zip([16] * 7 + [6], range(32, 150, 16))]
    mgr.run()
    for sid, p in zip(sids, PROMPTS):
        check_turn(engine, mgr, sid, p, 4)
    monkeypatch.undo()
    monkeypatch.setattr(LocalEngine, "PREFILL_CHUNK", 16)
    _two_turns(engine, PagedSessionManager(engine, block_size=16,
                                           num_blocks=96))


@pytest.mark.parametrize("budget", [1, 30, 64])
def test_max_batch_tokens_smaller_than_the_total(engine, budget):
    _two_turns(engine, PagedSessionManager(engine, block_size=16,
                                           num_blocks=96),
               max_batch_tokens=budget)


def test_fp8_pool(engine):
    engine8 = LocalEngine.create("llama3-tiny", device=CPU, kv_quant="fp8")
    mgr = PagedSessionManager(engine8, block_size=16, num_blocks=96)
    assert mgr.pool.kv_quant == "fp8"
    _two_turns(engine8, mgr)


def test_extend_many_interleaved_with_decoding(engine):
    """Two sessions extended together while a third keeps decoding."""
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=96)
    a, b, c = mgr.open_many(PROMPTS[:3], max_new_tokens=30)
    mgr.sessions[a].max_new_tokens = 3
    mgr.sessions[b].max_new_tokens = 4
    while not (mgr.sessions[a].done and mgr.sessions[b].done):
        mgr.step_chunk(2)
    ta = check_turn(engine, mgr, a, PROMPTS[0], 3)
    tb = check_turn(engine, mgr, b, PROMPTS[1], 4)
    mgr.extend_many([(b, EXTS[1]), (a, EXTS[0])], max_new_tokens=7)
    mgr.run(chunk=3)
    check_turn(engine, mgr, a, PROMPTS[0] + ta + EXTS[0], 7)
    check_turn(engine, mgr, b, PROMPTS[1] + tb + EXTS[1], 7)
    check_turn(engine, mgr, c, PROMPTS[2], 30)


def test_open_many_of_one_prompt_equals_open(engine):
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    p = PROMPTS[2]
    a = mgr.open(p, max_new_tokens=6)
    (b,) = mgr.open_many([p], max_new_tokens=6)
    sa, sb = vars(mgr.sessions[a]).copy(), vars(mgr.sessions[b]).copy()
    assert sa.pop("sid") == a and sb.pop("sid") == b and sa == sb
    ta, tb = mgr.pool.table(a), mgr.pool.table(b)
    assert len(ta.blocks) == len(tb.blocks) and ta.length == tb.length
    for li in range(len(mgr.pool.k)):
        for pool in (mgr.pool.k[li], mgr.pool.v[li]):
            assert torch.equal(pool[ta.blocks], pool[tb.blocks])
    assert mgr.open_many([]) == [] and mgr.extend_many([]) == []
    assert mgr.open_many(["abc abc"])[0] in mgr.sessions    # a string prompt


# -- all or nothing ----------------------------------------------------------------

def test_open_many_pool_exhaustion_changes_nothing(engine):
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=8)
    keep = mgr.open(_ids(20, 7, 1), max_new_tokens=3)        # 2 blocks
    snap = snapshot(mgr)
    # 2 + 3 blocks fit in the 6 free ones, the third prompt's 2 do not: the
    # pool runs out in the middle of the batch, after a partial growth
    batch = [_ids(30, 3, 2), _ids(40, 5, 4), _ids(31, 11, 6)]
    with pytest.raises(MemoryError):
        mgr.open_many(batch, max_new_tokens=3)
    assert snapshot(mgr) == snap
    mgr.close(keep)
    sids = mgr.open_many(batch, max_new_tokens=2)            # now it fits
    mgr.run(chunk=1)                     # one more row each: still 7 blocks
    for sid, p in zip(sids, batch):
        check_turn(engine, mgr, sid, p, 2)


def test_extend_many_pool_exhaustion_changes_nothing(engine):
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=7)
    a, b, c = mgr.open_many([_ids(20, 7, 1), _ids(10, 3, 5), _ids(12, 9, 2)],
                            max_new_tokens=3)
    mgr.run(chunk=1)                     # no block is reserved ahead of need
    assert mgr.pool.free_blocks() == 3
    snap = snapshot(mgr)
    res = {sid: mgr.result(sid) for sid in (a, b, c)}
    # a grows by 2 blocks, b needs 2 more: one is left
    exts = [(a, _ids(30, 41, 2)), (b, _ids(30, 43, 3))]
    with pytest.raises(MemoryError):
        mgr.extend_many(exts, max_new_tokens=4)
    assert snapshot(mgr) == snap
    assert {sid: mgr.result(sid) for sid in (a, b, c)} == res
    mgr.close(c)                                   # evict -> the same call fits
    mgr.extend_many(exts, max_new_tokens=4)
    mgr.run(chunk=1)
    for sid, ext in exts:
        ctx = mgr.sessions[sid].prompt_ids + res[sid]["token_ids"] + ext
        check_turn(engine, mgr, sid, ctx, 4)


def test_extend_many_errors_change_nothing(engine):
    mgr = PagedSessionManager(engine, block_size=16, num_blocks=64)
    a, b = mgr.open_many([_ids(12, 7, 40), _ids(9, 5, 60)], max_new_tokens=3)
    mgr.run()
    mgr.eos = -1                                   # nothing ends this turn early
    live = mgr.open(_ids(12, 3, 80), max_new_tokens=40)
    assert not mgr.sessions[live].done
    snap = snapshot(mgr)
    ok = (a, [1, 2, 3])
    limit = engine.model.max_seq_len
    with pytest.raises(KeyError):
        mgr.extend_many([ok, (12345, [4])])
    with pytest.raises(ValueError, match="active"):
        mgr.extend_many([ok, (live, [4])])
    with pytest.raises(ValueError, match="twice"):
        mgr.extend_many([ok, (b, [4]), (a, [5])])
    with pytest.raises(ValueError, match="max_seq_len"):
        mgr.extend_many([ok, (b, [4])], max_new_tokens=limit)
    with pytest.raises(ValueError, match="empty"):
        mgr.open_many([[1, 2], []])
    assert snapshot(mgr) == snap
    mgr.extend_many([ok, (b, [4])], max_new_tokens=3)
    assert mgr.sessions[a].turn == 1 and mgr.sessions[b].turn == 1


# -- HTTP -----------------------------------------------------------------------------

def _client(engine, blocks):
    from fastapi.testclient import TestClient
    from fei_amd.serve.api import create_app
    return TestClient(create_app(engine=engine, session_blocks=blocks))


def test_http_batch_round_trip(engine):
    c = _client(engine, 64)
    prompts = ["abc abc", "def main():\n    return", "x"]
    r = c.post("/v1/sessions/batch", json={"prompts": prompts,
                                           "max_tokens": 4})
    assert r.status_code == 200
    sids = r.json()["session_ids"]
    assert len(sids) == 3 and len(set(sids)) == 3
    for _ in range(8):
        c.post("/v1/sessions/step?n=4")
    for sid, p in zip(sids, prompts):
        body = c.get(f"/v1/sessions/{sid}").json()
        assert body["done"] and body["turn"] == 0
        got = body["token_ids"]
        assert got == solo(engine, engine.tokenizer.encode(p), 4)[:len(got)]
        c.delete(f"/v1/sessions/{sid}")
    assert c.post("/v1/sessions/step").json()["free_blocks"] == 64


def test_http_batch_errors(engine):
    c = _client(engine, 3)
    assert c.post("/v1/sessions/batch",
                  json={"prompts": []}).status_code == 400
    assert c.post("/v1/sessions/batch", json={}).status_code == 422
    # 3 blocks = 48 rows: the first prompt fits, both together do not
    small, big = "abcdefgh" * 2, "ijklmnop" * 5
    n1 = len(engine.tokenizer.encode(small))
    n2 = len(engine.tokenizer.encode(big))
    assert -(-(n1 + 1) // 16) <= 3 < -(-(n1 + 1) // 16) + -(-(n2 + 1) // 16), \
        "prompt sizes no longer straddle the 3-block pool"
    r = c.post("/v1/sessions/batch", json={"prompts": [small, big]})
    assert r.status_code == 503
    state = c.post("/v1/sessions/step").json()
    assert state["open"] == 0 and state["free_blocks"] == 3
    r = c.post("/v1/sessions/batch", json={"prompts": [small],
                                           "max_tokens": 2})
    assert r.status_code == 200 and len(r.json()["session_ids"]) == 1
