"""Per-session sampling in the paged session manager on the GPU: mixed
sampled / greedy sessions over open_many -> run -> extend_many -> run, eager
and graph stepping, bf16 and fp8 pools."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCKS = 48
N1, N2 = 10, 7
PARAMS = dict(temperature=[0.8, 0.0, 1.2], top_k=[20, 0, 0],
              top_p=[0.9, 1.0, 0.8], seed=[5, 0, 2 ** 33 + 1])
GREEDY = dict(temperature=0.0, top_k=0, top_p=1.0, seed=0)


@pytest.fixture(scope="module")
def engine():
    from fei_amd.engine.engine import LocalEngine
    return LocalEngine.create("llama3-tiny", max_seq_len=256, seed=7,
                              use_hip_graph=False)


def prompts(V):
    return [[(17 * i + 3) % V for i in range(40)],
            [5, 9, 2],
            [(7 * i + 1) % V for i in range(23)]]


def script(engine, params=PARAMS, graph=False, kv_quant=None, cls=None):
    """open_many -> run -> extend_many -> run; returns per-session
    (turn-0 tokens, turn-1 tokens) and checks the bookkeeping on the way."""
    from fei_amd.engine.sessions import PagedSessionManager
    V = engine.model.spec.vocab_size
    mgr = (cls or PagedSessionManager)(engine, block_size=16,
                                       num_blocks=BLOCKS, kv_quant=kv_quant)
    mgr.use_graph = graph
    free0 = mgr.pool.free_blocks()
    ps = prompts(V)
    sids = mgr.open_many(ps, max_new_tokens=N1, **params)
    for sid, p in zip(sids, ps):
        s = mgr.sessions[sid]
        assert (s.pos, s.turn, s.sampled, len(s.generated)) == (len(p), 0, 1, 1)
    mgr.run(chunk=4)
    out = []
    for sid, p in zip(sids, ps):
        s, res = mgr.sessions[sid], mgr.result(sid)
        t = res["token_ids"]
        assert res["done"] and 1 <= len(t) <= N1
        assert all(0 <= x < V for x in t)
        assert s.sampled == len(s.generated)
        assert s.pos == len(p) + len(s.generated) - 1
        out.append([t])
    kept = [mgr.sessions[sid].sampled for sid in sids]
    pos1 = [mgr.sessions[sid].pos for sid in sids]
    exts = [[3, 141, 59], [(11 * i + 5) % V for i in range(30)], [8]]
    firsts = mgr.extend_many(list(zip(sids, exts)), max_new_tokens=N2)
    mgr.run(chunk=4)
    for i, sid in enumerate(sids):
        s, res = mgr.sessions[sid], mgr.result(sid)
        t = res["token_ids"]
        assert res["done"] and res["turn"] == 1 and t[0] == firsts[i]
        assert 1 <= len(t) <= N2 and all(0 <= x < V for x in t)
        assert s.sampled == kept[i] + len(s.generated)
        assert s.pos == pos1[i] + 1 + len(exts[i]) + len(s.generated) - 1
        out[i].append(t)
    for sid in sids:
        mgr.close(sid)
    assert mgr.pool.free_blocks() == free0
    return out, mgr


@pytest.fixture(scope="module")
def eager_run(engine):
    out, mgr = script(engine)
    assert mgr._seen_sampled and not mgr._graphs
    return out


def test_mixed_sessions_two_turns(engine, eager_run):
    # the sampled sessions really sample: not the greedy continuation
    greedy, _ = script(engine, GREEDY)
    assert eager_run[1] == greedy[1]            # the greedy session is greedy
    assert eager_run[0] != greedy[0] or eager_run[2] != greedy[2]


def test_two_managers_agree(engine, eager_run):
    again, _ = script(engine)
    assert again == eager_run


def test_graph_stepping_matches_eager(engine, eager_run):
    out, mgr = script(engine, graph=True)
    assert mgr.use_graph, "graph capture fell back to eager"
    assert mgr._graphs and all(k[2] for k in mgr._graphs)
    assert all(e["draw"] is not None for e in mgr._graphs.values())
    assert out == eager_run


def test_all_greedy_is_the_plain_argmax_path(engine):
    """All-greedy serving never reaches the sampler, and gives the tokens of
    a manager that picks every token with logits.argmax directly."""
    from fei_amd.engine.sessions import PagedSessionManager

    class ArgmaxOnly(PagedSessionManager):
        def _first_token(self, logits, draw):
            return int(logits[0].argmax())

        def _select(self, logits, draws):
            return logits.argmax(dim=-1)

        def _sample_rows(self, logits, bufs):
            raise AssertionError("sampler reached on a greedy script")

    want, _ = script(engine, GREEDY, cls=ArgmaxOnly)
    got, mgr = script(engine, GREEDY)
    assert got == want and not mgr._seen_sampled
    got_g, mgr_g = script(engine, GREEDY, graph=True)
    assert mgr_g.use_graph and all(not k[2] for k in mgr_g._graphs)
    assert got_g == want


def test_mixed_sessions_two_turns_fp8_pool(engine):
    out, mgr = script(engine, kv_quant="fp8")
    assert mgr.pool.kv_dtype == "fp8" and mgr._seen_sampled
    again, _ = script(engine, kv_quant="fp8")
    assert again == out
