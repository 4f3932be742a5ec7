"""Per-session sampling in the paged session manager (CPU engine): a
session's tokens depend only on its own prompt, parameters, seed and draw
count — not on who else is in the batch, on its row index or on how it was
admitted — and greedy serving is unchanged."""

import pytest
import torch

from fei_amd import ops
from fei_amd.engine.engine import LocalEngine
from fei_amd.engine.sessions import PagedSessionManager


@pytest.fixture(scope="module")
def engine():
    return LocalEngine.create("llama3-tiny")


SAMPLED = dict(temperature=0.8, top_k=20, top_p=0.9, seed=5)
OTHER = dict(temperature=1.3, top_k=0, top_p=0.7, seed=2 ** 40 + 9)
P_SAMPLED = "def add(a, b):\n    return"
P_GREEDY = "The quick brown fox"
P_OTHER = "x = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,"
EXT = " and then"
N1, N2 = 14, 9


def manager(engine, blocks=64):
    return PagedSessionManager(engine, block_size=16, num_blocks=blocks)


def two_turns(mgr, sid):
    """run -> extend -> run for session sid; returns both turns' tokens."""
    mgr.run(chunk=4)
    t1 = mgr.result(sid)["token_ids"]
    mgr.extend(sid, EXT, max_new_tokens=N2)
    mgr.run(chunk=4)
    return t1, mgr.result(sid)["token_ids"]


@pytest.fixture(scope="module")
def solo(engine):
    mgr = manager(engine)
    sid = mgr.open(P_SAMPLED, max_new_tokens=N1, **SAMPLED)
    out = two_turns(mgr, sid)
    return out, mgr.sessions[sid].sampled


@pytest.fixture(scope="module")
def greedy_solo(engine):
    mgr = manager(engine)
    sid = mgr.open(P_GREEDY, max_new_tokens=5)
    mgr.run(chunk=4)
    assert not mgr._seen_sampled
    return mgr.result(sid)["token_ids"]


def test_sampling_is_not_greedy(engine, solo):
    """The sampled script really samples: it differs from the greedy run of
    the same prompt (otherwise the invariance tests would show nothing)."""
    mgr = manager(engine)
    sid = mgr.open(P_SAMPLED, max_new_tokens=N1)
    mgr.run(chunk=4)
    assert mgr.result(sid)["token_ids"] != solo[0][0]


def test_batch_invariance_open(engine, solo, greedy_solo):
    """Row 1 of 3, then row 0 of 2 once the greedy session has finished and
    been closed (row indices shift mid-run)."""
    mgr = manager(engine)
    g = mgr.open(P_GREEDY, max_new_tokens=5)
    s = mgr.open(P_SAMPLED, max_new_tokens=N1, **SAMPLED)
    o = mgr.open(P_OTHER, max_new_tokens=N1 + 7, **OTHER)
    assert [x.sid for x in mgr.active].index(s) == 1
    while not mgr.sessions[g].done:
        mgr.step_chunk(3)
    assert mgr.result(g)["token_ids"] == greedy_solo
    assert not mgr.sessions[s].done
    mgr.close(g)
    assert [x.sid for x in mgr.active].index(s) == 0
    while not mgr.sessions[s].done:
        mgr.step_chunk(4)
    t1 = mgr.result(s)["token_ids"]
    assert not mgr.sessions[o].done
    mgr.extend(s, EXT, max_new_tokens=N2)      # turn 1 decodes alongside o
    mgr.run(chunk=4)
    assert (t1, mgr.result(s)["token_ids"]) == solo[0]
    assert mgr.sessions[s].sampled == solo[1]


def test_batch_invariance_open_many(engine, solo, greedy_solo):
    mgr = manager(engine)
    g, o, s = mgr.open_many(
        [P_GREEDY, P_OTHER, P_SAMPLED], max_new_tokens=N1,
        temperature=[0.0, OTHER["temperature"], SAMPLED["temperature"]],
        top_k=[0, OTHER["top_k"], SAMPLED["top_k"]],
        top_p=[1.0, OTHER["top_p"], SAMPLED["top_p"]],
        seed=[0, OTHER["seed"], SAMPLED["seed"]])
    mgr.sessions[g].max_new_tokens = 5
    while not mgr.sessions[g].done:
        mgr.step_chunk(2)
    assert mgr.result(g)["token_ids"] == greedy_solo
    mgr.close(g)
    mgr.run(chunk=4)
    t1 = mgr.result(s)["token_ids"]
    firsts = mgr.extend_many([(o, " more"), (s, EXT)], max_new_tokens=N2)
    mgr.run(chunk=4)
    t2 = mgr.result(s)["token_ids"]
    assert t2[0] == firsts[1]
    assert (t1, t2) == solo[0]
    assert mgr.sessions[s].sampled == solo[1]
    assert mgr.sessions[o].temperature == pytest.approx(OTHER["temperature"])


def test_each_token_is_sample_filtered_on_its_row(engine):
    mgr = manager(engine)
    rows = []
    fwd, pre = mgr._forward_paged, mgr._prefill_paged

    def rec_fwd(*a, **k):
        out = fwd(*a, **k)
        rows.append(out[0:1].clone())
        return out

    def rec_pre(*a, **k):
        out = pre(*a, **k)
        rows.append(out[0:1].clone())
        return out

    mgr._forward_paged, mgr._prefill_paged = rec_fwd, rec_pre
    sid = mgr.open(P_SAMPLED, max_new_tokens=10, **SAMPLED)
    while mgr.active:
        mgr.step()
    toks = mgr.sessions[sid].generated
    assert len(toks) >= 2 and len(rows) >= len(toks)
    f32 = torch.tensor([SAMPLED["temperature"], SAMPLED["top_p"]],
                       dtype=torch.float32)      # what the op's tensors hold
    for i, t in enumerate(toks):
        tok = torch.zeros(1, dtype=torch.int32)
        ops.sample_filtered(rows[i].contiguous(), tok,
                            torch.tensor([i], dtype=torch.int32),
                            torch.zeros(1, 2), temperature=float(f32[0]),
                            seed=SAMPLED["seed"], top_k=SAMPLED["top_k"],
                            top_p=float(f32[1]))
        assert int(tok[0]) == t, i


def test_sampled_counts_kept_tokens(engine, solo):
    (t1, t2), sampled = solo
    assert sampled == len(t1) + len(t2)
    mgr = manager(engine)
    sid = mgr.open(P_SAMPLED, max_new_tokens=N1, **SAMPLED)
    assert mgr.sessions[sid].sampled == 1
    mgr.run(chunk=4)
    assert mgr.sessions[sid].sampled == len(mgr.sessions[sid].generated) \
        == len(t1)


def test_eos_mid_chunk_does_not_over_advance(engine, solo):
    t1 = solo[0][0]
    # a token whose first occurrence is strictly inside the first chunk of 8
    j = next(i for i in range(2, 8) if t1[i] not in t1[:i])
    mgr = manager(engine)
    mgr.eos = t1[j]
    sid = mgr.open(P_SAMPLED, max_new_tokens=N1, **SAMPLED)
    mgr.step_chunk(8)
    s = mgr.sessions[sid]
    assert s.done and s.generated == t1[:j + 1]
    assert s.sampled == j + 1 and s.pos == len(s.prompt_ids) + j


def test_extend_keeps_or_replaces_parameters(engine):
    mgr = manager(engine)
    sid = mgr.open(P_GREEDY, max_new_tokens=5, **SAMPLED)
    mgr.run()
    mgr.extend(sid, EXT, max_new_tokens=4, seed=None, top_k=7)
    s = mgr.sessions[sid]
    assert (s.seed, s.top_k) == (SAMPLED["seed"], 7)
    assert s.temperature == pytest.approx(0.8) and s.top_p == pytest.approx(0.9)
    res = mgr.result(sid)
    assert (res["seed"], res["top_k"]) == (5, 7)
    assert res["temperature"] == pytest.approx(0.8)
    assert res["top_p"] == pytest.approx(0.9)
    mgr.run()
    # temperature=0 turns the session greedy: its next turn is the argmax
    # continuation of its own context
    before = mgr.sessions[sid].sampled
    seen = []
    pre = mgr._prefill_paged

    def rec(*a, **k):
        out = pre(*a, **k)
        seen.append(out[0].clone())
        return out

    mgr._prefill_paged = rec
    first = mgr.extend(sid, EXT, max_new_tokens=4, temperature=0)
    assert first == int(seen[0].argmax())
    assert mgr.sessions[sid].temperature == 0.0
    assert mgr.sessions[sid].sampled == before + 1
    assert mgr.result(sid)["temperature"] == 0.0


BAD = (dict(temperature=-0.1), dict(temperature=float("nan")),
       dict(top_k=-1), dict(top_k=1.5), dict(top_p=0.0), dict(top_p=1.01),
       dict(seed=1.0), dict(seed=-3))


def snapshot(mgr):
    return (mgr.pool.free_blocks(),
            {sid: (s.pos, s.turn, s.sampled, list(s.generated), s.done,
                   s.temperature, s.top_k, s.top_p, s.seed,
                   len(mgr.pool.table(sid).blocks))
             for sid, s in mgr.sessions.items()})


@pytest.fixture(scope="module")
def finished(engine):
    mgr = manager(engine)
    a = mgr.open(P_GREEDY, max_new_tokens=3)
    b = mgr.open(P_SAMPLED, max_new_tokens=3, **SAMPLED)
    mgr.run()
    return mgr, a, b


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(
    f"{k}={v}" for k, v in d.items()))
def test_bad_parameters_touch_nothing(finished, bad):
    mgr, a, b = finished
    before = snapshot(mgr)
    with pytest.raises(ValueError):
        mgr.open("new one", **bad)
    with pytest.raises(ValueError):
        mgr.open_many(["new one", "another"], **bad)
    with pytest.raises(ValueError):           # one bad entry in a list
        mgr.open_many(["new one", "another"],
                      **{k: [dict(SAMPLED, seed=1)[k], v]
                         for k, v in bad.items()})
    with pytest.raises(ValueError):
        mgr.extend(a, EXT, **bad)
    with pytest.raises(ValueError):
        mgr.extend_many([(a, EXT), (b, EXT)], **bad)
    with pytest.raises(ValueError):
        mgr.extend_many([(a, EXT), (b, EXT)],
                        **{k: [None, v] for k, v in bad.items()})
    assert snapshot(mgr) == before


def test_bad_list_lengths_touch_nothing(finished):
    mgr, a, b = finished
    before = snapshot(mgr)
    for name, two, three in (("temperature", [0.5, 0.5], [0.5] * 3),
                             ("top_k", [4, 4], [4] * 3),
                             ("top_p", [0.9, 0.9], [0.9] * 3),
                             ("seed", [1, 2], [1, 2, 3])):
        with pytest.raises(ValueError, match=name):
            mgr.open_many(["p", "q", "r"], **{name: two})
        with pytest.raises(ValueError, match=name):
            mgr.extend_many([(a, EXT), (b, EXT)], **{name: three})
    assert snapshot(mgr) == before
