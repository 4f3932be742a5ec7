"""Top-k / top-p filtered sampling: reference definition (filter_keep), the
CPU op path, LocalEngine.generate and the HTTP API (CPU tiny engine)."""

import pytest
import torch

from fei_amd import ops
from fei_amd.ops import reference as ref

KS = (1, 5, 127, 0)
PS = (0.1, 0.5, 0.9, 1.0)


def _tie_free_rows(B=3, V=128):
    g = torch.Generator().manual_seed(7)
    base = torch.linspace(-4, 4, V)
    rows = torch.stack([base[torch.randperm(V, generator=g)]
                        for _ in range(B)]).to(torch.bfloat16)
    for r in rows:
        assert r.float().unique().numel() == V      # all values distinct
    return rows


def _legacy_keep(x, k, p):
    masked = x.float()
    if k:
        masked = ref.topk_mask(masked, k)
    if p < 1.0:
        masked = ref.topp_mask(masked, p)
    return torch.isfinite(masked)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("p", PS)
def test_filter_keep_matches_masks_on_tie_free_rows(k, p):
    x = _tie_free_rows()
    keep, thr, count = ref.filter_keep(x, k, p)
    want = _legacy_keep(x, k, p)
    assert torch.equal(keep, want)
    assert torch.equal(count, want.sum(-1).to(torch.int32))
    lo = torch.where(want, x.float(), torch.full_like(x.float(), float("inf")))
    assert torch.equal(thr, lo.amin(-1))


@pytest.mark.parametrize("k", (0, 1, 7, 64))
@pytest.mark.parametrize("p", (1e-6, 0.3, 0.9, 1.0))
def test_filter_keep_all_equal_row_keeps_everything(k, p):
    x = torch.full((2, 64), 1.5, dtype=torch.bfloat16)
    keep, thr, count = ref.filter_keep(x, k, p)
    assert keep.all()
    assert count.tolist() == [64, 64]
    assert thr.tolist() == [1.5, 1.5]


def test_filter_keep_two_level_row_keeps_boundary_group_whole():
    # 4 tokens at 2.0, 12 at 0.0
    x = torch.zeros(1, 16, dtype=torch.bfloat16)
    x[0, [1, 5, 9, 13]] = 2.0
    hi = x[0].float() == 2.0
    # k inside the top group / the bottom group: the tie group is kept whole
    for k, want in ((1, 4), (3, 4), (4, 4), (5, 16), (15, 16)):
        keep, thr, count = ref.filter_keep(x, k, 1.0)
        assert int(count) == want, k
        assert torch.equal(keep[0], hi if want == 4 else torch.ones(16, dtype=torch.bool))
    # mass of the top group = 4e^2 / (4e^2 + 12) = 0.711
    keep, thr, count = ref.filter_keep(x, 0, 0.5)
    assert int(count) == 4 and float(thr) == 2.0
    keep, thr, count = ref.filter_keep(x, 0, 0.72)
    assert int(count) == 16 and float(thr) == 0.0
    # top-k cuts first, then the nucleus is taken inside the top-k set
    keep, thr, count = ref.filter_keep(x, 2, 0.99)
    assert int(count) == 4


def _run_op(x, step, **kw):
    B = x.shape[0]
    token = torch.zeros(B, dtype=torch.int32)
    info = torch.zeros(B, 2, dtype=torch.float32)
    out = torch.full((B, 4), -1, dtype=torch.int32)
    ops.sample_filtered(x, token, torch.tensor([step], dtype=torch.int32),
                        info, out_tokens=out, **kw)
    return token, info, out


def test_op_cpu_draws_inside_keep_set_and_is_seeded():
    x = _tie_free_rows()
    keep, thr, count = ref.filter_keep(x, 5, 0.9)
    seen = set()
    for step in range(4):
        t, info, out = _run_op(x, step, temperature=1.0, seed=3, top_k=5,
                               top_p=0.9)
        t2, _, _ = _run_op(x, step, temperature=1.0, seed=3, top_k=5,
                           top_p=0.9)
        assert torch.equal(t, t2)
        assert torch.equal(out[:, step], t)
        assert torch.equal(info[:, 0], thr)
        assert torch.equal(info[:, 1].view(torch.int32), count)
        for b in range(x.shape[0]):
            assert keep[b, int(t[b])]
        seen.add(tuple(t.tolist()))
    assert len(seen) > 1                    # the step feeds the noise


def test_op_cpu_inactive_filter_equals_sample():
    x = _tie_free_rows()
    for temperature in (0.0, 0.8):
        for step in range(3):
            t, info, _ = _run_op(x, step, temperature=temperature, seed=5,
                                 top_k=0, top_p=1.0)
            want = torch.zeros(3, dtype=torch.int32)
            ops.sample(x, want, torch.tensor([step], dtype=torch.int32), None,
                       temperature=temperature, seed=5)
            assert torch.equal(t, want)
            assert info[:, 1].view(torch.int32).tolist() == [128] * 3
    # k >= V is "off" as well
    t, _, _ = _run_op(x, 2, temperature=0.8, seed=5, top_k=128)
    assert torch.equal(t, want)             # `want` is the step-2, T=0.8 draw
    # greedy ignores the filter
    t, _, _ = _run_op(x, 0, temperature=0.0, seed=5, top_k=3, top_p=0.2)
    assert torch.equal(t, x.float().argmax(-1).to(torch.int32))


@pytest.mark.parametrize("kw", ({"top_p": 0.0}, {"top_p": 1.5},
                                {"top_k": -1}))
def test_op_validates_filter_arguments(kw):
    x = _tie_free_rows()
    with pytest.raises(ValueError):
        _run_op(x, 0, temperature=1.0, seed=0, **kw)


@pytest.fixture(scope="module")
def engine():
    from fei_amd.engine.engine import LocalEngine
    return LocalEngine.create("llama3-tiny")


@pytest.mark.parametrize("kw", ({"top_k": 8}, {"top_p": 0.9}))
def test_generate_filtered_is_deterministic_by_seed(engine, kw):
    from fei_amd.engine.engine import LocalEngine
    a = engine.generate("sampling test", max_new_tokens=12, temperature=1.0,
                        stop_on_eos=False, **kw)
    b = engine.generate("sampling test", max_new_tokens=12, temperature=1.0,
                        stop_on_eos=False, **kw)
    assert a["token_ids"] == b["token_ids"] and len(a["token_ids"]) == 12
    other = LocalEngine.create("llama3-tiny")   # same weights seed, no history
    c = other.generate("sampling test", max_new_tokens=12, temperature=1.0,
                       stop_on_eos=False, **kw)
    assert c["token_ids"] == a["token_ids"]


def test_generate_top_k_one_is_greedy(engine):
    # the per-step argmax of fp32 CPU logits is unique (no exact ties), so
    # top_k=1 leaves one candidate whatever the noise
    g = engine.generate("greedy check", max_new_tokens=10, stop_on_eos=False)
    s = engine.generate("greedy check", max_new_tokens=10, temperature=0.7,
                        top_k=1, stop_on_eos=False)
    assert s["token_ids"] == g["token_ids"]
    assert engine.sample_info[0, 1].view(torch.int32).item() == 1


@pytest.mark.parametrize("kw", ({"top_p": 0.0}, {"top_p": 1.5},
                                {"top_k": -1}))
def test_generate_rejects_bad_filters(engine, kw):
    with pytest.raises(ValueError):
        engine.generate("x", max_new_tokens=2, temperature=1.0, **kw)
    with pytest.raises(ValueError):
        next(engine.generate_stream("x", max_new_tokens=2, temperature=1.0,
                                    **kw))
    with pytest.raises(ValueError):
        engine.generate_batch(["x"], max_new_tokens=2, temperature=1.0, **kw)


def test_generate_stream_and_batch_take_filters(engine):
    full = engine.generate("stream me", max_new_tokens=10, temperature=1.0,
                           top_p=0.9, stop_on_eos=False)
    toks = []
    for c in engine.generate_stream("stream me", max_new_tokens=10,
                                    temperature=1.0, top_p=0.9,
                                    stop_on_eos=False, chunk=3):
        toks += c["new_token_ids"]
    assert toks == full["token_ids"]
    rows = engine.generate_batch(["stream me"], max_new_tokens=10,
                                 temperature=1.0, top_p=0.9,
                                 stop_on_eos=False)
    assert rows[0]["token_ids"] == full["token_ids"]


def test_graph_params_cover_the_filters(monkeypatch):
    """A filter change must recapture (CPU has no graphs: simulate the
    gate, as test_engine_cpu.test_graph_params_tracked does)."""
    from fei_amd.engine.engine import LocalEngine
    eng = LocalEngine.create("llama3-tiny")
    eng.use_graph = True
    captured = []

    def fake_capture():
        captured.append((eng.top_k, eng.top_p))
        eng._graph = object()
        eng._graph_params = eng._sampling_params()

    monkeypatch.setattr(eng, "_capture_graph", fake_capture)
    eng.temperature = 0.8
    eng.ensure_graph()
    eng.ensure_graph()
    assert captured == [(0, 1.0)]
    eng.top_k = 8
    eng.ensure_graph()
    eng.top_p = 0.9
    eng.ensure_graph()
    eng.ensure_graph()
    assert captured == [(0, 1.0), (8, 1.0), (8, 0.9)]
    assert eng._graph_params == (0.8, eng.seed, 8, 0.9)


def test_tensor_parallel_rejects_active_filter(engine, monkeypatch):
    class _TP:
        is_distributed = True
    monkeypatch.setattr(engine, "tp", _TP())
    with pytest.raises(ValueError, match="tensor"):
        engine._set_sampling(0.8, 8, 1.0)
    engine._set_sampling(0.0, 8, 1.0)        # greedy: the filter is moot
    engine._set_sampling(0.8, 0, 1.0)


# -- HTTP ---------------------------------------------------------------------

fastapi = pytest.importorskip("fastapi")


@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient

    from fei_amd.serve.api import create_app
    return TestClient(create_app(model="llama3-tiny"))


def test_http_top_k_request_honours_stop(client):
    req = {"prompt": "stop test", "max_tokens": 40, "temperature": 0.9,
           "top_k": 20, "stop_on_eos": False}
    text = client.post("/v1/completions", json=req).json()["choices"][0]["text"]
    assert len(text) > 6
    ss = text[3:5]
    r = client.post("/v1/completions", json={**req, "stop": [ss]})
    assert r.status_code == 200
    choice = r.json()["choices"][0]
    assert choice["text"] == text[: text.find(ss)]
    assert ss not in choice["text"]
    assert choice["finish_reason"] == "stop"


def test_http_filtered_request_uses_and_keeps_prefix_cache(client):
    req = {"prompt": "prefix cache prompt, long enough to matter",
           "max_tokens": 6, "temperature": 0.9, "top_p": 0.9,
           "stop_on_eos": False}
    a = client.post("/v1/completions", json=req).json()
    assert a["metrics"]["cached_prefix"] >= 0
    b = client.post("/v1/completions", json=req).json()
    # the first request left its prompt in the cross-request cache
    assert b["metrics"]["cached_prefix"] >= len(req["prompt"]) - 1
    assert b["choices"][0]["text"] == a["choices"][0]["text"]


def test_http_bad_filter_is_a_client_error(client):
    r = client.post("/v1/completions", json={
        "prompt": "x", "max_tokens": 2, "temperature": 0.9, "top_p": 0.0})
    assert r.status_code == 422


def test_http_stream_takes_filters(client):
    import json
    req = {"prompt": "stream abc", "max_tokens": 12, "temperature": 0.9,
           "top_k": 8, "stop_on_eos": False}
    want = client.post("/v1/completions", json=req).json()["choices"][0]["text"]
    text = ""
    with client.stream("POST", "/v1/completions",
                       json={**req, "stream": True}) as r:
        for line in r.iter_lines():
            if line.startswith("data: ") and line != "data: [DONE]":
                text += json.loads(line[6:])["choices"][0]["text"]
    assert text == want
