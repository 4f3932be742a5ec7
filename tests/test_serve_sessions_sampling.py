"""Sampling fields of the session endpoints (fastapi TestClient; CPU tiny
engine)."""

import pytest

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient

from fei_amd.engine.engine import LocalEngine
from fei_amd.engine.sessions import PagedSessionManager
from fei_amd.serve.api import create_app

SAMPLING = {"temperature": 0.8, "top_k": 20, "top_p": 0.9, "seed": 5}


@pytest.fixture(scope="module")
def engine():
    return LocalEngine.create("llama3-tiny")


@pytest.fixture(scope="module")
def client(engine):
    return TestClient(create_app(engine=engine, session_blocks=96))


def drain(client):
    for _ in range(64):
        if client.post("/v1/sessions/step?n=4").json()["active"] == 0:
            return
    raise AssertionError("sessions did not finish")


def echoed(res):
    return {k: res[k] for k in SAMPLING}


def test_open_step_get_echoes_parameters(client, engine):
    r = client.post("/v1/sessions", json={"prompt": "abc abc",
                                          "max_tokens": 8, **SAMPLING})
    assert r.status_code == 200
    sid = r.json()["session_id"]
    drain(client)
    res = client.get(f"/v1/sessions/{sid}").json()
    assert res["done"] and echoed(res) == pytest.approx(SAMPLING)
    # the tokens are the manager's for the same request
    mgr = PagedSessionManager(engine, num_blocks=16)
    ref = mgr.open("abc abc", max_new_tokens=8, **SAMPLING)
    mgr.run()
    assert res["token_ids"] == mgr.result(ref)["token_ids"]
    client.delete(f"/v1/sessions/{sid}")


@pytest.mark.parametrize("bad", ({"top_p": 1.5}, {"top_p": 0.0},
                                 {"temperature": -1.0}, {"top_k": -2},
                                 {"seed": -1}))
def test_bad_parameter_is_400(client, bad):
    before = client.post("/v1/sessions/step").json()
    r = client.post("/v1/sessions", json={"prompt": "abc", **bad})
    assert r.status_code == 400
    r = client.post("/v1/sessions/batch", json={"prompts": ["abc", "de"],
                                                **bad})
    assert r.status_code == 400
    after = client.post("/v1/sessions/step").json()
    assert (after["open"], after["free_blocks"]) == \
        (before["open"], before["free_blocks"])


def test_batch_accepts_lists_and_scalars(client):
    r = client.post("/v1/sessions/batch", json={
        "prompts": ["abc abc", "xyz xyz"], "max_tokens": 6,
        "temperature": [0.0, 0.8], "top_k": [0, 20], "top_p": 0.9,
        "seed": [0, 5]})
    assert r.status_code == 200
    a, b = r.json()["session_ids"]
    drain(client)
    ra = client.get(f"/v1/sessions/{a}").json()
    rb = client.get(f"/v1/sessions/{b}").json()
    assert echoed(ra) == pytest.approx(
        {"temperature": 0.0, "top_k": 0, "top_p": 0.9, "seed": 0})
    assert echoed(rb) == pytest.approx(SAMPLING)
    r = client.post("/v1/sessions/batch", json={
        "prompts": ["abc abc", "xyz xyz"], "seed": [1, 2, 3]})
    assert r.status_code == 400           # list length != len(prompts)
    for sid in (a, b):
        client.delete(f"/v1/sessions/{sid}")


def test_extend_without_fields_keeps_parameters(client):
    sid = client.post("/v1/sessions", json={
        "prompt": "abc abc", "max_tokens": 4, **SAMPLING}).json()["session_id"]
    drain(client)
    r = client.post(f"/v1/sessions/{sid}/extend",
                    json={"prompt": " next", "max_tokens": 4})
    assert r.status_code == 200
    res = client.get(f"/v1/sessions/{sid}").json()
    assert res["turn"] == 1 and echoed(res) == pytest.approx(SAMPLING)
    drain(client)
    r = client.post(f"/v1/sessions/{sid}/extend",
                    json={"prompt": " more", "max_tokens": 4,
                          "temperature": 0.0, "seed": 9})
    assert r.status_code == 200
    res = client.get(f"/v1/sessions/{sid}").json()
    assert echoed(res) == pytest.approx(dict(SAMPLING, temperature=0.0,
                                             seed=9))
    drain(client)
    r = client.post(f"/v1/sessions/{sid}/extend",
                    json={"prompt": " bad", "top_p": 2.0})
    assert r.status_code == 400
    assert client.get(f"/v1/sessions/{sid}").json()["turn"] == 2
    client.delete(f"/v1/sessions/{sid}")


def test_requests_without_new_fields_are_greedy_as_before(client, engine):
    """No sampling field: the tokens of a greedy engine.generate() — what the
    endpoint returned before it had sampling fields."""
    sid = client.post("/v1/sessions", json={
        "prompt": "The quick brown fox", "max_tokens": 8}).json()["session_id"]
    b = client.post("/v1/sessions/batch", json={
        "prompts": ["The quick brown fox"],
        "max_tokens": 8}).json()["session_ids"][0]
    drain(client)
    want = engine.generate("The quick brown fox",
                           max_new_tokens=8)["token_ids"]
    for s in (sid, b):
        res = client.get(f"/v1/sessions/{s}").json()
        assert res["token_ids"] == want
        assert echoed(res) == {"temperature": 0.0, "top_k": 0, "top_p": 1.0,
                               "seed": 0}
        client.delete(f"/v1/sessions/{s}")
