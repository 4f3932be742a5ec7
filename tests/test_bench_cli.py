"""bench.py command line: --steps sets the timed step count, the result
line carries ms_per_step, --dump-outputs writes the decode outputs and is
reproducible run to run, and --full leaves the headline fields and the
outputs as they are. Those runs use the tiny model on the CPU path (GPUs
hidden from the child) so they are quick everywhere; the move of the
tool-turn measurement behind --full is checked on the GPU, where it runs."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 5, 2
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype",
                 "ms_per_step")


def _bench(tmp_path, *extra):
    env = dict(os.environ, HOME=str(tmp_path), HIP_VISIBLE_DEVICES="",
               CUDA_VISIBLE_DEVICES="")
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--model", "llama3-tiny", "--steps", str(STEPS),
         "--warmup", str(WARMUP), *extra],
        capture_output=True, text=True, timeout=120, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bench")
    plain = _bench(tmp, "--dump-outputs", str(tmp / "a"))
    full = _bench(tmp, "--full", "--dump-outputs", str(tmp / "b"))
    return tmp, plain, full


def test_result_line(runs):
    _, plain, full = runs
    for res in (plain, full):
        for key in HEADLINE_KEYS:
            assert key in res
        assert res["steps"] == STEPS and res["warmup"] == WARMUP
        assert res["ms_per_step"] > 0
        # value is tokens per second of the timed steps (batch 1)
        assert res["value"] == pytest.approx(1000.0 / res["ms_per_step"],
                                             rel=0.01)
    assert not any(k.startswith("tool_turn") for k in plain["config"])
    assert {k: plain[k] for k in ("metric", "unit", "dtype")} == \
        {k: full[k] for k in ("metric", "unit", "dtype")}


def test_dump_outputs_reproducible(runs):
    tmp, _, _ = runs
    a = {n: np.load(tmp / "a" / f"{n}.npy") for n in ("tokens", "logits")}
    b = {n: np.load(tmp / "b" / f"{n}.npy") for n in ("tokens", "logits")}
    assert sorted(os.listdir(tmp / "a")) == ["logits.npy", "tokens.npy"]
    # prefill's token + one per warmup and timed step
    assert a["tokens"].shape == (1, 1 + WARMUP + STEPS)
    assert a["logits"].shape == (1, 512)          # llama3-tiny vocab
    for n in a:
        assert a[n].dtype in (np.float32, np.float64)
        assert np.isfinite(a[n]).all()
        assert np.array_equal(a[n], b[n])
    # greedy decode: the last token is the argmax of the last step's logits
    assert int(a["tokens"][0, -1]) == int(a["logits"][0].argmax())


def _bench_here(monkeypatch, capsys, *extra):
    """bench.main() in this process (saves two interpreter start-ups)."""
    import bench

    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--model", "llama3-1b",
        "--steps", str(STEPS), "--warmup", str(WARMUP), *extra])
    assert bench.main() == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.gpu
def test_tool_turns_only_with_full(monkeypatch, capsys):
    """On the GPU a plain run reports no tool-turn figures; --full reports
    them next to an unchanged headline (llama3-1b: the smallest model that
    takes the packaged tokenizer and a 2k context, as the 8B run does)."""
    plain = _bench_here(monkeypatch, capsys)
    full = _bench_here(monkeypatch, capsys, "--full")
    assert plain["dtype"] == full["dtype"] == "bf16"
    assert not any(k.startswith("tool_turn") for k in plain["config"])
    assert full["config"]["tool_turn_p50_s"] > 0
    assert full["config"]["tool_turn_n"] == 9
    assert {k: v for k, v in full["config"].items()
            if not k.startswith("tool_turn") and k != "tokenizer"
            and k != "prefill_tok_s"} == \
        {k: v for k, v in plain["config"].items() if k != "prefill_tok_s"}
    assert plain["metric"] == full["metric"]


def test_dump_outputs_budget_sample(tmp_path, monkeypatch):
    """An array over its share of the byte budget is cut to a fixed seeded
    sample (same indices every call, original order); smaller ones are
    written whole; the total stays within the budget."""
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1024)   # 512 B per array
    big = np.arange(1000, dtype=np.float32).reshape(10, 100)  # 4000 B
    small = np.arange(7, dtype=np.float64)
    for d in ("a", "b"):
        bench._dump_outputs(str(tmp_path / d), {"big": big, "small": small}, 0)
    a_big = np.load(tmp_path / "a" / "big.npy")
    assert a_big.shape == (128,) and a_big.dtype == np.float32
    assert np.all(np.diff(a_big) > 0)              # distinct, in flat order
    assert np.isin(a_big, big).all()
    assert np.array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    assert a_big.nbytes + small.nbytes <= 1024
    # other ranks write next to rank 0, not over it
    bench._dump_outputs(str(tmp_path / "a"), {"small": small}, 3)
    assert (tmp_path / "a" / "small.rank3.npy").exists()
