"""gemv_addnorm / gemv_swiglu_addnorm on the GPU: bit-identical to the
two-kernel sequence they replace (fused_add_rmsnorm, then linear_decode or
gemv_swiglu, in the same build). No tolerance anywhere: torch.equal only.

Shapes: K = 512 (64 of the 256 prologue threads have work, one dot
iteration), 1024, 4096 (two prologue iterations per thread, weight preload
exactly full), 8704 (prologue and dot tail loops past the preload); N and I
cover an odd last row, a partly empty last workgroup and waves that idle at
the barrier."""

import json
import os
import subprocess
import sys

import pytest
import torch

from fei_amd import ops

pytestmark = pytest.mark.gpu

EPS = 1e-5
KS = (512, 1024, 4096, 8704)
NS = (1, 2, 7, 8, 9, 25)
IS = (1, 3, 4, 5, 13)


def _inputs(K, rows, seed):
    g = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16
    h = torch.randn(1, K, generator=g).to(bf).cuda()
    delta = (8.0 * torch.randn(1, K, generator=g)).to(bf).cuda()
    wn = (1.0 + 0.1 * torch.randn(K, generator=g)).to(bf).cuda()
    w = (torch.randn(rows, K, generator=g) / K ** 0.5).to(bf).cuda()
    return h, delta, wn, w


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _plain(delta, h, wn, w, swiglu):
    res = h.clone()
    x, _ = ops.fused_add_rmsnorm(delta, res, wn, EPS)
    out = ops.gemv_swiglu(x, w) if swiglu else ops.linear_decode(x, w)
    return out, res


def _check(K, rows, swiglu, seed):
    h, delta, wn, w = _inputs(K, rows, seed)
    want_out, want_res = _plain(delta, h, wn, w, swiglu)
    assert not torch.equal(want_res, h)          # the add really rounds
    h_copy = h.clone()
    res_out = _nan_like(h)
    fn = ops.gemv_swiglu_addnorm if swiglu else ops.gemv_addnorm
    out = fn(delta, h, res_out, wn, w, EPS)
    torch.cuda.synchronize()
    assert out.shape == want_out.shape
    assert torch.equal(out, want_out)
    assert torch.equal(res_out, want_res)
    assert torch.equal(h, h_copy)                # res_in untouched, bit for bit


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_gemv_addnorm_bit_identical(K, N):
    assert ops._addnorm_ok(1, K)                 # the kernel runs, not the fallback
    _check(K, N, swiglu=False, seed=1000 + K + N)


@pytest.mark.parametrize("I", IS)
@pytest.mark.parametrize("K", KS)
def test_gemv_swiglu_addnorm_bit_identical(K, I):
    assert ops._addnorm_ok(1, K)
    _check(K, 2 * I, swiglu=True, seed=2000 + K + I)


def test_row_groups_do_not_change_bits(monkeypatch):
    """Walking several row groups per workgroup is pure scheduling, also when
    the last workgroup's later groups lie wholly past N."""
    for rg in (1, 2, 3, 4):
        monkeypatch.setattr(ops, "_ADDNORM_ROW_GROUPS", rg)
        monkeypatch.setattr(ops, "_ADDNORM_ROW_GROUPS_SWIGLU", rg)
        _check(4096, 25, swiglu=False, seed=31)
        _check(4096, 2 * 13, swiglu=True, seed=32)
        _check(8704, 9, swiglu=False, seed=33)


def test_gate_failure_falls_back_and_matches():
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(5)
    # batch 2 fails M == 1; K = 16392 fails the 32 KB LDS row
    for M, K in ((2, 1024), (1, 16392)):
        assert not ops._addnorm_ok(M, K)
        h = torch.randn(M, K, generator=g).to(bf).cuda()
        delta = (8.0 * torch.randn(M, K, generator=g)).to(bf).cuda()
        wn = (1.0 + 0.1 * torch.randn(K, generator=g)).to(bf).cuda()
        for swiglu in (False, True):
            w = (torch.randn(10, K, generator=g) / K ** 0.5).to(bf).cuda()
            res = h.clone()
            x, _ = ops.fused_add_rmsnorm(delta, res, wn, EPS)
            want = ops.gemv_swiglu(x, w) if swiglu else ops.linear_decode(x, w)
            h_copy, res_out = h.clone(), _nan_like(h)
            fn = ops.gemv_swiglu_addnorm if swiglu else ops.gemv_addnorm
            out = fn(delta, h, res_out, wn, w, EPS)
            assert torch.equal(out, want)
            assert torch.equal(res_out, res)
            assert torch.equal(h, h_copy)


def test_aliased_residuals_raise():
    h, delta, wn, w = _inputs(1024, 8, 7)
    with pytest.raises(ValueError):
        ops.gemv_addnorm(delta, h, h, wn, w, EPS)
    with pytest.raises(ValueError):
        ops.gemv_swiglu_addnorm(delta, h, h, wn, w, EPS)
    both = torch.zeros(2, 1, 1024, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):              # same storage, same bytes
        ops.gemv_addnorm(delta, both[0], both.view(2, 1, 1024)[0], wn, w, EPS)
    wide = torch.zeros(1, 2048, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):              # strided view
        ops.gemv_addnorm(delta, h, wide[:, ::2], wn, w, EPS)
    # two halves of one allocation do not overlap: allowed
    out = ops.gemv_addnorm(delta, h, both[1], wn, w, EPS)
    assert out.shape == (1, 8)


def test_ping_pong_chain_in_graph_matches_eager_plain_chain():
    """Four fused calls over two residual buffers (the decode layer pattern:
    gate/up, qkv, gate/up, qkv), captured once and replayed twice with new
    inputs copied in."""
    K, N, I = 1024, 24, 16
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    wn = [(1.0 + 0.1 * torch.randn(K, generator=g)).to(bf).cuda()
          for _ in range(4)]
    wgu = [(torch.randn(2 * I, K, generator=g) / K ** 0.5).to(bf).cuda()
           for _ in range(2)]
    wqkv = [(torch.randn(N, K, generator=g) / K ** 0.5).to(bf).cuda()
            for _ in range(2)]
    # stand-ins for the GEMVs between two norms: map a kernel output back to
    # a residual-sized delta
    wback_i = (torch.randn(K, I, generator=g) / I ** 0.5).to(bf).cuda()
    wback_n = (torch.randn(K, N, generator=g) / N ** 0.5).to(bf).cuda()

    def fresh(seed):
        gg = torch.Generator().manual_seed(seed)
        return (torch.randn(1, K, generator=gg).to(bf).cuda(),
                (8.0 * torch.randn(1, K, generator=gg)).to(bf).cuda())

    def plain(h0, d0):
        h, d = h0.clone(), d0
        outs = []
        for j in range(4):
            x, _ = ops.fused_add_rmsnorm(d, h, wn[j], EPS)
            if j % 2 == 0:
                o = ops.gemv_swiglu(x, wgu[j // 2])
                d = ops.linear_decode(o, wback_i)
            else:
                o = ops.linear_decode(x, wqkv[j // 2])
                d = ops.linear_decode(o, wback_n)
            outs.append(o)
        return outs, h

    h_static, d_static = fresh(0)
    hb = torch.empty(2, 1, K, dtype=bf, device="cuda")

    def fused():
        h, d, nb = h_static, d_static, 0
        outs = []
        for j in range(4):
            if j % 2 == 0:
                o = ops.gemv_swiglu_addnorm(d, h, hb[nb], wn[j], wgu[j // 2],
                                            EPS)
                d = ops.linear_decode(o, wback_i)
            else:
                o = ops.gemv_addnorm(d, h, hb[nb], wn[j], wqkv[j // 2], EPS)
                d = ops.linear_decode(o, wback_n)
            h, nb = hb[nb], nb ^ 1
            outs.append(o)
        return outs, h

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused()                                   # warm up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_outs, g_h = fused()
    for seed in (21, 22):
        h0, d0 = fresh(seed)
        want_outs, want_h = plain(h0, d0)
        h_static.copy_(h0)
        d_static.copy_(d0)
        hb.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(g_outs, want_outs):
            assert torch.equal(got, want)
        assert torch.equal(g_h, want_h)
        assert torch.equal(h_static, h0)


_CHILD = r"""
import json, sys, torch
from fei_amd import ops
from fei_amd.engine.engine import LocalEngine
res = {"addnorm": ops._ADDNORM_GEMV}
for graph in (True, False):
    eng = LocalEngine.create("llama3-tiny", max_seq_len=256, seed=7,
                             use_hip_graph=graph)
    last = {}
    orig = eng.model.forward_decode
    def wrapped(*a, _orig=orig, **k):
        last["logits"] = _orig(*a, **k)
        return last["logits"]
    eng.model.forward_decode = wrapped           # before capture, as bench.py
    out = eng.generate("fold the norm into the gemv", max_new_tokens=40,
                       stop_on_eos=False)
    torch.cuda.synchronize()
    key = "graph" if graph else "eager"
    res[key + "_used_graph"] = eng._graph is not None
    res[key + "_tokens"] = [int(t) for t in out["token_ids"]]
    res[key + "_logits"] = last["logits"].view(torch.int16).cpu().flatten().tolist()
    eng.shutdown()
print("RESULT " + json.dumps(res))
"""


def test_engine_tokens_and_logits_identical_with_and_without_fusion():
    """llama3-tiny, greedy, 40 steps, FEI_ADDNORM_GEMV=1 and =0 each in a
    fresh child process, with and without hipGraph: identical token ids and
    bit-identical last-step logits in all four runs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for flag in ("1", "0"):
        env = dict(os.environ, FEI_ADDNORM_GEMV=flag)
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        procs.append(subprocess.Popen(
            [sys.executable, "-c", _CHILD], env=env, cwd=root,
            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    runs = []
    for p in procs:
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, se[-2000:]
        line = [ln for ln in so.splitlines() if ln.startswith("RESULT ")][-1]
        runs.append(json.loads(line[len("RESULT "):]))
    on, off = runs
    assert on["addnorm"] is True and off["addnorm"] is False
    assert on["graph_used_graph"] and off["graph_used_graph"]
    assert not on["eager_used_graph"] and not off["eager_used_graph"]
    assert len(on["graph_tokens"]) == 40
    for key in ("graph_tokens", "eager_tokens"):
        assert on[key] == off[key] == on["graph_tokens"]
    for key in ("graph_logits", "eager_logits"):
        assert on[key] == off[key] == on["graph_logits"]
