"""The ring schedule of gemv_addnorm / gemv_swiglu_addnorm on the GPU: weight
slots refilled across row groups, groups dealt grid-stride over one resident
round. Pure scheduling, so every check is torch.equal against the two-launch
sequence of the same build (fused_add_rmsnorm, then linear_decode /
gemv_swiglu).

K = 512 (a partly clamped ring), 1024, 4096 (a full ring), 8704 (past the
ring: the drain schedule). Groups per workgroup forced to 1, 2, 3, 5, 7, 8
and automatic (0); for each, N / I give fewer groups than a workgroup walks
(later groups wholly past N), exactly that many, one more (two workgroups
with different trip counts), an odd last row and a last group with idle
waves."""

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
RGS = (1, 2, 3, 5, 7, 8, 0)
PAD = 16


def _ns(rg):
    r = max(rg, 1)
    return (1, 7, 8, 9, 8 * r, 8 * r + 1, 8 * (2 * r) + 3)


def _is(rg):
    r = max(rg, 1)
    return (1, 3, 4 * r, 4 * r + 1, 4 * (2 * r) + 1)


def _inputs(K, rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    bf = torch.bfloat16
    h = torch.randn(1, K, generator=g, device="cuda").to(bf)
    delta = (8.0 * torch.randn(1, K, generator=g, device="cuda")).to(bf)
    wn = (1.0 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(bf)
    w = (torch.randn(rows, K, generator=g, device="cuda") / K ** 0.5).to(bf)
    return h, delta, wn, w


def _plain(delta, h, wn, w, swiglu):
    res = h.clone()
    x, _ = ops.fused_add_rmsnorm(delta, res, wn, EPS)
    out = ops.gemv_swiglu(x, w) if swiglu else ops.linear_decode(x, w)
    return out, res


def _check(K, rows, swiglu, seed):
    h, delta, wn, w = _inputs(K, rows, seed)
    n_out = rows // 2 if swiglu else rows
    want_out, want_res = _plain(delta, h, wn, w, swiglu)
    assert not torch.equal(want_res, h)          # the add really rounds
    h_copy = h.clone()
    res_out = torch.full_like(h, float("nan"))
    buf = torch.full((1, n_out + PAD), float("nan"), dtype=h.dtype,
                     device="cuda")
    fn = ops.gemv_swiglu_addnorm if swiglu else ops.gemv_addnorm
    out = fn(delta, h, res_out, wn, w, EPS, out=buf[:, :n_out])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert not torch.isnan(buf[:, :n_out]).any()       # every row written
    assert torch.equal(buf[:, :n_out], want_out)
    assert torch.isnan(buf[:, n_out:]).all()           # nothing past N
    assert torch.equal(res_out, want_res)
    assert torch.equal(h, h_copy)                # res_in untouched, bit for bit


@pytest.mark.parametrize("rg", RGS)
@pytest.mark.parametrize("K", KS)
def test_ring_gemv_addnorm_bit_identical(monkeypatch, K, rg):
    assert ops._ADDNORM_RING and ops._addnorm_ok(1, K)
    monkeypatch.setattr(ops, "_ADDNORM_ROW_GROUPS", rg)
    for N in _ns(rg):
        _check(K, N, swiglu=False, seed=3000 + K + 31 * N + rg)


@pytest.mark.parametrize("rg", RGS)
@pytest.mark.parametrize("K", KS)
def test_ring_gemv_swiglu_addnorm_bit_identical(monkeypatch, K, rg):
    assert ops._ADDNORM_RING and ops._addnorm_ok(1, K)
    monkeypatch.setattr(ops, "_ADDNORM_ROW_GROUPS_SWIGLU", rg)
    for I in _is(rg):
        _check(K, 2 * I, swiglu=True, seed=4000 + K + 31 * I + rg)


def test_auto_grid_wraps_past_the_resident_round(monkeypatch):
    """More groups than the device holds workgroups: the automatic plan's
    grid is the slot count and five workgroups walk a second group."""
    K = 4096
    monkeypatch.setattr(ops, "_ADDNORM_ROW_GROUPS", 0)
    slots = max(ops._addnorm_slots(False, 1, t, K) for t in (1, 2))
    groups = slots + 5
    N = 8 * groups
    assert N * K * 2 >= ops._GEMV_NT_MIN_BYTES         # the instance queried
    grid, trips = ops._addnorm_auto_plan(False, 1, K, groups)
    assert trips == 2 and grid < groups
    assert grid == ops._addnorm_slots(False, 1, 2, K)
    _check(K, N, swiglu=False, seed=77)


def test_ring_chain_in_graph_matches_eager_plain_chain(monkeypatch):
    """Two layers of the decode pattern (gate/up, qkv, gate/up, qkv) over two
    residual buffers with the ring on, several trips per workgroup, captured
    once and replayed three times with new inputs."""
    monkeypatch.setattr(ops, "_ADDNORM_ROW_GROUPS", 3)
    monkeypatch.setattr(ops, "_ADDNORM_ROW_GROUPS_SWIGLU", 5)
    assert ops._ADDNORM_RING
    K, N, I = 2048, 8 * 7 + 3, 4 * 11 + 1
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(13)
    wn = [(1.0 + 0.1 * torch.randn(K, generator=g)).to(bf).cuda()
          for _ in range(4)]
    wgu = [(torch.randn(2 * I, K, generator=g) / K ** 0.5).to(bf).cuda()
           for _ in range(2)]
    wqkv = [(torch.randn(N, K, generator=g) / K ** 0.5).to(bf).cuda()
            for _ in range(2)]
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
    for seed in (41, 42, 43):
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


_AB_CASES = [(4096, 8 * 5 + 3, 4 * 9 + 1), (1024, 9, 5), (512, 25, 13)]

_CHILD = r"""
import json, sys, torch
from fei_amd import ops
sys.path.insert(0, "tests")
import test_gemv_addnorm_ring_gpu as t
res = {"ring": ops._ADDNORM_RING, "outs": []}
for K, N, I in t._AB_CASES:
    for swiglu, rows in ((False, N), (True, 2 * I)):
        h, delta, wn, w = t._inputs(K, rows, 900 + K)
        res_out = torch.empty_like(h)
        fn = ops.gemv_swiglu_addnorm if swiglu else ops.gemv_addnorm
        out = fn(delta, h, res_out, wn, w, t.EPS)
        torch.cuda.synchronize()
        res["outs"].append(out.view(torch.int16).cpu().flatten().tolist())
        res["outs"].append(res_out.view(torch.int16).cpu().flatten().tolist())
print("RESULT " + json.dumps(res))
"""


def test_ring_switch_off_gives_the_same_bits():
    """FEI_ADDNORM_RING=0 (the drain schedule, contiguous groups) and the
    default, each in a fresh child process, at the default group counts."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for flag in ("1", "0"):
        env = dict(os.environ, FEI_ADDNORM_RING=flag)
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
    assert on["ring"] is True and off["ring"] is False
    assert len(on["outs"]) == 4 * len(_AB_CASES)
    assert on["outs"] == off["outs"]
