"""GPU tests of the per-row sampler (csrc/sample_rows.hip). The contract is
bit equality: row b of ops.sample_rows equals ops.sample_filtered run with
B = 1 on that row alone with that row's scalars — token and both info
words — wherever the row sits in the batch."""

import ctypes
import functools

import pytest
import torch

from fei_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID = ((1, 4096), (3, 1003), (9, 1003), (2, 128256))
# (top_k, top_p, temperature), cycled over the rows
MIXES = ((0, 1.0, 0.0),          # greedy
         (1, 1.0, 0.8),
         (50, 1.0, 1.0),
         (0, 0.9, 1.0),
         (40, 0.5, 0.7),
         (0, 1.0, 0.7))          # inactive filter
SEEDS = (11, 2 ** 32 + 12345, 3, 2 ** 40 + 1, 5, 6, 7, 8, 9)
STEPS = (0, 3, 1, 17, 250, 2, 9, 40, 5)


@functools.lru_cache(maxsize=None)
def rows_for(B, V):
    g = torch.Generator().manual_seed(500 + B)
    x = (torch.randn(B, V, generator=g) * 4.0).to(torch.bfloat16)
    return x


@functools.lru_cache(maxsize=None)
def special_rows():
    """6 rows at V = 1003: only two distinct values (massive ties) x3 and a
    constant row x3, so that each meets several parameter mixes."""
    g = torch.Generator().manual_seed(9)
    two = torch.where(torch.rand(3, 1003, generator=g) < 0.3, 1.5, -0.25)
    const = torch.full((3, 1003), 0.75)
    return torch.cat([two, const]).to(torch.bfloat16)


def param_tensors(B, offset=0, dev=DEV):
    mix = [MIXES[(b + offset) % len(MIXES)] for b in range(B)]
    return dict(
        top_k=torch.tensor([m[0] for m in mix], dtype=torch.int32, device=dev),
        top_p=torch.tensor([m[1] for m in mix], dtype=torch.float32,
                           device=dev),
        temperature=torch.tensor([m[2] for m in mix], dtype=torch.float32,
                                 device=dev),
        seed=torch.tensor(SEEDS[:B], dtype=torch.int64, device=dev))


def step_tensor(B):
    return torch.tensor(STEPS[:B], dtype=torch.int32, device=DEV)


def run_rows(xg, p, step):
    B = xg.shape[0]
    token = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    info = torch.zeros(B, 2, dtype=torch.float32, device=DEV)
    ops.sample_rows(xg, token, step, info, **p)
    return token.cpu(), info.cpu().view(torch.int32)


def run_single(xg, b, p, step):
    token = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    info = torch.zeros(1, 2, dtype=torch.float32, device=DEV)
    ops.sample_filtered(xg[b:b + 1], token, step[b:b + 1].clone(), info,
                        temperature=float(p["temperature"][b]),
                        seed=int(p["seed"][b]), top_k=int(p["top_k"][b]),
                        top_p=float(p["top_p"][b]))
    return int(token[0]), info.cpu().view(torch.int32)[0]


def check_bit_equal(x, offset=0):
    xg = x.to(DEV)
    B = x.shape[0]
    p, step = param_tensors(B, offset), step_tensor(B)
    token, info = run_rows(xg, p, step)
    for b in range(B):
        t1, i1 = run_single(xg, b, p, step)
        print(f"B={B} V={x.shape[1]} row {b} mix {MIXES[(b + offset) % 6]} "
              f"token {int(token[b])} vs {t1} info {info[b].tolist()} vs "
              f"{i1.tolist()}")
        assert int(token[b]) == t1, b
        assert torch.equal(info[b], i1), b
        assert 0 <= t1 < x.shape[1]


@pytest.mark.parametrize("B,V", GRID)
def test_bit_equal_to_sample_filtered_per_row(B, V):
    # the two production-vocabulary rows take the nucleus mixes (the ones
    # that make every pass over the row)
    check_bit_equal(rows_for(B, V), offset=3 if V == 128256 else 0)


@pytest.mark.parametrize("offset", (0, 3))
def test_bit_equal_on_tied_and_constant_rows(offset):
    """offset 0 and 3 together put every mix on a two-valued row and on a
    constant row."""
    check_bit_equal(special_rows(), offset)


def test_position_independence():
    V = 1003
    x = rows_for(9, V).clone()
    for r in (3, 8):
        x[r] = x[0]
    xg = x.to(DEV)
    p, step = param_tensors(9), step_tensor(9)
    for name in p:                  # rows 3 and 8 get row 0's request...
        p[name][3] = p[name][0]
        p[name][8] = p[name][0]
    for name in ("top_k", "top_p", "temperature"):      # ...a sampled one
        p[name][[0, 3, 8]] = param_tensors(9)[name][4]
    step[[3, 8]] = int(step[0])
    token, info = run_rows(xg, p, step)
    assert int(token[0]) == int(token[3]) == int(token[8])
    assert torch.equal(info[0], info[3]) and torch.equal(info[0], info[8])


def test_seeds_give_different_streams():
    V = 1003
    x = rows_for(3, V)[:1].expand(2, V).contiguous().to(DEV)
    p = dict(top_k=torch.zeros(2, dtype=torch.int32, device=DEV),
             top_p=torch.ones(2, dtype=torch.float32, device=DEV),
             temperature=torch.ones(2, dtype=torch.float32, device=DEV),
             seed=torch.tensor([1, 2], dtype=torch.int64, device=DEV))
    step = torch.zeros(2, dtype=torch.int32, device=DEV)
    token = torch.zeros(2, dtype=torch.int32, device=DEV)
    info = torch.zeros(2, 2, device=DEV)
    out = []
    for _ in range(64):
        ops.sample_rows(x, token, step, info, **p)
        step.add_(1)
        out.append(token.clone())
    seq = torch.stack(out, dim=1).cpu()
    assert seq[0].tolist() != seq[1].tolist()
    assert len(set(seq[0].tolist())) > 8          # a spread-out T = 1 stream


def test_inputs_are_not_modified():
    x = rows_for(9, 1003).to(DEV)
    p, step = param_tensors(9), step_tensor(9)
    x0, step0 = x.clone(), step.clone()
    p0 = {k: v.clone() for k, v in p.items()}
    run_rows(x, p, step)
    assert torch.equal(x, x0) and torch.equal(step, step0)
    for k in p:
        assert torch.equal(p[k], p0[k]), k


@pytest.mark.parametrize("B,V", ((0, 1003), (2, 0)))
def test_entry_point_refuses_empty_shapes(B, V):
    lib = ops.require_lib()
    x = rows_for(3, 1003).to(DEV)
    p, step = param_tensors(3), step_tensor(3)
    token = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    info = torch.zeros(3, 2, device=DEV)
    rc = lib.fei_sample_filtered_rows(
        x.data_ptr(), token.data_ptr(), info.data_ptr(),
        p["top_k"].data_ptr(), p["top_p"].data_ptr(),
        p["temperature"].data_ptr(), p["seed"].data_ptr(), step.data_ptr(),
        B, V, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0
    assert token.tolist() == [-7, -7, -7]
    assert not info.any()


def test_graph_replay_follows_in_place_parameter_changes():
    B, V = 3, 1003
    x = rows_for(B, V).to(DEV)

    def eager(p, step, n):
        step = step.clone()
        token = torch.zeros(B, dtype=torch.int32, device=DEV)
        info = torch.zeros(B, 2, device=DEV)
        out = []
        for _ in range(n):
            ops.sample_rows(x, token, step, info, **p)
            step.add_(1)
            out.append(token.clone())
        return torch.stack(out, dim=1).cpu(), info.cpu().view(torch.int32)

    p, step = param_tensors(B, offset=2), step_tensor(B)
    start = step.clone()
    token = torch.zeros(B, dtype=torch.int32, device=DEV)
    info = torch.zeros(B, 2, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):               # warm-up outside the capture
        ops.sample_rows(x, token, step, info, **p)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.sample_rows(x, token, step, info, **p)
        step.add_(1)
    step.copy_(start)
    got = []
    for _ in range(4):
        g.replay()
        got.append(token.clone())
    want, want_info = eager(p, start, 4)
    assert torch.equal(torch.stack(got, dim=1).cpu(), want)
    assert torch.equal(info.cpu().view(torch.int32), want_info)
    assert torch.equal(step, start + 4)

    # new requests in the same rows: no recapture
    p["top_k"].copy_(torch.tensor([5, 0, 2], dtype=torch.int32))
    p["seed"].copy_(torch.tensor([2 ** 35 + 7, 99, 100], dtype=torch.int64))
    now = step.clone()
    g.replay()
    want, want_info = eager(p, now, 1)
    assert torch.equal(token.cpu(), want[:, 0])
    assert torch.equal(info.cpu().view(torch.int32), want_info)
