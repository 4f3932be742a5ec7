"""CPU tests of ops.sample_rows: per-row parameters, and the contract that
row b equals ops.sample_filtered on that row alone with that row's scalars."""

import pytest
import torch

from fei_amd import ops

B, V = 4, 1003
# (top_k, top_p, temperature, seed, step): greedy; top_k only; top_p only;
# both with temperature > 0
ROWS = ((0, 1.0, 0.0, 3, 0),
        (50, 1.0, 1.0, 7, 5),
        (0, 0.9, 1.0, 2 ** 33 + 1, 2),
        (40, 0.5, 0.7, 11, 9))


def logits():
    g = torch.Generator().manual_seed(21)
    return torch.randn(B, V, generator=g) * 4.0


def params(rows=ROWS):
    return dict(
        top_k=torch.tensor([r[0] for r in rows], dtype=torch.int32),
        top_p=torch.tensor([r[1] for r in rows], dtype=torch.float32),
        temperature=torch.tensor([r[2] for r in rows], dtype=torch.float32),
        seed=torch.tensor([r[3] for r in rows], dtype=torch.int64))


def steps(rows=ROWS):
    return torch.tensor([r[4] for r in rows], dtype=torch.int32)


def run_rows(x, rows=ROWS):
    n = x.shape[0]
    token = torch.full((n,), -1, dtype=torch.int32)
    info = torch.zeros(n, 2)
    out = ops.sample_rows(x, token, steps(rows), info, **params(rows))
    assert out is token
    return token, info


def run_single(x, b, rows=ROWS):
    """ops.sample_filtered on row b alone with the scalars the op reads."""
    p = params(rows)
    token = torch.full((1,), -1, dtype=torch.int32)
    info = torch.zeros(1, 2)
    ops.sample_filtered(x[b:b + 1], token, steps(rows)[b:b + 1], info,
                        temperature=float(p["temperature"][b]),
                        seed=int(p["seed"][b]), top_k=int(p["top_k"][b]),
                        top_p=float(p["top_p"][b]))
    return token, info


def test_rows_equal_sample_filtered_per_row():
    x = logits()
    token, info = run_rows(x)
    for b in range(B):
        t1, i1 = run_single(x, b)
        assert int(token[b]) == int(t1[0]), b
        assert torch.equal(info[b].view(torch.int32),
                           i1[0].view(torch.int32)), b
    assert int(token[0]) == int(x[0].argmax())           # the greedy row
    kept = info[:, 1].view(torch.int32).tolist()
    assert kept[0] == V and 50 <= kept[1] < V and 1 <= kept[2] < V
    assert 1 <= kept[3] <= kept[1]


def test_permuting_rows_permutes_outputs():
    x = logits()
    token, info = run_rows(x)
    perm = [2, 0, 3, 1]
    token_p, info_p = run_rows(x[perm].contiguous(),
                               [ROWS[i] for i in perm])
    assert torch.equal(token_p, token[perm])
    assert torch.equal(info_p.view(torch.int32), info[perm].view(torch.int32))


def test_step_and_parameters_are_not_written():
    x = logits()
    p, st = params(), steps()
    before = {k: v.clone() for k, v in p.items()}
    token = torch.zeros(B, dtype=torch.int32)
    ops.sample_rows(x, token, st, torch.zeros(B, 2), **p)
    assert torch.equal(st, steps())
    for k, v in p.items():
        assert torch.equal(v, before[k]), k


BAD = {
    "top_k": lambda p: p["top_k"].to(torch.int64),
    "top_p": lambda p: p["top_p"][:3],
    "temperature": lambda p: p["temperature"].to(torch.float64),
    "seed": lambda p: p["seed"].to(torch.int32),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_parameter_tensor_raises_with_its_name(name):
    p = params()
    p[name] = BAD[name](p)
    with pytest.raises(ValueError, match=name):
        ops.sample_rows(logits(), torch.zeros(B, dtype=torch.int32), steps(),
                        torch.zeros(B, 2), **p)


def test_bad_state_tensors_raise():
    x, p = logits(), params()
    tok, info = torch.zeros(B, dtype=torch.int32), torch.zeros(B, 2)
    with pytest.raises(ValueError, match="token"):
        ops.sample_rows(x, tok.to(torch.int64), steps(), info, **p)
    with pytest.raises(ValueError, match="step"):
        ops.sample_rows(x, tok, steps()[:1], info, **p)
    with pytest.raises(ValueError, match="info"):
        ops.sample_rows(x, tok, steps(), torch.zeros(B, 3), **p)
    with pytest.raises(ValueError, match="top_p"):     # not contiguous
        p2 = dict(p, top_p=torch.ones(B, 2)[:, 0])
        ops.sample_rows(x, tok, steps(), info, **p2)
    with pytest.raises(ValueError, match="top_k"):     # not a tensor
        ops.sample_rows(x, tok, steps(), info, **dict(p, top_k=50))
    with pytest.raises(ValueError, match="logits"):
        ops.sample_rows(x.t(), tok, steps(), info, **p)
