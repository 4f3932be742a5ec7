"""The add+norm GEMVs' grid rule and CPU fallbacks, without a GPU.

_addnorm_plan turns (groups, slots) into (grid, trips) for the grid-stride
walk group = block + g * grid, g < trips, groups past the end skipped."""

import pytest
import torch

from fei_amd import ops

PAIRS = [(3584, 768), (768, 768), (1, 768), (769, 768), (767, 768),
         (1536, 768), (1537, 768), (6144, 768), (5, 1), (13, 4),
         (3584, 1024), (4096, 512)]


def _per_block(groups, grid, trips):
    return [sum(1 for g in range(trips) if b + g * grid < groups)
            for b in range(grid)]


@pytest.mark.parametrize("groups,slots", PAIRS)
def test_plan_is_one_even_resident_round(groups, slots):
    grid, trips = ops._addnorm_plan(groups, slots)
    assert 1 <= grid <= slots
    assert 1 <= trips <= ops._ADDNORM_RING_MAX_TRIPS
    assert grid * trips >= groups
    per = _per_block(groups, grid, trips)
    assert sum(per) == groups                      # each group exactly once
    assert max(per) - min(per) <= 1
    assert min(per) >= 1                           # no workgroup without work


def test_plan_known_values():
    assert ops._addnorm_plan(3584, 768) == (768, 5)
    per = _per_block(3584, 768, 5)
    assert per.count(5) == 512 and per.count(4) == 256
    assert ops._addnorm_plan(768, 768) == (768, 1)
    assert ops._addnorm_plan(1, 768) == (1, 1)
    assert ops._addnorm_plan(769, 768) == (768, 2)


def test_plan_past_the_largest_instance_covers_every_group():
    """More groups than max_trips * slots: the trip count stops at the
    largest kernel instance and the grid grows instead."""
    cap = ops._ADDNORM_RING_MAX_TRIPS
    grid, trips = ops._addnorm_plan(cap * 768 + 1, 768)
    assert trips == cap and grid * trips >= cap * 768 + 1
    per = _per_block(cap * 768 + 1, grid, trips)
    assert sum(per) == cap * 768 + 1 and max(per) - min(per) <= 1


def test_plan_rejects_empty_input():
    for groups, slots in ((0, 768), (5, 0)):
        with pytest.raises(ValueError):
            ops._addnorm_plan(groups, slots)


def test_fixed_plan_keeps_groups_per_workgroup():
    for groups in (1, 7, 8, 9, 3584):
        for rg in (1, 2, 3, 5, 7, 8):
            grid, trips = ops._addnorm_fixed_plan(groups, rg)
            assert trips == rg and grid * trips >= groups
            assert (grid - 1) * trips < groups     # no wholly idle workgroup


def test_defaults_and_switches_exist():
    assert ops._ADDNORM_ROW_GROUPS >= 0
    assert ops._ADDNORM_ROW_GROUPS_SWIGLU >= 0
    assert isinstance(ops._ADDNORM_RING, bool)


def _inputs(K, rows, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(1, K, generator=g)
    delta = torch.randn(1, K, generator=g)
    wn = 1.0 + 0.1 * torch.randn(K, generator=g)
    w = torch.randn(rows, K, generator=g) / K ** 0.5
    return h, delta, wn, w


@pytest.mark.parametrize("rg", (0, 1, 2, 5))
@pytest.mark.parametrize("swiglu", (False, True))
def test_cpu_fallback_is_the_two_step_sequence(monkeypatch, swiglu, rg):
    monkeypatch.setattr(ops, "_ADDNORM_ROW_GROUPS", rg)
    monkeypatch.setattr(ops, "_ADDNORM_ROW_GROUPS_SWIGLU", rg)
    h, delta, wn, w = _inputs(64, 10, 3)
    res = h.clone()
    x, _ = ops.fused_add_rmsnorm(delta, res, wn, 1e-5)
    want = ops.gemv_swiglu(x, w) if swiglu else ops.linear_decode(x, w)
    h_copy, res_out = h.clone(), torch.full_like(h, float("nan"))
    fn = ops.gemv_swiglu_addnorm if swiglu else ops.gemv_addnorm
    out = fn(delta, h, res_out, wn, w, 1e-5)
    assert out.shape == want.shape
    assert torch.equal(out, want)
    assert torch.equal(res_out, res)
    assert torch.equal(h, h_copy)
