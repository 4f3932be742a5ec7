"""The deep GEMV's dispatch helpers and the CPU path of linear_decode: no GPU
needed."""

import torch

from fei_amd import ops


def test_deep_ok_follows_the_unrolled_trip_limit():
    trips = ops._GEMV_DEEP_MAX_TRIPS
    assert ops._gemv_deep_ok(1, 8)
    assert ops._gemv_deep_ok(1, 4096)
    assert ops._gemv_deep_ok(1, 28672)
    assert ops._gemv_deep_ok(1, 4096 * trips)
    assert not ops._gemv_deep_ok(1, 4096 * trips + 8)
    assert not ops._gemv_deep_ok(1, 4100)         # K % 8
    assert not ops._gemv_deep_ok(1, 0)
    assert not ops._gemv_deep_ok(2, 4096)         # batch 1 only


def test_cpu_linear_decode_ignores_the_keyword():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 64, generator=g)
    w = torch.randn(5, 64, generator=g)
    want = torch.nn.functional.linear(x, w)
    for deep in (None, True, False):
        assert torch.equal(ops.linear_decode(x, w, deep=deep), want)
