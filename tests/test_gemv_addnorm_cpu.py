"""gemv_addnorm / gemv_swiglu_addnorm on the CPU: the wrappers compose the
reference functions, write the new residual into res_out, leave res_in
alone, and refuse an aliased or strided residual pair."""

import pytest
import torch
import torch.nn.functional as F

from fei_amd import ops
from fei_amd.ops import reference as ref

EPS = 1e-5


def _inputs(M, K, rows, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(M, K, generator=g).to(dtype)
    delta = (8.0 * torch.randn(M, K, generator=g)).to(dtype)
    wn = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dtype)
    w = (torch.randn(rows, K, generator=g) / K ** 0.5).to(dtype)
    return h, delta, wn, w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,K,N", [(1, 64, 7), (1, 256, 24), (3, 128, 10)])
def test_gemv_addnorm_cpu_equals_composed_reference(M, K, N, dtype):
    h, delta, wn, w = _inputs(M, K, N, dtype)
    x, res = ref.fused_add_rmsnorm(delta, h, wn, EPS)
    want = F.linear(x, w)
    h_copy = h.clone()
    res_out = torch.full_like(h, float("nan"))
    out = ops.gemv_addnorm(delta, h, res_out, wn, w, EPS)
    assert torch.equal(out, want)
    assert torch.equal(res_out, res.to(dtype))
    assert torch.equal(h, h_copy)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,K,I", [(1, 64, 3), (1, 256, 16), (2, 128, 5)])
def test_gemv_swiglu_addnorm_cpu_equals_composed_reference(M, K, I, dtype):
    h, delta, wn, w = _inputs(M, K, 2 * I, dtype, seed=1)
    x, res = ref.fused_add_rmsnorm(delta, h, wn, EPS)
    want = ref.swiglu(F.linear(x, w))
    h_copy = h.clone()
    res_out = torch.full_like(h, float("nan"))
    out = ops.gemv_swiglu_addnorm(delta, h, res_out, wn, w, EPS)
    assert out.shape == (M, I)
    assert torch.equal(out, want)
    assert torch.equal(res_out, res.to(dtype))
    assert torch.equal(h, h_copy)


@pytest.mark.parametrize("fn", [ops.gemv_addnorm, ops.gemv_swiglu_addnorm])
def test_aliased_or_strided_residuals_raise(fn):
    h, delta, wn, w = _inputs(1, 64, 8, torch.float32)
    with pytest.raises(ValueError):
        fn(delta, h, h, wn, w, EPS)
    with pytest.raises(ValueError):                 # a view of the same bytes
        fn(delta, h, h.view(1, 64), wn, w, EPS)
    buf = torch.zeros(1, 96)
    with pytest.raises(ValueError):                 # partial overlap
        fn(delta, buf[:, :64], buf[:, 32:].contiguous().set_(
            buf.untyped_storage(), 32, (1, 64), (64, 1)), wn, w, EPS)
    wide = torch.zeros(1, 128)
    with pytest.raises(ValueError):                 # res_out not contiguous
        fn(delta, h, wide[:, ::2], wn, w, EPS)
    with pytest.raises(ValueError):                 # res_in not contiguous
        fn(delta, wide[:, ::2], torch.zeros(1, 64), wn, w, EPS)
    with pytest.raises(ValueError):                 # shape mismatch
        fn(delta, h, torch.zeros(1, 128), wn, w, EPS)
    pair = torch.zeros(2, 1, 64)                    # disjoint halves: allowed
    pair[0] = h
    fn(delta, pair[0], pair[1], wn, w, EPS)


def test_gate():
    assert ops._addnorm_ok(1, 4096)
    assert ops._addnorm_ok(1, 16384)                # exactly 32 KB
    assert not ops._addnorm_ok(1, 16392)            # over the LDS row cap
    assert not ops._addnorm_ok(2, 4096)             # batch 1 only
    assert not ops._addnorm_ok(1, 4100)             # not a multiple of 8


def test_decode_on_cpu_is_unchanged_by_the_switch(monkeypatch):
    """The fused path engages on the GPU only: on the CPU both settings run
    the same reference chain."""
    from fei_amd.engine.engine import LocalEngine

    outs = []
    for flag in (True, False):
        monkeypatch.setattr(ops, "_ADDNORM_GEMV", flag)
        eng = LocalEngine.create("llama3-tiny", max_seq_len=64, seed=7)
        outs.append(eng.generate("abc", max_new_tokens=8,
                                 stop_on_eos=False)["token_ids"])
    assert outs[0] == outs[1]
