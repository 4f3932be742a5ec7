"""k_gemv_deep (the deep-pipelined batch-1 GEMV) on the GPU: bit-identical
to k_gemv<1,*> in the same build. No tolerance anywhere: torch.equal only.

K reaches each edge of the register ring (8 loop iterations of 512 columns):
8 (one vec8, 63 idle lanes), 512 (exactly one iteration), 520 (lane 0 has
two iterations, the others one), 4096 (the ring exactly full), 4608 (one
full ring plus one tail iteration), 14336 and 28672 (several trips round the
ring, partial last trip). N covers the odd last row, a partly empty last
workgroup and more than one workgroup."""

import pytest
import torch

from fei_amd import ops

pytestmark = pytest.mark.gpu

KS = (8, 512, 520, 4096, 4608, 14336, 28672)
NS = (1, 2, 7, 8, 9, 24)
NT_ON, NT_OFF = 0, 1 << 62            # values of ops._GEMV_NT_MIN_BYTES


def _inputs(K, N, seed):
    g = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16
    x = torch.randn(1, K, generator=g).to(bf).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(bf).cuda()
    return x, w


def _both(x, w, monkeypatch):
    """(old, deep) outputs for nontemporal and plain weight loads."""
    pairs = []
    for nt_min in (NT_ON, NT_OFF):
        monkeypatch.setattr(ops, "_GEMV_NT_MIN_BYTES", nt_min)
        old = ops.linear_decode(x, w, deep=False)
        new = ops.linear_decode(x, w, deep=True)
        torch.cuda.synchronize()
        pairs.append((old, new))
    return pairs


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_deep_bit_identical(K, N, monkeypatch):
    assert ops._gemv_deep_ok(1, K)
    x, w = _inputs(K, N, 3000 + K + N)
    for old, new in _both(x, w, monkeypatch):
        assert new.shape == old.shape == (1, N)
        assert old.float().abs().max() > 0        # the reference is not empty
        assert torch.equal(new, old)


@pytest.mark.parametrize("N,K", [(4096, 4096), (4096, 14336)])
def test_deep_bit_identical_real_shapes(N, K, monkeypatch):
    x, w = _inputs(K, N, 17 + K)
    for old, new in _both(x, w, monkeypatch):
        assert torch.equal(new, old)


@pytest.mark.parametrize("K", (520, 4608, 14336))
def test_deep_zeros_and_negatives(K, monkeypatch):
    """Exact zeros (+0 and -0), an all-negative stretch and whole zero weight
    rows: masked and zero iterations leave the chain's bits alone."""
    x, w = _inputs(K, 9, 41 + K)
    x[0, ::3] = 0.0
    x[0, 1::7] = -0.0
    x[0, K // 2:] = -x[0, K // 2:].abs()
    w[4] = 0.0
    w[8, : K // 2] = 0.0
    for old, new in _both(x, w, monkeypatch):
        assert torch.equal(new.view(torch.int16), old.view(torch.int16))
        assert float(old[0, 4]) == 0.0


def test_deep_preallocated_out():
    x, w = _inputs(4608, 9, 5)
    want = ops.linear_decode(x, w, deep=False)
    buf = torch.full((2, 9), float("nan"), dtype=torch.bfloat16, device="cuda")
    got = ops.linear_decode(x, w, out=buf[:1], deep=True)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:1], want)
    assert torch.isnan(buf[1]).all()              # nothing past the N outputs


class _Recorder:
    """Stands in for the loaded library and notes which entry points run."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def _gemv_calls(rec):
    return [c for c in rec.calls if c in ("fei_gemv", "fei_gemv_deep")]


def test_keyword_switch_and_rule_select_the_kernel(monkeypatch):
    rec = _Recorder(ops.require_lib())
    monkeypatch.setattr(ops, "_LIB", rec)
    x, w = _inputs(512, 24, 9)
    ops.linear_decode(x, w, deep=True)
    ops.linear_decode(x, w, deep=False)
    assert _gemv_calls(rec) == ["fei_gemv_deep", "fei_gemv"]

    rec.calls.clear()                             # the rule: 3 workgroups
    monkeypatch.setattr(ops, "_GEMV_DEEP", True)
    ops.linear_decode(x, w)
    monkeypatch.setattr(ops, "_GEMV_DEEP", False)  # what FEI_GEMV_DEEP=0 sets
    ops.linear_decode(x, w)
    assert _gemv_calls(rec) == ["fei_gemv_deep", "fei_gemv"]

    rec.calls.clear()                             # a grid that fills the CUs
    monkeypatch.setattr(ops, "_GEMV_DEEP", True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_full = int(ops._GEMV_DEEP_MAX_WG_PER_CU * cus) * 8
    xs, ws = _inputs(8, n_full, 10)
    ops.linear_decode(xs, ws)
    ops.linear_decode(xs, ws[: n_full - 8])       # one workgroup fewer
    assert _gemv_calls(rec) == ["fei_gemv", "fei_gemv_deep"]

    rec.calls.clear()                             # batch 2 and a K past the
    x2 = torch.cat([x, x])                        # unrolled trips: old kernel
    ops.linear_decode(x2, w)
    k_big = 8 * 512 * ops._GEMV_DEEP_MAX_TRIPS + 8
    assert not ops._gemv_deep_ok(1, k_big)
    xb, wb = _inputs(k_big, 2, 11)
    ops.linear_decode(xb, wb)
    assert _gemv_calls(rec) == ["fei_gemv", "fei_gemv"]
    torch.cuda.synchronize()


def test_deep_refuses_what_it_cannot_run():
    x, w = _inputs(512, 8, 12)
    with pytest.raises(ValueError):
        ops.linear_decode(torch.cat([x, x]), w, deep=True)
    k_big = 8 * 512 * ops._GEMV_DEEP_MAX_TRIPS + 8
    xb, wb = _inputs(k_big, 2, 13)
    with pytest.raises(ValueError):
        ops.linear_decode(xb, wb, deep=True)


def test_engine_logits_identical_with_and_without_deep(monkeypatch):
    """llama3-tiny, greedy, eager decode: every step's logits with the deep
    kernel dispatched equal those with it switched off."""
    from fei_amd.engine.engine import LocalEngine

    runs = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "_GEMV_DEEP", on)
        rec = _Recorder(ops.require_lib())
        monkeypatch.setattr(ops, "_LIB", rec)
        eng = LocalEngine.create("llama3-tiny", max_seq_len=256, seed=7,
                                 use_hip_graph=False)
        steps = []
        orig = eng.model.forward_decode

        def wrapped(*a, _orig=orig, _steps=steps, **k):
            _steps.append(_orig(*a, **k).clone())
            return _steps[-1]
        eng.model.forward_decode = wrapped
        out = eng.generate("keep the weight stream in flight",
                           max_new_tokens=6, stop_on_eos=False)
        torch.cuda.synchronize()
        eng.shutdown()
        runs[on] = (steps, [int(t) for t in out["token_ids"]], rec.calls)
    (s_on, t_on, c_on), (s_off, t_off, c_off) = runs[True], runs[False]
    assert "fei_gemv_deep" in c_on and "fei_gemv_deep" not in c_off
    assert t_on == t_off
    assert len(s_on) == len(s_off) >= 5
    for a, b in zip(s_on, s_off):
        assert torch.equal(a, b)
