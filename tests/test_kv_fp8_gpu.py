"""GPU tests of the fp8 KV cache kernels (csrc/kv_fp8.hip) and the engine
running on them.

Caches are built by quantising random bf16 with the reference
(reference.quant_kv_fp8, on the CPU) and the attention kernels are compared
with the reference attention over the DEQUANTISED cache, which isolates
kernel error from quantisation error.

Rows get very different magnitudes: some positions are multiplied by 8 and
others by 1/64, at different positions for K and for V, so a kernel that
drops, swaps or mis-indexes a scale is off by far more than the tolerance.
q is drawn at 2x so that the softmax concentrates on a handful of the
boosted keys and the output is a few V rows, not an average that would hide
a wrong scale. Base magnitudes are K 1/8 and V 1/8 (a boosted row is 1
sigma). Computed on the CPU, the expected outputs of the cases below reach
max |out| 0.2-3.1 (rms 0.02-0.26): below 4, where one bf16 ulp (2^-6) is
still under the 2e-2 absolute bound the bf16 kernels' tests use.

Because the long cases (n >= 300) have an output rms near that absolute
bound, every comparison ALSO asserts a relative L2 error below 1e-2. Kernel
and reference see the same dequantised values, so what separates them is
rounding: both outputs are rounded to bf16 (2 roundings), and the prefill
kernel also rounds the dequantised K, V and the probabilities to bf16 for
the MFMAs (3 more). Each is at most 2^-9 relative; five of them add up to
9.8e-3 < 1e-2 in the worst case (f32 accumulation order and __expf are
orders of magnitude below that).
"""

import functools

import pytest
import torch

from fei_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT_CODE, SENT_SCALE = 0x55, -3.0


@pytest.fixture(scope="module")
def lib():
    from fei_amd import ops
    ops.require_lib()
    return ops


def randbf(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _cache_cpu(B, Hkv, MS, D, seed, which):
    """(codes, scales, dequantised f32) of a random cache, on the CPU."""
    base = 1.0 / 8
    x = randbf(B, Hkv, MS, D, seed=seed, scale=base).float()
    p = torch.arange(MS)
    up, down = ((p % 7 == 1, p % 5 == 2) if which == "k"
                else (p % 6 == 3, p % 4 == 1))
    x[:, :, up] *= 8.0
    x[:, :, down] /= 64.0
    codes, scales = ref.quant_kv_fp8(x.to(torch.bfloat16))
    return codes, scales, ref.dequant_kv_fp8(codes, scales)


def _cache(lib, B, Hkv, MS, D, seed, which):
    codes, scales, dq = _cache_cpu(B, Hkv, MS, D, seed, which)
    return lib.QuantKV(codes.to(DEV), scales.to(DEV)), dq


def _sentinel_cache(lib, B, Hkv, MS, D):
    return lib.QuantKV(
        torch.full((B, Hkv, MS, D), SENT_CODE, dtype=torch.uint8, device=DEV),
        torch.full((B, Hkv, MS), SENT_SCALE, dtype=torch.float32, device=DEV))


def _format_bound(x, scale):
    """the format's own error bound (tests/test_kv_fp8_cpu.py)"""
    return x.abs() / 16 + scale.unsqueeze(-1) * 2.0 ** -10


def _check_out(out, expected, what):
    """abs < 2e-2 (the bf16 tests' bound) and rel-L2 < 1e-2 (module
    docstring); figures are printed before they are asserted."""
    o, e = out.cpu().float(), expected.float()
    err = (o - e).abs().max().item()
    rel = ((o - e).norm() / e.norm()).item()
    print(f"{what}: max abs err {err:.3e}, rel L2 {rel:.3e}, "
          f"max |out| {e.abs().max().item():.3f}")
    assert err < 2e-2, f"{what}: max abs err {err}"
    assert rel < 1e-2, f"{what}: rel L2 err {rel}"


def _check_append(kc, vc, k_raw, v_raw, k_roped, written):
    """kc/vc: QuantKV after the kernel. k_raw/v_raw/k_roped: CPU tensors
    [B, Hkv, MS, D] holding the expected rows at the written positions
    (k_roped = reference RoPE, f32). written: bool [B, MS]."""
    kd, ks = kc.data.cpu(), kc.scale.cpu()
    vd, vs = vc.data.cpu(), vc.scale.cpu()
    B = kd.shape[0]
    for b in range(B):
        w = written[b]
        # V: bit-equal codes and scales
        vq, vsq = ref.quant_kv_fp8(v_raw[b][:, w])
        assert torch.equal(vd[b][:, w], vq)
        assert torch.equal(vs[b][:, w], vsq)
        # K at position 0: RoPE is the identity there -> bit-equal
        if w[0]:
            kq, ksq = ref.quant_kv_fp8(k_raw[b][:, 0])
            assert torch.equal(kd[b][:, 0], kq)
            assert torch.equal(ks[b][:, 0], ksq)
        # K elsewhere: format bound + the 2e-2 the bf16 RoPE tests allow
        dq = ref.dequant_kv_fp8(kd[b][:, w], ks[b][:, w])
        want = k_roped[b][:, w]
        err = (dq - want).abs()
        assert bool((err <= _format_bound(want, ks[b][:, w]) + 2e-2).all()), \
            f"max K err {err.max().item()}"
        # every other row still holds the sentinel
        assert bool((kd[b][:, ~w] == SENT_CODE).all())
        assert bool((vd[b][:, ~w] == SENT_CODE).all())
        assert bool((ks[b][:, ~w] == SENT_SCALE).all())
        assert bool((vs[b][:, ~w] == SENT_SCALE).all())


@pytest.mark.parametrize("D", [64, 128])
def test_append_decode_form(lib, D):
    B, Hq, Hkv, MS = 2, 8, 2, 64
    q = randbf(B, Hq, D, seed=7)
    k = randbf(B, Hkv, D, seed=8)
    v = randbf(B, Hkv, D, seed=9)
    pos = torch.tensor([0, 11], dtype=torch.int32)
    table = ref.rope_table(MS, D)
    kc, vc = (_sentinel_cache(lib, B, Hkv, MS, D) for _ in range(2))
    q_gpu = q.to(DEV)
    lib.rope_kv_decode(q_gpu, k.to(DEV), v.to(DEV), kc, vc, pos.to(DEV),
                       table.to(DEV))
    q_ref = ref.apply_rope(q, pos, table)
    assert (q_gpu.cpu().float() - q_ref.float()).abs().max() < 2e-2
    written = torch.zeros(B, MS, dtype=torch.bool)
    k_raw = torch.zeros(B, Hkv, MS, D, dtype=torch.bfloat16)
    v_raw = torch.zeros_like(k_raw)
    k_roped = torch.zeros(B, Hkv, MS, D)
    kr = ref.apply_rope(k.float(), pos, table)
    for b, p in enumerate(pos.tolist()):
        written[b, p] = True
        k_raw[b, :, p], v_raw[b, :, p], k_roped[b, :, p] = k[b], v[b], kr[b]
    _check_append(kc, vc, k_raw, v_raw, k_roped, written)


@pytest.mark.parametrize("D", [64, 128])
def test_append_prefill_form_strided(lib, D):
    """q/k/v as strided views into a fused qkv buffer."""
    B, S, Hq, Hkv, MS = 2, 9, 4, 2, 64
    W = (Hq + 2 * Hkv) * D
    qkv_cpu = randbf(B * S, W, seed=10)
    qkv = qkv_cpu.to(DEV)

    def views(t):
        return (t.as_strided((B, S, Hq, D), (S * W, W, D, 1)),
                t.as_strided((B, S, Hkv, D), (S * W, W, D, 1),
                             storage_offset=Hq * D),
                t.as_strided((B, S, Hkv, D), (S * W, W, D, 1),
                             storage_offset=(Hq + Hkv) * D))

    q, k, v = views(qkv)
    qc, kcpu, vcpu = (t.contiguous() for t in views(qkv_cpu))
    pos0 = torch.tensor([0, 5], dtype=torch.int32)
    table = ref.rope_table(MS, D)
    kc, vc = (_sentinel_cache(lib, B, Hkv, MS, D) for _ in range(2))
    lib.rope_kv_prefill(q, k, v, kc, vc, pos0.to(DEV), table.to(DEV))
    positions = pos0.view(B, 1).long() + torch.arange(S).view(1, S)
    q_ref = ref.apply_rope(qc, positions, table)
    assert (q.cpu().float() - q_ref.float()).abs().max() < 2e-2
    kr = ref.apply_rope(kcpu.float(), positions, table)       # [B,S,Hkv,D]
    written = torch.zeros(B, MS, dtype=torch.bool)
    k_raw = torch.zeros(B, Hkv, MS, D, dtype=torch.bfloat16)
    v_raw = torch.zeros_like(k_raw)
    k_roped = torch.zeros(B, Hkv, MS, D)
    for b, p in enumerate(pos0.tolist()):
        written[b, p:p + S] = True
        k_raw[b, :, p:p + S] = kcpu[b].transpose(0, 1)
        v_raw[b, :, p:p + S] = vcpu[b].transpose(0, 1)
        k_roped[b, :, p:p + S] = kr[b].transpose(0, 1)
    _check_append(kc, vc, k_raw, v_raw, k_roped, written)


# (n, splits, D, MS, pos): the bf16 test's cases, one D=64 case, and a long
# one where sequence 0 has chunk >= 64 and sequence 1 a short chunk in the
# same launch
DECODE_CASES = [
    (1, 1, 128, 1024, None), (7, 4, 128, 1024, None),
    (20, 32, 128, 1024, None), (300, 16, 128, 1024, None),
    (1000, 32, 128, 1024, None), (300, 32, 64, 1024, None),
    (2100, 32, 128, 4096, [2099, 700]),
]


def _decode_inputs(lib, n, D, MS, pos):
    B, Hq, Hkv = 2, 8, 2
    q = randbf(B, Hq, D, seed=20 + n, scale=2.0).to(DEV)
    kc, kdq = _cache(lib, B, Hkv, MS, D, 21 + n, "k")
    vc, vdq = _cache(lib, B, Hkv, MS, D, 22 + n, "v")
    if pos is None:
        pos = [n - 1, max(n // 2 - 1, 0)]
    return q, kc, vc, kdq, vdq, torch.tensor(pos, dtype=torch.int32)


@pytest.mark.parametrize("n,splits,D,MS,pos", DECODE_CASES)
def test_attn_decode(lib, n, splits, D, MS, pos):
    q, kc, vc, kdq, vdq, pos = _decode_inputs(lib, n, D, MS, pos)
    out = lib.attn_decode(q, kc, vc, pos.to(DEV), splits=splits)
    expected = ref.attn_decode(q.cpu(), kdq, vdq, pos + 1)
    _check_out(out, expected, f"n={n} splits={splits} D={D}")


@pytest.mark.parametrize("n,splits,D,MS,pos", DECODE_CASES)
def test_attn_decode_tail_safety(lib, n, splits, D, MS, pos):
    """Positions >= n hold NaN codes and inf scales: the kernel must never
    read them — output finite and bit-identical to the zero-tail run."""
    q, kc, vc, _, _, pos = _decode_inputs(lib, n, D, MS, pos)
    outs = []
    for code, sc in ((0, 0.0), (0x7F, float("inf"))):
        caches = []
        for c in (kc, vc):
            d, s = c.data.clone(), c.scale.clone()
            for b, p in enumerate(pos.tolist()):
                d[b, :, p + 1:] = code
                s[b, :, p + 1:] = sc
            caches.append(lib.QuantKV(d, s))
        outs.append(lib.attn_decode(q, caches[0], caches[1], pos.to(DEV),
                                    splits=splits).cpu())
    assert bool(torch.isfinite(outs[1].float()).all())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("splits", [4, 32])
@pytest.mark.parametrize("n", [1, 20, 300])
def test_attn_decode_rope_append_fused(lib, n, splits):
    B, Hq, Hkv, D, MS = 2, 8, 2, 128, 1024
    W = (Hq + 2 * Hkv) * D
    qkv_cpu = randbf(B, W, seed=200 + n)
    qkv_cpu[:, :Hq * D] *= 2.0                  # q at 2x (module docstring)
    qkv_cpu[:, Hq * D:(Hq + Hkv) * D] *= 0.5    # k
    qkv_cpu[:, (Hq + Hkv) * D:] *= 0.125        # v
    qkv = qkv_cpu.to(DEV)

    def views(t):
        return (t.as_strided((B, Hq, D), (W, D, 1)),
                t.as_strided((B, Hkv, D), (W, D, 1), storage_offset=Hq * D),
                t.as_strided((B, Hkv, D), (W, D, 1),
                             storage_offset=(Hq + Hkv) * D))

    q, k, v = views(qkv)
    qc, kcpu, vcpu = (t.contiguous() for t in views(qkv_cpu))
    kc, _ = _cache(lib, B, Hkv, MS, D, 201 + n, "k")
    vc, _ = _cache(lib, B, Hkv, MS, D, 202 + n, "v")
    pos = torch.tensor([n - 1, max(n // 2 - 1, 0)], dtype=torch.int32)
    table = ref.rope_table(MS, D)

    # reference: append, then attention over the dequantised cache
    kd_r, ks_r = kc.data.cpu(), kc.scale.cpu()
    vd_r, vs_r = vc.data.cpu(), vc.scale.cpu()
    q_ref = ref.rope_kv_decode_fp8(qc, kcpu, vcpu, kd_r, ks_r, vd_r, vs_r,
                                   pos, table)
    expected = ref.attn_decode(q_ref, ref.dequant_kv_fp8(kd_r, ks_r),
                               ref.dequant_kv_fp8(vd_r, vs_r), pos + 1)

    # the stand-alone append kernel on copies of the same caches
    kc_a = lib.QuantKV(kc.data.clone(), kc.scale.clone())
    vc_a = lib.QuantKV(vc.data.clone(), vc.scale.clone())
    lib.rope_kv_decode(q.contiguous(), k, v, kc_a, vc_a, pos.to(DEV),
                       table.to(DEV))

    out = lib.attn_decode(q, kc, vc, pos.to(DEV), splits=splits, k=k, v=v,
                          table=table.to(DEV))
    _check_out(out, expected, f"fused n={n} splits={splits}")
    # the whole cache — the written row included — is byte-identical to
    # what the stand-alone append kernel leaves
    assert torch.equal(kc.data, kc_a.data)
    assert torch.equal(kc.scale, kc_a.scale)
    assert torch.equal(vc.data, vc_a.data)
    assert torch.equal(vc.scale, vc_a.scale)
    # and the row really was written (V codes equal the reference's)
    for b, p in enumerate(pos.tolist()):
        assert torch.equal(vc.data[b, :, p].cpu(), vd_r[b, :, p])
        assert torch.equal(vc.scale[b, :, p].cpu(), vs_r[b, :, p])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S,pos0", [(1, [0, 0]), (9, [0, 5]), (70, [0, 3]),
                                    (64, [130, 1])])
def test_attn_prefill(lib, D, S, pos0):
    B, Hq, Hkv, MS = 2, 4, 2, 256
    q = randbf(B, S, Hq, D, seed=30 + S + D, scale=2.0).to(DEV)
    kc, kdq = _cache(lib, B, Hkv, MS, D, 31 + S, "k")
    vc, vdq = _cache(lib, B, Hkv, MS, D, 32 + S, "v")
    # poison everything past each sequence's valid length: never read
    pos0 = torch.tensor(pos0, dtype=torch.int32)
    kc = lib.QuantKV(kc.data.clone(), kc.scale.clone())
    vc = lib.QuantKV(vc.data.clone(), vc.scale.clone())
    for b, p in enumerate(pos0.tolist()):
        for c in (kc, vc):
            c.data[b, :, p + S:] = 0x7F
            c.scale[b, :, p + S:] = float("inf")
    out = lib.attn_prefill(q, kc, vc, pos0.to(DEV))
    expected = ref.attn_prefill(q.cpu(), kdq, vdq, pos0)
    _check_out(out, expected, f"prefill D={D} S={S}")


# -- engine --------------------------------------------------------------------

PROMPT = [(7 * i + 3) % 250 + 1 for i in range(40)]
MORE = [(11 * i + 5) % 250 + 1 for i in range(9)]
N_NEW = 16


def _engine(**kw):
    from fei_amd.engine.engine import LocalEngine
    return LocalEngine.create("llama3-tiny", kv_quant="fp8", **kw)


def _gen(eng, ids, **kw):
    return eng.generate(ids, max_new_tokens=N_NEW, stop_on_eos=False,
                        **kw)["token_ids"]


@pytest.fixture(scope="module")
def fresh_full(lib):
    """greedy tokens of PROMPT and of PROMPT+MORE from engines that prefill
    the whole prompt once and never recapture"""
    return _gen(_engine(), PROMPT), _gen(_engine(), PROMPT + MORE)


def test_engine_graph_matches_eager(lib, fresh_full):
    eng = _engine(use_hip_graph=True)
    first = _gen(eng, PROMPT)
    assert eng._graph is not None and eng.kv_dtype == "fp8"
    assert isinstance(eng.k_caches[0], lib.QuantKV)
    assert len(first) == N_NEW
    assert first == _gen(_engine(use_hip_graph=False), PROMPT)
    assert first == fresh_full[0]
    # a second, replayed request
    assert _gen(eng, PROMPT) == first


def test_engine_prefix_cache_continuation(lib, fresh_full):
    eng = _engine()
    _gen(eng, PROMPT)
    cont = eng.generate(PROMPT + MORE, max_new_tokens=N_NEW,
                        stop_on_eos=False, from_pos=len(PROMPT))
    assert cont["cached_prefix"] == len(PROMPT) and cont["kv_dtype"] == "fp8"
    assert cont["token_ids"] == fresh_full[1]


def test_engine_recapture_keeps_prefix(lib, fresh_full):
    """A sampling-parameter change recaptures the graph AFTER the prefix is
    cached; the warm-up steps overwrite rows 1..3 of codes AND scales, and
    both must be restored."""
    eng = _engine()
    _gen(eng, PROMPT, temperature=0.8, top_k=5)       # capture #1
    g1 = eng._graph
    cont = _gen(eng, PROMPT + MORE, from_pos=len(PROMPT))   # greedy: recapture
    assert eng._graph is not g1
    assert cont == fresh_full[1]
