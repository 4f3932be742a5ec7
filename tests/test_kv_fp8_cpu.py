"""fp8 (e4m3fn + per-row f32 scale) KV cache: the storage format, the CPU
engine built on it, and the constructor's refusals. No GPU needed."""

import pytest
import torch

from fei_amd.ops import reference as ref

CPU = torch.device("cpu")


# -- format ------------------------------------------------------------------

@pytest.fixture(scope="module")
def rows():
    """10^5 random bf16 rows of D=128: Gaussian, with blocks scaled by 2^10
    and 2^-20, and some all-zero rows."""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(100_000, 128, generator=g)
    x[10_000:20_000] *= 2.0 ** 10
    x[20_000:30_000] *= 2.0 ** -20
    x[30_000:30_100] = 0.0
    x = x.to(torch.bfloat16)
    codes, scales = ref.quant_kv_fp8(x)
    return x, codes, scales


def test_format_scale(rows):
    x, codes, scales = rows
    assert codes.dtype == torch.uint8 and codes.shape == x.shape
    assert scales.dtype == torch.float32 and scales.shape == x.shape[:-1]
    amax = x.float().abs().amax(dim=-1)
    zero = amax == 0
    assert int(zero.sum()) == 100
    assert torch.equal(scales[~zero], amax[~zero] / 448.0)
    assert torch.equal(scales[zero], torch.ones(100))


def test_format_no_nan_codes(rows):
    _, codes, _ = rows
    assert not bool(((codes == 0x7F) | (codes == 0xFF)).any())


def test_format_error_bound(rows):
    """|dq - x| <= |x|/16 + scale * 2^-10: half a step of a 3-bit mantissa
    on the normal grid plus half a step of the subnormal grid (2^-9 in code
    units), both derived from the format."""
    x, codes, scales = rows
    xf = x.float()
    dq = ref.dequant_kv_fp8(codes, scales)
    bound = xf.abs() / 16 + scales.unsqueeze(-1) * 2.0 ** -10
    assert bool(((dq - xf).abs() <= bound).all())


def test_format_equals_quant_fp8(rows):
    """The row format IS reference.quant_fp8 per row. The one deliberate
    difference: an all-zero row REPORTS scale 1 (the format's rule) where
    quant_fp8 reports its clamp floor; the codes agree on every row."""
    x, codes, scales = rows
    w8, ws = ref.quant_fp8(x)
    assert torch.equal(codes, w8)
    nz = x.float().abs().amax(dim=-1) > 0
    assert torch.equal(scales[nz], ws[nz])


def test_append_reference_quantises_roped_k():
    """CPU append: v rows are quant_kv_fp8(v); k rows quantise the roped k;
    untouched rows keep their contents."""
    B, Hq, Hkv, D, MS = 2, 4, 2, 64, 16
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, Hq, D, generator=g)
    k = torch.randn(B, Hkv, D, generator=g)
    v = torch.randn(B, Hkv, D, generator=g)
    from fei_amd import ops
    kc = ops.QuantKV.zeros((B, Hkv, MS, D), CPU)
    vc = ops.QuantKV.zeros((B, Hkv, MS, D), CPU)
    kc.data.fill_(0x55); kc.scale.fill_(-3.0)
    vc.data.fill_(0x55); vc.scale.fill_(-3.0)
    pos = torch.tensor([0, 5], dtype=torch.int32)
    table = ref.rope_table(MS, D)
    ops.rope_kv_decode(q.clone(), k, v, kc, vc, pos, table)
    vq, vs = ref.quant_kv_fp8(v)
    kq, ks = ref.quant_kv_fp8(ref.apply_rope(k, pos, table))
    for b, p in enumerate(pos.tolist()):
        assert torch.equal(vc.data[b, :, p], vq[b])
        assert torch.equal(vc.scale[b, :, p], vs[b])
        assert torch.equal(kc.data[b, :, p], kq[b])
        assert torch.equal(kc.scale[b, :, p], ks[b])
        rest = torch.ones(MS, dtype=torch.bool)
        rest[p] = False
        assert bool((kc.data[b][:, rest] == 0x55).all())
        assert bool((vc.scale[b][:, rest] == -3.0).all())


# -- CPU engine ----------------------------------------------------------------

PROMPT = [(7 * i + 3) % 250 + 1 for i in range(40)]
MORE = [(11 * i + 5) % 250 + 1 for i in range(9)]
N_NEW = 12


def _engine(**kw):
    from fei_amd.engine.engine import LocalEngine
    return LocalEngine.create("llama3-tiny", device=CPU, kv_quant="fp8", **kw)


@pytest.fixture(scope="module")
def eng():
    return _engine()


@pytest.fixture(scope="module")
def greedy(eng):
    return eng.generate(PROMPT, max_new_tokens=N_NEW, stop_on_eos=False)


def test_engine_cache_layout(eng, greedy):
    from fei_amd import ops
    s = eng.spec
    for c in (*eng.k_caches, *eng.v_caches):
        assert isinstance(c, ops.QuantKV)
        assert c.data.dtype == torch.uint8
        assert c.data.shape == (1, s.num_kv_heads, eng.max_seq_len, s.head_dim)
        assert c.scale.dtype == torch.float32
        assert c.scale.shape == (1, s.num_kv_heads, eng.max_seq_len)
    assert eng._kv_bytes_per_token() == \
        s.num_layers * s.num_kv_heads * 2 * (s.head_dim + 4)


def test_engine_reports_kv_dtype(eng, greedy, monkeypatch):
    assert greedy["kv_dtype"] == "fp8"
    assert eng.last_metrics["kv_dtype"] == "fp8"
    assert eng.kv_dtype == "fp8"
    from fei_amd.engine.engine import LocalEngine
    monkeypatch.delenv("FEI_KV_QUANT", raising=False)
    plain = LocalEngine.create("llama3-tiny", device=CPU)
    assert plain.kv_dtype == "fp32"
    assert plain.generate(PROMPT[:4], max_new_tokens=2,
                          stop_on_eos=False)["kv_dtype"] == "fp32"


def test_engine_greedy_repeatable(eng, greedy):
    assert len(greedy["token_ids"]) == N_NEW
    again = eng.generate(PROMPT, max_new_tokens=N_NEW, stop_on_eos=False)
    assert again["token_ids"] == greedy["token_ids"]


def test_engine_prefix_cache_continuation(eng):
    eng.generate(PROMPT, max_new_tokens=N_NEW, stop_on_eos=False)
    cont = eng.generate(PROMPT + MORE, max_new_tokens=N_NEW,
                        stop_on_eos=False, from_pos=len(PROMPT))
    assert cont["cached_prefix"] == len(PROMPT)
    fresh = _engine().generate(PROMPT + MORE, max_new_tokens=N_NEW,
                               stop_on_eos=False)
    assert cont["token_ids"] == fresh["token_ids"]


def test_engine_speculative_matches_greedy(eng, greedy):
    spec = eng.generate(PROMPT, max_new_tokens=N_NEW, stop_on_eos=False,
                        speculative=True)
    assert spec["token_ids"] == greedy["token_ids"]
    assert "spec_blocks" in spec


def test_engine_stream_and_loglikelihood(eng, greedy):
    chunks = list(eng.generate_stream(PROMPT, max_new_tokens=N_NEW,
                                      stop_on_eos=False, chunk=5))
    assert chunks[-1]["token_ids"] == greedy["token_ids"]
    assert chunks[-1]["kv_dtype"] == "fp8"
    ll = eng.loglikelihood(PROMPT, greedy["token_ids"][:1])
    assert ll["is_greedy"] and ll["logprob"] <= 0.0


def test_engine_batch_rows_equal_solo(eng):
    prompts = [PROMPT, PROMPT[:17] + MORE]
    batch = _engine(batch_size=2).generate_batch(
        prompts, max_new_tokens=N_NEW, stop_on_eos=False)
    for p, row in zip(prompts, batch):
        solo = eng.generate(p, max_new_tokens=N_NEW, stop_on_eos=False)
        assert row["token_ids"] == solo["token_ids"]


# -- refusals --------------------------------------------------------------------

def test_unknown_kv_quant_raises():
    from fei_amd.engine.engine import LocalEngine
    with pytest.raises(ValueError, match="kv_quant"):
        LocalEngine.create("llama3-tiny", device=CPU, kv_quant="int4")


def test_env_selects_and_validates(monkeypatch):
    from fei_amd.engine.engine import LocalEngine
    monkeypatch.setenv("FEI_KV_QUANT", "fp8")
    assert LocalEngine.create("llama3-tiny", device=CPU).kv_dtype == "fp8"
    monkeypatch.setenv("FEI_KV_QUANT", "int4")
    with pytest.raises(ValueError, match="kv_quant"):
        LocalEngine.create("llama3-tiny", device=CPU)


def test_fused_attn_conflict(monkeypatch):
    monkeypatch.setenv("FEI_FUSED_ATTN", "1")
    with pytest.raises(ValueError, match="FEI_FUSED_ATTN"):
        _engine()


def test_stream_engine_conflict(monkeypatch):
    monkeypatch.setenv("FEI_STREAM_DECODE", "1")
    with pytest.raises(ValueError, match="stream"):
        _engine()


def test_tensor_parallel_conflict():
    from fei_amd.parallel.pg import ParallelContext
    with pytest.raises(ValueError, match="tensor parallel"):
        _engine(tp=ParallelContext(rank=0, world_size=2))
