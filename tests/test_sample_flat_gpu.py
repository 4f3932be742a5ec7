"""k_sample_onepass_flat against k_sample_onepass: the same token and the
same out_tokens write, greedy and Gumbel, across the vocab % 8 tail, rows
that exactly fill a preload depth (4, 8, 16 vectors per thread) and rows one
vector past the deepest, which fall back to the looping kernel."""

import pytest
import torch

from fei_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 8: one vector. 1000: no tail, one partial slot. 8192 / 8200: thread 1023's
# last vector of slot 0 / thread 0's first of slot 1. 32768, 65536, 131072
# fill depths 4, 8, 16 exactly; +8 is one vector into the next depth, and
# 131080 is past the deepest instance. 131085 adds a vocab % 8 tail to that.
VOCABS = (8, 1000, 1003, 8192, 8200, 32768, 32776, 65536, 65544, 131072,
          131080, 131085)
MAX_NEW = 6


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ops.require_lib()


def _run(logits, flat, temperature=0.0, seed=1234, step=2, max_new=MAX_NEW):
    """-> (token [B], out_tokens [B, max_new]) on the CPU; out_tokens starts
    at -7 so a write shows."""
    B = logits.shape[0]
    token = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    out = torch.full((B, max_new), -7, dtype=torch.int32, device=DEV)
    st = torch.tensor([step], dtype=torch.int32, device=DEV)
    ws = torch.empty(1, dtype=torch.float32, device=DEV)   # unused at B <= 8
    ops.sample(logits, token, st, ws, out_tokens=out, temperature=temperature,
               seed=seed, flat=flat)
    torch.cuda.synchronize()
    return token.cpu(), out.cpu()


def _check_same(logits, **kw):
    tn, on = _run(logits, True, **kw)
    to, oo = _run(logits, False, **kw)
    assert torch.equal(tn, to), f"tokens {tn.tolist()} vs {to.tolist()}"
    assert torch.equal(on, oo)
    return tn, on


@pytest.mark.parametrize("temperature", (0.0, 0.8))
@pytest.mark.parametrize("B", (1, 2))
@pytest.mark.parametrize("vocab", VOCABS)
def test_flat_sampler_equals_loop_sampler(vocab, B, temperature):
    g = torch.Generator().manual_seed(vocab + B)
    logits = (torch.randn(B, vocab, generator=g) * 4.0).to(torch.bfloat16)
    tok, out = _check_same(logits.to(DEV), temperature=temperature)
    assert ((tok >= 0) & (tok < vocab)).all()
    assert torch.equal(out[:, 2], tok)                  # step 2's column
    assert (out[:, [0, 1, 3, 4, 5]] == -7).all()
    if temperature == 0.0:
        # bf16 ties are common in a wide row: argmax with the lowest index
        want = torch.stack([(row == row.max()).nonzero()[0, 0]
                            for row in logits.float()])
        assert torch.equal(tok.long(), want)


@pytest.mark.parametrize("lo,hi", [
    (8 * 5 + 1, 8 * 5 + 6),              # inside one vector
    (8 * 5, 8 * (5 + 1024)),             # thread 5's slots 0 and 1
    (8 * 5, 8 * (5 + 15 * 1024) + 7),    # thread 5's first and last slot
    (8 * 70 + 3, 8 * 900),               # waves 1 and 14
    (8 * 1023, 131072 - 1),              # last thread, both ends of its strip
    (0, 131072 + 3),                     # vector body against the % 8 tail
])
def test_equal_maxima_take_the_lower_index(lo, hi):
    """vocab 131077 is 16384 vectors, the deepest instance's limit, plus a
    5-element tail."""
    vocab = 131072 + 5
    g = torch.Generator().manual_seed(lo)
    logits = (torch.randn(2, vocab, generator=g)).to(torch.bfloat16)
    logits[0, lo] = logits[0, hi] = 30.0
    logits[1, hi] = 30.0                                 # row 1: no tie
    tok, _ = _check_same(logits.to(DEV))
    assert tok.tolist() == [lo, hi]


def test_tail_tie_in_a_row_the_flat_kernel_takes():
    """vocab 65541: depth 8 with a 5-element tail; the maximum sits in the
    vector body and again in the tail."""
    vocab = 65541
    logits = torch.zeros(1, vocab, dtype=torch.bfloat16)
    logits[0, 40000] = logits[0, vocab - 2] = 9.0
    tok, _ = _check_same(logits.to(DEV))
    assert tok.tolist() == [40000]
    logits[0, 40000] = 0.0
    tok, _ = _check_same(logits.to(DEV))
    assert tok.tolist() == [vocab - 2]


@pytest.mark.parametrize("vocab,at", [(131072, 77777), (8200, 8199),
                                      (1003, 1001), (8, 0)])
def test_all_minus_inf_but_one(vocab, at):
    logits = torch.full((2, vocab), float("-inf"), dtype=torch.bfloat16)
    logits[0, at] = -3.0
    # row 1 stays all -inf: every element ties, index 0 wins
    for t in (0.0, 0.8):
        tok, _ = _check_same(logits.to(DEV), temperature=t)
        assert tok.tolist() == [at, 0]


@pytest.mark.parametrize("step", (MAX_NEW, MAX_NEW + 3))
@pytest.mark.parametrize("vocab", (1000, 131072))
def test_step_past_max_new_writes_no_out_token(vocab, step):
    g = torch.Generator().manual_seed(step)
    logits = torch.randn(2, vocab, generator=g).to(torch.bfloat16).to(DEV)
    tok, out = _check_same(logits, step=step)
    assert (tok >= 0).all()
    assert (out == -7).all()


def test_default_follows_the_module_flag():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(1, 4096, generator=g).to(torch.bfloat16).to(DEV)
    want, _ = _run(logits, False, temperature=0.8)
    for flag in (True, False):
        saved = ops._SAMPLE_FLAT
        ops._SAMPLE_FLAT = flag
        try:
            got, _ = _run(logits, None, temperature=0.8)
        finally:
            ops._SAMPLE_FLAT = saved
        assert torch.equal(got, want)
