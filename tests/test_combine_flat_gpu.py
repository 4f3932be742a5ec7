"""k_attn_decode_combine_flat against k_attn_decode_combine: bit-equal output
at every instantiated split count, on partials shaped like the ones the
attention kernels write (empty splits, underflowing weights), plus the
fallback for a count with no instance and one fp32 reference of the formula."""

import pytest
import torch

from fei_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FLAT_SPLITS = (16, 32)                # instances of the flat kernel
# no instance: both switches run the loop kernel, so these are held to the
# fp32 reference as well
OTHER_SPLITS = (3, 4, 8, 33, 64)
KINDS = ("plain", "some_empty", "only_first", "all_empty", "underflow")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ops.require_lib()


def _partials(kind, B, Hq, S, D, seed):
    """part_o [B,Hq,S,D], part_ml [B,Hq,S,2] on the CPU. An empty split is
    (m, l, o) = (-inf, 0, 0), as k_attn_decode writes it."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(B, Hq, S, generator=g) * 3.0
    l = torch.rand(B, Hq, S, generator=g) * 50.0 + 0.5
    o = torch.randn(B, Hq, S, D, generator=g) * l[..., None]
    if kind == "underflow":
        # exp(m_s - m*) is 0 in f32 below about -104: spread m over +-150
        m = (torch.rand(B, Hq, S, generator=g) - 0.5) * 300.0
    empty = torch.zeros(B, Hq, S, dtype=torch.bool)
    if kind == "some_empty":
        empty = torch.rand(B, Hq, S, generator=g) < 0.4
        empty[..., S - 1] = True                  # the tail split, always
    elif kind == "only_first":
        empty[..., 1:] = True
    elif kind == "all_empty":
        empty[:] = True
    m = m.masked_fill(empty, float("-inf"))
    l = l.masked_fill(empty, 0.0)
    o = o.masked_fill(empty[..., None], 0.0)
    return o.contiguous(), torch.stack([m, l], dim=-1).contiguous()


def _reference(part_o, part_ml):
    """fp32 torch: sum_s exp(m_s-m*) o_s / sum_s exp(m_s-m*) l_s, 0 where the
    denominator is 0."""
    m, l = part_ml[..., 0], part_ml[..., 1]
    mstar = m.max(dim=-1, keepdim=True).values
    w = torch.exp(m - mstar)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)   # -inf - -inf
    den = (w * l).sum(-1)
    num = (w[..., None] * part_o).sum(-2)
    return torch.where(den[..., None] > 0, num / den[..., None],
                       torch.zeros_like(num))


def _both(part_o, part_ml):
    po, pml = part_o.to(DEV), part_ml.to(DEV)
    new = ops.attn_decode_combine(po, pml, flat=True)
    old = ops.attn_decode_combine(po, pml, flat=False)
    torch.cuda.synchronize()
    return new.cpu(), old.cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", FLAT_SPLITS + OTHER_SPLITS)
@pytest.mark.parametrize("D", (64, 128))
def test_flat_combine_equals_loop_combine(D, S, kind):
    for B in (1, 3):
        for Hq in (1, 4):
            part_o, part_ml = _partials(kind, B, Hq, S, D,
                                        seed=1000 * S + 10 * B + Hq)
            new, old = _both(part_o, part_ml)
            assert torch.equal(new.view(torch.int16), old.view(torch.int16)), \
                f"B{B} Hq{Hq} D{D} S{S} {kind}: " \
                f"{(new.float() - old.float()).abs().max().item()}"
            if kind == "all_empty":
                assert torch.equal(new, torch.zeros_like(new))
            else:
                assert torch.isfinite(new.float()).all()
            if S in OTHER_SPLITS:
                # equal by construction here: what is checked is that the
                # dispatch lands on a kernel that computes this count
                err = (new.float() - _reference(part_o, part_ml)).abs().max()
                assert err.item() < 2e-2, f"B{B} Hq{Hq} D{D} S{S} {kind}"


@pytest.mark.parametrize("kind", ("plain", "some_empty", "underflow"))
@pytest.mark.parametrize("S,D", [(32, 128), (16, 64), (32, 64), (16, 128)])
def test_flat_combine_against_fp32_reference(S, D, kind):
    """Bound 2e-2 absolute, the decode-attention tests' own (test_ops_gpu.py
    test_attn_decode): the output is a weighted mean of o_s / l_s rows drawn
    from N(0, 1), so it stays within a few units, where bf16 rounds to 2^-7
    at the worst."""
    part_o, part_ml = _partials(kind, 3, 4, S, D, seed=77 + S + D)
    new, _ = _both(part_o, part_ml)
    err = (new.float() - _reference(part_o, part_ml)).abs().max().item()
    assert err < 2e-2, f"max err {err}"


def test_default_follows_the_module_flag():
    """flat=None follows the module flag, which FEI_CMB_FLAT=0 clears."""
    part_o, part_ml = _partials("plain", 1, 4, 32, 128, seed=5)
    po, pml = part_o.to(DEV), part_ml.to(DEV)
    want = ops.attn_decode_combine(po, pml, flat=False)
    for flag in (True, False):
        saved = ops._CMB_FLAT
        ops._CMB_FLAT = flag
        try:
            got = ops.attn_decode_combine(po, pml)
        finally:
            ops._CMB_FLAT = saved
        assert torch.equal(got, want)
