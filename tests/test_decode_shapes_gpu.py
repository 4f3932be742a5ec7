"""Decode attention and greedy samplers on the GPU at every dispatched
shape: G = Hq/Hkv in {1,2,4,8} x D in {64,128}, every form (plain,
RoPE-fused, fused combine, paged at three block sizes, one-kernel fused),
at the split / tile / lane-map boundaries. fp64 CPU reference, per-element
bounds — tables, references and bounds live in decode_shape_cases.py and
are proven against the fp32 reference in test_decode_shapes_cpu.py."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_shape_cases as C  # noqa: E402

from fei_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ops.require_lib()


@pytest.mark.parametrize("splits,n", C.SPLIT_CASES)
@pytest.mark.parametrize("G,D", C.GD_PAIRS)
def test_attn_split_forms(G, D, splits, n):
    """plain / fused-combine / RoPE-fused / paged (BS 8,16,64; plain and
    RoPE-fused). splits=64 at D=64 needs the strided m/l staging in
    k_attn_decode_combine: with `if (d < 2*splits)` and D threads, half of
    the 128 staged values were uninitialised LDS."""
    C.run_split_case(G, D, splits, n, DEV)


@pytest.mark.parametrize("splits,n", C.ROPE_EXTRA)
@pytest.mark.parametrize("G,D", C.GD_PAIRS)
def test_attn_rope_new_key_edges(G, D, splits, n):
    """New key = only key of the last split / first key of a tile."""
    C.run_split_case(G, D, splits, n, DEV,
                     forms=["rope"] + [f"paged{bs}rope" for bs in C.PAGED_BS])


@pytest.mark.parametrize("n", C.FUSED_N)
@pytest.mark.parametrize("G,D", C.GD_PAIRS)
def test_attn_decode_fused_shapes(G, D, n):
    C.run_fused_case(G, D, n, DEV)


def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16, device=DEV)


def test_attn_refuses_unsupported_group():
    """Hq/Hkv = 3 has no kernel instance: every wrapper raises before any
    launch (the C dispatch would launch nothing and return torch.empty)."""
    Bq, Hq, Hkv, D = 1, 6, 2, 64
    q, k, v = _bf(Bq, Hq, D), _bf(Bq, Hkv, D), _bf(Bq, Hkv, D)
    kc, vc = _bf(Bq, Hkv, 16, D), _bf(Bq, Hkv, 16, D)
    pos = torch.zeros(Bq, dtype=torch.int32, device=DEV)
    table = C.rope_tab(D).to(DEV)
    with pytest.raises(ValueError):
        ops.attn_decode(q, kc, vc, pos, splits=1)
    with pytest.raises(ValueError):
        ops.attn_decode_fused(q, k, v, kc, vc, pos, table)
    bt = torch.zeros(Bq, 1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.attn_decode_paged(q, _bf(2, Hkv, 16, D), _bf(2, Hkv, 16, D), bt,
                              pos, splits=1)
    with pytest.raises(ValueError):       # Hq % Hkv != 0
        ops.attn_decode(_bf(Bq, 5, D), kc, vc, pos, splits=1)


def test_attn_decode_fused_refuses_small_head():
    """D=32 would index past the kernel's osh[8][64][2]; never launched."""
    Bq, Hq, Hkv, D = 1, 4, 2, 32
    pos = torch.zeros(Bq, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.attn_decode_fused(_bf(Bq, Hq, D), _bf(Bq, Hkv, D), _bf(Bq, Hkv, D),
                              _bf(Bq, Hkv, 16, D), _bf(Bq, Hkv, 16, D), pos,
                              C.rope_tab(64).to(DEV))


# -- samplers -----------------------------------------------------------------

@pytest.mark.parametrize("V", [64 * 37, 4099, 40])
@pytest.mark.parametrize("Bn", [9, 16])
def test_sample_two_stage_greedy(Bn, V):
    """B > 8: k_sample_partial + k_sample_final against the known argmax
    (last element, element 0, exact tie -> lowest index; V=40 < nchunks)."""
    C.run_sample_case(Bn, V, DEV, step_val=1)
    C.run_sample_case(Bn, V, DEV, step_val=4)       # step >= max_new


@pytest.mark.parametrize("V", [4099, 40])
def test_sample_onepass_tail_greedy(V):
    """B <= 8 one-pass kernel; V % 8 != 0 puts the maximum in the tail."""
    C.run_sample_case(3, V, DEV, step_val=0)
    C.run_sample_case(3, V, DEV, step_val=9)


def test_sample_shard_offset_greedy():
    C.run_sample_shard_case(3, 4099, 1000, DEV)


def test_advance_clamps_at_max_pos():
    C.run_advance_case(DEV)
