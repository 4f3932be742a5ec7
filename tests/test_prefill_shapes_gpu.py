"""The prefill path on the GPU at every tile, mask and stride edge: the MFMA
attention kernels k_attn_prefill<64|128> and k_attn_prefill_kv8<64|128>
(G 1/2/4/8 and 3, per-sequence pos0, contiguous q and the engine's strided
qkv view, bf16 and fp8 caches, bidirectional form), k_rope_kv_prefill, and
the row-wise / element-wise kernels at their loop edges. fp64 CPU reference,
per-element bounds, planted diagonal keys and NaN canaries — tables,
references and bounds live in prefill_shape_cases.py and are proven against
the fp32 reference and a model of the kernel in test_prefill_shapes_cpu.py."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_shape_cases as P  # noqa: E402

from fei_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ops.require_lib()


@pytest.mark.parametrize("S,pos0", P.CAUSAL_CASES)
@pytest.mark.parametrize("G,D", P.GD_PAIRS)
def test_attn_prefill_causal(G, D, S, pos0):
    """bf16 and QuantKV caches x contiguous q and the fused-qkv view; the
    diagonal each (S, pos0) pair reaches is noted in CAUSAL_CASES."""
    P.run_causal_case(G, D, S, pos0, DEV)


@pytest.mark.parametrize("G,D", P.G3_PAIRS)
def test_attn_prefill_group3(G, D):
    """Hq = 6, Hkv = 2: prefill is not templated on the group size."""
    P.run_causal_case(G, D, 65, (64, 15), DEV, hq=6)


@pytest.mark.parametrize("S,kv_len", P.BIDIR_CASES)
@pytest.mark.parametrize("G,D", P.GD_PAIRS)
def test_attn_prefill_bidirectional(G, D, S, kv_len):
    """kv_len per sequence, pos0 ignored, kv_len = 0 gives exact zeros."""
    P.run_bidir_case(G, D, S, kv_len, DEV)


@pytest.mark.parametrize("layout", ["contig", "fused"])
@pytest.mark.parametrize("D,hq,hkv,S,pos0", P.ROPE_CASES)
def test_rope_kv_prefill(D, hq, hkv, S, pos0, layout):
    P.run_rope_case(D, hq, hkv, S, pos0, layout, DEV)


@pytest.mark.parametrize("rows,cols", P.ROW_SHAPES)
def test_rmsnorm_shapes(rows, cols):
    P.run_rmsnorm_case(rows, cols, DEV)


@pytest.mark.parametrize("rows,cols", P.ROW_SHAPES)
def test_fused_add_rmsnorm_shapes(rows, cols):
    P.run_add_rmsnorm_case(rows, cols, DEV)


@pytest.mark.parametrize("kind", P.LN_KINDS)
@pytest.mark.parametrize("rows,cols", P.ROW_SHAPES)
def test_layernorm_shapes(rows, cols, kind):
    P.run_layernorm_case(rows, cols, kind, DEV)


@pytest.mark.parametrize("rows,inter", P.ELT_SHAPES)
def test_swiglu_shapes(rows, inter):
    P.run_swiglu_case(rows, inter, DEV)


@pytest.mark.parametrize("rows,cols", P.ELT_SHAPES)
def test_gelu_shapes(rows, cols):
    P.run_gelu_case(rows, cols, DEV)


def test_wrappers_refuse_unsupported_shapes():
    """ValueError before any launch: Hq % Hkv != 0 (hkv would reach Hkv),
    D = 32 with bf16 caches (the C entry point launches nothing and the
    output was uninitialised memory), a last dimension or element count that
    is no multiple of 8 (the tail stayed unwritten), a strided residual."""
    for name, call in P.refusals(DEV) + P.gpu_refusals(DEV):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{name}: not refused")
    torch.cuda.synchronize()


def test_zero_rows_launch_nothing():
    P.run_empties(DEV)
    torch.cuda.synchronize()
