"""Decode GEMV family on the GPU at every template instance: M in
{1,2,4,8} on the VALU kernels (shapes chosen so the MFMA tile is NOT
taken), odd N / N < one block, K tails (K/8 and K/16 not a multiple of 64,
and below 64), the MFMA tile at M in 4..8, the fp8 GEMVs up to the 64 KB
LDS limit, and quant_fp8. fp64 CPU reference and per-element bounds from
decode_shape_cases.py (proven against the fp32 reference in
test_decode_shapes_cpu.py)."""

import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_shape_cases as C  # noqa: E402

from fei_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ops.require_lib()


@pytest.mark.parametrize("M", C.GEMV_M)
@pytest.mark.parametrize("op", C.BF16_OPS)
def test_gemv_bf16_shapes(op, M):
    """k_gemv / k_gemv_swiglu / k_gemv_res / k_gemv_norm /
    k_gemv_swiglu_norm <M>: run_gemv_case asserts _gemm_m8_ok is False, so
    M=4 and M=8 reach the VALU kernels too."""
    for N in (C.SWIGLU_I if op.startswith("swiglu") else C.GEMV_N):
        for K in C.K_BF16:
            C.run_gemv_case(op, M, N, K, DEV)
    C.run_gemv_case(op, M, 9 if not op.startswith("swiglu") else 7, 520, DEV,
                    ramp=True)


@pytest.mark.parametrize("M", C.GEMV_M)
@pytest.mark.parametrize("op", C.FP8_OPS)
def test_gemv_fp8_shapes(op, M):
    for N in (C.SWIGLU_I if op.startswith("swiglu") else C.GEMV_N):
        for K in C.K_FP8:
            C.run_gemv_case(op, M, N, K, DEV)
    C.run_gemv_case(op, M, 9 if not op.startswith("swiglu") else 7, 1040, DEV,
                    ramp=True)


@pytest.mark.parametrize("op", C.FP8_OPS)
def test_gemv_fp8_lds_limit(op):
    """M=8, K=4096: M*K*2 = 64 KB, exactly the dynamic-LDS limit the
    wrappers assert."""
    C.run_gemv_case(op, 8, 9 if op != "swiglu_norm_fp8" else 5, 4096, DEV)


@pytest.mark.parametrize("M,K", [(3, 64), (1, 72), (3, 72)])
@pytest.mark.parametrize("op", C.FP8_OPS)
def test_gemv_fp8_unsupported_shapes_fall_back(op, M, K):
    """M not in {1,2,4,8} has no kernel instance and K % 16 != 0 would lose
    the last 8 columns: the wrappers take the dequantise + linear path and
    still meet the fp64 bound."""
    assert not ops._gemv_fp8_ok(M, K)
    C.run_gemv_case(op, M, 9 if op != "swiglu_norm_fp8" else 5, K, DEV)


@pytest.mark.parametrize("K", [1024, 2048])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("M", [4, 5, 6, 7, 8])
@pytest.mark.parametrize("op", ["linear", "swiglu"])
def test_gemm_m8_tile(op, M, N, K):
    """k_gemm_m8 (arow = min(l15, M-1) for M in 5..7): distinct x rows and
    a sentinel-filled output with guard rows."""
    C.run_mfma_case(op, M, N, K, DEV)


@pytest.mark.parametrize("N,K,zero_row", [(2050, 24, 2049), (3, 520, 1)])
def test_quant_fp8_shapes(N, K, zero_row):
    """N=2050 reaches the grid-stride loop past 2048 blocks with K <
    blockDim; scales bit-equal to amax/448, codes equal to the torch e4m3fn
    cast except within 2^-20 of a rounding boundary."""
    C.run_quant_case(N, K, DEV, zero_row=zero_row)
