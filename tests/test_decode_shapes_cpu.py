"""CPU self-check of the decode shape tests: the same case tables and the
same checking helpers as test_decode_shapes_gpu.py / test_gemv_shapes_gpu.py,
run with CPU tensors, where fei_amd.ops dispatches to the fp32 torch
reference. Passing here proves that a correct fp32 implementation meets
every per-element bound the GPU tests apply (docs/TESTING.md), that every
case satisfies the conditions the bounds were derived under (n <= 1024,
|score| <= 64) and that the near-tie caps hold for the committed seeds."""

import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_shape_cases as C  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("G,D", C.GD_PAIRS)
def test_attn_split_forms_cpu(G, D):
    for splits, n in C.SPLIT_CASES:
        C.run_split_case(G, D, splits, n, DEV)
    for splits, n in C.ROPE_EXTRA:
        C.run_split_case(G, D, splits, n, DEV,
                         forms=["rope"] + [f"paged{bs}rope" for bs in C.PAGED_BS])


@pytest.mark.parametrize("G,D", C.GD_PAIRS)
def test_attn_decode_fused_shapes_cpu(G, D):
    for n in C.FUSED_N:
        C.run_fused_case(G, D, n, DEV)


def test_planted_keys_cover_boundaries():
    """The planted positions really are the boundary keys."""
    assert C.planted(260, 4) == [0, 64, 65, 129, 130, 194, 195, 259]
    assert C.planted(257, 1) == [0, 255, 256]
    assert C.planted(13, 4) == [0, 3, 4, 7, 8, 11, 12]
    assert C.planted(962, 32)[-2:] == [960, 961]      # split 31 = {961}
    assert C.planted(1, 64) == [0]
    for splits, n in C.SPLIT_CASES + C.ROPE_EXTRA:
        lens = C._lens(n, splits)
        assert len(set(lens)) == 3 and max(lens) <= C.MS
        wide = [-(-m // splits) >= 64 for m in lens[:2]]
        if splits <= 4:
            assert wide[0] != wide[1], "sequence 1 must take the other map"


def test_samplers_cpu():
    for Bn in (9, 16, 3):
        for V in (64 * 37, 4099, 40):
            C.run_sample_case(Bn, V, DEV, step_val=1)
            C.run_sample_case(Bn, V, DEV, step_val=4)
    C.run_sample_shard_case(3, 4099, 1000, DEV)
    C.run_advance_case(DEV)


@pytest.mark.parametrize("op", C.BF16_OPS + C.FP8_OPS)
def test_gemv_bounds_cpu(op):
    fp8 = op.endswith("fp8")
    swi = op.startswith("swiglu")
    for M in C.GEMV_M + (3,):
        for N in (C.SWIGLU_I if swi else C.GEMV_N):
            for K in (C.K_FP8 if fp8 else C.K_BF16):
                C.run_gemv_case(op, M, N, K, DEV)
        C.run_gemv_case(op, M, 7 if swi else 9, 1040 if fp8 else 520, DEV,
                        ramp=True)
    if fp8:
        C.run_gemv_case(op, 8, 5 if swi else 9, 4096, DEV)
        C.run_gemv_case(op, 1, 5 if swi else 9, 72, DEV)


def test_gemm_m8_bounds_cpu():
    for op in ("linear", "swiglu"):
        for M in (4, 5, 6, 7, 8):
            for N in (16, 48):
                for K in (1024, 2048):
                    C.run_mfma_case(op, M, N, K, DEV)


def test_quant_fp8_cpu():
    C.run_quant_case(2050, 24, DEV, zero_row=2049)
    C.run_quant_case(3, 520, DEV, zero_row=1)
