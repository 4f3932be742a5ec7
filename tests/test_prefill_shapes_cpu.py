"""CPU self-check of the prefill shape tests: the tables and checkers of
test_prefill_shapes_gpu.py run on CPU tensors, where fei_amd.ops dispatches
to the fp32 torch reference. Passing here proves that a correct fp32
implementation meets every bound applied on the GPU (docs/TESTING.md), that
every case satisfies the conditions its bound assumes (|score| <= 64,
kv_end <= 1024, the near-tie cap) and — through a torch model of the MFMA
kernel's arithmetic (64-key tiles, online softmax, P rounded to bf16) — that
the P-rounding term 2^-8 A_d is right (2^-9 is not). The mutants of that
model show the checker catches what a flat 2e-2 tolerance on random inputs
cannot."""

import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_shape_cases as P  # noqa: E402

DEV = "cpu"


@pytest.mark.parametrize("G,D", P.GD_PAIRS)
def test_attn_prefill_causal_cpu(G, D):
    for S, pos0 in P.CAUSAL_CASES:
        P.run_causal_case(G, D, S, pos0, DEV)


@pytest.mark.parametrize("G,D", P.G3_PAIRS)
def test_attn_prefill_group3_cpu(G, D):
    P.run_causal_case(G, D, 65, (64, 15), DEV, hq=6)


@pytest.mark.parametrize("G,D", P.GD_PAIRS)
def test_attn_prefill_bidir_cpu(G, D):
    for S, kv in P.BIDIR_CASES:
        P.run_bidir_case(G, D, S, kv, DEV)


@pytest.mark.parametrize("G,D", P.GD_PAIRS + P.G3_PAIRS)
def test_kernel_model_meets_the_bound(G, D):
    """64-key tiles, f32 online softmax, P rounded to bf16 per tile, f32 PV,
    bf16 output — on both cache kinds, causal and bidirectional."""
    hq = 6 if G == 3 else P.HQ
    for S, pos0 in P.CAUSAL_CASES:
        for rnd in range(P.AttnCase.rounds(S, pos0)):
            case = P.AttnCase(G, D, S, pos0, rnd, hq=hq)
            P.check_model(case, "bf16")
            P.check_model(case, "kv8")
    if G != 3:
        for S, kv in P.BIDIR_CASES:
            for rnd in range(P.AttnCase.rounds(S, P.BIDIR_POS0, kv)):
                P.check_model(P.AttnCase(G, D, S, P.BIDIR_POS0, rnd, kv_len=kv))


def _all_cases(D):
    for G in (2, 4, 1, 8):
        for S, pos0 in P.CAUSAL_CASES:
            for rnd in range(P.AttnCase.rounds(S, pos0)):
                yield P.AttnCase(G, D, S, pos0, rnd)
        for S, kv in P.BIDIR_CASES:
            for rnd in range(P.AttnCase.rounds(S, P.BIDIR_POS0, kv)):
                yield P.AttnCase(G, D, S, P.BIDIR_POS0, rnd, kv_len=kv)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("mut", P.MUTANTS)
def test_checker_catches_mutant(mut, D):
    """Each deliberate defect of the model fails at least one table case."""
    for case in _all_cases(D):
        try:
            P.check_model(case, "bf16", mut)
        except AssertionError:
            return
    pytest.fail(f"mutant {mut} passed every case at D={D}")


def test_planted_keys_cover_the_edges():
    """The table reaches the diagonals it claims, every chosen row follows
    each of its targets in some round, and every tile-edge key is followed
    by a row that may see it."""
    first_last = lambda S: [s for s in range(S) if s % 16 in (0, 15)]  # noqa: E731
    diag = {(p0 + s) for S, pos0 in P.CAUSAL_CASES for p0 in pos0
            for s in first_last(S)}
    assert {15, 16, 17, 31, 32, 63, 64, 65, 127, 128} <= diag
    assert any(p0 + S == P.MS for S, pos0 in P.CAUSAL_CASES for p0 in pos0)
    assert {S for S, _ in P.CAUSAL_CASES} == \
        {1, 3, 4, 5, 15, 16, 17, 33, 63, 64, 65, 129}
    assert P.chosen_rows(17, 15) == [0, 1, 4, 5, 6, 7, 15, 16]
    assert P.edge_keys(130) == [0, 63, 64, 127, 128]
    for S, pos0 in P.CAUSAL_CASES:
        assert pos0[0] != pos0[1] and max(pos0) + S <= P.MS
        seen = [set(), set()]
        for rnd in range(P.AttnCase.rounds(S, pos0)):
            case = P.AttnCase(2, 64, S, pos0, rnd)
            for b in range(P.B):
                seen[b] |= case.followed[b]
        for b in range(P.B):
            for s in P.chosen_rows(S, pos0[b]):
                for t in P.causal_targets(S, pos0[b], s):
                    assert (s, t) in seen[b], (S, pos0, b, s, t)
            keys = {k for _, t in seen[b] for k in t}
            assert set(P.edge_keys(pos0[b] + S - 1)) <= keys
    for S, kv in P.BIDIR_CASES:
        assert all(P.BIDIR_POS0[b] not in (0, kv[b]) for b in range(P.B))
        seen = [set(), set()]
        for rnd in range(P.AttnCase.rounds(S, P.BIDIR_POS0, kv)):
            case = P.AttnCase(2, 64, S, P.BIDIR_POS0, rnd, kv_len=kv)
            for b in range(P.B):
                seen[b] |= {t for _, t in case.followed[b]}
        for b in range(P.B):
            assert seen[b] == set(P.bidir_targets(kv[b]))


@pytest.mark.parametrize("layout", ["contig", "fused"])
def test_rope_kv_prefill_cpu(layout):
    for D, hq, hkv, S, pos0 in P.ROPE_CASES:
        P.run_rope_case(D, hq, hkv, S, pos0, layout, DEV)


def test_row_kernels_cpu():
    for rows, cols in P.ROW_SHAPES:
        P.run_rmsnorm_case(rows, cols, DEV)
        P.run_add_rmsnorm_case(rows, cols, DEV)
        for kind in P.LN_KINDS:
            P.run_layernorm_case(rows, cols, kind, DEV)


def test_elementwise_kernels_cpu():
    for rows, cols in P.ELT_SHAPES:
        P.run_swiglu_case(rows, cols, DEV)
        P.run_gelu_case(rows, cols, DEV)


def test_wrappers_refuse_before_dispatch():
    """The shape checks sit before the CPU / GPU branch."""
    for name, call in P.refusals(DEV):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{name}: not refused")


def test_zero_rows_cpu():
    P.run_empties(DEV)
