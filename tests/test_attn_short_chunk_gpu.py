"""Decode attention's one-pass path for split chunks under 64 keys
(attn_short_chunk in fei_kernels.hip), at the boundaries of its lane map
that test_decode_shapes_gpu.py does not hit. A K or V row is covered by
D/8 adjacent lanes and lane-group kg owns keys kg, kg + kgroups, ... of the
chunk (kgroups = 16 at D=128, 32 at D=64). Same fp64 reference, bounds,
NaN-poisoned tails and in-place row checks as the shape tests
(decode_shape_cases.py)."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_shape_cases as C  # noqa: E402

from fei_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = ["plain", "cmb", "rope"]

# (splits, n) -> chunk
LANE_MAP = [
    (32, 512),    # 16: one key per lane-group at D=128
    (32, 513),    # 17: one group with two keys; split 30 short, 31 empty
    (32, 545),    # 18: the benchmark's first timed shape
    (32, 800),    # 25: the benchmark's last timed shape
    (16, 528),    # 33: 16-key round over at D=128, 32-key at D=64
]
SWITCH = [
    (16, 1008),   # 63: last short chunk
    (16, 1009),   # 64: first chunk on the tiled path
]
NEW_KEY = [
    (8, 9),       # 2: new key is the only key of split 4; 5-7 empty
    (2, 3),       # 2: new key is the only key of the last split
    (32, 33),     # 2: the same at 32 splits
]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    ops.require_lib()


@pytest.mark.parametrize("splits,n", LANE_MAP + SWITCH + NEW_KEY)
@pytest.mark.parametrize("G,D", C.GD_PAIRS)
def test_short_chunk_forms(G, D, splits, n):
    C.run_split_case(G, D, splits, n, DEV, forms=FORMS)


@pytest.mark.parametrize("G,D", [(4, 128), (8, 64)])
def test_short_chunk_repeatable(G, D):
    """No atomics and a fixed reduction order: the same RoPE-fused call on
    fresh caches gives the same bits, output and caches."""
    splits, n = 32, 545
    case = C.AttnCase(G, D, splits, C._lens(n, splits))
    table = C.rope_tab(D).to(DEV)
    pos = case.pos.to(DEV)
    idx = torch.arange(C.B, device=DEV)
    runs = []
    for _ in range(2):
        Kd, Vd = case.caches(DEV, hole=True)
        out = ops.attn_decode(C.put(case.q_raw, DEV), Kd, Vd, pos,
                              k=C.put(case.kin, DEV), v=C.put(case.vin, DEV),
                              table=table, splits=splits, scale=case.scale)
        rows = [t[idx, :, pos.long()] for t in (Kd, Vd)]
        runs.append([C.bits(t).cpu() for t in [out] + rows])
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)
