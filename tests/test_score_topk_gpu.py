"""ops.score_topk on the GPU: the shared case table bit for bit against the
reference at every grid size, the kernel's refusal codes, and the scoped /
batched index equal to the same index on the CPU."""

import pytest
import torch

import score_topk_cases as cases
from fei_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _to_dev(c):
    """emb and mask keep their poisoned tails on the device: the views are
    cut from the copied larger buffers."""
    emb, mask = c["emb"], c["mask"]
    N = emb.shape[0]
    emb_d = emb._base.to(DEV)[:N] if emb._base is not None else emb.to(DEV)
    mask_d = None
    if mask is not None:
        mask_d = mask._base.to(DEV)[:N]
    return emb_d, c["q"].to(DEV), mask_d


@pytest.mark.parametrize("spec", cases.SPECS, ids=cases.spec_id)
def test_case_table(spec):
    c = cases.case(spec)
    emb, q, mask = _to_dev(c)
    assert emb.shape[0] == spec[0] and emb.is_contiguous()
    for wg in cases.WORKGROUPS:
        got = ops.score_topk(emb, q, c["k"], mask, workgroups=wg)
        cases.assert_bit_equal(got, c["want"], f"{c['name']} workgroups={wg}")
    s1, i1 = ops.score_topk(emb, q[0], c["k"], mask)
    assert s1.shape == i1.shape == (c["k"],)
    assert torch.equal(i1.cpu(), c["want"][1][0])


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_normal_corpus(dtype):
    c = cases.normal_case(dtype)
    for wg in (None, 7):
        got = ops.score_topk(c["emb"].to(DEV), c["q"].to(DEV), c["k"],
                             c["mask"].to(DEV), workgroups=wg)
        cases.check_normal(c, got)


def test_kernel_refusal_codes():
    """The C entry point refuses bad arguments itself: a negative code,
    nothing launched, the outputs untouched."""
    lib = ops.require_lib()
    N, C, Q, k, WG = 64, 16, 2, 4, 2
    emb = torch.zeros(N, C, device=DEV)
    q = torch.zeros(Q, C, device=DEV)
    part_s = torch.full((Q, WG, k), 7.0, device=DEV)
    part_i = torch.full((Q, WG, k), 7, dtype=torch.int32, device=DEV)
    out_s = torch.full((Q, k), 7.0, device=DEV)
    out_i = torch.full((Q, k), 7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(emb_p=emb.data_ptr(), q_p=q.data_ptr(), N=N, C=C, Q=Q, k=k,
             WG=WG):
        return lib.fei_score_topk(emb_p, q_p, None, part_s.data_ptr(),
                                  part_i.data_ptr(), out_s.data_ptr(),
                                  out_i.data_ptr(), N, C, Q, k, WG, 0, 0,
                                  stream)

    assert call(emb_p=None) == -1
    assert call(k=0) == -2 and call(k=65) == -2
    assert call(Q=0) == -3 and call(Q=9) == -3
    assert call(C=12) == -4 and call(C=2056) == -4 and call(C=0) == -4
    assert call(N=0) == -5
    assert call(WG=0) == -6 and call(WG=N + 1) == -6
    assert call(emb_p=emb.data_ptr() + 4) == -7
    assert call(q_p=q.data_ptr() + 8) == -7
    torch.cuda.synchronize()
    for t in (part_s, part_i, out_s, out_i):
        assert (t == 7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert out_i.tolist() == [[0, 1, 2, 3]] * 2 and not out_s.any()


def test_wrapper_refuses_before_launch():
    emb = torch.zeros(10, 12, device=DEV)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.score_topk(emb, torch.zeros(12, device=DEV), 3)
    with pytest.raises(ValueError, match="lives on"):
        ops.score_topk(torch.zeros(10, 16, device=DEV), torch.zeros(16), 3)
    with pytest.raises(ValueError, match="mask lives on"):
        ops.score_topk(torch.zeros(10, 16, device=DEV),
                       torch.zeros(16, device=DEV), 3,
                       torch.ones(10, dtype=torch.uint8))


# -- the index on the device, equal to the same index on the CPU -------------------

@pytest.fixture
def scoped_base(memdir_base):
    cases.build_scoped_memdir(memdir_base)
    return memdir_base


def test_index_scoping(scoped_base):
    cases.check_scoping(cases.scoped_index(scoped_base, DEV))


def test_index_batching(scoped_base):
    cases.check_batching(cases.scoped_index(scoped_base, DEV))


def test_index_mutation(scoped_base):
    cases.check_mutation(cases.scoped_index(scoped_base, DEV))


def test_index_f16_scan(scoped_base):
    cases.check_f16_scan(scoped_base, DEV)


def test_index_equals_cpu_index(scoped_base):
    gpu = cases.scoped_index(scoped_base, DEV)
    cpu = cases.scoped_index(scoped_base, "cpu")
    assert gpu.ids == cpu.ids
    assert gpu.folder_codes.is_cuda and gpu.status_codes.is_cuda
    queries = ["q0", "q1", "q01", "other"]
    for scope in ({}, {"folders": [".Projects/x"]}, {"statuses": ["new"]},
                  {"folders": ["", ".Projects/y"], "statuses": ["cur"]},
                  {"folders": [".Projects/none"]}):
        for topk in (1, 5, 64):
            assert gpu.search_many(queries, topk, **scope) == \
                cpu.search_many(queries, topk, **scope)
    assert gpu._scope_mask([".Projects/x"], None).is_cuda
