"""ops.score_topk on the CPU (reference dispatch, argument checks) and the
scoped / batched EmbeddingIndex, tool and CLI built on it."""

import json

import pytest
import torch

import score_topk_cases as cases
from fei_amd import ops
from fei_amd.ops import reference as ref


# -- the reference against a brute-force loop ----------------------------------

def _brute(emb, q, k, mask):
    N, Q = emb.shape[0], q.shape[0]
    e = emb.float()
    out_s = torch.full((Q, k), float("-inf"))
    out_i = torch.full((Q, k), -1, dtype=torch.int32)
    for u in range(Q):
        cand = []
        for r in range(N):
            if mask is not None and mask[r] == 0:
                continue
            s = float(e[r] @ q[u])
            if s != s:
                s = float("-inf")
            cand.append((-s, r))
        cand.sort()                                # score desc, then row asc
        for j, (ns, r) in enumerate(cand[:k]):
            out_s[u, j] = -ns
            out_i[u, j] = r
    return out_s, out_i


SMALL = [s for s in cases.SPECS if s[0] <= 257]


@pytest.mark.parametrize("spec", SMALL, ids=cases.spec_id)
def test_reference_matches_brute_force(spec):
    c = cases.case(spec)
    cases.assert_bit_equal(c["want"], _brute(c["emb"], c["q"], c["k"],
                                             c["mask"]), c["name"])


def test_table_covers_every_listed_value():
    for pos, values in enumerate((cases.NS, cases.CS, cases.KS, cases.QS,
                                  cases.DTYPES, cases.MASKS, cases.CORPORA)):
        assert {s[pos] for s in cases.SPECS} == set(values)
    for N in cases.NS:
        assert {s[5] for s in cases.SPECS if s[0] == N} == set(cases.MASKS)
    assert len(set(cases.SPECS)) == len(cases.SPECS)
    # the table does hold ties: some case returns equal scores on
    # different rows
    assert any((cases.case(s)["want"][0][:, :-1]
                == cases.case(s)["want"][0][:, 1:]).any()
               for s in SMALL if s[2] > 1)


@pytest.mark.parametrize("spec", cases.SPECS[::7], ids=cases.spec_id)
def test_cpu_dispatch_is_the_reference(spec):
    c = cases.case(spec)
    got = ops.score_topk(c["emb"], c["q"], c["k"], c["mask"], workgroups=7)
    cases.assert_bit_equal(got, c["want"], c["name"])
    s1, i1 = ops.score_topk(c["emb"], c["q"][0], c["k"], c["mask"])
    assert s1.shape == i1.shape == (c["k"],)
    cases.assert_bit_equal((s1[None], i1[None]),
                           (c["want"][0][:1], c["want"][1][:1]), c["name"])


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_normal_corpus_reference(dtype):
    c = cases.normal_case(dtype)
    cases.check_normal(c, ref.score_topk(c["emb"], c["q"], c["k"], c["mask"]))


# -- every refusal ---------------------------------------------------------------

def _good():
    return {"emb": torch.zeros(10, 16), "q": torch.zeros(2, 16), "k": 3,
            "mask": torch.ones(10, dtype=torch.uint8), "workgroups": None}


REFUSALS = {
    "emb not 2-d": {"emb": torch.zeros(10)},
    "emb dtype": {"emb": torch.zeros(10, 16, dtype=torch.bfloat16)},
    "emb not a tensor": {"emb": [[0.0] * 16]},
    "q 3-d": {"q": torch.zeros(1, 2, 16)},
    "q dtype": {"q": torch.zeros(2, 16, dtype=torch.float16)},
    "q width": {"q": torch.zeros(2, 8)},
    "k zero": {"k": 0},
    "k 65": {"k": 65},
    "k float": {"k": 3.0},
    "k bool": {"k": True},
    "9 queries": {"q": torch.zeros(9, 16)},
    "no queries": {"q": torch.zeros(0, 16)},
    "C not a multiple of 8": {"emb": torch.zeros(10, 12),
                              "q": torch.zeros(2, 12)},
    "C too wide": {"emb": torch.zeros(10, 2056), "q": torch.zeros(2, 2056)},
    "no rows": {"emb": torch.zeros(0, 16), "mask": None},
    "emb strided": {"emb": torch.zeros(10, 32)[:, :16]},
    "emb transposed": {"emb": torch.zeros(16, 10).t()},
    "emb misaligned": {"emb": torch.zeros(10 * 16 + 1)[1:].view(10, 16)},
    "q strided": {"q": torch.zeros(2, 32)[:, :16]},
    "q misaligned": {"q": torch.zeros(2 * 16 + 1)[1:].view(2, 16)},
    "mask dtype": {"mask": torch.ones(10, dtype=torch.bool)},
    "mask length": {"mask": torch.ones(11, dtype=torch.uint8)},
    "mask 2-d": {"mask": torch.ones(10, 1, dtype=torch.uint8)},
    "mask strided": {"mask": torch.ones(20, dtype=torch.uint8)[::2]},
    "workgroups zero": {"workgroups": 0},
    "workgroups float": {"workgroups": 2.0},
    "workgroups huge": {"workgroups": 1 << 20},
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals(what):
    args = {**_good(), **REFUSALS[what]}
    with pytest.raises(ValueError, match="score_topk"):
        ops.score_topk(args["emb"], args["q"], args["k"], args["mask"],
                       workgroups=args["workgroups"])


def test_good_arguments_pass():
    a = _good()
    s, i = ops.score_topk(a["emb"], a["q"], a["k"], a["mask"])
    assert i.tolist() == [[0, 1, 2], [0, 1, 2]] and not s.any()


# -- the index --------------------------------------------------------------------

@pytest.fixture
def scoped_base(memdir_base):
    cases.build_scoped_memdir(memdir_base)
    return memdir_base


def test_index_scoping(scoped_base):
    cases.check_scoping(cases.scoped_index(scoped_base, "cpu"))


def test_index_batching(scoped_base):
    cases.check_batching(cases.scoped_index(scoped_base, "cpu"))


def test_index_mutation(scoped_base):
    cases.check_mutation(cases.scoped_index(scoped_base, "cpu"))


def test_index_f16_scan(scoped_base):
    cases.check_f16_scan(scoped_base, "cpu")
    from fei_amd.memdir.embed_index import EmbeddingIndex
    with pytest.raises(ValueError):
        EmbeddingIndex(base=scoped_base, scan_dtype="bf16")


def test_index_scope_is_computed_on_the_device_codes(scoped_base):
    """The mask comes from the code tensors, not from a walk over ids."""
    idx = cases.scoped_index(scoped_base, "cpu")
    idx.ids = [k.replace(".Projects/x", ".Projects/renamed") for k in idx.ids]
    assert cases.numbers(idx.search("q0", topk=2,
                                    folders=[".Projects/x"])) == [9, 7]


# -- tool and CLI -------------------------------------------------------------------

@pytest.fixture
def tools(scoped_base):
    from fei_amd.tools.memory_tools import MemoryTools
    t = MemoryTools(base=scoped_base)
    t._index = cases.scoped_index(scoped_base, "cpu")
    return t


def _subjects(results):
    return [m["headers"]["Subject"].split()[0] for m in results]


def test_tool_old_argument_form(tools):
    out = tools.semantic_search({"query": "q0", "topk": 3})
    assert out["count"] == 3
    assert _subjects(out["results"]) == ["s16", "s15", "s14"]
    assert all("score" in m for m in out["results"])
    assert tools.semantic_search({"query": "q0"})["count"] == 10


def test_tool_folder_and_status(tools):
    out = tools.semantic_search({"query": "q0", "topk": 3,
                                 "folder": ".Projects/x"})
    assert _subjects(out["results"]) == ["s9", "s7", "s5"]
    out = tools.semantic_search({"query": "q0", "topk": 3,
                                 "folder": ".Projects/x", "status": "new"})
    assert _subjects(out["results"]) == ["s7", "s2"] and out["count"] == 2
    out = tools.semantic_search({"query": "q0", "topk": 2, "folder": ""})
    assert _subjects(out["results"]) == ["s16", "s15"]
    out = tools.semantic_search({"query": "q0", "status": "tmp"})
    assert out == {"count": 0, "results": []}


def test_tool_queries(tools):
    out = tools.semantic_search({"queries": ["q0", "q1"], "topk": 2,
                                 "folder": ".Projects/x"})
    assert out["queries"] == ["q0", "q1"]
    assert [_subjects(r) for r in out["results"]] == [["s9", "s7"],
                                                      ["s1", "s2"]]
    assert out["count"] == 4
    assert "error" in tools.semantic_search({"topk": 2})


def test_tool_schema_and_recall(scoped_base, tools):
    from fei_amd.tools.memory_tools import (MEMORY_SEMANTIC_SEARCH_TOOL,
                                            MemoryManager)
    props = MEMORY_SEMANTIC_SEARCH_TOOL["input_schema"]["properties"]
    assert {"query", "queries", "topk", "folder", "status"} <= set(props)
    mgr = MemoryManager(base=scoped_base)
    mgr.tools = tools
    got = mgr.recall("q0", semantic=True, topk=2, folder=".Projects/x",
                     status="cur")
    assert _subjects(got) == ["s9", "s5"]
    assert _subjects(mgr.recall("q0", semantic=True, topk=1)) == ["s16"]


def test_cli_semantic_search(scoped_base, capsys):
    """memdir search --semantic (the real encoder on the CPU: ranks are not
    under control, the scope is)."""
    from fei_amd.memdir.cli import main
    assert main(["--base", scoped_base, "index", "--semantic"]) == 0
    assert f"indexed {len(cases.SCOPED_MEMORIES)}" in capsys.readouterr().out
    assert main(["--base", scoped_base, "search", "--semantic", "--format",
                 "json", "--folder", ".Projects/x", "--status", "cur",
                 "project", "notes"]) == 0
    got = json.loads(capsys.readouterr().out)
    assert len(got) == 4
    assert {(m["folder"], m["status"]) for m in got} == {(".Projects/x",
                                                          "cur")}
    assert main(["--base", scoped_base, "search", "--semantic", "--format",
                 "json", "--topk", "3", "anything"]) == 0
    assert len(json.loads(capsys.readouterr().out)) == 3
