"""Shared case table for ops.score_topk (CPU and GPU tests).

Exact inputs: every element of emb and q is a multiple of 1/8 in [-2, 2], so
products are multiples of 1/64 of magnitude <= 4 and, with C <= 1024, every
partial sum is a multiple of 1/64 below 2^12: 18 significant bits. The f32
score is exact in any summation order and the inputs are exact in f16, so the
criterion is bit equality with reference.score_topk: scores, rows, tie order
and padding.

Every corpus is a view into a larger buffer with NaN rows behind row N, every
mask a view into a longer one whose tail says "eligible", and masked-out rows
hold NaN / Inf: a read past N or of a masked-out row shows up as a NaN.
"""

import zlib

import torch

NS = (1, 3, 63, 257, 4099)
CS = (8, 136, 384, 768, 1024)
KS = (1, 10, 64)
QS = (1, 3, 8)
DTYPES = (torch.float32, torch.float16)
WORKGROUPS = (1, 2, 7, None)
MASKS = ("none", "zero", "single", "half", "last_slab", "few")
CORPORA = ("random", "dup", "equal")


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _eighths(shape, g) -> torch.Tensor:
    return torch.randint(-16, 17, shape, generator=g).float() / 8.0


def make_mask(kind: str, N: int, k: int, g):
    """bool [N] of eligible rows, or None."""
    if kind == "none":
        return None
    el = torch.zeros(N, dtype=torch.bool)
    if kind == "single":
        el[int(torch.randint(0, N, (1,), generator=g))] = True
    elif kind == "half":
        el = torch.rand(N, generator=g) < 0.5
    elif kind == "last_slab":
        el[N - max(1, N // 8):] = True          # inside the last of 7 slabs
    elif kind == "few":
        n = min(k - 1, N)                       # fewer eligible rows than k
        el[torch.randperm(N, generator=g)[:n]] = True
    elif kind != "zero":
        raise ValueError(kind)
    return el


def make_case(N, C, k, Q, dtype, mask_kind, corpus):
    """A dict with emb [N, C] (dtype), q [Q, C] f32, mask u8 [N] or None, k,
    all on the CPU; emb and mask are views into poisoned larger buffers."""
    name = f"N{N}-C{C}-k{k}-Q{Q}-{str(dtype)[6:]}-{mask_kind}-{corpus}"
    g = _gen(zlib.crc32(name.encode()))
    if corpus == "random":
        rows = _eighths((N, C), g)
        # duplicated rows straddling the slab cuts of 2 and 7 workgroups and
        # the wave cuts inside them: exact ties across every boundary
        for cut in sorted({N * a // 28 for a in range(1, 28)}):
            if 1 <= cut < N:
                rows[cut] = rows[cut - 1]
    elif corpus == "dup":
        pool = _eighths((5, C), g)
        rows = pool[torch.randint(0, 5, (N,), generator=g)]
    elif corpus == "equal":
        rows = _eighths((1, C), g).expand(N, C).clone()
    else:
        raise ValueError(corpus)
    q = _eighths((Q, C), g)
    el = make_mask(mask_kind, N, k, g)

    buf = torch.full((N + 3, C), float("nan"))
    buf[:N] = rows
    mask = None
    if el is not None:
        out = torch.nonzero(~el).flatten()
        buf[out[0::2]] = float("nan")
        buf[out[1::2]] = float("inf")
        mbuf = torch.ones(N + 5, dtype=torch.uint8)
        mbuf[:N] = el.to(torch.uint8)
        mask = mbuf[:N]
    emb = buf.to(dtype)[:N]
    return {"name": name, "emb": emb, "q": q, "mask": mask, "k": k}


def _table():
    """Every N with every mask condition, the other parameters cycling so
    that each listed value of C, k, Q, dtype and corpus kind occurs (the CPU
    test asserts the coverage), plus the all-equal corpus and the largest
    shape in both dtypes."""
    specs = []
    i = 0
    for rnd in range(2):
        for N in NS:
            for m in MASKS:
                specs.append((N, CS[(i + rnd) % 5], KS[(i + i // 3) % 3],
                              QS[(i // 2 + rnd) % 3], DTYPES[(i + rnd) % 2],
                              m, CORPORA[0 if i % 4 else 1]))
                i += 1
    for dtype in DTYPES:
        specs.append((257, 136, 10, 3, dtype, "none", "equal"))
        specs.append((4099, 384, 64, 8, dtype, "half", "equal"))
        specs.append((4099, 1024, 64, 8, dtype, "none", "random"))
        specs.append((4099, 768, 64, 1, dtype, "half", "dup"))
        specs.append((63, 8, 64, 8, dtype, "none", "dup"))
    return specs


SPECS = _table()
_CASES = {}


def case(spec):
    """The case of one spec, built once and shared: inputs plus the
    reference result ``want`` = (scores, rows). Callers leave it unchanged."""
    if spec not in _CASES:
        from fei_amd.ops import reference as ref
        c = make_case(*spec)
        c["want"] = ref.score_topk(c["emb"], c["q"], c["k"], c["mask"])
        _CASES[spec] = c
    return _CASES[spec]


def spec_id(spec) -> str:
    N, C, k, Q, dtype, m, corpus = spec
    return f"N{N}-C{C}-k{k}-Q{Q}-{str(dtype)[6:]}-{m}-{corpus}"


def assert_bit_equal(got, want, what: str) -> None:
    gs, gi = got
    ws, wi = want
    assert gs.dtype == torch.float32 and gi.dtype == torch.int32, what
    assert gs.shape == ws.shape and gi.shape == wi.shape, what
    assert not torch.isnan(gs).any(), f"{what}: NaN in the scores"
    assert torch.equal(gi.cpu(), wi), f"{what}: rows differ"
    assert torch.equal(gs.cpu().view(torch.int32), ws.view(torch.int32)), \
        f"{what}: scores differ"


# -- random normal corpus -----------------------------------------------------

NORMAL_N, NORMAL_C, NORMAL_K, NORMAL_Q = 4099, 768, 10, 3


def normal_case(dtype):
    g = _gen(20240 + (dtype == torch.float16))
    emb = torch.randn(NORMAL_N, NORMAL_C, generator=g).to(dtype)
    q = torch.randn(NORMAL_Q, NORMAL_C, generator=g)
    el = torch.rand(NORMAL_N, generator=g) < 0.5
    return {"emb": emb, "q": q, "mask": el.to(torch.uint8), "k": NORMAL_K}


def check_normal(c, got) -> None:
    """Each returned score within B = 2 * C * 2^-24 * sum_i |e_i||q_i| of its
    row's fp64 score (the standard f32 accumulation bound, factor 2), and the
    selection right up to that bound."""
    gs, gi = got[0].cpu().double(), got[1].cpu().long()
    e64, q64 = c["emb"].double(), c["q"].double()
    el = c["mask"] != 0
    k = c["k"]
    for u in range(q64.shape[0]):
        exact = e64 @ q64[u]
        B = 2 * NORMAL_C * 2.0 ** -24 * (e64.abs() @ q64[u].abs())
        rows = gi[u]
        assert (rows >= 0).all() and len(set(rows.tolist())) == k
        assert el[rows].all(), "a masked row was returned"
        err = (gs[u] - exact[rows]).abs()
        assert (err <= B[rows]).all(), f"score error {err.max()}"
        # 2B: a returned row's computed score is at least that of the true
        # k-th best row t, so exact_r + B_r >= exact_t - B_t; an unreturned
        # row's is at most that of the returned row with the lowest exact
        # score, which is <= the k-th best
        elig = torch.nonzero(el).flatten()
        t = elig[torch.sort(exact[elig], descending=True).indices[k - 1]]
        kth = exact[t]
        assert (exact[rows] >= kth - (B[rows] + B[t])).all()
        rest = el.clone()
        rest[rows] = False
        assert (exact[rest] <= kth + B[rest] + B[rows].max()).all()
        assert (gs[u][:-1] >= gs[u][1:]).all(), "not sorted"


# -- index tests: an exact-arithmetic encoder and a tiny scoped memdir ---------

class ExactEncoder:
    """Stands in for the bge encoder with exact arithmetic: a memory whose
    text starts "s<n>" embeds as (n/8, (16-n)/8, 1/8, 0...), the queries
    "q0" / "q1" / "q01" as e0 / e1 / e0+e1, anything else as e2. The score
    of memory n is n/8 under q0, (16-n)/8 under q1 and 2 (a tie between all
    memories) under q01."""

    C = 16

    def __init__(self, device):
        self.device = torch.device(device)
        self.calls = 0

    def encode_texts(self, texts, batch_size=None):
        self.calls += 1
        out = torch.zeros(len(texts), self.C)
        for j, t in enumerate(texts):
            head = t.split()[0] if t.split() else ""
            if head == "q0":
                out[j, 0] = 1.0
            elif head == "q1":
                out[j, 1] = 1.0
            elif head == "q01":
                out[j, 0] = out[j, 1] = 1.0
            elif head[:1] == "s" and head[1:].isdigit():
                n = int(head[1:])
                out[j, 0], out[j, 1], out[j, 2] = n / 8, (16 - n) / 8, 1 / 8
            else:
                out[j, 2] = 1.0
        return out.to(self.device)


# (folder, status, n): the globally best matches of q0 (largest n) sit in the
# root folder, outside the scope ".Projects/x"
SCOPED_MEMORIES = (
    [("", "cur", n) for n in (16, 15, 14, 13, 12, 11)] +
    [(".Projects/x", "cur", n) for n in (5, 3, 9, 1)] +
    [(".Projects/x", "new", n) for n in (7, 2)] +
    [(".Projects/y", "cur", n) for n in (10, 4)])


def build_scoped_memdir(base: str) -> None:
    from fei_amd.memdir import utils as mu
    for folder, status, n in SCOPED_MEMORIES:
        mu.create_memory(folder, {"Subject": f"s{n} memory"}, f"body {n}",
                         base=base, status=status)


def scoped_index(base: str, device, **kw):
    from fei_amd.memdir.embed_index import EmbeddingIndex
    idx = EmbeddingIndex(base=base, encoder=ExactEncoder(device),
                         device=torch.device(device), **kw)
    assert idx.build() == len(SCOPED_MEMORIES)
    return idx


def numbers(hits):
    """The n of each (id, score) hit: q0 scores memory n as n/8."""
    return [round(score * 8) for _, score in hits]


def folder_of(key: str) -> str:
    return key.split("\x00")[0]


def status_of(key: str) -> str:
    return key.split("\x00")[1]


def check_scoping(idx) -> None:
    """Scoped search is the scope's own top-k, not a filtered global one."""
    assert numbers(idx.search("q0", topk=3)) == [16, 15, 14]
    # the 6 best rows are all outside the scope: a global top-3 filtered
    # afterwards would be empty
    hits = idx.search("q0", topk=3, folders=[".Projects/x"])
    assert numbers(hits) == [9, 7, 5]
    assert all(folder_of(k) == ".Projects/x" for k, _ in hits)
    hits = idx.search("q0", topk=3, folders=[".Projects/x"], statuses=["cur"])
    assert numbers(hits) == [9, 5, 3]
    assert all(status_of(k) == "cur" for k, _ in hits)
    hits = idx.search("q0", topk=10, statuses=["new"])
    assert numbers(hits) == [7, 2]                       # fewer than topk
    hits = idx.search("q0", topk=4, folders=[".Projects/x", ".Projects/y"])
    assert numbers(hits) == [10, 9, 7, 5]
    assert idx.search("q0", topk=3, folders=[".Projects/none"]) == []
    assert idx.search("q0", topk=3, folders=[".Projects/y"],
                      statuses=["new"]) == []
    # topk > 64 keeps the torch expression, scoped too
    hits = idx.search("q0", topk=100, folders=[".Projects/x"])
    assert numbers(hits) == [9, 7, 5, 3, 2, 1]
    assert len(idx.search("q0", topk=100)) == len(SCOPED_MEMORIES)
    mems = idx.search_memories("q0", topk=2, folders=[".Projects/x"])
    assert [m["headers"]["Subject"] for m in mems] == ["s9 memory",
                                                       "s7 memory"]


def check_batching(idx) -> None:
    """search_many equals search per query, in one encoder batch."""
    queries = ["q0", "q1", "q01"] * 4                    # 12: two scans
    for scope in ({}, {"folders": [".Projects/x"]},
                  {"statuses": ["cur"], "folders": ["", ".Projects/y"]}):
        calls = idx.encoder.calls
        many = idx.search_many(queries, topk=4, **scope)
        assert idx.encoder.calls == calls + 1
        assert len(many) == len(queries)
        for text, got in zip(queries, many):
            assert got == idx.search(text, topk=4, **scope)
    # q01 scores every memory 2.0: the tie resolves by row, lowest first
    tie = idx.search("q01", topk=5)
    assert [k for k, _ in tie] == idx.ids[:5]
    assert idx.search_many([], topk=3) == []


def check_mutation(idx) -> None:
    """Codes and cached masks follow add_texts and remove."""
    scope = {"folders": [".Projects/x"]}
    assert numbers(idx.search("q0", topk=2, **scope)) == [9, 7]
    assert len(idx._masks) == 1                          # cached
    idx.search("q0", topk=2, **scope)
    assert len(idx._masks) == 1
    idx.add_texts(["s12 late", "s6 late"],
                  [".Projects/x\x00new\x00late12", "\x00cur\x00late6"])
    assert idx.folder_codes.shape[0] == len(idx.ids) == idx.embeddings.shape[0]
    assert idx.folder_codes.dtype == idx.status_codes.dtype == torch.int16
    assert idx.folder_codes.device.type == idx.device.type
    assert numbers(idx.search("q0", topk=2, **scope)) == [12, 9]
    assert numbers(idx.search("q0", topk=2, folders=[".Projects/x"],
                              statuses=["cur"])) == [9, 5]
    # remove the scope's best two: never returned again, scoped or not
    gone = [k for k, _ in idx.search("q0", topk=2, **scope)]
    for key in gone:
        assert idx.remove(key.split("\x00")[2]) == 1
    assert idx.folder_codes.shape[0] == len(idx.ids)
    assert numbers(idx.search("q0", topk=2, **scope)) == [7, 5]
    every = idx.search("q0", topk=64) + idx.search("q0", topk=64, **scope)
    assert not {k for k, _ in every} & set(gone)
    # a folder first seen through add_texts gets a code of its own
    idx.add_texts(["s8 fresh"], [".Projects/z\x00cur\x00fresh8"])
    assert numbers(idx.search("q0", topk=3, folders=[".Projects/z"])) == [8]


def check_f16_scan(base: str, device) -> None:
    """scan_dtype="f16" scans exactly what save() persists."""
    idx16 = scoped_index(base, device, scan_dtype="f16")
    assert idx16.embeddings.dtype == torch.float32
    from fei_amd.memdir.embed_index import EmbeddingIndex
    loaded = EmbeddingIndex(base=base, encoder=ExactEncoder(device),
                            device=torch.device(device))
    assert loaded.load()
    assert torch.equal(idx16._scan_matrix().float().cpu(),
                       loaded.embeddings.cpu())
    assert idx16._scan_matrix().dtype == torch.float16
    for scope in ({}, {"folders": [".Projects/x"]}):
        for text in ("q0", "q1"):
            a = idx16.search(text, topk=5, **scope)
            b = loaded.search(text, topk=5, **scope)
            assert [k for k, _ in a] == [k for k, _ in b]
    assert loaded.folder_codes is not None               # rebuilt on load
    assert numbers(loaded.search("q0", topk=2,
                                 folders=[".Projects/x"])) == [9, 7]
