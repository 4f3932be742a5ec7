"""GPU tests of the top-k / top-p sampling kernel (csrc/sample_filtered.hip)
against ops/reference.py filter_keep, and of the engine paths built on it.

Inputs are generated on the CPU from fixed seeds. The seeds were chosen so
that the preconditions below hold for EVERY case; the tests assert the
preconditions (they are conditions on the inputs, not skips)."""

import functools

import pytest
import torch

from fei_amd import ops
from fei_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID = ((1, 64), (2, 1003), (9, 4096), (1, 128256))
PS = (1e-6, 0.5, 0.9, 1.0)
# rows ~ N(0, 3^2) rounded to bf16: a realistic spread, many exact ties at
# V = 128 256
ROW_SEED = {(1, 64): 0, (2, 1003): 0, (9, 4096): 4, (1, 128256): 0}
# the fp32 kernel's mass error (tree sum over <= 2^17 terms + fast exp) is
# <~ 1e-6 relative; a nucleus boundary this far from every group is decided
# identically in fp32 and fp64
P_MARGIN = 1e-4
# |x/T + g| gaps this large are far above the __logf-vs-log difference
GAP = 1e-3


@functools.lru_cache(maxsize=None)
def grid_rows(B, V):
    g = torch.Generator().manual_seed(1000 + ROW_SEED[(B, V)])
    return (torch.randn(B, V, generator=g) * 3.0).to(torch.bfloat16)


def ks_for(V):
    return (0, 1, 50, V)


def assert_p_margin(x, k, p):
    """Precondition of an exact comparison: no value group of any row has
    above(v) within P_MARGIN of p. The row maximum is exempt: its above(v)
    is exactly 0 in the kernel and in the reference alike (an empty sum),
    and 0 < p always. With p >= 1 the nucleus filter is off."""
    if p >= 1.0:
        return
    xd = x.to(torch.float64)
    V = xd.shape[1]
    for b in range(xd.shape[0]):
        row = xd[b]
        if 0 < k < V:
            row = row[row >= torch.topk(row, k).values[-1]]
        vals, counts = torch.unique(row, return_counts=True)
        vals, counts = vals.flip(0), counts.flip(0)
        w = torch.exp(vals - vals[0]) * counts.to(torch.float64)
        above = ((w.cumsum(0) - w) / w.sum())[1:]
        if above.numel():
            d = (above - p).abs().min().item()
            assert d >= P_MARGIN, (b, k, p, d)


class Bufs:
    def __init__(self, B, max_new=4):
        self.token = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        self.info = torch.zeros(B, 2, dtype=torch.float32, device=DEV)
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.out = torch.full((B, max_new), -1, dtype=torch.int32, device=DEV)


def launch(x_gpu, bufs, step, k, p, temperature=1.0, seed=11):
    bufs.step.fill_(step)
    ops.sample_filtered(x_gpu, bufs.token, bufs.step, bufs.info,
                        out_tokens=bufs.out, temperature=temperature,
                        seed=seed, top_k=k, top_p=p)
    return (bufs.token.cpu(), bufs.info[:, 0].cpu(),
            bufs.info[:, 1].view(torch.int32).cpu())


def check_info_exact(x, cases):
    xg = x.to(DEV)
    bufs = Bufs(x.shape[0])
    for k, p in cases:
        assert_p_margin(x, k, p)
    for k, p in cases:
        keep, thr, count = ref.filter_keep(x, k, p)
        tok, g_thr, g_count = launch(xg, bufs, 0, k, p)
        print(f"B={x.shape[0]} V={x.shape[1]} k={k} p={p} "
              f"thr {g_thr.tolist()} vs {thr.tolist()} "
              f"count {g_count.tolist()} vs {count.tolist()}")
        assert torch.equal(g_count, count), (k, p)
        assert torch.equal(g_thr, thr), (k, p)
        for b in range(x.shape[0]):
            assert keep[b, int(tok[b])], (k, p, b)


@pytest.mark.parametrize("B,V", GRID)
def test_threshold_and_count_exact_on_grid(B, V):
    x = grid_rows(B, V)
    check_info_exact(x, [(k, p) for k in ks_for(V) for p in PS])


def adversarial_rows():
    g = torch.Generator().manual_seed(77)
    rows = {}
    rows["all_equal"] = torch.full((2, 1003), 0.75)
    peaked = torch.randn(1, 4096, generator=g)
    peaked[0, 1234] = 20.0
    rows["peaked"] = peaked
    vals4 = torch.tensor([-1.0, 0.0, 0.5, 2.0])
    rows["four_values"] = vals4[torch.randint(0, 4, (3, 4096), generator=g)]
    tie = torch.randn(2, 1003, generator=g) * 0.5       # all far below 2.0
    tie = tie.clamp(max=1.5)
    perm = torch.randperm(1003, generator=g)
    tie[:, perm[:30]] = 3.0
    tie[:, perm[30:70]] = 2.0                           # ranks 31..70
    rows["k_boundary_tie"] = tie
    return {n: r.to(torch.bfloat16) for n, r in rows.items()}


ADV_CASES = {
    "all_equal": [(0, 0.5), (50, 0.9), (1, 1e-6), (1, 1.0), (0, 1.0)],
    "peaked": [(0, 0.9), (50, 0.9), (0, 0.5), (50, 1.0)],
    "four_values": [(0, 0.5), (0, 0.9), (50, 0.9), (50, 1.0), (2000, 0.5),
                    (1, 1.0)],
    "k_boundary_tie": [(50, 1.0), (50, 0.9), (50, 0.5), (31, 1.0),
                       (30, 1.0), (71, 1.0)],
}


@pytest.mark.parametrize("name", sorted(ADV_CASES))
def test_threshold_and_count_exact_on_adversarial_rows(name):
    x = adversarial_rows()[name]
    check_info_exact(x, ADV_CASES[name])
    keep, thr, count = ref.filter_keep(x, *ADV_CASES[name][0])
    if name == "all_equal":
        assert count.tolist() == [1003, 1003]
    if name == "peaked":                     # > 0.999 of the mass in one token
        q = torch.softmax(x.double(), -1)
        assert q[0, 1234] > 0.999
        assert count.tolist() == [1] and keep[0, 1234]
    if name == "k_boundary_tie":             # k = 50 lands inside the 2.0 group
        assert count.tolist() == [70, 70] and thr.tolist() == [2.0, 2.0]


# -- token ----------------------------------------------------------------

TOKEN_CASES = (  # (B, V), k, p, seed
    ((2, 1003), 50, 0.9, 1),
    ((9, 4096), 0, 0.5, 1),
    ((1, 128256), 50, 0.9, 1),
)


def reference_tokens(x, keep, T, seed, step):
    """argmax over the keep set of x/T + Gumbel, and the top-2 gap."""
    B, V = x.shape
    s = x.float() / T + ref.hash_gumbel(B, V, 0, seed, step)
    s = s.masked_fill(~keep, float("-inf"))
    top = s.topk(2, dim=-1)
    return top.indices[:, 0].to(torch.int32), top.values[:, 0] - top.values[:, 1]


@pytest.mark.parametrize("shape,k,p,seed", TOKEN_CASES)
def test_token_exact(shape, k, p, seed):
    x = grid_rows(*shape)
    assert_p_margin(x, k, p)
    keep, _, _ = ref.filter_keep(x, k, p)
    xg = x.to(DEV)
    bufs = Bufs(shape[0], max_new=16)
    min_gap = float("inf")
    for T in (1.0, 0.5):
        for step in range(16):
            want, gap = reference_tokens(x, keep, T, seed, step)
            min_gap = min(min_gap, gap.min().item())
            assert gap.min().item() >= GAP, (T, step, gap)
            tok, _, _ = launch(xg, bufs, step, k, p, temperature=T, seed=seed)
            assert torch.equal(tok, want), (T, step)
            assert torch.equal(bufs.out[:, step].cpu(), want)
    print(f"{shape} k={k} p={p}: smallest reference top-2 gap {min_gap:.3e}")


def test_draws_cover_the_nucleus():
    """512 steps at V=64, top_p=0.5: every token is in the keep set and
    every kept token with renormalised probability >= 0.05 is drawn (miss
    probability < 1e-11; the noise is deterministic anyway)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, generator=g).to(torch.bfloat16)   # a flat row
    assert_p_margin(x, 0, 0.5)
    keep, _, _ = ref.filter_keep(x, 0, 0.5)
    xg = x.to(DEV)
    bufs = Bufs(1, max_new=512)
    for step in range(512):
        bufs.step.fill_(step)
        ops.sample_filtered(xg, bufs.token, bufs.step, bufs.info,
                            out_tokens=bufs.out, temperature=1.0, seed=5,
                            top_k=0, top_p=0.5)
    drawn = bufs.out[0].cpu().long()
    assert keep[0, drawn].all()
    q = torch.softmax(x[0].double().masked_fill(~keep[0], float("-inf")), -1)
    likely = (q >= 0.05).nonzero().flatten().tolist()
    assert len(likely) >= 2
    assert set(likely) <= set(drawn.tolist())


@pytest.mark.parametrize("B,V", ((2, 1003), (9, 4096)))
def test_inactive_filter_equals_plain_sampler(B, V):
    x = grid_rows(B, V)
    xg = x.to(DEV)
    bufs = Bufs(B)
    ws = torch.zeros(B, 64 * 2, dtype=torch.float32, device=DEV)
    want = torch.zeros(B, dtype=torch.int32, device=DEV)
    for T in (0.0, 0.8, 1.0):
        for step in range(4):
            tok, thr, count = launch(xg, bufs, step, 0, 1.0, temperature=T,
                                     seed=9)
            ops.sample(xg, want, bufs.step, ws, temperature=T, seed=9)
            assert torch.equal(tok, want.cpu()), (T, step)
            assert count.tolist() == [V] * B
            assert torch.equal(thr, x.float().amin(-1))
    tok, _, _ = launch(xg, bufs, 3, V, 1.0, temperature=1.0, seed=9)  # k >= V
    assert torch.equal(tok, want.cpu())


def test_out_tokens_written_only_inside_max_new():
    x = grid_rows(2, 1003)
    xg = x.to(DEV)
    bufs = Bufs(2, max_new=4)
    tok, _, _ = launch(xg, bufs, 2, 50, 0.9)
    out = bufs.out.cpu()
    assert torch.equal(out[:, 2], tok)
    assert (out[:, [0, 1, 3]] == -1).all()
    for step in (4, 7):                      # step >= max_new writes nothing
        before = bufs.out.clone()
        tok, _, _ = launch(xg, bufs, step, 50, 0.9)
        assert torch.equal(bufs.out, before)
        assert (tok >= 0).all()              # token itself is still produced


def test_repeatable():
    x = grid_rows(9, 4096)
    xg = x.to(DEV)
    a = launch(xg, Bufs(9), 3, 50, 0.9)
    b = launch(xg, Bufs(9), 3, 50, 0.9)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# -- engine -------------------------------------------------------------------

def make_engine(graph):
    from fei_amd.engine.engine import LocalEngine
    return LocalEngine.create("llama3-tiny", max_seq_len=256, seed=7,
                              use_hip_graph=graph)


@pytest.fixture(scope="module")
def graph_engine():
    return make_engine(True)


@pytest.fixture(scope="module")
def eager_engine():
    return make_engine(False)


def test_engine_graph_matches_eager_with_top_k(graph_engine, eager_engine):
    kw = dict(max_new_tokens=24, temperature=1.0, top_k=8, stop_on_eos=False)
    a = graph_engine.generate("filtered graph test", **kw)
    assert graph_engine._graph is not None
    assert graph_engine._graph_params == (1.0, graph_engine.seed, 8, 1.0)
    b = eager_engine.generate("filtered graph test", **kw)
    assert len(a["token_ids"]) == 24
    assert a["token_ids"] == b["token_ids"]
    # the filter really ran: at most 8 + ties candidates at the last step
    n = graph_engine.sample_info[0, 1].view(torch.int32).item()
    assert 8 <= n < graph_engine.spec.vocab_size


def test_engine_recaptures_when_filter_changes(graph_engine):
    graph_engine.generate("recapture", max_new_tokens=8, temperature=1.0,
                          top_k=1, stop_on_eos=False)
    kw = dict(max_new_tokens=16, temperature=1.5, top_k=0, stop_on_eos=False)
    got = graph_engine.generate("recapture", **kw)
    assert graph_engine._graph_params == (1.5, graph_engine.seed, 0, 1.0)
    fresh = make_engine(True).generate("recapture", **kw)
    assert got["token_ids"] == fresh["token_ids"]


def test_engine_top_k_one_is_greedy(graph_engine, eager_engine):
    """temperature=0.7, top_k=1 == greedy where each step's argmax is unique
    (a tie at the top would be kept whole and broken by the noise). The
    probe records the logits the sampler sees on the eager path."""
    seen = []
    orig = eager_engine._sample

    def probe(logits):
        seen.append(logits.float().cpu())
        return orig(logits)

    eager_engine._sample = probe
    try:
        for prompt in ("unique argmax", "top-k one", "greedy probe",
                       "another prompt", "fifth candidate", "sixth"):
            del seen[:]
            greedy = eager_engine.generate(prompt, max_new_tokens=8,
                                           stop_on_eos=False)
            top2 = [l[0].topk(2).values for l in seen]
            if all(float(t[0]) > float(t[1]) for t in top2):
                break
        else:
            pytest.fail("no candidate prompt has a unique argmax per step")
    finally:
        eager_engine._sample = orig
    assert len(seen) == 8
    out = graph_engine.generate(prompt, max_new_tokens=8, temperature=0.7,
                                top_k=1, stop_on_eos=False)
    assert out["token_ids"] == greedy["token_ids"]


def test_engine_stream_matches_generate_with_top_p(graph_engine):
    kw = dict(max_new_tokens=20, temperature=1.0, top_p=0.9,
              stop_on_eos=False)
    plain = graph_engine.generate("gpu stream check", **kw)
    chunks = list(graph_engine.generate_stream("gpu stream check", chunk=6,
                                               **kw))
    ids = [t for c in chunks for t in c["new_token_ids"]]
    assert ids == plain["token_ids"]
    assert chunks[-1]["done"]
