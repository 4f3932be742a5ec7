"""Case tables, input builders, fp64 references and per-element bounds for
the decode attention, sampler and GEMV shape tests.

Shared by test_decode_shapes_gpu.py / test_gemv_shapes_gpu.py (device
"cuda:0", the HIP kernels) and test_decode_shapes_cpu.py (device "cpu",
where fei_amd.ops dispatches to the fp32 torch reference): the CPU run
proves that a correct fp32 implementation meets every bound used on the GPU.

All inputs are built on the CPU as f32 tensors holding bf16-representable
values; every reference is fp64 arithmetic on exactly those values. The
bounds are the ones written down in docs/TESTING.md ("Decode shape tests").
"""

import functools
import math

import torch

from fei_amd import ops
from fei_amd.ops import reference as ref

F64 = torch.float64
NAN = float("nan")


def bf16r(t):
    """Round to the bf16 grid, keep f32 storage."""
    return t.to(torch.bfloat16).float()


def ulp(x):
    """bf16 spacing at |x| (fp64 in, fp64 out)."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 8)


def put(t, device, dtype=None):
    """CPU f32 master -> test tensor. GPU kernels take bf16; the CPU
    reference takes f32 unless the op's documented semantics need a bf16
    rounding step (dtype=torch.bfloat16)."""
    if dtype is None:
        dtype = torch.bfloat16 if device != "cpu" else torch.float32
    return t.to(dtype).to(device).contiguous().clone()   # never the master


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def assert_within(out, want, bound, what):
    out = out.detach().to("cpu").to(F64)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    err = (out - want).abs()
    bad = err > bound
    if bad.any():
        i = int((err - bound).argmax())
        raise AssertionError(
            f"{what}: {int(bad.sum())}/{bad.numel()} outside the bound; worst "
            f"|err|={err.flatten()[i].item():.3e} bound="
            f"{bound.flatten()[i].item():.3e} ref={want.flatten()[i].item():.6g}"
            f" at flat index {i}")
    return float((err / bound).max())


# ===========================================================================
# Decode attention
# ===========================================================================

B, HQ, MS = 3, 8, 1024
GD_PAIRS = [(g, d) for g in (1, 2, 4, 8) for d in (64, 128)]
PAGED_BS = (8, 16, 64)

# (splits, n): n is sequence 0's length; _lens() adds two more sequences
SPLIT_CASES = (
    [(s, 1) for s in (1, 4, 32, 64)]
    + [(1, n) for n in (255, 256, 257, 513)]          # DEC_TILE inside a WG
    + [(4, n) for n in (252, 253, 256, 257, 260)]     # chunk 63 / 64 / 65
    + [(32, 20), (32, 1024), (64, 700)])
# RoPE-fused extras: the new key is the only key of the last split
# (n=13: chunk 4, split 3 = {12}; n=962: chunk 31, split 31 = {961}) / the
# first key of a tile (n=257, 513)
ROPE_EXTRA = [(4, 13), (32, 962), (1, 257), (1, 513)]
FUSED_N = (1, 255, 256, 257, 640, 1024)


def _lens(n, splits):
    """Sequence 0 has n keys; sequence 1 sits on the OTHER V lane map where
    the split count allows (chunk >= 64 is WIDE, below is PAIR); sequence 2
    is a third, different length."""
    chunk = -(-n // splits)
    if chunk >= 64:
        n2 = 25 * splits
    else:
        n2 = 75 * splits if 75 * splits <= MS else 777
    n3 = max(1, n // 2 - 1)
    while n3 in (n, n2):
        n3 += 2
    return (n, n2, n3)


def planted(n, splits):
    """Key positions a split or tile boundary touches: key 0, key n-1, the
    first/last key of the first four and the last non-empty split with
    their outside neighbours, and both sides of every DEC_TILE=256 step
    inside those splits."""
    chunk = -(-n // splits)
    nsp = -(-n // chunk)
    pts = {0, n - 1}
    for sp in {0, 1, 2, 3, nsp - 1}:
        if sp >= nsp:
            continue
        start, end = sp * chunk, min(sp * chunk + chunk, n)
        pts |= {start - 1, start, end - 1, end}
        for t in range(start + 256, end, 256):
            pts |= {t - 1, t}
    return sorted(p for p in pts if 0 <= p < n)


def rounds(lens, splits):
    """Each of the 8 q heads follows ONE planted key per launch; enough
    launches that every planted position of every sequence gets a head."""
    return -(-max(len(planted(n, splits)) for n in lens) // HQ)


@functools.lru_cache(maxsize=None)
def _base(hkv, D):
    g = torch.Generator().manual_seed(1000 + 10 * hkv + D)
    K = bf16r(torch.randn(B, hkv, MS, D, generator=g))
    V = bf16r(torch.randn(B, hkv, MS, D, generator=g))
    q = bf16r(3.0 * torch.randn(B, HQ, D, generator=g))
    sgn = torch.randint(0, 2, (B, hkv, 16, D), generator=g).float() * 2 - 1
    return K, V, q, sgn


@functools.lru_cache(maxsize=None)
def rope_tab(D):
    return ref.rope_table(MS, D)                   # f32 [MS, D/2, 2]


def _cs(D, pos):
    t = rope_tab(D)[torch.as_tensor(pos).long()].to(F64)   # [B, D/2, 2]
    return t[..., 0].unsqueeze(1), t[..., 1].unsqueeze(1)  # [B, 1, D/2]


def rope64(x, pos):
    """fp64 half-split RoPE of x [B, H, D] at pos [B], from the f32 table
    the kernels read."""
    D = x.shape[-1]
    c, s = _cs(D, pos)
    x1, x2 = x[..., :D // 2].to(F64), x[..., D // 2:].to(F64)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def unrope(y, pos):
    D = y.shape[-1]
    c, s = _cs(D, pos)
    y1, y2 = y[..., :D // 2].to(F64), y[..., D // 2:].to(F64)
    return bf16r(torch.cat([y1 * c + y2 * s, y2 * c - y1 * s], dim=-1).float())


class AttnCase:
    """One (G, D, splits, lens, round) problem. K/V are the CPU masters
    [B, Hkv, MS, D] with the planted keys in place (unpoisoned); q is the
    roped query, q_raw / kin / vin the un-roped inputs of the RoPE-fused
    forms (kin/vin reproduce cache row n-1)."""

    def __init__(self, G, D, splits, lens, rnd=0):
        self.G, self.D, self.splits, self.lens, self.rnd = G, D, splits, lens, rnd
        self.hkv = hkv = HQ // G
        self.scale = float(torch.tensor(1.0 / math.sqrt(D)).float())
        K0, V0, q0, sgn = _base(hkv, D)
        K, V, q = K0.clone(), V0.clone(), q0.clone()
        gamma = 30.0 / math.sqrt(D)
        d = torch.arange(D).float()
        for b, n in enumerate(lens):
            P = planted(n, splits)
            assert len(P) <= sgn.shape[2]
            for j, p in enumerate(P):
                K[b, :, p] = sgn[b, :, j]
                # asymmetric ramp, distinct per planted key
                V[b, :, p] = bf16r((-1.0) ** j * (0.5 + 0.25 * j + d / D))
            for hq in range(HQ):
                j = (hq + HQ * rnd) % len(P)
                q[b, hq] += gamma * sgn[b, hq // G, j]
        self.K, self.V, self.q = K, V, bf16r(q)
        self.pos = torch.tensor([n - 1 for n in lens], dtype=torch.int32)
        idx = torch.arange(B)
        self.q_raw = unrope(self.q, self.pos)
        self.kin = unrope(K[idx, :, self.pos.long()], self.pos)
        self.vin = V[idx, :, self.pos.long()].clone()
        self._ref = {}

    def name(self):
        return (f"G{self.G} D{self.D} splits{self.splits} lens{self.lens} "
                f"round{self.rnd}")

    def reference(self, q64, knew=None):
        """fp64 softmax(q K^T scale) V over the first lens[b] rows; knew
        [B, Hkv, D] replaces cache row n-1 (the row a fused kernel wrote).
        Returns (out [B,HQ,D], bound [B,HQ,D])."""
        key = (q64.numpy().tobytes(),
               None if knew is None else knew.numpy().tobytes())
        if key in self._ref:
            return self._ref[key]
        out = torch.empty(B, HQ, self.D, dtype=F64)
        vmax = torch.empty(B, HQ, 1, dtype=F64)
        for b, n in enumerate(self.lens):
            k = self.K[b, :, :n].to(F64)
            v = self.V[b, :, :n].to(F64)
            if knew is not None:
                k[:, n - 1] = knew[b].to(F64)
            qb = q64[b].view(self.hkv, self.G, self.D)
            s = torch.einsum("hgd,hnd->hgn", qb, k) * self.scale
            # the bound's derivation assumes n <= 1024 and |score| <= 64
            assert n <= 1024 and float(s.abs().max()) <= 64.0, self.name()
            p = torch.softmax(s, dim=-1)
            out[b] = torch.einsum("hgn,hnd->hgd", p, v).reshape(HQ, self.D)
            vmax[b] = v.abs().amax(dim=(1, 2)).repeat_interleave(self.G)[:, None]
        res = (out, ulp(out) + 2.0 ** -13 * vmax)
        self._ref[key] = res
        return res

    # -- device tensors ------------------------------------------------------

    def caches(self, device, hole):
        """Poisoned caches: every row >= n is NaN; with hole, row n-1 too
        (the RoPE-fused forms write it)."""
        Kd, Vd = put(self.K, device), put(self.V, device)
        for b, n in enumerate(self.lens):
            Kd[b, :, n - (1 if hole else 0):] = NAN
            Vd[b, :, n - (1 if hole else 0):] = NAN
        return Kd, Vd

    def pools(self, device, BS, hole):
        """Scrambled paged pool of the same content. Unused pool blocks are
        NaN; table entries past the last used block point at a NaN block."""
        Kd, Vd = self.caches(device, hole)
        nblk = MS // BS
        g = torch.Generator().manual_seed(BS + 7 * self.D)
        perm = torch.randperm(B * nblk + 4, generator=g)
        bt = torch.full((B, nblk), int(perm[-1]), dtype=torch.int32)
        kp = torch.full((B * nblk + 4, self.hkv, BS, self.D), NAN,
                        dtype=Kd.dtype, device=device)
        vp = kp.clone()
        for b, n in enumerate(self.lens):
            used = -(-n // BS)
            ids = perm[b * nblk: b * nblk + used]
            bt[b, :used] = ids.to(torch.int32)
            src = slice(0, used * BS)
            kp[ids.to(device)] = Kd[b, :, src].reshape(
                self.hkv, used, BS, self.D).transpose(0, 1)
            vp[ids.to(device)] = Vd[b, :, src].reshape(
                self.hkv, used, BS, self.D).transpose(0, 1)
        return kp, vp, bt.to(device)


def run_attn_form(case, form, device):
    """Run one form of one case and check it. Returns the output (CPU f64)
    so forms can be compared with each other."""
    what = f"{form} {case.name()}"
    pos = case.pos.to(device)
    kw = dict(splits=case.splits, scale=case.scale)
    idx = torch.arange(B, device=device)
    if form in ("plain", "cmb"):
        Kd, Vd = case.caches(device, hole=False)
        if form == "cmb":
            ws = (torch.zeros(B, HQ, case.splits, case.D, device=device),
                  torch.zeros(B, HQ, case.splits, 2, device=device),
                  torch.zeros(B * case.hkv * case.splits, dtype=torch.int32,
                              device=device))
            saved, ops._FUSED_CMB = ops._FUSED_CMB, True
            try:
                out = ops.attn_decode(put(case.q, device), Kd, Vd, pos,
                                      workspace=ws, layer=5, **kw)
            finally:
                ops._FUSED_CMB = saved
        else:
            out = ops.attn_decode(put(case.q, device), Kd, Vd, pos, **kw)
        want, bound = case.reference(case.q.to(F64))
    elif form.startswith("paged") and not form.endswith("rope"):
        kp, vp, bt = case.pools(device, int(form[5:]), hole=False)
        out = ops.attn_decode_paged(put(case.q, device), kp, vp, bt, pos, **kw)
        want, bound = case.reference(case.q.to(F64))
    else:
        q_raw, kin, vin = (put(t, device) for t in
                           (case.q_raw, case.kin, case.vin))
        table = rope_tab(case.D).to(device)
        if form.startswith("paged"):
            BS = int(form[5:-4])
            kp, vp, bt = case.pools(device, BS, hole=True)
            before = (kp.clone(), vp.clone())
            out = ops.attn_decode_paged(q_raw, kp, vp, bt, pos, k=kin, v=vin,
                                        table=table, **kw)
            blk = bt[idx, (pos >> (BS.bit_length() - 1)).long()].long()

            def rows_view(t, blk=blk, within=(pos & (BS - 1)).long()):
                return _Rows(t, (blk, slice(None), within))
            after = (kp, vp)
        else:
            Kd, Vd = case.caches(device, hole=True)
            before = (Kd.clone(), Vd.clone())
            if form == "rope":
                out = ops.attn_decode(q_raw, Kd, Vd, pos, k=kin, v=vin,
                                      table=table, **kw)
            else:
                assert form == "fused"
                out = ops.attn_decode_fused(q_raw, kin, vin, Kd, Vd, pos,
                                            table, scale=case.scale)
            def rows_view(t, p=pos.long()):
                return _Rows(t, (idx, slice(None), p))
            after = (Kd, Vd)
        knew = _check_inplace_rows(case, before, after, rows_view, what)
        want, bound = case.reference(rope64(case.q_raw, case.pos), knew)
    assert_within(out, want, bound, what)
    return out.detach().to("cpu").to(F64)


class _Rows:
    """The [B, Hkv, D] rows of a cache / pool selected by an advanced index
    (read = gather, zero = scatter)."""

    def __init__(self, t, index):
        self.t, self.index = t, index

    def get(self):
        return self.t[self.index]

    def zero(self):
        self.t[self.index] = 0


def _check_inplace_rows(case, before, after, rows_view, what):
    """Everything outside the appended rows must be bit-equal to its value
    before the call; the appended K row within ulp of the fp64 RoPE of kin;
    the V row bit-equal to vin. Returns the K rows the kernel left."""
    knew = rows_view(after[0]).get().detach().to("cpu").float()
    vnew = rows_view(after[1]).get().detach().to("cpu").float()
    for a, b_ in zip(before, after):
        a, b_ = a.clone(), b_.clone()
        rows_view(a).zero()
        rows_view(b_).zero()
        assert torch.equal(bits(a), bits(b_)), \
            f"{what}: wrote outside the appended row"
    want = rope64(case.kin, case.pos)
    assert_within(knew, want, ulp(want), f"{what}: appended K row")
    assert torch.equal(vnew, case.vin), f"{what}: appended V row"
    return knew


SPLIT_FORMS = (["plain", "cmb", "rope"] + [f"paged{bs}" for bs in PAGED_BS]
               + [f"paged{bs}rope" for bs in PAGED_BS])


def run_split_case(G, D, splits, n, device, forms=SPLIT_FORMS):
    lens = _lens(n, splits)
    for rnd in range(rounds(lens, splits)):
        case = AttnCase(G, D, splits, lens, rnd)
        outs = {f: run_attn_form(case, f, device) for f in forms}
        if "plain" in outs and "cmb" in outs:
            # same partials, only the reduction site moves
            assert_within(outs["cmb"], outs["plain"], ulp(outs["plain"]),
                          f"cmb vs separate combine {case.name()}")


def run_fused_case(G, D, n, device):
    lens = (n, max(1, n // 2 - 1) if n > 4 else 3, 37 if n != 37 else 41)
    for rnd in range(rounds(lens, 1)):
        run_attn_form(AttnCase(G, D, 1, lens, rnd), "fused", device)


# ===========================================================================
# Samplers (greedy: exact)
# ===========================================================================

def sampler_logits(Bn, V, seed):
    """Random bf16 logits with a known argmax per row: row 0's maximum is
    the LAST element, row 1's is element 0, row 2 has an exact tie (lowest
    index must win) placed as far apart as V allows, other rows a random
    unique maximum."""
    g = torch.Generator().manual_seed(seed)
    x = bf16r(torch.randn(Bn, V, generator=g))
    want = torch.randint(0, V, (Bn,), generator=g)
    want[0], want[1] = V - 1, 0
    if Bn > 2:
        want[2] = min(5, V - 2)
        x[2, V - 1] = 50.0                         # the tie's high index
    x[torch.arange(Bn), want] = 50.0
    return x, want.to(torch.int32)


def run_sample_case(Bn, V, device, step_val=1, max_new=4):
    x, want = sampler_logits(Bn, V, seed=Bn * 100003 + V)
    token = torch.full((Bn,), -1, dtype=torch.int32, device=device)
    step = torch.tensor([step_val], dtype=torch.int32, device=device)
    out_tokens = torch.full((Bn, max_new), -7, dtype=torch.int32, device=device)
    ws = torch.zeros(Bn, 64 * 2, dtype=torch.float32, device=device)
    ops.sample(put(x, device), token, step, ws, out_tokens=out_tokens,
               temperature=0.0, nchunks=64)
    what = f"sample B{Bn} V{V} step{step_val}"
    assert torch.equal(token.cpu(), want), \
        f"{what}: {token.cpu().tolist()} != {want.tolist()}"
    exp = torch.full((Bn, max_new), -7, dtype=torch.int32)
    if step_val < max_new:
        exp[:, step_val] = want
    assert torch.equal(out_tokens.cpu(), exp), f"{what}: out_tokens"


def run_sample_shard_case(Bn, V, v_offset, device):
    x, want = sampler_logits(Bn, V, seed=Bn * 7 + V)
    step = torch.zeros(1, dtype=torch.int32, device=device)
    out = torch.zeros(Bn, 2, dtype=torch.float32, device=device)
    ops.sample_shard(put(x, device), step, v_offset, out, temperature=0.0)
    got = out[:, 1].contiguous().view(torch.int32).cpu()
    assert torch.equal(got, want + v_offset), (got.tolist(), want.tolist())
    assert torch.equal(out[:, 0].cpu(), torch.full((Bn,), 50.0))


def run_advance_case(device):
    pos = torch.tensor([5, 9, 10], dtype=torch.int32, device=device)
    step = torch.tensor([3], dtype=torch.int32, device=device)
    ops.advance(pos, step, max_pos=10)
    assert pos.tolist() == [6, 10, 10] and int(step) == 4
    ops.advance(pos, step, max_pos=10)
    assert pos.tolist() == [7, 10, 10] and int(step) == 5


# ===========================================================================
# GEMV family
# ===========================================================================

GEMV_M = (1, 2, 4, 8)
GEMV_N = (1, 7, 9, 33)          # two-row kernels: odd N, tail block, N < 8
SWIGLU_I = (1, 5, 6, 7)         # per half; 4 rows per block
K_BF16 = (64, 520, 1024)        # K/8  = 8, 65, 128
K_FP8 = (64, 1040, 2048)        # K/16 = 4, 65, 128
BF16_OPS = ("linear", "swiglu", "res", "res_ssq", "norm", "norm_ssq",
            "swiglu_norm", "swiglu_norm_ssq")
FP8_OPS = ("norm_fp8", "res_fp8", "swiglu_norm_fp8")
EPS = 1e-5
TIE_CAP = 8


def _is_swiglu(op):
    return op.startswith("swiglu")


def gemv_weights(rows, K, seed, ramp):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows, K, generator=g) / math.sqrt(K)
    if ramp:
        # row n carries its own ramp: a swapped row pair or a transposed
        # write cannot cancel
        r = (torch.arange(rows).float()[:, None] + 1) / rows
        w = w + r * (0.5 + torch.arange(K).float()[None] / K) / math.sqrt(K)
    return bf16r(w)


def normed(x64, wn64, K):
    """fp64 RMSNorm, rounded to bf16 (the documented semantics of the
    norm-prologue GEMVs). Returns (xn rounded, near-tie mask, ulp(xn)):
    an element within relative 2^-20 of a bf16 rounding boundary may round
    either way in an f32 implementation."""
    eps = float(torch.tensor(EPS).float())
    inv = 1.0 / torch.sqrt((x64 * x64).sum(-1, keepdim=True) / K + eps)
    xn = x64 * inv * wn64
    u = ulp(xn)
    frac = xn.abs() / u
    frac = frac - torch.floor(frac)
    tie = ((frac - 0.5).abs() * u <= 2.0 ** -20 * xn.abs()) & (xn != 0)
    assert int(tie.sum(-1).max()) <= TIE_CAP, \
        f"near-tie cap: {tie.sum(-1).tolist()} (pick another seed)"
    return xn.float().to(torch.bfloat16).to(F64), tie, u


def _dots(x64, w64, K, tie=None, u=None):
    dot = x64 @ w64.T
    e = K * 2.0 ** -23 * (x64.abs() @ w64.abs().T)
    if tie is not None:
        e = e + (tie.to(F64) * u) @ w64.abs().T
    return dot, e


def _swiglu_ref(dot, e, I):
    g, u_ = dot[:, :I], dot[:, I:]
    sg = g * torch.sigmoid(g)
    want = sg * u_
    bound = (ulp(want) + 1.1 * u_.abs() * e[:, :I] + sg.abs() * e[:, I:]
             + 2.0 ** -20 * want.abs())
    return want, bound


def run_gemv_case(op, M, N, K, device, ramp=False, expect_mfma=False,
                  seed=None):
    """One op at one shape. For the swiglu ops N is the per-half width I."""
    what = f"{op} M{M} N{N} K{K}{' ramp' if ramp else ''}"
    if seed is None:
        seed = M * 1009 + N * 9176 + K * 31 + len(op)
    g = torch.Generator().manual_seed(seed)
    fp8 = op.endswith("fp8")
    rows = 2 * N if _is_swiglu(op) else N
    x = bf16r(torch.randn(M, K, generator=g))          # distinct rows
    w = gemv_weights(rows, K, seed + 1, ramp)
    wn = bf16r(1.0 + 0.5 * torch.randn(K, generator=g))
    res0 = bf16r(torch.randn(M, N, generator=g))
    x64 = x.to(F64)
    # the CPU reference rounds where its dtype says: bf16 tensors for the ops
    # whose semantics include a bf16 rounding of the normed activation
    cpu_dt = torch.bfloat16 if ("norm" in op or fp8) else torch.float32
    dt = None if device != "cpu" else cpu_dt
    if fp8:
        w8, sc = ref.quant_fp8(w)
        w64 = ref.dequant_fp8(w8, torch.ones_like(sc)).to(F64) \
            * sc.to(F64)[:, None]
        w8d, scd = w8.to(device), sc.to(device)
    else:
        w64 = w.to(F64)
        wd = put(w, device, dt)
    mfma = ops._gemm_m8_ok(M, rows, K)
    assert mfma == expect_mfma, f"{what}: wrong kernel (_gemm_m8_ok={mfma})"
    if device != "cpu" and not expect_mfma and op in BF16_OPS:
        assert ops._gemv_ok(M, K), what
    tie = u = None
    if "norm" in op:
        xin64, tie, u = normed(x64, wn.to(F64), K)
    else:
        xin64 = x64
    dot, e = _dots(xin64, w64, K, tie, u)
    ssq = None
    if op.endswith("_ssq") and "norm" in op:
        ssq = (x64 * x64).sum(-1).float().to(device)
    xd, wnd = put(x, device, dt), put(wn, device, dt)

    if op == "linear":
        out = ops.linear_decode(xd, wd)
        want, bound = dot, ulp(dot) + e
    elif op == "swiglu":
        out = ops.gemv_swiglu(xd, wd)
        want, bound = _swiglu_ref(dot, e, N)
    elif op in ("res", "res_ssq", "res_fp8"):
        resd = put(res0, device, dt)
        guard = resd.clone()
        ssq_out = (torch.zeros(M, dtype=torch.float32, device=device)
                   if op == "res_ssq" else None)
        if fp8:
            out = ops.gemv_res_fp8(xd, w8d, scd, resd)
        else:
            out = ops.gemv_res(xd, wd, resd, ssq_out=ssq_out)
        assert out.data_ptr() == resd.data_ptr() and guard.shape == out.shape
        want = (res0.to(F64) + dot).float().to(torch.bfloat16).to(F64)
        bound = ulp(want) + e
        if ssq_out is not None and device != "cpu":
            # contract: sum of squares of the kernel's OWN updated residual
            r2 = (out.detach().cpu().to(F64) ** 2).sum(-1)
            assert_within(ssq_out, r2, N * 2.0 ** -23 * r2 + 1e-300,
                          f"{what}: ssq_out")
    elif op in ("norm", "norm_ssq"):
        out = ops.gemv_norm(xd, wnd, wd, EPS, ssq=ssq)
        want, bound = dot, ulp(dot) + e
    elif op in ("swiglu_norm", "swiglu_norm_ssq"):
        out = ops.gemv_swiglu_norm(xd, wnd, wd, EPS, ssq=ssq)
        want, bound = _swiglu_ref(dot, e, N)
    elif op == "norm_fp8":
        out = ops.gemv_norm_fp8(xd, wnd, w8d, scd, EPS)
        want, bound = dot, ulp(dot) + e
    elif op == "swiglu_norm_fp8":
        out = ops.gemv_swiglu_norm_fp8(xd, wnd, w8d, scd, EPS)
        want, bound = _swiglu_ref(dot, e, N)
    else:
        raise ValueError(op)
    assert tuple(out.shape) == (M, N), (what, tuple(out.shape))
    return assert_within(out, want, bound, what)


def run_mfma_case(op, M, N, K, device):
    """k_gemm_m8 through linear_decode / gemv_swiglu (N = total W rows):
    distinct x rows, and a sentinel-filled output with guard rows — exactly
    M*N (M*N/2 for swiglu) elements written and none beyond."""
    assert ops._gemm_m8_ok(M, N, K)
    g = torch.Generator().manual_seed(M * 131 + N * 7 + K)
    x = bf16r(torch.randn(M, K, generator=g)
              + torch.arange(M).float()[:, None] * 0.25)
    w = gemv_weights(N, K, M + N + K, ramp=True)
    cols = N // 2 if op == "swiglu" else N
    xd, wd = put(x, device), put(w, device)
    buf = torch.empty(M + 9, cols, dtype=xd.dtype, device=device)
    buf.fill_(-12345.0)                             # far outside any output
    sent = buf[0, 0].clone()                        # (as rounded to buf.dtype)
    if op == "swiglu":
        out = ops.gemv_swiglu(xd, wd, out=buf[:M])
    else:
        out = ops.linear_decode(xd, wd, out=buf[:M])
    dot, e = _dots(x.to(F64), w.to(F64), K)
    if op == "swiglu":
        want, bound = _swiglu_ref(dot, e, cols)
        if device != "cpu":
            # the MFMA route rounds g and u to bf16 ([M, 2I] intermediate
            # feeding k_swiglu): one more half-ulp on each factor
            g_, u_ = dot[:, :cols], dot[:, cols:]
            sg = g_ * torch.sigmoid(g_)
            bound = bound + 1.1 * u_.abs() * ulp(g_) / 2 + sg.abs() * ulp(u_) / 2
    else:
        want, bound = dot, ulp(dot) + e
    what = f"mfma {op} M{M} N{N} K{K}"
    if device != "cpu":
        assert out.data_ptr() == buf.data_ptr()
        assert bool((buf[M:] == sent).all()), f"{what}: wrote past row M"
        assert bool((buf[:M] != sent).all()), f"{what}: left elements unwritten"
    return assert_within(out, want, bound, what)


# -- quant_fp8 ----------------------------------------------------------------

E4M3_GRID = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn) \
    .float().to(F64)
E4M3_POS = torch.unique(E4M3_GRID[torch.isfinite(E4M3_GRID) & (E4M3_GRID >= 0)])


def run_quant_case(N, K, device, zero_row=None):
    g = torch.Generator().manual_seed(N * 31 + K)
    w = bf16r((torch.randn(N, K, generator=g) * 0.05).clamp(-0.24, 0.24))
    # w/scale = 448 * w/amax hits an e4m3 rounding boundary EXACTLY whenever
    # 7 * mant(w) = odd * mant(amax) * 2^k, which short bf16 mantissas do for
    # ~0.5 % of random elements. An odd amax mantissa that is no multiple of
    # 7 rules that out, which keeps the near-boundary cap below.
    mant = torch.tensor([m for m in range(129, 256, 2) if m % 7])
    w[:, 0] = (mant[torch.arange(N) % len(mant)].float() / 128) * 0.25
    if zero_row is not None:
        w[zero_row] = 0
    w8, sc = ops.quant_fp8(put(w, device))
    w8, sc = w8.cpu(), sc.cpu()
    amax = w.abs().amax(-1)
    want_sc = amax / 448.0                          # f32 division
    nz = amax > 0
    assert torch.equal(bits(sc[nz]), bits(want_sc[nz])), "scale != amax/448"
    if zero_row is not None:
        assert not bool(w8[zero_row].any()), "zero row: codes must be 0"
        if device != "cpu":                         # ref.quant_fp8 reports its
            assert float(sc[zero_row]) == 1.0       # clamp floor instead
    scale64 = torch.where(nz, want_sc, torch.ones_like(want_sc)).to(F64)
    t = w.to(F64) / scale64[:, None]
    cast = t.float().to(torch.float8_e4m3fn).view(torch.uint8)
    # rounding boundaries = midpoints of adjacent e4m3 values
    mids = (E4M3_POS[1:] + E4M3_POS[:-1]) / 2
    a = t.abs()
    j = torch.searchsorted(mids, a.contiguous()).clamp(1, len(mids) - 1)
    dist = torch.minimum((a - mids[j - 1]).abs(), (a - mids[j]).abs())
    near = dist <= 2.0 ** -20 * a
    diff = w8 != cast
    # +0 / -0 are the same value
    diff &= ~((w8 & 0x7F == 0) & (cast & 0x7F == 0))
    assert not bool((diff & ~near).any()), \
        f"quant N{N} K{K}: {int((diff & ~near).sum())} codes differ away " \
        "from a rounding boundary"
    assert float(near.float().mean()) <= 1e-3, "near-boundary cap (0.1 %)"
