"""Case tables, input builders, fp64 references and per-element bounds for
the prefill path: the MFMA attention kernels (k_attn_prefill<D>,
k_attn_prefill_kv8<D>), k_rope_kv_prefill and the row-wise / element-wise
kernels (k_rmsnorm, k_add_rmsnorm, k_add_layernorm, k_swiglu, k_gelu).

Shared by test_prefill_shapes_gpu.py (device "cuda:0", the HIP kernels) and
test_prefill_shapes_cpu.py (device "cpu", where fei_amd.ops dispatches to the
fp32 torch reference, plus a torch model of the attention kernel's arithmetic
and its mutants). Same conventions as decode_shape_cases.py: inputs are CPU
f32 masters holding bf16-representable values, every reference is fp64
arithmetic on exactly those values, the bounds are the ones derived in
docs/TESTING.md ("Prefill shape tests").
"""

import functools
import math

import torch

from fei_amd import ops
from fei_amd.ops import reference as ref

from decode_shape_cases import (F64, NAN, assert_within, bf16r, bits, put,
                                rope64, rope_tab, ulp)

INF = float("inf")


# ===========================================================================
# Prefill attention
# ===========================================================================

B, HQ, MS = 2, 8, 320            # MS: cache rows per (sequence, kv head)
QT = KT = 64                     # q rows per workgroup / keys per LDS tile
GD_PAIRS = [(g, d) for g in (1, 2, 4, 8) for d in (64, 128)]
G3_PAIRS = [(3, 64), (3, 128)]   # Hq = 6, Hkv = 2: the kernel has no G template

# (S, (pos0 of sequence 0, of sequence 1)): the diagonal of row s is key
# pos0 + s; wave w owns rows 16w .. 16w+15 of a 64-row q tile.
CAUSAL_CASES = [
    (1, (0, 37)),      # one row; sequence 0 attends key 0 alone
    (3, (1, 63)),      # seq 1: diagonals 63 / 64 / 65 (key-tile edge), rows 0-2
    (4, (64, 15)),     # one full C-row group; seq 1: diagonals 15 / 16 / 17
    (5, (130, 1)),     # C-row group + 1; seq 0 starts in the third key tile
    (15, (0, 37)),     # wave 0 short by one row
    (16, (1, 63)),     # wave 0 full; seq 0: last row of wave 0 on diagonal 16
    (17, (64, 15)),    # wave 1 with one row; seq 1: its first row on 31
    (17, (0, 37)),     # seq 0: last row of wave 0 on 15, first of wave 1 on 16
    (33, (1, 63)),     # seq 0: first row of wave 1 on 17, last on 32, wave 2 on 33
    (63, (0, 37)),     # q tile short by one row; seq 0: last row of wave 1 on 31,
                       # first of wave 2 on 32
    (64, (1, 63)),     # q tile full; seq 0: last row of wave 3 on 64;
                       # seq 1: last row of wave 3 on 126, kv_end = 127
    (65, (64, 15)),    # second workgroup with one row; seq 0: last row of
                       # wave 3 on 127, row 64 (tile 1, wave 0) on 128;
                       # seq 1: first row of wave 3 on 63
    (65, (0, 37)),     # seq 0: last row of wave 3 on 63, row 64 on 64
    (65, (MS - 65, 2)),  # pos0 + S == max_seq exactly (seq 0)
    (129, (0, 37)),    # three q tiles; seq 0: rows 127 / 128 on 127 / 128
    (129, (1, 63)),    # seq 0: last row of wave 3, tile 1 on 128; seq 1: rows
                       # 64 / 65 on 127 / 128
    (129, (130, 1)),   # longest: kv_end = 259, five key tiles
]
# bidirectional (bf16 caches only): (S, kv_len per sequence); pos0 is set to
# BIDIR_POS0, non-zero and different from kv_len, and must be ignored
BIDIR_KV = [(33, 64), (1, 65), (64, 128), (0, 17)]
BIDIR_CASES = [(S, kv) for S in (33, 70) for kv in BIDIR_KV]
BIDIR_POS0 = (5, 9)

FORMS = [(kind, layout) for kind in ("bf16", "kv8")
         for layout in ("contig", "fused")]
MUTANTS = ("drop_diag", "future", "tile_first", "tile_last", "kvend0",
           "hkv_mod", "wave0", "nopad", "no_alpha")


def chosen_rows(S, p0):
    """q rows that follow planted keys: the first and last row of every wave,
    the last row, every row of one C-fragment group per q tile (rows 4..7 of
    wave 0), and the rows whose diagonal is the last key before / the first
    key after a 16-key chunk edge (which contains the 32- and 64-key ones)."""
    rows = {s for s in range(S) if s % 16 in (0, 15)} | {S - 1}
    rows |= {s for s in range(S) if s % QT in (4, 5, 6, 7)}
    rows |= {s for s in range(S) if (p0 + s) % 16 in (15, 0)}
    return sorted(rows)


def edge_keys(n):
    """Key 0 and the first and last key of every 64-key tile below n."""
    return sorted({k for t in range(0, n, KT) for k in (t, t + KT - 1) if k < n})


def causal_targets(S, p0, s):
    """What row s may follow: its diagonal key together with the key just
    past it, then each tile-edge key below the diagonal on its own."""
    d = p0 + s
    return [(d, d + 1)] + [(k,) for k in edge_keys(p0 + S) if k < d]


def bidir_targets(n):
    """Key 0, key n-1 and both sides of every 16-key chunk edge below n."""
    keys = {0, n - 1} | {k for k in range(n) if k % 16 in (15, 0)}
    return [(k,) for k in sorted(k for k in keys if 0 <= k < n)]


@functools.lru_cache(maxsize=None)
def _base(hkv, D):
    g = torch.Generator().manual_seed(2000 + 10 * hkv + D)
    K = bf16r(torch.randn(B, hkv, MS, D, generator=g))
    V = bf16r(torch.randn(B, hkv, MS, D, generator=g))
    q = bf16r(3.0 * torch.randn(B, 129, HQ, D, generator=g))
    sgn = torch.randint(0, 2, (B, hkv, MS, D), generator=g).float() * 2 - 1
    return K, V, q, sgn


def _ramps(b, hkv, P, D):
    """Asymmetric V ramps [hkv, len(P), D] of the planted keys P: distinct
    for neighbouring keys, for every kv head and for the two sequences."""
    p = torch.tensor(P).view(1, -1, 1)
    h = torch.arange(hkv).view(-1, 1, 1)
    amp = 0.5 + 0.25 * ((7 * p + 3 * h + 5 * b) % 13).float()
    sign = 1.0 - 2.0 * (p % 2).float()
    return bf16r(sign * (amp + torch.arange(D).float().view(1, 1, D) / D))


class AttnCase:
    """One (G, D, S, pos0 | kv_len, round) problem. K / V are the unpoisoned
    CPU masters [B, Hkv, MS, D] with the planted keys in place, q the roped
    queries [B, S, Hq, D]."""

    def __init__(self, G, D, S, pos0, rnd=0, kv_len=None, hq=HQ):
        self.G, self.D, self.S, self.rnd, self.hq = G, D, S, rnd, hq
        self.pos0, self.kv_len = tuple(pos0), kv_len
        self.causal = kv_len is None
        self.hkv = hkv = hq // G
        self.scale = float(torch.tensor(1.0 / math.sqrt(D)).float())
        K0, V0, q0, sgn = _base(hkv, D)
        K, V, q = K0.clone(), V0.clone(), q0[:, :S, :hq].clone()
        gamma = 30.0 / math.sqrt(D)
        self.followed = []                      # per sequence: {key tuples}
        self.planted = []
        for b in range(B):
            n = self.n(b)
            rows = chosen_rows(S, self.pos0[b] if self.causal else 0)
            tg = {s: (causal_targets(S, self.pos0[b], s) if self.causal
                      else bidir_targets(n)) for s in rows}
            P = sorted({k for T in tg.values() for t in T for k in t if k < n})
            self.planted.append(P)
            if P:
                K[b, :, P] = sgn[b, :, P]
                V[b, :, P] = _ramps(b, hkv, P, D)
            si, hi, ki = [], [], []
            seen = set()
            for j, s in enumerate(rows):
                T = tg[s]
                for h in range(hq):
                    if not T:
                        continue
                    off = 0 if self.causal else 3 * j
                    t = T[(h + 8 * rnd + off) % len(T)]
                    seen.add((s, t))
                    for k in t:
                        if k < n:
                            si.append(s), hi.append(h), ki.append(k)
            self.followed.append(seen)
            if si:
                si, hi, ki = (torch.tensor(x) for x in (si, hi, ki))
                q[b].index_put_((si, hi), gamma * sgn[b, hi // G, ki],
                                accumulate=True)
        self.K, self.V, self.q = K, V, bf16r(q)
        self._kv8 = None
        self._ref = {}

    def n(self, b):
        """Valid cache rows of sequence b."""
        return self.pos0[b] + self.S if self.causal else self.kv_len[b]

    def name(self):
        tail = f"pos0{self.pos0}" if self.causal else f"kv_len{self.kv_len}"
        return f"G{self.G} D{self.D} S{self.S} {tail} round{self.rnd}"

    @staticmethod
    def rounds(S, pos0, kv_len=None):
        """Launches needed so that every chosen row follows each of its
        targets with some head."""
        m = 1
        for b in range(B):
            if kv_len is None:
                m = max([m] + [len(causal_targets(S, pos0[b], s))
                               for s in chosen_rows(S, pos0[b])])
            else:
                m = max(m, len(bidir_targets(kv_len[b])))
        return -(-m // HQ)

    # -- what the kernel is given ------------------------------------------

    def quant(self):
        """(K codes, K scales, V codes, V scales) of the masters, and the
        values the kv8 kernel stages: bf16(f32(code) * scale)."""
        if self._kv8 is None:
            kq, ks = ref.quant_kv_fp8(self.K)
            vq, vs = ref.quant_kv_fp8(self.V)
            deq = [bf16r(c.view(torch.float8_e4m3fn).float() * s.unsqueeze(-1))
                   for c, s in ((kq, ks), (vq, vs))]
            self._kv8 = (kq, ks, vq, vs, deq[0], deq[1])
        return self._kv8

    def masters(self, kind):
        if kind == "bf16":
            return self.K, self.V
        return self.quant()[4:]

    def poisoned(self, kind):
        """f32 [B+1, Hkv, MS, D] copies of what the kernel may read, NaN in
        every row >= n(b) and in the whole extra sequence."""
        out = []
        for m in self.masters(kind):
            t = torch.full((B + 1,) + tuple(m.shape[1:]), NAN)
            for b in range(B):
                t[b, :, :self.n(b)] = m[b, :, :self.n(b)]
            out.append(t)
        return out

    def caches(self, device, kind):
        if kind == "bf16":
            return tuple(put(t, device) for t in self.poisoned("bf16"))
        kq, ks, vq, vs = self.quant()[:4]
        res = []
        for c, s in ((kq, ks), (vq, vs)):
            data = torch.full((B + 1,) + tuple(c.shape[1:]), 0x7F,
                              dtype=torch.uint8)
            sc = torch.full((B + 1,) + tuple(s.shape[1:]), INF)
            for b in range(B):
                data[b, :, :self.n(b)] = c[b, :, :self.n(b)]
                sc[b, :, :self.n(b)] = s[b, :, :self.n(b)]
            res.append(ops.QuantKV(data.to(device), sc.to(device)))
        return tuple(res)

    def q_dev(self, device, layout, dtype=None):
        """contig: [B, S, Hq, D]. fused: the engine's view into a
        [B*S, (Hq + 2 Hkv) * D] qkv buffer whose k / v columns are NaN.
        Returns (q, buffer or None)."""
        if layout == "contig":
            return put(self.q, device, dtype), None
        W = (self.hq + 2 * self.hkv) * self.D
        buf = torch.full((B * self.S, W), NAN)
        buf[:, :self.hq * self.D] = self.q.reshape(B * self.S, -1)
        buf = put(buf, device, dtype)
        qv = buf.as_strided((B, self.S, self.hq, self.D),
                            (self.S * W, W, self.D, 1))
        return qv, buf

    # -- fp64 reference and bound --------------------------------------------

    def reference(self, kind):
        """fp64 softmax(q K^T scale + mask) V; bound = ulp(ref) + 2^-8 A_d +
        2^-13 max|V over the attended rows|, A_d = sum_i p_i |v_id|. (bf16
        keeps 8 significant bits: rounding p_i to nearest errs by up to
        2^-8 p_i, not 2^-9 — the kernel model in the CPU twin needs it.)"""
        if kind in self._ref:
            return self._ref[kind]
        Km, Vm = self.masters(kind)
        S, D, G, hkv = self.S, self.D, self.G, self.hkv
        out = torch.zeros(B, S, self.hq, D, dtype=F64)
        bound = torch.zeros_like(out)
        for b in range(B):
            n = self.n(b)
            if n == 0:
                continue                        # exact zeros, bound 0
            k, v = Km[b, :, :n].to(F64), Vm[b, :, :n].to(F64)
            qb = self.q[b].to(F64).view(S, hkv, G, D)
            s = torch.einsum("shgd,hnd->hgsn", qb, k) * self.scale
            # the bound's derivation assumes kv_end <= 1024 and |score| <= 64
            assert n <= 1024 and float(s.abs().max()) <= 64.0, self.name()
            vrow = v.abs().amax(-1)                             # [hkv, n]
            if self.causal:
                diag = self.pos0[b] + torch.arange(S)
                s = s.masked_fill(torch.arange(n).view(1, 1, 1, n)
                                  > diag.view(1, 1, S, 1), -INF)
                vmax = torch.cummax(vrow, dim=1).values[:, diag]    # [hkv, S]
            else:
                vmax = vrow.amax(1, keepdim=True).expand(hkv, S)
            p = torch.softmax(s, dim=-1)
            o = torch.einsum("hgsn,hnd->shgd", p, v).reshape(S, self.hq, D)
            A = torch.einsum("hgsn,hnd->shgd", p, v.abs()).reshape(S, self.hq, D)
            vm = vmax.t().repeat_interleave(G, dim=1).unsqueeze(-1)  # [S,Hq,1]
            out[b] = o
            bound[b] = ulp(o) + 2.0 ** -8 * A + 2.0 ** -13 * vm
        self._ref[kind] = (out, bound)
        return out, bound


def run_attn_form(case, kind, layout, device):
    what = f"{kind}/{layout} {case.name()}"
    # a CPU run of the fp8 form states the kernel's bf16 staging by dtype
    dt = torch.bfloat16 if (device == "cpu" and kind == "kv8") else None
    qd, buf = case.q_dev(device, layout, dt)
    guard = None if buf is None else buf.clone()
    Kd, Vd = case.caches(device, kind)
    pos0 = torch.tensor(case.pos0, dtype=torch.int32, device=device)
    kw = {}
    if not case.causal:
        kw = dict(causal=False, kv_len=torch.tensor(
            case.kv_len, dtype=torch.int32, device=device))
    out = ops.attn_prefill(qd, Kd, Vd, pos0, scale=case.scale, **kw)
    assert tuple(out.shape) == (B, case.S, case.hq, case.D), what
    if guard is not None:
        assert torch.equal(bits(guard), bits(buf)), f"{what}: qkv buffer written"
    want, bound = case.reference(kind)
    for b in range(B):
        if case.n(b) == 0:
            assert not bool(out[b].float().cpu().any()), \
                f"{what}: kv_len = 0 must give exact zeros"
    return assert_within(out, want, bound, what)


def run_causal_case(G, D, S, pos0, device, forms=FORMS, hq=HQ):
    for rnd in range(AttnCase.rounds(S, pos0)):
        case = AttnCase(G, D, S, pos0, rnd, hq=hq)
        for kind, layout in forms:
            run_attn_form(case, kind, layout, device)


def run_bidir_case(G, D, S, kv_len, device):
    for rnd in range(AttnCase.rounds(S, BIDIR_POS0, kv_len)):
        case = AttnCase(G, D, S, BIDIR_POS0, rnd, kv_len=kv_len)
        for layout in ("contig", "fused"):
            run_attn_form(case, "bf16", layout, device)


# -- a torch model of the kernel's arithmetic, and its mutants ----------------

def model_prefill(case, kind="bf16", mut=None):
    """k_attn_prefill's arithmetic in f32 torch: 64-row q tiles with clamped
    tail rows, 64-key tiles zero-padded past kv_end, online softmax with the
    running maximum, P rounded to bf16 per tile before PV, l summed from the
    unrounded P, f32 accumulation, bf16 output. Reads the POISONED caches, so
    anything it must not touch is NaN. mut names one deliberate defect."""
    assert mut is None or mut in MUTANTS, mut
    Kp, Vp = case.poisoned(kind)
    S, D, G, hkv, hq = case.S, case.D, case.G, case.hkv, case.hq
    heads = torch.arange(hq)
    hk = heads % hkv if mut == "hkv_mod" else heads // G
    out = torch.zeros(B, S, hq, D)
    r = torch.arange(QT)
    for b in range(B):
        p0 = case.pos0[b]
        bsrc = 0 if mut == "kvend0" else b
        for qt in range(-(-S // QT)):
            rel = qt * QT + r
            src = qt * QT + (r % 16) if mut == "wave0" else rel
            qa = case.q[b, src.clamp(max=S - 1)].transpose(0, 1)   # [hq,64,D]
            q_hi = min(qt * QT + QT, S)
            kv_end = (case.pos0[bsrc] + q_hi) if case.causal \
                else case.kv_len[bsrc]
            qabs = (p0 + rel).view(1, QT, 1)
            m = torch.full((hq, QT), -INF)
            l = torch.zeros(hq, QT)
            o = torch.zeros(hq, QT, D)
            for t in range(-(-kv_end // KT)):
                keys = t * KT + torch.arange(KT)
                ld = keys.clamp(max=MS - 1)
                kt, vt = Kp[b][:, ld].clone(), Vp[b][:, ld].clone()
                if mut != "nopad":
                    kt[:, keys >= kv_end] = 0
                    vt[:, keys >= kv_end] = 0
                s = torch.einsum("hrd,hkd->hrk", qa, kt[hk]) * case.scale
                kk = keys.view(1, 1, KT)
                mask = (kk >= kv_end).expand(1, QT, KT)
                if case.causal:
                    if mut == "drop_diag":
                        mask = mask | (kk >= qabs)
                    elif mut == "future":
                        mask = mask | (kk > qabs + 1)
                    else:
                        mask = mask | (kk > qabs)
                if mut == "tile_first":
                    mask = mask | (kk % KT == 0)
                if mut == "tile_last":
                    mask = mask | (kk % KT == KT - 1)
                s = torch.where(mask, torch.tensor(-INF), s)
                m_new = torch.maximum(m, s.amax(-1))
                alpha = torch.exp(m - m_new)
                p = torch.where(mask, torch.tensor(0.0),
                                torch.exp(s - m_new.unsqueeze(-1)))
                l = l * alpha + p.sum(-1)
                if mut != "no_alpha":
                    o = o * alpha.unsqueeze(-1)
                o = o + torch.einsum("hrk,hkd->hrd", bf16r(p), vt[hk])
                m = m_new
            inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
            res = bf16r(o * inv.unsqueeze(-1))
            nv = q_hi - qt * QT
            out[b, qt * QT: q_hi] = res[:, :nv].transpose(0, 1)
    return out


def check_model(case, kind="bf16", mut=None):
    """Bound check of the model's output; raises AssertionError outside."""
    want, bound = case.reference(kind)
    return assert_within(model_prefill(case, kind, mut), want, bound,
                         f"model[{mut}] {kind} {case.name()}")


# ===========================================================================
# k_rope_kv_prefill
# ===========================================================================

ROPE_CASES = [(D, hq, hkv, S, pos0)
              for D in (64, 128) for hq, hkv in ((8, 2), (4, 4))
              for S, pos0 in ((1, (0, 5)), (7, (0, 5)), (33, (MS - 33, 1)))]


def run_rope_case(D, hq, hkv, S, pos0, layout, device):
    what = f"rope_kv_prefill D{D} Hq{hq} Hkv{hkv} S{S} pos0{pos0} {layout}"
    g = torch.Generator().manual_seed(D + 7 * hq + 13 * S)
    q = bf16r(torch.randn(B, S, hq, D, generator=g))
    k = bf16r(torch.randn(B, S, hkv, D, generator=g))
    v = bf16r(torch.randn(B, S, hkv, D, generator=g))
    if layout == "contig":
        qd, kd, vd = put(q, device), put(k, device), put(v, device)
        buf = None
    else:
        W = (hq + 2 * hkv) * D
        buf = put(torch.cat([t.reshape(B * S, -1) for t in (q, k, v)], dim=1),
                  device)
        so = buf.storage_offset()

        def view(h, off):
            return buf.as_strided((B, S, h, D), (S * W, W, D, 1), so + off)
        qd, kd, vd = view(hq, 0), view(hkv, hq * D), view(hkv, (hq + hkv) * D)
        guard = buf.clone()
    Kc = put(torch.full((B + 1, hkv, MS, D), NAN), device)      # canaries
    Vc = Kc.clone()
    before = (Kc.clone(), Vc.clone())
    pos0d = torch.tensor(pos0, dtype=torch.int32, device=device)
    ret = ops.rope_kv_prefill(qd, kd, vd, Kc, Vc, pos0d,
                              rope_tab(D).to(device))
    assert ret.data_ptr() == qd.data_ptr(), f"{what}: q is roped in place"
    # everything outside the S appended rows is bit-equal
    for old, new in zip(before, (Kc, Vc)):
        a, c = old.clone(), new.clone()
        for b in range(B):
            a[b, :, pos0[b]:pos0[b] + S] = 0
            c[b, :, pos0[b]:pos0[b] + S] = 0
        assert torch.equal(bits(a), bits(c)), \
            f"{what}: wrote outside the appended rows"
    pos = (torch.tensor(pos0).view(B, 1) + torch.arange(S).view(1, S)).reshape(-1)
    for b in range(B):
        vnew = Vc[b, :, pos0[b]:pos0[b] + S].detach().cpu().float()
        assert torch.equal(vnew, v[b].transpose(0, 1)), f"{what}: appended V"
    knew = torch.stack([Kc[b, :, pos0[b]:pos0[b] + S].transpose(0, 1)
                        for b in range(B)]).detach().cpu().float()
    want_k = rope64(k.reshape(B * S, hkv, D), pos).view(B, S, hkv, D)
    assert_within(knew, want_k, ulp(want_k), f"{what}: appended K")
    want_q = rope64(q.reshape(B * S, hq, D), pos).view(B, S, hq, D)
    assert_within(qd, want_q, ulp(want_q), f"{what}: roped q")
    if buf is not None:
        assert torch.equal(bits(buf[:, hq * D:]), bits(guard[:, hq * D:])), \
            f"{what}: k / v columns of the qkv buffer changed"


# ===========================================================================
# Row-wise and element-wise kernels
# ===========================================================================

# cols 8: 255 idle threads; 2048: one vector per thread; 2056: second trip of
# the vector loop; rows 2049 > the 2048-block grid: grid-stride and red[] reuse
ROW_SHAPES = [(r, c) for c in (8, 264, 2048, 2056, 4096) for r in (1, 3)] \
    + [(2049, 8)]
EPS = 1e-5
EPS32 = float(torch.tensor(EPS).float())
RES_TIE_CAP = 8
LN_KINDS = ("plain", "res", "mean8", "res_cancel")
# > 2048 * 256 vectors of 8: the grid-stride loop of k_swiglu / k_gelu runs
BIG_ROWS, BIG_INTER = 1025, 4104
ELT_SHAPES = [(3, 8), (BIG_ROWS, BIG_INTER)]
assert BIG_ROWS * (BIG_INTER // 8) > 2048 * 256


def bf16_from64(t):
    """fp64 -> nearest bf16 value (ties to even) in ONE rounding."""
    u = ulp(t)
    return torch.round(t / u) * u


def _row_inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed + 31 * rows + cols)
    amp = 0.5 + (torch.arange(rows) % 3).float()[:, None]     # distinct rows
    x = bf16r(amp * torch.randn(rows, cols, generator=g))
    w = bf16r(1.0 + 0.5 * torch.randn(cols, generator=g))
    return x, w, g


def rms_ref(x64, w64):
    """ulp(ref) + |ref| (cols 2^-24 + 2^-21): f32 sum of cols non-negative
    squares, one rsqrtf, two multiplies."""
    cols = x64.shape[-1]
    inv = 1.0 / torch.sqrt((x64 * x64).mean(-1, keepdim=True) + EPS32)
    want = x64 * inv * w64
    return want, ulp(want) + want.abs() * (cols * 2.0 ** -24 + 2.0 ** -21)


def run_rmsnorm_case(rows, cols, device):
    x, w, _ = _row_inputs(rows, cols, 1)
    out = ops.rmsnorm(put(x, device), put(w, device), EPS)
    assert tuple(out.shape) == (rows, cols)
    want, bound = rms_ref(x.to(F64), w.to(F64))
    return assert_within(out, want, bound, f"rmsnorm {rows}x{cols}")


def run_add_rmsnorm_case(rows, cols, device):
    what = f"fused_add_rmsnorm {rows}x{cols}"
    x, w, g = _row_inputs(rows, cols, 2)
    res = bf16r(torch.randn(rows, cols, generator=g))
    if cols >= 16:
        # summands 2^17 .. 2^24 apart: the f32 add itself rounds
        res[:, 3] = bf16r(x[:, 3] * 2.0 ** -20)
        x[:, 5] = bf16r(res[:, 5] * 2.0 ** -17)
    # the op's semantics include the bf16 rounding of the sum: bf16 on the CPU
    bf = torch.bfloat16
    xd, rd, wd = put(x, device, bf), put(res, device, bf), put(w, device, bf)
    out, newres = ops.fused_add_rmsnorm(xd, rd, wd, EPS)
    assert newres.data_ptr() == rd.data_ptr(), f"{what}: not in place"
    s = res.to(F64) + x.to(F64)                     # exact in fp64
    want_res = bf16_from64(s)
    u = ulp(s)
    frac = s.abs() / u
    frac = frac - torch.floor(frac)
    # the f32 sum can round twice only where it is inexact AND the exact sum
    # sits within relative 2^-20 of a bf16 rounding boundary
    near = ((frac - 0.5).abs() * u <= 2.0 ** -20 * s.abs()) \
        & (s.float().to(F64) != s)
    assert int(near.sum(-1).max()) <= RES_TIE_CAP, \
        f"{what}: near-tie cap {near.sum(-1).max()} (pick another seed)"
    got_res = newres.detach().cpu().to(F64)
    diff = (got_res - want_res).abs()
    assert bool((diff[~near] == 0).all()), \
        f"{what}: {int((diff[~near] != 0).sum())} residual elements differ"
    assert bool((diff[near] <= ulp(want_res)[near]).all()), what
    # norm output: against the residual the kernel itself left
    want, bound = rms_ref(got_res, w.to(F64))
    return assert_within(out, want, bound, what)


def run_layernorm_case(rows, cols, kind, device):
    """ulp(ref) + |w| (|x-mean| (cols 2^-24 + 2^-21) + (|x|+|mean|) 2^-23)
    inv_std, x the (x + residual) sum."""
    what = f"layernorm {kind} {rows}x{cols}"
    x, w, g = _row_inputs(rows, cols, 3 + LN_KINDS.index(kind))
    bias = bf16r(0.1 * torch.randn(cols, generator=g))
    res = None
    if kind == "res":
        res = bf16r(torch.randn(rows, cols, generator=g))
    elif kind == "mean8":                 # a one-pass variance would fail
        x = bf16r(8.0 + torch.randn(rows, cols, generator=g))
    elif kind == "res_cancel":            # the sum is near zero
        res = bf16r(-x + 2.0 ** -6 * torch.randn(rows, cols, generator=g))
    out = ops.layernorm(put(x, device), put(w, device), put(bias, device), EPS,
                        residual=None if res is None else put(res, device))
    assert tuple(out.shape) == (rows, cols)
    s = x.to(F64) if res is None else x.to(F64) + res.to(F64)
    mean = s.mean(-1, keepdim=True)
    inv = 1.0 / torch.sqrt(((s - mean) ** 2).mean(-1, keepdim=True) + EPS32)
    w64 = w.to(F64)
    want = (s - mean) * inv * w64 + bias.to(F64)
    bound = ulp(want) + w64.abs() * inv * (
        (s - mean).abs() * (cols * 2.0 ** -24 + 2.0 ** -21)
        + (s.abs() + mean.abs()) * 2.0 ** -23)
    return assert_within(out, want, bound, what)


def run_swiglu_case(rows, inter, device):
    """ulp(ref) + 2^-20 |ref| with exact g, u."""
    g = torch.Generator().manual_seed(rows + inter)
    gu = bf16r((2.0 * torch.randn(rows, 2 * inter, generator=g)).clamp(-8, 8))
    out = ops.swiglu(put(gu, device))
    assert tuple(out.shape) == (rows, inter)
    g64, u64 = gu[:, :inter].to(F64), gu[:, inter:].to(F64)
    want = g64 * torch.sigmoid(g64) * u64
    return assert_within(out, want, ulp(want) + 2.0 ** -20 * want.abs(),
                         f"swiglu {rows}x{inter}")


GELU_SPECIAL = [0.0, -0.0, 8.5, -8.5, 20.0, -20.0, 100.0, -100.0] \
    + [-3.0 - 3.0 * i / 15 for i in range(16)]


def run_gelu_case(rows, cols, device):
    """ulp(ref) + 2^-23 |x|: for x <~ -3 the kernel forms 1 + erf(.) in f32,
    and what is bounded is its absolute error."""
    g = torch.Generator().manual_seed(rows * 3 + cols)
    x = bf16r(2.0 * torch.randn(rows, cols, generator=g))
    sp = bf16r(torch.tensor(GELU_SPECIAL))
    flat = x.view(-1)
    k = min(len(sp), flat.numel() // 2)
    flat[:k] = sp[:k]                       # first vectors
    flat[-k:] = sp[-k:]                     # the last vector(s)
    out = ops.gelu(put(x, device))
    assert tuple(out.shape) == (rows, cols)
    x64 = x.to(F64)
    want = 0.5 * x64 * torch.special.erfc(-x64 / math.sqrt(2.0))
    return assert_within(out, want, ulp(want) + 2.0 ** -23 * x64.abs(),
                         f"gelu {rows}x{cols}")


# -- refusals and empties ------------------------------------------------------

def _t(device, *shape):
    dt = torch.bfloat16 if device != "cpu" else torch.float32
    return torch.zeros(*shape, dtype=dt, device=device)


def _q8(device, *shape):
    return ops.QuantKV.zeros(shape, device)


def refusals(device):
    """(name, thunk): every thunk must raise ValueError before any launch."""
    pos0 = torch.zeros(1, dtype=torch.int32, device=device)
    w = _t(device, 12)
    strided = _t(device, 4, 32)[:, :16]
    return [
        ("attn_prefill Hq=6 Hkv=4, bf16 caches", lambda: ops.attn_prefill(
            _t(device, 1, 4, 6, 64), _t(device, 1, 4, 16, 64),
            _t(device, 1, 4, 16, 64), pos0)),
        ("attn_prefill Hq=6 Hkv=4, QuantKV", lambda: ops.attn_prefill(
            _t(device, 1, 4, 6, 64), _q8(device, 1, 4, 16, 64),
            _q8(device, 1, 4, 16, 64), pos0)),
        ("rmsnorm cols=12", lambda: ops.rmsnorm(_t(device, 2, 12), w)),
        ("fused_add_rmsnorm cols=12", lambda: ops.fused_add_rmsnorm(
            _t(device, 2, 12), _t(device, 2, 12), w)),
        ("fused_add_rmsnorm strided residual", lambda: ops.fused_add_rmsnorm(
            _t(device, 4, 16), strided, _t(device, 16))),
        ("layernorm cols=12", lambda: ops.layernorm(_t(device, 2, 12), w, w)),
        ("swiglu inter=12", lambda: ops.swiglu(_t(device, 2, 24))),
        ("gelu numel=12", lambda: ops.gelu(_t(device, 3, 4))),
    ]


def gpu_refusals(device):
    """Refusals of a missing kernel instance: the fp32 reference has no such
    limit (the tiny CPU models use D = 32), so these hold on the GPU only."""
    pos0 = torch.zeros(1, dtype=torch.int32, device=device)
    return [
        ("attn_prefill D=32, bf16 caches", lambda: ops.attn_prefill(
            _t(device, 1, 4, 4, 32), _t(device, 1, 2, 16, 32),
            _t(device, 1, 2, 16, 32), pos0)),
    ]


def run_empties(device):
    """Zero rows: an empty result of the right shape, nothing launched."""
    w = _t(device, 16)
    assert tuple(ops.rmsnorm(_t(device, 0, 16), w).shape) == (0, 16)
    res = _t(device, 0, 16)
    out, r2 = ops.fused_add_rmsnorm(_t(device, 0, 16), res, w)
    assert tuple(out.shape) == (0, 16) and r2 is res
    assert tuple(ops.layernorm(_t(device, 0, 16), w, w).shape) == (0, 16)
    assert tuple(ops.layernorm(_t(device, 0, 16), w, w,
                               residual=_t(device, 0, 16)).shape) == (0, 16)
    assert tuple(ops.swiglu(_t(device, 0, 32)).shape) == (0, 16)
    assert tuple(ops.swiglu(_t(device, 2, 0, 32)).shape) == (2, 0, 16)
    assert tuple(ops.gelu(_t(device, 0, 16)).shape) == (0, 16)
