"""Pure-PyTorch reference implementations of every engine op.

These define the *semantics* each HIP kernel must reproduce:
  - used directly on CPU (tests, tiny models, gloo multi-process tests)
  - GPU numerics tests compare the HIP kernels against these in fp32
    (tests/test_ops_gpu.py)

Shapes use B=batch, S=sequence, H/Hq/Hkv=heads, D=head_dim, C=hidden.
KV caches are contiguous ``[B, Hkv, max_seq, D]``.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch


# -- normalisation -----------------------------------------------------------

def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """RMSNorm over the last dim; accumulate in fp32, output in x.dtype."""
    xf = x.float()
    var = xf.pow(2).mean(dim=-1, keepdim=True)
    out = xf * torch.rsqrt(var + eps) * weight.float()
    return out.to(x.dtype)


def fused_add_rmsnorm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5
) -> Tuple[torch.Tensor, torch.Tensor]:
    """residual = residual + x (in fp32, rounded back); out = rmsnorm(residual).
    Returns (out, new_residual)."""
    new_res = (residual.float() + x.float()).to(x.dtype)
    return rmsnorm(new_res, weight, eps), new_res


# -- rotary embeddings -------------------------------------------------------

def rope_table(max_seq: int, dim: int, theta: float = 500000.0,
               device=None) -> torch.Tensor:
    """[max_seq, dim/2, 2] fp32 cos/sin table (half-split RoPE: pairs are
    (x[i], x[i + dim/2]) — Llama convention)."""
    inv = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float32,
                                        device=device) / dim))
    t = torch.arange(max_seq, dtype=torch.float32, device=device)
    freqs = torch.outer(t, inv)                      # [max_seq, dim/2]
    return torch.stack([freqs.cos(), freqs.sin()], dim=-1).contiguous()


def apply_rope(x: torch.Tensor, positions: torch.Tensor,
               table: torch.Tensor) -> torch.Tensor:
    """x: [..., S, H, D] or [..., H, D]; positions: [...,(S)] int.
    Half-split pairing: (x[:d/2], x[d/2:])."""
    D = x.shape[-1]
    cs = table[positions]                            # [..., D/2, 2]
    cos, sin = cs[..., 0], cs[..., 1]                # [..., D/2]
    cos = cos.unsqueeze(-2)                          # broadcast over heads
    sin = sin.unsqueeze(-2)
    x1 = x[..., : D // 2].float()
    x2 = x[..., D // 2:].float()
    o1 = x1 * cos - x2 * sin
    o2 = x2 * cos + x1 * sin
    return torch.cat([o1, o2], dim=-1).to(x.dtype)


def rope_kv_decode(
    q: torch.Tensor,            # [B, Hq, D] (modified logically; returns new)
    k: torch.Tensor,            # [B, Hkv, D]
    v: torch.Tensor,            # [B, Hkv, D]
    k_cache: torch.Tensor,      # [B, Hkv, max_seq, D]
    v_cache: torch.Tensor,
    pos: torch.Tensor,          # [B] int32 — write position (= current length)
    table: torch.Tensor,
) -> torch.Tensor:
    """Apply RoPE to q,k at pos; write k,v into the caches. Returns roped q."""
    q_out = apply_rope(q, pos, table)                # positions broadcast per batch
    k_rot = apply_rope(k, pos, table)
    B = q.shape[0]
    for b in range(B):
        p = int(pos[b])
        k_cache[b, :, p, :] = k_rot[b]
        v_cache[b, :, p, :] = v[b]
    return q_out


def rope_kv_prefill(
    q: torch.Tensor,            # [B, S, Hq, D]
    k: torch.Tensor,            # [B, S, Hkv, D]
    v: torch.Tensor,            # [B, S, Hkv, D]
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    pos0: torch.Tensor,         # [B] int32 — first absolute position
    table: torch.Tensor,
) -> torch.Tensor:
    B, S = q.shape[0], q.shape[1]
    positions = pos0.view(B, 1).long() + torch.arange(S, device=q.device).view(1, S)
    q_out = apply_rope(q, positions, table)
    k_rot = apply_rope(k, positions, table)
    for b in range(B):
        p = int(pos0[b])
        k_cache[b, :, p:p + S, :] = k_rot[b].transpose(0, 1)
        v_cache[b, :, p:p + S, :] = v[b].transpose(0, 1)
    return q_out


# -- attention ---------------------------------------------------------------

def attn_decode(
    q: torch.Tensor,            # [B, Hq, D] (already roped)
    k_cache: torch.Tensor,      # [B, Hkv, max_seq, D]
    v_cache: torch.Tensor,
    seqlen: torch.Tensor,       # [B] int32 — number of valid cache entries
    scale: Optional[float] = None,
) -> torch.Tensor:
    """Single-token GQA attention over the cache. Returns [B, Hq, D]."""
    B, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    scale = scale or 1.0 / math.sqrt(D)
    out = torch.empty_like(q)
    for b in range(B):
        n = int(seqlen[b])
        k = k_cache[b, :, :n, :].float()             # [Hkv, n, D]
        v = v_cache[b, :, :n, :].float()
        qb = q[b].float().view(Hkv, G, D)            # [Hkv, G, D]
        s = torch.einsum("hgd,hnd->hgn", qb, k) * scale
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgn,hnd->hgd", p, v)
        out[b] = o.reshape(Hq, D).to(q.dtype)
    return out


def attn_prefill(
    q: torch.Tensor,            # [B, S, Hq, D] (already roped)
    k_cache: torch.Tensor,      # [B, Hkv, max_seq, D] (k/v already appended)
    v_cache: torch.Tensor,
    pos0: torch.Tensor,         # [B] int32 — q token s sits at pos0+s
    scale: Optional[float] = None,
) -> torch.Tensor:
    """Causal GQA prefill attention over the cache. q token s attends cache
    positions [0, pos0+s]. Returns [B, S, Hq, D]."""
    B, S, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    scale = scale or 1.0 / math.sqrt(D)
    out = torch.empty_like(q)
    for b in range(B):
        p0 = int(pos0[b])
        n = p0 + S
        k = k_cache[b, :, :n, :].float()             # [Hkv, n, D]
        v = v_cache[b, :, :n, :].float()
        qb = q[b].float().view(S, Hkv, G, D)
        s = torch.einsum("shgd,hnd->hgsn", qb, k) * scale
        key_pos = torch.arange(n, device=q.device).view(1, 1, 1, n)
        q_pos = (p0 + torch.arange(S, device=q.device)).view(1, 1, S, 1)
        s = s.masked_fill(key_pos > q_pos, float("-inf"))
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgsn,hnd->shgd", p, v)
        out[b] = o.reshape(S, Hq, D).to(q.dtype)
    return out


# -- encoder ops (BERT/bge architecture) --------------------------------------

def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              eps: float = 1e-5,
              residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(x [+ residual]) -> LayerNorm over the last dim; f32 stats."""
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
    mean = xf.mean(dim=-1, keepdim=True)
    var = (xf - mean).pow(2).mean(dim=-1, keepdim=True)
    out = (xf - mean) * torch.rsqrt(var + eps) * weight.float() + bias.float()
    return out.to(x.dtype)


def gelu(x: torch.Tensor) -> torch.Tensor:
    """Exact (erf) GELU."""
    return torch.nn.functional.gelu(x.float()).to(x.dtype)


# -- MLP ---------------------------------------------------------------------

def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    """gate_up: [..., 2*inter] (gate first half, up second). silu(g)*u."""
    inter = gate_up.shape[-1] // 2
    g = gate_up[..., :inter].float()
    u = gate_up[..., inter:].float()
    return (torch.nn.functional.silu(g) * u).to(gate_up.dtype)


# -- sampling ----------------------------------------------------------------

def argmax_sample(logits: torch.Tensor) -> torch.Tensor:
    """Greedy: [B, V] -> [B] int32."""
    return logits.float().argmax(dim=-1).to(torch.int32)


def gumbel_sample(logits: torch.Tensor, temperature: float,
                  generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Exact categorical sampling via the Gumbel-max trick:
    argmax(logits/T + G) with G ~ Gumbel(0,1)."""
    if temperature <= 0:
        return argmax_sample(logits)
    u = torch.rand(logits.shape, device=logits.device, dtype=torch.float32,
                   generator=generator).clamp_(1e-10, 1.0)
    g = -torch.log(-torch.log(u))
    return (logits.float() / temperature + g).argmax(dim=-1).to(torch.int32)


def topk_mask(logits: torch.Tensor, k: int) -> torch.Tensor:
    """Mask all but the top-k logits to -inf."""
    if k <= 0 or k >= logits.shape[-1]:
        return logits
    kth = torch.topk(logits.float(), k, dim=-1).values[..., -1:]
    return logits.masked_fill(logits.float() < kth, float("-inf"))


def topp_mask(logits: torch.Tensor, p: float) -> torch.Tensor:
    """Nucleus mask: keep the smallest prefix of sorted probs with mass >= p."""
    if p >= 1.0:
        return logits
    sorted_logits, idx = torch.sort(logits.float(), descending=True, dim=-1)
    probs = torch.softmax(sorted_logits, dim=-1)
    cum = probs.cumsum(dim=-1)
    keep = cum - probs < p                           # always keep the first
    masked = sorted_logits.masked_fill(~keep, float("-inf"))
    out = torch.full_like(masked, float("-inf"))
    out.scatter_(-1, idx, masked)
    return out.to(logits.dtype)


def filter_keep(logits: torch.Tensor, top_k: int = 0, top_p: float = 1.0
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Tie-inclusive top-k / top-p keep set, computed in fp64 on the exact
    input values (so it does not depend on any sort order).

    Order as in the eager path: top-k first, then top-p, both on the RAW
    logits (temperature applies only at the draw).
      top-k (0 < k < V): tau_k = k-th largest value counting multiplicity,
        K = {i : x_i >= tau_k}; otherwise K is everything.
      top-p (p < 1): q_i = exp(x_i - max) / sum_K; a value group v of K is
        kept iff above(v) = sum_{i in K, x_i > v} q_i < p (the max group is
        therefore always kept).
    Equals topk_mask -> topp_mask except inside the boundary tie group,
    which is kept whole here.

    Returns (keep [B,V] bool, thr [B] f32 = smallest kept value,
    count [B] i32 = number of kept tokens), on the CPU."""
    x = logits.detach().to("cpu").to(torch.float64)
    B, V = x.shape
    if 0 < top_k < V:
        tau = torch.topk(x, top_k, dim=-1).values[:, -1:]
        keep = x >= tau
    else:
        keep = torch.ones(B, V, dtype=torch.bool)
    if top_p < 1.0:
        for b in range(B):
            vals, counts = torch.unique(x[b][keep[b]], return_counts=True)
            vals, counts = vals.flip(0), counts.flip(0)      # descending
            w = torch.exp(vals - vals[0]) * counts.to(torch.float64)
            above = (w.cumsum(0) - w) / w.sum()
            kept_vals = vals[above < top_p]
            keep[b] &= x[b] >= kept_vals[-1]
    thr = torch.where(keep, x, torch.full_like(x, float("inf"))).amin(dim=-1)
    return keep, thr.to(torch.float32), keep.sum(dim=-1).to(torch.int32)


# -- fp8 weight quantization (OCP e4m3fn; decode-path serving mode) ----------

def quant_fp8(w: torch.Tensor):
    """Per-output-row absmax/448 scaling + e4m3fn encode.
    Returns (w8 uint8 [N,K], scales fp32 [N])."""
    wf = w.float()
    amax = wf.abs().amax(dim=-1).clamp_min(1e-12)
    scales = amax / 448.0
    q = (wf / scales.unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scales


def dequant_fp8(w8: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    return w8.view(torch.float8_e4m3fn).float() * scales.unsqueeze(-1).float()


# -- fp8 KV cache (OCP e4m3fn, one f32 scale per cached row) -----------------
#
# THE definition of the storage format; csrc/kv_fp8.hip matches it bit for
# bit. A cached row = the D elements of one (batch, kv-head, position):
#   data  uint8   [B, Hkv, max_seq, D]   e4m3fn codes
#   scale float32 [B, Hkv, max_seq]      amax/448, or 1 for an all-zero row
#   code = e4m3fn(x / scale): IEEE f32 division, round-to-nearest-even,
#   saturating at +-448 (|x / scale| <= 448 up to one rounding, so the cast
#   never reaches the NaN codes 0x7F / 0xFF).
# x is the value the unquantised cache would have stored (bf16 on the GPU
# path: K after RoPE and bf16 rounding; fp32 on the CPU engine).

def quant_kv_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., D] -> (codes uint8 [..., D], scales f32 [...]). quant_fp8 on
    each row; differs from it only in the scale REPORTED for an all-zero
    row (1 instead of quant_fp8's clamp floor — the codes are 0 either way)."""
    D = x.shape[-1]
    rows = x.reshape(-1, D)
    codes, scales = quant_fp8(rows)
    zero = rows.float().abs().amax(dim=-1) == 0
    scales = torch.where(zero, torch.ones_like(scales), scales)
    return codes.view(x.shape), scales.view(x.shape[:-1])


def dequant_kv_fp8(data: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """(codes [..., D], scales [...]) -> f32 [..., D]."""
    return data.view(torch.float8_e4m3fn).float() * scale.float().unsqueeze(-1)


def rope_kv_decode_fp8(q, k, v, k_data, k_scale, v_data, v_scale, pos,
                       table) -> torch.Tensor:
    """rope_kv_decode into an fp8 cache: the roped k (rounded to k.dtype, as
    the unquantised cache would store it) and v are quantised per row and
    written at pos[b]. Returns roped q."""
    q_out = apply_rope(q, pos, table)
    kq, ks = quant_kv_fp8(apply_rope(k, pos, table))
    vq, vs = quant_kv_fp8(v)
    for b in range(q.shape[0]):
        p = int(pos[b])
        k_data[b, :, p, :] = kq[b]
        k_scale[b, :, p] = ks[b]
        v_data[b, :, p, :] = vq[b]
        v_scale[b, :, p] = vs[b]
    return q_out


def rope_kv_prefill_fp8(q, k, v, k_data, k_scale, v_data, v_scale, pos0,
                        table) -> torch.Tensor:
    """rope_kv_prefill into an fp8 cache (rows pos0[b] .. pos0[b]+S-1)."""
    B, S = q.shape[0], q.shape[1]
    positions = pos0.view(B, 1).long() + torch.arange(S, device=q.device).view(1, S)
    q_out = apply_rope(q, positions, table)
    kq, ks = quant_kv_fp8(apply_rope(k, positions, table))   # [B,S,Hkv,D]
    vq, vs = quant_kv_fp8(v)
    for b in range(B):
        p = int(pos0[b])
        k_data[b, :, p:p + S, :] = kq[b].transpose(0, 1)
        k_scale[b, :, p:p + S] = ks[b].transpose(0, 1)
        v_data[b, :, p:p + S, :] = vq[b].transpose(0, 1)
        v_scale[b, :, p:p + S] = vs[b].transpose(0, 1)
    return q_out


def hash_gumbel(B: int, v_local: int, v_offset: int, seed: int,
                step: int) -> torch.Tensor:
    """CPU replica of the GPU sampler's per-element Gumbel noise
    (fei_common.h hash_uniform: splitmix64 -> 24-bit uniform in (0,1]),
    keyed by (seed, step, batch row, GLOBAL vocab index) — so the
    tensor-parallel shard sampler matches the full sampler bit-for-bit
    in its noise stream."""
    import numpy as np

    idx = np.arange(v_offset, v_offset + v_local, dtype=np.uint64)
    out = np.empty((B, v_local), dtype=np.float32)
    with np.errstate(over="ignore"):
        for b in range(B):
            x = (np.uint64(seed)
                 ^ (np.uint64(step) * np.uint64(0x51ED27F1))
                 ^ (np.uint64(b) << np.uint64(40))
                 ^ idx)
            x = x + np.uint64(0x9E3779B97F4A7C15)
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            x = x ^ (x >> np.uint64(31))
            m = (x >> np.uint64(40)).astype(np.float32)
            out[b] = (m + 1.0) * (1.0 / 16777216.0)
    u = torch.from_numpy(out)
    return -torch.log(-torch.log(u))


def score_topk(emb: torch.Tensor, q: torch.Tensor, k: int,
               mask: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k best eligible rows of emb [N, C] per query of q [Q, C]:
    (scores f32 [Q, k], rows int32 [Q, k]). Scores are
    ``emb.float() @ q.float().T``; rows are taken in the total order (score
    descending, then row ascending), which torch.topk does not promise on
    ties. ``mask`` [N]: non-zero rows are eligible (None: all). A NaN score
    counts as -inf. With fewer than k eligible rows the tail is (-inf, -1)."""
    N = emb.shape[0]
    Q = q.shape[0]
    scores = (emb.float() @ q.float().t()).t().contiguous()      # [Q, N]
    scores = torch.nan_to_num(scores, nan=float("-inf"),
                              posinf=float("inf"), neginf=float("-inf"))
    elig = torch.ones(N, dtype=torch.bool) if mask is None else mask != 0
    rows = torch.nonzero(elig).flatten()
    out_s = torch.full((Q, k), float("-inf"), dtype=torch.float32)
    out_i = torch.full((Q, k), -1, dtype=torch.int32)
    n = min(k, rows.numel())
    if n == 0:
        return out_s, out_i
    for u in range(Q):
        s = scores[u, rows]
        # stable sort of rows already in ascending order: ties keep the
        # lower row first
        order = torch.sort(s, descending=True, stable=True).indices[:n]
        out_s[u, :n] = s[order]
        out_i[u, :n] = rows[order].to(torch.int32)
    return out_s, out_i
