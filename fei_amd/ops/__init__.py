"""fei_amd.ops — engine ops with a single dispatch rule:

  - CUDA (= ROCm/HIP) tensors -> the in-tree gfx950 kernel library,
    loaded via ctypes. If the library is missing on a GPU machine, ops
    FAIL LOUDLY — there is no silent eager fallback on GPU.
  - CPU tensors -> the fp32-accurate torch reference implementations
    (fei_amd/ops/reference.py), used by CPU tests and tiny models.

All kernels launch on torch's current CUDA stream, so the decode step can
be captured into a hipGraph (torch.cuda.CUDAGraph) — see engine/engine.py.
"""

from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Tuple

import torch

from fei_amd.ops import reference as ref

_LIB: Optional[ctypes.CDLL] = None
_LIB_ERR: Optional[str] = None
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         "libfei_kernels.so")

_c = ctypes
_vp, _i, _f, _u64, _l = _c.c_void_p, _c.c_int, _c.c_float, _c.c_ulonglong, _c.c_long


def _try_load() -> None:
    global _LIB, _LIB_ERR
    if _LIB is not None or _LIB_ERR is not None:
        return
    try:
        lib = ctypes.CDLL(_LIB_PATH)
    except OSError as e:
        _LIB_ERR = str(e)
        return
    lib.fei_rmsnorm.argtypes = [_vp, _vp, _vp, _i, _i, _f, _vp]
    lib.fei_add_rmsnorm.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]
    lib.fei_rope_kv_decode.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _i, _i, _i, _i, _i, _l, _l, _vp]
    lib.fei_rope_kv_prefill.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _i, _i, _i, _i, _i, _i, _l, _l, _vp]
    lib.fei_attn_decode.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp,
                                    _i, _i, _i, _i, _i, _i, _f, _l,
                                    _vp, _vp, _vp, _l, _vp, _vp, _i, _vp]
    lib.fei_attn_decode_combine.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i,
                                            _vp]
    lib.fei_swiglu.argtypes = [_vp, _vp, _l, _i, _vp]
    lib.fei_sample.argtypes = [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _u64,
                               _i, _vp]
    lib.fei_advance.argtypes = [_vp, _vp, _i, _i, _vp]
    lib.fei_attn_prefill.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp,
                                     _i, _i, _i, _i, _i, _i, _f, _i, _l, _vp]
    lib.fei_mfma_probe.argtypes = [_vp, _vp, _vp, _vp]
    lib.fei_gemv.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _vp]
    lib.fei_gemm_m8.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _vp]
    lib.fei_attn_decode_fused.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _i, _i, _i, _i, _i, _f,
                                          _l, _l, _vp]
    lib.fei_sample_onepass.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _f, _u64,
                                       _i, _i, _vp]
    lib.fei_sample_shard.argtypes = [_vp, _vp, _vp, _i, _i, _i, _f, _u64, _vp]
    lib.fei_sample_filtered.argtypes = [_vp, _vp, _vp, _vp, _vp, _i, _i, _i,
                                        _f, _f, _u64, _i, _vp]
    lib.fei_sample_filtered_rows.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp,
                                             _vp, _vp, _i, _i, _vp]
    lib.fei_sample_filtered_rows.restype = _i
    lib.fei_rope_kv8_decode.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _i, _i, _i, _i, _i, _l, _l,
                                        _vp]
    lib.fei_rope_kv8_prefill.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _i, _i, _i, _i, _i, _i,
                                         _l, _l, _vp]
    lib.fei_attn_decode_kv8.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _i, _i, _i, _i, _i, _i, _f, _l,
                                        _vp, _vp, _vp, _l, _vp]
    lib.fei_attn_decode_kv8.restype = _i
    lib.fei_attn_prefill_kv8.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _i, _i, _i, _i, _i, _i, _f, _l, _vp]
    lib.fei_attn_prefill_kv8.restype = _i
    lib.fei_stream_layer_check.argtypes = [_i, _i, _i, _i, _i]
    lib.fei_stream_layer_check.restype = _i
    lib.fei_stream_layer.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _i, _i, _i, _i, _i,
                                     _i, _i, _f, _f, _vp]
    lib.fei_attn_decode_paged.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _i, _i, _i, _i, _i, _i, _i, _f,
                                          _l, _vp, _vp, _vp, _l, _vp]
    lib.fei_rope_kv_prefill_paged.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _i, _i, _i, _i, _i,
                                              _i, _i, _l, _l, _vp]
    lib.fei_rope_kv_prefill_paged.restype = _i
    lib.fei_attn_prefill_paged.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp,
                                           _i, _i, _i, _i, _i, _i, _i, _f,
                                           _l, _vp]
    lib.fei_attn_prefill_paged.restype = _i
    lib.fei_rope_kv8_prefill_paged.argtypes = [
        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
        _i, _i, _i, _i, _i, _i, _i, _l, _l, _vp]
    lib.fei_rope_kv8_prefill_paged.restype = _i
    lib.fei_attn_decode_paged_kv8.argtypes = [
        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
        _i, _i, _i, _i, _i, _i, _i, _f, _l, _vp, _vp, _vp, _l, _vp]
    lib.fei_attn_decode_paged_kv8.restype = _i
    lib.fei_attn_prefill_paged_kv8.argtypes = [
        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
        _i, _i, _i, _i, _i, _i, _i, _f, _l, _vp]
    lib.fei_attn_prefill_paged_kv8.restype = _i
    lib.fei_rope_kv_prefill_paged_ragged.argtypes = [
        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
        _i, _i, _i, _i, _i, _i, _i, _l, _l, _vp]
    lib.fei_rope_kv_prefill_paged_ragged.restype = _i
    lib.fei_attn_prefill_paged_ragged.argtypes = [
        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
        _i, _i, _i, _i, _i, _i, _i, _i, _f, _l, _vp]
    lib.fei_attn_prefill_paged_ragged.restype = _i
    lib.fei_add_layernorm.argtypes = [_vp, _vp, _vp, _vp, _vp, _i, _i, _f,
                                      _i, _vp]
    lib.fei_gelu.argtypes = [_vp, _vp, _l, _vp]
    lib.fei_gemv_norm_fp8.argtypes = [_vp, _vp, _vp, _vp, _vp, _i, _i, _i,
                                      _f, _vp]
    lib.fei_gemv_res_fp8.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]
    lib.fei_gemv_swiglu_norm_fp8.argtypes = [_vp, _vp, _vp, _vp, _vp, _i, _i,
                                             _i, _f, _vp]
    lib.fei_quant_fp8_rows.argtypes = [_vp, _vp, _vp, _i, _i, _vp]
    lib.fei_gemv_swiglu.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _vp]
    lib.fei_prefetch.argtypes = [_vp, _l, _vp, _i, _vp]
    lib.fei_gemv_res.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]
    lib.fei_gemv_norm.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp,
                                  _vp]
    lib.fei_gemv_swiglu_norm.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _f,
                                         _i, _vp, _vp]
    for fn in (lib.fei_gemv_addnorm, lib.fei_gemv_swiglu_addnorm):
        fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i,
                       _vp]
        fn.restype = _i
    for fn in (lib.fei_gemv_addnorm_ring, lib.fei_gemv_swiglu_addnorm_ring):
        fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i,
                       _i, _vp]
        fn.restype = _i
    lib.fei_gemv_addnorm_ring_slots.argtypes = [_i, _i, _i, _i]
    lib.fei_gemv_addnorm_ring_slots.restype = _i
    lib.fei_gemv_addnorm_ring_max_trips.argtypes = []
    lib.fei_gemv_addnorm_ring_max_trips.restype = _i
    lib.fei_gemv_deep.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _vp]
    lib.fei_gemv_deep.restype = _i
    lib.fei_score_topk.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _i, _i, _i, _i, _i, _i, _i, _vp]
    lib.fei_score_topk.restype = _i
    _LIB = lib


def kernels_available() -> bool:
    _try_load()
    return _LIB is not None


def require_lib() -> ctypes.CDLL:
    _try_load()
    if _LIB is None:
        raise RuntimeError(
            "fei_amd HIP kernel library not found at "
            f"{_LIB_PATH} ({_LIB_ERR}). Build it with "
            "`python -m fei_amd.ops.build` — GPU execution refuses to fall "
            "back to eager PyTorch.")
    return _LIB


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


# ---------------------------------------------------------------------------


class QuantKV:
    """One layer's K (or V) cache in the fp8 storage format of
    reference.quant_kv_fp8: ``data`` uint8 [B, Hkv, max_seq, D] e4m3fn codes
    plus ``scale`` f32 [B, Hkv, max_seq], one per cached row. It takes a
    tensor's place in the engine's k_caches / v_caches lists; the append and
    attention entry points below dispatch on it."""

    __slots__ = ("data", "scale")

    def __init__(self, data: torch.Tensor, scale: torch.Tensor):
        assert data.dtype == torch.uint8 and scale.dtype == torch.float32
        assert tuple(scale.shape) == tuple(data.shape[:-1])
        # the kernels take raw pointers and index rows as
        # ((b*Hkv + h)*max_seq + p): a sliced or strided view would read
        # the wrong rows; their 16 B / 8 B vector loads need an aligned base
        assert data.is_contiguous() and scale.is_contiguous(), \
            "QuantKV needs contiguous data and scale"
        assert data.data_ptr() % 16 == 0, "QuantKV data must be 16 B aligned"
        self.data = data
        self.scale = scale

    @classmethod
    def zeros(cls, shape, device) -> "QuantKV":
        return cls(torch.zeros(shape, dtype=torch.uint8, device=device),
                   torch.ones(shape[:-1], dtype=torch.float32, device=device))

    @property
    def shape(self):
        return self.data.shape

    def dequant(self, length: Optional[int] = None) -> torch.Tensor:
        """f32 [B, Hkv, length or max_seq, D] (reference / diagnostics)."""
        n = self.data.shape[2] if length is None else length
        return ref.dequant_kv_fp8(self.data[:, :, :n], self.scale[:, :, :n])


def _kv8_pair(k_cache, v_cache) -> bool:
    k8, v8 = isinstance(k_cache, QuantKV), isinstance(v_cache, QuantKV)
    if k8 != v8:
        raise TypeError("k_cache and v_cache must both be QuantKV or both "
                        "be tensors")
    return k8


def _check_gqa(name: str, Hq: int, Hkv: int) -> None:
    """The decode-attention kernels are instantiated for GQA group sizes
    1/2/4/8 only; the C entry points launch nothing for any other."""
    if Hkv <= 0 or Hq % Hkv != 0 or Hq // Hkv not in (1, 2, 4, 8):
        raise ValueError(f"{name}: unsupported GQA group Hq={Hq}, Hkv={Hkv} "
                         "(Hq/Hkv must be 1, 2, 4 or 8)")


def _check_vec8(name: str, n: int, what: str = "last dimension") -> None:
    """The row-wise and element-wise kernels move 8 bf16 per lane and size
    their loops as n >> 3: a tail of n % 8 elements would stay unwritten."""
    if n % 8 != 0:
        raise ValueError(f"{name}: {what} must be a multiple of 8, got {n}")


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RMSNorm over the last dim. x: [..., C] bf16 (GPU) / any float (CPU)."""
    _check_vec8("rmsnorm", x.shape[-1])
    if x.numel() == 0:                  # zero rows: an empty grid is an error
        return torch.empty_like(x) if out is None else out
    if not x.is_cuda:
        return ref.rmsnorm(x, weight, eps)
    lib = require_lib()
    x2 = x.contiguous()
    if out is None:
        out = torch.empty_like(x2)
    rows = x2.numel() // x2.shape[-1]
    lib.fei_rmsnorm(_ptr(out), _ptr(x2), _ptr(weight), rows, x2.shape[-1],
                    eps, _stream())
    return out


def fused_add_rmsnorm(x: torch.Tensor, residual: torch.Tensor,
                      weight: torch.Tensor, eps: float = 1e-5,
                      out: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """residual += x (in place on GPU); out = rmsnorm(residual)."""
    _check_vec8("fused_add_rmsnorm", x.shape[-1])
    # the kernel updates residual through its raw pointer, row r at r * cols:
    # a strided view would be read and written at the wrong addresses, and a
    # contiguous copy would lose the in-place update
    if not residual.is_contiguous():
        raise ValueError("fused_add_rmsnorm: residual must be contiguous "
                         "(it is updated in place)")
    if x.numel() == 0:
        return (torch.empty_like(x) if out is None else out), residual
    if not x.is_cuda:
        o, res = ref.fused_add_rmsnorm(x, residual, weight, eps)
        residual.copy_(res)
        return o, residual
    lib = require_lib()
    x2 = x.contiguous()
    if out is None:
        out = torch.empty_like(x2)
    rows = x2.numel() // x2.shape[-1]
    lib.fei_add_rmsnorm(_ptr(out), _ptr(residual), _ptr(x2), _ptr(weight),
                        rows, x2.shape[-1], eps, _stream())
    return out, residual


def rope_kv_decode(q, k, v, k_cache, v_cache, pos, table) -> torch.Tensor:
    """In-place RoPE on q; k roped + v appended into caches at pos[b].
    q [B,Hq,D], k/v [B,Hkv,D], caches [B,Hkv,max_seq,D], pos [B] int32.
    QuantKV caches: the rows are quantised on the way in (kv_fp8.hip)."""
    kv8 = _kv8_pair(k_cache, v_cache)
    if not q.is_cuda:
        if kv8:
            q_out = ref.rope_kv_decode_fp8(
                q, k, v, k_cache.data, k_cache.scale, v_cache.data,
                v_cache.scale, pos, table)
        else:
            q_out = ref.rope_kv_decode(q, k, v, k_cache, v_cache, pos, table)
        q.copy_(q_out)
        return q
    lib = require_lib()
    B, Hq, D = q.shape
    Hkv = k.shape[1]
    assert q.stride(2) == 1 and q.stride(1) == D, "head rows must be contiguous"
    assert k.stride(1) == D and v.stride(1) == D
    assert k.stride(0) == v.stride(0)
    if kv8:
        assert D in (64, 128), f"fp8 KV append supports D in (64,128), got {D}"
        lib.fei_rope_kv8_decode(_ptr(q), _ptr(k), _ptr(v), _ptr(k_cache.data),
                                _ptr(k_cache.scale), _ptr(v_cache.data),
                                _ptr(v_cache.scale), _ptr(table), _ptr(pos),
                                B, Hq, Hkv, D, k_cache.shape[2],
                                q.stride(0), k.stride(0), _stream())
        return q
    lib.fei_rope_kv_decode(_ptr(q), _ptr(k), _ptr(v), _ptr(k_cache),
                           _ptr(v_cache), _ptr(table), _ptr(pos),
                           B, Hq, Hkv, D, k_cache.shape[2],
                           q.stride(0), k.stride(0), _stream())
    return q


def rope_kv_prefill(q, k, v, k_cache, v_cache, pos0, table) -> torch.Tensor:
    """In-place RoPE on q [B,S,Hq,D]; k roped + v appended at pos0[b]+s
    (quantised per row when the caches are QuantKV)."""
    kv8 = _kv8_pair(k_cache, v_cache)
    if not q.is_cuda:
        if kv8:
            q_out = ref.rope_kv_prefill_fp8(
                q, k, v, k_cache.data, k_cache.scale, v_cache.data,
                v_cache.scale, pos0, table)
        else:
            q_out = ref.rope_kv_prefill(q, k, v, k_cache, v_cache, pos0, table)
        q.copy_(q_out)
        return q
    lib = require_lib()
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    assert q.stride(3) == 1 and q.stride(2) == D
    assert q.stride(0) == S * q.stride(1), "token rows must be uniform"
    assert k.stride(2) == D and k.stride(0) == S * k.stride(1)
    assert k.stride(1) == v.stride(1)
    if kv8:
        assert D in (64, 128), f"fp8 KV append supports D in (64,128), got {D}"
        lib.fei_rope_kv8_prefill(_ptr(q), _ptr(k), _ptr(v), _ptr(k_cache.data),
                                 _ptr(k_cache.scale), _ptr(v_cache.data),
                                 _ptr(v_cache.scale), _ptr(table), _ptr(pos0),
                                 B, S, Hq, Hkv, D, k_cache.shape[2],
                                 q.stride(1), k.stride(1), _stream())
        return q
    lib.fei_rope_kv_prefill(_ptr(q), _ptr(k), _ptr(v), _ptr(k_cache),
                            _ptr(v_cache), _ptr(table), _ptr(pos0),
                            B, S, Hq, Hkv, D, k_cache.shape[2],
                            q.stride(1), k.stride(1), _stream())
    return q


def attn_decode(q, k_cache, v_cache, pos, splits: int = 32,
                scale: Optional[float] = None,
                workspace: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                out: Optional[torch.Tensor] = None,
                k: Optional[torch.Tensor] = None,
                v: Optional[torch.Tensor] = None,
                table: Optional[torch.Tensor] = None,
                layer: int = 0) -> torch.Tensor:
    """Single-token GQA attention over n = pos[b]+1 cache entries.
    q [B,Hq,D] -> out [B,Hq,D]. The length is read on DEVICE (hipGraph).
    When (k, v, table) are given, the kernel also fuses the step's RoPE +
    KV-append: q is the RAW qkv view and cache[pos] is written in-kernel.
    QuantKV caches run the fp8 kernel (kv_fp8.hip): same partials, always
    the separate combine launch."""
    B, Hq, D = q.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    kv8 = _kv8_pair(k_cache, v_cache)
    if not q.is_cuda:
        if table is not None:
            rope_kv_decode(q, k, v, k_cache, v_cache, pos, table)
        seqlen = pos + 1
        if kv8:
            n = int(seqlen.max())
            return ref.attn_decode(q, k_cache.dequant(n), v_cache.dequant(n),
                                   seqlen, scale)
        return ref.attn_decode(q, k_cache, v_cache, seqlen, scale)
    lib = require_lib()
    if kv8:
        return _attn_decode_kv8(lib, q, k_cache, v_cache, pos, splits, scale,
                                workspace, out, k, v, table)
    _check_gqa("attn_decode", Hq, k_cache.shape[1])
    arrive = None
    if workspace is None:
        part_o = torch.empty(B, Hq, splits, D, dtype=torch.float32, device=q.device)
        part_ml = torch.empty(B, Hq, splits, 2, dtype=torch.float32, device=q.device)
    else:
        part_o, part_ml = workspace[0], workspace[1]
        # a 3rd workspace element (zeroed int32 [B*Hkv*splits] per-split
        # done-flag buffer) selects the FUSED combine: split 0 of each
        # (b, hkv) pair polls the flags and reduces the partials in-kernel,
        # and the separate combine launch is skipped (FEI_FUSED_CMB=0 opts
        # out for A/B; pass `layer` so the flag tags stay unique across the
        # layers of one step).
        if len(workspace) >= 3 and _FUSED_CMB:
            arrive = workspace[2]
        assert part_o.shape[2] == splits and part_ml.shape[2] == splits, \
            f"workspace sized for {part_o.shape[2]} splits, kernel asked {splits}"
    if out is None:
        out = torch.empty_like(q)
    Hkv = k_cache.shape[1]
    assert q.stride(2) == 1 and q.stride(1) == D
    # the kernel's V lane maps tile 256 threads by D/2 and D/8 — both must
    # divide the block (holds for the llama head dims 64/128; D=96 would
    # silently under-cover a tile)
    assert D in (64, 128), f"decode attention supports D in (64,128), got {D}"
    assert splits <= 64, "combine kernel stages at most 64 split partials"
    if table is not None:
        assert k is not None and v is not None
        assert k.stride(1) == D and k.stride(0) == v.stride(0)
        kin, vin, cs, kv_bs = _ptr(k), _ptr(v), _ptr(table), k.stride(0)
    else:
        kin = vin = cs = None
        kv_bs = 0
    if arrive is not None:
        assert arrive.dtype == torch.int32 and \
            arrive.numel() >= B * Hkv * splits
    lib.fei_attn_decode(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(part_o),
                        _ptr(part_ml), _ptr(pos), B, Hq, Hkv, D,
                        k_cache.shape[2], splits, scale, q.stride(0),
                        kin, vin, cs, kv_bs,
                        _ptr(out) if arrive is not None else None,
                        _ptr(arrive) if arrive is not None else None,
                        layer, _stream())
    if arrive is None:
        lib.fei_attn_decode_combine(_ptr(out), _ptr(part_o), _ptr(part_ml),
                                    B, Hq, D, splits, int(_CMB_FLAT),
                                    _stream())
    return out


def attn_decode_combine(part_o: torch.Tensor, part_ml: torch.Tensor,
                        out: Optional[torch.Tensor] = None,
                        flat: Optional[bool] = None) -> torch.Tensor:
    """The split-K combine of decode attention on its own: part_o
    [B,Hq,splits,D] f32 and part_ml [B,Hq,splits,2] f32 (m, l) as the
    attention kernels write them -> out [B,Hq,D] bf16. `flat` as in
    sample(): None follows FEI_CMB_FLAT."""
    lib = require_lib()
    B, Hq, splits, D = part_o.shape
    assert part_o.dtype == torch.float32 and part_o.is_contiguous()
    assert part_ml.dtype == torch.float32 and part_ml.is_contiguous()
    assert part_ml.shape == (B, Hq, splits, 2)
    assert D in (64, 128), f"decode attention supports D in (64,128), got {D}"
    assert 1 <= splits <= 64, "combine kernel stages at most 64 split partials"
    if out is None:
        out = torch.empty(B, Hq, D, dtype=torch.bfloat16,
                          device=part_o.device)
    assert out.shape == (B, Hq, D) and out.is_contiguous()
    lib.fei_attn_decode_combine(_ptr(out), _ptr(part_o), _ptr(part_ml),
                                B, Hq, D, splits,
                                int(_CMB_FLAT if flat is None else flat),
                                _stream())
    return out


def _attn_decode_kv8(lib, q, k_cache, v_cache, pos, splits, scale, workspace,
                     out, k, v, table) -> torch.Tensor:
    B, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    if workspace is None:
        part_o = torch.empty(B, Hq, splits, D, dtype=torch.float32, device=q.device)
        part_ml = torch.empty(B, Hq, splits, 2, dtype=torch.float32, device=q.device)
    else:
        # a 3rd element (fused-combine flags) is ignored: the fp8 path
        # always takes the separate combine launch
        part_o, part_ml = workspace[0], workspace[1]
        assert part_o.shape[2] == splits and part_ml.shape[2] == splits, \
            f"workspace sized for {part_o.shape[2]} splits, kernel asked {splits}"
    if out is None:
        out = torch.empty_like(q)
    assert q.stride(2) == 1 and q.stride(1) == D
    assert D in (64, 128), f"decode attention supports D in (64,128), got {D}"
    # the combine kernel stages its 2*splits m/l values with D threads
    assert 2 * splits <= D, \
        f"fp8 decode attention needs 2*splits <= D (splits={splits}, D={D})"
    assert Hq % Hkv == 0 and Hq // Hkv in (1, 2, 4, 8), \
        f"unsupported GQA group size {Hq}/{Hkv}"
    if table is not None:
        assert k is not None and v is not None
        assert k.stride(1) == D and k.stride(0) == v.stride(0)
        kin, vin, cs, kv_bs = _ptr(k), _ptr(v), _ptr(table), k.stride(0)
    else:
        kin = vin = cs = None
        kv_bs = 0
    rc = lib.fei_attn_decode_kv8(
        _ptr(q), _ptr(k_cache.data), _ptr(k_cache.scale), _ptr(v_cache.data),
        _ptr(v_cache.scale), _ptr(part_o), _ptr(part_ml), _ptr(pos),
        B, Hq, Hkv, D, k_cache.shape[2], splits, scale, q.stride(0),
        kin, vin, cs, kv_bs, _stream())
    if rc != 0:
        raise RuntimeError(f"fei_attn_decode_kv8 refused the launch (rc={rc})")
    lib.fei_attn_decode_combine(_ptr(out), _ptr(part_o), _ptr(part_ml),
                                B, Hq, D, splits, int(_CMB_FLAT), _stream())
    return out


def attn_decode_fused(q, k, v, k_cache, v_cache, pos, table,
                      scale: Optional[float] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused decode attention: RoPE(q,k) + KV-append + GQA attention in one
    kernel (grid Hkv x B, no split partials). For agent-length sequences;
    long-context uses rope_kv_decode + attn_decode (split-K)."""
    B, Hq, D = q.shape
    Hkv = k.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if _kv8_pair(k_cache, v_cache):
        raise ValueError("attn_decode_fused has no fp8 KV form; use "
                         "attn_decode (split-K) with QuantKV caches")
    if not q.is_cuda:
        rope_kv_decode(q, k, v, k_cache, v_cache, pos, table)
        return ref.attn_decode(q, k_cache, v_cache, pos + 1, scale)
    lib = require_lib()
    _check_gqa("attn_decode_fused", Hq, Hkv)
    # the kernel's osh[8][DEC_DMAX/2][2] holds 256/(D/2) key groups: D < 64
    # would index past it
    if D not in (64, 128):
        raise ValueError(
            f"attn_decode_fused supports D in (64,128), got {D}")
    assert q.stride(2) == 1 and q.stride(1) == D
    assert k.stride(1) == D and k.stride(0) == v.stride(0)
    if out is None:
        out = torch.empty(B, Hq, D, dtype=torch.bfloat16, device=q.device)
    lib.fei_attn_decode_fused(_ptr(q), _ptr(k), _ptr(v), _ptr(k_cache),
                              _ptr(v_cache), _ptr(out), _ptr(table), _ptr(pos),
                              B, Hq, Hkv, D, k_cache.shape[2], scale,
                              q.stride(0), k.stride(0), _stream())
    return out


def attn_prefill(q, k_cache, v_cache, pos0, scale: Optional[float] = None,
                 causal: bool = True, kv_len: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal (or bidirectional) GQA attention of q [B,S,Hq,D] over the
    caches. q token s attends [0, pos0[b]+s] when causal, else [0, kv_len[b])."""
    B, S, Hq, D = q.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    kv8 = _kv8_pair(k_cache, v_cache)
    if kv8 and not causal:
        raise ValueError("fp8 KV prefill attention is causal-only")
    Hkv = k_cache.shape[1]
    # the kernels index the cache with hkv = hq / (Hq / Hkv): a group that is
    # not integral reaches hkv = Hkv, one head past the cache (any integral
    # group is fine: the prefill kernels are not templated on it)
    if Hkv <= 0 or Hq % Hkv != 0:
        raise ValueError(f"attn_prefill: Hq={Hq} is not a multiple of "
                         f"Hkv={Hkv}")
    if not q.is_cuda:
        if kv8:
            n = int(pos0.max()) + S
            kd, vd = k_cache.dequant(n), v_cache.dequant(n)
            if q.dtype == torch.bfloat16:
                # bf16 run: the kernel stages bf16(f32(code) * scale)
                kd, vd = kd.to(q.dtype), vd.to(q.dtype)
            return ref.attn_prefill(q, kd, vd, pos0, scale)
        if causal:
            return ref.attn_prefill(q, k_cache, v_cache, pos0, scale)
        # bidirectional reference: softmax over [0, kv_len)
        return _ref_bidir(q, k_cache, v_cache, kv_len, scale)
    lib = require_lib()
    # k_attn_prefill / k_attn_prefill_kv8 are instantiated for these two head
    # sizes; the bf16 C entry point launches nothing for any other and the
    # output would be uninitialised memory
    if D not in (64, 128):
        raise ValueError(f"attn_prefill supports D in (64,128), got {D}")
    if out is None:
        out = torch.empty(B, S, Hq, D, dtype=q.dtype, device=q.device)
    if kv8:
        assert q.stride(3) == 1 and q.stride(2) == D
        assert q.stride(0) == S * q.stride(1)
        assert out.is_contiguous()
        rc = lib.fei_attn_prefill_kv8(
            _ptr(q), _ptr(k_cache.data), _ptr(k_cache.scale),
            _ptr(v_cache.data), _ptr(v_cache.scale), _ptr(out), _ptr(pos0),
            B, S, Hq, k_cache.shape[1], D, k_cache.shape[2], scale,
            q.stride(1), _stream())
        if rc != 0:
            raise RuntimeError(
                f"fp8 KV prefill attention supports D in (64,128), got {D}")
        return out
    if kv_len is None:
        kv_len = pos0  # unused when causal
    assert q.stride(3) == 1 and q.stride(2) == D
    assert q.stride(0) == S * q.stride(1)
    assert out.is_contiguous()
    lib.fei_attn_prefill(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out),
                         _ptr(pos0), _ptr(kv_len), B, S, Hq, Hkv, D,
                         k_cache.shape[2], scale, 1 if causal else 0,
                         q.stride(1), _stream())
    return out


def _ref_bidir(q, k_cache, v_cache, kv_len, scale):
    B, S, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    out = torch.empty_like(q)
    for b in range(B):
        n = int(kv_len[b])
        k = k_cache[b, :, :n, :].float()
        v = v_cache[b, :, :n, :].float()
        qb = q[b].float().view(S, Hkv, G, D)
        s = torch.einsum("shgd,hnd->hgsn", qb, k) * scale
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgsn,hnd->shgd", p, v)
        out[b] = o.reshape(S, Hq, D).to(q.dtype)
    return out


def swiglu(gate_up: torch.Tensor,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gate_up [..., 2*inter] -> [..., inter]: silu(gate) * up."""
    inter = gate_up.shape[-1] // 2
    if gate_up.shape[-1] != 2 * inter:
        raise ValueError("swiglu: the last dimension must be even, got "
                         f"{gate_up.shape[-1]}")
    _check_vec8("swiglu", inter, "inter")
    if gate_up.numel() == 0:
        return gate_up.new_empty(*gate_up.shape[:-1], inter) \
            if out is None else out
    if not gate_up.is_cuda:
        return ref.swiglu(gate_up)
    lib = require_lib()
    gu = gate_up.contiguous()
    rows = gu.numel() // gu.shape[-1]
    if out is None:
        out = torch.empty(*gu.shape[:-1], inter, dtype=gu.dtype, device=gu.device)
    lib.fei_swiglu(_ptr(out), _ptr(gu), rows, inter, _stream())
    return out


def sample(logits: torch.Tensor, token: torch.Tensor,
           step: torch.Tensor, workspace: torch.Tensor,
           out_tokens: Optional[torch.Tensor] = None,
           temperature: float = 0.0, seed: int = 0,
           nchunks: int = 64, flat: Optional[bool] = None) -> torch.Tensor:
    """Greedy (T<=0) or Gumbel-max categorical (T>0) sampling.
    logits [B,V] bf16 -> token [B] int32 (written in place; also appended to
    out_tokens[b, step] when given). All state on device (hipGraph-safe).
    `flat` picks the one-pass kernel at B <= 8: the preloading one (True,
    rows up to 131072 wide) or the looping one (False); None follows
    FEI_SAMPLE_FLAT. Same token either way."""
    B, V = logits.shape
    if not logits.is_cuda:
        if temperature <= 0:
            t = ref.argmax_sample(logits)
        else:
            # deterministic by (seed, step) like the GPU kernel's splitmix
            # hash (not bit-identical, but the same reproducibility
            # contract on both paths)
            g = torch.Generator().manual_seed(
                (int(seed) * 1000003 + int(step)) & 0x7FFFFFFF)
            t = ref.gumbel_sample(logits, temperature, g)
        token.copy_(t)
        if out_tokens is not None:
            st = int(step)
            for b in range(B):
                if st < out_tokens.shape[1]:
                    out_tokens[b, st] = t[b]
        return token
    lib = require_lib()
    max_new = out_tokens.shape[1] if out_tokens is not None else 0
    out_ptr = _ptr(out_tokens) if out_tokens is not None else None
    if B <= 8:
        lib.fei_sample_onepass(_ptr(logits), _ptr(token), out_ptr, _ptr(step),
                               B, V, temperature, seed, max_new,
                               int(_SAMPLE_FLAT if flat is None else flat),
                               _stream())
    else:
        lib.fei_sample(_ptr(logits), _ptr(token), out_ptr, _ptr(step),
                       _ptr(workspace), B, V, nchunks, temperature, seed,
                       max_new, _stream())
    return token


def sample_filtered(logits: torch.Tensor, token: torch.Tensor,
                    step: torch.Tensor, info: torch.Tensor,
                    out_tokens: Optional[torch.Tensor] = None,
                    temperature: float = 0.0, seed: int = 0,
                    top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """sample() restricted to the top-k / top-p keep set of each row
    (reference.filter_keep: tie-inclusive, top-k then top-p on the raw
    logits, temperature only at the draw). One kernel for any B; all state
    on device and the filter parameters are kernel arguments, so the call is
    hipGraph-capturable. ``info`` [B,2] f32 receives (smallest kept value,
    kept count as int32 bits). With the filter inactive (top_k 0 or >= V and
    top_p >= 1) the token equals sample()'s; temperature <= 0 is greedy."""
    if top_k < 0:
        raise ValueError(f"top_k must be >= 0, got {top_k}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    B, V = logits.shape
    if not logits.is_cuda:
        keep, thr, count = ref.filter_keep(logits, top_k, top_p)
        info[:, 0] = thr
        info[:, 1].view(torch.int32).copy_(count)
        if keep.all():
            masked = logits
        else:
            masked = logits.float().masked_fill(~keep, float("-inf"))
        # the (seed, step)-seeded draw of sample()'s CPU path
        return sample(masked, token, step, None, out_tokens=out_tokens,
                      temperature=temperature, seed=seed)
    lib = require_lib()
    max_new = out_tokens.shape[1] if out_tokens is not None else 0
    out_ptr = _ptr(out_tokens) if out_tokens is not None else None
    lib.fei_sample_filtered(_ptr(logits), _ptr(token), out_ptr, _ptr(step),
                            _ptr(info), B, V, int(top_k), float(top_p),
                            float(temperature), int(seed), max_new, _stream())
    return token


def _check_rows_arg(name: str, t, dtype: torch.dtype, shape, device) -> None:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got "
                         f"{tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name} must be on {device}, got {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def sample_rows(logits: torch.Tensor, token: torch.Tensor,
                step: torch.Tensor, info: torch.Tensor, *,
                top_k: torch.Tensor, top_p: torch.Tensor,
                temperature: torch.Tensor, seed: torch.Tensor) -> torch.Tensor:
    """sample_filtered() with every parameter per row, for continuous
    batching: row b of ``logits`` [B,V] is drawn with top_k[b] (i32),
    top_p[b] (f32), temperature[b] (f32), seed[b] (i64) and step[b] (i32),
    all device tensors of length B. ``token`` [B] i32 and ``info`` [B,2] f32
    are written; ``step`` is not (the caller advances it with step.add_(1)).

    Row b's token and info equal sample_filtered() on logits[b:b+1] alone
    with that row's scalars, wherever the row sits in the batch (the noise
    does not depend on the row index). Nothing is a kernel argument except
    the sizes, so the call is hipGraph-capturable and a captured launch
    follows in-place parameter changes. Argument dtype / shape / device /
    contiguity errors raise ValueError naming the argument; parameter VALUES
    are not checked here (that would need a sync)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError("logits must be a [B, V] tensor")
    if not logits.is_contiguous():
        raise ValueError("logits must be contiguous")
    if logits.is_cuda and logits.dtype != torch.bfloat16:
        raise ValueError(f"logits must be bfloat16 on the GPU, got "
                         f"{logits.dtype}")
    B, V = logits.shape
    dev = logits.device
    _check_rows_arg("token", token, torch.int32, (B,), dev)
    _check_rows_arg("step", step, torch.int32, (B,), dev)
    _check_rows_arg("info", info, torch.float32, (B, 2), dev)
    _check_rows_arg("top_k", top_k, torch.int32, (B,), dev)
    _check_rows_arg("top_p", top_p, torch.float32, (B,), dev)
    _check_rows_arg("temperature", temperature, torch.float32, (B,), dev)
    _check_rows_arg("seed", seed, torch.int64, (B,), dev)
    if not logits.is_cuda:
        for b in range(B):
            sample_filtered(logits[b:b + 1], token[b:b + 1], step[b:b + 1],
                            info[b:b + 1], temperature=float(temperature[b]),
                            seed=int(seed[b]), top_k=int(top_k[b]),
                            top_p=float(top_p[b]))
        return token
    lib = require_lib()
    rc = lib.fei_sample_filtered_rows(
        _ptr(logits), _ptr(token), _ptr(info), _ptr(top_k), _ptr(top_p),
        _ptr(temperature), _ptr(seed), _ptr(step), B, V, _stream())
    if rc != 0:
        raise ValueError(f"sample_rows: empty batch or vocabulary "
                         f"(B={B}, V={V})")
    return token


def sample_shard(logits: torch.Tensor, step: torch.Tensor,
                 v_offset: int, out: torch.Tensor,
                 temperature: float = 0.0, seed: int = 0) -> torch.Tensor:
    """Tensor-parallel shard sampler: reduce THIS rank's logits shard
    [B, V_local] (bf16 on GPU) to (best value, best GLOBAL index) per
    sequence, written into ``out`` [B, 2] f32 (index stored as int bits).
    The ranks then all-gather 8 bytes/seq instead of the vocab row.
    Gumbel noise is keyed by the global index (same splitmix hash as the
    full sampler), so shard+combine is bit-identical to sampling the
    gathered logits. CPU path mirrors the hash exactly."""
    B, Vl = logits.shape
    if not logits.is_cuda:
        vals = logits.float()
        if temperature > 0:
            vals = vals / temperature + ref.hash_gumbel(
                B, Vl, v_offset, int(seed), int(step))
        best = vals.max(dim=-1)
        out[:, 0] = best.values
        out[:, 1].view(torch.int32).copy_(
            (best.indices + v_offset).to(torch.int32))
        return out
    lib = require_lib()
    lib.fei_sample_shard(_ptr(logits), _ptr(out), _ptr(step), B, Vl,
                         int(v_offset), float(temperature), int(seed),
                         _stream())
    return out


# -- persistent weight-streaming decode layer (csrc/stream_layer.hip) -------

STREAM_NSPLIT = 32


def stream_layer_check(C: int, Hq: int, Hkv: int, D: int, I: int) -> int:
    """Residency + shape guard for the persistent layer engine. 0 = OK;
    negative = unsupported (caller uses the launch path). GPU only."""
    lib = require_lib()
    return int(lib.fei_stream_layer_check(C, Hq, Hkv, D, I))


def stream_workspace(spec, device) -> dict:
    """Granule buffers (u64 {tag, payload}) + fail word for the stream
    engine. ~1.3 MB for llama3-8b; zeroed by the engine whenever pos can
    move backwards (prefill) — tags are pos-keyed otherwise."""
    C, D = spec.hidden_size, spec.head_dim
    Hq, Hkv, I = spec.num_heads, spec.num_kv_heads, spec.intermediate_size
    mk = lambda n: torch.zeros(n, dtype=torch.int64, device=device)
    return {
        "g_qkv": mk((Hq + 2 * Hkv) * D),
        "g_att": mk(Hq * D // 2),
        "g_h2": mk(C // 2),
        "g_act": mk(I),
        "g_done": mk(6 * 256),        # [stage, NWG] producer-done granules
        "fail": torch.zeros(1, dtype=torch.int32, device=device),
    }


def stream_layer(x_in: torch.Tensor, h_out: torch.Tensor, lw, spec,
                 k_cache: torch.Tensor, v_cache: torch.Tensor,
                 cos_sin: torch.Tensor, pos: torch.Tensor, ws: dict,
                 layer: int, scale: float) -> None:
    """ONE persistent launch = one decode layer at batch 1 (S1 qkv GEMV ->
    attention -> combine -> O GEMV -> SwiGLU GEMV -> down GEMV with the
    LDS-DMA loader streaming weights ahead across every stage edge).
    Replaces six launch-path kernels; see csrc/stream_layer.hip."""
    lib = require_lib()
    lib.fei_stream_layer(
        _ptr(x_in), _ptr(h_out), _ptr(lw.wqkv), _ptr(lw.wo), _ptr(lw.wgu),
        _ptr(lw.wdown), _ptr(lw.norm_attn), _ptr(lw.norm_mlp),
        _ptr(k_cache), _ptr(v_cache), _ptr(cos_sin), _ptr(pos),
        _ptr(ws["g_qkv"]), _ptr(ws["g_att"]),
        _ptr(ws["g_h2"]), _ptr(ws["g_act"]), _ptr(ws["g_done"]),
        _ptr(ws["dbg"]) if "dbg" in ws else None,
        _ptr(ws["fail"]),
        spec.hidden_size, spec.num_heads, spec.num_kv_heads, spec.head_dim,
        spec.intermediate_size, k_cache.shape[-2], layer, spec.norm_eps,
        scale, _stream())


def advance(pos: torch.Tensor, step: torch.Tensor,
            max_pos: int = 1 << 30) -> None:
    """pos[b] = min(pos[b]+1, max_pos); step += 1 (device-side,
    graph-capturable). max_pos guards the RoPE table / KV cache against
    out-of-bounds indexing when a caller decodes at capacity."""
    if not pos.is_cuda:
        pos.clamp_(max=max_pos - 1)
        pos += 1
        step += 1
        return
    lib = require_lib()
    lib.fei_advance(_ptr(pos), _ptr(step), pos.shape[0], max_pos, _stream())


def mfma_probe(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """GPU-only: 16x32 @ 32x16 through one MFMA with the kernels' fragment
    maps; falsifies layout assumptions (tests/test_ops_gpu.py)."""
    lib = require_lib()
    C = torch.empty(16, 16, dtype=torch.float32, device=A.device)
    lib.fei_mfma_probe(_ptr(A.contiguous()), _ptr(B.contiguous()), _ptr(C),
                       _stream())
    return C


# -- decode GEMV dispatch ----------------------------------------------------

# Nontemporal weight loads for ALL decode GEMVs: in the real decode loop
# every weight byte is cache-cold (the 15 GB per-step cycle flushes the
# 256 MB L3), so NT never hurts and avoids polluting L2/L3 for the hot
# activations — measured 257.2 vs 255.6 tok/s on the 8B headline. The
# microbench that suggested a 512 MB threshold was L3-warm across runs.
# FEI_GEMV_NT_MIN (bytes) restores a threshold.
_GEMV_NT_MIN_BYTES = int(os.environ.get("FEI_GEMV_NT_MIN", 0))
# Fused split-K combine in decode attention (per-head reducer splits poll
# sc1 done-flags and reduce the partials in-kernel; needs the 3-element
# workspace). Verified token-identical and measured at PARITY with the
# separate k_attn_decode_combine launch (275.5 vs 275.8 tok/s on the 8B
# chain — in a captured graph the combine launch already overlaps the
# attention grid's drain, so there was no boundary to win; the full
# 4-protocol measurement ladder is profiles/r02_fused_combine.md).
# Opt-in via FEI_FUSED_CMB=1; the launch form stays the default.
_FUSED_CMB = os.environ.get("FEI_FUSED_CMB", "0") == "1"
# Split-K combine and one-pass sampler with every load issued before the
# first wait (k_attn_decode_combine_flat at 16 and 32 splits,
# k_sample_onepass_flat up to vocab 131072), bit-identical to the looping
# kernels they replace. Both read what other XCDs have just written, so each
# dependent load was a full trip to memory. FEI_CMB_FLAT=0 / FEI_SAMPLE_FLAT=0
# restore the looping kernels for A/B inside one build
# (profiles/combine_sample_flat.md).
_CMB_FLAT = os.environ.get("FEI_CMB_FLAT", "1") != "0"
_SAMPLE_FLAT = os.environ.get("FEI_SAMPLE_FLAT", "1") != "0"
# Batch-1 plain decode chain: run the residual add + RMSNorm in front of the
# gate/up and qkv GEMVs as those GEMVs' prologue (gemv_addnorm /
# gemv_swiglu_addnorm, bit-identical to the launches they replace) instead
# of 63 single-workgroup k_add_rmsnorm launches per step. FEI_ADDNORM_GEMV=0
# restores the launches for A/B inside one build
# (profiles/gemv_addnorm.md).
_ADDNORM_GEMV = os.environ.get("FEI_ADDNORM_GEMV", "1") == "1"
# Batch-1 GEMVs whose grid is too small to hide HBM latency with occupancy
# (o and down at N = 4096: 2 workgroups per CU) run the deep-pipelined
# k_gemv_deep, bit-identical to k_gemv. The gate is workgroups per CU, not a
# shape: below _GEMV_DEEP_MAX_WG_PER_CU the plain kernel cannot fill a CU's
# 8 resident workgroups. FEI_GEMV_DEEP=0 restores k_gemv everywhere for A/B
# inside one build (profiles/gemv_deep.md).
_GEMV_DEEP = os.environ.get("FEI_GEMV_DEEP", "1") == "1"
_GEMV_DEEP_MAX_WG_PER_CU = float(
    os.environ.get("FEI_GEMV_DEEP_MAX_WG_PER_CU", "8") or 8)
_GEMV_DEEP_MAX_TRIPS = 8           # trips of 4096 columns, as in gemv.hip
_CU_COUNT: dict = {}


def _gemm_m8_ok(M: int, N: int, K: int) -> bool:
    # MFMA GEMM tile: A-fragment rows clamp to M-1 so M <= 16 is CORRECT,
    # but at M = 16 hipBLASLt measured faster (serving-16: 2473 vs 2337
    # tok/s) — route only the 4..8 range where the tile wins 1.27-1.65x
    return 4 <= M <= 8 and K % 1024 == 0 and N % 16 == 0


def _gemv_ok(M: int, K: int) -> bool:
    return M in (1, 2, 4, 8) and K % 8 == 0


def _cu_count(device: torch.device) -> int:
    idx = device.index if device.index is not None else \
        torch.cuda.current_device()
    if idx not in _CU_COUNT:
        _CU_COUNT[idx] = torch.cuda.get_device_properties(
            idx).multi_processor_count
    return _CU_COUNT[idx]


def _gemv_deep_ok(M: int, K: int) -> bool:
    return (M == 1 and K > 0 and K % 8 == 0
            and -(-K // 4096) <= _GEMV_DEEP_MAX_TRIPS)


def _gemv_deep_wins(N: int, K: int, device: torch.device) -> bool:
    """The dispatch rule: k_gemv's grid ((N + 7) // 8 workgroups) leaves the
    CUs short of resident waves."""
    return (_GEMV_DEEP and _gemv_deep_ok(1, K)
            and (N + 7) // 8 < _GEMV_DEEP_MAX_WG_PER_CU * _cu_count(device))


def linear_decode(x: torch.Tensor, w: torch.Tensor,
                  out: Optional[torch.Tensor] = None,
                  deep: Optional[bool] = None) -> torch.Tensor:
    """F.linear for skinny M: hand-rolled streaming GEMV on GPU
    (profiles/r01: rocBLAS reaches ~4 TB/s on M=1; streaming reaches the
    flat-read ceiling). Falls back to torch for unsupported shapes/CPU.

    ``deep`` picks the batch-1 kernel: True the deep-pipelined k_gemv_deep
    (an error where it does not apply), False k_gemv, None the dispatch rule
    (_gemv_deep_wins). Both give the same bits."""
    M = x.numel() // x.shape[-1]
    K = x.shape[-1]
    N = w.shape[0]
    if not x.is_cuda or not (_gemv_ok(M, K) or _gemm_m8_ok(M, N, K)):
        return torch.nn.functional.linear(x, w)
    lib = require_lib()
    x2 = x.contiguous().view(M, K)
    if out is None:
        out = torch.empty(*x.shape[:-1], N, dtype=x.dtype, device=x.device)
    nt = 1 if (N * K * 2 >= _GEMV_NT_MIN_BYTES) else 0
    if _gemm_m8_ok(M, N, K):
        # MFMA tile: beats the VALU GEMV at every llama batch shape
        # (1.27-1.65x — profiles/r02_batch_attention.md addendum).
        # ALWAYS plain loads: the nt hint on the 16 B/lane staged W
        # fetch measured 6.50 vs 5.01 ms/step at batch 8.
        lib.fei_gemm_m8(_ptr(out), _ptr(x2), _ptr(w), M, N, K, 0,
                        _stream())
        return out
    if deep is None:
        deep = M == 1 and _gemv_deep_wins(N, K, x.device)
    if deep:
        rc = lib.fei_gemv_deep(_ptr(out), _ptr(x2), _ptr(w), M, N, K, nt,
                               _stream())
        if rc != 0:
            raise ValueError(
                f"gemv_deep does not take M={M} N={N} K={K} (code {rc})")
        return out
    lib.fei_gemv(_ptr(out), _ptr(x2), _ptr(w), M, N, K, nt, _stream())
    return out


def gemv_swiglu(x: torch.Tensor, wgu: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused gate/up GEMV + SwiGLU: x [M,K] @ [2I,K]^T -> silu(g)*u [M,I]."""
    M = x.numel() // x.shape[-1]
    K = x.shape[-1]
    I = wgu.shape[0] // 2
    if not x.is_cuda:
        # the reference has no vector width: any I
        return ref.swiglu(torch.nn.functional.linear(x, wgu))
    if not (_gemv_ok(M, K) or _gemm_m8_ok(M, 2 * I, K)):
        return swiglu(torch.nn.functional.linear(x, wgu))
    lib = require_lib()
    x2 = x.contiguous().view(M, K)
    if out is None:
        out = torch.empty(*x.shape[:-1], I, dtype=x.dtype, device=x.device)
    nt = 1 if (2 * I * K * 2 >= _GEMV_NT_MIN_BYTES) else 0
    if _gemm_m8_ok(M, 2 * I, K):
        # MFMA over the stacked [2I, K] weight (its [M, 2I] output is
        # k_swiglu's packed input): 68.3 -> ~47 us on the 8B gate/up at
        # batch 8 vs the fused VALU kernel
        gu = torch.empty(M, 2 * I, dtype=x.dtype, device=x.device)
        lib.fei_gemm_m8(_ptr(gu), _ptr(x2), _ptr(wgu), M, 2 * I, K, 0,
                        _stream())
        lib.fei_swiglu(_ptr(out), _ptr(gu), M, I, _stream())
        return out
    lib.fei_gemv_swiglu(_ptr(out), _ptr(x2), _ptr(wgu), M, I, K, nt,
                        _stream())
    return out


def gemv_res(x: torch.Tensor, w: torch.Tensor, res: torch.Tensor,
             ssq_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """res += x @ w^T (epilogue residual add; in place on res [M,N]).

    ``ssq_out`` [M] f32, pre-zeroed: the kernel also accumulates the
    sum-of-squares of the updated residual rows so a following
    gemv_norm/gemv_swiglu_norm can skip its sumsq prologue pass (pass the
    same tensor as their ``ssq``). Ignored on the CPU fallback — consumers
    recompute exactly there."""
    M = x.numel() // x.shape[-1]
    K = x.shape[-1]
    N = w.shape[0]
    if not x.is_cuda or not _gemv_ok(M, K):
        lin = torch.nn.functional.linear(x, w)
        res.copy_((res.float() + lin.float().view_as(res)).to(res.dtype))
        return res
    lib = require_lib()
    x2 = x.contiguous().view(M, K)
    nt = 1 if (N * K * 2 >= _GEMV_NT_MIN_BYTES) else 0
    lib.fei_gemv_res(_ptr(res), _ptr(x2), _ptr(w), M, N, K, nt,
                     _ptr(ssq_out) if ssq_out is not None else None,
                     _stream())
    return res


def gemv_norm(res: torch.Tensor, wnorm: torch.Tensor, w: torch.Tensor,
              eps: float = 1e-5,
              out: Optional[torch.Tensor] = None,
              ssq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = rmsnorm(res)*wnorm @ w^T (norm-prologue GEMV).

    ``ssq`` [M] f32: precomputed sum-of-squares of res rows (from a prior
    gemv_res ``ssq_out``); skips the prologue pass over res."""
    M = res.numel() // res.shape[-1]
    K = res.shape[-1]
    N = w.shape[0]
    if not res.is_cuda or not _gemv_ok(M, K):
        return torch.nn.functional.linear(rmsnorm(res, wnorm, eps), w)
    lib = require_lib()
    r2 = res.contiguous().view(M, K)
    if out is None:
        out = torch.empty(*res.shape[:-1], N, dtype=res.dtype, device=res.device)
    nt = 1 if (N * K * 2 >= _GEMV_NT_MIN_BYTES) else 0
    lib.fei_gemv_norm(_ptr(out), _ptr(r2), _ptr(wnorm), _ptr(w), M, N, K,
                      eps, nt, _ptr(ssq) if ssq is not None else None,
                      _stream())
    return out


def gemv_swiglu_norm(res: torch.Tensor, wnorm: torch.Tensor,
                     wgu: torch.Tensor, eps: float = 1e-5,
                     out: Optional[torch.Tensor] = None,
                     ssq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = silu(g)*u where [g;u] = rmsnorm(res)*wnorm @ wgu^T.
    ``ssq``: see gemv_norm."""
    M = res.numel() // res.shape[-1]
    K = res.shape[-1]
    I = wgu.shape[0] // 2
    if not res.is_cuda or not _gemv_ok(M, K):
        # normed activation rounds to res.dtype, g/u stay f32 through silu
        # (the kernel's semantics)
        gu = torch.nn.functional.linear(rmsnorm(res, wnorm, eps).float(),
                                        wgu.float())
        return ref.swiglu(gu).to(res.dtype)
    lib = require_lib()
    r2 = res.contiguous().view(M, K)
    if out is None:
        out = torch.empty(*res.shape[:-1], I, dtype=res.dtype, device=res.device)
    nt = 1 if (wgu.shape[0] * K * 2 >= _GEMV_NT_MIN_BYTES) else 0
    lib.fei_gemv_swiglu_norm(_ptr(out), _ptr(r2), _ptr(wnorm), _ptr(wgu),
                             M, I, K, eps, nt,
                             _ptr(ssq) if ssq is not None else None,
                             _stream())
    return out


# -- residual add + RMSNorm folded into the consuming GEMV -------------------

# The ring schedule (K <= 4096): a wave refills each weight slot with the
# next row group's as soon as it has been dotted, and groups are dealt
# grid-stride. FEI_ADDNORM_RING=0 restores the drain-between-groups kernels
# with contiguous groups, 2 per workgroup unless a count is forced.
_ADDNORM_RING = os.environ.get("FEI_ADDNORM_RING", "1") != "0"

# Row groups one workgroup walks behind a single add+norm prologue (a group
# is 8 rows in gemv_addnorm, 4 in gemv_swiglu_addnorm). Pure scheduling: a
# row's sum does not depend on which workgroup owns it. 0 = automatic: one
# resident round of workgroups covers every group (_addnorm_plan); measured
# behind the fixed counts below at 8B, so opt-in.
# FEI_ADDNORM_RG / FEI_ADDNORM_RG_SWIGLU override
# (profiles/gemv_addnorm.md, profiles/gemv_addnorm_ring.md).
_ADDNORM_DRAIN_RG = 2
_ADDNORM_RG_DEFAULT = 2
_ADDNORM_RG_SWIGLU_DEFAULT = 5 if _ADDNORM_RING else _ADDNORM_DRAIN_RG
_ADDNORM_ROW_GROUPS = max(0, int(
    os.environ.get("FEI_ADDNORM_RG", "") or _ADDNORM_RG_DEFAULT))
_ADDNORM_ROW_GROUPS_SWIGLU = max(0, int(
    os.environ.get("FEI_ADDNORM_RG_SWIGLU", "") or _ADDNORM_RG_SWIGLU_DEFAULT))

_ADDNORM_RING_MAX_K = 4096           # the preload holds the whole row slice
_ADDNORM_RING_MAX_TRIPS = 8          # kernel instances, one per trip count


def _addnorm_plan(groups: int, slots: int,
                  max_trips: int = _ADDNORM_RING_MAX_TRIPS) -> Tuple[int, int]:
    """(grid, trips) of the automatic rule: min(groups, slots) workgroups,
    each walking group = block + g * grid for g < trips, so trip counts are
    at most one apart. More than max_trips * slots groups need further
    rounds: the grid then grows past `slots` at max_trips."""
    if groups < 1 or slots < 1:
        raise ValueError("groups and slots must be positive")
    grid = min(groups, slots)
    trips = -(-groups // grid)
    if trips > max_trips:
        trips = max_trips
        grid = -(-groups // trips)
    return grid, trips


def _addnorm_fixed_plan(groups: int, rg: int) -> Tuple[int, int]:
    """(grid, trips) for a forced count of groups per workgroup."""
    return -(-groups // rg), rg


_ADDNORM_SLOTS: dict = {}
_ADDNORM_PLANS: dict = {}


def _addnorm_slots(swiglu: bool, nt: int, trips: int, K: int) -> int:
    """Workgroups of one ring kernel instance the device holds at once (the
    occupancy query, once per instance and K)."""
    key = (bool(swiglu), int(nt), int(trips), int(K),
           torch.cuda.current_device())
    slots = _ADDNORM_SLOTS.get(key)
    if slots is None:
        slots = require_lib().fei_gemv_addnorm_ring_slots(
            int(swiglu), int(nt), int(trips), int(K))
        if slots < 1:
            raise RuntimeError(
                f"fei_gemv_addnorm_ring_slots failed (rc={slots})")
        _ADDNORM_SLOTS[key] = slots
    return slots


def _addnorm_auto_plan(swiglu: bool, nt: int, K: int,
                       groups: int) -> Tuple[int, int]:
    """The automatic plan on this device. An instance's slots depend on its
    trip count and the trip count on the slots: take the smallest trip count
    whose own instance covers every group in one round."""
    key = (bool(swiglu), int(nt), int(K), int(groups),
           torch.cuda.current_device())
    plan = _ADDNORM_PLANS.get(key)
    if plan is None:
        for t in range(1, _ADDNORM_RING_MAX_TRIPS + 1):
            plan = _addnorm_plan(groups, _addnorm_slots(swiglu, nt, t, K))
            if plan[1] <= t:
                break
        _ADDNORM_PLANS[key] = plan
    return plan


def _addnorm_launch(swiglu: bool, rg: int, out, delta, res_in, res_out, wnorm,
                    w, M: int, N: int, K: int, eps: float, nt: int) -> None:
    lib = require_lib()
    name = "fei_gemv_swiglu_addnorm" if swiglu else "fei_gemv_addnorm"
    ptrs = (_ptr(out), _ptr(delta), _ptr(res_in), _ptr(res_out), _ptr(wnorm),
            _ptr(w))
    if (_ADDNORM_RING and K <= _ADDNORM_RING_MAX_K
            and rg <= _ADDNORM_RING_MAX_TRIPS):
        groups = -(-N // (4 if swiglu else 8))
        grid, trips = (_addnorm_fixed_plan(groups, rg) if rg >= 1 else
                       _addnorm_auto_plan(swiglu, nt, K, groups))
        name += "_ring"
        rc = getattr(lib, name)(*ptrs, M, N, K, eps, nt, grid, trips,
                                _stream())
    else:
        rc = getattr(lib, name)(*ptrs, M, N, K, eps, nt,
                                rg if rg >= 1 else _ADDNORM_DRAIN_RG,
                                _stream())
    if rc != 0:
        raise RuntimeError(f"{name} refused the launch (rc={rc})")


def _addnorm_ok(M: int, K: int) -> bool:
    # batch 1 only, and the normalised row is staged in LDS (32 KB cap, the
    # one forward_decode uses for the norm-prologue chain)
    return M == 1 and _gemv_ok(M, K) and M * K * 2 <= 32 * 1024


def _addnorm_check(name: str, delta, res_in, res_out) -> None:
    if not res_in.is_contiguous() or not res_out.is_contiguous():
        raise ValueError(f"{name}: res_in and res_out must be contiguous")
    if res_in.shape != res_out.shape or res_in.dtype != res_out.dtype:
        raise ValueError(f"{name}: res_in and res_out must match in shape "
                         "and dtype")
    if delta.shape != res_in.shape:
        raise ValueError(f"{name}: delta must have the residual's shape")
    # every workgroup reads res_in while one of them writes res_out: the two
    # may not share storage, wholly or in part
    a0, b0 = res_in.data_ptr(), res_out.data_ptr()
    nbytes = res_in.numel() * res_in.element_size()
    if a0 < b0 + nbytes and b0 < a0 + nbytes:
        raise ValueError(f"{name}: res_in and res_out must not share storage "
                         "(the new residual cannot be written in place)")


def gemv_addnorm(delta: torch.Tensor, res_in: torch.Tensor,
                 res_out: torch.Tensor, wnorm: torch.Tensor, w: torch.Tensor,
                 eps: float = 1e-5,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """res_out = res_in + delta; out = rmsnorm(res_out)*wnorm @ w^T in ONE
    kernel at batch 1 — bit-identical to fused_add_rmsnorm followed by
    linear_decode, which is also what every other shape and the CPU run
    (through res_out; res_in is left untouched)."""
    _addnorm_check("gemv_addnorm", delta, res_in, res_out)
    K = res_in.shape[-1]
    M = res_in.numel() // max(K, 1)
    N = w.shape[0]
    if not res_in.is_cuda or not _addnorm_ok(M, K):
        res_out.copy_(res_in)
        x, _ = fused_add_rmsnorm(delta, res_out, wnorm, eps)
        return linear_decode(x, w, out=out)
    lib = require_lib()
    d2 = delta.contiguous()
    if out is None:
        out = torch.empty(*res_in.shape[:-1], N, dtype=res_in.dtype,
                          device=res_in.device)
    nt = 1 if (N * K * 2 >= _GEMV_NT_MIN_BYTES) else 0
    _addnorm_launch(False, _ADDNORM_ROW_GROUPS, out, d2, res_in, res_out,
                    wnorm, w, M, N, K, eps, nt)
    return out


def gemv_swiglu_addnorm(delta: torch.Tensor, res_in: torch.Tensor,
                        res_out: torch.Tensor, wnorm: torch.Tensor,
                        wgu: torch.Tensor, eps: float = 1e-5,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """res_out = res_in + delta; out = silu(g)*u with [g;u] =
    rmsnorm(res_out)*wnorm @ wgu^T in ONE kernel at batch 1 — bit-identical
    to fused_add_rmsnorm followed by gemv_swiglu (the fallback for every
    other shape and the CPU)."""
    _addnorm_check("gemv_swiglu_addnorm", delta, res_in, res_out)
    K = res_in.shape[-1]
    M = res_in.numel() // max(K, 1)
    I = wgu.shape[0] // 2
    if not res_in.is_cuda or not _addnorm_ok(M, K):
        res_out.copy_(res_in)
        x, _ = fused_add_rmsnorm(delta, res_out, wnorm, eps)
        return gemv_swiglu(x, wgu, out=out)
    lib = require_lib()
    d2 = delta.contiguous()
    if out is None:
        out = torch.empty(*res_in.shape[:-1], I, dtype=res_in.dtype,
                          device=res_in.device)
    nt = 1 if (wgu.shape[0] * K * 2 >= _GEMV_NT_MIN_BYTES) else 0
    _addnorm_launch(True, _ADDNORM_ROW_GROUPS_SWIGLU, out, d2, res_in,
                    res_out, wnorm, wgu, M, I, K, eps, nt)
    return out


def prefetch(w: torch.Tensor, max_bytes: int, sink: torch.Tensor,
             n_blocks: int = 512, stream=None) -> None:
    """Stream the first ``max_bytes`` of ``w`` through cache-filling loads
    (L2/L3 prefill for a later kernel's reads). GPU-only no-op helper for
    the decode prefetch experiment; launched on a side stream."""
    if not w.is_cuda:
        return
    lib = require_lib()
    bytes_ = min(max_bytes, w.numel() * w.element_size())
    sp = stream if stream is not None else _stream()
    lib.fei_prefetch(_ptr(w), bytes_, _ptr(sink), n_blocks, sp)


def attn_decode_paged(q, k_pool, v_pool, block_table, pos, splits: int = 32,
                      scale: Optional[float] = None,
                      workspace: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                      out: Optional[torch.Tensor] = None,
                      k: Optional[torch.Tensor] = None,
                      v: Optional[torch.Tensor] = None,
                      table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode attention over a PAGED KV pool (engine/kv_cache.PagedKVPool):
    pools [num_blocks, Hkv, BS, D], block_table [B, max_blocks] int32 maps
    logical key blocks to physical pool blocks. n = pos[b]+1 keys.
    When (k, v, table) are given the kernel also fuses the step's RoPE +
    paged KV-append: q is the RAW qkv view and the pool row for position
    pos[b] is written in-kernel (mirrors attn_decode's fused form).
    QuantKV pools (data [num_blocks, Hkv, BS, D], scale [num_blocks, Hkv,
    BS]) run the fp8 kernel (kv_fp8_paged.hip): bit-equal to attn_decode
    over a contiguous QuantKV holding the same rows."""
    if _kv8_pair(k_pool, v_pool):
        return _attn_decode_paged_kv8(q, k_pool, v_pool, block_table, pos,
                                      splits, scale, workspace, out, k, v,
                                      table)
    B, Hq, D = q.shape
    n_blocks, Hkv, BS, _ = k_pool.shape
    assert BS & (BS - 1) == 0, "block size must be a power of two"
    bs_log = BS.bit_length() - 1
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if not q.is_cuda:
        if table is not None:
            # reference path: rope q/k and append into the POOL rows
            q = ref.apply_rope(q, pos.long(), table).to(q.dtype)
            k_r = ref.apply_rope(k, pos.long(), table).to(k.dtype)
            for b in range(B):
                p = int(pos[b])
                blk = int(block_table[b, p >> bs_log])
                k_pool[blk, :, p & (BS - 1), :] = k_r[b]
                v_pool[blk, :, p & (BS - 1), :] = v[b]
        # gather logical order into a contiguous cache, then reference
        max_len = block_table.shape[1] * BS
        kc = torch.zeros(B, Hkv, max_len, D, dtype=k_pool.dtype)
        vc = torch.zeros_like(kc)
        for b in range(B):
            for j, blk in enumerate(block_table[b].tolist()):
                if blk < 0:
                    continue
                kc[b, :, j * BS:(j + 1) * BS] = k_pool[blk]
                vc[b, :, j * BS:(j + 1) * BS] = v_pool[blk]
        return ref.attn_decode(q, kc, vc, pos + 1, scale)
    lib = require_lib()
    _check_gqa("attn_decode_paged", Hq, Hkv)
    if workspace is None:
        part_o = torch.empty(B, Hq, splits, D, dtype=torch.float32, device=q.device)
        part_ml = torch.empty(B, Hq, splits, 2, dtype=torch.float32, device=q.device)
    else:
        part_o, part_ml = workspace
        assert part_o.shape[2] == splits and part_ml.shape[2] == splits
    if out is None:
        out = torch.empty_like(q)
    assert q.stride(2) == 1 and q.stride(1) == D
    assert D in (64, 128), f"paged attention supports D in (64,128), got {D}"
    assert splits <= 64
    if table is not None:
        assert k is not None and v is not None
        assert k.stride(1) == D and k.stride(0) == v.stride(0)
        kin, vin, cs, kv_bs = _ptr(k), _ptr(v), _ptr(table), k.stride(0)
    else:
        kin = vin = cs = None
        kv_bs = 0
    lib.fei_attn_decode_paged(_ptr(q), _ptr(k_pool), _ptr(v_pool),
                              _ptr(block_table), _ptr(part_o), _ptr(part_ml),
                              _ptr(pos), B, Hq, Hkv, D, bs_log,
                              block_table.shape[1], splits, scale,
                              q.stride(0), kin, vin, cs, kv_bs, _stream())
    lib.fei_attn_decode_combine(_ptr(out), _ptr(part_o), _ptr(part_ml),
                                B, Hq, D, splits, int(_CMB_FLAT), _stream())
    return out


# -- prefill over a paged KV pool (csrc/attn_prefill_paged.hip) --------------

def _paged_check(name: str, q, k_pool, block_table, pos0) -> Tuple[int, int]:
    """Shared argument checks of the paged prefill ops; returns (Hkv, BS)."""
    B, S, Hq, D = q.shape
    Hkv, BS = k_pool.shape[1], k_pool.shape[2]
    if Hkv <= 0 or Hq % Hkv != 0:
        raise ValueError(f"{name}: Hq={Hq} is not a multiple of Hkv={Hkv}")
    if BS <= 0 or BS & (BS - 1):
        raise ValueError(f"{name}: block size must be a power of two, "
                         f"got {BS}")
    if q.is_cuda and D not in (64, 128):
        raise ValueError(f"{name} supports D in (64,128), got {D}")
    if block_table.dim() != 2 or block_table.shape[0] != B or \
            block_table.dtype != torch.int32:
        raise ValueError(f"{name}: block_table must be int32 [B, max_blocks]")
    if not pos0.is_cuda and B > 0 and \
            block_table.shape[1] * BS < int(pos0.max()) + S:
        raise ValueError(
            f"{name}: block_table covers {block_table.shape[1] * BS} rows, "
            f"the prefill reaches row {int(pos0.max()) + S}")
    return Hkv, BS


def _gather_pool(pool: torch.Tensor, block_table: torch.Tensor,
                 n_rows) -> torch.Tensor:
    """Contiguous [B, Hkv, max(n_rows), D] copy of the first n_rows[b] logical
    rows of every sequence (reference path). Table entries past a sequence's
    last needed block are never looked at (production tables hold -1)."""
    _, Hkv, BS, D = pool.shape
    B = block_table.shape[0]
    out = pool.new_zeros(B, Hkv, max(max(n_rows), 1), D)
    for b in range(B):
        for j in range(0, n_rows[b], BS):
            n = min(BS, n_rows[b] - j)
            out[b, :, j:j + n] = pool[int(block_table[b, j // BS]), :, :n]
    return out


def _gather_pool_kv8(pool: QuantKV, block_table: torch.Tensor,
                     n_rows) -> torch.Tensor:
    """_gather_pool of an fp8 pool, dequantised: f32 [B, Hkv, max(n_rows), D]
    (reference path; rows past n_rows[b] are zero)."""
    data = _gather_pool(pool.data, block_table, n_rows)
    scale = _gather_pool(pool.scale.unsqueeze(-1), block_table,
                         n_rows).squeeze(-1)
    return ref.dequant_kv_fp8(data, scale)


def _scatter_pool_kv8(pool: QuantKV, block_table: torch.Tensor, b: int,
                      p: int, codes: torch.Tensor, scales: torch.Tensor):
    """Write one logical row (codes [Hkv, D], scales [Hkv]) of sequence b
    through the table (reference path)."""
    BS = pool.shape[2]
    blk = int(block_table[b, p // BS])
    pool.data[blk, :, p % BS, :] = codes
    pool.scale[blk, :, p % BS] = scales


def _attn_decode_paged_kv8(q, k_pool, v_pool, block_table, pos, splits, scale,
                           workspace, out, k, v, table) -> torch.Tensor:
    B, Hq, D = q.shape
    _, Hkv, BS, _ = k_pool.shape
    name = "attn_decode_paged (fp8)"
    if BS <= 0 or BS & (BS - 1):
        raise ValueError(f"{name}: block size must be a power of two, "
                         f"got {BS}")
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if not q.is_cuda:
        if table is not None:
            # the contiguous reference append (ref.rope_kv_decode_fp8): K
            # roped and rounded to k.dtype, then quantised per row
            q = ref.apply_rope(q, pos.long(), table)
            kq, ks = ref.quant_kv_fp8(ref.apply_rope(k, pos.long(), table))
            vq, vs = ref.quant_kv_fp8(v)
            for b in range(B):
                p = int(pos[b])
                _scatter_pool_kv8(k_pool, block_table, b, p, kq[b], ks[b])
                _scatter_pool_kv8(v_pool, block_table, b, p, vq[b], vs[b])
        n_rows = [int(pos[b]) + 1 for b in range(B)]
        return ref.attn_decode(q, _gather_pool_kv8(k_pool, block_table, n_rows),
                               _gather_pool_kv8(v_pool, block_table, n_rows),
                               pos + 1, scale)
    lib = require_lib()
    _check_gqa(name, Hq, Hkv)
    if D not in (64, 128):
        raise ValueError(f"{name} supports D in (64,128), got {D}")
    # the combine kernel stages its 2*splits m/l values with D threads
    if splits <= 0 or 2 * splits > D:
        raise ValueError(f"{name} needs 0 < 2*splits <= D (splits={splits}, "
                         f"D={D})")
    if block_table.dim() != 2 or block_table.shape[0] != B or \
            block_table.dtype != torch.int32 or \
            not block_table.is_contiguous():
        raise ValueError(f"{name}: block_table must be a contiguous int32 "
                         "[B, max_blocks]")
    if workspace is None:
        part_o = torch.empty(B, Hq, splits, D, dtype=torch.float32, device=q.device)
        part_ml = torch.empty(B, Hq, splits, 2, dtype=torch.float32, device=q.device)
    else:
        part_o, part_ml = workspace[0], workspace[1]
        assert part_o.shape[2] == splits and part_ml.shape[2] == splits, \
            f"workspace sized for {part_o.shape[2]} splits, kernel asked {splits}"
    if out is None:
        out = torch.empty_like(q)
    assert q.stride(2) == 1 and q.stride(1) == D
    if table is not None:
        assert k is not None and v is not None
        assert k.stride(1) == D and k.stride(0) == v.stride(0)
        kin, vin, cs, kv_bs = _ptr(k), _ptr(v), _ptr(table), k.stride(0)
    else:
        kin = vin = cs = None
        kv_bs = 0
    rc = lib.fei_attn_decode_paged_kv8(
        _ptr(q), _ptr(k_pool.data), _ptr(k_pool.scale), _ptr(v_pool.data),
        _ptr(v_pool.scale), _ptr(block_table), _ptr(part_o), _ptr(part_ml),
        _ptr(pos), B, Hq, Hkv, D, BS, block_table.shape[1], splits, scale,
        q.stride(0), kin, vin, cs, kv_bs, _stream())
    if rc != 0:
        raise RuntimeError(
            f"fei_attn_decode_paged_kv8 refused the launch (rc={rc})")
    lib.fei_attn_decode_combine(_ptr(out), _ptr(part_o), _ptr(part_ml),
                                B, Hq, D, splits, int(_CMB_FLAT), _stream())
    return out


def rope_kv_prefill_paged(q, k, v, k_pool, v_pool, block_table, pos0,
                          table) -> torch.Tensor:
    """rope_kv_prefill into a PAGED pool: in-place RoPE on q [B,S,Hq,D]; k
    roped + v appended at logical row pos0[b]+s, i.e. pool[block_table[b,
    p >> log2(BS)], :, p & (BS-1), :]. Pools [num_blocks, Hkv, BS, D], BS a
    power of two; block_table [B, max_blocks] int32. Same arithmetic as
    rope_kv_prefill: the rows are bit-equal to the contiguous cache's.

    Contract on GPU (not checked: it would cost a host sync): block_table
    holds a valid block for every row below max(pos0) + S."""
    kv8 = _kv8_pair(k_pool, v_pool)
    Hkv, BS = _paged_check("rope_kv_prefill_paged", q, k_pool, block_table,
                           pos0)
    B, S, Hq, D = q.shape
    if not q.is_cuda and kv8:
        # the contiguous reference append into scratch rows, then the
        # appended codes and scales go through the table
        n = int(pos0.max()) + S if B > 0 else 0
        kc = QuantKV.zeros((B, Hkv, max(n, 1), D), q.device)
        vc = QuantKV.zeros((B, Hkv, max(n, 1), D), q.device)
        q_out = ref.rope_kv_prefill_fp8(q, k, v, kc.data, kc.scale, vc.data,
                                        vc.scale, pos0, table)
        for b in range(B):
            for p in range(int(pos0[b]), int(pos0[b]) + S):
                _scatter_pool_kv8(k_pool, block_table, b, p,
                                  kc.data[b, :, p], kc.scale[b, :, p])
                _scatter_pool_kv8(v_pool, block_table, b, p,
                                  vc.data[b, :, p], vc.scale[b, :, p])
        q.copy_(q_out)
        return q
    if not q.is_cuda:
        n = int(pos0.max()) + S if B > 0 else 0
        kc = k_pool.new_zeros(B, Hkv, max(n, 1), D)
        vc = torch.zeros_like(kc)
        q_out = ref.rope_kv_prefill(q, k, v, kc, vc, pos0, table)
        bs_log = BS.bit_length() - 1
        for b in range(B):
            for p in range(int(pos0[b]), int(pos0[b]) + S):
                blk = int(block_table[b, p >> bs_log])
                k_pool[blk, :, p & (BS - 1)] = kc[b, :, p]
                v_pool[blk, :, p & (BS - 1)] = vc[b, :, p]
        q.copy_(q_out)
        return q
    lib = require_lib()
    assert q.stride(3) == 1 and q.stride(2) == D
    assert q.stride(0) == S * q.stride(1), "token rows must be uniform"
    assert k.stride(2) == D and k.stride(0) == S * k.stride(1)
    assert k.stride(1) == v.stride(1)
    assert block_table.is_contiguous()
    if kv8:
        # (QuantKV asserts its own contiguity and alignment)
        rc = lib.fei_rope_kv8_prefill_paged(
            _ptr(q), _ptr(k), _ptr(v), _ptr(k_pool.data), _ptr(k_pool.scale),
            _ptr(v_pool.data), _ptr(v_pool.scale), _ptr(block_table),
            _ptr(table), _ptr(pos0), B, S, Hq, Hkv, D, BS,
            block_table.shape[1], q.stride(1), k.stride(1), _stream())
        if rc != 0:
            raise RuntimeError(
                f"fei_rope_kv8_prefill_paged refused the launch (rc={rc})")
        return q
    assert k_pool.is_contiguous() and v_pool.is_contiguous()
    rc = lib.fei_rope_kv_prefill_paged(
        _ptr(q), _ptr(k), _ptr(v), _ptr(k_pool), _ptr(v_pool),
        _ptr(block_table), _ptr(table), _ptr(pos0), B, S, Hq, Hkv, D, BS,
        block_table.shape[1], q.stride(1), k.stride(1), _stream())
    if rc != 0:
        raise RuntimeError(
            f"fei_rope_kv_prefill_paged refused the launch (rc={rc})")
    return q


def attn_prefill_paged(q, k_pool, v_pool, block_table, pos0,
                       scale: Optional[float] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal GQA attention of q [B,S,Hq,D] (roped) over a PAGED pool: q
    token s attends the logical rows [0, pos0[b]+s] of sequence b. Pools
    [num_blocks, Hkv, BS, D], BS a power of two; block_table [B, max_blocks]
    int32. Bit-equal to attn_prefill over the gathered rows. Table entries
    of blocks no row below pos0[b]+S lives in are never read (-1 is fine).

    Contract on GPU (not checked: it would cost a host sync): block_table
    holds a valid block for every row below max(pos0) + S."""
    kv8 = _kv8_pair(k_pool, v_pool)
    Hkv, BS = _paged_check("attn_prefill_paged", q, k_pool, block_table, pos0)
    B, S, Hq, D = q.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if not q.is_cuda:
        n_rows = [int(pos0[b]) + S for b in range(B)]
        if kv8:
            kc = _gather_pool_kv8(k_pool, block_table, n_rows)
            vc = _gather_pool_kv8(v_pool, block_table, n_rows)
            if q.dtype == torch.bfloat16:
                # bf16 run: the kernel stages bf16(f32(code) * scale)
                kc, vc = kc.to(q.dtype), vc.to(q.dtype)
        else:
            kc = _gather_pool(k_pool, block_table, n_rows)
            vc = _gather_pool(v_pool, block_table, n_rows)
        res = ref.attn_prefill(q, kc, vc, pos0, scale)
        if out is not None:
            out.copy_(res)
            return out
        return res
    lib = require_lib()
    if out is None:
        out = torch.empty(B, S, Hq, D, dtype=q.dtype, device=q.device)
    assert q.stride(3) == 1 and q.stride(2) == D
    assert q.stride(0) == S * q.stride(1)
    assert out.is_contiguous()
    assert block_table.is_contiguous()
    if kv8:
        rc = lib.fei_attn_prefill_paged_kv8(
            _ptr(q), _ptr(k_pool.data), _ptr(k_pool.scale),
            _ptr(v_pool.data), _ptr(v_pool.scale), _ptr(block_table),
            _ptr(out), _ptr(pos0), B, S, Hq, Hkv, D, BS,
            block_table.shape[1], scale, q.stride(1), _stream())
        if rc != 0:
            raise RuntimeError(
                f"fei_attn_prefill_paged_kv8 refused the launch (rc={rc})")
        return out
    assert k_pool.is_contiguous() and v_pool.is_contiguous()
    rc = lib.fei_attn_prefill_paged(
        _ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(block_table), _ptr(out),
        _ptr(pos0), B, S, Hq, Hkv, D, BS, block_table.shape[1], scale,
        q.stride(1), _stream())
    if rc != 0:
        raise RuntimeError(
            f"fei_attn_prefill_paged refused the launch (rc={rc})")
    return out


# -- ragged prefill over a paged KV pool (csrc/attn_prefill_ragged.hip) ------

class RaggedBatch:
    """The host-built description of ONE packed prefill forward over a paged
    pool: B sequences of seq_lens[b] tokens, packed back to back (T tokens),
    sequence b's row s being logical KV row pos0[b] + s behind row b of
    block_table [B, W] int32. Built once per forward and reused by every
    layer's rope_kv_prefill_paged_ragged / attn_prefill_paged_ragged.

    On the device: ``cu_seqlens`` int32 [B+1]; ``tile_map`` int32
    [n_tiles, 2], the (sequence, 64-row q tile) work list of the attention
    kernel, n_tiles = sum(ceil(len_b / 64)); ``tok_seq`` int32 [T], each
    packed token's sequence (the append kernel's lookup); ``pos0`` int32 [B];
    ``block_table``; ``last_index`` int64 [B], the packed row of every
    sequence's last token. The four int32 arrays are slices of one buffer:
    one upload. ``seq_lens`` and ``pos0_host`` stay as host lists.

    ``block_size``, when given, checks the table's width here; the ops check
    it against their pool in any case (host integers only, no sync)."""

    Q_TILE = 64

    def __init__(self, seq_lens, pos0, block_table, device,
                 block_size: Optional[int] = None):
        seq_lens = [int(n) for n in seq_lens]
        pos0 = [int(p) for p in pos0]
        if not seq_lens:
            raise ValueError("RaggedBatch: no sequences")
        if len(seq_lens) != len(pos0):
            raise ValueError(
                f"RaggedBatch: {len(seq_lens)} lengths, {len(pos0)} pos0")
        if min(seq_lens) < 1:
            raise ValueError(
                f"RaggedBatch: every length must be >= 1, got {seq_lens}")
        if min(pos0) < 0:
            raise ValueError(f"RaggedBatch: negative pos0 in {pos0}")
        B = len(seq_lens)
        if not torch.is_tensor(block_table) or block_table.dim() != 2 or \
                block_table.shape[0] != B or \
                block_table.dtype != torch.int32:
            raise ValueError("RaggedBatch: block_table must be int32 "
                             f"[B={B}, max_blocks]")
        self.seq_lens, self.pos0_host = seq_lens, pos0
        self.B = B
        self.max_blocks = int(block_table.shape[1])
        if block_size is not None:
            self.check_table("RaggedBatch", int(block_size))
        cu = [0]
        for n in seq_lens:
            cu.append(cu[-1] + n)
        self.T = T = cu[-1]
        tiles, tok_seq = [], []
        for b, n in enumerate(seq_lens):
            for qt in range(-(-n // self.Q_TILE)):
                tiles += [b, qt]
            tok_seq += [b] * n
        self.n_tiles = len(tiles) // 2
        device = torch.device(device)
        self.device = device
        packed = torch.tensor(cu + tiles + tok_seq + pos0,
                              dtype=torch.int32).to(device)
        a, b_, c = B + 1, B + 1 + len(tiles), B + 1 + len(tiles) + T
        self.cu_seqlens = packed[:a]
        self.tile_map = packed[a:b_].view(self.n_tiles, 2)
        self.tok_seq = packed[b_:c]
        self.pos0 = packed[c:]
        self.block_table = block_table.to(device).contiguous()
        self.last_index = torch.tensor([e - 1 for e in cu[1:]],
                                       dtype=torch.int64).to(device)
        self._cu_host = cu

    def rows(self, b: int) -> slice:
        """The packed rows of sequence b."""
        return slice(self._cu_host[b], self._cu_host[b + 1])

    def check_table(self, name: str, BS: int) -> None:
        """ValueError when the table is narrower than a sequence needs."""
        if BS <= 0 or BS & (BS - 1):
            raise ValueError(f"{name}: block size must be a power of two, "
                             f"got {BS}")
        for b, (n, p) in enumerate(zip(self.seq_lens, self.pos0_host)):
            need = -(-(p + n) // BS)
            if self.max_blocks < need:
                raise ValueError(
                    f"{name}: block_table has {self.max_blocks} entries per "
                    f"row, sequence {b} (pos0 {p} + {n} rows, block size "
                    f"{BS}) needs {need}")


def _ragged_check(name: str, q, k_pool, batch: RaggedBatch) -> Tuple[int, int]:
    """Shared argument checks of the ragged paged ops; returns (Hkv, BS)."""
    if q.dim() != 3 or q.shape[0] != batch.T:
        raise ValueError(f"{name}: q must be [T={batch.T}, Hq, D], got "
                         f"{tuple(q.shape)}")
    _, Hq, D = q.shape
    Hkv, BS = k_pool.shape[1], k_pool.shape[2]
    if Hkv <= 0 or Hq % Hkv != 0:
        raise ValueError(f"{name}: Hq={Hq} is not a multiple of Hkv={Hkv}")
    if BS <= 0 or BS & (BS - 1):
        raise ValueError(f"{name}: block size must be a power of two, "
                         f"got {BS}")
    if q.is_cuda and D not in (64, 128):
        raise ValueError(f"{name} supports D in (64,128), got {D}")
    batch.check_table(name, BS)
    if batch.device != q.device:
        raise ValueError(f"{name}: batch lives on {batch.device}, q on "
                         f"{q.device}")
    return Hkv, BS


def rope_kv_prefill_paged_ragged(q, k, v, k_pool, v_pool, batch: RaggedBatch,
                                 table) -> torch.Tensor:
    """rope_kv_prefill_paged for a PACKED batch: in-place RoPE on q
    [T, Hq, D]; k [T, Hkv, D] roped + v appended at logical row pos0[b] + s of
    sequence b for packed row cu[b] + s, through row b of batch.block_table.
    ``table`` is the RoPE cos/sin table. Per sequence the rows are bit-equal
    to rope_kv_prefill_paged's on that sequence alone.

    CPU tensors: the uniform op's reference dispatch, sequence by sequence
    (fp8 pools included). GPU: k_rope_kv_prefill_paged_ragged; an fp8 pool
    has no ragged kernel and raises NotImplementedError."""
    kv8 = _kv8_pair(k_pool, v_pool)
    name = "rope_kv_prefill_paged_ragged"
    Hkv, BS = _ragged_check(name, q, k_pool, batch)
    T, Hq, D = q.shape
    if not q.is_cuda:
        for b in range(batch.B):
            r = batch.rows(b)
            rope_kv_prefill_paged(
                q[r].unsqueeze(0), k[r].unsqueeze(0), v[r].unsqueeze(0),
                k_pool, v_pool, batch.block_table[b:b + 1],
                batch.pos0[b:b + 1], table)
        return q
    if kv8:
        raise NotImplementedError(
            f"{name}: no ragged kernel for an fp8 pool; admit serially "
            "(rope_kv_prefill_paged)")
    lib = require_lib()
    assert q.stride(2) == 1 and q.stride(1) == D
    assert k.stride(2) == 1 and k.stride(1) == D
    assert v.stride(2) == 1 and v.stride(1) == D
    assert k.stride(0) == v.stride(0)
    assert k_pool.is_contiguous() and v_pool.is_contiguous()
    rc = lib.fei_rope_kv_prefill_paged_ragged(
        _ptr(q), _ptr(k), _ptr(v), _ptr(k_pool), _ptr(v_pool),
        _ptr(batch.block_table), _ptr(table), _ptr(batch.pos0),
        _ptr(batch.cu_seqlens), _ptr(batch.tok_seq), T, batch.B, Hq, Hkv, D,
        BS, batch.max_blocks, q.stride(0), k.stride(0), _stream())
    if rc != 0:
        raise RuntimeError(
            f"fei_rope_kv_prefill_paged_ragged refused the launch (rc={rc})")
    return q


def attn_prefill_paged_ragged(q, k_pool, v_pool, batch: RaggedBatch,
                              scale: Optional[float] = None,
                              out: Optional[torch.Tensor] = None
                              ) -> torch.Tensor:
    """attn_prefill_paged for a PACKED batch: packed q row cu[b] + s (roped)
    attends the logical rows [0, pos0[b] + s] of sequence b. q [T, Hq, D];
    returns (or fills the first T rows of) out [T, Hq, D]. One launch over a
    (sequence, q tile) work list; per sequence the rows are bit-equal to
    attn_prefill_paged's on that sequence alone. No table entry of a block
    at or past ceil((pos0[b] + len_b) / BS) is read.

    CPU tensors: the uniform op's reference dispatch, sequence by sequence
    (fp8 pools included). GPU: k_attn_prefill_paged_ragged<D>; an fp8 pool
    raises NotImplementedError."""
    kv8 = _kv8_pair(k_pool, v_pool)
    name = "attn_prefill_paged_ragged"
    Hkv, BS = _ragged_check(name, q, k_pool, batch)
    T, Hq, D = q.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if out is not None and (out.dim() != 3 or out.shape[0] < T or
                            tuple(out.shape[1:]) != (Hq, D)):
        raise ValueError(f"{name}: out must be [>= {T}, {Hq}, {D}], got "
                         f"{tuple(out.shape)}")
    if not q.is_cuda:
        if out is None:
            out = torch.empty(T, Hq, D, dtype=q.dtype)
        for b in range(batch.B):
            r = batch.rows(b)
            out[r] = attn_prefill_paged(
                q[r].unsqueeze(0), k_pool, v_pool,
                batch.block_table[b:b + 1], batch.pos0[b:b + 1],
                scale=scale)[0]
        return out
    if kv8:
        raise NotImplementedError(
            f"{name}: no ragged kernel for an fp8 pool; admit serially "
            "(attn_prefill_paged)")
    lib = require_lib()
    if out is None:
        out = torch.empty(T, Hq, D, dtype=q.dtype, device=q.device)
    assert q.stride(2) == 1 and q.stride(1) == D
    assert out.is_contiguous() and out.dtype == q.dtype
    assert k_pool.is_contiguous() and v_pool.is_contiguous()
    rc = lib.fei_attn_prefill_paged_ragged(
        _ptr(q), _ptr(k_pool), _ptr(v_pool), _ptr(batch.block_table),
        _ptr(out), _ptr(batch.pos0), _ptr(batch.cu_seqlens),
        _ptr(batch.tile_map), batch.n_tiles, T, batch.B, Hq, Hkv, D, BS,
        batch.max_blocks, scale, q.stride(0), _stream())
    if rc != 0:
        raise RuntimeError(
            f"fei_attn_prefill_paged_ragged refused the launch (rc={rc})")
    return out


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm of (x [+ residual]) over the last dim (encoder blocks)."""
    _check_vec8("layernorm", x.shape[-1])
    if x.numel() == 0:
        return torch.empty_like(x) if out is None else out
    if not x.is_cuda:
        return ref.layernorm(x, weight, bias, eps, residual)
    lib = require_lib()
    x2 = x.contiguous()
    rows = x2.numel() // x2.shape[-1]
    if out is None:
        out = torch.empty_like(x2)
    res_ptr = _ptr(residual.contiguous()) if residual is not None else _ptr(x2)
    lib.fei_add_layernorm(_ptr(out), _ptr(x2), res_ptr, _ptr(weight),
                          _ptr(bias), rows, x2.shape[-1], eps,
                          1 if residual is not None else 0, _stream())
    return out


def gelu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact (erf) GELU, element-wise."""
    _check_vec8("gelu", x.numel(), "element count")
    if x.numel() == 0:
        return torch.empty_like(x) if out is None else out
    if not x.is_cuda:
        return ref.gelu(x)
    lib = require_lib()
    x2 = x.contiguous()
    if out is None:
        out = torch.empty_like(x2)
    lib.fei_gelu(_ptr(out), _ptr(x2), x2.numel(), _stream())
    return out


# -- fp8 weight-quantized decode path (OCP e4m3fn; serving mode) -------------

def quant_fp8(w: torch.Tensor):
    """Quantize a weight matrix [N,K] to e4m3fn + per-row fp32 scales."""
    if not w.is_cuda:
        return ref.quant_fp8(w)
    lib = require_lib()
    N, K = w.shape
    w8 = torch.empty(N, K, dtype=torch.uint8, device=w.device)
    scales = torch.empty(N, dtype=torch.float32, device=w.device)
    lib.fei_quant_fp8_rows(_ptr(w8), _ptr(scales), _ptr(w.contiguous()),
                           N, K, _stream())
    return w8, scales


def _gemv_fp8_ok(M: int, K: int) -> bool:
    # k_gemv_*_fp8 are instantiated for M in {1,2,4,8} and stream 16 codes
    # per load (nv = K >> 4): a K % 16 tail would be dropped
    return M in (1, 2, 4, 8) and K % 16 == 0


def _linear_fp8(x: torch.Tensor, w8: torch.Tensor,
                wscale: torch.Tensor) -> torch.Tensor:
    """x [..., K] @ dequant(w8, wscale)^T in f32, like the kernels: the dot
    runs over the exact e4m3 values and the f32 row scale multiplies the
    sum (rounding code*scale to bf16 first would cost 2^-9 per weight)."""
    codes = w8.view(torch.float8_e4m3fn).float()
    return torch.nn.functional.linear(x.float(), codes) * wscale.float()


def gemv_norm_fp8(res, wnorm, w8, wscale, eps: float = 1e-5,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    M = res.numel() // res.shape[-1]
    K = res.shape[-1]
    N = w8.shape[0]
    if not res.is_cuda or not _gemv_fp8_ok(M, K):
        return _linear_fp8(rmsnorm(res, wnorm, eps), w8, wscale).to(res.dtype)
    assert M * K * 2 <= 64 * 1024, \
        "fp8 norm-GEMV stages M*K bf16 activations in LDS (<=64 KB)"
    lib = require_lib()
    r2 = res.contiguous().view(M, K)
    if out is None:
        out = torch.empty(*res.shape[:-1], N, dtype=res.dtype, device=res.device)
    lib.fei_gemv_norm_fp8(_ptr(out), _ptr(r2), _ptr(wnorm), _ptr(w8),
                          _ptr(wscale), M, N, K, eps, _stream())
    return out


def gemv_res_fp8(x, w8, wscale, res) -> torch.Tensor:
    M = x.numel() // x.shape[-1]
    K = x.shape[-1]
    N = w8.shape[0]
    if not x.is_cuda or not _gemv_fp8_ok(M, K):
        lin = _linear_fp8(x, w8, wscale)
        res.copy_((res.float() + lin.view_as(res)).to(res.dtype))
        return res
    lib = require_lib()
    x2 = x.contiguous().view(M, K)
    lib.fei_gemv_res_fp8(_ptr(res), _ptr(x2), _ptr(w8), _ptr(wscale),
                         M, N, K, _stream())
    return res


def gemv_swiglu_norm_fp8(res, wnorm, w8, wscale, eps: float = 1e-5,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    M = res.numel() // res.shape[-1]
    K = res.shape[-1]
    I = w8.shape[0] // 2
    if not res.is_cuda or not _gemv_fp8_ok(M, K):
        # g/u stay f32 through silu, as in the kernel
        gu = _linear_fp8(rmsnorm(res, wnorm, eps), w8, wscale)
        return ref.swiglu(gu).to(res.dtype)
    assert M * K * 2 <= 64 * 1024
    lib = require_lib()
    r2 = res.contiguous().view(M, K)
    if out is None:
        out = torch.empty(*res.shape[:-1], I, dtype=res.dtype, device=res.device)
    lib.fei_gemv_swiglu_norm_fp8(_ptr(out), _ptr(r2), _ptr(wnorm), _ptr(w8),
                                 _ptr(wscale), M, I, K, eps, _stream())
    return out


# -- fused score + top-k over an embedding corpus (csrc/score_topk.hip) ------

SCORE_TOPK_MAX_K = 64
SCORE_TOPK_MAX_Q = 8
SCORE_TOPK_MAX_C = 2048
SCORE_TOPK_MAX_WG = 65536
# Corpus bytes past which the scan loads nontemporal: a corpus that fits the
# 256 MiB L3 is worth keeping there between queries, a larger one only
# evicts everything else (k_gemv's rule, with the threshold this op needs
# because a corpus, unlike a decode step's weights, can be small).
_SCORE_TOPK_NT_MIN_BYTES = int(os.environ.get("FEI_SCORE_TOPK_NT_MIN",
                                              256 << 20))
# Scan workgroups per CU: 4 up to four queries, 2 beyond (at Q = 8 the
# per-wave top-k warm-up and the 226-register instance favour fewer, longer
# slabs: 1.15 vs 1.33 ms at 1M x 768; profiles/score_topk.md).
_SCORE_TOPK_WG_PER_CU = 4
_SCORE_TOPK_WG_PER_CU_WIDE = 2


def _score_topk_check(emb, q, k, mask, workgroups) -> Tuple[int, int, int]:
    """Argument checks of score_topk, the same on CPU and GPU; returns
    (N, C, Q) with q seen as [Q, C]."""
    name = "score_topk"
    if not isinstance(emb, torch.Tensor) or emb.dim() != 2:
        raise ValueError(f"{name}: emb must be a [N, C] tensor")
    if emb.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"{name}: emb must be float32 or float16, got "
                         f"{emb.dtype}")
    N, C = emb.shape
    if not isinstance(q, torch.Tensor) or q.dim() not in (1, 2):
        raise ValueError(f"{name}: q must be a [C] or [Q, C] tensor")
    if q.dtype != torch.float32:
        raise ValueError(f"{name}: q must be float32, got {q.dtype}")
    Q = 1 if q.dim() == 1 else q.shape[0]
    if q.shape[-1] != C:
        raise ValueError(f"{name}: q has {q.shape[-1]} columns, emb has {C}")
    if q.device != emb.device:
        raise ValueError(f"{name}: q lives on {q.device}, emb on "
                         f"{emb.device}")
    if isinstance(k, bool) or not isinstance(k, int) \
            or not 1 <= k <= SCORE_TOPK_MAX_K:
        raise ValueError(f"{name}: k must be an int in 1.."
                         f"{SCORE_TOPK_MAX_K}, got {k!r}")
    if not 1 <= Q <= SCORE_TOPK_MAX_Q:
        raise ValueError(f"{name}: 1..{SCORE_TOPK_MAX_Q} queries per call, "
                         f"got {Q}")
    if C < 8 or C % 8 != 0 or C > SCORE_TOPK_MAX_C:
        raise ValueError(f"{name}: C must be a multiple of 8 in 8.."
                         f"{SCORE_TOPK_MAX_C}, got {C}")
    if not 1 <= N < 2 ** 31:
        raise ValueError(f"{name}: N must be in 1..2^31-1, got {N}")
    if not emb.is_contiguous():
        raise ValueError(f"{name}: emb must be contiguous (row stride C)")
    if not q.is_contiguous():
        raise ValueError(f"{name}: q must be contiguous")
    if emb.data_ptr() % 16 or q.data_ptr() % 16:
        raise ValueError(f"{name}: emb and q must be 16-byte aligned")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8:
            raise ValueError(f"{name}: mask must be a uint8 tensor")
        if tuple(mask.shape) != (N,):
            raise ValueError(f"{name}: mask must have shape ({N},), got "
                             f"{tuple(mask.shape)}")
        if mask.device != emb.device:
            raise ValueError(f"{name}: mask lives on {mask.device}, emb on "
                             f"{emb.device}")
        if not mask.is_contiguous():
            raise ValueError(f"{name}: mask must be contiguous")
    if workgroups is not None:
        if isinstance(workgroups, bool) or not isinstance(workgroups, int) \
                or not 1 <= workgroups <= SCORE_TOPK_MAX_WG:
            raise ValueError(f"{name}: workgroups must be an int in 1.."
                             f"{SCORE_TOPK_MAX_WG}, got {workgroups!r}")
    return N, C, Q


def score_topk(emb: torch.Tensor, q: torch.Tensor, k: int,
               mask: Optional[torch.Tensor] = None, *,
               workgroups: Optional[int] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k best rows of emb [N, C] (f32 or f16) for each query of q [Q, C]
    (f32, Q <= 8) by dot product: (scores f32 [Q, k], rows int32 [Q, k]),
    sorted by (score descending, row ascending). q may be [C]; the result is
    then [k]. ``mask``: uint8 [N], non-zero = eligible; ineligible rows are
    skipped inside the scan, not filtered afterwards, and are never read.
    With fewer than k eligible rows the tail is (-inf, -1).

    GPU: one pass of k_score_topk_partial over the corpus plus
    k_score_topk_final (csrc/score_topk.hip); the score vector is never
    materialised. ``workgroups`` overrides the scan's grid (tests: the
    result does not depend on it); the default is a few workgroups per CU,
    clamped so each has rows. CPU: reference.score_topk. Shapes, dtypes,
    limits (k <= 64, C % 8 == 0, C <= 2048), contiguity and alignment are
    checked first: ValueError, nothing launched."""
    N, C, Q = _score_topk_check(emb, q, k, mask, workgroups)
    q2 = q.view(Q, C)
    if not emb.is_cuda:
        s, i = ref.score_topk(emb, q2, k, mask)
    else:
        lib = require_lib()
        if workgroups is None:
            per_cu = _SCORE_TOPK_WG_PER_CU if Q <= 4 \
                else _SCORE_TOPK_WG_PER_CU_WIDE
            workgroups = per_cu * _cu_count(emb.device)
        WG = max(1, min(workgroups, N))
        dev = emb.device
        part_s = torch.empty(Q, WG, k, dtype=torch.float32, device=dev)
        part_i = torch.empty(Q, WG, k, dtype=torch.int32, device=dev)
        s = torch.empty(Q, k, dtype=torch.float32, device=dev)
        i = torch.empty(Q, k, dtype=torch.int32, device=dev)
        nt = 1 if N * C * emb.element_size() > _SCORE_TOPK_NT_MIN_BYTES else 0
        rc = lib.fei_score_topk(
            _ptr(emb), _ptr(q2), _ptr(mask) if mask is not None else None,
            _ptr(part_s), _ptr(part_i), _ptr(s), _ptr(i), N, C, Q, k, WG,
            1 if emb.dtype == torch.float16 else 0, nt, _stream())
        if rc != 0:
            raise ValueError(f"score_topk: the kernel refused N={N} C={C} "
                             f"Q={Q} k={k} workgroups={WG} (code {rc})")
    if q.dim() == 1:
        return s[0], i[0]
    return s, i
