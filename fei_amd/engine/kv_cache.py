"""Paged KV-cache allocator.

Sized for MI355X's 288 GB HBM3E: the pool reserves a fraction of free GPU
memory as fixed-size blocks; sequences map logical block indices to physical
blocks so many agent sessions can share one engine without fragmentation.
The flagship single-conversation path uses contiguous per-sequence caches
([B,Hkv,max_seq,D]); the paged serving path (engine/sessions.py) keeps every
session's KV in blocks of this pool and reads and writes them through a block
table with the HIP kernels k_attn_decode_paged (decode, fused RoPE + append),
k_rope_kv_prefill_paged and k_attn_prefill_paged (prefill and multi-turn
continuation). The allocator is host-side bookkeeping only: blocks are
handed out, grown (ensure_capacity), given back (truncate, release) and
copied (fork); it never moves a row.

``kv_quant="fp8"`` stores the rows in the fp8 format of
reference.quant_kv_fp8: every layer is an ops.QuantKV (e4m3fn codes
[num_blocks, Hkv, BS, D] + one f32 scale per row [num_blocks, Hkv, BS]) and
the kernels are their fp8 forms in csrc/kv_fp8_paged.hip
(k_attn_decode_paged_kv8, k_rope_kv8_prefill_paged,
k_attn_prefill_paged_kv8). A row costs D + 4 bytes instead of 2*D, so the
same memory budget holds 2*D / (D + 4) times the blocks (1.94x at D = 128).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

from fei_amd import ops
from fei_amd.utils.logging import get_logger

logger = get_logger("engine.kv_cache")


@dataclass
class BlockTable:
    """Logical -> physical block mapping for one sequence."""
    seq_id: int
    blocks: List[int] = field(default_factory=list)
    length: int = 0                       # tokens used


class PagedKVPool:
    """Fixed-size block pool over one big tensor pair per layer.

    layout per layer: [num_blocks, Hkv, block_size, D] — a sequence's
    logical block i lives at physical index table.blocks[i]. With
    ``kv_quant="fp8"`` a layer is an ops.QuantKV of that shape (codes) plus
    [num_blocks, Hkv, block_size] f32 scales; ``dtype`` is then unused.
    """

    def __init__(
        self,
        num_layers: int,
        num_kv_heads: int,
        head_dim: int,
        block_size: int = 16,
        num_blocks: Optional[int] = None,
        device: Optional[torch.device] = None,
        dtype: torch.dtype = torch.bfloat16,
        mem_fraction: float = 0.6,
        kv_quant: Optional[str] = None,
    ):
        if kv_quant not in (None, "fp8"):
            raise ValueError(
                f"kv_quant must be None or 'fp8', got {kv_quant!r}")
        self.kv_quant = kv_quant
        self.block_size = block_size
        self.device = device or (torch.device("cuda:0") if torch.cuda.is_available()
                                 else torch.device("cpu"))
        self.dtype = dtype
        if num_blocks is None:
            if self.device.type == "cuda":
                free, _total = torch.cuda.mem_get_info(self.device)
                budget = int(free * mem_fraction)
            else:
                budget = 1 << 28
            # bytes of one row: D elements, or D codes + one f32 scale
            row_bytes = (head_dim + 4 if kv_quant == "fp8" else
                         head_dim * torch.tensor([], dtype=dtype).element_size())
            bytes_per_block = (2 * num_layers * num_kv_heads * block_size *
                               row_bytes)
            num_blocks = max(16, budget // bytes_per_block)
        self.num_blocks = int(num_blocks)
        shape = (self.num_blocks, num_kv_heads, block_size, head_dim)
        if kv_quant == "fp8":
            self.k = [ops.QuantKV.zeros(shape, self.device)
                      for _ in range(num_layers)]
            self.v = [ops.QuantKV.zeros(shape, self.device)
                      for _ in range(num_layers)]
        else:
            self.k = [torch.zeros(shape, device=self.device, dtype=dtype)
                      for _ in range(num_layers)]
            self.v = [torch.zeros(shape, device=self.device, dtype=dtype)
                      for _ in range(num_layers)]
        self._free: List[int] = list(range(self.num_blocks - 1, -1, -1))
        self._tables: Dict[int, BlockTable] = {}
        self._next_id = 0

    @property
    def kv_dtype(self) -> str:
        """Element format of the pool's rows: "fp8", "bf16" or "fp32"."""
        if self.kv_quant == "fp8":
            return "fp8"
        return "bf16" if self.dtype == torch.bfloat16 else "fp32"

    # -- sessions ------------------------------------------------------------

    def free_blocks(self) -> int:
        return len(self._free)

    def new_sequence(self) -> int:
        sid = self._next_id
        self._next_id += 1
        self._tables[sid] = BlockTable(seq_id=sid)
        return sid

    def table(self, seq_id: int) -> BlockTable:
        return self._tables[seq_id]

    def ensure_capacity(self, seq_id: int, n_tokens: int) -> List[int]:
        """Grow a sequence to hold n_tokens; returns its block list."""
        t = self._tables[seq_id]
        need = (n_tokens + self.block_size - 1) // self.block_size
        while len(t.blocks) < need:
            if not self._free:
                raise MemoryError(
                    f"KV pool exhausted ({self.num_blocks} blocks); free a "
                    "sequence first")
            t.blocks.append(self._free.pop())
        t.length = max(t.length, n_tokens)
        return t.blocks

    def truncate(self, seq_id: int, n_tokens: int) -> List[int]:
        """Shrink a sequence to n_tokens: the blocks beyond
        ceil(n_tokens / block_size) go back to the free list — in the
        reverse of the order ensure_capacity took them, so undoing a growth
        leaves the free list as it was — and ``length`` becomes n_tokens.
        Returns the remaining block list."""
        if n_tokens < 0:
            raise ValueError(f"n_tokens must be >= 0, got {n_tokens}")
        t = self._tables[seq_id]
        keep = (n_tokens + self.block_size - 1) // self.block_size
        if keep > len(t.blocks):
            raise ValueError(
                f"truncate cannot grow a sequence ({len(t.blocks)} blocks "
                f"held, {keep} asked); use ensure_capacity")
        freed = t.blocks[keep:]
        del t.blocks[keep:]
        self._free.extend(reversed(freed))
        t.length = n_tokens
        return t.blocks

    def release(self, seq_id: int) -> None:
        t = self._tables.pop(seq_id, None)
        if t:
            self._free.extend(t.blocks)

    def fork(self, seq_id: int) -> int:
        """Copy-on-write-free fork is not supported (blocks are mutable);
        makes a physical copy of the parent's blocks (codes and scales in
        an fp8 pool)."""
        parent = self._tables[seq_id]
        child_id = self.new_sequence()
        child = self._tables[child_id]
        for pb in parent.blocks:
            if not self._free:
                raise MemoryError("KV pool exhausted during fork")
            nb = self._free.pop()
            for layer in self.k + self.v:
                parts = ((layer.data, layer.scale)
                         if isinstance(layer, ops.QuantKV) else (layer,))
                for t in parts:
                    t[nb].copy_(t[pb])
            child.blocks.append(nb)
        child.length = parent.length
        return child_id

    def block_table_tensor(self, seq_id: int) -> torch.Tensor:
        return torch.tensor(self._tables[seq_id].blocks, dtype=torch.int32,
                            device=self.device)
