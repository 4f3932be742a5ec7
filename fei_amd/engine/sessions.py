"""Paged multi-session serving: continuous batching over a PagedKVPool.

The reference serves one remote conversation per Assistant; this engine
serves MANY resident agent sessions on one GPU: each session's KV lives in
16-token blocks of a shared pool (`engine/kv_cache.py`), sessions join and
leave the decode batch at any step, and the attention read path is the HIP
block-table kernel (`k_attn_decode_paged`). Admission is explicit — a
session that cannot get blocks raises and the caller can evict.

Prompts are prefilled straight into the session's blocks
(`LlamaModel.forward_prefill_paged`: `k_rope_kv_prefill_paged` +
`k_attn_prefill_paged`), and a finished session can be continued with new
prompt tokens (`extend`: a tool result, the next user message) without
re-prefilling the conversation: open -> step -> result -> extend -> step ...
Several admissions at once (agents that start together, tool results that
come back together) share packed ragged forwards instead of paying one
forward each: `open_many` / `extend_many` over
`LlamaModel.forward_prefill_paged_ragged` (`k_rope_kv_prefill_paged_ragged`
+ `k_attn_prefill_paged_ragged`), all or nothing on pool exhaustion.

The pool follows the engine's KV format: on an engine built with
``kv_quant="fp8"`` (or with an explicit ``kv_quant="fp8"`` here) the sessions
live in fp8 blocks (e4m3fn codes + one f32 scale per row, ops.QuantKV pool
layers) and every read and write goes through the fp8 paged kernels
(csrc/kv_fp8_paged.hip) — 2*D / (D + 4) times the blocks for the same
``mem_fraction``.

Control-plane costs stay host-side (per-step RoPE/append scatter is a few
microseconds of torch indexing per layer); the O(context) work — attention
over the pool — is the paged HIP kernel, and all GEMVs take the same
streaming kernels as the single-session path. Graphs are off by default
(batch membership changes).

Every session carries its own sampling parameters (temperature, top_k,
top_p, seed) and its own count of tokens drawn (``Session.sampled``). A
batch whose sessions are all at temperature 0 decodes greedily with
``argmax``, exactly as before sampling existed; otherwise all rows go
through ``ops.sample_rows`` (`k_sample_filtered_rows`), which reads every
parameter per row and whose noise depends only on the session's own (seed,
sampled) — so a session's tokens do not depend on who else is in the batch
or on its row index, sampled or not.
"""

from __future__ import annotations

import logging
import math
import os as _os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Union

logger = logging.getLogger(__name__)

import torch
import torch.nn.functional as F

from fei_amd import ops
from fei_amd.engine.kv_cache import PagedKVPool
from fei_amd.ops import reference as ref


@dataclass
class Session:
    sid: int
    prompt_ids: List[int]
    generated: List[int] = field(default_factory=list)
    pos: int = 0                     # current context length in the pool
    max_new_tokens: int = 256
    done: bool = False
    turn: int = 0                    # 0 = the turn open() started
    # everything in front of the current turn's tokens: prompt_ids, then for
    # every finished turn its emitted tokens (EOS included) and the
    # extension that followed
    context_ids: List[int] = field(default_factory=list)
    # sampling parameters (ops.sample_filtered semantics; temperature 0 is
    # greedy) and the number of tokens drawn so far over ALL turns: the
    # sampler's `step` for the next draw. Monotone, so noise is never reused
    # across turns; turn 0 numbers its draws like engine.generate().
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0
    sampled: int = 0


class _Draw(NamedTuple):
    """One row's sampling parameters and step, as the sampler reads them."""
    temperature: float
    top_k: int
    top_p: float
    seed: int
    step: int


_GREEDY = _Draw(0.0, 0, 1.0, 0, 0)


def _check_sampling(temperature, top_k, top_p, seed) -> None:
    """ValueError unless the values are ones the sampler accepts."""
    if isinstance(temperature, bool) or \
            not isinstance(temperature, (int, float)) or \
            not (0.0 <= temperature < float("inf")):
        raise ValueError(f"temperature must be a number >= 0, got "
                         f"{temperature!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or \
            not 0 <= top_k < 2 ** 31:
        raise ValueError(f"top_k must be an int >= 0, got {top_k!r}")
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or \
            not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or \
            not 0 <= seed < 2 ** 63:
        raise ValueError(f"seed must be an int in [0, 2^63), got {seed!r}")


def _per_item(value, n: int, name: str) -> list:
    """A scalar applied to all n items, or one entry per item."""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{name}: {len(value)} entries for {n} items")
        return list(value)
    return [value] * n


class PagedSessionManager:
    def __init__(self, engine, block_size: int = 16,
                 num_blocks: Optional[int] = None,
                 mem_fraction: float = 0.25,
                 kv_quant: Optional[str] = None):
        """``kv_quant``: None inherits ``engine.kv_quant``; "fp8" asks for an
        fp8 pool; "none" for an unquantised pool whatever the engine uses."""
        self.engine = engine
        self.model = engine.model
        m = self.model
        assert m.tp_size == 1, "paged session serving is single-GPU"

        if kv_quant is None:
            kv_quant = getattr(engine, "kv_quant", None)
        elif kv_quant == "none":
            kv_quant = None
        self.pool = PagedKVPool(
            num_layers=m.spec.num_layers, num_kv_heads=m.hkv_l,
            head_dim=m.D, block_size=block_size, num_blocks=num_blocks,
            device=m.device, dtype=m.dtype, mem_fraction=mem_fraction,
            kv_quant=kv_quant)
        self.sessions: Dict[int, Session] = {}
        self.eos = engine.tokenizer.eos_id
        self._ws: Dict[int, tuple] = {}     # split-K workspace per batch size
        self._serial_logged = False         # fp8 batched-admission notice
        # hipGraph per (B, table_width): one captured decode step (forward
        # + argmax feedback + pos advance) over static buffers. Measured
        # NEUTRAL (836 vs 869 tok/s eager at 8 sessions): the eager chunk
        # loop already queues launches ahead of the GPU, so the step is
        # GPU-time-bound, not host-bound. Opt-in via FEI_SESS_GRAPH=1.
        self._graphs: Dict[tuple, dict] = {}
        self.use_graph = m.device.type == "cuda" and \
            _os.environ.get("FEI_SESS_GRAPH", "0") == "1"
        # True once any session has asked for temperature > 0: from then on
        # captured steps contain the per-row sampler (greedy rows ride along
        # at temperature 0). An all-greedy manager never sets it.
        self._seen_sampled = False

    # -- token selection -------------------------------------------------------

    def _draw_bufs(self, draws: List[_Draw]) -> dict:
        """The per-row sampler's device state for ``draws``."""
        dev, B = self.model.device, len(draws)
        return {
            "top_k": torch.tensor([d.top_k for d in draws],
                                  dtype=torch.int32, device=dev),
            "top_p": torch.tensor([d.top_p for d in draws],
                                  dtype=torch.float32, device=dev),
            "temperature": torch.tensor([d.temperature for d in draws],
                                        dtype=torch.float32, device=dev),
            "seed": torch.tensor([d.seed for d in draws],
                                 dtype=torch.int64, device=dev),
            "step": torch.tensor([d.step for d in draws],
                                 dtype=torch.int32, device=dev),
            "token": torch.zeros(B, dtype=torch.int32, device=dev),
            "info": torch.zeros(B, 2, dtype=torch.float32, device=dev),
        }

    @staticmethod
    def _sample_rows(logits: torch.Tensor, bufs: dict) -> torch.Tensor:
        """One ops.sample_rows draw per logits row into bufs["token"] (which
        is returned); bufs["step"] is left for the caller to advance."""
        return ops.sample_rows(
            logits.contiguous(), bufs["token"], bufs["step"], bufs["info"],
            top_k=bufs["top_k"], top_p=bufs["top_p"],
            temperature=bufs["temperature"], seed=bufs["seed"])

    def _select(self, logits: torch.Tensor, draws: List[_Draw]
                ) -> torch.Tensor:
        """Next token of every logits row ([B] on the device), row i drawn
        with draws[i]. All rows greedy: the argmax this manager has always
        run. Otherwise one per-row sampler launch over all rows."""
        if all(d.temperature == 0 for d in draws):
            return logits.argmax(dim=-1)
        self._seen_sampled = True
        return self._sample_rows(logits, self._draw_bufs(draws))

    def _splits(self, B: int) -> int:
        # batch-aware split count (engine ctor note): the B-wide grid
        # already fills the chip at 16 splits once B >= 4 — 32 over-splits
        # (batch-8 plain path measured 6.34 -> 5.85 ms/step at 16)
        sp = min(self.engine.attn_splits, 16) if B >= 4 \
            else self.engine.attn_splits
        if self.pool.kv_quant == "fp8":
            sp = min(sp, self.model.D // 2)     # the fp8 kernel's own limit
        return sp

    def _workspace(self, B: int):
        if B not in self._ws:
            m = self.model
            sp = self._splits(B)
            self._ws[B] = (
                torch.zeros(B, m.hq_l, sp, m.D, dtype=torch.float32,
                            device=m.device),
                torch.zeros(B, m.hq_l, sp, 2, dtype=torch.float32,
                            device=m.device))
        return self._ws[B]

    def _chunk_graph(self, B: int, max_blocks: int, token, pos, table,
                     draws: Optional[List[_Draw]] = None):
        """Capture (or fetch) the hipGraph of ONE decode step for batch B
        and a table of width >= max_blocks: forward + in-place argmax
        token feedback + pos advance over static buffers. With ``draws``
        (the manager has seen a sampled session) the token comes from the
        per-row sampler instead, whose parameter and step tensors are static
        buffers of the entry too (the capture then also advances step); the
        two kinds of step are captured under different keys. Warm-up runs 2
        real steps whose KV rows are garbage; they are rewritten by the
        first replays before anything attends them (the per-layer append
        at `pos` precedes the attention read of key `pos`, and rows past
        the accepted stream are never attended). In an fp8 pool the same
        holds for a row's scale as for its codes: the append writes both
        before the row is read."""
        W = 16
        while W < max_blocks:
            W *= 2
        key = (B, W, draws is not None)
        ent = self._graphs.get(key)
        if ent is not None:
            return ent
        dev = self.model.device
        bt = torch.zeros(B, W, dtype=torch.int32, device=dev)
        tk = torch.zeros(B, dtype=torch.int64, device=dev)
        ps = torch.zeros(B, dtype=torch.int32, device=dev)
        bt[:, :max_blocks].copy_(table)
        tk.copy_(token)
        ps.copy_(pos)
        bufs = self._draw_bufs(draws) if draws is not None else None

        def one_step():
            lg = self._forward_paged(tk, ps, bt)
            if bufs is None:
                tk.copy_(lg.argmax(dim=-1))
            else:
                tk.copy_(self._sample_rows(lg, bufs))
                bufs["step"].add_(1)
            ps.add_(1)

        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    one_step()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                one_step()
            torch.cuda.synchronize()
        except Exception as e:                      # pragma: no cover - GPU
            logger.warning("sessions graph capture failed (%s); "
                           "falling back to eager chunks", e)
            self.use_graph = False
            return None
        ent = {"graph": g, "token": tk, "pos": ps, "table": bt,
               "draw": bufs}
        self._graphs[key] = ent
        logger.info("sessions decode step captured (B=%d, W=%d, %s)", B, W,
                    "greedy" if bufs is None else "per-row sampler")
        return ent

    # -- admission -----------------------------------------------------------

    def open(self, prompt: Union[str, List[int]],
             max_new_tokens: int = 256, temperature: float = 0.0,
             top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> int:
        """Prefill a new session into the pool; returns its id. The session
        draws its tokens with (temperature, top_k, top_p, seed) —
        ops.sample_filtered semantics, temperature 0 is greedy. Raises
        ValueError for parameters the sampler does not accept (nothing is
        reserved) and MemoryError when the pool has no blocks (caller
        evicts/queues)."""
        _check_sampling(temperature, top_k, top_p, seed)
        ids = (self.engine.tokenizer.encode(prompt)
               if isinstance(prompt, str) else list(prompt))
        S = len(ids)
        sid = self.pool.new_sequence()
        try:
            self.pool.ensure_capacity(sid, S + 1)
        except MemoryError:
            self.pool.release(sid)
            raise
        logits = self._prefill_paged(sid, ids, 0)
        draw = _Draw(float(temperature), top_k, float(top_p), seed, 0)
        first = self._first_token(logits, draw)
        sess = Session(sid=sid, prompt_ids=ids, generated=[first], pos=S,
                       max_new_tokens=max_new_tokens, context_ids=list(ids),
                       temperature=draw.temperature, top_k=top_k,
                       top_p=draw.top_p, seed=seed, sampled=1)
        if first == self.eos:
            sess.done = True
        self.sessions[sid] = sess
        return sid

    def _first_token(self, logits: torch.Tensor, draw: _Draw) -> int:
        """The first token of a turn from its prefill logits [1, vocab]."""
        if draw.temperature == 0:
            return int(logits[0].argmax())
        return int(self._select(logits[:1], [draw])[0])

    def _resolve(self, s: Session, temperature, top_k, top_p, seed) -> _Draw:
        """extend()'s sampling arguments (None keeps the session's value),
        validated, with the session's next step."""
        d = _Draw(s.temperature if temperature is None else temperature,
                  s.top_k if top_k is None else top_k,
                  s.top_p if top_p is None else top_p,
                  s.seed if seed is None else seed, s.sampled)
        _check_sampling(d.temperature, d.top_k, d.top_p, d.seed)
        return d._replace(temperature=float(d.temperature),
                          top_p=float(d.top_p))

    @staticmethod
    def _start_turn(s: Session, draw: _Draw) -> None:
        s.temperature, s.top_k = draw.temperature, draw.top_k
        s.top_p, s.seed = draw.top_p, draw.seed
        s.sampled += 1                      # the turn's first token

    def _prefill_paged(self, sid: int, ids: List[int],
                       pos0: int) -> torch.Tensor:
        """Prefill ``ids`` at rows [pos0, pos0 + len(ids)) of session sid's
        blocks (already reserved), in slices of LocalEngine.PREFILL_CHUNK;
        returns the last position's logits [1, vocab]."""
        m, dev = self.model, self.model.device
        table = torch.tensor([self.pool.table(sid).blocks],
                             dtype=torch.int32, device=dev)
        chunk = self.engine.PREFILL_CHUNK
        logits = None
        for j in range(0, len(ids), chunk):
            tokens = torch.tensor([ids[j:j + chunk]], dtype=torch.int64,
                                  device=dev)
            p0 = torch.full((1,), pos0 + j, dtype=torch.int32, device=dev)
            logits = m.forward_prefill_paged(tokens, p0, self.pool.k,
                                             self.pool.v, table)
        return logits

    def extend(self, sid: int, prompt: Union[str, List[int]],
               max_new_tokens: int = 256, temperature: Optional[float] = None,
               top_k: Optional[int] = None, top_p: Optional[float] = None,
               seed: Optional[int] = None) -> int:
        """Continue a FINISHED session with new prompt tokens (a tool
        result, the next user message); returns the first token of the new
        turn. The conversation so far is not prefilled again. A sampling
        parameter left at None keeps the session's value; the session's
        draw count carries on, so a turn never reuses an earlier turn's
        noise.

        The pool holds KV rows for prompt + generated[:-1] and ``pos``
        counts them: the last emitted token has no row yet. So the prefill
        is [generated[-1]] + new tokens at pos0 = pos. A turn that ended at
        an EOS inside a step_chunk left garbage rows past ``pos``; they are
        never attended: this prefill writes rows pos .. pos + len(new)
        before it reads them, attention is causal, and every later decode
        step writes row p before it attends [0, p].

        Raises KeyError (unknown session), ValueError (the session is still
        active, a sampling parameter is out of range, or pos + 1 + len(new)
        + max_new_tokens exceeds the model's max_seq_len) and MemoryError
        (no blocks); after any of them the session, its block list and the
        free list are exactly as they were."""
        s = self.sessions[sid]                      # KeyError: unknown
        if not s.done:
            raise ValueError(f"session {sid} is still active")
        draw = self._resolve(s, temperature, top_k, top_p, seed)
        new_ids = (self.engine.tokenizer.encode(prompt)
                   if isinstance(prompt, str) else list(prompt))
        n = 1 + len(new_ids)
        if s.pos + n + max_new_tokens > self.model.max_seq_len:
            raise ValueError(
                f"session {sid}: context {s.pos} + {n} new + "
                f"{max_new_tokens} to generate exceeds max_seq_len "
                f"{self.model.max_seq_len}")
        t = self.pool.table(sid)
        held, length = len(t.blocks), t.length
        try:
            self.pool.ensure_capacity(sid, s.pos + n + 1)
        except MemoryError:
            self.pool.truncate(sid, held * self.pool.block_size)
            t.length = length
            raise
        logits = self._prefill_paged(sid, [s.generated[-1]] + new_ids, s.pos)
        first = self._first_token(logits, draw)
        s.context_ids = s.context_ids + self._emitted(s) + new_ids
        s.pos += n
        s.generated = [first]
        s.max_new_tokens = max_new_tokens
        s.turn += 1
        self._start_turn(s, draw)
        s.done = first == self.eos
        return first

    # -- batched admission ----------------------------------------------------

    def _ids(self, prompt: Union[str, List[int]]) -> List[int]:
        return (self.engine.tokenizer.encode(prompt)
                if isinstance(prompt, str) else list(prompt))

    def _ragged_admission(self) -> bool:
        """False for an fp8 pool on the GPU: there is no fp8 ragged kernel,
        so open_many / extend_many admit one session per forward there."""
        if self.pool.kv_quant == "fp8" and self.model.device.type == "cuda":
            if not self._serial_logged:
                logger.info("fp8 KV pool: batched admission runs one "
                            "session per forward (no fp8 ragged prefill "
                            "kernel)")
                self._serial_logged = True
            return False
        return True

    def open_many(self, prompts, max_new_tokens: int = 256,
                  max_batch_tokens: Optional[int] = None,
                  temperature=0.0, top_k=0, top_p=1.0, seed=0) -> List[int]:
        """open() for several prompts at once; returns their session ids in
        order. The prompts share packed ragged prefill forwards
        (LlamaModel.forward_prefill_paged_ragged) instead of paying one
        forward each; see _prefill_many for the schedule. Every session ends
        up exactly as open() would leave it. Each sampling parameter is a
        scalar for all prompts or a list with one entry per prompt; a bad
        value or list length raises ValueError before anything is reserved.

        All or nothing: blocks for every prompt are reserved first, and when
        the pool runs out MemoryError is raised with the sessions, every
        block list and the free list exactly as before the call."""
        all_ids = [self._ids(p) for p in prompts]
        if any(not ids for ids in all_ids):
            raise ValueError("open_many: empty prompt")
        n = len(all_ids)
        draws = []
        for t, k, p, sd in zip(_per_item(temperature, n, "temperature"),
                               _per_item(top_k, n, "top_k"),
                               _per_item(top_p, n, "top_p"),
                               _per_item(seed, n, "seed")):
            _check_sampling(t, k, p, sd)
            draws.append(_Draw(float(t), k, float(p), sd, 0))
        if not all_ids:
            return []
        sids: List[int] = []

        def rollback():
            for sid in reversed(sids):
                self.pool.truncate(sid, 0)      # undoes the take order
                self.pool.release(sid)

        try:
            for ids in all_ids:
                sids.append(self.pool.new_sequence())
                self.pool.ensure_capacity(sids[-1], len(ids) + 1)
        except MemoryError:
            rollback()
            raise
        if not self._ragged_admission():
            rollback()                          # open() takes the same blocks
            return [self.open(ids, max_new_tokens, d.temperature, d.top_k,
                              d.top_p, d.seed)
                    for ids, d in zip(all_ids, draws)]
        firsts = self._prefill_many(
            [(sid, ids, 0) for sid, ids in zip(sids, all_ids)],
            max_batch_tokens, draws)
        for sid, ids, first, d in zip(sids, all_ids, firsts, draws):
            self.sessions[sid] = Session(
                sid=sid, prompt_ids=ids, generated=[first], pos=len(ids),
                max_new_tokens=max_new_tokens, done=first == self.eos,
                context_ids=list(ids), temperature=d.temperature,
                top_k=d.top_k, top_p=d.top_p, seed=d.seed, sampled=1)
        return sids

    def extend_many(self, items, max_new_tokens: int = 256,
                    max_batch_tokens: Optional[int] = None,
                    temperature=None, top_k=None, top_p=None,
                    seed=None) -> List[int]:
        """extend() for several finished sessions at once: ``items`` are
        (sid, prompt) pairs; returns the first token of every new turn, in
        order. The extensions share packed ragged prefill forwards. Each
        sampling parameter is None (every session keeps its value), a scalar
        for all items, or a list with one entry (a value or None) per item.

        Everything is validated before anything is touched, with extend()'s
        errors (KeyError unknown session; ValueError still active, a sampling
        parameter out of range or a list of the wrong length, or the
        context would exceed max_seq_len) and ValueError for a session that
        appears twice. Then all or nothing: MemoryError leaves every session,
        block list, length and the free list exactly as before the call."""
        items = list(items)
        n_items = len(items)
        per = list(zip(_per_item(temperature, n_items, "temperature"),
                       _per_item(top_k, n_items, "top_k"),
                       _per_item(top_p, n_items, "top_p"),
                       _per_item(seed, n_items, "seed")))
        todo = []
        draws = []
        seen = set()
        for (sid, prompt), given in zip(items, per):
            s = self.sessions[sid]                  # KeyError: unknown
            if sid in seen:
                raise ValueError(f"session {sid} appears twice")
            seen.add(sid)
            if not s.done:
                raise ValueError(f"session {sid} is still active")
            new_ids = self._ids(prompt)
            n = 1 + len(new_ids)
            if s.pos + n + max_new_tokens > self.model.max_seq_len:
                raise ValueError(
                    f"session {sid}: context {s.pos} + {n} new + "
                    f"{max_new_tokens} to generate exceeds max_seq_len "
                    f"{self.model.max_seq_len}")
            draws.append(self._resolve(s, *given))
            todo.append((s, new_ids))
        if not todo:
            return []
        grown = []                                  # (sid, blocks held, length)

        def rollback():
            for sid, held, length in reversed(grown):
                self.pool.truncate(sid, held * self.pool.block_size)
                self.pool.table(sid).length = length

        try:
            for s, new_ids in todo:
                t = self.pool.table(s.sid)
                grown.append((s.sid, len(t.blocks), t.length))
                self.pool.ensure_capacity(s.sid, s.pos + 1 + len(new_ids) + 1)
        except MemoryError:
            rollback()
            raise
        if not self._ragged_admission():
            rollback()                              # extend() grows them again
            return [self.extend(s.sid, new_ids, max_new_tokens,
                                d.temperature, d.top_k, d.top_p, d.seed)
                    for (s, new_ids), d in zip(todo, draws)]
        firsts = self._prefill_many(
            [(s.sid, [s.generated[-1]] + new_ids, s.pos)
             for s, new_ids in todo], max_batch_tokens, draws)
        for (s, new_ids), first, d in zip(todo, firsts, draws):
            s.context_ids = s.context_ids + self._emitted(s) + new_ids
            s.pos += 1 + len(new_ids)
            s.generated = [first]
            s.max_new_tokens = max_new_tokens
            s.turn += 1
            s.done = first == self.eos
            self._start_turn(s, d)
        return firsts

    def _prefill_many(self, work, max_batch_tokens: Optional[int],
                      draws: Optional[List[_Draw]] = None) -> List[int]:
        """Prefill ``work`` = [(sid, ids, pos0)] into blocks already
        reserved; returns every item's first token, item i drawn with
        draws[i] (greedy without ``draws``). A forward whose finished items
        are all greedy takes the argmax of its logits as it always did; one
        that finishes a sampled item samples its finished rows only.

        Schedule: each item is cut into the pieces _prefill_paged would cut
        it into (LocalEngine.PREFILL_CHUNK tokens from its own start). A
        forward takes the next piece of every unfinished item, in order, as
        long as it stays within ``max_batch_tokens`` tokens (default
        PREFILL_CHUNK) — at most one piece per item, since a later piece
        attends the rows its predecessor writes; an item's later pieces go
        into later forwards with pos0 advanced. A forward always takes at
        least one piece, so a budget below the piece size degrades to one
        piece per forward. One host sync per forward (the token download),
        and only in forwards that finish an item."""
        if draws is None:
            draws = [_GREEDY] * len(work)
        m, dev = self.model, self.model.device
        chunk = self.engine.PREFILL_CHUNK
        budget = chunk if max_batch_tokens is None else int(max_batch_tokens)
        if budget < 1:
            raise ValueError(f"max_batch_tokens must be >= 1, got {budget}")
        done_at = [0] * len(work)                   # tokens prefilled so far
        firsts: List[Optional[int]] = [None] * len(work)
        blocks = [self.pool.table(sid).blocks for sid, _, _ in work]
        while any(d < len(w[1]) for d, w in zip(done_at, work)):
            take, used = [], 0                      # (item, piece length)
            for i, (_, ids, _) in enumerate(work):
                left = len(ids) - done_at[i]
                if left <= 0:
                    continue
                n = min(chunk, left)
                if take and used + n > budget:
                    continue
                take.append((i, n))
                used += n
            width = max(len(blocks[i]) for i, _ in take)
            table = torch.full((len(take), width), -1, dtype=torch.int32)
            flat: List[int] = []
            for row, (i, n) in enumerate(take):
                table[row, :len(blocks[i])] = torch.tensor(blocks[i],
                                                           dtype=torch.int32)
                flat += work[i][1][done_at[i]:done_at[i] + n]
            batch = ops.RaggedBatch(
                [n for _, n in take],
                [work[i][2] + done_at[i] for i, _ in take], table, dev,
                block_size=self.pool.block_size)
            tokens = torch.tensor(flat, dtype=torch.int64, device=dev)
            logits = m.forward_prefill_paged_ragged(tokens, batch,
                                                    self.pool.k, self.pool.v)
            finished = []
            for row, (i, n) in enumerate(take):
                done_at[i] += n
                if done_at[i] == len(work[i][1]):
                    finished.append((row, i))
            if finished and all(draws[i].temperature == 0
                                for _, i in finished):
                top = logits.argmax(dim=-1).tolist()        # the one sync
                for row, i in finished:
                    firsts[i] = int(top[row])
            elif finished:
                rows = torch.tensor([row for row, _ in finished],
                                    dtype=torch.int64, device=dev)
                top = self._select(logits.index_select(0, rows),
                                   [draws[i] for _, i in finished]
                                   ).tolist()               # the one sync
                for (_, i), t in zip(finished, top):
                    firsts[i] = int(t)
        return firsts

    def _emitted(self, s: Session) -> List[int]:
        """The current turn's tokens, cut at the first EOS (inclusive)."""
        gen = s.generated
        if self.eos in gen:
            gen = gen[: gen.index(self.eos) + 1]
        return list(gen)

    def close(self, sid: int) -> None:
        self.pool.release(sid)
        self.sessions.pop(sid, None)

    # -- decode --------------------------------------------------------------

    @property
    def active(self) -> List[Session]:
        return [s for s in self.sessions.values() if not s.done]

    def step(self) -> int:
        """One decode step for every active session. Returns the number of
        sessions that advanced."""
        return self.step_chunk(1)

    def step_chunk(self, chunk: int = 8) -> int:
        """Up to ``chunk`` decode steps for the CURRENT active set (every
        session drawing with its own sampling parameters and draw count)
        with device-resident token feedback — ONE host sync (the chunk's
        token download) instead of one per step; block capacity for the
        whole chunk is reserved up front and the table tensor is built
        once. Admission/retirement happens between chunks. A session that
        hits EOS mid-chunk keeps decoding garbage rows into its reserved
        blocks until the chunk ends (its `generated`/`pos` stop at the
        EOS, so the extra rows are never attended and the blocks are
        freed on close), and keeps drawing; its ``sampled`` advances only by
        the tokens it keeps. Returns sessions advanced (0 = none active)."""
        act = self.active
        if not act:
            return 0
        m, dev = self.model, self.model.device
        # +3 headroom: graph capture warm-up runs 2 extra steps (their
        # garbage KV rows are rewritten by real replays before any
        # attention reads them — append-at-pos precedes the read of pos)
        reserve = max(chunk, 3) if self.use_graph else chunk
        for s in act:
            self.pool.ensure_capacity(s.sid, s.pos + reserve)
        max_blocks = max(len(self.pool.table(s.sid).blocks) for s in act)
        table = torch.full((len(act), max_blocks), -1, dtype=torch.int32)
        for i, s in enumerate(act):
            blocks = self.pool.table(s.sid).blocks
            table[i, :len(blocks)] = torch.tensor(blocks, dtype=torch.int32)
        table = table.to(dev)
        token = torch.tensor([s.generated[-1] for s in act],
                             dtype=torch.int64, device=dev)
        pos = torch.tensor([s.pos for s in act], dtype=torch.int32, device=dev)
        draws = [_Draw(s.temperature, s.top_k, s.top_p, s.seed, s.sampled)
                 for s in act]
        greedy = all(d.temperature == 0 for d in draws)
        # a manager that has served a sampled session keeps ONE kind of
        # captured step (the sampler; greedy rows ride along at T = 0)
        g = self._chunk_graph(
            len(act), max_blocks, token, pos, table,
            draws if self._seen_sampled else None) \
            if self.use_graph else None
        if g is not None:
            g["token"].copy_(token)
            g["pos"].copy_(pos)
            if g["draw"] is not None:
                fresh = self._draw_bufs(draws)
                for name in ("top_k", "top_p", "temperature", "seed", "step"):
                    g["draw"][name].copy_(fresh[name])
            g["table"].zero_()
            g["table"][:, :max_blocks].copy_(table)
            outs = torch.empty(len(act), chunk, dtype=torch.int64,
                               device=dev)
            for j in range(chunk):
                g["graph"].replay()
                outs[:, j].copy_(g["token"])
            allt = outs.tolist()                           # the one sync
        else:
            bufs = None if greedy else self._draw_bufs(draws)
            steps = []
            for _ in range(chunk):
                logits = self._forward_paged(token, pos, table)
                if bufs is None:
                    token = logits.argmax(dim=-1)
                else:
                    token = self._sample_rows(logits, bufs).to(torch.int64)
                    bufs["step"].add_(1)
                steps.append(token)
                pos = pos + 1
            allt = torch.stack(steps, dim=1).tolist()      # the one sync
        for i, s in enumerate(act):
            for t in allt[i]:
                s.generated.append(int(t))
                s.pos += 1
                s.sampled += 1
                if int(t) == self.eos or \
                        len(s.generated) >= s.max_new_tokens:
                    s.done = True
                    break
        return len(act)

    def run(self, max_steps: int = 4096, chunk: int = 8) -> None:
        done = 0
        while done < max_steps:
            k = min(chunk, max_steps - done)
            if self.step_chunk(k) == 0:
                break
            done += k

    def result(self, sid: int) -> Dict[str, object]:
        s = self.sessions[sid]
        gen = self._emitted(s)
        return {"token_ids": gen,
                "text": self.engine.tokenizer.decode(gen),
                "done": s.done,
                "turn": s.turn,
                "temperature": s.temperature,
                "top_k": s.top_k,
                "top_p": s.top_p,
                "seed": s.seed}

    # -- model forward over the pool ------------------------------------------

    def _forward_paged(self, token: torch.Tensor, pos: torch.Tensor,
                       table: torch.Tensor) -> torch.Tensor:
        """Plain decode forward with block-table attention. Same GEMV /
        norm kernels as LlamaModel.forward_decode (llama.py); RoPE + the
        single-row KV append are torch-side (control plane — O(Hkv*D) per
        session, independent of context length) and fully device-resident:
        the block/offset of the appended row derive from `pos` and `table`
        with gather/advanced indexing, so a whole step chain runs without
        a host sync (step_chunk)."""
        m = self.model
        s = m.spec
        B = token.shape[0]
        BS = self.pool.block_size
        h = F.embedding(token.long(), m.emb)
        scale = 1.0 / math.sqrt(m.D)
        n_layers = len(m.layers)
        x = ops.rmsnorm(h, m.layers[0].norm_attn, s.norm_eps)
        pos_l = pos.long()
        gpu = m.device.type == "cuda"
        # an fp8 pool is never written from here: the op quantises the row
        fused = gpu or self.pool.kv_quant == "fp8"
        if not fused:
            blk = table.gather(1, (pos_l // BS).unsqueeze(1)) \
                .squeeze(1).long()
            off = pos_l % BS
        for li, lw in enumerate(m.layers):
            qkv = ops.linear_decode(x, lw.wqkv)
            q, k, v = m._qkv_views(qkv, B)
            kp, vp = self.pool.k[li], self.pool.v[li]
            if fused:
                # fused in-kernel RoPE + paged append (the eager torch
                # rope/append chain was ~15 launches/layer — ~30% of the
                # serving step)
                att = ops.attn_decode_paged(q, kp, vp, table, pos,
                                            splits=self._splits(B),
                                            scale=scale,
                                            workspace=self._workspace(B),
                                            k=k, v=v, table=m.rope)
            else:
                q_r = ref.apply_rope(q, pos_l, m.rope).contiguous()
                k_r = ref.apply_rope(k, pos_l, m.rope)
                kp[blk, :, off, :] = k_r
                vp[blk, :, off, :] = v
                att = ops.attn_decode_paged(q_r, kp, vp, table, pos,
                                            splits=self._splits(B),
                                            scale=scale,
                                            workspace=self._workspace(B))
            o = ops.linear_decode(att.reshape(B, -1), lw.wo)
            x, h = ops.fused_add_rmsnorm(o, h, lw.norm_mlp, s.norm_eps)
            act = ops.gemv_swiglu(x, lw.wgu)
            d = ops.linear_decode(act, lw.wdown)
            next_norm = (m.layers[li + 1].norm_attn if li + 1 < n_layers
                         else m.norm_f)
            x, h = ops.fused_add_rmsnorm(d, h, next_norm, s.norm_eps)
        return ops.linear_decode(x, m.lm_head)
