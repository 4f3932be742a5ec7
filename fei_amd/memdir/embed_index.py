"""memdir semantic search: a persisted embedding index over the corpus.

Replaces the reference's O(corpus) per-query full file scan
(memdir_tools/search.py:361-367) for semantic retrieval: embeddings are
computed by the MI355X encoder (fei_amd/models/bge.py — GEMMs on MFMA),
persisted next to the Memdir tree, and queried with one fused score + top-k
scan on GPU (ops.score_topk; BASELINE.json configs[3]: 1M-memory corpus,
1 GPU). A search can be scoped to folders and statuses, applied inside the
scan, and up to 8 queries share one scan (``search_many``). The lexical
query language stays available for format compatibility.

Index layout on disk (under ``<base>/.index/``):
  embeddings.npy   float16 [N, C]
  meta.json        {"ids": [...], "dim": C, "version": 1}
"""

from __future__ import annotations

import json
import os
import time
from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from fei_amd import ops
from fei_amd.memdir import utils as mu
from fei_amd.utils.logging import get_logger

logger = get_logger("memdir.embed_index")


def _scope_key(names: Optional[Iterable[str]]) -> Optional[Tuple[str, ...]]:
    if names is None:
        return None
    if isinstance(names, str):
        names = [names]
    return tuple(sorted(set(names)))


class EmbeddingIndex:
    def __init__(self, base: Optional[str] = None, encoder=None,
                 device: Optional[torch.device] = None,
                 scan_dtype: str = "f32"):
        if scan_dtype not in ("f32", "f16"):
            raise ValueError(f"scan_dtype must be 'f32' or 'f16', got "
                             f"{scan_dtype!r}")
        self.base = mu.get_memdir_base(base)
        self.index_dir = os.path.join(self.base, ".index")
        self._encoder = encoder
        if device is None:
            device = torch.device("cuda:0") if torch.cuda.is_available() \
                else torch.device("cpu")
        self.device = device
        self.embeddings: Optional[torch.Tensor] = None    # [N, C] on device
        self.ids: List[str] = []                          # "folder/status/filename"
        self._loaded = False
        # scan state, kept in step with ids (see _reset_scan_state)
        self.scan_dtype = scan_dtype
        self.folder_codes: Optional[torch.Tensor] = None  # int16 [N] on device
        self.status_codes: Optional[torch.Tensor] = None  # int16 [N] on device
        self._folder_code: Dict[str, int] = {}
        self._status_code: Dict[str, int] = {}
        self._masks: Dict[Tuple, Optional[torch.Tensor]] = {}
        self._scan_f16: Optional[torch.Tensor] = None

    # -- encoder -------------------------------------------------------------

    @property
    def encoder(self):
        if self._encoder is None:
            from fei_amd.models.bge import BgeEncoder
            self._encoder = BgeEncoder(device=self.device)
        return self._encoder

    # -- persistence ---------------------------------------------------------

    def save(self) -> None:
        os.makedirs(self.index_dir, exist_ok=True)
        if self.embeddings is None:
            return
        np.save(os.path.join(self.index_dir, "embeddings.npy"),
                self.embeddings.cpu().to(torch.float16).numpy())
        with open(os.path.join(self.index_dir, "meta.json"), "w") as f:
            json.dump({"ids": self.ids, "dim": self.embeddings.shape[1],
                       "version": 1}, f)

    def load(self) -> bool:
        try:
            emb = np.load(os.path.join(self.index_dir, "embeddings.npy"))
            with open(os.path.join(self.index_dir, "meta.json")) as f:
                meta = json.load(f)
            self.embeddings = torch.from_numpy(emb).to(self.device).float()
            self.ids = meta["ids"]
            self._loaded = True
            self._reset_scan_state()
            return True
        except (OSError, json.JSONDecodeError, ValueError):
            return False

    # -- building ------------------------------------------------------------

    @staticmethod
    def _memory_text(mem: Dict[str, Any]) -> str:
        headers = mem.get("headers", {})
        return (headers.get("Subject", "") + "\n" +
                headers.get("Tags", "") + "\n" +
                mem.get("content", ""))[:2000]

    def build(self, folders: Optional[List[str]] = None,
              statuses: Optional[List[str]] = None,
              batch_size: int = 64) -> int:
        """(Re)build the index over the memdir corpus. Off the query
        critical path by design (SURVEY.md §7 hard-part 4)."""
        t0 = time.time()
        texts: List[str] = []
        ids: List[str] = []
        for folder in folders if folders is not None else mu.list_folders(self.base):
            for status in statuses if statuses is not None else ["cur", "new"]:
                for mem in mu.list_memories(folder, status, include_content=True,
                                            base=self.base):
                    texts.append(self._memory_text(mem))
                    ids.append(f"{folder}\x00{status}\x00{mem['filename']}")
        if not texts:
            self.embeddings = None
            self.ids = []
            self._reset_scan_state()
            return 0
        emb = self.encoder.encode_texts(texts, batch_size=batch_size)
        self.embeddings = emb.float()
        self.ids = ids
        self._loaded = True
        self._reset_scan_state()
        self.save()
        logger.info("indexed %d memories in %.2fs", len(ids), time.time() - t0)
        return len(ids)

    def remove(self, id_substr: str) -> int:
        """Drop rows whose id contains ``id_substr`` (e.g. a filename when
        the memory was moved/deleted). Returns how many were removed."""
        if self.embeddings is None:
            return 0
        keep = [i for i, k in enumerate(self.ids) if id_substr not in k]
        removed = len(self.ids) - len(keep)
        if removed:
            rows = torch.tensor(keep, dtype=torch.long, device=self.device)
            self.embeddings = self.embeddings[rows]
            self.ids = [self.ids[i] for i in keep]
            if self.folder_codes is not None:
                self.folder_codes = self.folder_codes[rows]
                self.status_codes = self.status_codes[rows]
            self._index_changed()
        return removed

    def add_texts(self, texts: List[str], ids: List[str]) -> None:
        """Incremental append (used by tests and live updates)."""
        emb = self.encoder.encode_texts(texts).float()
        if self.embeddings is None:
            self.embeddings = emb
            self.ids = list(ids)
            self._reset_scan_state()
        else:
            if self.folder_codes is None:
                self._reset_scan_state()
            self.embeddings = torch.cat([self.embeddings, emb], dim=0)
            self.ids.extend(ids)
            f, st = self._codes_of(ids)
            self.folder_codes = torch.cat([self.folder_codes, f])
            self.status_codes = torch.cat([self.status_codes, st])
            self._index_changed()

    # -- scan state ----------------------------------------------------------

    def _codes_of(self, ids: List[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        """int16 folder and status codes of ``ids`` ("folder\0status\0file"),
        new names getting the next code. An id of another form gets -1 and
        belongs to no scope."""
        fc = np.full(len(ids), -1, dtype=np.int16)
        sc = np.full(len(ids), -1, dtype=np.int16)
        for j, key in enumerate(ids):
            parts = key.split("\x00")
            if len(parts) != 3:
                continue
            fc[j] = self._folder_code.setdefault(parts[0],
                                                 len(self._folder_code))
            sc[j] = self._status_code.setdefault(parts[1],
                                                 len(self._status_code))
        if len(self._folder_code) > 32767:
            raise ValueError("more than 32767 folders in one index")
        return (torch.from_numpy(fc).to(self.device),
                torch.from_numpy(sc).to(self.device))

    def _index_changed(self) -> None:
        """Rows changed: drop what was derived from them."""
        self._masks.clear()
        self._scan_f16 = None
        e = self.embeddings
        if e is not None and (not e.is_contiguous() or e.data_ptr() % 16):
            self.embeddings = e.clone(memory_format=torch.contiguous_format)

    def _reset_scan_state(self) -> None:
        """Rebuild the per-row codes from ``ids`` (build, load, first add)."""
        self._folder_code, self._status_code = {}, {}
        if self.embeddings is None:
            self.folder_codes = self.status_codes = None
        else:
            self.folder_codes, self.status_codes = self._codes_of(self.ids)
        self._index_changed()

    def _scope_mask(self, folders, statuses) -> Optional[torch.Tensor]:
        """uint8 [N] on the device, non-zero where the row's folder and
        status are both listed; None for no restriction. Computed from the
        code tensors and cached until the index next changes."""
        key = (_scope_key(folders), _scope_key(statuses))
        if key == (None, None):
            return None
        if key not in self._masks:
            ok = torch.ones(len(self.ids), dtype=torch.bool,
                            device=self.device)
            for names, table, codes in (
                    (key[0], self._folder_code, self.folder_codes),
                    (key[1], self._status_code, self.status_codes)):
                if names is None:
                    continue
                want = torch.tensor(
                    [table[n] for n in names if n in table],
                    dtype=torch.int16, device=self.device)
                ok &= torch.isin(codes, want)
            self._masks[key] = ok.to(torch.uint8)
        return self._masks[key]

    def _scan_matrix(self) -> torch.Tensor:
        """What the scan reads: the f32 embeddings, or with scan_dtype="f16"
        an f16 copy holding exactly the values save() persists."""
        if self.scan_dtype == "f32":
            return self.embeddings
        if self._scan_f16 is None:
            self._scan_f16 = self.embeddings.to(torch.float16)
        return self._scan_f16

    def _ready(self) -> bool:
        if self.embeddings is None and not self._loaded:
            self.load()                    # fall back to the on-disk index
        return self.embeddings is not None and len(self.ids) > 0

    def _topk_rows(self, qmat: torch.Tensor, topk: int,
                   mask: Optional[torch.Tensor]
                   ) -> List[List[Tuple[str, float]]]:
        """[(id, score)] per row of qmat [Q, C] f32, Q <= 8."""
        emb = self._scan_matrix()
        C = emb.shape[1]
        # every search the kernel takes goes through it, the unscoped
        # single query included: 2.8x the torch expression at 1M x 768 f32
        # (profiles/score_topk.md)
        fused = (1 <= topk <= ops.SCORE_TOPK_MAX_K and C % 8 == 0
                 and C <= ops.SCORE_TOPK_MAX_C)
        if fused:
            vals, idx = ops.score_topk(emb, qmat, topk, mask)
            vals, idx = vals.tolist(), idx.tolist()
        else:
            # topk > 64 (or a width the kernel does not take): score every
            # row, then select
            scores = qmat @ self.embeddings.t()                 # [Q, N]
            n = scores.shape[1]
            if mask is not None:
                scores = scores.masked_fill(mask == 0, float("-inf"))
                n = int(mask.sum())
            v, i = torch.topk(scores, min(topk, n), dim=1)
            vals, idx = v.tolist(), i.tolist()
        return [[(self.ids[i], float(v)) for v, i in zip(vr, ir) if i >= 0]
                for vr, ir in zip(vals, idx)]

    # -- querying ------------------------------------------------------------

    def search(self, query: str, topk: int = 10,
               folders: Optional[List[str]] = None,
               statuses: Optional[List[str]] = None
               ) -> List[Tuple[str, float]]:
        """Cosine top-k over the index: one fused score + top-k scan
        (ops.score_topk). Returns [(id, score)], best first.

        ``folders`` / ``statuses`` restrict the search to rows whose id has a
        listed folder and a listed status. The restriction is applied inside
        the scan, so the result is the true top-k of the scope, shorter than
        ``topk`` only when the scope has fewer rows."""
        return self.search_many([query], topk, folders, statuses)[0]

    def search_many(self, queries: List[str], topk: int = 10,
                    folders: Optional[List[str]] = None,
                    statuses: Optional[List[str]] = None
                    ) -> List[List[Tuple[str, float]]]:
        """search() for several queries: one encoder batch, and one corpus
        scan per 8 queries instead of one per query."""
        if not queries:
            return []
        if not self._ready() or topk < 1:
            return [[] for _ in queries]
        qmat = self.encoder.encode_texts(list(queries)).float().contiguous()
        mask = self._scope_mask(folders, statuses)
        out: List[List[Tuple[str, float]]] = []
        for j in range(0, len(queries), ops.SCORE_TOPK_MAX_Q):
            out.extend(self._topk_rows(qmat[j:j + ops.SCORE_TOPK_MAX_Q],
                                       topk, mask))
        return out

    def search_memories(self, query: str, topk: int = 10,
                        with_content: bool = True,
                        folders: Optional[List[str]] = None,
                        statuses: Optional[List[str]] = None
                        ) -> List[Dict[str, Any]]:
        """Top-k resolved back to memdir records with scores."""
        return self._resolve(self.search(query, topk, folders, statuses),
                             with_content)

    def _resolve(self, hits: List[Tuple[str, float]],
                 with_content: bool) -> List[Dict[str, Any]]:
        out = []
        for key, score in hits:
            folder, status, filename = key.split("\x00")
            mem = mu.read_memory(folder, status, filename, base=self.base)
            if mem is None:
                continue
            mem["score"] = round(score, 4)
            if not with_content:
                mem.pop("content", None)
            out.append(mem)
        return out
