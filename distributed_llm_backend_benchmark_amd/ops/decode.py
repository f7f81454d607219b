"""KV cache and single-query (decode) attention (``csrc/attn_decode.hip``).

Layout, per layer and per rank: ``k_cache`` / ``v_cache`` are ``[B, H_local, L_max, D]`` bf16,
contiguous (the key stream of one ``(b, h)`` is one contiguous run). ``length`` is ONE device
``int32[1]`` — the tokens already cached — shared by the batch and by every layer. The kernels
read it from device memory, so a decode step captured in a HIP graph replays for successive
positions without recapture; the host keeps a mirror (``KVCache.pos``) for bounds checks only.

* :func:`kv_append` copies the K / V rows of a fused ``[B, T, 3C]`` QKV tensor into cache
  positions ``[length, length + T)`` (prefill: ``T = S``; decode: ``T = 1``).
* :func:`decode_attention` takes ``qkv [B, 1, 3C]``, stores the token's K / V at ``length`` and
  attends over ``length + 1`` keys: a split over the key axis in chunks of :data:`CHUNK` keys
  (one workgroup per chunk, head and batch entry, fp32 partials ``(m, l, o[D])`` in a workspace)
  and a combine kernel that merges the live chunks in chunk order and writes ``[B, 1, C]`` with
  heads interleaved, as :func:`..attention.causal_attention` returns. No atomics: bit-identical
  from run to run. It does NOT advance ``length``: the model does, once per step, after its
  last layer (:meth:`KVCache.advance`).

On the GPU with head dim 64 / 128 the HIP kernels are the only path (a missing library raises).
CPU tensors, ``DLBB_KERNELS=torch`` and other head dims use torch (:func:`torch_kv_append`,
:func:`torch_decode_attention`): an index copy into the cache and
``F.scaled_dot_product_attention`` on ``cache[:, :, :pos + 1]``. That path slices by the HOST
position, so it is not replayable across positions in a captured graph.

FP8 cache (opt-in, ``KVCache(kv_dtype="fp8")``; the same file's ``KvE4m3`` kernels). The contract:

* ``k_cache`` / ``v_cache`` are ``[B, H_local, L_max, D]`` ``torch.float8_e4m3fn``, contiguous;
  ``k_scale`` / ``v_scale`` are ``[B, H_local, L_max]`` fp32, contiguous: one scale per cached
  row of ``D`` values, ``row ~= float(code) * scale``.
* A row is quantised exactly as :mod:`.fp8` quantises one (``fp8._quantize_torch`` is the
  reference, compared bit for bit): ``amax == 0`` gives scale 1 and bytes 0; otherwise ``inv =
  448 / amax``, ``scale = amax / 448`` (IEEE fp32 divisions) and ``code = e4m3fn_rne(float(x) *
  inv)``.
* A row stores ``D + 4`` bytes against ``2 D``: 0.516 of the bf16 cache at D = 128, 0.531 at 64.
* A decode step stores the new token QUANTISED and attends to it in its quantised form: the
  step's result is attention over the cache contents after the append, exactly, and a replayed
  graph gives the same bits as eager. The prefill is unchanged: it attends over the bf16 ``qkv``
  it was given, only its :func:`kv_append` quantises.
* ``length``, ``len_bound``, the fp32 ``(m, l, o[D])`` workspace and the combine step keep their
  meaning; the split runs in chunks of :data:`CHUNK_FP8` keys.

:func:`kv_append` / :func:`decode_attention` take the scales as ``k_scale`` / ``v_scale``
(``None`` = the bf16 cache). The dispatch rule is the same: the HIP kernels on a GPU tensor with
head dim 64 / 128 and contiguous bf16 ``qkv``; the torch forms otherwise (the append quantises
with ``fp8._quantize_torch``, the decode dequantises ``cache[:, :, :pos + 1]`` to fp32 and runs
SDPA).

Per-sequence lengths (opt-in, ``KVCache(per_sequence=True)``; the ``*_seq`` entry points, the same
kernel templates with ``length[b]`` in place of ``*length``). The contract:

* ``length`` is a device ``int32[B]``: row ``b`` of the batch holds ``length[b]`` cached tokens.
  :func:`kv_append` and :func:`decode_attention` dispatch on ``length.numel()``: 1 is the shared
  length above, ``B`` the per-sequence path, anything else raises ``ValueError`` (so a batch of
  one always takes the shared-length kernels).
* ``length[b] < 0`` marks an EMPTY slot: the append writes nothing for it, its split workgroups
  exit before any load or store and its output row is zeros. (The shared-length kernels clamp a
  negative length to 0; that stays.)
* The device guards are per row: ``length[b] >= L_max`` attends over ``L_max`` keys and stores
  nothing, append positions ``>= L_max`` are dropped.
* ``len_bound`` is the host's upper bound of ``max_b length[b] + 1``; ``pos`` may be a sequence of
  ``B`` host positions (overflow checks, and the torch path).
* For a given ``(b, h, chunk, L)`` a workgroup does exactly what the shared-length kernel does,
  so row ``b`` of a ragged launch has the bits of a batch-1 shared-length launch at
  ``length[b]``.
* Torch forms: a per-row index copy for the append and, for the decode, the shared-length torch
  form on each row's batch-1 slice at its host position (bit-identical to it; a single masked
  SDPA is not); empty slots give zero rows.

Paged cache (opt-in, ``KVCache(page_size=P, n_pages=N)``; the ``*_paged`` entry points, the same
kernel templates with the row address taken through a block table). The contract:

* Pools: per layer and rank ``k_pool`` / ``v_pool`` are ``[n_pages, H_local, P, D]``, contiguous,
  bf16 or ``float8_e4m3fn``; for FP8 ``k_scale`` / ``v_scale`` are ``[n_pages, H_local, P]`` fp32.
  The ``P`` rows of one ``(page, head)`` are one contiguous run. The pools are shared by every
  batch row; they are handed to :func:`kv_append` / :func:`decode_attention` as the caches.
* ``block_table`` is a device ``int32[B, max_pages]``, ``max_pages = ceil(L_max / P)``; one table
  serves every layer, as one ``length`` does. Logical position ``t`` of row ``b`` lives in
  physical page ``block_table[b, t // P]`` at row ``t % P``. A negative entry (and on the device
  any entry outside ``[0, n_pages)``) means the page is NOT MAPPED.
* ``P`` is a power of two in :data:`PAGE_SIZES` and must divide the split kernel's ``chunk`` (a
  chunk covers whole pages, at most 64 of them); the ops raise ``ValueError`` otherwise.
* ``length`` is always the per-sequence ``int32[B]`` (also for ``B = 1``) and every per-sequence
  rule above holds; ``L_max`` (``max_len``) is the logical cap. The workspace and the combine
  kernel keep their meaning.
* Unmapped pages on the device: an entry outside ``[0, n_pages)`` never produces an address. A
  store to such a position (append, fused append) is dropped; a key on such a page below ``L`` is
  masked out of the softmax (its loads go to a mapped row). This is a contract, not only a guard:
  the right-padded prefill appends all ``T`` rows with only ``prompt_lens[b]`` positions reserved.
  A live row without any mapped key has no defined output.
* With ``pos`` given, a page holding a position in ``[0, pos[b] + T)`` of a live row that is
  unmapped in the host mirror (``table_host``) raises ``ValueError`` before any launch
  (``n_keep`` bounds the check per row for the padded prefill).
* For a given ``(b, h, chunk, L)`` a workgroup does the arithmetic of the ``*_seq`` kernel in the
  same order, only the addresses differ: with equal contents row ``b`` of a paged launch, and the
  cache gathered through the table afterwards, have the bits of the contiguous per-sequence launch.
* Torch forms: the row's mapped pages are gathered into a contiguous batch-1 cache, the
  contiguous torch form runs on it and the written pages are copied back, so the torch path is
  bit-identical to the contiguous torch path too.
"""

from __future__ import annotations

import math
from typing import List, Optional, Sequence, Union

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, use_hip
from .attention import HEAD_DIMS, _views
from .fp8 import E4M3, _quantize_torch

# keys per workgroup of the split kernel (csrc/attn_decode.hip takes it per launch; the
# alternatives measured are in docs/PERFORMANCE.md)
CHUNK = 256
# keys per workgroup of the FP8-cache split kernel (csrc/attn_decode.hip too), a constant of its
# own: a 256-key chunk holds half the bytes there. 256 / 512 / 1024 measured (docs/PERFORMANCE.md):
# 512 is 10-15 % faster on the rows of >= 128 MiB of bf16 K + V and 6-32 % slower on the smaller
# head-dim-128 ones, 1024 is 3-17 % faster from 256 MiB and up to 67 % slower below
CHUNK_FP8 = 256
KV_DTYPES = ("bf16", "fp8")
# page sizes of the paged cache (positions per page; csrc/attn_decode.hip checks the same set)
PAGE_SIZES = (16, 32, 64, 128, 256)
# default page size of the paged cache. 16 / 64 / 256 measured against the contiguous per-sequence
# kernel (docs/PERFORMANCE.md, "Paged KV cache"): on the bf16 cache none lies inside that kernel's
# own spread on every row (2-11 % / 0-10 % / 2-9 % slower), on the FP8 cache all are within
# -2 .. +3 %. So 256, where a chunk is one page and a workgroup does one table look-up
PAGE_SIZE = 256
# table entries one split workgroup holds: chunk / P may not exceed it
MAX_CHUNK_PAGES = 64
# append + attend in one launch (the chunk owning position `length` takes the token's K / V from
# qkv and stores them) instead of a kv_append launch before the attention
FUSED_APPEND = True


def workspace_numel(batch: int, n_head: int, head_dim: int, max_len: int,
                    chunk: int = CHUNK) -> int:
    """fp32 elements of the split kernel's partials: ``[B, H, n_chunks, D + 2]``."""
    return batch * n_head * ((max_len + chunk - 1) // chunk) * (head_dim + 2)


def check_page_size(page_size: int, chunk: Optional[int] = None) -> int:
    """``page_size`` as an int; ``ValueError`` unless it is one of :data:`PAGE_SIZES` and (with
    ``chunk``) a chunk is 1 .. :data:`MAX_CHUNK_PAGES` whole pages."""
    P = int(page_size)
    if P not in PAGE_SIZES:
        raise ValueError(f"page_size {page_size}: need a power of two in {PAGE_SIZES}")
    if chunk is not None and (chunk % P or chunk // P > MAX_CHUNK_PAGES):
        raise ValueError(f"page_size {P} must divide the chunk of {chunk} keys into at most "
                         f"{MAX_CHUNK_PAGES} pages")
    return P


class _PageAllocator:
    """The page pool's bookkeeping, shared by a paged :class:`KVCache` and its slot views: the
    LIFO free list, the host mirror of the block table, the device table and the pages each row
    holds (a row's pages are always its first ``held[b]`` table entries)."""

    def __init__(self, n_pages: int, page_size: int, batch: int, max_pages: int, device):
        self.n_pages, self.page_size = int(n_pages), int(page_size)
        self.free = list(range(self.n_pages - 1, -1, -1))       # pop() hands out page 0 first
        self.host = torch.full((batch, max_pages), -1, dtype=torch.int32)
        self.table = torch.full((batch, max_pages), -1, dtype=torch.int32, device=device)
        self.held = [0] * batch
        self.peak = 0

    @property
    def in_use(self) -> int:
        return self.n_pages - len(self.free)

    def update(self, want, release=()) -> None:
        """Rows in ``release`` give every page back, then each row ``r`` of ``want`` grows to
        ``want[r]`` pages. All or nothing: a request the free list cannot satisfy raises
        ``ValueError`` and changes nothing, and so does (``RuntimeError``) one that would have to
        change the table while the stream is capturing. Changed rows are uploaded with a device
        copy on the current stream."""
        release = [r for r in dict.fromkeys(release) if self.held[r]]
        grow = {r: n for r, n in want.items() if n > (0 if r in release else self.held[r])}
        if not release and not grow:
            return
        need = sum(n - (0 if r in release else self.held[r]) for r, n in grow.items())
        free = len(self.free) + sum(self.held[r] for r in release)
        if need > free:
            raise ValueError(f"KV page pool exhausted: {need} pages needed, {free} free "
                             f"(pool of {self.n_pages} pages of {self.page_size} positions)")
        if self.table.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the block table cannot change while the stream is capturing: "
                               "reserve_all(len_bound) before the capture")
        for r in release:
            pages = self.host[r, :self.held[r]].tolist()
            self.free.extend(reversed(pages))                   # LIFO: the row's first page on top
            self.host[r, :self.held[r]] = -1
            self.held[r] = 0
        for r, n in grow.items():
            while self.held[r] < n:
                self.host[r, self.held[r]] = self.free.pop()
                self.held[r] += 1
        self.peak = max(self.peak, self.in_use)
        for r in list(release) + [r for r in grow if r not in release]:
            self.table[r].copy_(self.host[r])


class KVCache:
    """K / V of every layer of one rank, the shared device ``length``, and the split kernel's
    workspace. ``num_layers = 0`` holds no K / V (the stateless ``attention="slice"`` stub):
    only the position bookkeeping. ``kv_dtype="fp8"``: ``k`` / ``v`` hold e4m3 codes and
    ``k_scale`` / ``v_scale`` one fp32 scale per cached row (module docstring); with ``"bf16"``
    the two scale lists hold ``None`` per layer.

    ``per_sequence=True``: ``length`` is ``int32[B]`` and ``pos`` a list of ``B`` host mirrors, one
    per batch row; a negative entry is an empty slot (module docstring). :meth:`set_lengths`,
    :meth:`retire`, :meth:`slot` and :meth:`live_bytes` belong to that form; :meth:`advance` moves
    the live rows only.

    ``page_size=P`` (with ``n_pages=N``, default ``B * ceil(max_len / P)``) is the PAGED cache
    (module docstring): it implies ``per_sequence=True``; ``k`` / ``v`` (and the scales) are the
    pools ``[N, H, P, D]``, ``block_table`` the device ``int32[B, ceil(max_len / P)]`` table and
    ``table_host`` its host mirror. Pages come from a LIFO free list: :meth:`reserve`,
    :meth:`reserve_all`, :meth:`set_lengths` and :meth:`advance` map what a row needs,
    :meth:`retire` and ``set_length(0)`` give pages back. A request the free list cannot satisfy
    raises ``ValueError`` and changes nothing; one that would change the table while the stream
    is capturing raises ``RuntimeError``, so a runner that replays one captured step calls
    ``reserve_all(len_bound)`` before the capture."""

    def __init__(self, num_layers: int, batch: int, n_head_local: int, head_dim: int,
                 max_len: int, device, dtype=torch.bfloat16, kv_dtype: str = "bf16",
                 per_sequence: bool = False, page_size: Optional[int] = None,
                 n_pages: Optional[int] = None):
        if max_len < 1 or batch < 1:
            raise ValueError(f"KVCache needs batch >= 1 and max_len >= 1, got {batch}, {max_len}")
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"KVCache kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
        self.kv_dtype = kv_dtype
        self.per_sequence = bool(per_sequence) or page_size is not None
        self.page_size: Optional[int] = None
        self._pages: Optional[_PageAllocator] = None
        # paged, during a right-padded prefill: the tokens per row that must land on mapped
        # pages (kv_append's n_keep); set and cleared by the model around that one forward
        self.n_keep: Optional[List[int]] = None
        if page_size is None and n_pages is not None:
            raise ValueError("KVCache n_pages needs a page_size")
        if page_size is not None:
            self.page_size = check_page_size(page_size,
                                             CHUNK_FP8 if kv_dtype == "fp8" else CHUNK)
            max_pages = (int(max_len) + self.page_size - 1) // self.page_size
            n_pages = int(batch) * max_pages if n_pages is None else int(n_pages)
            if n_pages < 1:
                raise ValueError(f"KVCache n_pages must be >= 1, got {n_pages}")
        self._parent, self._row = None, 0       # set on a slot view (:meth:`slot`)
        self._staged = None                     # (values, device tensor) of :meth:`set_lengths`
        fp8 = kv_dtype == "fp8"
        if fp8:
            dtype = E4M3
        self.num_layers, self.batch = int(num_layers), int(batch)
        self.n_head, self.head_dim, self.max_len = int(n_head_local), int(head_dim), int(max_len)
        self.device = torch.device(device)
        shape = (self.batch, self.n_head, self.max_len, self.head_dim)
        if self.page_size is not None:
            shape = (n_pages, self.n_head, self.page_size, self.head_dim)
            self._pages = _PageAllocator(n_pages, self.page_size, self.batch, max_pages,
                                         self.device)
        self.k: List[torch.Tensor] = [torch.zeros(shape, dtype=dtype, device=self.device)
                                      for _ in range(self.num_layers)]
        self.v: List[torch.Tensor] = [torch.zeros(shape, dtype=dtype, device=self.device)
                                      for _ in range(self.num_layers)]
        self.k_scale: List[Optional[torch.Tensor]] = [
            torch.ones(shape[:3], dtype=torch.float32, device=self.device) if fp8 else None
            for _ in range(self.num_layers)]
        self.v_scale: List[Optional[torch.Tensor]] = [
            torch.ones(shape[:3], dtype=torch.float32, device=self.device) if fp8 else None
            for _ in range(self.num_layers)]
        self.length = torch.zeros(self.batch if self.per_sequence else 1, dtype=torch.int32,
                                  device=self.device)
        # host mirror of `length`: bounds checks only (a list of B with per_sequence)
        self._pos: Union[int, List[int]] = [0] * self.batch if self.per_sequence else 0
        # host upper bound of length + 1 for the split grid (None = max_len); a runner that
        # replays one captured step sets the final position here before the capture
        self.len_bound: Optional[int] = None
        self.workspace = (torch.empty(workspace_numel(self.batch, self.n_head, self.head_dim,
                                                      self.max_len, CHUNK_FP8 if fp8 else CHUNK),
                                      dtype=torch.float32, device=self.device)
                          if self.num_layers else None)

    @property
    def pos(self):
        return self._pos

    @pos.setter
    def pos(self, value) -> None:
        self._pos = value
        if self._parent is not None:            # a slot view mirrors its position back
            self._parent._pos[self._row] = int(value[0] if isinstance(value, list) else value)

    # ---- the paged form: the pool's bookkeeping (rows of a slot view are the parent's) ----
    @property
    def paged(self) -> bool:
        return self._pages is not None

    @property
    def block_table(self) -> Optional[torch.Tensor]:
        """The device ``int32[B, max_pages]`` table (None for a contiguous cache)."""
        return None if self._pages is None else self._pages.table[self._row:self._row + self.batch]

    @property
    def table_host(self) -> Optional[torch.Tensor]:
        """The host mirror of :attr:`block_table` (a CPU ``int32`` view; do not write it)."""
        return None if self._pages is None else self._pages.host[self._row:self._row + self.batch]

    @property
    def n_pages(self) -> int:
        return self._need_paged("n_pages").n_pages

    @property
    def pages_in_use(self) -> int:
        return self._need_paged("pages_in_use").in_use

    @property
    def peak_pages_in_use(self) -> int:
        return self._need_paged("peak_pages_in_use").peak

    @property
    def free_pages(self) -> List[int]:
        """The free list, the next page to be handed out last."""
        return list(self._need_paged("free_pages").free)

    def _need_paged(self, what: str) -> _PageAllocator:
        if self._pages is None:
            raise ValueError(f"KVCache.{what} needs a paged cache (page_size=...)")
        return self._pages

    def _pages_for(self, n_tokens: int) -> int:
        n = min(max(int(n_tokens), 0), self.max_len)
        return (n + self.page_size - 1) // self.page_size

    def reserve(self, b: int, n_tokens: int) -> None:
        """Map pages so that row ``b`` can hold ``n_tokens`` positions (never unmaps)."""
        pages = self._need_paged("reserve")
        if not 0 <= b < self.batch or n_tokens > self.max_len:
            raise ValueError(f"KVCache.reserve({b}, {n_tokens}): batch {self.batch}, max_len "
                             f"{self.max_len}")
        pages.update({self._row + b: self._pages_for(n_tokens)})

    def reserve_all(self, n_tokens: Union[int, Sequence[int]]) -> None:
        """:meth:`reserve` for every live row (one value, or one per row), all or nothing."""
        pages = self._need_paged("reserve_all")
        vals = [int(n_tokens)] * self.batch if isinstance(n_tokens, int) else \
            [int(v) for v in n_tokens]
        if len(vals) != self.batch or any(v > self.max_len for v in vals):
            raise ValueError(f"KVCache.reserve_all({n_tokens}): need {self.batch} values <= "
                             f"{self.max_len}")
        pages.update({self._row + b: self._pages_for(v)
                      for b, (v, p) in enumerate(zip(vals, self._pos)) if p >= 0})

    def set_length(self, n: int, keep_pages: bool = False) -> None:
        """Set the device length and the host mirror (0 = empty the cache); with
        ``per_sequence`` every row gets ``n``. Paged: 0 gives every page back, another value
        reserves for it; ``keep_pages=True`` empties the rows and leaves the table as it is (a
        runner that replays captured steps: one device fill, the table must not change)."""
        if not 0 <= n <= self.max_len:
            raise ValueError(f"KVCache length {n} outside [0, {self.max_len}]")
        if self._pages is not None:
            rows = range(self._row, self._row + self.batch)
            if n == 0 and keep_pages:
                pass
            elif n == 0:
                self._pages.update({}, release=rows)
            else:
                self._pages.update({r: self._pages_for(n) for r in rows})
        self.length.fill_(int(n))
        self.pos = [int(n)] * self.batch if self.per_sequence else int(n)

    def _need_per_sequence(self, what: str) -> None:
        if not self.per_sequence:
            raise ValueError(f"KVCache.{what} needs a per_sequence=True cache")

    def set_lengths(self, lengths: Sequence[int]) -> None:
        """Set every row's device length and host mirror; a negative entry empties the slot.
        The values are staged in a device tensor that the same values reuse, so a call repeated
        under HIP-graph capture (after an eager call with these values) is a device copy."""
        self._need_per_sequence("set_lengths")
        vals = [int(v) for v in lengths]
        if len(vals) != self.batch or any(v > self.max_len for v in vals):
            raise ValueError(f"KVCache lengths {vals}: need {self.batch} values <= {self.max_len}")
        vals = [max(v, -1) for v in vals]
        if self._pages is not None:             # a negative entry gives the row's pages back
            self._pages.update({self._row + b: self._pages_for(v)
                                for b, v in enumerate(vals) if v >= 0},
                               release=[self._row + b for b, v in enumerate(vals) if v < 0])
        if self._staged is None or self._staged[0] != vals:
            self._staged = (vals, torch.tensor(vals, dtype=torch.int32, device=self.device))
        self.length.copy_(self._staged[1])
        self.pos = vals

    def retire(self, b: int) -> None:
        """Row ``b`` holds no sequence any more: ``length[b] = -1``. Paged: its pages go back
        to the free list and its table row is unmapped."""
        self._need_per_sequence("retire")
        if self._pages is not None:
            self._pages.update({}, release=[self._row + b])
        self.length[b:b + 1].fill_(-1)
        self._pos[b] = -1

    def check_room(self, t: int) -> None:
        top = max(self._pos) if self.per_sequence else self._pos     # the longest live row
        if top + t > self.max_len:
            raise ValueError(f"KVCache overflow: position {top} + {t} tokens > max_len "
                             f"{self.max_len}")

    def advance(self, t: int) -> None:
        """``length += t``: a device add on the current stream (captured with the step). With
        ``per_sequence`` the add is ``(length >= 0) * t``: empty slots stay empty."""
        self.check_room(t)
        if self._pages is not None:             # the live rows' pages for pos + t
            self._pages.update({self._row + b: self._pages_for(p + int(t))
                                for b, p in enumerate(self._pos) if p >= 0})
        if self.per_sequence:
            self.length.add_((self.length >= 0).to(torch.int32) * int(t))
            self.pos = [p + int(t) if p >= 0 else p for p in self._pos]
            return
        self.length.add_(int(t))
        self.pos += int(t)

    def slot(self, b: int) -> "KVCache":
        """A batch-1 shared-length :class:`KVCache` over row ``b``: views of its K / V, scales
        and ``length[b:b + 1]`` (``[B, H, L_max, D]`` is contiguous in ``b``) and the parent's
        workspace, so a prompt can be prefilled into one slot while the other rows keep their
        contents. Its position is mirrored back to the parent. A retired row reads -1: claim it
        with ``set_length(0)`` first. Paged: a batch-1 PAGED view (per-sequence, as every paged
        cache): ``length[b:b + 1]``, ``block_table[b:b + 1]``, the shared pools and workspace;
        its reservations come from the parent's free list."""
        self._need_per_sequence("slot")
        if not 0 <= b < self.batch:
            raise ValueError(f"KVCache.slot({b}): batch is {self.batch}")
        s = object.__new__(KVCache)
        s.kv_dtype, s.per_sequence = self.kv_dtype, False
        s.num_layers, s.batch = self.num_layers, 1
        s.n_head, s.head_dim, s.max_len = self.n_head, self.head_dim, self.max_len
        s.device = self.device
        s.page_size, s._pages, s.n_keep = self.page_size, self._pages, None
        if self._pages is not None:
            s.per_sequence = True
            s.k, s.v, s.k_scale, s.v_scale = self.k, self.v, self.k_scale, self.v_scale
            s.length = self.length[b:b + 1]
            s._parent, s._row, s._staged = self, self._row + int(b), None
            s._pos = [self._pos[b]]
            s.len_bound = None
            s.workspace = self.workspace
            return s
        s.k = [t[b:b + 1] for t in self.k]
        s.v = [t[b:b + 1] for t in self.v]
        s.k_scale = [None if t is None else t[b:b + 1] for t in self.k_scale]
        s.v_scale = [None if t is None else t[b:b + 1] for t in self.v_scale]
        s.length = self.length[b:b + 1]
        s._parent, s._row, s._staged = self, int(b), None
        s._pos = self._pos[b]
        s.len_bound = None
        s.workspace = self.workspace
        return s

    def _position_bytes(self) -> int:
        """K, V and scale bytes of one cached position of one batch row, over every layer."""
        row = self.head_dim + 4 if self.kv_dtype == "fp8" else 2 * self.head_dim
        return self.num_layers * self.n_head * row * 2

    def live_bytes(self) -> int:
        """K, V and scale bytes of the live rows only: the cached positions below each row's
        length (by the host mirrors), over every layer."""
        held = (sum(p for p in self._pos if p > 0) if self.per_sequence
                else self.batch * max(self._pos, 0))
        return held * self._position_bytes()

    @property
    def nbytes(self) -> int:
        """Bytes of K and V over every layer (codes and scales for the FP8 cache)."""
        return sum(t.numel() * t.element_size()
                   for t in self.k + self.v + self.k_scale + self.v_scale if t is not None)


def hip_supported(qkv: torch.Tensor, n_head: int, k_cache: torch.Tensor,
                  v_cache: torch.Tensor, k_scale: Optional[torch.Tensor] = None,
                  v_scale: Optional[torch.Tensor] = None) -> bool:
    if qkv.dim() != 3 or qkv.dtype != torch.bfloat16 or not qkv.is_contiguous():
        return False
    C = qkv.shape[2] // 3
    if qkv.shape[2] % 3 or C % n_head or C // n_head not in HEAD_DIMS:
        return False
    shape = (qkv.shape[0], n_head, k_cache.shape[2] if k_cache.dim() == 4 else -1, C // n_head)
    if k_scale is not None or v_scale is not None:
        return (all(t.dtype == E4M3 and t.is_contiguous() and tuple(t.shape) == shape
                    for t in (k_cache, v_cache))
                and all(t is not None and t.dtype == torch.float32 and t.is_contiguous()
                        and tuple(t.shape) == shape[:3] for t in (k_scale, v_scale)))
    return all(t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == shape
               for t in (k_cache, v_cache))


def _host_pos(length: torch.Tensor, pos: Optional[int]) -> int:
    return int(length.item()) if pos is None else int(pos)


def _check_fp8_cache(k_cache, v_cache, k_scale, v_scale) -> bool:
    """True for the FP8 cache (both scales given), False for bf16 (neither); raises on a mix."""
    if k_scale is None and v_scale is None:
        if k_cache.dtype == E4M3 or v_cache.dtype == E4M3:
            raise ValueError("an e4m3 KV cache needs its k_scale / v_scale")
        return False
    if k_scale is None or v_scale is None:
        raise ValueError("k_scale and v_scale go together")
    if k_cache.dtype != E4M3 or v_cache.dtype != E4M3:
        raise ValueError(f"k_scale / v_scale go with an e4m3 KV cache, got {k_cache.dtype} / "
                         f"{v_cache.dtype}")
    if k_scale.dtype != torch.float32 or v_scale.dtype != torch.float32 \
            or tuple(k_scale.shape) != tuple(k_cache.shape[:3]) \
            or tuple(v_scale.shape) != tuple(v_cache.shape[:3]):
        raise ValueError("k_scale / v_scale must be fp32 [B, H, L_max]")
    return True


def torch_kv_append(qkv, n_head: int, k_cache, v_cache, pos: int, k_scale=None,
                    v_scale=None) -> None:
    """Torch form of :func:`kv_append` at the host position ``pos``."""
    T = qkv.shape[1]
    _, k, v = _views(qkv, n_head)
    if k_scale is None:
        k_cache[:, :, pos:pos + T] = k
        v_cache[:, :, pos:pos + T] = v
        return
    for rows, cache, scale in ((k, k_cache, k_scale), (v, v_cache, v_scale)):
        code, s = _quantize_torch(rows)
        cache.view(torch.uint8)[:, :, pos:pos + T] = code.view(torch.uint8)
        scale[:, :, pos:pos + T] = s


def dequantize(cache: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 rows of an FP8 cache (or a slice of one): ``float(code) * scale``."""
    return cache.float() * scale[..., None]


def torch_decode_attention(qkv, n_head: int, k_cache, v_cache, pos: int, k_scale=None,
                           v_scale=None) -> torch.Tensor:
    """Torch form of :func:`decode_attention` at the host position ``pos`` (not replayable
    across positions: the slice bound is a host value)."""
    B, _, C3 = qkv.shape
    torch_kv_append(qkv, n_head, k_cache, v_cache, pos, k_scale, v_scale)
    q, _, _ = _views(qkv, n_head)
    if k_scale is None:
        o = F.scaled_dot_product_attention(q, k_cache[:, :, :pos + 1], v_cache[:, :, :pos + 1])
    else:
        o = F.scaled_dot_product_attention(
            q.float(), dequantize(k_cache[:, :, :pos + 1], k_scale[:, :, :pos + 1]),
            dequantize(v_cache[:, :, :pos + 1], v_scale[:, :, :pos + 1])).to(qkv.dtype)
    return o.transpose(1, 2).reshape(B, 1, C3 // 3)


def _per_sequence(length: torch.Tensor, batch: int, what: str) -> bool:
    """The dispatch on ``length.numel()``: 1 = the shared length, ``B`` = one per batch row."""
    n = length.numel()
    if n == 1:
        return False
    if n != batch:
        raise ValueError(f"{what}: length has {n} elements, need 1 (shared) or the batch "
                         f"size {batch} (per sequence)")
    return True


def _host_positions(length: torch.Tensor, pos) -> List[int]:
    """The ``B`` host positions of the per-sequence path (from the device when ``pos`` is None)."""
    p = length.tolist() if pos is None else [int(v) for v in pos]
    if len(p) != length.numel():
        raise ValueError(f"pos has {len(p)} entries for a length of {length.numel()}")
    return p


def torch_kv_append_seq(qkv, n_head: int, k_cache, v_cache, pos: Sequence[int], k_scale=None,
                        v_scale=None) -> None:
    """Torch form of the per-sequence :func:`kv_append`: row ``b`` is copied at the host position
    ``pos[b]``; nothing for an empty slot (``pos[b] < 0``)."""
    for b, p in enumerate(pos):
        if p < 0:
            continue
        torch_kv_append(qkv[b:b + 1], n_head, k_cache[b:b + 1], v_cache[b:b + 1], p,
                        None if k_scale is None else k_scale[b:b + 1],
                        None if v_scale is None else v_scale[b:b + 1])


def torch_decode_attention_seq(qkv, n_head: int, k_cache, v_cache, pos: Sequence[int],
                               k_scale=None, v_scale=None) -> torch.Tensor:
    """Torch form of the per-sequence :func:`decode_attention` at the host positions ``pos``:
    row ``b`` is :func:`torch_decode_attention` on the batch-1 slice of its cache at ``pos[b]``,
    so a row has the bits of the shared-length form; empty slots give zero rows. (One SDPA over
    the batch with a boolean key mask was tried first: with a mask torch's CPU kernel rounds the
    scaled scores differently, and a bf16 row differed from the shared-length form by an ulp.)"""
    B, _, C3 = qkv.shape
    out = torch.zeros(B, 1, C3 // 3, dtype=qkv.dtype, device=qkv.device)
    for b, p in enumerate(pos):
        if p < 0:
            continue
        out[b:b + 1] = torch_decode_attention(
            qkv[b:b + 1], n_head, k_cache[b:b + 1], v_cache[b:b + 1], p,
            None if k_scale is None else k_scale[b:b + 1],
            None if v_scale is None else v_scale[b:b + 1])
    return out


def _hip_append(qkv, n_head: int, k_cache, v_cache, k_scale, v_scale, length, T: int) -> None:
    """The HIP append of ``T`` tokens; the FP8 entry point when the cache has scales, the
    ``_seq`` one when ``length`` has an element per batch row."""
    B, _, C3 = qkv.shape
    fp8 = k_scale is not None
    scales = (k_scale.data_ptr(), v_scale.data_ptr()) if fp8 else ()
    name = ("dlbb_kv_append_fp8" if fp8 else "dlbb_kv_append") + \
        ("_seq" if length.numel() != 1 else "")
    fn = getattr(_lib.lib(), name)
    check(fn(qkv.data_ptr(), C3, k_cache.data_ptr(), v_cache.data_ptr(), *scales,
             length.data_ptr(), B, T, n_head, C3 // 3 // n_head, k_cache.shape[2],
             _lib.stream(qkv.device)), name[5:])


def _hip_decode(qkv, n_head: int, k_cache, v_cache, k_scale, v_scale, length, workspace, out,
                bound: int, chunk: int, fused: bool) -> None:
    """The HIP split + combine launches; the FP8 entry point when the cache has scales, the
    ``_seq`` one when ``length`` has an element per batch row."""
    B, _, C3 = qkv.shape
    C = C3 // 3
    D = C // n_head
    fp8 = k_scale is not None
    scales = (k_scale.data_ptr(), v_scale.data_ptr()) if fp8 else ()
    name = ("dlbb_attn_decode_fp8" if fp8 else "dlbb_attn_decode") + \
        ("_seq" if length.numel() != 1 else "")
    fn = getattr(_lib.lib(), name)
    check(fn(qkv.data_ptr(), C3, k_cache.data_ptr(), v_cache.data_ptr(), *scales,
             length.data_ptr(), workspace.data_ptr(), out.data_ptr(), C, B, n_head, D,
             k_cache.shape[2], bound, chunk, int(fused), 1.0 / math.sqrt(D),
             _lib.stream(qkv.device)), name[5:])


class _Paged:
    """The geometry of one paged call, checked: pools ``[n_pages, H, P, D]``, ``block_table``
    ``int32[B, max_pages]`` on the pools' device, ``length`` ``int32[B]``, ``L_max`` the logical
    cap (default: what the table covers)."""

    def __init__(self, what: str, qkv, k_pool, v_pool, length, block_table, table_host, max_len):
        B = qkv.shape[0]
        if k_pool.dim() != 4 or k_pool.shape != v_pool.shape:
            raise ValueError(f"{what}: the pools must be [n_pages, H, P, D], got "
                             f"{tuple(k_pool.shape)} / {tuple(v_pool.shape)}")
        self.n_pages, self.P = int(k_pool.shape[0]), check_page_size(k_pool.shape[2])
        if block_table.dim() != 2 or block_table.dtype != torch.int32 \
                or block_table.shape[0] != B or block_table.device != k_pool.device \
                or (block_table.shape[1] > 1 and block_table.stride(1) != 1):
            raise ValueError(f"{what}: block_table must be int32 [{B}, max_pages] on the pools' "
                             f"device, rows contiguous")
        if length.numel() != B:
            raise ValueError(f"{what}: a paged cache takes the per-sequence length int32[{B}], "
                             f"got {length.numel()} elements")
        self.max_pages = int(block_table.shape[1])
        self.L_max = self.max_pages * self.P if max_len is None else int(max_len)
        if not 0 < self.L_max <= self.max_pages * self.P:
            raise ValueError(f"{what}: max_len {self.L_max} outside (0, {self.max_pages} pages "
                             f"of {self.P}]")
        self.table, self._host, self.what = block_table, table_host, what

    def host(self) -> List[List[int]]:
        """The table on the host: the mirror when given, else read from the device."""
        t = self.table if self._host is None else self._host
        rows = t.tolist() if isinstance(t, torch.Tensor) else [list(r) for r in t]
        if len(rows) != self.table.shape[0] or any(len(r) < self.max_pages for r in rows):
            raise ValueError(f"{self.what}: table_host does not have block_table's shape")
        return rows

    def mapped(self, page: int) -> bool:
        return 0 <= page < self.n_pages

    def check_mapped(self, pos: Sequence[int], tokens: Sequence[int]) -> None:
        """Raise unless every page holding a position in ``[0, pos[b] + tokens[b])`` (below the
        cap) of a live row is mapped on the host."""
        rows = self.host()
        for b, (p, t) in enumerate(zip(pos, tokens)):
            if p < 0:
                continue
            need = (min(p + t, self.L_max) + self.P - 1) // self.P
            bad = [j for j in range(need) if not self.mapped(rows[b][j])]
            if bad:
                raise ValueError(f"{self.what}: row {b} needs {need} pages for {p} + {t} "
                                 f"positions, pages {bad} of its block table are not mapped")

    def hip_ok(self, qkv, n_head: int, k_pool, v_pool, k_scale, v_scale) -> bool:
        if qkv.dim() != 3 or qkv.dtype != torch.bfloat16 or not qkv.is_contiguous():
            return False
        C = qkv.shape[2] // 3
        if qkv.shape[2] % 3 or C % n_head or C // n_head not in HEAD_DIMS:
            return False
        shape = (self.n_pages, n_head, self.P, C // n_head)
        dt = torch.bfloat16 if k_scale is None else E4M3
        ok = all(t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape
                 for t in (k_pool, v_pool))
        if k_scale is not None:
            ok = ok and all(t.dtype == torch.float32 and t.is_contiguous()
                            and tuple(t.shape) == shape[:3] for t in (k_scale, v_scale))
        return ok

    def args(self):
        """block_table, its row stride, n_pages, P: the paged entry points' extra arguments."""
        return (self.table.data_ptr(), self.table.stride(0), self.n_pages, self.P)


def _gather_pages(pool: torch.Tensor, pages: Sequence[int]) -> torch.Tensor:
    """``pool[pages]`` as one contiguous batch-1 cache ``[1, H, len(pages) * P, ...]``."""
    raw = pool.view(torch.uint8) if pool.dtype == E4M3 else pool
    g = raw[torch.as_tensor(list(pages), dtype=torch.long, device=pool.device)]
    g = g.transpose(0, 1)                                        # [H, n, P, ...]
    return g.reshape(1, g.shape[0], g.shape[1] * g.shape[2], *g.shape[3:]).view(pool.dtype)


def _scatter_page(pool: torch.Tensor, page: int, cache: torch.Tensor, j: int) -> None:
    """Page ``j`` of the gathered batch-1 ``cache`` back to ``pool[page]``."""
    P = pool.shape[2]
    src = cache[0, :, j * P:(j + 1) * P]
    if pool.dtype == E4M3:
        pool.view(torch.uint8)[page] = src.view(torch.uint8)
    else:
        pool[page] = src


def torch_kv_append_paged(qkv, n_head: int, k_pool, v_pool, table: Sequence[Sequence[int]],
                          pos: Sequence[int], k_scale=None, v_scale=None,
                          max_len: Optional[int] = None) -> None:
    """Torch form of the paged :func:`kv_append` at the host positions ``pos`` and the host
    table ``table``: per live row the pages of ``[0, pos + T)`` are gathered into a contiguous
    batch-1 cache, :func:`torch_kv_append` runs on it and the mapped pages it wrote are copied
    back; positions on unmapped pages (and at or past ``max_len``) are dropped."""
    n_pages, P = k_pool.shape[0], k_pool.shape[2]
    L_max = len(table[0]) * P if max_len is None else max_len
    for b, p in enumerate(pos):
        T = min(qkv.shape[1], L_max - p)
        if p < 0 or T <= 0:
            continue
        first, n = p // P, (p + T + P - 1) // P
        ids = [int(e) for e in table[b][:n]]
        ok = [0 <= e < n_pages for e in ids]
        pools = [t for t in (k_pool, v_pool, k_scale, v_scale) if t is not None]
        flat = [_gather_pages(t, [e if g else 0 for e, g in zip(ids, ok)]) for t in pools]
        torch_kv_append(qkv[b:b + 1, :T], n_head, flat[0], flat[1], p,
                        *(flat[2:] if k_scale is not None else (None, None)))
        for j in range(first, n):
            if ok[j]:
                for t, f in zip(pools, flat):
                    _scatter_page(t, ids[j], f, j)


def torch_decode_attention_paged(qkv, n_head: int, k_pool, v_pool, table: Sequence[Sequence[int]],
                                 pos: Sequence[int], k_scale=None, v_scale=None) -> torch.Tensor:
    """Torch form of the paged :func:`decode_attention`: row ``b`` is
    :func:`torch_decode_attention` at ``pos[b]`` on the contiguous batch-1 gather of its pages
    (bit-identical to the contiguous torch form), the page holding the token is copied back;
    empty slots give zero rows. Every page below ``pos[b] + 1`` must be mapped: this form cannot
    mask an unmapped page, it raises."""
    B, _, C3 = qkv.shape
    n_pages, P = k_pool.shape[0], k_pool.shape[2]
    out = torch.zeros(B, 1, C3 // 3, dtype=qkv.dtype, device=qkv.device)
    for b, p in enumerate(pos):
        if p < 0:
            continue
        ids = [int(e) for e in table[b][:p // P + 1]]
        if any(not 0 <= e < n_pages for e in ids):
            raise ValueError(f"decode_attention: row {b} at position {p} has unmapped pages "
                             f"{ids}")
        pools = [t for t in (k_pool, v_pool, k_scale, v_scale) if t is not None]
        flat = [_gather_pages(t, ids) for t in pools]
        out[b:b + 1] = torch_decode_attention(
            qkv[b:b + 1], n_head, flat[0], flat[1], p,
            *(flat[2:] if k_scale is not None else (None, None)))
        for t, f in zip(pools, flat):
            _scatter_page(t, ids[-1], f, len(ids) - 1)
    return out


def _kv_append_paged(qkv, n_head, k_pool, v_pool, length, pos, k_scale, v_scale, block_table,
                     table_host, max_len, n_keep) -> None:
    """:func:`kv_append` with a block table (module docstring, "Paged cache")."""
    g = _Paged("kv_append", qkv, k_pool, v_pool, length, block_table, table_host, max_len)
    T = qkv.shape[1]
    _check_fp8_cache(k_pool, v_pool, k_scale, v_scale)
    if pos is not None:
        pos = _host_positions(length, pos)
        if max(pos) + T > g.L_max:
            raise ValueError(f"kv_append: position {max(pos)} + {T} tokens > cache length "
                             f"{g.L_max}")
        keep = [T] * len(pos) if n_keep is None else [int(v) for v in n_keep]
        if len(keep) != len(pos) or any(not 0 <= v <= T for v in keep):
            raise ValueError(f"kv_append: n_keep {keep}: need {len(pos)} values in [0, {T}]")
        g.check_mapped(pos, keep)
    if use_hip(qkv) and g.hip_ok(qkv, n_head, k_pool, v_pool, k_scale, v_scale):
        B, _, C3 = qkv.shape
        fp8 = k_scale is not None
        scales = (k_scale.data_ptr(), v_scale.data_ptr()) if fp8 else ()
        name = "dlbb_kv_append_fp8_paged" if fp8 else "dlbb_kv_append_paged"
        fn = getattr(_lib.lib(), name)
        check(fn(qkv.data_ptr(), C3, k_pool.data_ptr(), v_pool.data_ptr(), *scales,
                 length.data_ptr(), *g.args(), B, T, n_head, C3 // 3 // n_head, g.L_max,
                 _lib.stream(qkv.device)), name[5:])
        return
    p = _host_positions(length, pos)
    if max(p) + T > g.L_max:
        raise ValueError(f"kv_append: position {max(p)} + {T} tokens > cache length {g.L_max}")
    torch_kv_append_paged(qkv, n_head, k_pool, v_pool, g.host(), p, k_scale, v_scale, g.L_max)


def _decode_attention_paged(qkv, n_head, k_pool, v_pool, length, len_bound, workspace, pos, chunk,
                            fused, k_scale, v_scale, block_table, table_host, max_len):
    """:func:`decode_attention` with a block table (module docstring, "Paged cache")."""
    g = _Paged("decode_attention", qkv, k_pool, v_pool, length, block_table, table_host, max_len)
    L_max = g.L_max
    fp8 = _check_fp8_cache(k_pool, v_pool, k_scale, v_scale)
    chunk = int(chunk or (CHUNK_FP8 if fp8 else CHUNK))
    check_page_size(g.P, chunk)
    host = None
    if pos is not None:
        host = _host_positions(length, pos)
        if max(host) + 1 > L_max:
            raise ValueError(f"decode_attention: position {max(host)} + 1 > cache length {L_max}")
        g.check_mapped(host, [1] * len(host))
    if use_hip(qkv) and g.hip_ok(qkv, n_head, k_pool, v_pool, k_scale, v_scale):
        B, _, C3 = qkv.shape
        C = C3 // 3
        D = C // n_head
        fused = FUSED_APPEND if fused is None else bool(fused)
        bound = L_max if len_bound is None else max(1, min(int(len_bound), L_max))
        if host is not None and max(host) + 1 > bound:
            raise ValueError(f"decode_attention: position {max(host)} + 1 > len_bound {bound}")
        need = workspace_numel(B, n_head, D, bound, chunk)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.float32, device=qkv.device)
        elif workspace.numel() < need or workspace.dtype != torch.float32:
            raise ValueError(f"decode_attention: workspace of {workspace.numel()} fp32 < {need}")
        out = torch.empty(B, 1, C, dtype=qkv.dtype, device=qkv.device)
        scales = (k_scale.data_ptr(), v_scale.data_ptr()) if fp8 else ()
        lib = _lib.lib()
        if not fused:
            name = "dlbb_kv_append_fp8_paged" if fp8 else "dlbb_kv_append_paged"
            check(getattr(lib, name)(qkv.data_ptr(), C3, k_pool.data_ptr(), v_pool.data_ptr(),
                                     *scales, length.data_ptr(), *g.args(), B, 1, n_head, D,
                                     L_max, _lib.stream(qkv.device)), name[5:])
        name = "dlbb_attn_decode_fp8_paged" if fp8 else "dlbb_attn_decode_paged"
        check(getattr(lib, name)(qkv.data_ptr(), C3, k_pool.data_ptr(), v_pool.data_ptr(),
                                 *scales, length.data_ptr(), *g.args(), workspace.data_ptr(),
                                 out.data_ptr(), C, B, n_head, D, L_max, bound, chunk,
                                 int(fused), 1.0 / math.sqrt(D), _lib.stream(qkv.device)),
              name[5:])
        return out
    host = _host_positions(length, None) if host is None else host
    if max(host) + 1 > L_max:
        raise ValueError(f"decode_attention: position {max(host)} + 1 > cache length {L_max}")
    return torch_decode_attention_paged(qkv, n_head, k_pool, v_pool, g.host(), host, k_scale,
                                        v_scale)


def kv_append(qkv: torch.Tensor, n_head: int, k_cache: torch.Tensor, v_cache: torch.Tensor,
              length: torch.Tensor, pos: Union[None, int, Sequence[int]] = None,
              k_scale: Optional[torch.Tensor] = None,
              v_scale: Optional[torch.Tensor] = None,
              block_table: Optional[torch.Tensor] = None, table_host=None,
              max_len: Optional[int] = None, n_keep: Optional[Sequence[int]] = None) -> None:
    """K / V rows of ``qkv [B, T, 3C]`` -> cache positions ``[length, length + T)``. ``pos``:
    the host's copy of ``length`` (raises before launch on overflow; None on the HIP path = no
    host check, the kernel drops positions past the cache). ``k_scale`` / ``v_scale``: the row
    scales of an FP8 cache (module docstring), whose rows are quantised on the way in. A
    ``length`` of ``B`` elements is the per-sequence form (module docstring): row ``b`` goes to
    ``[length[b], length[b] + T)``, ``pos`` is then a sequence of ``B`` host positions.

    ``block_table`` (None = the contiguous caches): the paged form (module docstring); the caches
    are then the pools, ``max_len`` the logical cap (default ``max_pages * P``) and
    ``table_host`` the host mirror of the table that the ``pos`` check reads (default: the device
    table). ``n_keep``: per row, how many of the ``T`` tokens must land on mapped pages (default
    ``T``; the padded prefill passes its ``prompt_lens``, the padding past them may be dropped)."""
    if block_table is not None:
        return _kv_append_paged(qkv, n_head, k_cache, v_cache, length, pos, k_scale, v_scale,
                                block_table, table_host, max_len, n_keep)
    T, L_max = qkv.shape[1], k_cache.shape[2]
    if _per_sequence(length, qkv.shape[0], "kv_append"):
        if pos is not None:
            pos = _host_positions(length, pos)
            if max(pos) + T > L_max:
                raise ValueError(f"kv_append: position {max(pos)} + {T} tokens > cache length "
                                 f"{L_max}")
        _check_fp8_cache(k_cache, v_cache, k_scale, v_scale)
        if use_hip(qkv) and hip_supported(qkv, n_head, k_cache, v_cache, k_scale, v_scale):
            _hip_append(qkv, n_head, k_cache, v_cache, k_scale, v_scale, length, T)
            return
        p = _host_positions(length, pos)
        if max(p) + T > L_max:
            raise ValueError(f"kv_append: position {max(p)} + {T} tokens > cache length {L_max}")
        torch_kv_append_seq(qkv, n_head, k_cache, v_cache, p, k_scale, v_scale)
        return
    if pos is not None and pos + T > L_max:
        raise ValueError(f"kv_append: position {pos} + {T} tokens > cache length {L_max}")
    _check_fp8_cache(k_cache, v_cache, k_scale, v_scale)
    if use_hip(qkv) and hip_supported(qkv, n_head, k_cache, v_cache, k_scale, v_scale):
        _hip_append(qkv, n_head, k_cache, v_cache, k_scale, v_scale, length, T)
        return
    p = _host_pos(length, pos)
    if p + T > L_max:
        raise ValueError(f"kv_append: position {p} + {T} tokens > cache length {L_max}")
    torch_kv_append(qkv, n_head, k_cache, v_cache, p, k_scale, v_scale)


def decode_attention(qkv: torch.Tensor, n_head: int, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, length: torch.Tensor,
                     len_bound: Optional[int] = None, workspace: Optional[torch.Tensor] = None,
                     pos: Union[None, int, Sequence[int]] = None, chunk: Optional[int] = None,
                     fused: Optional[bool] = None, k_scale: Optional[torch.Tensor] = None,
                     v_scale: Optional[torch.Tensor] = None,
                     block_table: Optional[torch.Tensor] = None, table_host=None,
                     max_len: Optional[int] = None) -> torch.Tensor:
    """One decode step of causal attention: ``qkv [B, 1, 3C]`` -> ``[B, 1, C]``; the token's
    K / V are stored at cache position ``length`` and the query attends over ``length + 1``
    keys. ``length`` is not advanced.

    ``len_bound``: host upper bound of ``length + 1`` that sizes the split grid (default: the
    cache length); chunks past the device length exit at once, so one captured launch serves
    every position below the bound. ``workspace``: the cache's fp32 partials buffer
    (:func:`workspace_numel`; allocated per call when None). ``pos``: the host's copy of
    ``length`` for the overflow check (and the torch path). ``chunk`` / ``fused``: A/B knobs of
    ``tools/decode_bench.py`` (defaults :data:`CHUNK`, :data:`FUSED_APPEND`). ``k_scale`` /
    ``v_scale``: the row scales of an FP8 cache (module docstring): the token is stored
    quantised and attended to in that form; the chunk default is then :data:`CHUNK_FP8`.

    A ``length`` of ``B`` elements is the per-sequence form (module docstring): row ``b`` attends
    over ``length[b] + 1`` keys, an empty slot (``length[b] < 0``) gives a zero row; ``len_bound``
    bounds ``max_b length[b] + 1`` and ``pos`` is a sequence of ``B`` host positions.

    ``block_table`` (None = the contiguous caches): the paged form (module docstring); the caches
    are then the pools, ``max_len`` the logical cap (default ``max_pages * P``) and
    ``table_host`` the host mirror of the table for the ``pos`` check."""
    if qkv.dim() != 3 or qkv.shape[1] != 1:
        raise ValueError(f"decode_attention takes qkv [B, 1, 3C], got {tuple(qkv.shape)}")
    if block_table is not None:
        return _decode_attention_paged(qkv, n_head, k_cache, v_cache, length, len_bound,
                                       workspace, pos, chunk, fused, k_scale, v_scale,
                                       block_table, table_host, max_len)
    L_max = k_cache.shape[2]
    seq = _per_sequence(length, qkv.shape[0], "decode_attention")
    if seq and pos is not None:
        host = _host_positions(length, pos)
        pos = max(host)                          # the longest row: what the checks below bound
    if pos is not None and pos + 1 > L_max:
        raise ValueError(f"decode_attention: position {pos} + 1 > cache length {L_max}")
    fp8 = _check_fp8_cache(k_cache, v_cache, k_scale, v_scale)
    if use_hip(qkv) and hip_supported(qkv, n_head, k_cache, v_cache, k_scale, v_scale):
        B, _, C3 = qkv.shape
        C = C3 // 3
        D = C // n_head
        chunk = int(chunk or (CHUNK_FP8 if fp8 else CHUNK))
        fused = FUSED_APPEND if fused is None else bool(fused)
        bound = L_max if len_bound is None else max(1, min(int(len_bound), L_max))
        if pos is not None and pos + 1 > bound:
            raise ValueError(f"decode_attention: position {pos} + 1 > len_bound {bound}")
        need = workspace_numel(B, n_head, D, bound, chunk)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.float32, device=qkv.device)
        elif workspace.numel() < need or workspace.dtype != torch.float32:
            raise ValueError(f"decode_attention: workspace of {workspace.numel()} fp32 < {need}")
        out = torch.empty(B, 1, C, dtype=qkv.dtype, device=qkv.device)
        if not fused:
            _hip_append(qkv, n_head, k_cache, v_cache, k_scale, v_scale, length, 1)
        _hip_decode(qkv, n_head, k_cache, v_cache, k_scale, v_scale, length, workspace, out,
                    bound, chunk, fused)
        return out
    if seq:
        host = _host_positions(length, None) if pos is None else host
        if max(host) + 1 > L_max:
            raise ValueError(f"decode_attention: position {max(host)} + 1 > cache length {L_max}")
        return torch_decode_attention_seq(qkv, n_head, k_cache, v_cache, host, k_scale, v_scale)
    p = _host_pos(length, pos)
    if p + 1 > L_max:
        raise ValueError(f"decode_attention: position {p} + 1 > cache length {L_max}")
    return torch_decode_attention(qkv, n_head, k_cache, v_cache, p, k_scale, v_scale)
