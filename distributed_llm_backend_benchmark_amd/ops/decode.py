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
# append + attend in one launch (the chunk owning position `length` takes the token's K / V from
# qkv and stores them) instead of a kv_append launch before the attention
FUSED_APPEND = True


def workspace_numel(batch: int, n_head: int, head_dim: int, max_len: int,
                    chunk: int = CHUNK) -> int:
    """fp32 elements of the split kernel's partials: ``[B, H, n_chunks, D + 2]``."""
    return batch * n_head * ((max_len + chunk - 1) // chunk) * (head_dim + 2)


class KVCache:
    """K / V of every layer of one rank, the shared device ``length``, and the split kernel's
    workspace. ``num_layers = 0`` holds no K / V (the stateless ``attention="slice"`` stub):
    only the position bookkeeping. ``kv_dtype="fp8"``: ``k`` / ``v`` hold e4m3 codes and
    ``k_scale`` / ``v_scale`` one fp32 scale per cached row (module docstring); with ``"bf16"``
    the two scale lists hold ``None`` per layer.

    ``per_sequence=True``: ``length`` is ``int32[B]`` and ``pos`` a list of ``B`` host mirrors, one
    per batch row; a negative entry is an empty slot (module docstring). :meth:`set_lengths`,
    :meth:`retire`, :meth:`slot` and :meth:`live_bytes` belong to that form; :meth:`advance` moves
    the live rows only."""

    def __init__(self, num_layers: int, batch: int, n_head_local: int, head_dim: int,
                 max_len: int, device, dtype=torch.bfloat16, kv_dtype: str = "bf16",
                 per_sequence: bool = False):
        if max_len < 1 or batch < 1:
            raise ValueError(f"KVCache needs batch >= 1 and max_len >= 1, got {batch}, {max_len}")
        if kv_dtype not in KV_DTYPES:
            raise ValueError(f"KVCache kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
        self.kv_dtype = kv_dtype
        self.per_sequence = bool(per_sequence)
        self._parent, self._row = None, 0       # set on a slot view (:meth:`slot`)
        self._staged = None                     # (values, device tensor) of :meth:`set_lengths`
        fp8 = kv_dtype == "fp8"
        if fp8:
            dtype = E4M3
        self.num_layers, self.batch = int(num_layers), int(batch)
        self.n_head, self.head_dim, self.max_len = int(n_head_local), int(head_dim), int(max_len)
        self.device = torch.device(device)
        shape = (self.batch, self.n_head, self.max_len, self.head_dim)
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
            self._parent._pos[self._row] = int(value)

    def set_length(self, n: int) -> None:
        """Set the device length and the host mirror (0 = empty the cache); with
        ``per_sequence`` every row gets ``n``."""
        if not 0 <= n <= self.max_len:
            raise ValueError(f"KVCache length {n} outside [0, {self.max_len}]")
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
        if self._staged is None or self._staged[0] != vals:
            self._staged = (vals, torch.tensor(vals, dtype=torch.int32, device=self.device))
        self.length.copy_(self._staged[1])
        self.pos = vals

    def retire(self, b: int) -> None:
        """Row ``b`` holds no sequence any more: ``length[b] = -1``."""
        self._need_per_sequence("retire")
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
        with ``set_length(0)`` first."""
        self._need_per_sequence("slot")
        if not 0 <= b < self.batch:
            raise ValueError(f"KVCache.slot({b}): batch is {self.batch}")
        s = object.__new__(KVCache)
        s.kv_dtype, s.per_sequence = self.kv_dtype, False
        s.num_layers, s.batch = self.num_layers, 1
        s.n_head, s.head_dim, s.max_len = self.n_head, self.head_dim, self.max_len
        s.device = self.device
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


def kv_append(qkv: torch.Tensor, n_head: int, k_cache: torch.Tensor, v_cache: torch.Tensor,
              length: torch.Tensor, pos: Union[None, int, Sequence[int]] = None,
              k_scale: Optional[torch.Tensor] = None,
              v_scale: Optional[torch.Tensor] = None) -> None:
    """K / V rows of ``qkv [B, T, 3C]`` -> cache positions ``[length, length + T)``. ``pos``:
    the host's copy of ``length`` (raises before launch on overflow; None on the HIP path = no
    host check, the kernel drops positions past the cache). ``k_scale`` / ``v_scale``: the row
    scales of an FP8 cache (module docstring), whose rows are quantised on the way in. A
    ``length`` of ``B`` elements is the per-sequence form (module docstring): row ``b`` goes to
    ``[length[b], length[b] + T)``, ``pos`` is then a sequence of ``B`` host positions."""
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
                     v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
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
    bounds ``max_b length[b] + 1`` and ``pos`` is a sequence of ``B`` host positions."""
    if qkv.dim() != 3 or qkv.shape[1] != 1:
        raise ValueError(f"decode_attention takes qkv [B, 1, 3C], got {tuple(qkv.shape)}")
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
