"""Tensor-parallel transformer (forward / inference benchmark model).

Reference ``models.py``: ``TransformerBlock`` (107-190), ``LLM`` (197-245), ``MODEL_CONFIGS``
(252-271), ``create_model`` (278-307), ``create_model_from_config`` (310-335).

Kept from the reference (workload parity): pre-LN blocks; column-parallel QKV computing all
``3H/P`` columns; the "attention" stub that keeps the first ``H/P`` columns (``models.py:162-167``)
— the GEMM reads that strided view directly (lda = 3H/P), no copy; row-parallel attention-out;
GELU (erf) MLP; 2 all-reduces per layer; final LayerNorm; ``randn`` weights (unscaled, as the
reference; ``init_std`` lets callers scale them).

MI355X-specific: all compute on-device in bf16 through the gfx950 kernels (MFMA GEMM with fused
GELU, fused residual+LayerNorm); the residual add of each sublayer is fused into the NEXT
LayerNorm, so the block is ``LN1 → QKV → out-proj → AR → (add+LN2) → up+GELU → down → AR →
(add+LN1 of the next block)``. ``attention="sdpa"`` swaps the stub for real causal attention
(torch SDPA), ``attention="flash"`` for our causal flash kernel (``ops.causal_attention``).
``overlap_chunks`` > 1 interleaves micro-batches so the all-reduces run under GEMMs (forward()).
``gemm_dtype="fp8"`` runs the four linears of every block through the FP8 GEMM (``ops.fp8``:
per-token activation scales, per-output-row weight scales); the default stays bf16.
``forward(x, kv_cache=...)`` is the autoregressive path: a prefill that fills a per-rank KV cache
(``LLM.new_kv_cache``), then one-token decode steps over it (``ops.decode_attention``).
``decode_weight_dtype="fp8"`` (opt-in) streams the e4m3 copy of every linear's weight in those
decode steps (``ops.w8_linear``, bf16 activations); prefill and cache-less forwards keep the bf16
weights. Both copies are resident: + 50 % weight memory.
``decode_weight_dtype="mxfp4"`` (opt-in) streams the MXFP4 copy instead (``ops.w4_linear``: e2m1
codes, one e8m0 scale per 32 k — K/2 + K/32 bytes per row). Both copies are resident here too:
+ 26.6 % weight memory.
``kv_cache_dtype="fp8"`` (opt-in) makes ``new_kv_cache`` hold e4m3 codes with one fp32 scale per
cached row (``ops.decode``): the appends quantise, a decode step attends to the quantised rows, the
prefill attention itself stays on the bf16 ``qkv``.
"""

from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..ops import gemm as gemm_ops
from ..parallel.comm import Comm
from ..parallel.streams import concurrent_stream
from ..parallel.tensor_parallel import (ColumnParallelLinear, RowParallelLinear,
                                        _check_decode_weight_dtype)

MODEL_CONFIGS: Dict[str, Dict[str, int]] = {
    "1B": {"hidden_size": 2048, "num_layers": 24, "num_heads": 16, "ffn_intermediate": 8192},
    "7B": {"hidden_size": 4096, "num_layers": 32, "num_heads": 32, "ffn_intermediate": 16384},
    "13B": {"hidden_size": 5120, "num_layers": 40, "num_heads": 40, "ffn_intermediate": 20480},
}


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class LayerNormParams(nn.Module):
    def __init__(self, hidden: int, device, dtype=torch.bfloat16):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden, device=device, dtype=dtype),
                                   requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(hidden, device=device, dtype=dtype),
                                 requires_grad=False)
        self.eps = 1e-5

    def forward(self, x, residual=None, kernels="hip"):
        if kernels == "torch":
            h = x + residual if residual is not None else x
            return F.layer_norm(h, (h.shape[-1],), self.weight, self.bias, self.eps), h
        y, h = ops.layernorm(x, self.weight, self.bias, self.eps, residual=residual)
        return y, (h if h is not None else x)


class TransformerBlock(nn.Module):
    def __init__(self, hidden_size: int, num_heads: int, ffn_intermediate: int, comm: Comm,
                 generator=None, init_std: float = 1.0, allreduce: str = "rccl",
                 allreduce_dtype: str = "bf16", attention: str = "slice",
                 kernels: str = "hip", gemm_dtype: str = "bf16",
                 decode_weight_dtype: str = "bf16"):
        super().__init__()
        P = comm.world_size
        self.hidden_size, self.num_heads, self.P = hidden_size, num_heads, P
        self.attention = attention
        self.kernels = kernels
        dev = comm.device
        self.ln1 = LayerNormParams(hidden_size, dev)
        self.qkv_proj = ColumnParallelLinear(hidden_size, 3 * hidden_size, comm,
                                             generator=generator, std=init_std, kernels=kernels,
                                             gemm_dtype=gemm_dtype,
                                             decode_weight_dtype=decode_weight_dtype)
        self.out_proj = RowParallelLinear(hidden_size, hidden_size, comm, generator=generator,
                                          std=init_std, allreduce=allreduce,
                                          allreduce_dtype=allreduce_dtype, kernels=kernels,
                                          gemm_dtype=gemm_dtype,
                                          decode_weight_dtype=decode_weight_dtype)
        self.ln2 = LayerNormParams(hidden_size, dev)
        self.ffn_up = ColumnParallelLinear(hidden_size, ffn_intermediate, comm,
                                           generator=generator, std=init_std, kernels=kernels,
                                           gemm_dtype=gemm_dtype,
                                           decode_weight_dtype=decode_weight_dtype)
        self.ffn_down = RowParallelLinear(ffn_intermediate, hidden_size, comm,
                                          generator=generator, std=init_std, allreduce=allreduce,
                                          allreduce_dtype=allreduce_dtype, kernels=kernels,
                                          gemm_dtype=gemm_dtype,
                                          decode_weight_dtype=decode_weight_dtype)

    def _attn(self, qkv: torch.Tensor, cache=None, layer: int = 0) -> torch.Tensor:
        hpr = self.hidden_size // self.P
        if self.attention == "slice":
            return qkv[..., :hpr]               # reference stub, models.py:166-167 (a view)
        B, S, _ = qkv.shape
        heads = self.num_heads // self.P
        hd = hpr // heads
        if cache is not None:
            return self._attn_cached(qkv, heads, cache, layer)
        if self.attention == "flash" and self.kernels != "torch":
            # our causal flash kernel (csrc/attention.hip, head dim 64 / 128) straight on the
            # rank's fused [B, S, 3, heads, hd] QKV shard — no unbind / transpose copies
            return ops.causal_attention(qkv, heads)
        q, k, v = qkv.view(B, S, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        return o.transpose(1, 2).reshape(B, S, hpr)

    def _attn_cached(self, qkv: torch.Tensor, heads: int, cache, layer: int) -> torch.Tensor:
        """Attention with a KV cache (:class:`ops.KVCache`): ``T > 1`` = prefill of an empty
        cache (causal attention over the prompt, K / V appended), ``T == 1`` = one decode step
        (the token's K / V stored at ``cache.length``, attention over ``length + 1`` keys).
        ``flash`` runs our kernels (``ops.causal_attention`` + ``ops.kv_append``,
        ``ops.decode_attention``); ``sdpa`` and ``kernels="torch"`` the torch forms at the host
        position. The cache is advanced by the model, not here. A per-sequence cache hands its
        ``int32[B]`` ``length`` and its list of host positions through the same calls: the ops
        dispatch on ``length.numel()``. A paged cache hands its pools, ``block_table`` and the
        table's host mirror through as well."""
        from ..ops import decode as dec

        k, v = cache.k[layer], cache.v[layer]
        # the row scales of an FP8 cache (None for bf16): handed through as they are
        ks, vs = cache.k_scale[layer], cache.v_scale[layer]
        hip = self.attention == "flash" and self.kernels != "torch"
        if cache.paged:
            table = dict(block_table=cache.block_table, table_host=cache.table_host,
                         max_len=cache.max_len)
            if qkv.shape[1] == 1:
                if hip:
                    return ops.decode_attention(qkv, heads, k, v, cache.length,
                                                len_bound=cache.len_bound,
                                                workspace=cache.workspace, pos=cache.pos,
                                                k_scale=ks, v_scale=vs, **table)
                return dec.torch_decode_attention_paged(qkv, heads, k, v,
                                                        cache.table_host.tolist(), cache.pos,
                                                        ks, vs)
            if hip:
                ops.kv_append(qkv, heads, k, v, cache.length, pos=cache.pos, k_scale=ks,
                              v_scale=vs, n_keep=cache.n_keep, **table)
                return ops.causal_attention(qkv, heads)
            dec.torch_kv_append_paged(qkv, heads, k, v, cache.table_host.tolist(), cache.pos,
                                      ks, vs, cache.max_len)
            return self._attn(qkv)
        if qkv.shape[1] == 1:
            if hip:
                return ops.decode_attention(qkv, heads, k, v, cache.length,
                                            len_bound=cache.len_bound,
                                            workspace=cache.workspace, pos=cache.pos,
                                            k_scale=ks, v_scale=vs)
            if cache.per_sequence:
                return dec.torch_decode_attention_seq(qkv, heads, k, v, cache.pos, ks, vs)
            return dec.torch_decode_attention(qkv, heads, k, v, cache.pos, ks, vs)
        if hip:
            ops.kv_append(qkv, heads, k, v, cache.length, pos=cache.pos, k_scale=ks, v_scale=vs)
            return ops.causal_attention(qkv, heads)
        if cache.per_sequence:
            dec.torch_kv_append_seq(qkv, heads, k, v, cache.pos, ks, vs)
        else:
            dec.torch_kv_append(qkv, heads, k, v, cache.pos, ks, vs)
        return self._attn(qkv)

    def forward(self, y1: torch.Tensor, h: torch.Tensor):
        """``y1`` = LN1(h) (computed by the caller's fused add+LN); returns (d, h) where the
        block output is ``h + d`` (added inside the next fused LayerNorm)."""
        gen = self.steps(y1, h)
        try:
            while True:
                next(gen)
        except StopIteration as e:
            return e.value

    def steps(self, y1: torch.Tensor, h: torch.Tensor, slot: int = 0, stream=None, cache=None,
              layer: int = 0):
        """The block as a generator that yields after launching each of its two all-reduces
        (the event to wait on before the all-reduced tensor is read; None when inline) —
        :meth:`LLM.forward` interleaves micro-batches on it. Returns ``(d, h)``. ``cache``: the
        KV cache this block appends to (as layer ``layer``) and decodes from. A one-token step
        over a cache is a decode step: its four linears are told so (``decode_weight_dtype``)."""
        decode = cache is not None and y1.shape[1] == 1
        qkv = self.qkv_proj(y1, decode=decode)
        a, ev = self.out_proj.launch(self._attn(qkv, cache, layer), slot, stream, decode=decode)
        yield ev
        y2, h = self.ln2(a, residual=h, kernels=self.kernels)          # h = h + attn_out
        u = self.ffn_up(y2, act="gelu", decode=decode)                  # GELU fused (erf)
        d, ev = self.ffn_down.launch(u, slot, stream, decode=decode)
        yield ev
        return d, h


class LLM(nn.Module):
    def __init__(self, hidden_size: int, num_layers: int, num_heads: int, ffn_intermediate: int,
                 comm: Comm, seed: int = 0, init_std: float = 1.0, allreduce: str = "rccl",
                 allreduce_dtype: str = "bf16", attention: str = "slice", kernels: str = "hip",
                 overlap_chunks: int = 1, gemm_dtype: str = "bf16",
                 decode_weight_dtype: str = "bf16", kv_cache_dtype: str = "bf16"):
        super().__init__()
        if kv_cache_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_cache_dtype must be bf16|fp8, got {kv_cache_dtype!r}")
        self.kv_cache_dtype = kv_cache_dtype
        self.gemm_dtype = gemm_dtype
        self.decode_weight_dtype = _check_decode_weight_dtype(decode_weight_dtype, gemm_dtype)
        self.attention = attention
        self.hidden_size, self.num_layers = hidden_size, num_layers
        # > 1: split the batch into this many micro-batches and interleave them so every
        # row-parallel all-reduce (on a side comm stream) runs under the next micro-batch's
        # GEMMs — see forward()
        self.overlap_chunks = max(1, int(overlap_chunks))
        # overlapped forward, A/B knob: each micro-batch on a compute stream of its own (so two
        # micro-batches' small per-rank GEMMs could share the chip) instead of one compute
        # stream. Measured worse (tools/diag/tp_overlap_probe.py, profiles/r03_tp): with three
        # busy streams the all-reduces stop overlapping at all (7B shard-8 at 300 GB/s: 25.0 vs
        # 18.0 ms), so the default is one compute stream + the comm stream.
        self.chunk_streams = False
        self._comm_stream = None
        self._chunk_streams = []
        self.num_heads, self.ffn_intermediate = num_heads, ffn_intermediate
        self.comm = comm
        self.world_size = comm.world_size
        self.kernels = kernels
        gen = torch.Generator(device=comm.device)
        gen.manual_seed(seed + 1000 * comm.rank)
        self.layers = nn.ModuleList([
            TransformerBlock(hidden_size, num_heads, ffn_intermediate, comm, gen, init_std,
                             allreduce, allreduce_dtype, attention, kernels, gemm_dtype,
                             decode_weight_dtype)
            for _ in range(num_layers)])
        self.ln_final = LayerNormParams(hidden_size, comm.device)

    @torch.inference_mode()
    def ipc_allreduce(self):
        """The IPC all-reduce instance the row-parallel layers may use (None: RCCL only)."""
        for m in self.modules():
            car = getattr(m, "_car", None)
            if car is not None:
                return car
        return None

    def new_kv_cache(self, batch: int, max_len: int, per_sequence: bool = False,
                     page_size: Optional[int] = None, n_pages: Optional[int] = None):
        """A :class:`ops.KVCache` for this rank's ``num_heads / P`` local heads, ``max_len``
        positions. ``attention="slice"`` (the stateless stub) gets one with no K / V storage:
        decode still runs, and measures the GEMMs and the ``[B, 1, H]`` all-reduces alone.
        With ``decode_weight_dtype="fp8"`` on the HIP path the batch is the M of the W8 skinny
        GEMM (``"mxfp4"``: of the W4 one): more than 16 rows raise here, not in the middle of a
        step. ``kv_cache_dtype`` picks the cache's storage (``"fp8"``: e4m3 codes + one fp32
        scale per row). ``per_sequence=True``: one length per batch row (``ops.decode``), for a
        batch whose sequences differ in length; see :meth:`forward`. ``page_size`` (with
        ``n_pages``, default: a page for every position of every row): a PAGED cache
        (``ops.decode``): one pool of ``n_pages`` pages of ``page_size`` positions per layer,
        shared by the rows through a block table; it is per-sequence."""
        if page_size is not None and self.attention == "slice":
            raise ValueError("a paged KV cache needs attention sdpa|flash: the slice stub keeps "
                             "no K / V")
        if (self.decode_weight_dtype != "bf16" and batch > 16 and self.kernels != "torch"
                and self.comm.device.type == "cuda" and not ops._lib.force_torch()):
            which = "W8" if self.decode_weight_dtype == "fp8" else "W4"
            raise ValueError(f"decode_weight_dtype={self.decode_weight_dtype!r}: batch {batch} "
                             f"is larger than the 16 rows of the {which} skinny GEMM; there is "
                             "no fall-back to bf16")
        heads = self.num_heads // self.world_size
        layers = 0 if self.attention == "slice" else self.num_layers
        return ops.KVCache(layers, batch, heads, self.hidden_size // self.num_heads, max_len,
                           self.comm.device, kv_dtype=self.kv_cache_dtype,
                           per_sequence=per_sequence, page_size=page_size, n_pages=n_pages)

    def _micro_batch(self, x: torch.Tensor, slot: int = 0, stream=None, cache=None):
        """One micro-batch's forward as a generator over its all-reduces (see
        :meth:`TransformerBlock.steps`); returns the final LayerNorm output."""
        if not self.layers:
            y, _ = self.ln_final(x, kernels=self.kernels)
            return y
        y, h = self.layers[0].ln1(x, kernels=self.kernels)
        for i, layer in enumerate(self.layers):
            d, h = yield from layer.steps(y, h, slot, stream, cache, i)
            nxt = self.layers[i + 1].ln1 if i + 1 < len(self.layers) else self.ln_final
            y, h = nxt(d, residual=h, kernels=self.kernels)
        return y

    def overlap_split(self, x: torch.Tensor) -> int:
        """Micro-batches the forward of ``x`` runs as: ``overlap_chunks`` when the batch splits
        evenly (and the model is TP over more than one rank), else 1."""
        n = self.overlap_chunks
        if n <= 1 or self.world_size <= 1 or x.shape[0] % n:
            return 1
        return n

    def forward(self, x: torch.Tensor, kv_cache=None, prompt_lens=None) -> torch.Tensor:
        """With ``kv_cache`` (:meth:`new_kv_cache`) and ``x [B, T, H]`` every block appends its
        K / V: ``T > 1`` on an empty cache is the prefill, ``T == 1`` a decode step over the
        cached tokens; ``T > 1`` on a non-empty cache raises ``ValueError`` (no chunked
        prefill). After the final LayerNorm the cache advances by ``T`` (a device add on the
        current stream, captured with the step). With a cache the forward runs as ONE
        micro-batch: ``overlap_chunks`` is ignored there.

        With a per-sequence cache (``new_kv_cache(..., per_sequence=True)``) ``T > 1`` is the
        prefill of a RIGHT-PADDED batch: every live row must be empty, all ``T`` rows are appended
        from position 0, the causal attention is the usual one (causality keeps every real
        token's output independent of the padding behind it) and the cache ends at
        ``set_lengths(prompt_lens)`` (default: ``T`` for every live row). The padding rows left
        in the cache lie at or past ``length[b]``: never read, overwritten as the sequence grows.
        ``T == 1`` is a decode step of the live rows, then ``advance(1)``; an empty slot's
        output row is not meaningful. A ``prompt_lens`` entry outside ``[1, T]`` raises before
        any launch, and so does ``prompt_lens`` on a shared-length cache. One slot of such a
        cache is refilled through ``kv_cache.slot(b)``, a batch-1 shared-length cache.

        With a paged cache (``new_kv_cache(..., page_size=P)``) the forward first reserves the
        pages its tokens need (``prompt_lens[b]`` positions per live row for the padded prefill,
        ``pos + T`` otherwise; a pool that cannot give them raises ``ValueError`` before any
        launch). The padded prefill still appends all ``T`` rows: padding that falls on unmapped
        pages is dropped on the device, padding inside the last mapped page lies past
        ``length[b]`` and is overwritten as the row grows. ``kv_cache.slot(b)`` is then a batch-1
        paged view.

        Without a cache — plain: one pass, each all-reduce inline. Overlapped (``overlap_chunks`` = n > 1): the
        batch is split into n micro-batches run round-robin, each advancing to its next
        all-reduce; the all-reduce goes to a side comm stream (normal priority: a high-priority one stretches
        every compute dispatch, profiles/r03_overlap) and the micro-batch resumes only after its compute
        stream waited for it. So all-reduce k of micro-batch A runs under the GEMMs of
        micro-batch B, and every rank issues its collectives in the same order on one comm
        stream. The reference blocks on each all-reduce (models.py:95)."""
        if kv_cache is not None:
            T = x.shape[1]
            if x.shape[0] != kv_cache.batch:
                raise ValueError(f"batch {x.shape[0]} != the cache's {kv_cache.batch}")
            if prompt_lens is not None:
                if not kv_cache.per_sequence:
                    raise ValueError("prompt_lens needs a per_sequence=True KV cache")
                prompt_lens = [int(v) for v in prompt_lens]
                if T == 1 or len(prompt_lens) != x.shape[0] \
                        or any(not 1 <= v <= T for v in prompt_lens):
                    raise ValueError(f"prompt_lens {prompt_lens}: need {x.shape[0]} values in "
                                     f"[1, {T}] with a prefill of T > 1 tokens")
            if T > 1 and (any(p > 0 for p in kv_cache.pos) if kv_cache.per_sequence
                          else kv_cache.pos != 0):
                raise ValueError(f"prefill of {T} tokens on a cache holding {kv_cache.pos}: "
                                 "chunked prefill is not supported")
            kv_cache.check_room(T)
            if kv_cache.paged:
                keep = prompt_lens if prompt_lens is not None else [T] * x.shape[0]
                kv_cache.reserve_all([min(max(p, 0) + n, kv_cache.max_len)
                                      for p, n in zip(kv_cache.pos, keep)])
                kv_cache.n_keep = prompt_lens
        n = 1 if kv_cache is not None else self.overlap_split(x)
        if n == 1:
            gen = self._micro_batch(x, cache=kv_cache)
            try:
                while True:
                    next(gen)
            except StopIteration as e:
                if kv_cache is not None:
                    kv_cache.n_keep = None
                    if prompt_lens is not None:
                        # empty slots stay empty: their rows of the padded batch are not kept
                        kv_cache.set_lengths([n if p >= 0 else -1
                                              for n, p in zip(prompt_lens, kv_cache.pos)])
                    else:
                        kv_cache.advance(x.shape[1])
                return e.value
        stream = None
        cur = torch.cuda.current_stream(x.device) if x.is_cuda else None
        work = [cur] * n                        # the stream each micro-batch computes on
        if x.is_cuda:
            if self._comm_stream is None:
                self._comm_stream = concurrent_stream(x.device, "tp_comm")
            stream = self._comm_stream
            # (not under HIP-graph capture: a capture forking the per-micro-batch streams crashed
            # the process on MI355X; the capture keeps one compute stream + the comm stream)
            if self.chunk_streams and not torch.cuda.is_current_stream_capturing():
                while len(self._chunk_streams) < n:
                    self._chunk_streams.append(
                        concurrent_stream(x.device, f"tp_chunk{len(self._chunk_streams)}"))
                work = self._chunk_streams[:n]
                for s in work:                  # fork: x (and last call's frees) are ready
                    s.wait_stream(cur)
        gens = [self._micro_batch(xc, slot, stream) for slot, xc in enumerate(x.chunk(n, 0))]
        pending = [None] * n
        outs = [None] * n
        live = n
        with gemm_ops.concurrent_comm():       # no persistent library GEMM beside comm kernels
            while live:
                for c in range(n):
                    if gens[c] is None:
                        continue
                    ctx = (torch.cuda.stream(work[c]) if x.is_cuda and work[c] is not cur
                           else _NullCtx())
                    with ctx:
                        if pending[c] is not None:
                            work[c].wait_event(pending[c])
                        try:
                            pending[c] = next(gens[c])
                        except StopIteration as e:
                            outs[c], gens[c], pending[c] = e.value, None, None
                            live -= 1
        if x.is_cuda:
            for s in work:                      # join
                if s is not cur:
                    cur.wait_stream(s)
        return torch.cat(outs, 0)

    @torch.no_grad()
    def load_from_dense(self, dense_state: Dict[str, torch.Tensor]) -> None:
        """Shard a world-1 model's state into this rank (Megatron layout): QKV rows are taken
        per projection (``q_r, k_r, v_r``) so the local shard is ``[q_r | k_r | v_r]`` and the
        reference's "first H/P columns" stub yields ``q_r``; FFN-up rows by block;
        row-parallel weights by column block. Used to test TP(P) == dense(1)."""
        P, r = self.world_size, self.comm.rank
        H = self.hidden_size
        for name, p in self.named_parameters():
            full = dense_state[name].to(p.device, p.dtype)
            if full.shape == p.shape:
                p.copy_(full)
            elif name.endswith("qkv_proj.weight"):
                hp = H // P
                p.copy_(torch.cat([full[j * H + r * hp: j * H + (r + 1) * hp] for j in range(3)]))
            elif name.endswith("ffn_up.weight"):
                n = p.shape[0]
                p.copy_(full[r * n:(r + 1) * n])
            elif name.endswith(("out_proj.weight", "ffn_down.weight")):
                k = p.shape[1]
                p.copy_(full[:, r * k:(r + 1) * k])
            else:
                raise KeyError(f"cannot shard {name}: {tuple(full.shape)} -> {tuple(p.shape)}")

    def get_num_parameters(self) -> int:
        """Reference formula (``models.py:240-241``): local numel × P (over-counts LN params)."""
        return sum(p.numel() for p in self.parameters()) * self.world_size

    def num_parameters_exact(self) -> int:
        local_ln = sum(p.numel() for n, p in self.named_parameters() if ".ln" in n or
                       n.startswith("ln_final"))
        local = sum(p.numel() for p in self.parameters())
        return (local - local_ln) * self.world_size + local_ln

    def get_memory_footprint(self) -> int:
        return sum(p.numel() * p.element_size() for p in self.parameters())

    def decode_weight_bytes(self) -> int:
        """Parameter bytes one decode step streams on this rank. ``decode_weight_dtype="fp8"``:
        every linear's N x K e4m3 bytes and its N fp32 row scales, plus the LayerNorm
        parameters; ``"mxfp4"``: every linear's N x K / 2 code bytes and N x K / 32 scale bytes,
        plus the LayerNorm parameters; ``"bf16"``: :meth:`get_memory_footprint`."""
        if self.decode_weight_dtype == "bf16":
            return self.get_memory_footprint()
        w4 = self.decode_weight_dtype == "mxfp4"
        total = 0
        for m in self.modules():
            if isinstance(m, (ColumnParallelLinear, RowParallelLinear)):
                n, k = m.weight.shape
                total += n * k // 2 + n * k // 32 if w4 else n * k + 4 * n
            elif isinstance(m, LayerNormParams):
                total += sum(p.numel() * p.element_size() for p in m.parameters())
        return total

    def comm_bytes(self) -> int:
        return sum(m.comm_bytes for m in self.modules() if isinstance(m, RowParallelLinear))

    def flops_per_forward(self, batch: int, seq: int) -> float:
        """GEMM FLOPs of one forward on ONE rank."""
        M = batch * seq
        H, F_, P = self.hidden_size, self.ffn_intermediate, self.world_size
        per_layer = 2 * M * H * (3 * H // P) + 2 * M * (H // P) * H \
            + 2 * M * H * (F_ // P) + 2 * M * (F_ // P) * H
        return float(per_layer * self.num_layers)


def create_model(model_size: str, comm: Comm, **kw) -> LLM:
    if model_size not in MODEL_CONFIGS:
        raise ValueError(f"Invalid model size: {model_size}. Choose from {list(MODEL_CONFIGS)}")
    return LLM(comm=comm, **MODEL_CONFIGS[model_size], **kw)


def create_model_from_config(config: Dict, comm: Comm) -> LLM:
    m = config["model"]
    ex = config.get("execution", {})
    allreduce = ex.get("allreduce", "auto")
    return LLM(hidden_size=int(m["hidden_size"]), num_layers=int(m["num_layers"]),
               num_heads=int(m["num_heads"]), ffn_intermediate=int(m["ffn_intermediate"]),
               comm=comm, seed=int(config.get("input", {}).get("seed", 42)),
               init_std=float(m.get("init_std", 1.0)),
               allreduce="rccl" if allreduce in ("torch",) else allreduce,
               allreduce_dtype=ex.get("allreduce_dtype", "bf16"),
               attention=ex.get("attention", "slice"), kernels=ex.get("kernels", "hip"),
               overlap_chunks=int(ex.get("overlap_chunks", 1)),
               gemm_dtype=ex.get("gemm_dtype", "bf16"),
               decode_weight_dtype=ex.get("decode_weight_dtype", "bf16"),
               kv_cache_dtype=ex.get("kv_cache_dtype", "bf16"))
