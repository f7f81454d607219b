"""The per-sequence decode kernels (csrc/attn_decode.hip, the ``*_seq`` entry points): one launch
over a batch whose rows hold different numbers of cached tokens, against the shared-length kernel
on every row's own batch-1 slice (bit for bit: the work per ``(b, h, chunk, L)`` is the same) and
against an fp32 softmax; empty slots, a full row, writes outside the appended rows, ragged
appends, the device-side lengths, HIP-graph replay and determinism. bf16 and FP8 caches, head dims
64 and 128, fused and unfused append."""

import functools
import math

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.ops.decode import (CHUNK, CHUNK_FP8, decode_attention,
                                                              kv_append)
from distributed_llm_backend_benchmark_amd.ops.fp8 import E4M3, _quantize_torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
NAN_CODE = 0x7F                      # the e4m3fn NaN byte
U8, I32 = torch.uint8, torch.int32
H = 2
FMTS = ["bf16", "fp8"]


def _chunk(fmt):
    return CHUNK_FP8 if fmt == "fp8" else CHUNK


def _lengths(fmt, third=-1):
    """An empty slot, an empty sequence, the chunk edges and a row of several chunks."""
    c = _chunk(fmt)
    return [-1, 0, c + third, c, c + 1, 3 * c + 16]


def _quant(x):
    """``_quantize_torch`` of CPU rows -> (code bytes uint8, fp32 scales)."""
    code, scale = _quantize_torch(x)
    return code.view(U8), scale


class _Case:
    """Row ``b`` has ``lens[b]`` cached keys (none for an empty slot) in NaN-filled caches and a
    random token to decode. ``tensors``: K, V (and the two scale planes of an FP8 cache) on the
    device, never written: every run works on :meth:`fresh` copies."""

    def __init__(self, fmt, D, lens, L_max, seed):
        self.fmt, self.fp8, self.D, self.lens, self.L_max = fmt, fmt == "fp8", D, lens, L_max
        B = self.B = len(lens)
        g = torch.Generator().manual_seed(seed)
        self.q = torch.randn(B, H, D, generator=g).to(torch.bfloat16)
        tok = [torch.randn(B, H, D, generator=g).to(torch.bfloat16) for _ in range(2)]
        held = [min(max(n, 0), L_max) for n in lens]
        rows = [[torch.randn(H, n, D, generator=g).to(torch.bfloat16) for n in held]
                for _ in range(2)]
        if self.fp8:
            planes = [torch.full((B, H, L_max, D), NAN_CODE, dtype=U8) for _ in range(2)] + \
                     [torch.full((B, H, L_max), NAN, dtype=torch.float32) for _ in range(2)]
        else:
            planes = [torch.full((B, H, L_max, D), NAN, dtype=torch.bfloat16) for _ in range(2)]
        # fp32 K / V every row attends over, the token last (where it has a cache position), and
        # the cache after the step
        self.keys, after = [], [p.clone() for p in planes]
        for b, n in enumerate(held):
            kv = []
            for j in range(2):
                x = rows[j][b]
                if lens[b] >= 0 and lens[b] < L_max:
                    x = torch.cat([x, tok[j][b][:, None]], dim=1)
                if x.shape[1] == 0:
                    kv.append(x.float())
                elif self.fp8:
                    code, scale = _quant(x)
                    planes[j][b, :, :n], planes[2 + j][b, :, :n] = code[:, :n], scale[:, :n]
                    after[j][b, :, :x.shape[1]], after[2 + j][b, :, :x.shape[1]] = code, scale
                    kv.append(code.view(E4M3).float() * scale[..., None])
                else:
                    planes[j][b, :, :n] = x[:, :n]
                    after[j][b, :, :x.shape[1]] = x
                    kv.append(x.float())
            self.keys.append(kv)
        self.tensors = [p.to(DEV) for p in planes]
        self.after = [p.to(DEV) for p in after]
        self.qkv = torch.cat([t.reshape(B, 1, H * D) for t in (self.q, *tok)], dim=2).to(DEV)
        self.length = torch.tensor(lens, dtype=I32, device=DEV)

    def fresh(self):
        return [t.clone() for t in self.tensors]

    def run(self, tensors, length=None, qkv=None, **kw):
        """``decode_attention`` over the caches ``tensors`` (default: the case's lengths and
        tokens)."""
        k, v = (t.view(E4M3) if self.fp8 else t for t in tensors[:2])
        ks, vs = (tensors[2], tensors[3]) if self.fp8 else (None, None)
        return decode_attention(self.qkv if qkv is None else qkv, H, k, v,
                                self.length if length is None else length, k_scale=ks,
                                v_scale=vs, **kw)

    def want(self, b, extra=0):
        """fp32 softmax attention of row ``b`` over its keys, the token ``extra`` more times."""
        K, V = (torch.cat([t] + [t[:, -1:]] * extra, dim=1) for t in self.keys[b])
        s = (self.q[b].float()[:, None, :] * K).sum(-1) / math.sqrt(self.D)
        return (torch.softmax(s, dim=-1)[..., None] * V).sum(1)            # [H, D]

    def after_steps(self, steps):
        """The cache after ``steps`` steps with ``advance(1)`` between them: the token once more
        per step at the next position of every live row."""
        out = [t.clone() for t in self.after]
        for b, n in enumerate(self.lens):
            for t in out:
                if n >= 0:
                    t[b, :, n + 1:n + steps] = t[b, :, n:n + 1]
        return out


def _bits(t):
    return t.contiguous().view(U8)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _worst_ratio(case, got, rows, extra=0):
    """max over ``rows`` of max|got_b - want_b| / max|want_b|, printed per row."""
    worst = 0.0
    for b in rows:
        want = case.want(b, extra)
        g = got[b].view(H, case.D).float().cpu()
        assert torch.isfinite(g).all(), b
        ratio = float((g - want).abs().max() / want.abs().max())
        print(f"  row {b} (length {case.lens[b]} + {extra}): max|got-want|/max|want| = {ratio:.3e}")
        worst = max(worst, ratio)
    return worst


@functools.lru_cache(maxsize=None)
def _case(fmt, D):
    c = _chunk(fmt)
    return _Case(fmt, D, _lengths(fmt), 3 * c + 40, seed=1000 * D + (7 if fmt == "fp8" else 0))


@functools.lru_cache(maxsize=None)
def _ragged(fmt, D, fused):
    """ONE ragged launch (plus the append launch when unfused) -> (output, the caches after)."""
    case = _case(fmt, D)
    tensors = case.fresh()
    got = case.run(tensors, fused=fused)
    torch.cuda.synchronize()
    return got, tensors


ALL = pytest.mark.parametrize("fmt,D,fused", [(f, d, u) for f in FMTS for d in (64, 128)
                                              for u in (True, False)])


@ALL
def test_rows_have_the_bits_of_the_shared_length_kernel(fmt, D, fused):
    """The reference is the merged kernel: for every live row, ``decode_attention`` with a
    one-element ``length`` on a copy of the row's cache slice. Output row and cache row of the
    one ragged launch carry the same bits."""
    case = _case(fmt, D)
    got, tensors = _ragged(fmt, D, fused)
    for b, n in enumerate(case.lens):
        if n < 0:
            continue
        mine = [t[b:b + 1].clone() for t in case.tensors]
        one = torch.tensor([n], dtype=I32, device=DEV)
        want = case.run(mine, length=one, qkv=case.qkv[b:b + 1], fused=fused)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got[b:b + 1]), _bits(want)), f"output row {b} (length {n})"
        assert _same([t[b:b + 1] for t in tensors], mine), f"cache row {b} (length {n})"


@ALL
def test_rows_match_fp32(fmt, D, fused):
    """Bound 2^-7 max|want| per row, as in the shared-length tests: one bf16 rounding of the
    output is <= 2^-9 relative, fp32 reassociation is orders below. For the FP8 cache the
    reference is over the dequantised codes (``_quantize_torch``), so the bound is the same.
    Cache rows past every length hold NaN: a read past a row's live length would show."""
    case = _case(fmt, D)
    got, _ = _ragged(fmt, D, fused)
    print(f"ragged decode {fmt} D={D} fused={fused}:")
    ratio = _worst_ratio(case, got, [b for b, n in enumerate(case.lens) if n >= 0])
    assert ratio <= 2.0 ** -7, f"max|got - want| / max|want| = {ratio:.3e} > 2^-7"


@ALL
def test_empty_slot_and_nothing_else_written(fmt, D, fused):
    """Row 0 (length -1): output all zero bits, cache slice still all NaN. Every cache element
    outside ``(b, :, length[b], :)`` keeps its bits, the appended rows are the token's (for the
    FP8 cache ``_quantize_torch``'s codes and scales); ``length`` is not advanced."""
    case = _case(fmt, D)
    got, tensors = _ragged(fmt, D, fused)
    assert not _bits(got[0]).any()
    assert _same([t[0] for t in tensors], [t[0] for t in case.tensors])
    if case.fp8:
        assert (tensors[0][0] == NAN_CODE).all() and torch.isnan(tensors[2][0]).all()
    else:
        assert torch.isnan(tensors[0][0].float()).all() and torch.isnan(tensors[1][0].float()).all()
    for name, mine, want in zip(("k", "v", "k_scale", "v_scale"), tensors, case.after):
        assert torch.equal(_bits(mine), _bits(want)), name
    assert case.length.tolist() == case.lens


@ALL
def test_full_row_attends_every_key_and_writes_nothing(fmt, D, fused):
    """``length[b] = L_max``: the row attends the L_max cached keys and neither the fused chunk nor
    the append launch stores anything (the device guard, per row), beside an empty slot and a
    short row."""
    L_max = _chunk(fmt) + 40
    case = _Case(fmt, D, [-1, L_max, 5], L_max, seed=D + 3)
    tensors = case.fresh()
    got = case.run(tensors, fused=fused)
    torch.cuda.synchronize()
    assert _worst_ratio(case, got, [1, 2]) <= 2.0 ** -7
    assert not _bits(got[0]).any()
    assert _same(tensors, case.after)
    assert _same([t[:2] for t in tensors], [t[:2] for t in case.tensors])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("T", [1, 70])
@pytest.mark.parametrize("D", [64, 128])
def test_ragged_append_is_bit_exact_and_writes_nothing_else(fmt, D, T):
    """Caches (and scales) are views into larger sentinel-filled allocations. Rows: an empty slot,
    position 0, a mid position, the last ``T`` positions, and one whose tail falls past the cache
    (dropped on the device, per row). Everything outside ``[length[b], length[b] + T)`` keeps its
    bits, margins included; the appended rows are qkv's K / V bits (FP8: ``_quantize_torch``)."""
    L_max, margin = 300, 4096
    lens = [-1, 0, 131, L_max - T, L_max - T + 3 if T > 3 else L_max]
    B, fp8 = len(lens), fmt == "fp8"
    rows = B * H * L_max
    g = torch.Generator().manual_seed(D + T)
    qkv = torch.randn(B, T, 3, H, D, generator=g).to(torch.bfloat16)
    qkv[1, 0, 1, 0] = 0                                           # an all-zero K row
    if fp8:
        bigs = [torch.full((rows * D + 2 * margin,), s, dtype=U8, device=DEV)
                for s in (0x5A, 0xA5)] + \
               [torch.full((rows + 2 * margin,), s, dtype=torch.float32, device=DEV)
                for s in (-12345.0, 54321.0)]
        shapes = [(B, H, L_max, D)] * 2 + [(B, H, L_max)] * 2
    else:
        bigs = [torch.full((rows * D + 2 * margin,), s, dtype=torch.bfloat16, device=DEV)
                for s in (-12345.0, 54321.0)]
        shapes = [(B, H, L_max, D)] * 2

    def inner(big, shape):
        return big[margin:margin + math.prod(shape)].view(shape)

    want = [b.clone() for b in bigs]
    for j in range(2):
        x = qkv[:, :, 1 + j].permute(0, 2, 1, 3).contiguous()                # [B, H, T, D]
        code, scale = _quant(x) if fp8 else (x, None)
        for b, n in enumerate(lens):
            keep = min(T, L_max - n)                                         # the rest is dropped
            if n < 0 or keep <= 0:
                continue
            inner(want[j], shapes[j])[b, :, n:n + keep] = code[b, :, :keep].to(DEV)
            if fp8:
                inner(want[2 + j], shapes[2 + j])[b, :, n:n + keep] = scale[b, :, :keep].to(DEV)
    views = [inner(b, s) for b, s in zip(bigs, shapes)]
    k, v = (t.view(E4M3) if fp8 else t for t in views[:2])
    ks, vs = (views[2], views[3]) if fp8 else (None, None)
    length = torch.tensor(lens, dtype=I32, device=DEV)
    qkv = qkv.view(B, T, 3 * H * D).to(DEV)
    kv_append(qkv, H, k, v, length, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    for name, mine, w in zip(("k", "v", "k_scale", "v_scale"), bigs, want):
        assert torch.equal(_bits(mine), _bits(w)), name
    if fp8:
        assert float(views[2][1, 0, 0]) == 1.0 and not views[0][1, 0, 0].any()
    with pytest.raises(ValueError):                               # host check: the longest row
        kv_append(qkv, H, k, v, length, pos=[-1, 0, 0, 0, L_max - T + 1], k_scale=ks, v_scale=vs)


def _cache_of(case):
    """A per-sequence :class:`ops.KVCache` of one layer holding the case's caches and lengths."""
    c = ops.KVCache(1, case.B, H, case.D, case.L_max, DEV, kv_dtype=case.fmt, per_sequence=True)
    lists = (c.k, c.v, c.k_scale, c.v_scale)
    for dst, src in zip(lists, case.tensors):
        dst[0].view(src.dtype).copy_(src)
    c.set_lengths(case.lens)
    return c


def _step(case, c, **kw):
    return decode_attention(case.qkv, H, c.k[0], c.v[0], c.length, workspace=c.workspace,
                            k_scale=c.k_scale[0], v_scale=c.v_scale[0], **kw)


def _cache_tensors(c):
    return [t for t in (c.k[0], c.v[0], c.k_scale[0], c.v_scale[0]) if t is not None]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("D", [64, 128])
def test_lengths_are_read_on_the_device(fmt, D):
    """Same host arguments twice, ``advance(1)`` between the calls: row 2 goes from CHUNK - 1 to
    CHUNK cached tokens, so its second call attends CHUNK + 1 keys over two chunks. Each call
    matches fp32 at its own lengths (the token appended once more), the retired row stays -1."""
    case = _case(fmt, D)
    c = _cache_of(case)
    live = [b for b, n in enumerate(case.lens) if n >= 0]
    outs = []
    for _ in range(2):
        outs.append(_step(case, c).clone())
        c.advance(1)
    torch.cuda.synchronize()
    assert c.length.tolist() == [-1] + [n + 2 for n in case.lens[1:]] == c.pos
    for i, got in enumerate(outs):
        print(f"ragged decode {fmt} D={D}, call {i}:")
        assert _worst_ratio(case, got, live, extra=i) <= 2.0 ** -7, i
        assert not _bits(got[0]).any()
    assert _same(_cache_tensors(c), case.after_steps(2))
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("D", [64, 128])
def test_graph_replay_walks_the_ragged_positions(fmt, D):
    """One captured step + ``advance(1)``, replayed 5 times from ``[-1, 0, CHUNK - 2, ...]`` on
    fixed inputs (single stream, no forked branches, as the shared-length replay test captures):
    every replay equals the eager step at the same lengths bit for bit; row 2 crosses a chunk
    edge on the way; the empty slot stays empty."""
    c0, steps = _chunk(fmt), 5
    case = _Case(fmt, D, _lengths(fmt, third=-2), 3 * c0 + 40, seed=31 + D)
    eager_c, graph_c = _cache_of(case), _cache_of(case)
    eager = []
    for _ in range(steps):
        eager.append(_step(case, eager_c).clone())
        eager_c.advance(1)
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up: writes the same token rows
        _step(case, graph_c)
        graph_c.advance(1)
    torch.cuda.current_stream().wait_stream(side)
    graph_c.set_lengths(case.lens)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _step(case, graph_c)
        graph_c.advance(1)
    assert graph_c.length.tolist() == case.lens          # the capture ran nothing
    for i in range(steps):
        graph.replay()
        torch.cuda.synchronize()
        assert graph_c.length.tolist() == [-1] + [n + i + 1 for n in case.lens[1:]]
        assert torch.equal(_bits(out), _bits(eager[i])), f"replay {i}"
    assert _same(_cache_tensors(graph_c), _cache_tensors(eager_c))
    assert _same(_cache_tensors(graph_c), case.after_steps(steps))
    assert not torch.equal(_bits(eager[0]), _bits(eager[-1]))


@pytest.mark.parametrize("fmt", FMTS)
def test_two_runs_are_bit_identical(fmt):
    case = _case(fmt, 128)
    first, tensors = _ragged(fmt, 128, True)
    again = case.fresh()
    second = case.run(again)
    torch.cuda.synchronize()
    assert torch.equal(_bits(first), _bits(second))
    assert _same(tensors, again)


def test_length_numel_must_be_1_or_the_batch():
    case = _case("bf16", 64)
    tensors = case.fresh()
    for n in (2, case.B + 1):
        with pytest.raises(ValueError):
            case.run(tensors, length=torch.zeros(n, dtype=I32, device=DEV))
    assert _same(tensors, case.tensors)
