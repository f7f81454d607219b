"""The paged decode kernels (csrc/attn_decode.hip, the ``*_paged`` entry points): K / V in a page
pool shared by the batch rows, addressed through a block table. Against the contiguous
per-sequence kernels on the same contents (bit for bit: only the addresses differ) and against an
fp32 softmax; writes outside the token's rows, unmapped pages, the paged prefill append, HIP-graph
replay across a page edge, determinism, page reuse and the launcher's refusals. bf16 and FP8
caches, head dims 64 and 128, page sizes 16 (many table look-ups per chunk) and 256 (one).

Every pool is a slice out of the middle of a larger NaN-filled allocation with guard pages on both
sides, physical pages are handed out in a seeded shuffled order, and the only out-of-range table
entries used are -1 and ``n_pages``: a missed guard reads or writes memory the test owns and shows
as a failed assertion."""

import functools
import math

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.ops import _lib
from distributed_llm_backend_benchmark_amd.ops.decode import (CHUNK, CHUNK_FP8, decode_attention,
                                                              kv_append)
from distributed_llm_backend_benchmark_amd.ops.fp8 import E4M3, _quantize_torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
NAN_CODE = 0x7F                      # the e4m3fn NaN byte
U8, I32 = torch.uint8, torch.int32
H = 2
GUARD = 2                            # owned NaN-filled pages on each side of a pool
FMTS = ["bf16", "fp8"]
PAGES = [16, 256]


def _chunk(fmt):
    return CHUNK_FP8 if fmt == "fp8" else CHUNK


def _quant(x):
    code, scale = _quantize_torch(x)
    return code.view(U8), scale


def _bits(t):
    return t.contiguous().view(U8)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _nan_planes(fp8, lead, P_or_L, D):
    """K, V (and the two scale planes of an FP8 cache), NaN in every element, on the CPU."""
    if fp8:
        return [torch.full((*lead, P_or_L, D), NAN_CODE, dtype=U8) for _ in range(2)] + \
               [torch.full((*lead, P_or_L), NAN, dtype=torch.float32) for _ in range(2)]
    return [torch.full((*lead, P_or_L, D), NAN, dtype=torch.bfloat16) for _ in range(2)]


def _shuffled(n, seed):
    """A seeded order of ``range(n)`` in which no two consecutive entries are physical
    neighbours (the seed is advanced until that holds; fewer than 4 entries have no such order)."""
    while True:
        order = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
        if n < 4 or all(abs(a - b) != 1 for a, b in zip(order, order[1:])):
            return order
        seed += 1


def _typed(tensors, fp8):
    """The op's arguments of a list of planes: k, v (e4m3 views of the code bytes), scales."""
    k, v = (t.view(E4M3) if fp8 else t for t in tensors[:2])
    return k, v, dict(k_scale=tensors[2], v_scale=tensors[3]) if fp8 else {}


class _Case:
    """Row ``b`` holds ``lens[b]`` cached keys and decodes one random token, twice over: in
    contiguous per-sequence caches (``flat``) and in a page pool (``back``: the whole backing
    allocation, ``pool()`` the slice the op gets) through ``table``. Both hold the same bits at
    every mapped position, NaN everywhere else. Never written: runs work on clones."""

    def __init__(self, fmt, D, P, lens, L_max, seed, spare=2):
        self.fmt, self.fp8, self.D, self.P = fmt, fmt == "fp8", D, P
        self.lens, self.L_max = lens, L_max
        B = self.B = len(lens)
        g = torch.Generator().manual_seed(seed)
        self.q = torch.randn(B, H, D, generator=g).to(torch.bfloat16)
        tok = [torch.randn(B, H, D, generator=g).to(torch.bfloat16) for _ in range(2)]
        held = [min(max(n, 0), L_max) for n in lens]
        rows = [[torch.randn(H, n, D, generator=g).to(torch.bfloat16) for n in held]
                for _ in range(2)]
        flat = _nan_planes(self.fp8, (B, H), L_max, D)
        # fp32 K / V every row attends over (the token last, where it has a position), per key
        self.keys, self.tok_bits = [], []
        for b, n in enumerate(held):
            kv, tb = [], []
            for j in range(2):
                x = rows[j][b]
                if 0 <= lens[b] < L_max:
                    x = torch.cat([x, tok[j][b][:, None]], dim=1)
                if x.shape[1] == 0:
                    kv.append(x.float())
                    tb.append(None)
                elif self.fp8:
                    code, scale = _quant(x)
                    flat[j][b, :, :n], flat[2 + j][b, :, :n] = code[:, :n], scale[:, :n]
                    kv.append(code.view(E4M3).float() * scale[..., None])
                    tb.append((code[:, -1], scale[:, -1]))
                else:
                    flat[j][b, :, :n] = x[:, :n]
                    kv.append(x.float())
                    tb.append((x[:, -1],))
            self.keys.append(kv)
            self.tok_bits.append(tb)
        # the pages every row needs for its keys and its token, and two spare
        self.max_pages = (L_max + P - 1) // P
        self.need = [0 if n < 0 else (min(n + 1, L_max) + P - 1) // P for n in lens]
        self.n_pages = sum(self.need) + spare
        order = _shuffled(self.n_pages, seed)
        table = torch.full((B, self.max_pages), -1, dtype=I32)
        back = _nan_planes(self.fp8, (self.n_pages + 2 * GUARD, H), P, D)
        for b in range(B):
            for j in range(self.need[b]):
                page = table[b, j] = order.pop(0)
                for dst, src in zip(back, flat):
                    dst[GUARD + page] = src[b, :, j * P:(j + 1) * P]
        self.free = order
        self.flat = [t.to(DEV) for t in flat]
        self.back = [t.to(DEV) for t in back]
        self.table = table.to(DEV)
        self.qkv = torch.cat([t.reshape(B, 1, H * D) for t in (self.q, *tok)], dim=2).to(DEV)
        self.length = torch.tensor(lens, dtype=I32, device=DEV)

    def fresh(self):
        return [t.clone() for t in self.back]

    def pool(self, back):
        return [t[GUARD:GUARD + self.n_pages] for t in back]

    def run(self, back, table=None, **kw):
        """The paged ``decode_attention`` on the pools inside ``back`` (no ``pos``: no host
        check)."""
        k, v, scales = _typed(self.pool(back), self.fp8)
        return decode_attention(self.qkv, H, k, v, self.length, max_len=self.L_max,
                                block_table=self.table if table is None else table, **scales,
                                **kw)

    def run_flat(self, flat, **kw):
        """The contiguous per-sequence ``decode_attention``: the reference of the bit identity."""
        k, v, scales = _typed(flat, self.fp8)
        return decode_attention(self.qkv, H, k, v, self.length, **scales, **kw)

    def gather(self, back, table=None):
        """The pools through the table as contiguous ``[B, H, max_pages * P, ...]`` planes and
        the mask of the mapped positions."""
        table = (self.table if table is None else table).tolist()
        out = _nan_planes(self.fp8, (self.B, H), self.max_pages * self.P, self.D)
        out = [t.to(DEV) for t in out]
        mapped = torch.zeros(self.B, self.max_pages * self.P, dtype=torch.bool)
        for b, row in enumerate(table):
            for j, page in enumerate(row):
                if 0 <= page < self.n_pages:
                    mapped[b, j * self.P:(j + 1) * self.P] = True
                    for dst, src in zip(out, self.pool(back)):
                        dst[b, :, j * self.P:(j + 1) * self.P] = src[page]
        return out, mapped.to(DEV)

    def want(self, b, drop=0):
        """fp32 softmax attention of row ``b`` over its keys without the last ``drop``."""
        K, V = (t[:, :t.shape[1] - drop] for t in self.keys[b])
        s = (self.q[b].float()[:, None, :] * K).sum(-1) / math.sqrt(self.D)
        return (torch.softmax(s, dim=-1)[..., None] * V).sum(1)            # [H, D]

    def expected_back(self, skip=()):
        """The backing allocation after one step: the token's row of every live row with room
        (but ``skip``), nothing else."""
        out = [t.clone() for t in self.back]
        tab = self.table.tolist()
        for b, n in enumerate(self.lens):
            if not 0 <= n < self.L_max or b in skip:
                continue
            page, r = GUARD + tab[b][n // self.P], n % self.P
            for j in range(2):
                bits = self.tok_bits[b][j]
                out[j][page, :, r] = bits[0].to(DEV)
                if self.fp8:
                    out[2 + j][page, :, r] = bits[1].to(DEV)
        return out


def _ratio(case, got, b, drop=0):
    want = case.want(b, drop)
    g = got[b].view(H, case.D).float().cpu()
    assert torch.isfinite(g).all(), b
    ratio = float((g - want).abs().max() / want.abs().max())
    print(f"  row {b} (length {case.lens[b]}, {drop} keys unmapped): "
          f"max|got-want|/max|want| = {ratio:.3e}")
    return ratio


@functools.lru_cache(maxsize=None)
def _case(fmt, D, P):
    """The shapes of test_decode_ragged_gpu.py: an empty slot, an empty sequence, the chunk edges
    and a row of several chunks; ``L_max`` = 4 chunks."""
    c = _chunk(fmt)
    return _Case(fmt, D, P, [-1, 0, c - 1, c, c + 1, 3 * c + 16], 4 * c,
                 seed=1000 * D + P + (7 if fmt == "fp8" else 0))


@functools.lru_cache(maxsize=None)
def _paged(fmt, D, P, fused):
    """ONE paged launch (plus the append launch when unfused) -> (output, the backing after)."""
    case = _case(fmt, D, P)
    back = case.fresh()
    got = case.run(back, fused=fused)
    torch.cuda.synchronize()
    return got, back


@functools.lru_cache(maxsize=None)
def _contiguous(fmt, D, P, fused):
    """The same step on the contiguous per-sequence caches -> (output, the caches after)."""
    case = _case(fmt, D, P)
    flat = [t.clone() for t in case.flat]
    got = case.run_flat(flat, fused=fused)
    torch.cuda.synchronize()
    return got, flat


ALL = pytest.mark.parametrize("fmt,D,P,fused", [(f, d, p, u) for f in FMTS for d in (64, 128)
                                                for p in PAGES for u in (True, False)])


@ALL
def test_bit_identical_to_the_contiguous_kernels(fmt, D, P, fused):
    """Output rows and the cache gathered through the table after the step have the bytes of
    ``decode_attention`` on contiguous per-sequence caches with the same contents."""
    case = _case(fmt, D, P)
    assert case.n_pages <= case.B * case.max_pages // 2            # far fewer than B * max_pages
    got, back = _paged(fmt, D, P, fused)
    want, flat = _contiguous(fmt, D, P, fused)
    assert torch.equal(_bits(got), _bits(want))
    mine, mapped = case.gather(back)
    for name, a, b in zip(("k", "v", "k_scale", "v_scale"), mine, flat):
        m = mapped[:, None, :case.L_max].expand(case.B, H, case.L_max)
        assert torch.equal(_bits(a[:, :, :case.L_max][m]), _bits(b[m])), name
    assert int(mapped.sum()) == sum(case.need) * P


@ALL
def test_rows_match_fp32(fmt, D, P, fused):
    """The project's bound, max|got - want| / max|want| <= 2^-7 per row (one bf16 rounding of the
    output is <= 2^-9 relative; for the FP8 cache the reference is over the dequantised codes).
    Everything in the pool that is no live key is NaN: a wrong page or row would show."""
    case = _case(fmt, D, P)
    got, _ = _paged(fmt, D, P, fused)
    print(f"paged decode {fmt} D={D} P={P} fused={fused}:")
    worst = max(_ratio(case, got, b) for b, n in enumerate(case.lens) if n >= 0)
    assert worst <= 2.0 ** -7, f"max|got - want| / max|want| = {worst:.3e} > 2^-7"


@ALL
def test_nothing_else_is_written(fmt, D, P, fused):
    """The whole backing allocation before and after: only the token's row of every live row may
    differ (and is the token's bits); free pages, other rows' pages, both guard zones and the
    scale planes keep theirs. The empty slot's output row is zero bits, ``length`` is not
    advanced, the table is not written."""
    case = _case(fmt, D, P)
    got, back = _paged(fmt, D, P, fused)
    assert not _bits(got[0]).any()
    for name, mine, want in zip(("k", "v", "k_scale", "v_scale"), back, case.expected_back()):
        assert torch.equal(_bits(mine), _bits(want)), name
    for t in back:                                                 # the guard zones, explicitly
        for zone in (t[:GUARD], t[GUARD + case.n_pages:]):
            assert (zone == NAN_CODE).all() if zone.dtype == U8 else torch.isnan(zone.float()).all()
    assert case.length.tolist() == case.lens
    assert int((case.table >= 0).sum()) == sum(case.need)


@ALL
def test_unmapped_pages_are_masked_and_their_stores_dropped(fmt, D, P, fused):
    """The last needed page of row 4 is unmapped with -1 and of row 5 with ``n_pages`` (one past
    the pool: its rows are the guard zone). No ``pos``, so no host check. Both rows attend their
    mapped keys only (fp32, the bound above), their token is not stored, and the backing
    allocation is otherwise as after the plain step."""
    case = _case(fmt, D, P)
    table = case.table.clone()
    drop = {}
    for b, entry in ((4, -1), (5, case.n_pages)):
        last = case.need[b] - 1
        table[b, last] = entry
        drop[b] = case.lens[b] + 1 - last * P                      # keys on that page, the token too
    assert drop[4] >= 1 and drop[5] >= 1
    back = case.fresh()
    got = case.run(back, table=table, fused=fused)
    torch.cuda.synchronize()
    print(f"paged decode {fmt} D={D} P={P} fused={fused}, rows 4 and 5 with an unmapped page:")
    worst = max(_ratio(case, got, b, drop.get(b, 0)) for b, n in enumerate(case.lens) if n >= 0)
    assert worst <= 2.0 ** -7, f"max|got - want| / max|want| = {worst:.3e} > 2^-7"
    for name, mine, want in zip(("k", "v", "k_scale", "v_scale"), back,
                                case.expected_back(skip=(4, 5))):
        assert torch.equal(_bits(mine), _bits(want)), name
    plain, _ = _paged(fmt, D, P, fused)                            # the other rows: untouched bits
    assert torch.equal(_bits(got[:4]), _bits(plain[:4]))
    assert not torch.equal(_bits(got[4:]), _bits(plain[4:]))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("P", PAGES)
@pytest.mark.parametrize("D", [64, 128])
def test_paged_prefill_append(fmt, D, P):
    """``T = P + 3`` tokens from ``length = [-1, 0, P - 2, 5]``: every live row crosses a page
    edge, row 3 has its second page unmapped (its tokens there are dropped). At the mapped
    positions the pools hold the bits of the contiguous ``_seq`` append; the rest of the backing
    allocation (free pages, guards, scales) keeps its bits."""
    T, lens, L_max, fp8 = P + 3, [-1, 0, P - 2, 5], 4 * P, fmt == "fp8"
    B, max_pages = len(lens), 4
    need = [0, 2, 3, 2]
    n_pages = sum(need) + 2
    g = torch.Generator().manual_seed(D + P)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(torch.bfloat16).to(DEV)
    order = _shuffled(n_pages, D + P)
    table = torch.full((B, max_pages), -1, dtype=I32)
    for b in range(B):
        for j in range(need[b]):
            table[b, j] = order.pop(0)
    gone = int(table[3, 1])
    table[3, 1] = -1
    flat = [t.to(DEV) for t in _nan_planes(fp8, (B, H), L_max, D)]
    back = [t.to(DEV) for t in _nan_planes(fp8, (n_pages + 2 * GUARD, H), P, D)]
    want = [t.clone() for t in back]
    length = torch.tensor(lens, dtype=I32, device=DEV)

    k, v, scales = _typed(flat, fp8)
    kv_append(qkv, H, k, v, length, **scales)                      # the contiguous reference
    for b, row in enumerate(table.tolist()):
        for j, page in enumerate(row):
            if page >= 0:
                for dst, src in zip(want, flat):
                    dst[GUARD + page] = src[b, :, j * P:(j + 1) * P]
    k, v, scales = _typed([t[GUARD:GUARD + n_pages] for t in back], fp8)
    dev_table = table.to(DEV)
    kv_append(qkv, H, k, v, length, block_table=dev_table, max_len=L_max, **scales)
    torch.cuda.synchronize()
    for name, mine, w in zip(("k", "v", "k_scale", "v_scale"), back, want):
        assert torch.equal(_bits(mine), _bits(w)), name
    page0 = back[0][GUARD + int(table[3, 0])]                      # row 3 did land on its page 0
    assert not (page0[:, 5:] == NAN_CODE).all() if fp8 else not torch.isnan(page0[:, 5:].float()).any()
    untouched = back[0][GUARD + gone]
    assert (untouched == NAN_CODE).all() if fp8 else torch.isnan(untouched.float()).all()
    with pytest.raises(ValueError, match="not mapped"):            # the host check sees it
        kv_append(qkv, H, k, v, length, pos=lens, block_table=dev_table, table_host=table,
                  max_len=L_max, **scales)
    kv_append(qkv, H, k, v, length, pos=lens, block_table=dev_table, table_host=table,
              max_len=L_max, n_keep=[0, T, T, P - 5], **scales)    # the padded prefill's bound


def _caches(fmt, D, P, lens, L_max, steps, seed, spare=2):
    """A contiguous per-sequence :class:`ops.KVCache` and a paged one (shuffled physical pages,
    reserved for ``steps`` more tokens) of one layer holding the same random rows below ``lens``,
    and the ``[B, 1, 3C]`` token every step decodes."""
    B, fp8 = len(lens), fmt == "fp8"
    g = torch.Generator().manual_seed(seed)
    flat = ops.KVCache(1, B, H, D, L_max, DEV, kv_dtype=fmt, per_sequence=True)
    need = sum((n + steps + P - 1) // P for n in lens if n >= 0)
    paged = ops.KVCache(1, B, H, D, L_max, DEV, kv_dtype=fmt, page_size=P, n_pages=need + spare)
    paged._pages.free = _shuffled(need + spare, seed)
    for c in (flat, paged):
        c.set_lengths(lens)
    paged.reserve_all([max(n, 0) + steps for n in lens])
    assert paged.pages_in_use == need
    for j, (dst, sc) in enumerate(((flat.k[0], flat.k_scale[0]), (flat.v[0], flat.v_scale[0]))):
        for b, n in enumerate(lens):
            if n > 0:
                x = torch.randn(H, n, D, generator=g).to(torch.bfloat16)
                if fp8:
                    code, scale = _quant(x)
                    dst.view(U8)[b, :, :n], sc[b, :, :n] = code.to(DEV), scale.to(DEV)
                else:
                    dst[b, :, :n] = x.to(DEV)
    _copy_pages(flat, paged)
    qkv = torch.randn(B, 1, 3 * H * D, generator=g).to(torch.bfloat16).to(DEV)
    return flat, paged, qkv


def _planes(c):
    return [t.view(U8) if t.dtype == E4M3 else t
            for t in (c.k[0], c.v[0], c.k_scale[0], c.v_scale[0]) if t is not None]


def _copy_pages(flat, paged):
    """The contiguous cache's contents into the paged cache's mapped pages."""
    P = paged.page_size
    for b, row in enumerate(paged.table_host.tolist()):
        for j, page in enumerate(row):
            if page >= 0:
                for dst, src in zip(_planes(paged), _planes(flat)):
                    dst[page] = src[b, :, j * P:(j + 1) * P]


def _gathered_equal(flat, paged):
    """The paged cache through its table equals the contiguous cache on every mapped page."""
    P = paged.page_size
    for b, row in enumerate(paged.table_host.tolist()):
        for j, page in enumerate(row):
            if page >= 0:
                for name, mine, want in zip("k v k_scale v_scale".split(), _planes(paged),
                                            _planes(flat)):
                    end = min((j + 1) * P, flat.max_len)
                    assert torch.equal(_bits(mine[page][:, :end - j * P]),
                                       _bits(want[b, :, j * P:end])), (name, b, j)


def _step(c, qkv, **kw):
    paged = dict(block_table=c.block_table, table_host=c.table_host, max_len=c.max_len) \
        if c.paged else {}
    kw.setdefault("pos", c.pos)
    return decode_attention(qkv, H, c.k[0], c.v[0], c.length, workspace=c.workspace,
                            k_scale=c.k_scale[0], v_scale=c.v_scale[0], **paged, **kw)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("P", PAGES)
@pytest.mark.parametrize("D", [64, 128])
def test_graph_replay_across_a_page_edge(fmt, D, P):
    """From ``[P - 2, 2P - 1, -1, 0]`` after ``reserve_all``: one captured step + ``advance(1)``
    replayed four times (single stream, as the ragged replay test captures) equals four eager
    paged steps and four contiguous steps bit for bit, outputs and gathered caches; rows 0 and 1
    cross a page edge on the way. Reserving during the capture raises ``RuntimeError`` (checked
    on the host before any device call) and the capture goes on."""
    steps, lens, L_max = 4, [P - 2, 2 * P - 1, -1, 0], 4 * P
    flat, eager_c, qkv = _caches(fmt, D, P, lens, L_max, steps, seed=31 + D + P)
    _, graph_c, _ = _caches(fmt, D, P, lens, L_max, steps, seed=31 + D + P)
    assert graph_c.table_host.tolist() == eager_c.table_host.tolist()
    want, eager = [], []
    for _ in range(steps):
        want.append(_step(flat, qkv).clone())
        flat.advance(1)
        eager.append(_step(eager_c, qkv).clone())
        eager_c.advance(1)
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up: writes the same token rows
        _step(graph_c, qkv)
        graph_c.advance(1)
    torch.cuda.current_stream().wait_stream(side)
    graph_c.set_lengths(lens)
    torch.cuda.synchronize()
    table = graph_c.table_host.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="capturing"):
            graph_c.reserve(3, 2 * P)                    # a free page is there: not exhaustion
        out = _step(graph_c, qkv)
        graph_c.advance(1)
    assert torch.equal(graph_c.table_host, table) and graph_c.pages_in_use == eager_c.pages_in_use
    assert graph_c.length.tolist() == lens               # the capture ran nothing
    for i in range(steps):
        graph.replay()
        torch.cuda.synchronize()
        assert graph_c.length.tolist() == [n + i + 1 if n >= 0 else n for n in lens]
        assert torch.equal(_bits(out), _bits(eager[i])), f"replay {i} against eager"
        assert torch.equal(_bits(out), _bits(want[i])), f"replay {i} against contiguous"
    assert _same(_planes(graph_c), _planes(eager_c))
    _gathered_equal(flat, graph_c)
    assert not torch.equal(_bits(eager[0]), _bits(eager[-1]))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("P", PAGES)
def test_two_runs_are_bit_identical(fmt, P):
    case = _case(fmt, 128, P)
    first, back = _paged(fmt, 128, P, True)
    again = case.fresh()
    second = case.run(again)
    torch.cuda.synchronize()
    assert torch.equal(_bits(first), _bits(second))
    assert _same(back, again)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("P", PAGES)
def test_a_retired_rows_pages_are_reused(fmt, P):
    """Row 1 is retired, a new sequence is placed in it and receives its pages (host mirror), is
    prefilled through ``slot(1)`` and decoded with the batch: the other rows' outputs have the
    bits of a run in which nothing was retired, the new row matches its own contiguous run."""
    D, lens, L_max, T = 128, [P + 3, 2 * P - 3, 7], 4 * P, P + 5
    flat, paged, qkv = _caches(fmt, D, P, lens, L_max, 2, seed=5 + P, spare=0)
    _, twin, _ = _caches(fmt, D, P, lens, L_max, 2, seed=5 + P, spare=0)
    want = _step(twin, qkv)                                        # nothing retired
    old = [p for p in paged.table_host[1].tolist() if p >= 0]
    assert len(old) == 2
    for c in (flat, paged):
        c.retire(1)
    assert paged.table_host[1].tolist() == [-1] * 4 and paged.free_pages[-2:] == old[::-1]
    new = torch.randn(1, T, 3 * H * D, generator=torch.Generator().manual_seed(P)) \
        .to(torch.bfloat16).to(DEV)
    for c in (flat, paged):
        s = c.slot(1)
        s.set_length(0)
        if c.paged:
            s.reserve(0, T)
            assert c.table_host[1].tolist()[:2] == old               # the retired row's pages
            kv_append(new, H, s.k[0], s.v[0], s.length, pos=s.pos, k_scale=s.k_scale[0],
                      v_scale=s.v_scale[0], block_table=s.block_table,
                      table_host=s.table_host, max_len=L_max)
        else:
            kv_append(new, H, s.k[0], s.v[0], s.length, pos=s.pos, k_scale=s.k_scale[0],
                      v_scale=s.v_scale[0])
        s.advance(T)
    assert paged.pos == [lens[0], T, lens[2]] == flat.pos
    with pytest.raises(ValueError, match="not mapped"):            # T + 1 = P + 6: still page 1
        _step(paged, qkv, pos=[lens[0], 2 * P, lens[2]])
    got, ref = _step(paged, qkv), _step(flat, qkv)
    torch.cuda.synchronize()
    for b in (0, 2):
        assert torch.equal(_bits(got[b]), _bits(want[b])), b
    assert torch.equal(_bits(got), _bits(ref))
    _gathered_equal(flat, paged)


def test_launcher_refusals():
    """``P = 24``, ``chunk = 256`` with ``P = 512`` and a null table: ``ValueError`` from the op
    or ``hipErrorInvalidValue`` from the C call, nothing launched: the NaN-filled output stays
    NaN."""
    D, B = 64, 2
    qkv = torch.zeros(B, 1, 3 * H * D, dtype=torch.bfloat16, device=DEV)
    length = torch.zeros(B, dtype=I32, device=DEV)
    table = torch.zeros(B, 4, dtype=I32, device=DEV)
    for P in (24, 512):
        pool = torch.zeros(2, H, P, D, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(ValueError):
            decode_attention(qkv, H, pool, pool.clone(), length, block_table=table, chunk=256)
        with pytest.raises(ValueError):
            kv_append(qkv, H, pool, pool.clone(), length, block_table=table)
    pool = torch.zeros(8, H, 64, D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        decode_attention(qkv, H, pool, pool.clone(), length, block_table=table, chunk=96)

    lib, stream = _lib.lib(), _lib.stream(qkv.device)
    out = torch.full((B, 1, H * D), NAN, dtype=torch.bfloat16, device=DEV)
    ws = torch.full((B * H * 4 * (D + 2),), NAN, dtype=torch.float32, device=DEV)
    kp, vp = pool, pool.clone()

    def decode(tab, stride, n_pages, P, chunk):
        return lib.dlbb_attn_decode_paged(qkv.data_ptr(), 3 * H * D, kp.data_ptr(), vp.data_ptr(),
                                          length.data_ptr(), tab, stride, n_pages, P,
                                          ws.data_ptr(), out.data_ptr(), H * D, B, H, D, 256, 256,
                                          chunk, 1, 0.125, stream)

    def append(tab, stride, n_pages, P):
        return lib.dlbb_kv_append_paged(qkv.data_ptr(), 3 * H * D, kp.data_ptr(), vp.data_ptr(),
                                        length.data_ptr(), tab, stride, n_pages, P, B, 1, H, D,
                                        256, stream)

    INVALID = 1                                                    # hipErrorInvalidValue
    t = table.data_ptr()
    assert decode(t, 4, 8, 24, 256) == INVALID                     # no power of two
    assert decode(t, 4, 8, 512, 256) == INVALID                    # P does not divide the chunk
    assert decode(t, 4, 8, 64, 96) == INVALID
    assert decode(None, 4, 8, 64, 256) == INVALID                  # a null table
    assert decode(t + 2, 4, 8, 64, 256) == INVALID                 # a misaligned one
    assert decode(t, 4, 0, 64, 256) == INVALID                     # no pages
    assert decode(t, 3, 8, 64, 256) == INVALID                     # rows shorter than L_max / P
    assert append(None, 4, 8, 64) == INVALID
    assert append(t, 4, 8, 24) == INVALID
    assert append(t, 4, 0, 64) == INVALID
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all() and torch.isnan(ws).all()
    assert not kp.any() and not vp.any()
