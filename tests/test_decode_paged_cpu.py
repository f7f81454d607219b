"""The paged KV cache, CPU side (torch path; gloo world 1): the page allocator's bookkeeping
(reserve, advance over a page edge, retire, LIFO reuse, the peak), pool exhaustion, the paged torch
forms of append and decode against the contiguous per-sequence torch forms (bit for bit), the
model's prefill + decode + retire-and-refill against the same model on a contiguous per-sequence
cache, the page-size refusals, the two config keys and the ``run_tp --kv-page-size`` argument
errors."""

import copy
import os
import subprocess
import sys

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
from distributed_llm_backend_benchmark_amd.ops import decode as dec
from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = torch.int32


def _state(c):
    return (list(c.pos), c.length.tolist(), c.table_host.tolist(), c.block_table.tolist(),
            c.free_pages, c.pages_in_use)


def test_allocator_bookkeeping():
    P = 16
    c = ops.KVCache(2, 3, 2, 64, 64, "cpu", page_size=P, n_pages=7)
    assert c.paged and c.per_sequence and c.page_size == P and c.n_pages == 7
    assert c.length.shape == (3,) and c.block_table.shape == (3, 4)
    assert c.block_table.dtype == I32 and c.table_host.tolist() == [[-1] * 4] * 3
    assert [t.shape for t in c.k + c.v] == [(7, 2, P, 64)] * 4
    assert c.nbytes == 2 * 2 * 7 * 2 * P * 64 * 2                  # the pools: layers, K + V
    assert c.pages_in_use == 0 and c.peak_pages_in_use == 0

    c.reserve(0, 17)                                               # two pages, page 0 first
    assert c.table_host[0].tolist() == [0, 1, -1, -1] and c.pages_in_use == 2
    c.reserve(0, 5)                                                # never unmaps
    assert c.table_host[0].tolist() == [0, 1, -1, -1]
    c.set_lengths([17, -1, 15])                                    # row 2: one page
    assert c.table_host.tolist() == [[0, 1, -1, -1], [-1] * 4, [2, -1, -1, -1]]
    assert c.block_table.tolist() == c.table_host.tolist()
    assert c.live_bytes() == (17 + 15) * 2 * 2 * 64 * 2 * 2
    c.advance(1)                                                   # row 2 crosses a page edge
    assert c.pos == [18, -1, 16] and c.table_host[2].tolist() == [2, -1, -1, -1]
    c.advance(1)                                                   # 17 positions: a second page
    assert c.pos == [19, -1, 17] and c.table_host[2].tolist() == [2, 3, -1, -1]
    assert c.pages_in_use == 4 and c.peak_pages_in_use == 4
    c.reserve_all(33)                                              # live rows only
    assert c.table_host.tolist() == [[0, 1, 4, -1], [-1] * 4, [2, 3, 5, -1]]
    assert c.pages_in_use == 6 and c.peak_pages_in_use == 6

    c.retire(0)                                                    # its pages go back ...
    assert c.pos == [-1, -1, 17] and c.table_host[0].tolist() == [-1] * 4
    assert c.pages_in_use == 3 and c.free_pages[-3:] == [4, 1, 0]
    s = c.slot(1)                                                  # ... and the next row gets them
    assert s.paged and s.batch == 1 and s.per_sequence and s.pos == [-1]
    assert s.k[0] is c.k[0] and s.workspace is c.workspace
    assert s.length.data_ptr() == c.length[1:].data_ptr()
    s.set_length(0)
    s.reserve(0, 40)
    assert c.table_host[1].tolist() == [0, 1, 4, -1] == s.table_host[0].tolist()
    assert s.block_table.data_ptr() == c.block_table[1:].data_ptr()
    s.advance(40)
    assert c.pos == [-1, 40, 17] and c.length.tolist() == [-1, 40, 17]
    assert c.peak_pages_in_use == 6 and c.pages_in_use == 6
    c.set_length(0, keep_pages=True)                               # empties the rows only
    assert c.pos == [0, 0, 0] and c.pages_in_use == 6 and c.table_host[1].tolist() == [0, 1, 4, -1]
    c.set_length(0)                                                # frees everything
    assert c.pages_in_use == 0 and c.table_host.tolist() == [[-1] * 4] * 3
    assert c.block_table.tolist() == [[-1] * 4] * 3 and c.pos == [0, 0, 0]
    assert sorted(c.free_pages) == list(range(7)) and c.peak_pages_in_use == 6


def test_exhaustion_raises_and_changes_nothing():
    c = ops.KVCache(1, 3, 2, 64, 64, "cpu", page_size=16, n_pages=4)
    c.set_lengths([20, 10, -1])                                    # 2 + 1 pages
    before = _state(c)
    for call in (lambda: c.reserve(1, 40),                         # 2 more, 1 free
                 lambda: c.reserve_all(33),                        # 1 + 2 more
                 lambda: c.set_lengths([20, 10, 30]),
                 lambda: c.set_lengths([50, -1, 17]),              # frees 1, needs 2 + 2
                 lambda: c.set_length(30)):
        with pytest.raises(ValueError, match=r"pages needed, \d+ free"):
            call()
        assert _state(c) == before
    c.set_lengths([12, 10, -1])
    c.advance(4)                                                   # 16 and 14: still one page each
    mid = _state(c)
    c.reserve(0, 48)                                               # the last free page
    with pytest.raises(ValueError, match="1 pages needed, 0 free"):
        c.advance(3)                                               # row 1 would need a second one
    assert c.pos == [16, 14] + [-1] and _state(c)[0] == mid[0]
    with pytest.raises(ValueError):
        c.reserve(0, 65)                                           # past max_len
    for call in (lambda: ops.KVCache(1, 2, 2, 64, 64, "cpu").reserve(0, 1),
                 lambda: ops.KVCache(1, 2, 2, 64, 64, "cpu", n_pages=3)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("page_size", [0, 8, 24, 48, 512])
def test_page_size_refusals(page_size):
    """Not a power of two in [16, 256] (512 does not divide the chunk of 256 keys either)."""
    with pytest.raises(ValueError):
        ops.KVCache(1, 2, 2, 64, 64, "cpu", page_size=page_size)
    H, D, P = 2, 64, page_size
    if P:
        qkv = torch.zeros(1, 1, 3 * H * D, dtype=torch.bfloat16)
        pool = torch.zeros(2, H, P, D, dtype=torch.bfloat16)
        table = torch.zeros(1, 2, dtype=I32)
        with pytest.raises(ValueError):
            dec.decode_attention(qkv, H, pool, pool.clone(), torch.zeros(1, dtype=I32),
                                 block_table=table)
        with pytest.raises(ValueError):
            dec.kv_append(qkv, H, pool, pool.clone(), torch.zeros(1, dtype=I32), block_table=table)


def test_page_size_must_divide_the_chunk():
    H, D = 2, 64
    qkv = torch.zeros(1, 1, 3 * H * D, dtype=torch.bfloat16)
    pool = torch.zeros(2, H, 64, D, dtype=torch.bfloat16)
    length, table = torch.zeros(1, dtype=I32), torch.zeros(1, 2, dtype=I32)
    for chunk in (32, 96, 64 * 65):                                # < P, no multiple, > 64 pages
        with pytest.raises(ValueError):
            dec.decode_attention(qkv, H, pool, pool.clone(), length, block_table=table, chunk=chunk)
    dec.decode_attention(qkv, H, pool, pool.clone(), length, block_table=table, chunk=128)
    for bad in (dict(block_table=table.long()), dict(block_table=torch.zeros(2, 2, dtype=I32)),
                dict(block_table=table, max_len=129)):
        with pytest.raises(ValueError):
            dec.decode_attention(qkv, H, pool, pool.clone(), length, **bad)
    with pytest.raises(ValueError):                                # the shared length: not paged
        dec.decode_attention(torch.zeros(2, 1, 3 * H * D, dtype=torch.bfloat16), H, pool,
                             pool.clone(), length, block_table=torch.zeros(2, 2, dtype=I32))


def _tensors(c):
    return [t for t in (c.k[0], c.v[0], c.k_scale[0], c.v_scale[0]) if t is not None]


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _gathered(c):
    """The paged cache's rows through the table, as the contiguous ``[B, H, L, ...]`` tensors;
    unmapped pages read as zeros."""
    P, out = c.page_size, []
    for pool in _tensors(c):
        raw = pool.view(torch.uint8) if pool.dtype == dec.E4M3 else pool
        full = torch.zeros(c.batch, c.n_head, c.table_host.shape[1] * P, *raw.shape[3:],
                           dtype=raw.dtype)
        for b, row in enumerate(c.table_host.tolist()):
            for j, page in enumerate(row):
                if page >= 0:
                    full[b, :, j * P:(j + 1) * P] = raw[page]
        out.append(full[:, :, :c.max_len])
    return out


def _pair(kv_dtype, B, H, D, L_max, P, lens, seed, spare=1):
    """A contiguous per-sequence cache and a paged one with shuffled physical pages, both holding
    the same random rows below ``lens`` (appended through the ops)."""
    g = torch.Generator().manual_seed(seed)
    flat = ops.KVCache(1, B, H, D, L_max, "cpu", kv_dtype=kv_dtype, per_sequence=True)
    need = sum((max(n, 0) + P) // P for n in lens)                 # room for one more token
    paged = ops.KVCache(1, B, H, D, L_max, "cpu", kv_dtype=kv_dtype, page_size=P,
                        n_pages=need + spare)
    order = torch.randperm(need + spare, generator=g).tolist()
    paged._pages.free = order                                      # logical neighbours apart
    for c in (flat, paged):
        c.set_lengths([0 if n >= 0 else -1 for n in lens])
    paged.reserve_all([max(n, 0) + 1 for n in lens])
    fill = torch.randn(B, max(lens), 3 * H * D, generator=g).to(torch.bfloat16)
    dec.kv_append(fill, H, flat.k[0], flat.v[0], flat.length, pos=flat.pos,
                  k_scale=flat.k_scale[0], v_scale=flat.v_scale[0])
    dec.kv_append(fill, H, paged.k[0], paged.v[0], paged.length, pos=paged.pos,
                  k_scale=paged.k_scale[0], v_scale=paged.v_scale[0],
                  block_table=paged.block_table, table_host=paged.table_host, max_len=L_max,
                  n_keep=[max(n, 0) for n in lens])
    for c in (flat, paged):
        c.set_lengths(lens)
    return flat, paged, g


def _same_below(flat, paged, lens, extra=0):
    """Bit identity of the two caches at every row's positions below ``lens[b] + extra``."""
    for name, a, b in zip("k v k_scale v_scale".split(), _tensors(flat), _gathered(paged)):
        a = a.view(torch.uint8) if a.dtype == dec.E4M3 else a
        for r, n in enumerate(lens):
            if n >= 0:
                assert torch.equal(_bits(a[r, :, :n + extra]), _bits(b[r, :, :n + extra])), \
                    (name, r)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [32, 64])
def test_paged_torch_forms_equal_the_contiguous_ones(kv_dtype, D):
    """Append (one token and a block crossing a page edge) and decode: the paged torch forms
    give the bits of the contiguous per-sequence torch forms, outputs and cache contents."""
    B, H, L_max, P, lens = 4, 2, 64, 16, [-1, 0, 15, 37]
    flat, paged, g = _pair(kv_dtype, B, H, D, L_max, P, lens, seed=D)
    _same_below(flat, paged, lens)
    kw = dict(block_table=paged.block_table, table_host=paged.table_host, max_len=L_max)

    qkv = torch.randn(B, 1, 3 * H * D, generator=g).to(torch.bfloat16)
    want = dec.decode_attention(qkv, H, flat.k[0], flat.v[0], flat.length, pos=flat.pos,
                                k_scale=flat.k_scale[0], v_scale=flat.v_scale[0])
    got = dec.decode_attention(qkv, H, paged.k[0], paged.v[0], paged.length, pos=paged.pos,
                               k_scale=paged.k_scale[0], v_scale=paged.v_scale[0], **kw)
    assert torch.equal(_bits(got), _bits(want)) and not _bits(got[0]).any()
    _same_below(flat, paged, lens, extra=1)
    for c in (flat, paged):
        c.advance(1)

    T = 5                                                          # rows 2 crosses a page edge
    blk = torch.randn(B, T, 3 * H * D, generator=g).to(torch.bfloat16)
    paged.reserve_all([p + T for p in paged.pos])
    dec.kv_append(blk, H, flat.k[0], flat.v[0], flat.length, pos=flat.pos,
                  k_scale=flat.k_scale[0], v_scale=flat.v_scale[0])
    dec.kv_append(blk, H, paged.k[0], paged.v[0], paged.length, pos=paged.pos,
                  k_scale=paged.k_scale[0], v_scale=paged.v_scale[0], **kw)
    _same_below(flat, paged, [n + 1 if n >= 0 else n for n in lens], extra=T)

    # a needed page that is not mapped: refused before anything is written
    paged.advance(T)
    before = [t.clone() for t in _tensors(paged)]
    full = [p for p in paged.pos]                                  # row 3 at 43: page 2 mapped
    paged._pages.host[3, 2] = -1
    for call in (lambda: dec.decode_attention(qkv, H, paged.k[0], paged.v[0], paged.length,
                                              pos=full, k_scale=paged.k_scale[0],
                                              v_scale=paged.v_scale[0], **kw),
                 lambda: dec.kv_append(qkv, H, paged.k[0], paged.v[0], paged.length, pos=full,
                                       k_scale=paged.k_scale[0], v_scale=paged.v_scale[0], **kw)):
        with pytest.raises(ValueError, match="not mapped"):
            call()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, _tensors(paged)))


def _model(attention="sdpa"):
    comm = Comm(0, 1, 0, "gloo", torch.device("cpu"))
    return LLM(hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=1024, comm=comm,
               seed=3, init_std=0.05, kernels="torch", attention=attention)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_model_paged_equals_contiguous(kv_dtype):
    """Padded prefill, decode steps across page edges, retire and refill through ``slot``: every
    output at a real position has the bits of the same model on a contiguous per-sequence cache.
    The pool holds exactly the pages the rows need."""
    m = _model()
    m.kv_cache_dtype = kv_dtype
    lens, S, steps, max_len, P = [3, 17, 16], 17, 3, 48, 16
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, S, 256, generator=g).to(torch.bfloat16)
    flat = m.new_kv_cache(3, max_len, per_sequence=True)
    need = sum((n + steps + 1 + P - 1) // P for n in lens)         # 1 + 2 + 2
    paged = m.new_kv_cache(3, max_len, page_size=P, n_pages=need)
    assert paged.paged and paged.nbytes < flat.nbytes

    def both(tok, **kw):
        return m(tok, kv_cache=flat, **kw), m(tok, kv_cache=paged, **kw)

    a, b = both(x, prompt_lens=lens)
    assert paged.pos == lens == flat.pos and paged.length.tolist() == lens
    assert paged.pages_in_use == 1 + 2 + 1
    for r, n in enumerate(lens):
        assert torch.equal(a[r, :n], b[r, :n]), r
    tok = torch.stack([a[r, n - 1] for r, n in enumerate(lens)])[:, None]
    for i in range(steps):
        a, b = both(tok)
        assert torch.equal(a, b), i
        tok = a
    assert paged.pos == [n + steps for n in lens] and paged.pages_in_use == 1 + 2 + 2

    with pytest.raises(ValueError, match="pages needed"):          # a pool of exactly the need
        paged.reserve(0, 40)
    for c in (flat, paged):
        c.retire(1)
    assert paged.pages_in_use == 3 and paged.table_host[1].tolist() == [-1] * 3
    new = torch.randn(1, 20, 256, generator=g).to(torch.bfloat16)
    outs = []
    for c in (flat, paged):
        s = c.slot(1)
        s.set_length(0)
        outs.append(m(new, kv_cache=s))
    assert torch.equal(outs[0], outs[1])
    assert paged.pos == [lens[0] + steps, 20, lens[2] + steps] == flat.pos
    assert paged.table_host[1].tolist()[:2] == [1, 2]              # the retired row's pages again
    tok = torch.cat([tok[0:1], outs[0][:, -1:], tok[2:3]])
    a, b = both(tok)
    assert torch.equal(a, b)
    assert paged.peak_pages_in_use == 5 and paged.length.tolist() == paged.pos


def test_model_paged_refusals():
    m = _model()
    x = torch.zeros(2, 20, 256, dtype=torch.bfloat16)
    small = m.new_kv_cache(2, 32, page_size=16, n_pages=2)
    with pytest.raises(ValueError, match="pages needed"):          # before any launch
        m(x, kv_cache=small)
    assert small.pos == [0, 0] and small.pages_in_use == 0
    m(x, kv_cache=small, prompt_lens=[16, 9])                      # the padding needs no page
    assert small.pos == [16, 9] and small.pages_in_use == 2
    with pytest.raises(ValueError, match="pages needed"):
        m(x[:, :1], kv_cache=small)                                # row 0 needs a second page
    with pytest.raises(ValueError):
        _model("slice").new_kv_cache(2, 32, page_size=16)


def test_config_accepts_the_paged_keys_and_has_no_default():
    from distributed_llm_backend_benchmark_amd.utils.config import (DEFAULT_CONFIG, ConfigError,
                                                                    validate_config)

    cfg = copy.deepcopy(DEFAULT_CONFIG)
    ex = validate_config(cfg)["execution"]
    assert "kv_page_size" not in ex and "kv_pool_pages" not in ex
    for page in (16, 32, 64, 128, 256):
        cfg["execution"]["kv_page_size"] = page
        assert validate_config(cfg)["execution"]["kv_page_size"] == page
    cfg["execution"]["kv_pool_pages"] = 40
    assert validate_config(cfg)["execution"]["kv_pool_pages"] == 40
    for bad in (0, -1, True, "8", 1.5):
        cfg["execution"]["kv_pool_pages"] = bad
        with pytest.raises(ConfigError):
            validate_config(cfg)
    cfg["execution"]["kv_pool_pages"] = 40
    for bad in (0, 8, 24, 512, True, "16"):
        cfg["execution"]["kv_page_size"] = bad
        with pytest.raises(ConfigError):
            validate_config(cfg)
    del cfg["execution"]["kv_page_size"]
    with pytest.raises(ConfigError):                               # a pool without a page size
        validate_config(cfg)


def _cfg(tmp_path, S=16):
    import yaml

    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "baseline_config.yaml")))
    cfg["model"].update(hidden_size=64, num_layers=2, num_heads=2, ffn_intermediate=128,
                        init_std=0.05)
    cfg["input"].update(batch_size=2, sequence_length=S)
    cfg["execution"].update(warmup_iterations=1, benchmark_iterations=2, attention="sdpa",
                            kernels="torch")
    cfg["parallelism"]["world_size"] = 1
    cfg["experiment"]["output_dir"] = str(tmp_path)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return p


def _run_tp(tmp_path, extra, S=16):
    return subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                           "--config", str(_cfg(tmp_path, S)), "--backend", "gloo", "--device", "cpu",
                           *extra], capture_output=True, text=True, timeout=600, cwd=REPO)


@pytest.mark.parametrize("extra", [["--kv-page-size", "16"],
                                   ["--decode", "4", "--attention", "slice", "--kv-page-size", "16"],
                                   ["--decode", "4", "--kv-page-size", "16", "--kv-pages", "3"],
                                   ["--decode", "4", "--kv-page-size", "24"],
                                   ["--decode", "4", "--kv-pages", "8"]])
def test_run_tp_paged_argument_errors(tmp_path, extra):
    """No ``--decode``, attention slice, a pool too small (two rows of 16 + 4 positions need four
    pages of 16), a page size outside the set and ``--kv-pages`` alone: exit code 1, ERROR, no JSON."""
    out = _run_tp(tmp_path, extra)
    assert out.returncode == 1 and "ERROR" in out.stdout and "--kv-page" in out.stdout, \
        out.stdout[-2000:] + out.stderr[-3000:]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".json")]


def test_run_tp_paged_record(tmp_path):
    """``--prompt-lens 5,28 --decode 4 --kv-page-size 16`` at sequence length 28: the default pool
    is exactly ceil(9 / 16) + ceil(32 / 16) = 3 pages, smaller than the contiguous cache of 2 x 32
    positions; the record carries the page fields and the suffix ``_paged16`` comes last."""
    import json

    out = _run_tp(tmp_path, ["--decode", "4", "--prompt-lens", "5,28", "--kv-page-size", "16"],
                  S=28)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    files = [f for f in os.listdir(tmp_path) if f.endswith(".json")]
    assert len(files) == 1 and files[0].endswith("_decode4_ragged_paged16.json"), files
    d = json.load(open(tmp_path / files[0]))["decode"]
    assert d["kv_page_size"] == 16 and d["kv_pool_pages"] == 3 and d["kv_pages_peak"] == 3
    per_position = 2 * 2 * 2 * 32 * 2                  # layers, K + V, heads, head dim 32 bf16
    assert d["kv_cache_bytes_per_rank"] == 3 * 16 * per_position < 2 * 32 * per_position
