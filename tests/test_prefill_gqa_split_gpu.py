"""Key-split grouped-query prefill (``ops.prefill_attention(..., n_kv_head=, key_split=)``) against
a plain fp32 softmax on the same bf16 bits, on the data of ``test_prefill_gqa_gpu.py`` (two
independent KV heads, ``randn * 1.5``, caches NaN outside the live rows). The workspace is NaN
before every call: a chunk the combine may not read, or a record the split did not write, shows.
TOL is the project's prefill bound; the split changes only an fp32 merge of the unsplit sums."""

import functools
import math

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops

pytestmark = pytest.mark.gpu

HKV, NAN, DEV = 2, float("nan"), "cuda"
TOL = dict(rtol=2e-2, atol=2e-2)


def _reference(rows, n, T, G):
    """fp32 attention of tokens [n, n + T) of ``rows [n + T, H_q + 2 H_kv, D]`` -> [T, H_q * D]."""
    HQ, D = G * HKV, rows.shape[2]
    x = rows.float()
    kv_of = torch.arange(HQ) // G                              # query head h -> KV head h // G
    s = torch.einsum("thd,khd->htk", x[n:, :HQ], x[:, HQ + kv_of]) / math.sqrt(D)
    s.masked_fill_(~torch.ones(T, n + T, dtype=torch.bool).tril(diagonal=n), -math.inf)
    return torch.einsum("htk,khd->thd", s.softmax(-1), x[:, HQ + HKV + kv_of]).reshape(T, HQ * D)


@functools.lru_cache(maxsize=None)
def _case(D, G, lens, T, slack=5):
    """The block's qkv, NaN caches holding rows [0, len_b + T) of every live row (written by
    ``ops.kv_append``), the device lengths and the fp32 reference per row (None = empty slot)."""
    B, HQ, top = len(lens), G * HKV, max(lens)
    g = torch.Generator().manual_seed(1000 * D + 10 * G + 7 * T + sum(lens))
    rows = torch.randn(B, top + T, HQ + 2 * HKV, D, generator=g).mul(1.5).bfloat16()
    k, v = (torch.full((B, HKV, top + T + slack, D), NAN, dtype=torch.bfloat16, device=DEV)
            for _ in "kv")
    seq = len(set(lens)) > 1
    qkv = torch.stack([rows[b, max(n, 0):max(n, 0) + T] for b, n in enumerate(lens)])
    qkv = qkv.reshape(B, T, -1).to(DEV)
    length = torch.tensor(lens if seq else lens[:1], dtype=torch.int32, device=DEV)
    if top > 0:
        start = torch.tensor([0 if n >= 0 else -1 for n in lens] if seq else [0],
                             dtype=torch.int32, device=DEV)
        ops.kv_append(rows[:, :top].reshape(B, top, -1).to(DEV), HQ, k, v, start, n_kv_head=HKV)
        for b, n in enumerate(lens):
            if n >= 0:
                k[b, :, n:], v[b, :, n:] = NAN, NAN            # a shorter row of a ragged batch
    ops.kv_append(qkv, HQ, k, v, length, n_kv_head=HKV)
    ref = [None if n < 0 else _reference(rows[b, :n + T], n, T, G) for b, n in enumerate(lens)]
    return qkv, k, v, length, ref


def _split(qkv, G, k, v, length, chunk=128, len_bound=None, **kw):
    """The split form with a workspace of exactly the needed size, NaN before the call."""
    B, T, W = qkv.shape
    bound = k.shape[2] if len_bound is None else len_bound
    ws = torch.full((ops.prefill_workspace_numel(B, G * HKV, W // ((G + 2) * HKV), T, bound,
                                                 chunk),), NAN, device=DEV)
    return ops.prefill_attention(qkv, G * HKV, k, v, length, n_kv_head=HKV, key_split=chunk,
                                 len_bound=len_bound, workspace=ws, **kw)


def _check(out, ref):
    for b, r in enumerate(ref):
        if r is None:
            assert not out[b].any()
        else:
            assert torch.isfinite(out[b]).all()
            torch.testing.assert_close(out[b].float().cpu(), r, **TOL)


@pytest.mark.parametrize("D,G,T,n,slack,bound", [
    (D, G, T, n, 5, n + T) for D in (64, 128) for G in (2, 4, 8, 16)
    for T in (1, 32 // G + 1, 128 // G + 3) for n in (0, 127, 257)] + [
    (128, 4, 35, 257, 0, None),              # L_max == n + T
    (64, 8, 19, 127, 300, None)])            # grid chunks past the live range, which no row reads
def test_shared_length(D, G, T, n, slack, bound):
    qkv, k, v, length, ref = _case(D, G, (n, n), T, slack)
    out = _split(qkv, G, k, v, length, len_bound=bound, pos=n)
    _check(out, ref)
    assert torch.equal(out, _split(qkv, G, k, v, length, len_bound=bound))


@pytest.mark.parametrize("D", [64, 128])
def test_per_sequence(D, G=4, lens=(0, 37, -1, 300), T=70):
    qkv, k, v, length, ref = _case(D, G, lens, T)
    out = _split(qkv, G, k, v, length, len_bound=max(lens) + T, pos=lens)
    _check(out, ref)
    assert k[2].isnan().all() and v[2].isnan().all()           # the empty slot
    for b in (0, 1, 3):                                        # the bits of a batch-1 shared launch
        one = _split(qkv[b:b + 1], G, k[b:b + 1], v[b:b + 1], length[b:b + 1],
                     len_bound=max(lens) + T, pos=lens[b])
        assert torch.equal(out[b:b + 1], one)


@pytest.mark.parametrize("chunk", [128, 256, 512])
def test_chunk_sizes(chunk, D=128, G=8, T=9, n=600):
    qkv, k, v, length, ref = _case(D, G, (n, n), T)
    out = _split(qkv, G, k, v, length, chunk=chunk, pos=n)
    _check(out, ref)
    whole = ops.prefill_attention(qkv, G * HKV, k, v, length, n_kv_head=HKV)
    torch.testing.assert_close(out.float(), whole.float(), **TOL)


@pytest.mark.parametrize("kw,match", [
    ({"key_split": 0}, "multiple"),
    ({"key_split": 192}, "multiple"),
    ({"key_split": 128, "n_kv_head": None}, "no key split"),
    ({"key_split": 128, "workspace": "half"}, "workspace"),
    ({"key_split": 128, "workspace": "short"}, "workspace"),
    ({"key_split": 128, "len_bound": 9, "pos": 8}, "len_bound"),
])
def test_argument_errors(kw, match, D=64, G=4, T=2, L=16):
    B, HQ = 2, G * HKV
    KV = kw.get("n_kv_head", HKV) or HQ
    need = ops.prefill_workspace_numel(B, HQ, D, T, L, 128)
    kw = dict({"n_kv_head": HKV}, **kw)
    if "workspace" in kw:
        kw["workspace"] = (torch.ones(need, dtype=torch.float16, device=DEV)
                           if kw["workspace"] == "half" else torch.ones(need - 1, device=DEV))
    qkv = torch.randn(B, T, (HQ + 2 * KV) * D, device=DEV).bfloat16()
    k, v = (torch.zeros(B, KV, L, D, dtype=torch.bfloat16, device=DEV) for _ in "kv")
    length = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match=match):
        ops.prefill_attention(qkv, HQ, k, v, length, **kw)
    assert not k.any() and not v.any() and not length.any()
    assert "workspace" not in kw or (kw["workspace"] == 1).all()
