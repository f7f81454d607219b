"""Grouped-query chunked prefill (``ops.prefill_attention(..., n_kv_head=)``,
``csrc/attn_prefill_gqa.hip``): a block of T tokens of G * H_kv query heads over a grouped KV cache
under a bottom-right causal mask, against a plain fp32 softmax on the same bf16 bits. The caches
are NaN everywhere except the live rows, which ``ops.kv_append(..., n_kv_head=)`` wrote: a load
past the live range, or a masked row that reaches the PV product, shows as NaN. The two KV heads
are independent random data, so a wrong head mapping (``h % H_kv``) fails the comparison. The
per-row arithmetic is the ungrouped prefill kernel's, which meets TOL on the same data scale."""

import functools
import math

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops

pytestmark = pytest.mark.gpu

HKV, NAN, DEV = 2, float("nan"), "cuda"
TOL = dict(rtol=2e-2, atol=2e-2)     # the project's prefill bound: bf16 P, bf16 output


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
    """qkv [B, T, (H_q + 2 H_kv) * D] of the block, NaN caches holding rows [0, len_b + T) of every
    live row (prefix and block both appended by ``ops.kv_append``), the device lengths and the
    fp32 reference per row (None for an empty slot)."""
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


def _check(out, ref):
    for b, r in enumerate(ref):
        if r is None:
            assert not out[b].any()
        else:
            assert torch.isfinite(out[b]).all()
            torch.testing.assert_close(out[b].float().cpu(), r, **TOL)


@pytest.mark.parametrize("D,G,T,n,slack", [
    (D, G, T, n, 5) for D in (64, 128) for G in (2, 4, 8, 16)
    for T in (1, 32 // G + 1, 128 // G + 3, 2 * (128 // G) + 5)
    for n in (0, 8192 // (2 * D) - 1, 257)] + [(128, 4, 35, 257, 0)])      # + L_max == n + T
def test_shared_length(D, G, T, n, slack):
    qkv, k, v, length, ref = _case(D, G, (n, n), T, slack)
    out = ops.prefill_attention(qkv, G * HKV, k, v, length, pos=n, n_kv_head=HKV)
    _check(out, ref)
    assert torch.equal(out, ops.prefill_attention(qkv, G * HKV, k, v, length, n_kv_head=HKV))


@pytest.mark.parametrize("D", [64, 128])
def test_per_sequence(D, G=4, lens=(0, 37, -1, 300), T=70):
    qkv, k, v, length, ref = _case(D, G, lens, T)
    out = ops.prefill_attention(qkv, G * HKV, k, v, length, pos=lens, n_kv_head=HKV)
    _check(out, ref)
    assert k[2].isnan().all() and v[2].isnan().all()           # the empty slot
    for b in (0, 1, 3):                                        # the bits of a batch-1 shared launch
        one = ops.prefill_attention(qkv[b:b + 1], G * HKV, k[b:b + 1], v[b:b + 1],
                                    length[b:b + 1], pos=lens[b], n_kv_head=HKV)
        assert torch.equal(out[b:b + 1], one)


def test_against_expanded_cache(D=128, G=4, n=300, T=40):
    qkv, k, v, length, _ = _case(D, G, (n, n), T)
    HQ = G * HKV
    out = ops.prefill_attention(qkv, HQ, k, v, length, n_kv_head=HKV)
    x = qkv.view(2, T, HQ + 2 * HKV, D)
    mha = torch.stack([x[:, :, :HQ], x[:, :, HQ:HQ + HKV].repeat_interleave(G, 2),
                       x[:, :, HQ + HKV:].repeat_interleave(G, 2)], 2).reshape(2, T, -1)
    want = ops.prefill_attention(mha, HQ, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1),
                                 length)
    torch.testing.assert_close(out.float(), want.float(), **TOL)


def test_prefill_then_decode(D=128, G=8, blocks=(20, 17)):
    HQ, n = G * HKV, sum(blocks)
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(1, n + 1, HQ + 2 * HKV, D, generator=g).mul(1.5).bfloat16()
    k, v = (torch.full((1, HKV, n + 6, D), NAN, dtype=torch.bfloat16, device=DEV) for _ in "kv")
    length = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs, at = [], 0
    for T in blocks:                                           # append, attend, advance
        qkv = rows[:, at:at + T].reshape(1, T, -1).to(DEV)
        ops.kv_append(qkv, HQ, k, v, length, pos=at, n_kv_head=HKV)
        outs.append(ops.prefill_attention(qkv, HQ, k, v, length, pos=at, n_kv_head=HKV))
        length += T
        at += T
    step = ops.decode_attention(rows[:, n:].reshape(1, 1, -1).to(DEV), HQ, k, v, length, pos=n,
                                n_kv_head=HKV)
    out = torch.cat(outs + [step], 1)[0]
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out.float().cpu(), _reference(rows[0], 0, n + 1, G), **TOL)


@pytest.mark.parametrize("heads,extra", [
    ((6, 4), {}),                                              # n_head % n_kv_head != 0
    ((6, 2), {}),                                              # a group of 3
    ((8, 2), {"block_table": "table"}),
    ((8, 2), {"k_scale": "scale", "v_scale": "scale"}),
])
def test_argument_errors(heads, extra, D=64, L=8):
    (HQ, KV), B = heads, 2
    dummy = {"table": torch.zeros(B, 1, dtype=torch.int32, device=DEV),
             "scale": torch.ones(B, KV, L, device=DEV)}
    extra = {key: dummy[name] for key, name in extra.items()}
    qkv = torch.randn(B, 2, (HQ + 2 * KV) * D, device=DEV).bfloat16()
    k, v = (torch.zeros(B, KV, L, D, dtype=torch.bfloat16, device=DEV) for _ in "kv")
    length = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="not built yet" if extra else "multiple|group"):
        ops.prefill_attention(qkv, HQ, k, v, length, n_kv_head=KV, **extra)
    assert not k.any() and not v.any() and not length.any()
