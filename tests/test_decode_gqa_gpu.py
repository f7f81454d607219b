"""Grouped-query decode (``ops.decode_attention(..., n_kv_head=)``, ``csrc/attn_decode_gqa.hip``)
against a plain fp32 softmax on the same bf16 bits. The cache is NaN past every live row, so a load
past the live range or a masked row reaching the PV product shows as NaN; it is filled by
``ops.kv_append(..., n_kv_head=)`` from a block of T > 1 tokens and compared with the source rows bit
for bit. bf16 P against an fp32 row sum costs at most 2^-8 * sum_k p_k |v_k| (0.003 for unit
normal V, 0.013 with the group-mapping case's 4 x rows): inside the decode tests' bound."""

import math

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.ops.decode import CHUNK_GQA

pytestmark = pytest.mark.gpu

HKV, NAN, DEV = 2, float("nan"), "cuda"
TOL = dict(rtol=2e-2, atol=2e-2)     # the project's decode and prefill bound: bf16 P, bf16 output
LENS = (0, 1, 37, CHUNK_GQA - 1, CHUNK_GQA, CHUNK_GQA + 1, 2 * CHUNK_GQA + 70)


def _case(D, G, lens, slack=5, head_scale=1.0):
    """rows [B, max(len) + 1, H_q + 2 H_kv, D] bf16 (row ``len_b`` is the decoded token); the NaN
    cache holding rows [0, len_b) of every live row, appended as one block; the fp32 reference."""
    B, HQ, n = len(lens), G * HKV, max(max(lens), 0)
    g = torch.Generator().manual_seed(1000 * D + 10 * G + n)
    rows = torch.randn(B, n + 1, HQ + 2 * HKV, D, generator=g)
    rows[:, :, [HQ + 1, HQ + HKV + 1]] *= head_scale           # K and V of KV head 1
    rows = rows.bfloat16().to(DEV)
    k, v = (torch.full((B, HKV, n + 1 + slack, D), NAN, dtype=torch.bfloat16, device=DEV)
            for _ in "kv")
    if n > 0:
        start = torch.tensor([0 if m >= 0 else -1 for m in lens] if B > 2 else [0],
                             dtype=torch.int32, device=DEV)
        ops.kv_append(rows[:, :n].reshape(B, n, -1), HQ, k, v, start, n_kv_head=HKV)
    ref = torch.zeros(B, HQ * D, device=DEV)
    for b, m in enumerate(lens):
        if m < 0:
            continue
        k[b, :, m:], v[b, :, m:] = NAN, NAN                    # a shorter row of a ragged batch
        x = rows[b, :m + 1].float()
        kv_of = torch.arange(HQ, device=DEV) // G              # query head h -> KV head h // G
        s = torch.einsum("hd,khd->hk", x[m, :HQ], x[:, HQ + kv_of]) / math.sqrt(D)
        ref[b] = torch.einsum("hk,khd->hd", s.softmax(-1), x[:, HQ + HKV + kv_of]).flatten()
    return rows, k, v, ref


def _decode(rows, k, v, lens, G, **kw):
    B = rows.shape[0]
    qkv = torch.stack([rows[b, max(m, 0)] for b, m in enumerate(lens)]).reshape(B, 1, -1)
    length = torch.tensor(lens if B > 2 else lens[:1], dtype=torch.int32, device=DEV)
    return ops.decode_attention(qkv, G * HKV, k, v, length, n_kv_head=HKV, **kw)[:, 0]


@pytest.mark.parametrize("D,G,n,slack", [(D, G, n, 5) for D in (64, 128) for G in (2, 4, 8, 16)
                                         for n in LENS] + [(128, 4, 37, 0)])
def test_shared_length(D, G, n, slack):
    rows, k, v, ref = _case(D, G, (n, n), slack)
    out = _decode(rows, k, v, (n, n), G)
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out.float(), ref, **TOL)
    assert torch.equal(out, _decode(rows, k, v, (n, n), G))
    HQ = G * HKV                                               # the append: the source rows' bits
    assert torch.equal(k[:, :, :n + 1], rows[:, :, HQ:HQ + HKV].transpose(1, 2))
    assert torch.equal(v[:, :, :n + 1], rows[:, :, HQ + HKV:].transpose(1, 2))
    assert k[:, :, n + 1:].isnan().all() and v[:, :, n + 1:].isnan().all()


@pytest.mark.parametrize("D", [64, 128])
def test_per_sequence(D, G=4, lens=(0, 37, -1, 300)):
    rows, k, v, ref = _case(D, G, lens)
    out = _decode(rows, k, v, lens, G)
    torch.testing.assert_close(out.float(), ref, **TOL)
    assert not out[2].any() and k[2].isnan().all() and v[2].isnan().all()    # the empty slot
    for b in (0, 1, 3):                                        # the bits of a batch-1 shared launch
        one = _decode(rows[b:b + 1], k[b:b + 1], v[b:b + 1], lens[b:b + 1], G)
        assert torch.equal(out[b:b + 1], one)


def test_group_mapping(D=128, G=4, n=37):
    rows, k, v, ref = _case(D, G, (n, n), head_scale=4.0)      # h % H_kv would pick the other scale
    torch.testing.assert_close(_decode(rows, k, v, (n, n), G).float(), ref, **TOL)


def test_against_expanded_cache(D=128, G=4, n=300):
    rows, k, v, _ = _case(D, G, (n, n))
    out = _decode(rows, k, v, (n, n), G)
    HQ = G * HKV
    tok = rows[:, n]
    mha = torch.stack([tok[:, :HQ], tok[:, HQ:HQ + HKV].repeat_interleave(G, 1),
                       tok[:, HQ + HKV:].repeat_interleave(G, 1)], 1).reshape(2, 1, -1)
    length = torch.tensor([n], dtype=torch.int32, device=DEV)
    want = ops.decode_attention(mha, HQ, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1),
                                length)[:, 0]
    torch.testing.assert_close(out.float(), want.float(), **TOL)


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
    qkv = torch.randn(B, 1, (HQ + 2 * KV) * D, device=DEV).bfloat16()
    k, v = (torch.zeros(B, KV, L, D, dtype=torch.bfloat16, device=DEV) for _ in "kv")
    length = torch.zeros(1, dtype=torch.int32, device=DEV)
    for fn in (ops.kv_append, ops.decode_attention):
        with pytest.raises(ValueError, match="not built yet" if extra else "multiple|group"):
            fn(qkv, HQ, k, v, length, n_kv_head=KV, **extra)
    assert not k.any() and not v.any()
