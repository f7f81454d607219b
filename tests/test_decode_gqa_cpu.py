"""Grouped-query decode on CPU tensors: the torch forms behind ``n_kv_head=`` against a plain fp32
softmax, the ``KVCache(n_q_head=)`` workspace, and the unchanged default."""

import math

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.ops import decode

TOL = dict(rtol=2e-2, atol=2e-2)


def _rows(B, n, heads, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n + 1, heads, D, generator=g).bfloat16()


@pytest.mark.parametrize("D,HQ,KV,lens", [(64, 4, 2, (9,)), (128, 8, 1, (9,)),
                                          (64, 4, 2, (0, 9, -1)), (128, 8, 1, (5, -1, 9))])
def test_torch_forms_match_fp32_softmax(D, HQ, KV, lens):
    B, n, G = max(len(lens), 2), max(lens), HQ // KV
    lens = lens * 2 if len(lens) == 1 else lens                # one length: shared by two rows
    rows = _rows(B, n, HQ + 2 * KV, D, D + HQ)
    k, v = (torch.full((B, KV, n + 2, D), float("nan"), dtype=torch.bfloat16) for _ in "kv")
    shared = len(set(lens)) == 1
    start = torch.tensor([0] if shared else [0 if m >= 0 else -1 for m in lens], dtype=torch.int32)
    ops.kv_append(rows[:, :n].reshape(B, n, -1), HQ, k, v, start, n_kv_head=KV)
    qkv = torch.stack([rows[b, max(m, 0)] for b, m in enumerate(lens)]).reshape(B, 1, -1)
    length = torch.tensor(lens[:1] if shared else lens, dtype=torch.int32)
    out = ops.decode_attention(qkv, HQ, k, v, length, n_kv_head=KV)[:, 0]
    for b, m in enumerate(lens):
        if m < 0:
            assert not out[b].any() and k[b].isnan().all()
            continue
        x, kv_of = rows[b, :m + 1].float(), torch.arange(HQ) // G
        s = torch.einsum("hd,khd->hk", x[m, :HQ], x[:, HQ + kv_of]) / math.sqrt(D)
        ref = torch.einsum("hk,khd->hd", s.softmax(-1), x[:, HQ + KV + kv_of]).flatten()
        torch.testing.assert_close(out[b].float(), ref, **TOL)
        assert torch.equal(k[b, :, m], rows[b, m, HQ:HQ + KV])  # the token, stored at `length`


def test_kvcache_sizes_the_workspace_by_the_query_heads():
    c = ops.KVCache(1, 2, 2, 64, 700, "cpu", n_q_head=8)
    assert (c.n_head, c.n_q_head) == (2, 8) and c.k[0].shape == (2, 2, 700, 64)
    assert c.workspace.numel() == decode.workspace_numel(2, 8, 64, 700, decode.CHUNK_GQA)
    d = ops.KVCache(1, 2, 2, 64, 700, "cpu")
    assert d.n_q_head == 2
    assert d.workspace.numel() == decode.workspace_numel(2, 2, 64, 700, decode.CHUNK)
    with pytest.raises(ValueError, match="not built yet"):
        ops.KVCache(1, 2, 2, 64, 700, "cpu", kv_dtype="fp8", n_q_head=8)


@pytest.mark.parametrize("n_kv_head", [None, 4])
def test_default_is_todays_call(n_kv_head, H=4, D=64, n=9):
    rows = _rows(2, n, 3 * H, D, 5)
    length, outs = torch.tensor([n], dtype=torch.int32), []
    for kw in ({}, {"n_kv_head": n_kv_head}):
        k, v = (torch.zeros(2, H, n + 2, D, dtype=torch.bfloat16) for _ in "kv")
        ops.kv_append(rows[:, :n].reshape(2, n, -1), H, k, v, length * 0, **kw)
        outs.append((ops.decode_attention(rows[:, n:].reshape(2, 1, -1), H, k, v, length, **kw),
                     k, v))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
