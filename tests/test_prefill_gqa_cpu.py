"""Torch forms of the grouped-query chunked prefill (``ops.prefill_attention(..., n_kv_head=)`` on
CPU tensors): equal to the ungrouped torch form on the ``repeat_interleave``d cache, and two blocks
equal one block."""

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops

HKV, G, D = 2, 4, 16
HQ = HKV * G


def _rows(B, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, HQ + 2 * HKV, D, generator=g).bfloat16()


def _expanded(x):
    """[B, T, H_q + 2 H_kv, D] -> the ungrouped [B, T, 3 * H_q * D] with K / V repeated per group."""
    B, T = x.shape[:2]
    return torch.stack([x[:, :, :HQ], x[:, :, HQ:HQ + HKV].repeat_interleave(G, 2),
                        x[:, :, HQ + HKV:].repeat_interleave(G, 2)], 2).reshape(B, T, -1)


@pytest.mark.parametrize("lens", [(5, 5), (0, 9, -1, 3)])
def test_equals_ungrouped_form_on_expanded_cache(lens, T=6):
    B, top = len(lens), max(lens)
    rows = _rows(B, top + T)
    seq = len(set(lens)) > 1
    length = torch.tensor(lens if seq else lens[:1], dtype=torch.int32)
    start = torch.tensor([0 if n >= 0 else -1 for n in lens] if seq else [0], dtype=torch.int32)
    k, v = (torch.zeros(B, HKV, top + T + 2, D, dtype=torch.bfloat16) for _ in "kv")
    ke, ve = (torch.zeros(B, HQ, top + T + 2, D, dtype=torch.bfloat16) for _ in "kv")
    qkv = torch.stack([rows[b, max(n, 0):max(n, 0) + T] for b, n in enumerate(lens)])
    ops.kv_append(rows[:, :top].reshape(B, top, -1), HQ, k, v, start, n_kv_head=HKV)
    ops.kv_append(qkv.reshape(B, T, -1), HQ, k, v, length, n_kv_head=HKV)
    ops.kv_append(_expanded(rows[:, :top]), HQ, ke, ve, start)
    ops.kv_append(_expanded(qkv), HQ, ke, ve, length)
    assert torch.equal(ke, k.repeat_interleave(G, 1))
    pos = list(lens) if seq else lens[0]
    out = ops.prefill_attention(qkv.reshape(B, T, -1), HQ, k, v, length, pos=pos, n_kv_head=HKV)
    want = ops.prefill_attention(_expanded(qkv), HQ, ke, ve, length, pos=pos)
    assert out.shape == (B, T, HQ * D) and torch.equal(out, want)
    if seq:
        assert not out[2].any() and not k[2].any()             # the empty slot


def test_two_blocks_equal_one_block(n=11, cut=4):
    """Both are fp32 softmax over the same bf16 rows, rounded to bf16 once: they differ by the
    rounding of one output, at most one bf16 ulp of a value below 4 (a convex mix of unit-normal
    V entries), 2^-6."""
    rows = _rows(1, n, seed=1).reshape(1, n, -1)
    whole = None
    for blocks in ((n,), (cut, n - cut)):
        k, v = (torch.zeros(1, HKV, n, D, dtype=torch.bfloat16) for _ in "kv")
        length = torch.zeros(1, dtype=torch.int32)
        outs, at = [], 0
        for T in blocks:
            ops.kv_append(rows[:, at:at + T], HQ, k, v, length, pos=at, n_kv_head=HKV)
            outs.append(ops.prefill_attention(rows[:, at:at + T], HQ, k, v, length, pos=at,
                                              n_kv_head=HKV))
            length += T
            at += T
        out = torch.cat(outs, 1)
        if whole is None:
            whole = out
    assert whole.abs().max() < 4
    torch.testing.assert_close(out.float(), whole.float(), rtol=0, atol=2 ** -6)
