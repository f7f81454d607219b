"""Torch forms of ``rope=`` (``ops.kv_append`` / ``decode_attention`` / ``prefill_attention`` on CPU
tensors with grouped heads) against the fp64 reference of ``gqa_rope_utils``: Q and K rotated in
fp64 and rounded to bf16, fp64 softmax. The bound is the GQA tests' (bf16 output of an fp32
softmax over the same bf16 rows; a rotated Q / K entry differs from the reference's by at most one
bf16 ulp)."""

import pytest
import torch

import gqa_rope_utils as U
from distributed_llm_backend_benchmark_amd import ops

HKV = 2
TOL = dict(rtol=2e-2, atol=2e-2)


def _run(D, G, lens, T, W=None, **extra):
    """Append [0, len_b), then the block of T tokens, then attend -> (out, k, v, per-row refs)."""
    B, HQ, top = len(lens), G * HKV, max(lens)
    g = torch.Generator().manual_seed(D + G + T + sum(lens))
    rows = torch.randn(B, top + T, HQ + 2 * HKV, D, generator=g).bfloat16()
    rope = U.table(top + T, D)
    kw = dict(n_kv_head=HKV, **({"rope": rope} if extra.pop("with_rope", True) else {}), **extra)
    k, v = (torch.zeros(B, HKV, top + T, D, dtype=torch.bfloat16) for _ in "kv")
    seq = len(set(lens)) > 1
    length = torch.tensor(lens if seq else lens[:1], dtype=torch.int32)
    start = torch.tensor([0 if n >= 0 else -1 for n in lens] if seq else [0], dtype=torch.int32)
    qkv = torch.stack([rows[b, max(n, 0):max(n, 0) + T] for b, n in enumerate(lens)])
    qkv = qkv.reshape(B, T, -1)
    ops.kv_append(rows[:, :top].reshape(B, top, -1), HQ, k, v, start, **kw)
    if W is not None:
        kw["window"] = W
    if T == 1:
        out = ops.decode_attention(qkv, HQ, k, v, length, **kw)
    else:
        ops.kv_append(qkv, HQ, k, v, length, **{x: y for x, y in kw.items() if x != "window"})
        out = ops.prefill_attention(qkv, HQ, k, v, length, **kw)
    ref = [None if n < 0 else U.reference(rows[b, :n + T], rope, n, T, G, HKV, W)
           for b, n in enumerate(lens)]
    return out, k, v, ref


@pytest.mark.parametrize("D,G,lens,T,W", [(16, 4, (9, 9), 1, None), (32, 2, (0, 9, -1, 3), 6, 5),
                                          (16, 4, (0, 9, -1, 3), 1, 4), (32, 2, (7, 7), 6, None)])
def test_torch_forms(D, G, lens, T, W):
    out, k, v, ref = _run(D, G, lens, T, W)
    for b, r in enumerate(ref):
        if r is None:
            assert not out[b].any() and not k[b].any() and not v[b].any()
        else:
            torch.testing.assert_close(out[b].double(), r, **TOL)


@pytest.mark.parametrize("T", [1, 6])
def test_rope_none_is_the_call_without_it(T, D=16, G=4, lens=(9, 9)):
    a = _run(D, G, lens, T, with_rope=False)
    b = _run(D, G, lens, T, with_rope=False, rope=None)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert not torch.equal(a[1], _run(D, G, lens, T)[1])       # and the table does rotate K
