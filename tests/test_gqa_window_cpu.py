"""``window=`` on CPU tensors (the torch forms of ``ops.decode_attention`` and
``ops.prefill_attention``) on the inputs and against the fp32 band-masked reference of
tests/test_gqa_window_gpu.py: the two agree before a kernel is held to them."""

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from test_gqa_window_gpu import HKV, _case, _check


@pytest.mark.parametrize("lens,T,W", [((40, 40), 1, 16), ((0, 37, -1, 90), 1, 30),
                                      ((40, 40), 9, 16), ((0, 37, -1, 90), 20, 30)])
def test_torch_forms_match_the_band_masked_reference(lens, T, W, D=64, G=4):
    qkv, k, v, length, ref = _case(D, G, lens, T, W, dev="cpu")
    fn = ops.decode_attention if T == 1 else ops.prefill_attention
    _check(fn(qkv, G * HKV, k, v, length, n_kv_head=HKV, window=W), ref)


@pytest.mark.parametrize("T", [1, 9])
def test_window_none_is_the_call_without_it(T, D=64, G=4, n=40):
    qkv, k, v, length, _ = _case(D, G, (n, n), T, n + T, dev="cpu")
    fn = ops.decode_attention if T == 1 else ops.prefill_attention
    out = fn(qkv, G * HKV, k, v, length, n_kv_head=HKV)
    assert torch.equal(out, fn(qkv, G * HKV, k, v, length, n_kv_head=HKV, window=None))
