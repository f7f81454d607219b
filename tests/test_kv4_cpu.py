"""The MXFP4 KV cache off the GPU: ``KVCache(kv_dtype="mxfp4")``, the torch forms of ``kv_append`` /
``decode_attention`` against an fp32 softmax over the dequantised codes, the refusals, the config
knob and the model's cache."""

import copy
import math

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.ops import decode as dec
from distributed_llm_backend_benchmark_amd.ops.decode import CHUNK_MXFP4, KVCache
from distributed_llm_backend_benchmark_amd.ops.mxfp4 import _quantize_rows, dequantize_mxfp4
from distributed_llm_backend_benchmark_amd.utils.config import (DEFAULT_CONFIG, ConfigError,
                                                                validate_config)

U8 = torch.uint8


@pytest.mark.parametrize("D", [64, 128])
def test_kvcache_mxfp4_shapes_and_bytes(D):
    c = KVCache(2, 3, 4, D, 300, "cpu", kv_dtype="mxfp4")
    assert dec.KV_DTYPES == ("bf16", "fp8", "mxfp4")
    for t, s in zip(c.k + c.v, c.k_scale + c.v_scale):
        assert t.dtype == U8 and tuple(t.shape) == (3, 4, 300, D // 2) and not t.any()
        assert s.dtype == U8 and tuple(s.shape) == (3, 4, 300, D // 32) and (s == 127).all()
    assert c.nbytes == 2 * 2 * 3 * 4 * 300 * (D // 2 + D // 32)
    assert c.workspace.numel() == dec.workspace_numel(3, 4, D, 300, CHUNK_MXFP4)
    c.set_length(7)
    assert c.live_bytes() == 3 * 7 * 2 * 2 * 4 * (D // 2 + D // 32)


def test_refusals():
    with pytest.raises(ValueError):
        KVCache(1, 1, 2, 64, 32, "cpu", kv_dtype="int8")
    with pytest.raises(ValueError):
        KVCache(1, 1, 2, 64, 32, "cpu", kv_dtype="mxfp4", page_size=16)
    with pytest.raises(ValueError):
        KVCache(1, 1, 2, 64, 32, "cpu", kv_dtype="mxfp4", n_q_head=4)
    c = KVCache(1, 2, 2, 64, 32, "cpu", kv_dtype="mxfp4", per_sequence=True)
    kw = dict(k_scale=c.k_scale[0], v_scale=c.v_scale[0])
    qkv = torch.randn(2, 1, 3 * 2 * 64).to(torch.bfloat16)
    table = torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="paged MXFP4"):
        ops.kv_append(qkv, 2, c.k[0], c.v[0], c.length, block_table=table, **kw)
    with pytest.raises(ValueError, match="paged MXFP4"):
        ops.decode_attention(qkv, 2, c.k[0], c.v[0], c.length, block_table=table, **kw)
    with pytest.raises(ValueError, match="prefill over an MXFP4"):
        ops.prefill_attention(qkv, 2, c.k[0], c.v[0], c.length, **kw)
    gq = torch.randn(2, 1, (4 + 2 * 2) * 64).to(torch.bfloat16)
    for fn in (ops.kv_append, ops.decode_attention, ops.prefill_attention):
        with pytest.raises(ValueError, match="GQA"):
            fn(gq, 4, c.k[0], c.v[0], c.length, n_kv_head=2, **kw)
    with pytest.raises(ValueError, match="D/32"):                 # a scale plane of the wrong width
        ops.decode_attention(qkv, 2, c.k[0], c.v[0], c.length, k_scale=c.k_scale[0][..., :1],
                             v_scale=c.v_scale[0][..., :1])
    with pytest.raises(ValueError, match="needs its uint8"):
        ops.kv_append(qkv, 2, c.k[0], c.v[0], c.length)


@pytest.mark.parametrize("seq", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_torch_append_and_decode_match_fp32_over_the_codes(D, seq):
    """The torch forms: the append stores ``_quantize_rows``' bits, the decode is within 2^-7 of
    max|want| of an fp32 softmax over the dequantised codes (one bf16 rounding of the output)."""
    B, H, T, L_max = 3, 2, 37, 48
    g = torch.Generator().manual_seed(D + seq)
    c = KVCache(1, B, H, D, L_max, "cpu", kv_dtype="mxfp4", per_sequence=seq)
    kc, vc, ks, vs = c.k[0], c.v[0], c.k_scale[0], c.v_scale[0]
    start = [2, -1, 5] if seq else [4] * B
    if seq:
        c.set_lengths(start)
    else:
        c.set_length(4)
    qkv = torch.randn(B, T, 3, H, D, generator=g).to(torch.bfloat16)
    ops.kv_append(qkv.view(B, T, -1), H, kc, vc, c.length, pos=c.pos, k_scale=ks, v_scale=vs)
    c.advance(T)
    step = torch.randn(B, 1, 3, H, D, generator=g).to(torch.bfloat16)
    got = ops.decode_attention(step.view(B, 1, -1), H, kc, vc, c.length, pos=c.pos, k_scale=ks,
                               v_scale=vs).view(B, H, D).float()
    for b, p in enumerate(start):
        if p < 0:
            assert not got[b].any() and not kc[b].any() and (ks[b] == 127).all()
            continue
        rows = torch.cat([qkv[b], step[b]])                       # [T + 1, 3, H, D]
        for j, (cache, scale) in ((1, (kc, ks)), (2, (vc, vs))):
            code, s = _quantize_rows(rows[:, j].transpose(0, 1).float().reshape(-1, D))
            assert torch.equal(cache[b, :, p:p + T + 1].reshape(-1, D // 2), code)
            assert torch.equal(scale[b, :, p:p + T + 1].reshape(-1, D // 32), s)
        n = p + T + 1
        K, V = (dequantize_mxfp4(t[b, :, :n].reshape(-1, D // 2), s[b, :, :n].reshape(-1, D // 32))
                .view(H, n, D) for t, s in ((kc, ks), (vc, vs)))
        w = torch.softmax((step[b, 0, 0].float()[:, None] * K).sum(-1) / math.sqrt(D), -1)
        want = (w[..., None] * V).sum(1)
        assert float((got[b] - want).abs().max() / want.abs().max()) <= 2.0 ** -7


def test_config_and_model():
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

    def config(**ex):
        raw = copy.deepcopy(DEFAULT_CONFIG)
        raw["execution"].update({"kv_cache_dtype": "mxfp4", **ex})
        return raw

    assert validate_config(config())["execution"]["kv_cache_dtype"] == "mxfp4"
    for extra in (dict(prefill_chunk=16), dict(kv_page_size=16), dict(kv_cache_dtype="int8")):
        with pytest.raises(ConfigError):
            validate_config(config(**extra))
    kw = dict(hidden_size=128, num_layers=1, num_heads=2, ffn_intermediate=256,
              comm=Comm(0, 1, 0, "gloo", torch.device("cpu")), attention="sdpa")
    with pytest.raises(ValueError):
        LLM(kv_cache_dtype="int8", **kw)
    model = LLM(kv_cache_dtype="mxfp4", **kw)
    cache = model.new_kv_cache(2, 12)
    x = torch.randn(2, 12, 128).to(torch.bfloat16)
    y = torch.cat([model(x[:, :8].contiguous(), kv_cache=cache)] +
                  [model(x[:, t:t + 1].contiguous(), kv_cache=cache) for t in range(8, 12)], 1)
    assert cache.kv_dtype == "mxfp4" and cache.k[0].dtype == U8 and cache.pos == 12
    assert tuple(cache.k_scale[0].shape) == (2, 2, 12, 2) and torch.isfinite(y.float()).all()
    assert cache.k[0].any() and (cache.k_scale[0] != 127).any()
    cache.set_length(4)
    with pytest.raises(ValueError, match="bf16"):                  # chunked prefill: bf16 only
        model(x[:, :4].contiguous(), kv_cache=cache, extend=True)
