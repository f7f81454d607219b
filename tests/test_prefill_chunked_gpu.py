"""Chunked prefill through the model on the GPU: ``attention="flash"`` (``ops.prefill_attention``,
csrc/attn_prefill.hip) on a paged cache of 16-position pages, head dim 128."""

import pytest
import torch

from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

pytestmark = pytest.mark.gpu


def _close(got, want):
    """The bound of tests/test_decode_tp_gpu.py: 3e-2 of max|ref|."""
    err = float((got.float() - want.float()).abs().max()) / float(want.float().abs().max())
    print(f"max error / max|ref|: {err:.3e}")
    assert err < 3e-2, err


def test_chunked_flash_prefill_matches_one_shot_then_decodes():
    dev = torch.device("cuda")
    m = LLM(hidden_size=256, num_layers=2, num_heads=2, ffn_intermediate=1024,
            comm=Comm(0, 1, 0, "gloo", dev), seed=3, init_std=0.05, attention="flash")
    B, S, chunk = 2, 150, 40                            # blocks of 40, 40, 40, 30: tiles straddled
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, S + 2, 256, generator=g).bfloat16().to(dev)
    one = m.new_kv_cache(B, S + 2, page_size=16)
    chunked = m.new_kv_cache(B, S + 2, page_size=16)
    with torch.no_grad():
        want, got = m(x[:, :S], kv_cache=one), m.prefill(x[:, :S], chunked, chunk)
        assert torch.isfinite(got).all()
        _close(got, want)
        assert chunked.pos == one.pos == [S] * B and chunked.pages_in_use == one.pages_in_use
        for i in range(2):
            tok = x[:, S + i:S + i + 1]
            _close(m(tok, kv_cache=chunked), m(tok, kv_cache=one))
