"""Chunked prefill, CPU side (torch path; gloo world 1): ``LLM.prefill`` in blocks equals the
one-shot prefill and leaves the cache where it does, ``extend=False`` still refuses, an FP8 cache
raises, and the config / CLI plumbing of ``prefill_chunk``."""

import copy
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=3e-2, atol=3e-2)        # the project's TP-vs-dense bound
B, S, LENS = 2, 24, [9, 24]


def _model(**kw):
    comm = Comm(0, 1, 0, "gloo", torch.device("cpu"))
    return LLM(hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=1024, comm=comm,
               seed=3, init_std=0.05, kernels="torch", attention="sdpa", **kw)


def _x(T=S):
    return torch.randn(B, T, 256, generator=torch.Generator().manual_seed(7)).bfloat16()


@pytest.mark.parametrize("cache_kw", [{}, {"per_sequence": True}, {"page_size": 16}])
def test_chunked_prefill_matches_one_shot_and_the_next_decode_step(cache_kw):
    m, x, tok = _model(), _x(), _x(1)
    one, chunked = m.new_kv_cache(B, S + 1, **cache_kw), m.new_kv_cache(B, S + 1, **cache_kw)
    want, got = m(x, kv_cache=one), m.prefill(x, chunked, chunk=5)
    torch.testing.assert_close(got.float(), want.float(), **TOL)
    assert chunked.pos == one.pos and torch.equal(chunked.length, one.length)
    torch.testing.assert_close(m(tok, kv_cache=chunked).float(), m(tok, kv_cache=one).float(),
                               **TOL)


@pytest.mark.parametrize("cache_kw", [{"per_sequence": True}, {"page_size": 16}])
def test_padded_chunked_prefill_ends_where_the_one_shot_does(cache_kw):
    m, x, tok = _model(), _x(), _x(1)
    one, chunked = m.new_kv_cache(B, S + 1, **cache_kw), m.new_kv_cache(B, S + 1, **cache_kw)
    want, got = m(x, kv_cache=one, prompt_lens=LENS), m.prefill(x, chunked, 5, prompt_lens=LENS)
    assert chunked.pos == one.pos == LENS and torch.equal(chunked.length, one.length)
    if chunked.paged:
        assert chunked.pages_in_use == one.pages_in_use == 1 + 2
    for b, n in enumerate(LENS):                         # the real tokens; padding rows are free
        torch.testing.assert_close(got[b, :n].float(), want[b, :n].float(), **TOL)
    torch.testing.assert_close(m(tok, kv_cache=chunked).float(), m(tok, kv_cache=one).float(),
                               **TOL)


def test_extend_is_opt_in_and_refuses_an_fp8_cache():
    m, x = _model(), _x()
    cache = m.new_kv_cache(B, S)
    m(x[:, :8], kv_cache=cache)
    with pytest.raises(ValueError, match="chunked prefill"):
        m(x[:, 8:12], kv_cache=cache)                    # extend=False: as before
    m(x[:, 8:12], kv_cache=cache, extend=True)
    assert cache.pos == 12
    m8 = _model(kv_cache_dtype="fp8")
    c8 = m8.new_kv_cache(B, S)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        m8.prefill(x, c8, chunk=5)
    m8(x[:, :8], kv_cache=c8)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        m8(x[:, 8:12], kv_cache=c8, extend=True)
    assert c8.pos == 8


def test_config_accepts_prefill_chunk_and_has_no_default():
    from distributed_llm_backend_benchmark_amd.utils.config import (DEFAULT_CONFIG, ConfigError,
                                                                    validate_config)

    cfg = copy.deepcopy(DEFAULT_CONFIG)
    assert "prefill_chunk" not in validate_config(cfg)["execution"]
    cfg["execution"]["prefill_chunk"] = 512
    assert validate_config(cfg)["execution"]["prefill_chunk"] == 512
    for bad in (0, -4, True, "8", 1.5):
        cfg["execution"]["prefill_chunk"] = bad
        with pytest.raises(ConfigError):
            validate_config(cfg)
    cfg["execution"].update(prefill_chunk=8, kv_cache_dtype="fp8")
    with pytest.raises(ConfigError):
        validate_config(cfg)


def test_run_tp_prefill_chunk_record_and_refusal(tmp_path):
    import yaml

    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "baseline_config.yaml")))
    cfg["model"].update(hidden_size=64, num_layers=2, num_heads=2, ffn_intermediate=128,
                        init_std=0.05)
    cfg["input"].update(batch_size=2, sequence_length=28)
    cfg["execution"].update(warmup_iterations=1, benchmark_iterations=2, attention="sdpa",
                            kernels="torch")
    cfg["parallelism"]["world_size"] = 1
    cfg["experiment"]["output_dir"] = str(tmp_path)
    (tmp_path / "c.yaml").write_text(yaml.safe_dump(cfg))

    def run(*extra):
        return subprocess.run([sys.executable, "-m",
                               "distributed_llm_backend_benchmark_amd.cli.run_tp", "--config",
                               str(tmp_path / "c.yaml"), "--backend", "gloo", "--device", "cpu",
                               *extra], capture_output=True, text=True, timeout=600, cwd=REPO)

    out = run("--prefill-chunk", "8")                    # no --decode: no cache to extend
    assert out.returncode == 1 and "--prefill-chunk" in out.stdout
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".json")]
    out = run("--decode", "4", "--prompt-lens", "5,28", "--kv-page-size", "16",
              "--prefill-chunk", "8")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    files = [f for f in os.listdir(tmp_path) if f.endswith(".json")]
    assert len(files) == 1 and files[0].endswith("_decode4_ragged_paged16_chunk8.json"), files
    d = json.load(open(tmp_path / files[0]))["decode"]
    assert d["prefill_chunk"] == 8 and d["prefill_ms"] > 0 and d["kv_pages_peak"] == 3
