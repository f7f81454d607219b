"""Ragged decode through the tensor-parallel model on the GPU (world 1, ``attention="flash"``):
a right-padded prefill with per-row prompt lengths, decode steps over the per-sequence KV cache
and a retire-and-refill of one slot against batch-1 runs of the unpadded prompts, every step on
the HIP kernels; and the ``run_tp --prompt-lens`` record."""

import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=1024, seed=11,
          init_std=0.05, attention="flash")


def _single(m, prompt, steps, max_len):
    """A batch-1 run on a shared-length cache: the prefill output at the last prompt token, then
    ``steps`` decode steps, each fed the previous output -> [1 + steps, hidden] fp32."""
    cache = m.new_kv_cache(1, max_len)
    rows = [m(prompt[None].contiguous(), kv_cache=cache)[:, -1:]]
    for _ in range(steps):
        rows.append(m(rows[-1].contiguous(), kv_cache=cache))
    return torch.cat(rows, dim=1)[0].float()


def _close(got, want, scale, what):
    """The bound of tests/test_decode_tp_gpu.py: 3e-2 of max|ref|."""
    err = float((got.float() - want).abs().max()) / scale
    print(f"{what}: {err:.3e}")
    assert err < 3e-2, (what, err)


def test_model_ragged_prefill_decode_retire_and_refill():
    from distributed_llm_backend_benchmark_amd import ops as O
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.ops import decode as dec
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

    dev = torch.device("cuda", 0)
    m = LLM(comm=Comm(0, 1, 0, "gloo", dev), **KW)
    lens, S, steps, max_len = [1, 70, 33], 70, 3, 80
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(3, S, 256, generator=g, device=dev).to(torch.bfloat16)
    for b, n in enumerate(lens):
        x[b, n:] = 100.0                                          # padding the model must not see
    refs = [_single(m, x[b, :n], steps + 1, max_len) for b, n in enumerate(lens)]
    scale = max(float(r.abs().max()) for r in refs)

    calls = [0, 0]                                                # ragged steps, on the kernel
    real = O.decode_attention

    def counted(qkv, n_head, k_cache, v_cache, length, **kw):
        if length.numel() == 3:
            calls[0] += 1
            calls[1] += int(dec.use_hip(qkv) and dec.hip_supported(qkv, n_head, k_cache, v_cache))
        return real(qkv, n_head, k_cache, v_cache, length, **kw)

    O.decode_attention = counted
    try:
        cache = m.new_kv_cache(3, max_len, per_sequence=True)
        y = m(x, kv_cache=cache, prompt_lens=lens)
        assert cache.pos == lens and cache.length.tolist() == lens
        tok = torch.stack([y[b, n - 1] for b, n in enumerate(lens)])[:, None].contiguous()
        for b in range(3):
            _close(tok[b, 0], refs[b][0], scale, f"prefill row {b}")
        for i in range(steps):
            tok = m(tok, kv_cache=cache)
            for b in range(3):
                _close(tok[b, 0], refs[b][1 + i], scale, f"step {i} row {b}")
        assert cache.pos == [n + steps for n in lens] == cache.length.tolist()

        # a twin that never touches slot 1, from the same state
        twin = m.new_kv_cache(3, max_len, per_sequence=True)
        for mine, theirs in zip(twin.k + twin.v, cache.k + cache.v):
            mine.copy_(theirs)
        twin.set_lengths(cache.pos)
        twin.retire(1)
        twin_out = m(tok, kv_cache=twin)

        cache.retire(1)
        new = torch.randn(21, 256, generator=g, device=dev).to(torch.bfloat16)
        fresh = _single(m, new, 1, max_len)
        slot = cache.slot(1)
        slot.set_length(0)
        y1 = m(new[None].contiguous(), kv_cache=slot)
        assert cache.pos == [lens[0] + steps, 21, lens[2] + steps] == cache.length.tolist()
        _close(y1[0, -1], fresh[0], scale, "refill prefill")
        tok = torch.cat([tok[0:1], y1[:, -1:], tok[2:3]]).contiguous()
        out = m(tok, kv_cache=cache)
    finally:
        O.decode_attention = real
    torch.cuda.synchronize()
    assert calls == [(steps + 2) * 2, (steps + 2) * 2], calls     # every layer of every ragged step
    for b in (0, 2):                                              # as if slot 1 was never touched
        assert torch.equal(out[b], twin_out[b]), b
        _close(out[b, 0], refs[b][1 + steps], scale, f"after the refill, row {b}")
    _close(out[1, 0], fresh[1], scale, "refilled row")
    assert cache.pos == [lens[0] + steps + 1, 22, lens[2] + steps + 1] == cache.length.tolist()


def _cfg(tmp_path):
    import yaml

    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "baseline_config.yaml")))
    cfg["model"].update(hidden_size=512, num_layers=2, num_heads=8, ffn_intermediate=2048,
                        init_std=0.02)
    cfg["input"].update(batch_size=2, sequence_length=64)
    cfg["execution"].update(warmup_iterations=1, benchmark_iterations=3)
    cfg["parallelism"]["world_size"] = 1
    cfg["experiment"]["output_dir"] = str(tmp_path)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return p, cfg["experiment"]["name"]


def test_run_tp_prompt_lens_record(tmp_path):
    p, name = _cfg(tmp_path)
    out = subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                          "--config", str(p), "--backend", "rccl", "--decode", "8", "--attention",
                          "flash", "--prompt-lens", "17,64"],
                         capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    files = [f for f in os.listdir(tmp_path) if f.endswith(".json")]
    assert files == [f"rccl_{name}_decode8_ragged.json"], files
    d = json.load(open(tmp_path / files[0]))["decode"]
    assert d["prompt_lengths"] == [17, 64]
    assert d["timing_mode"] == "hip_graph_replay", d["hip_graph_note"]
    assert d["attention_path"] == "hip" and d["kv_dtype"] == "bf16"
    assert (d["prompt_len"], d["new_tokens"], d["max_len"]) == (64, 8, 72)
    assert d["kv_cache_bytes_per_rank"] == 2 * 2 * 2 * 8 * 72 * 64 * 2
    # step i of row b reads positions [0, L_b + i]: 2 layers x 8 heads x 64 bf16 columns, K and V
    assert d["kv_bytes_read_per_step_mean"] == ((17 + 4.5) + (64 + 4.5)) * 2 * 8 * 64 * 2 * 2
    assert len(d["ms_per_token"]) == 3 and all(v > 0 for v in d["ms_per_token"])
