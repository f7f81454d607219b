"""The paged KV cache through the tensor-parallel model on the GPU (world 1, ``attention="flash"``):
a right-padded prefill with per-row prompt lengths and decode steps over a page pool of exactly the
needed pages, against the same model on a contiguous per-sequence cache, bit for bit at every row's
real positions; bf16 and FP8 caches, head dims 128 and 64, every step on the paged HIP kernels; and
the ``run_tp --kv-page-size`` record under HIP-graph replay."""

import json
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

P, STEPS = 16, 3
LENS, T = [3, 17, 16, 9], 17


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("heads", [2, 4])                          # head dims 128 and 64
def test_model_paged_equals_contiguous(heads, kv_dtype):
    from distributed_llm_backend_benchmark_amd import ops as O
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

    dev = torch.device("cuda", 0)
    m = LLM(comm=Comm(0, 1, 0, "gloo", dev), hidden_size=256, num_layers=2, num_heads=heads,
            ffn_intermediate=1024, seed=11, init_std=0.05, attention="flash",
            kv_cache_dtype=kv_dtype)
    B, max_len = len(LENS), 2 * P                                  # the cap of both caches
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(B, T, 256, generator=g, device=dev).to(torch.bfloat16)
    for b, n in enumerate(LENS):
        x[b, n:] = 100.0                                           # padding the model must not see
    need = sum((n + STEPS + P - 1) // P for n in LENS)             # 1 + 2 + 2 + 1
    flat = m.new_kv_cache(B, max_len, per_sequence=True)
    paged = m.new_kv_cache(B, max_len, page_size=P, n_pages=need)
    assert paged.paged and paged.n_pages == 6 and paged.nbytes < flat.nbytes

    calls = {"paged": 0, "appends": 0}
    real_decode, real_append = O.decode_attention, O.kv_append

    def decode(*a, **kw):
        calls["paged"] += kw.get("block_table") is not None
        return real_decode(*a, **kw)

    def append(*a, **kw):
        calls["appends"] += kw.get("block_table") is not None
        return real_append(*a, **kw)

    O.decode_attention, O.kv_append = decode, append
    try:
        a, b = (m(x, kv_cache=c, prompt_lens=LENS) for c in (flat, paged))
        assert paged.pos == LENS == flat.pos and paged.length.tolist() == LENS
        # only the prompts' pages are mapped: row 2's padding falls on an unmapped page
        assert paged.pages_in_use == sum((n + P - 1) // P for n in LENS) == 5
        for r, n in enumerate(LENS):
            assert torch.equal(a[r, :n], b[r, :n]), f"prefill row {r}"
        tok = torch.stack([a[r, n - 1] for r, n in enumerate(LENS)])[:, None].contiguous()
        for i in range(STEPS):
            a, b = (m(tok, kv_cache=c) for c in (flat, paged))
            assert torch.equal(a, b), f"step {i}"
            tok = a.contiguous()
    finally:
        O.decode_attention, O.kv_append = real_decode, real_append
    torch.cuda.synchronize()
    assert calls == {"paged": 2 * STEPS, "appends": 2}, calls      # every layer, the HIP path
    assert paged.pos == [n + STEPS for n in LENS] == paged.length.tolist()
    assert paged.pages_in_use == need == paged.peak_pages_in_use
    assert torch.isfinite(a.float()).all()
    # the caches agree at every real position, gathered through the table
    for layer in range(2):
        for mine, theirs in ((paged.k, flat.k), (paged.v, flat.v), (paged.k_scale, flat.k_scale),
                             (paged.v_scale, flat.v_scale)):
            if mine[layer] is None:
                continue
            u8 = (lambda t: t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t)
            pool, ref = u8(mine[layer]), u8(theirs[layer])
            for r, n in enumerate(paged.pos):
                for j in range((n + P - 1) // P):
                    end = min((j + 1) * P, n)
                    page = int(paged.table_host[r, j])
                    assert torch.equal(pool[page][:, :end - j * P], ref[r, :, j * P:end]), (r, j)


def test_run_tp_paged_record(tmp_path):
    """``--prompt-lens 17,64 --decode 8 --kv-page-size 16``: the table is fixed before the first
    forward, so the prefill and the decode step replay from HIP graphs; the default pool is
    exactly ceil(25 / 16) + ceil(72 / 16) = 7 pages, less than the contiguous 2 x 72 positions."""
    import yaml

    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "baseline_config.yaml")))
    cfg["model"].update(hidden_size=512, num_layers=2, num_heads=8, ffn_intermediate=2048,
                        init_std=0.02)
    cfg["input"].update(batch_size=2, sequence_length=64)
    cfg["execution"].update(warmup_iterations=1, benchmark_iterations=3)
    cfg["parallelism"]["world_size"] = 1
    cfg["experiment"]["output_dir"] = str(tmp_path)
    (tmp_path / "c.yaml").write_text(yaml.safe_dump(cfg))
    out = subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                          "--config", str(tmp_path / "c.yaml"), "--backend", "rccl", "--decode",
                          "8", "--attention", "flash", "--prompt-lens", "17,64",
                          "--kv-page-size", "16"],
                         capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "HIP graph replay off" not in out.stdout, out.stdout[-3000:]
    files = [f for f in os.listdir(tmp_path) if f.endswith(".json")]
    assert files == [f"rccl_{cfg['experiment']['name']}_decode8_ragged_paged16.json"], files
    d = json.load(open(tmp_path / files[0]))["decode"]
    assert d["timing_mode"] == "hip_graph_replay", d["hip_graph_note"]
    assert d["attention_path"] == "hip" and d["prompt_lengths"] == [17, 64]
    assert (d["kv_page_size"], d["kv_pool_pages"], d["kv_pages_peak"]) == (16, 7, 7)
    per_position = 2 * 2 * 8 * 64 * 2                  # layers, K + V, heads, head dim 64 bf16
    assert d["kv_cache_bytes_per_rank"] == 7 * 16 * per_position < 2 * 72 * per_position
    assert len(d["ms_per_token"]) == 3 and all(v > 0 for v in d["ms_per_token"])
