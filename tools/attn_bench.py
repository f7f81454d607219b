"""Device time of the causal attention forward / backward (ours vs torch SDPA vs the library
backward) at the GPT-2 shape and longer sequences, head dim 64 and 128.

``--prefill [--out FILE]``: the chunked-prefill kernel (``ops.prefill_attention``) instead: a block
of T queries over a cache that already holds ``prefix`` tokens, at the 7B head shape (H 32, D 128)
and GPT-2's (H 12, D 64), B 1 / 8, T 512 / 2048, prefix 0 / 2048 / 8192. Per row, in one process
and interleaved round by round: the kernel, torch SDPA under an explicit mask on the same cache, a
copy of the K / V bytes the kernel reads and, at prefix 0, ``attn_fwd`` on the same qkv (the same
FLOPs). One JSON line per row (default ``profiles/prefill_attention/attn_prefill.jsonl``).

``--prefill --fp8``: the FP8-cache form beside the bf16-cache kernel, and a copy of the bytes each
reads (bf16 rows; codes + scales), over T 128 / 512 / 2048 and prefix 0 / 2048 / 8192 / 16384 (a
short chunk over a long prefix is where the halved cache stream can show); no SDPA and no
``attn_fwd`` candidates (default ``profiles/prefill_attention/attn_prefill_fp8.jsonl``).

``--prefill --gqa``: the grouped-query kernel (``n_kv_head=``) at H_q 32, D 128, H_kv 8 / 4, T 8 /
128 / 512, prefix 0 / 2048 / 8192, B 1 / 8, beside the ungrouped kernel on the cache repeated to
32 heads and a copy of the grouped K + V bytes; median [min, max] over interleaved rounds (default
``profiles/prefill_gqa/attn_prefill_gqa.jsonl``).

``--prefill --gqa --split``: the same rows and candidates plus ``gqa_split``, the key-split form
(``key_split=``) at ``CHUNK_PREFILL_GQA`` with its workspace allocated outside the timed region
and ``len_bound`` = the live length; on the B 1 rows also at chunks 128 / 256 / 512 / 1024
(``gqa_split_<chunk>``) (default ``profiles/prefill_gqa_split/attn_prefill_gqa_split.jsonl``).

``--prefill --gqa --window W``: the sliding-window form (``window=W``): T 8 / 128 over a prefix of
8192 keys, ``gqa_window`` beside the unwindowed one-launch kernel (``gqa``), the key-split kernel
(``gqa_split``), ``expanded`` and ``kv_copy_window``, a copy of the ``W + T`` K + V rows the window
spans (default ``profiles/gqa_window/attn_prefill_gqa_window.jsonl``).

``--prefill --gqa --rope``: append + attend of 8 tokens over 8192 keys with ``rope=`` (``fused``)
beside the same calls without RoPE (``plain``) and beside ``qkv`` rotated in torch first
(``torch_rope``), one-launch and key-split (default
``profiles/gqa_rope/attn_prefill_gqa_rope.jsonl``)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llm_backend_benchmark_amd.ops import causal_attention  # noqa: E402
from distributed_llm_backend_benchmark_amd.ops.attention import (  # noqa: E402
    _torch_attention, attn_bwd, attn_bwd_library, attn_fwd)


def t_best(fn, iters=20, rounds=5):
    best = 1e9
    for _ in range(rounds):
        fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        best = min(best, s.elapsed_time(e) / iters * 1e-3)
    return best


def _fp8_cache(kc, vc, qkv, H, prefix, length):
    """The FP8 twin of a bf16 cache: the prefix rows re-appended quantised, T at a time (prefix
    is a multiple of T), then the chunk as ``kv_append`` stores it."""
    from distributed_llm_backend_benchmark_amd.ops import kv_append

    B, T = qkv.shape[:2]
    k8, v8 = (torch.zeros(c.shape, dtype=torch.float8_e4m3fn, device="cuda") for c in (kc, vc))
    ks, vs = (torch.ones(kc.shape[:3], device="cuda") for _ in "kv")
    buf = torch.zeros(B, T, 3, H, kc.shape[3], dtype=torch.bfloat16, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    for s in range(0, prefix, T):
        buf[:, :, 1] = kc[:, :, s:s + T].transpose(1, 2)
        buf[:, :, 2] = vc[:, :, s:s + T].transpose(1, 2)
        pos.fill_(s)
        kv_append(buf.view(B, T, -1), H, k8, v8, pos, k_scale=ks, v_scale=vs)
    kv_append(qkv, H, k8, v8, length, k_scale=ks, v_scale=vs)
    return k8, v8, ks, vs


def prefill_rows(out_path, fp8=False):
    import torch.nn.functional as F

    from distributed_llm_backend_benchmark_amd.ops import kv_append, prefill_attention
    from distributed_llm_backend_benchmark_amd.ops.attention import _views

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    with open(out_path, "w") as fh:
        for H, D in ((32, 128), (12, 64)):
            for B in (1, 8):
                for T in (128, 512, 2048) if fp8 else (512, 2048):
                    for prefix in (0, 2048, 8192, 16384) if fp8 else (0, 2048, 8192):
                        n = prefix + T
                        qkv = torch.randn(B, T, 3 * H * D, device="cuda", generator=gen).bfloat16()
                        kc = torch.randn(B, H, n, D, device="cuda", generator=gen).bfloat16()
                        vc = torch.randn(B, H, n, D, device="cuda", generator=gen).bfloat16()
                        length = torch.tensor([prefix], dtype=torch.int32, device="cuda")
                        kv_append(qkv, H, kc, vc, length)
                        mask = torch.ones(T, n, dtype=torch.bool, device="cuda").tril(prefix)
                        q = _views(qkv, H)[0]
                        fns = {"prefill": lambda: prefill_attention(qkv, H, kc, vc, length),
                               "sdpa_masked": lambda: F.scaled_dot_product_attention(
                                   q, kc, vc, attn_mask=mask),
                               "kv_copy": lambda: (kc.clone(), vc.clone())}
                        if prefix == 0:
                            fns["attn_fwd"] = lambda: attn_fwd(qkv, H)
                        if fp8:
                            k8, v8, ks, vs = _fp8_cache(kc, vc, qkv, H, prefix, length)
                            fns = {"prefill": fns["prefill"], "kv_copy": fns["kv_copy"],
                                   "prefill_fp8": lambda: prefill_attention(
                                       qkv, H, k8, v8, length, k_scale=ks, v_scale=vs),
                                   "kv_copy_fp8": lambda: (k8.view(torch.uint8).clone(),
                                                           v8.view(torch.uint8).clone(),
                                                           ks.clone(), vs.clone())}
                        other = (fns["prefill_fp8"]() if fp8 else fns["sdpa_masked"]()
                                 .transpose(1, 2).reshape(B, T, H * D))
                        err = float((fns["prefill"]().float() - other.float()).abs().max())
                        best = {k: 1e9 for k in fns}
                        for _ in range(5):                      # interleaved: one round of each
                            for k, fn in fns.items():
                                best[k] = min(best[k], t_best(fn, iters=10, rounds=1))
                        fl = 4.0 * B * H * D * (T * prefix + T * (T + 1) / 2)
                        nbytes = 2 * B * H * n * D * 2
                        rec = {"H": H, "D": D, "B": B, "T": T, "prefix": prefix,
                               "workgroups": -(-T // 128) * H * B,
                               "workgroups_per_cu": -(-T // 128) * H * B / 256,
                               "max_abs_diff_vs_fp8" if fp8 else "max_abs_diff_vs_sdpa": err,
                               "kv_bytes": nbytes,
                               "kv_copy_GBps": 2 * nbytes / best["kv_copy"] / 1e9,
                               "tflops_prefill": fl / best["prefill"] / 1e12}
                        if fp8:
                            rec["kv_bytes_fp8"] = 2 * B * H * n * (D + 4)
                            rec["tflops_prefill_fp8"] = fl / best["prefill_fp8"] / 1e12
                        else:
                            rec["tflops_sdpa_masked"] = fl / best["sdpa_masked"] / 1e12
                        rec.update({f"us_{k}": v * 1e6 for k, v in best.items()})
                        if "attn_fwd" in best:
                            rec["tflops_attn_fwd"] = fl / best["attn_fwd"] / 1e12
                        print(json.dumps(rec), flush=True)
                        fh.write(json.dumps(rec) + "\n")
                        fh.flush()


def prefill_gqa_rows(out_path, rounds=7, split=False, window=None):
    """Grouped-query chunked prefill at H_q 32, D 128: ``gqa`` (the grouped cache), ``expanded``
    (the ungrouped kernel on the cache repeated to 32 heads, built outside the timed region) and
    ``kv_copy`` (a device copy of the grouped K + V bytes read), one timed window of each per
    round, round by round; per candidate the median, min and max over the rounds. ``split``: also
    ``gqa_split`` (``key_split=CHUNK_PREFILL_GQA``, workspace allocated outside the timed region,
    ``len_bound`` the live length) and, at B 1, ``gqa_split_<chunk>`` over the chunk sweep.
    ``window``: the rows of a short block over a long prefix only, with ``gqa_split`` (no sweep),
    ``gqa_window`` (``window=``; checked against the torch form) and ``kv_copy_window``."""
    import statistics

    from distributed_llm_backend_benchmark_amd.ops import (CHUNK_PREFILL_GQA, kv_append,
                                                           prefill_attention,
                                                           prefill_workspace_numel)
    from distributed_llm_backend_benchmark_amd.ops.decode import torch_prefill_attention

    def split_fn(qkv, HKV, kc, vc, length, n, chunk):
        B, T = qkv.shape[:2]
        ws = torch.empty(prefill_workspace_numel(B, HQ, D, T, n, chunk), device="cuda")
        return lambda: prefill_attention(qkv, HQ, kc, vc, length, n_kv_head=HKV, key_split=chunk,
                                         len_bound=n, workspace=ws)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    HQ, D = 32, 128
    with open(out_path, "w") as fh:
        for HKV in (8, 4):
            G = HQ // HKV
            for B in (1, 8):
                for T in (8, 128) if window else (8, 128, 512):
                    for prefix in (8192,) if window else (0, 2048, 8192):
                        n = prefix + T
                        qkv = torch.randn(B, T, (HQ + 2 * HKV) * D, device="cuda",
                                          generator=gen).bfloat16()
                        kc = torch.randn(B, HKV, n, D, device="cuda", generator=gen).bfloat16()
                        vc = torch.randn(B, HKV, n, D, device="cuda", generator=gen).bfloat16()
                        length = torch.tensor([prefix], dtype=torch.int32, device="cuda")
                        kv_append(qkv, HQ, kc, vc, length, n_kv_head=HKV)
                        x = qkv.view(B, T, HQ + 2 * HKV, D)
                        mha = torch.stack(
                            [x[:, :, :HQ], x[:, :, HQ:HQ + HKV].repeat_interleave(G, 2),
                             x[:, :, HQ + HKV:].repeat_interleave(G, 2)], 2).reshape(B, T, -1)
                        ke, ve = kc.repeat_interleave(G, 1), vc.repeat_interleave(G, 1)
                        fns = {"gqa": lambda: prefill_attention(qkv, HQ, kc, vc, length,
                                                                n_kv_head=HKV),
                               "expanded": lambda: prefill_attention(mha, HQ, ke, ve, length),
                               "kv_copy": lambda: (kc.clone(), vc.clone())}
                        err = float((fns["gqa"]().float() - fns["expanded"]().float())
                                    .abs().max())
                        if window:
                            lo = max(0, prefix - window + 1)
                            fns["gqa_window"] = lambda: prefill_attention(
                                qkv, HQ, kc, vc, length, n_kv_head=HKV, window=window)
                            fns["kv_copy_window"] = lambda: (kc[:, :, lo:].clone(),
                                                             vc[:, :, lo:].clone())
                            want = torch_prefill_attention(qkv, HQ, kc, vc, prefix, n_kv_head=HKV,
                                                           window=window)
                            err_window = float((fns["gqa_window"]().float() - want.float())
                                               .abs().max())
                        if split or window:
                            fns["gqa_split"] = split_fn(qkv, HKV, kc, vc, length, n,
                                                        CHUNK_PREFILL_GQA)
                            for ck in (128, 256, 512, 1024) if B == 1 and not window else ():
                                if ck != CHUNK_PREFILL_GQA:
                                    fns[f"gqa_split_{ck}"] = split_fn(qkv, HKV, kc, vc, length,
                                                                      n, ck)
                            err_split = float((fns["gqa_split"]().float() - fns["gqa"]().float())
                                              .abs().max())
                        # a timed window of >= 20 ms per candidate and round
                        iters = {k: max(10, min(2000, int(0.02 / t_best(fn, iters=5, rounds=1))))
                                 for k, fn in fns.items()}
                        times = {k: [] for k in fns}
                        for _ in range(rounds):                 # interleaved: one round of each
                            for k, fn in fns.items():
                                times[k].append(t_best(fn, iters=iters[k], rounds=1) * 1e6)
                        med = {k: statistics.median(v) for k, v in times.items()}
                        rec = {"H_q": HQ, "H_kv": HKV, "D": D, "B": B, "T": T, "prefix": prefix,
                               "workgroups_gqa": -(-T * G // 128) * HKV * B,
                               "workgroups_expanded": -(-T // 128) * HQ * B,
                               "max_abs_diff_gqa_vs_expanded": err,
                               "kv_bytes_gqa": 2 * B * HKV * n * D * 2,
                               "kv_bytes_expanded": 2 * B * HQ * n * D * 2,
                               "gqa_over_expanded": med["gqa"] / med["expanded"]}
                        if window:
                            KB = 8192 // (2 * D)                # keys per tile of the kernel
                            rec.update({"window": window,
                                        "tiles_gqa": -(-n // KB), "tiles_gqa_window":
                                            -(-n // KB) - lo // KB,
                                        "kv_bytes_window": 2 * B * HKV * (n - lo) * D * 2,
                                        "max_abs_diff_gqa_window_vs_torch": err_window,
                                        "gqa_window_over_gqa": med["gqa_window"] / med["gqa"],
                                        "gqa_window_over_gqa_split":
                                            med["gqa_window"] / med["gqa_split"]})
                        if split or window:
                            nck = -(-n // CHUNK_PREFILL_GQA)
                            rec.update({"chunk": CHUNK_PREFILL_GQA,
                                        "workgroups_gqa_split": rec["workgroups_gqa"] * nck,
                                        "ws_bytes_gqa_split": 4 * prefill_workspace_numel(
                                            B, HQ, D, T, n, CHUNK_PREFILL_GQA),
                                        "max_abs_diff_gqa_split_vs_gqa": err_split,
                                        "gqa_split_over_gqa": med["gqa_split"] / med["gqa"],
                                        "gqa_split_over_expanded":
                                            med["gqa_split"] / med["expanded"]})
                        for k, v in times.items():
                            rec.update({f"us_{k}": med[k], f"us_{k}_min": min(v),
                                        f"us_{k}_max": max(v)})
                        print(json.dumps(rec), flush=True)
                        fh.write(json.dumps(rec) + "\n")
                        fh.flush()


def prefill_gqa_rope_rows(out_path, rounds=7):
    """``--prefill --gqa --rope``: append + attend of a block of 8 tokens over 8192 keys at H_q 32,
    D 128, through the one-launch kernel and through ``key_split=CHUNK_PREFILL_GQA``: ``fused``
    (``rope=`` on both calls), ``plain`` (today's calls, no RoPE) and ``torch_rope`` (``qkv``
    rotated in torch, then ``plain``), one timed window of each per round, round by round."""
    import statistics

    from decode_bench import rope_qkv_torch, rope_table
    from distributed_llm_backend_benchmark_amd.ops import (CHUNK_PREFILL_GQA, kv_append,
                                                           prefill_attention,
                                                           prefill_workspace_numel)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    HQ, D, T, prefix = 32, 128, 8, 8192
    n = prefix + T
    rope = rope_table(n, D, "cuda")
    with open(out_path, "w") as fh:
        for HKV in (8, 4):
            for B in (1, 8):
                for split in (False, True):
                    qkv = torch.randn(B, T, (HQ + 2 * HKV) * D, device="cuda",
                                      generator=gen).bfloat16()
                    kc = torch.randn(B, HKV, n, D, device="cuda", generator=gen).bfloat16()
                    vc = torch.randn(B, HKV, n, D, device="cuda", generator=gen).bfloat16()
                    length = torch.tensor([prefix], dtype=torch.int32, device="cuda")
                    kw = {"n_kv_head": HKV}
                    if split:
                        ws = torch.empty(prefill_workspace_numel(B, HQ, D, T, n,
                                                                 CHUNK_PREFILL_GQA), device="cuda")
                        kw.update(key_split=CHUNK_PREFILL_GQA, len_bound=n, workspace=ws)

                    def block(x, **r):
                        kv_append(x, HQ, kc, vc, length, n_kv_head=HKV, **r)
                        return prefill_attention(x, HQ, kc, vc, length, **kw, **r)

                    fns = {"plain": lambda: block(qkv), "fused": lambda: block(qkv, rope=rope),
                           "torch_rope": lambda: block(rope_qkv_torch(qkv, HQ + HKV, D,
                                                                      rope[prefix:n]))}
                    err = float((fns["fused"]().float() - fns["torch_rope"]().float())
                                .abs().max())
                    iters = {k: max(10, min(2000, int(0.02 / t_best(fn, iters=5, rounds=1))))
                             for k, fn in fns.items()}
                    times = {k: [] for k in fns}
                    for _ in range(rounds):                     # interleaved: one round of each
                        for k, fn in fns.items():
                            times[k].append(t_best(fn, iters=iters[k], rounds=1) * 1e6)
                    med = {k: statistics.median(v) for k, v in times.items()}
                    rec = {"H_q": HQ, "H_kv": HKV, "D": D, "B": B, "T": T, "prefix": prefix,
                           "key_split": CHUNK_PREFILL_GQA if split else None,
                           "max_abs_diff_fused_vs_torch_rope": err,
                           "fused_over_plain": med["fused"] / med["plain"],
                           "plain_spread": [min(times["plain"]) / med["plain"],
                                            max(times["plain"]) / med["plain"]],
                           "fused_over_torch_rope": med["fused"] / med["torch_rope"]}
                    for k, v in times.items():
                        rec.update({f"us_{k}": med[k], f"us_{k}_min": min(v),
                                    f"us_{k}_max": max(v)})
                    print(json.dumps(rec), flush=True)
                    fh.write(json.dumps(rec) + "\n")
                    fh.flush()


_ap = argparse.ArgumentParser()
_ap.add_argument("--prefill", action="store_true")
_ap.add_argument("--fp8", action="store_true", help="with --prefill: the FP8-cache rows")
_ap.add_argument("--gqa", action="store_true",
                 help="with --prefill: the grouped-query kernel beside the expanded cache")
_ap.add_argument("--split", action="store_true",
                 help="with --prefill --gqa: the key-split form and its chunk sweep as well")
_ap.add_argument("--window", type=int, default=None,
                 help="with --prefill --gqa: the sliding-window form over a prefix of 8192 keys")
_ap.add_argument("--rope", action="store_true",
                 help="with --prefill --gqa: rope= beside no RoPE and beside a torch rotation")
_ap.add_argument("--out", default=None)
_args = _ap.parse_args()
if _args.prefill and _args.gqa and _args.rope:
    prefill_gqa_rope_rows(_args.out or os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gqa_rope",
        "attn_prefill_gqa_rope.jsonl"))
    sys.exit(0)
if _args.prefill and _args.gqa:
    _name = "prefill_gqa_split" if _args.split else "prefill_gqa"
    _dir = "gqa_window" if _args.window else _name
    prefill_gqa_rows(_args.out or os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", _dir,
        f"attn_{'prefill_gqa_window' if _args.window else _name}.jsonl"), split=_args.split,
        window=_args.window)
    sys.exit(0)
if _args.prefill:
    prefill_rows(_args.out or os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
        "prefill_attention", "attn_prefill_fp8.jsonl" if _args.fp8 else "attn_prefill.jsonl"),
        _args.fp8)
    sys.exit(0)

for B, T, H, D in ((16, 1024, 12, 64), (8, 2048, 12, 64), (4, 4096, 16, 64),
                   (16, 1024, 6, 128), (4, 4096, 8, 128)):
    qkv = torch.randn(B, T, 3 * H * D, device="cuda").to(torch.bfloat16)
    fl = 4.0 * B * H * T * T * D / 2          # causal
    t_ours = t_best(lambda: attn_fwd(qkv, H))
    t_torch = t_best(lambda: _torch_attention(qkv, H))
    x = qkv.clone().requires_grad_(True)
    go = torch.randn(B, T, H * D, device="cuda").to(torch.bfloat16)
    t_fb_ours = t_best(lambda: causal_attention(x, H).backward(go), iters=5, rounds=3)
    t_fb_torch = t_best(lambda: _torch_attention(x, H).backward(go), iters=5, rounds=3)
    o, lse = attn_fwd(qkv, H)
    rec = {"B": B, "T": T, "H": H, "D": D, "fwd_us_ours": t_ours * 1e6,
           "fwd_us_torch": t_torch * 1e6, "fwd_tflops_ours": fl / t_ours / 1e12,
           "fwd_tflops_torch": fl / t_torch / 1e12,
           "fwd_bwd_us_ours": t_fb_ours * 1e6, "fwd_bwd_us_torch": t_fb_torch * 1e6}
    t_lib = t_best(lambda: attn_bwd_library(qkv, o, lse, go, H), iters=10, rounds=3)
    rec["bwd_us_library"] = t_lib * 1e6
    t_bwd = t_best(lambda: attn_bwd(qkv, o, lse, go, H), iters=10, rounds=3)
    rec.update(bwd_us_ours=t_bwd * 1e6, bwd_tflops_ours=2.5 * fl / t_bwd / 1e12)
    print(json.dumps(rec), flush=True)
