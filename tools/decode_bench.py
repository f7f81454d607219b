#!/usr/bin/env python
"""Decode attention A/B: our split + combine kernels against torch SDPA on the same cache slice
and against a plain device copy of the same K / V bytes (the bandwidth yardstick).

For every (B, H, D, L) row all candidates are timed interleaved in ONE process: each is warmed,
captured in a HIP graph of ``--inner`` back-to-back calls (so host launch cost is out of the
number, as in ``run_tp``'s replayed decode step), and the graphs are replayed in alternation for
``--rounds`` rounds; the median round is reported. Calls rotate over enough distinct caches
that the working set exceeds the 256 MiB last-level cache (``--rotate-mb``), so small shapes are
timed from HBM as a long-running decode would see them.

Printed per candidate: microseconds per call and K / V bytes / time. The copy moves the K / V
bytes twice (read + write), so its rate is given over 2x the bytes; ``share_of_copy`` is our
read rate over that. ``--chunks`` adds our kernel at other split sizes, ``two_launch`` is the
kv_append + attention form of the same step. Rows go to ``profiles/decode/attn_decode.jsonl``.

``--fp8`` adds the FP8 (e4m3) KV cache beside it, same protocol and same process: ``ours_fp8`` is
the decode step over caches holding the same K / V as e4m3 codes + one fp32 scale per row
(``D + 4`` bytes per row; rotated over as many caches as the bf16 form), ``copy_fp8`` a device copy
of exactly those code + scale bytes, ``ours_fp8_chunk<N>`` the kernel at the other ``--fp8-chunks``.
``GBps`` of these candidates is over the bytes they actually read (``kv_bytes_fp8``);
``fp8_over_bf16`` is ``us[ours_fp8] / us[ours]``, ``fp8_vs_bf16_max_rel_diff`` the output distance
of the two cache types on the row's inputs.

``--ragged`` times the per-sequence kernels instead (same protocol, same process; rows go to
``profiles/ragged_decode/attn_decode_ragged.jsonl``). For every shape: ``ragged`` is one decode
step over a batch whose rows attend ``L (b + 1) / B`` keys, b = 0 .. B - 1 (spread evenly over
``(0, L]``), through ``length = int32[B]``; ``uniform`` the shared-length step of all rows at
``L`` (the ``ours`` of the default mode); ``uniform_seq`` the per-sequence kernel with every row at
``L``, which isolates what ``length[b]`` costs; ``copy_live`` a device copy of exactly the ragged
batch's live K / V bytes and ``copy`` of all of them. With ``--fp8`` the same five over the FP8
cache (``*_fp8``). ``ragged_over_uniform`` is the time ratio, ``live_share`` the byte ratio it
would equal if time followed the live bytes alone.

``--paged`` times the paged kernels on the same ragged batches (same protocol, same process; rows
go to ``profiles/paged_decode/attn_decode_paged.jsonl``). For every shape and each page size ``P``
in ``--page-sizes`` (default 16, 64, 256): ``paged<P>`` is the decode step over a page pool holding
exactly the live pages, the block table in a seeded shuffled physical order; ``paged_identity<P>``
the same pool with every row's pages in logical order; beside them ``ragged`` (the contiguous
per-sequence kernel at the same lengths) and ``copy_live``. With ``--fp8`` the same over the FP8
cache (``*_fp8``). ``paged_over_ragged`` is the ratio of the medians per ``P``, ``ragged_spread``
the min and max round of ``ragged`` over its median, and ``within_ragged_spread`` whether the
ratio lies inside it; ``paged_bits_equal_ragged`` checks the outputs' bytes.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# 7B per-rank shapes (32 heads / P for P = 1, 4, 8; head dim 128) and the GPT-2 shape
DEFAULT_ROWS = [(8, h, 128, L) for h in (32, 8, 4) for L in (512, 2048, 8192)] + [(8, 12, 64, 1024)]


def bench_row(B, H, D, L, args):
    import torch
    import torch.nn.functional as F

    from distributed_llm_backend_benchmark_amd.ops import decode as dec

    dev = torch.device("cuda", 0)
    kv_bytes = 2 * B * H * L * D * 2
    nbuf = max(1, min(16, -(-args.rotate_mb * (1 << 20) // kv_bytes)))
    g = torch.Generator(device=dev).manual_seed(L + H)
    caches = [torch.randn(2, B, H, L, D, generator=g, device=dev).to(torch.bfloat16)
              for _ in range(nbuf)]
    sink = torch.empty_like(caches[0])
    qkv = torch.randn(B, 1, 3 * H * D, generator=g, device=dev).to(torch.bfloat16)
    q = qkv[:, 0, :H * D].reshape(B, H, 1, D)
    length = torch.tensor([L - 1], dtype=torch.int32, device=dev)
    chunks = sorted(set(args.chunks))
    ws = torch.empty(dec.workspace_numel(B, H, D, L, min(chunks + [dec.CHUNK])),
                     dtype=torch.float32, device=dev)

    def ours(i, **kw):
        kc, vc = caches[i % nbuf]
        return dec.decode_attention(qkv, H, kc, vc, length, workspace=ws, **kw)

    def sdpa(i):
        kc, vc = caches[i % nbuf]
        return F.scaled_dot_product_attention(q, kc, vc)

    def copy(i):
        sink.copy_(caches[i % nbuf])

    cands = {"ours": ours, "two_launch": lambda i: ours(i, fused=False), "sdpa": sdpa,
             "copy": copy}
    for c in chunks:
        if c != dec.CHUNK:
            cands[f"ours_chunk{c}"] = lambda i, c=c: ours(i, chunk=c)

    kv_bytes_fp8 = 2 * B * H * L * (D + 4)
    if args.fp8:
        from distributed_llm_backend_benchmark_amd.ops import fp8

        # the same K / V, quantised per row: codes [2, B, H, L, D] and scales [2, B, H, L]
        caches8 = []
        for kv in caches:
            q8, s8 = fp8.quantize_rows(kv.reshape(-1, D))
            caches8.append((q8.view(2, B, H, L, D), s8.view(2, B, H, L)))
        sink8 = (torch.empty_like(caches8[0][0]), torch.empty_like(caches8[0][1]))
        chunks8 = sorted(set(args.fp8_chunks))
        ws8 = torch.empty(dec.workspace_numel(B, H, D, L, min(chunks8 + [dec.CHUNK_FP8])),
                          dtype=torch.float32, device=dev)

        def ours_fp8(i, **kw):
            (kc, vc), (ks, vs) = caches8[i % nbuf]
            return dec.decode_attention(qkv, H, kc, vc, length, workspace=ws8, k_scale=ks,
                                        v_scale=vs, **kw)

        def copy_fp8(i):
            sink8[0].copy_(caches8[i % nbuf][0])
            sink8[1].copy_(caches8[i % nbuf][1])

        cands["ours_fp8"] = ours_fp8
        cands["copy_fp8"] = copy_fp8
        for c in chunks8:
            if c != dec.CHUNK_FP8:
                cands[f"ours_fp8_chunk{c}"] = lambda i, c=c: ours_fp8(i, chunk=c)

    graphs = {}
    for name, fn in cands.items():                       # warm every candidate, then capture
        for i in range(nbuf + 1):
            fn(i)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for i in range(args.inner):
                fn(i)
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    times = {n: [] for n in graphs}
    for _ in range(args.rounds):                         # alternate the candidates
        for name, gr in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            gr.replay()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.inner)
    # same result from every form (the fused / two-launch / chunk variants differ by fp32
    # reassociation only)
    ref = sdpa(0).transpose(1, 2).reshape(B, 1, H * D).float()
    err = float((ours(0).float() - ref).abs().max() / ref.abs().max())
    us = {n: statistics.median(v) for n, v in times.items()}
    row = {"B": B, "H": H, "D": D, "L": L, "kv_bytes": kv_bytes, "rotated_caches": nbuf,
           "chunk": dec.CHUNK, "fused_append": dec.FUSED_APPEND, "inner": args.inner,
           "rounds": args.rounds, "us": us,
           "us_min": {n: min(v) for n, v in times.items()},
           "GBps": {n: (2 if n.startswith("copy") else 1)
                    * (kv_bytes_fp8 if "fp8" in n else kv_bytes) / (t * 1e-6) / 1e9
                    for n, t in us.items()},
           "max_rel_diff_vs_sdpa": err}
    row["share_of_copy"] = row["GBps"]["ours"] / row["GBps"]["copy"]
    row["ours_over_sdpa"] = us["ours"] / us["sdpa"]
    if args.fp8:
        row["kv_bytes_fp8"] = kv_bytes_fp8
        row["chunk_fp8"] = dec.CHUNK_FP8
        row["share_of_copy_fp8"] = row["GBps"]["ours_fp8"] / row["GBps"]["copy_fp8"]
        row["fp8_over_bf16"] = us["ours_fp8"] / us["ours"]
        row["fp8_vs_bf16_max_rel_diff"] = float((ours_fp8(0).float() - ours(0).float()).abs().max()
                                                / ref.abs().max())
    return row


def bench_ragged_row(B, H, D, L, args):
    import torch

    from distributed_llm_backend_benchmark_amd.ops import decode as dec

    dev = torch.device("cuda", 0)
    keys = [max(1, L * (b + 1) // B) for b in range(B)]          # keys row b attends, <= L
    live_keys = sum(keys)
    kv_bytes = 2 * B * H * L * D * 2
    nbuf = max(1, min(16, -(-args.rotate_mb * (1 << 20) // kv_bytes)))
    g = torch.Generator(device=dev).manual_seed(L + H)
    caches = [torch.randn(2, B, H, L, D, generator=g, device=dev).to(torch.bfloat16)
              for _ in range(nbuf)]
    qkv = torch.randn(B, 1, 3 * H * D, generator=g, device=dev).to(torch.bfloat16)
    shared = torch.tensor([L - 1], dtype=torch.int32, device=dev)
    full = torch.full((B,), L - 1, dtype=torch.int32, device=dev)
    ragged = torch.tensor([k - 1 for k in keys], dtype=torch.int32, device=dev)
    ws = torch.empty(dec.workspace_numel(B, H, D, L, dec.CHUNK), dtype=torch.float32, device=dev)
    # the live bytes as one flat run of a cache (K and V rows of H heads over sum(keys) positions)
    live = 2 * H * live_keys * D
    sink = torch.empty_like(caches[0])

    def step(length):
        def fn(i):
            kc, vc = caches[i % nbuf]
            return dec.decode_attention(qkv, H, kc, vc, length, workspace=ws)
        return fn

    def copy(n):
        def fn(i):
            sink.view(-1)[:n].copy_(caches[i % nbuf].view(-1)[:n])
        return fn

    cands = {"ragged": step(ragged), "uniform": step(shared), "uniform_seq": step(full),
             "copy_live": copy(live), "copy": copy(sink.numel())}
    nbytes = {"ragged": live * 2, "uniform": kv_bytes, "uniform_seq": kv_bytes,
              "copy_live": live * 2, "copy": kv_bytes}
    if args.fp8:
        from distributed_llm_backend_benchmark_amd.ops import fp8

        caches8 = []
        for kv in caches:
            q8, s8 = fp8.quantize_rows(kv.reshape(-1, D))
            caches8.append((q8.view(2, B, H, L, D), s8.view(2, B, H, L)))
        sink8 = (torch.empty_like(caches8[0][0]), torch.empty_like(caches8[0][1]))
        ws8 = torch.empty(dec.workspace_numel(B, H, D, L, dec.CHUNK_FP8), dtype=torch.float32,
                          device=dev)
        rows_live = 2 * H * live_keys

        def step8(length):
            def fn(i):
                (kc, vc), (ks, vs) = caches8[i % nbuf]
                return dec.decode_attention(qkv, H, kc, vc, length, workspace=ws8, k_scale=ks,
                                            v_scale=vs)
            return fn

        def copy8(rows):
            def fn(i):
                sink8[0].view(-1)[:rows * D].copy_(caches8[i % nbuf][0].view(-1)[:rows * D])
                sink8[1].view(-1)[:rows].copy_(caches8[i % nbuf][1].view(-1)[:rows])
            return fn

        all_rows = 2 * B * H * L
        cands.update({"ragged_fp8": step8(ragged), "uniform_fp8": step8(shared),
                      "uniform_seq_fp8": step8(full), "copy_live_fp8": copy8(rows_live),
                      "copy_fp8": copy8(all_rows)})
        nbytes.update({"ragged_fp8": rows_live * (D + 4), "uniform_fp8": all_rows * (D + 4),
                       "uniform_seq_fp8": all_rows * (D + 4),
                       "copy_live_fp8": rows_live * (D + 4), "copy_fp8": all_rows * (D + 4)})

    graphs = {}
    for name, fn in cands.items():                       # warm every candidate, then capture
        for i in range(nbuf + 1):
            fn(i)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for i in range(args.inner):
                fn(i)
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    times = {n: [] for n in graphs}
    for _ in range(args.rounds):                         # alternate the candidates
        for name, gr in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            gr.replay()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.inner)
    # the per-sequence kernel at uniform lengths gives the shared-length kernel's bits
    same = bool(torch.equal(step(full)(0).view(torch.int16), step(shared)(0).view(torch.int16)))
    us = {n: statistics.median(v) for n, v in times.items()}
    row = {"B": B, "H": H, "D": D, "L": L, "keys_per_row": keys, "kv_bytes": kv_bytes,
           "live_kv_bytes": live * 2, "live_share": live_keys / (B * L), "rotated_caches": nbuf,
           "chunk": dec.CHUNK, "inner": args.inner, "rounds": args.rounds, "us": us,
           "us_min": {n: min(v) for n, v in times.items()},
           "us_max": {n: max(v) for n, v in times.items()},
           # bytes each candidate reads (a copy also writes them: its rate is over 2x)
           "GBps": {n: (2 if n.startswith("copy") else 1) * nbytes[n] / (t * 1e-6) / 1e9
                    for n, t in us.items()},
           "uniform_seq_bits_equal_uniform": same,
           "ragged_over_uniform": us["ragged"] / us["uniform"],
           "uniform_seq_over_uniform": us["uniform_seq"] / us["uniform"],
           "copy_live_over_copy": us["copy_live"] / us["copy"]}
    if args.fp8:
        row["live_kv_bytes_fp8"] = nbytes["ragged_fp8"]
        row["chunk_fp8"] = dec.CHUNK_FP8
        row["ragged_over_uniform_fp8"] = us["ragged_fp8"] / us["uniform_fp8"]
        row["uniform_seq_over_uniform_fp8"] = us["uniform_seq_fp8"] / us["uniform_fp8"]
    return row


def bench_paged_row(B, H, D, L, args):
    import torch

    from distributed_llm_backend_benchmark_amd.ops import decode as dec

    dev = torch.device("cuda", 0)
    keys = [max(1, L * (b + 1) // B) for b in range(B)]          # keys row b attends, <= L
    live_keys = sum(keys)
    kv_bytes = 2 * B * H * L * D * 2
    nbuf = max(1, min(16, -(-args.rotate_mb * (1 << 20) // kv_bytes)))
    g = torch.Generator(device=dev).manual_seed(L + H)
    caches = [torch.randn(2, B, H, L, D, generator=g, device=dev).to(torch.bfloat16)
              for _ in range(nbuf)]
    qkv = torch.randn(B, 1, 3 * H * D, generator=g, device=dev).to(torch.bfloat16)
    ragged = torch.tensor([k - 1 for k in keys], dtype=torch.int32, device=dev)
    ws = torch.empty(dec.workspace_numel(B, H, D, L, dec.CHUNK), dtype=torch.float32, device=dev)
    live = 2 * H * live_keys * D
    sink = torch.empty_like(caches[0])
    caches8 = []
    if args.fp8:
        from distributed_llm_backend_benchmark_amd.ops import fp8

        for kv in caches:
            q8, s8 = fp8.quantize_rows(kv.reshape(-1, D))
            caches8.append((q8.view(2, B, H, L, D), s8.view(2, B, H, L)))
        sink8 = (torch.empty_like(caches8[0][0]), torch.empty_like(caches8[0][1]))
        ws8 = torch.empty(dec.workspace_numel(B, H, D, L, dec.CHUNK_FP8), dtype=torch.float32,
                          device=dev)

    def tables(P, shuffled):
        """The block table of the batch (exactly the live pages) and the pool size."""
        need = [-(-k // P) for k in keys]
        n_pages = sum(need)
        order = (torch.randperm(n_pages, generator=torch.Generator().manual_seed(P + L)).tolist()
                 if shuffled else list(range(n_pages)))
        table = torch.full((B, -(-L // P)), -1, dtype=torch.int32)
        for b in range(B):
            for j in range(need[b]):
                table[b, j] = order.pop(0)
        return table, n_pages

    def pooled(x, table, n_pages, P):
        """``x [2, B, H, L, ...]`` -> the pool ``[2, n_pages, H, P, ...]`` through ``table``."""
        pool = torch.zeros(2, n_pages, H, P, *x.shape[4:], dtype=x.dtype, device=dev)
        raw, src = (t.view(torch.uint8) if t.dtype == dec.E4M3 else t for t in (pool, x))
        for b in range(B):
            idx = table[b][table[b] >= 0].to(dev).long()
            n = idx.numel()
            rows = src[:, b, :, :n * P].reshape(2, H, n, P, *x.shape[4:])
            raw[:, idx] = rows.transpose(1, 2)
        return pool

    def step(length, bufs, wsp, **kw):
        def fn(i):
            (kc, vc), sc = bufs[i % nbuf]
            return dec.decode_attention(qkv, H, kc, vc, length, workspace=wsp,
                                        **({} if sc is None
                                           else dict(k_scale=sc[0], v_scale=sc[1])), **kw)
        return fn

    def copy(n):
        def fn(i):
            sink.view(-1)[:n].copy_(caches[i % nbuf].view(-1)[:n])
        return fn

    cands = {"ragged": step(ragged, [(c, None) for c in caches], ws), "copy_live": copy(live)}
    if args.fp8:
        rows_live = 2 * H * live_keys

        def copy8(i):
            sink8[0].view(-1)[:rows_live * D].copy_(caches8[i % nbuf][0].view(-1)[:rows_live * D])
            sink8[1].view(-1)[:rows_live].copy_(caches8[i % nbuf][1].view(-1)[:rows_live])

        cands["ragged_fp8"] = step(ragged, caches8, ws8)
        cands["copy_live_fp8"] = copy8
    pool_pages = {}
    for P in args.page_sizes:
        if L % P or dec.CHUNK % P:
            raise SystemExit(f"--paged needs page sizes dividing L = {L} and the chunk")
        for name, shuffled in ((f"paged{P}", True), (f"paged_identity{P}", False)):
            table, n_pages = tables(P, shuffled)
            pool_pages[P] = n_pages
            kw = dict(block_table=table.to(dev), max_len=L)
            cands[name] = step(ragged, [(pooled(c, table, n_pages, P), None) for c in caches],
                               ws, **kw)
            if args.fp8:
                cands[name + "_fp8"] = step(
                    ragged, [(pooled(c8, table, n_pages, P), pooled(s8, table, n_pages, P))
                             for c8, s8 in caches8], ws8, **kw)

    graphs = {}
    for name, fn in cands.items():                       # warm every candidate, then capture
        for i in range(nbuf + 1):
            fn(i)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for i in range(args.inner):
                fn(i)
        gr.replay()
        graphs[name] = gr
    torch.cuda.synchronize()
    times = {n: [] for n in graphs}
    for _ in range(args.rounds):                         # alternate the candidates
        for name, gr in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            gr.replay()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.inner)
    us = {n: statistics.median(v) for n, v in times.items()}
    ref = cands["ragged"](0).view(torch.int16)
    same = {n: bool(torch.equal(fn(0).view(torch.int16), ref)) for n, fn in cands.items()
            if n.startswith("paged") and not n.endswith("_fp8")}
    row = {"B": B, "H": H, "D": D, "L": L, "keys_per_row": keys, "kv_bytes": kv_bytes,
           "live_kv_bytes": live * 2, "live_share": live_keys / (B * L), "rotated_caches": nbuf,
           "chunk": dec.CHUNK, "inner": args.inner, "rounds": args.rounds,
           "page_sizes": list(args.page_sizes), "pool_pages": pool_pages, "us": us,
           "us_min": {n: min(v) for n, v in times.items()},
           "us_max": {n: max(v) for n, v in times.items()},
           "paged_bits_equal_ragged": same}
    for sfx in ("", "_fp8") if args.fp8 else ("",):
        lo, hi = (min(times["ragged" + sfx]) / us["ragged" + sfx],
                  max(times["ragged" + sfx]) / us["ragged" + sfx])
        row["ragged_spread" + sfx] = [lo, hi]
        row["paged_over_ragged" + sfx] = {P: us[f"paged{P}{sfx}"] / us["ragged" + sfx]
                                          for P in args.page_sizes}
        row["paged_identity_over_ragged" + sfx] = {
            P: us[f"paged_identity{P}{sfx}"] / us["ragged" + sfx] for P in args.page_sizes}
        row["within_ragged_spread" + sfx] = {P: bool(r <= hi) for P, r in
                                             row["paged_over_ragged" + sfx].items()}
    if args.fp8:
        ref8 = cands["ragged_fp8"](0).view(torch.int16)
        row["paged_bits_equal_ragged_fp8"] = {
            n: bool(torch.equal(fn(0).view(torch.int16), ref8)) for n, fn in cands.items()
            if n.startswith("paged") and n.endswith("_fp8")}
    return row


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", nargs="*", default=None, metavar="B,H,D,L")
    ap.add_argument("--chunks", type=int, nargs="*", default=[128, 256, 512])
    ap.add_argument("--fp8", action="store_true",
                    help="also time the FP8 (e4m3) KV cache: ours_fp8, copy_fp8, --fp8-chunks")
    ap.add_argument("--fp8-chunks", type=int, nargs="*", default=[256, 512, 1024])
    ap.add_argument("--ragged", action="store_true",
                    help="time the per-sequence kernels on a batch of spread lengths instead: "
                         "ragged, uniform, uniform_seq, copy_live, copy (with --fp8 also *_fp8)")
    ap.add_argument("--paged", action="store_true",
                    help="time the paged kernels on the ragged batches instead: paged<P>, "
                         "paged_identity<P>, ragged, copy_live (with --fp8 also *_fp8)")
    ap.add_argument("--page-sizes", type=int, nargs="*", default=[16, 64, 256])
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--rotate-mb", type=int, default=512)
    ap.add_argument("--out", default=None,
                    help="default profiles/decode/attn_decode.jsonl (--ragged: "
                         "profiles/ragged_decode/attn_decode_ragged.jsonl)")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", *(("paged_decode", "attn_decode_paged.jsonl")
                                                    if args.paged else
                                                    ("ragged_decode", "attn_decode_ragged.jsonl")
                                                    if args.ragged
                                                    else ("decode", "attn_decode.jsonl")))
    rows = ([tuple(int(v) for v in r.split(",")) for r in args.rows] if args.rows
            else DEFAULT_ROWS)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for B, H, D, L in rows:
            if args.paged:
                row = bench_paged_row(B, H, D, L, args)
                f.write(json.dumps(row) + "\n")
                f.flush()
                print(f"B={B} H={H} D={D} L={L} (live share {row['live_share']:.3f}): " +
                      "  ".join(f"{n} {t:.1f} us" for n, t in row["us"].items()) +
                      f"  paged/ragged {row['paged_over_ragged']}  ragged spread "
                      f"{row['ragged_spread']}" +
                      (f"  fp8 {row['paged_over_ragged_fp8']}" if args.fp8 else ""), flush=True)
                continue
            if args.ragged:
                row = bench_ragged_row(B, H, D, L, args)
                f.write(json.dumps(row) + "\n")
                f.flush()
                print(f"B={B} H={H} D={D} L={L} (live share {row['live_share']:.3f}): " +
                      "  ".join(f"{n} {t:.1f} us ({row['GBps'][n]:.0f} GB/s)"
                                for n, t in row["us"].items()) +
                      f"  ragged/uniform {row['ragged_over_uniform']:.3f}" +
                      (f"  fp8 {row['ragged_over_uniform_fp8']:.3f}" if args.fp8 else ""),
                      flush=True)
                continue
            row = bench_row(B, H, D, L, args)
            f.write(json.dumps(row) + "\n")
            f.flush()
            us = row["us"]
            print(f"B={B} H={H} D={D} L={L} ({row['kv_bytes'] / 2**20:.0f} MiB K+V, "
                  f"{row['rotated_caches']} caches): " +
                  "  ".join(f"{n} {t:.1f} us ({row['GBps'][n]:.0f} GB/s)" for n, t in us.items())
                  + f"  share_of_copy {row['share_of_copy']:.2f}  ours/sdpa "
                  f"{row['ours_over_sdpa']:.2f}" +
                  (f"  fp8/bf16 {row['fp8_over_bf16']:.2f}  share_of_copy_fp8 "
                   f"{row['share_of_copy_fp8']:.2f}" if args.fp8 else ""), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
