"""Global gradient-norm clipping on the GPU: the sum-of-squares and coefficient kernels
(csrc/grad_clip.hip), the AdamW forms that read the coefficient on the device, and the DDP /
ZeRO-2 trainers with ``clip_grad_norm`` (eager and as a captured HIP graph)."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24          # fp32 unit roundoff
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from distributed_llm_backend_benchmark_amd.ops import _lib

    _lib.lib()  # must load: no silent fallback on a GPU box
    yield


def _plan(n):
    from distributed_llm_backend_benchmark_amd.ops import sumsq_plan

    return sumsq_plan(n)


def _sumsq_depth(n):
    """Longest chain of fp32 additions a term of the kernel's sum passes through, from the launch
    geometry: a lane owns 8 accumulators (one per element position of its 16-byte vectors) and
    adds ``unroll`` squares (one fma each, the square itself is not rounded) into each per grid
    sweep, over ceil(vectors / (grid * block * unroll)) sweeps; + 1 for the n % 8 tail element
    added to accumulator 0 of workgroup 0; + 3 for the 8 -> 1 tree of the accumulators; + 6 for
    the 64-lane butterfly; + (waves - 1) for the waves' sums added in order."""
    p = _plan(n)
    sweeps = -(-(n // 8) // (p["grid"] * p["block"] * p["unroll"]))
    return sweeps * p["unroll"] + 1 + 3 + 6 + (p["block"] // 64 - 1)


def _coef_depth(count, block=256):
    """clip_coef: thread t adds partials t, t + 256, ... in order (ceil(count / 256) additions,
    the first onto 0), then the same workgroup tree (6 + 3)."""
    return -(-count // block) + 6 + (block // 64 - 1)


def _guarded(n, guard=64):
    buf = torch.full((n + 2 * guard,), NAN, device=DEV)
    return buf, buf[guard:guard + n]


def _guards_intact(buf, n, guard=64):
    return bool(torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all())


@pytest.fixture(scope="module")
def exact_case():
    """Integer data in {-2..2} (both dtypes hold it exactly) and the int64 prefix sums of its
    squares, made once: every (offset, size) reference below is one subtraction."""
    p = _plan(1 << 40)                     # a size at which the grid is at its cap
    wg = p["block"] * p["unroll"] * 8      # elements one workgroup reads per sweep
    sweep = p["grid"] * wg                 # elements the whole grid reads per sweep
    assert p["grid"] == p["slots"]
    sizes = [0, 1, 7, 8, 9, wg - 1, wg, wg + 1, sweep - 1, sweep, sweep + 1, 3 * sweep + 5,
             1 << 22]
    total = max(sizes) + 72
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randint(-2, 3, (total,), device=DEV, generator=g, dtype=torch.int8)
    prefix = torch.zeros(total + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(x.to(torch.int64) ** 2, 0, out=prefix[1:])
    return {"x": x, "prefix": prefix.cpu(), "sizes": sizes, "plan": p}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grad_sumsq_exact(exact_case, dtype):
    """Every partial stays below 2^24 (a workgroup reads at most 4 sweeps of block * unroll * 8
    <= 2^15 elements, each square <= 4; 2^22 elements sum to at most 2^24 in all — asserted per
    case), so fp32 addition is exact and the partials must sum
    to the int64 reference exactly — at every size where the kernel takes another path, at
    range starts 0 / 8 / 64 / 72 elements into the buffer, with the slots past the grid zeroed,
    nothing written outside the slots, and the same bits from a second run."""
    from distributed_llm_backend_benchmark_amd.ops import grad_sumsq

    x = exact_case["x"].to(dtype)
    prefix, slots = exact_case["prefix"], exact_case["plan"]["slots"]
    for n in exact_case["sizes"]:
        grid = _plan(n)["grid"]
        for off in (0, 8, 64, 72):
            buf, row = _guarded(slots)
            buf2, row2 = _guarded(slots)
            grad_sumsq(x[off:off + n], row)
            grad_sumsq(x[off:off + n], row2)
            want = int(prefix[off + n] - prefix[off])
            got = row.cpu()
            assert float(got.max()) < 2 ** 24
            assert int(got.double().sum()) == want, (n, off, int(got.double().sum()), want)
            assert not got[grid:].any(), (n, off)              # slots with no work hold 0
            assert torch.equal(row, row2), (n, off)
            assert _guards_intact(buf, slots) and _guards_intact(buf2, slots), (n, off)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grad_sumsq_rejects_bad_arguments(dtype):
    from distributed_llm_backend_benchmark_amd.ops import KernelError, grad_sumsq, sumsq_plan

    slots = sumsq_plan(0)["slots"]
    x = torch.ones(4096, device=DEV, dtype=dtype)
    row = torch.zeros(slots, device=DEV)
    for off in (1, 2, 3):                                      # 2..12 bytes past 16-byte alignment
        with pytest.raises(KernelError, match="grad_sumsq"):
            grad_sumsq(x[off:off + 1024], row)
    big = 8 * 256 * sumsq_plan(0)["unroll"] * 2                # needs 2 workgroups
    with pytest.raises(KernelError, match="grad_sumsq"):
        grad_sumsq(torch.ones(big, device=DEV, dtype=dtype), row[:1])
    with pytest.raises(ValueError):
        grad_sumsq(x.to(torch.float16), row)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grad_sumsq_randn_against_fp64(dtype):
    """Non-negative terms: a sum through chains of at most d fp32 additions is within d u of the
    exact sum to first order; (d + 1) u is the bound. The partials are added in fp64 here, so d
    is the kernel's own depth."""
    from distributed_llm_backend_benchmark_amd.ops import grad_sumsq

    p = _plan(1 << 40)
    sweep = p["grid"] * p["block"] * p["unroll"] * 8
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(3 * sweep + 5, device=DEV, generator=g).to(dtype)
    row = torch.empty(p["slots"], device=DEV)
    for n in (1000003, sweep + 1, 3 * sweep + 5):
        grad_sumsq(x[:n], row)
        got = float(row.double().sum())
        want = float(x[:n].double().square().sum())
        d = _sumsq_depth(n)
        print(f"{dtype} n={n} depth {d} rel err {abs(got - want) / want:.3e} "
              f"bound {(d + 1) * U:.3e}")
        assert abs(got - want) <= (d + 1) * U * want, (n, got, want)


def _ulps(got, want64):
    want = np.float32(want64)
    return abs(float(np.float32(got)) - want64) / float(np.spacing(want))


def test_clip_coef():
    from distributed_llm_backend_benchmark_amd.ops import clip_coef

    g = torch.Generator(device=DEV).manual_seed(7)
    eps = float(np.float32(1e-6))
    for count in (1, 255, 257, 5 * 1024):
        parts = torch.rand(count, device=DEV, generator=g) * 3 + 2      # norm >= 1.41 * scale
        for pre_scale, max_norm in ((1.0, 1.0), (0.125, 0.03), (1.0 / 3.0, 0.4)):
            buf, out = _guarded(3, guard=4)
            clip_coef(parts, pre_scale, max_norm, out)
            norm, coef, total = (float(v) for v in out.cpu())
            assert _guards_intact(buf, 3, guard=4)
            # out[2]: the fixed fp32 tree over non-negative partials against their fp64 sum
            want_sum = float(parts.double().sum())
            assert abs(total - want_sum) <= (_coef_depth(count) + 1) * U * want_sum
            # norm and coef from the kernel's OWN sum: sqrt, multiply | add, divide, each
            # correctly rounded, so a few ulps of the fp64 formula
            ps, mn = float(np.float32(pre_scale)), float(np.float32(max_norm))
            norm64 = math.sqrt(total) * ps
            assert norm64 > mn                                 # the clipping branch
            assert _ulps(norm, norm64) <= 4, (count, norm, norm64)
            assert _ulps(coef, mn / (norm64 + eps)) <= 4, (count, coef)
            assert coef < 1.0
    # below max_norm: exactly 1
    out = torch.empty(3, device=DEV)
    clip_coef(torch.full((300,), 1e-4, device=DEV), 1.0, 1.0, out)
    assert float(out[1]) == 1.0 and 0 < float(out[0]) < 1.0
    # pre_scale acts on the norm before the coefficient is formed: sum 16 -> 4 | 0.5
    sixteen = torch.full((16,), 1.0, device=DEV)
    clip_coef(sixteen, 1.0, 1.0, out)
    assert float(out[0]) == 4.0 and float(out[1]) == pytest.approx(0.25, rel=1e-6)
    clip_coef(sixteen, 0.125, 1.0, out)
    assert float(out[0]) == 0.5 and float(out[1]) == 1.0 and float(out[2]) == 16.0
    # a non-finite partial: NaN norm and NaN coefficient (never 1 or 0)
    for bad in (float("inf"), NAN):
        parts = torch.ones(700, device=DEV)
        parts[333] = bad
        clip_coef(parts, 1.0, 1.0, out)
        assert math.isnan(float(out[0])) and math.isnan(float(out[1])), (bad, out)
    # an already reduced sum in place (count 1 from out[2], the sharded form)
    out.copy_(torch.tensor([NAN, NAN, 9.0]))
    clip_coef(out[2:3], 0.5, 1.0, out)
    assert [float(v) for v in out] == [1.5, pytest.approx(1 / 1.500001, rel=1e-6), 9.0]


@pytest.mark.parametrize("devstep", [False, True])
@pytest.mark.parametrize("gdt", [torch.bfloat16, torch.float32])
def test_adamw_clip(gdt, devstep):
    from distributed_llm_backend_benchmark_amd.ops import FlatAdamW

    n = 100003
    gen = torch.Generator(device=DEV).manual_seed(28)
    p0 = torch.randn(n, device=DEV, generator=gen)
    grads = [torch.randn(n, device=DEV, generator=gen).to(gdt) for _ in range(3)]
    kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)

    def run(scale, coef):
        p = p0.clone()
        opt = FlatAdamW(p, **kw)
        if devstep:
            opt.enable_device_step()
        shadow = torch.empty(n, dtype=torch.bfloat16, device=DEV)
        c = None if coef is None else torch.tensor([coef], device=DEV)
        for g in grads:
            opt.step(g, working_bf16=shadow, grad_scale=scale, coef_dev=c)
        assert opt.t == 3 and (not devstep or int(opt.t_dev.item()) == 3)
        return p, opt.m, opt.v, shadow

    base = run(0.5, None)
    for a, b in zip(base, run(0.5, 1.0)):                     # g * 1.0 is g
        assert torch.equal(a, b)
    for a, b in zip(run(0.25, None), run(0.5, 0.5)):          # scaling by 2^-1 is exact
        assert torch.equal(a, b)
    p, _, _, shadow = run(0.5, 0.3)
    pref = p0.clone().requires_grad_(True)
    ref = torch.optim.AdamW([pref], **kw)
    for g in grads:
        pref.grad = g.float() * 0.5 * 0.3
        ref.step()
    torch.testing.assert_close(p, pref.detach(), rtol=1e-5, atol=1e-6)   # test_adamw's
    torch.testing.assert_close(shadow, p.to(torch.bfloat16), rtol=0, atol=0)
    assert not torch.equal(p, base[0])


# ------------------------------------------------------------------------------ trainers
def _gpt2(seed, **kw):
    from distributed_llm_backend_benchmark_amd.models.gpt2 import GPT2, GPT2Config

    cfg = GPT2Config(**{**dict(vocab_size=512, block_size=64, n_layer=3, n_head=4, n_embd=256),
                        **kw})
    return GPT2(cfg, device=torch.device(DEV, 0), seed=seed)


def _tokens(steps, seq=64, vocab=512, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, vocab, (steps, 4, seq + 1), device=DEV, generator=g)


def _norm_tolerance(tr, ranges):
    """Relative bound on the reported norm against the fp64 norm of the same buffer: the sum of
    squares passes through the deepest range's chain, then clip_coef's tree over every slot;
    sqrt halves the sum's relative error and adds a rounding, the scale adds one."""
    d = max(_sumsq_depth(n) for n in ranges) + _coef_depth(tr._clipper.partials.numel()) + 2
    return (d + 1) * U


def _check_one_clipped_step(tr, grad, ranges, x, y):
    """One step of a clipping trainer whose optimizer state is fresh: the reported norm against
    the fp64 norm of the reduced gradient buffer read after the step, and the masters against
    ONE torch-path FlatAdamW step fed that buffer and the device coefficient."""
    from distributed_llm_backend_benchmark_amd.ops import FlatAdamW

    assert tr.opt.t == 0
    ref_master = tr.master.detach().cpu().clone()      # updated in place by the reference
    tr.step(x, y)
    got = tr.last_grad_norm()
    want = float(grad.double().square().sum().sqrt())
    tol = _norm_tolerance(tr, ranges)
    print(f"norm {got!r} fp64 {want!r} rel {abs(got - want) / want:.3e} bound {tol:.3e}")
    assert got > tr.clip_grad_norm                             # the clip bites
    assert abs(got - want) <= tol * want, (got, want)
    coef = tr._clipper.coef.cpu()
    assert float(coef) == pytest.approx(tr.clip_grad_norm / (got + 1e-6), rel=1e-5)
    ref = FlatAdamW(ref_master, lr=tr.opt.lr, betas=tr.opt.betas, eps=tr.opt.eps,
                    weight_decay=tr.opt.wd)
    ref.step(grad.cpu(), grad_scale=1.0, coef_dev=coef)
    torch.testing.assert_close(tr.master.cpu(), ref_master, rtol=1e-5, atol=1e-6)  # test_adamw's
    return got


@pytest.mark.parametrize("ov", [0, 2])
def test_ddp_clip_world1(ov):
    """Config of test_ddp_overlapped_optimizer_is_bit_exact. A clip that never bites (1e30) is
    bit-identical to clipping off — 3 eager steps, a captured step and 2 replays, the step count
    advancing once per step; a clip at half the first norm reports the right norm, updates as
    the torch formula, and its graph replay equals its eager steps bit for bit."""
    from distributed_llm_backend_benchmark_amd.parallel.ddp import FlatParamTrainer

    data = _tokens(6)

    def trainer(clip):
        tr = FlatParamTrainer(_gpt2(6), None, lr=1e-3, bucket_mb=0.3, clip_grad_norm=clip)
        tr.opt_overlap = ov
        assert len(tr.buckets) > 2 and tr._split_optimizer_ok()
        return tr

    def run(tr, graph):
        losses, norms = [], []
        for s in range(3):
            losses.append(tr.step(data[s, :, :-1], data[s, :, 1:]))
            norms.append(tr.last_grad_norm() if tr.grad_norm is not None else None)
        if tr._clipper is not None and ov:
            assert tr._opt_issued == len(tr.buckets) - 1 and tr._opt_stream is not None
        if graph:
            replay = tr.capture_step(data[3, :, :-1], data[3, :, 1:])
            for s in (4, 5):
                losses.append(float(replay(data[s, :, :-1], data[s, :, 1:]).item()))
                norms.append(tr.last_grad_norm() if tr.grad_norm is not None else None)
            torch.cuda.synchronize()
            assert int(tr.opt.t_dev.item()) == 6
        else:
            # capture_step moves the step count to device memory, where the kernel forms the
            # bias corrections itself (device powf): the eager side takes the same form from
            # the same step on, so both sides run the same kernels on the same inputs
            tr.opt.enable_device_step()
            for s in (3, 4, 5):
                loss = tr.step(data[s, :, :-1], data[s, :, 1:])
                if s > 3:
                    losses.append(loss)
                    norms.append(tr.last_grad_norm() if tr.grad_norm is not None else None)
        torch.cuda.synchronize()
        assert tr.opt.t == 6 and tr.step_count == 6
        out = (losses, norms, tr.master.clone())
        tr.close()
        return out

    off = run(trainer(None), graph=True)
    big = run(trainer(1e30), graph=True)
    assert off[0] == big[0]
    assert torch.equal(off[2], big[2])
    norm1 = big[1][0]
    assert norm1 > 0 and all(n > 0 for n in big[1])

    tr = trainer(0.5 * norm1)
    nb = [b.end - b.start for b in tr.buckets]
    got = _check_one_clipped_step(tr, tr.flat_grad, nb, data[0, :, :-1], data[0, :, 1:])
    assert got == norm1                                        # same first step, same bits
    tr.close()

    eager = run(trainer(0.5 * norm1), graph=False)
    graphed = run(trainer(0.5 * norm1), graph=True)
    assert eager[0] == graphed[0] and eager[1] == graphed[1]
    assert torch.equal(eager[2], graphed[2])
    assert not torch.equal(eager[2], off[2])


def test_ddp_clip_flatten_fp32_buckets():
    """mode="flatten" with fp32 buckets (one range over flat_grad, fp32 sum-of-squares and AdamW
    kernels): one clipped step against the torch reference."""
    from distributed_llm_backend_benchmark_amd.parallel.ddp import FlatParamTrainer

    data = _tokens(1)
    x, y = data[0, :, :-1], data[0, :, 1:]
    probe = FlatParamTrainer(_gpt2(6), None, lr=1e-3, bucket_mb=0.3, mode="flatten",
                             grad_dtype=torch.float32, clip_grad_norm=1e30)
    probe.step(x, y)
    norm1 = probe.last_grad_norm()
    probe.close()
    tr = FlatParamTrainer(_gpt2(6), None, lr=1e-3, bucket_mb=0.3, mode="flatten",
                          grad_dtype=torch.float32, clip_grad_norm=0.5 * norm1)
    assert tr._clipper.partials.shape[0] == 1 and tr.flat_grad.dtype == torch.float32
    _check_one_clipped_step(tr, tr.flat_grad, [tr.numel], x, y)
    tr.close()


def test_zero2_clip_world1_rccl(tmp_path):
    """ZeRO-2 on RCCL (world 1, as test_zero2_and_checkpoint_world1_gpu): its clipped norm is
    DDP's up to the summation order (one range over the shard against one per bucket), the
    one-float all-reduce form of the norm gives the bits of the local form at world 1, and a
    checkpoint resumes bit-exactly with clipping on."""
    import torch.distributed as dist

    from distributed_llm_backend_benchmark_amd.ops import GradClipper
    from distributed_llm_backend_benchmark_amd.parallel.comm import init_distributed
    from distributed_llm_backend_benchmark_amd.parallel.ddp import FlatParamTrainer
    from distributed_llm_backend_benchmark_amd.parallel.zero import ShardedTrainer

    comm = init_distributed("rccl")
    try:
        kw = dict(vocab_size=1024, block_size=128, n_layer=2, n_head=4, n_embd=256)
        data = _tokens(6, seq=128, vocab=1024, seed=0)
        clip = 0.5                                             # below every norm seen here
        ddp = FlatParamTrainer(_gpt2(2, **kw), comm, lr=1e-3, bucket_mb=1, clip_grad_norm=clip)
        zero = ShardedTrainer(_gpt2(2, **kw), comm, lr=1e-3, bucket_mb=1, clip_grad_norm=clip)
        assert len(ddp.buckets) > 1 and zero._clipper.partials.shape[0] == 1
        tol = (_norm_tolerance(ddp, [b.end - b.start for b in ddp.buckets])
               + _norm_tolerance(zero, [zero.shard_numel]))
        for s in range(3):
            ld = ddp.step(data[s, :, :-1], data[s, :, 1:])
            lz = zero.step(data[s, :, :-1], data[s, :, 1:])
            nd, nz = ddp.last_grad_norm(), zero.last_grad_norm()
            print(f"step {s} norm ddp {nd!r} zero {nz!r} rel {abs(nd - nz) / nd:.3e} "
                  f"bound {tol:.3e}")
            assert abs(ld - lz) < 2e-2, (s, ld, lz)
            assert nd > clip and nz > clip
            if s == 0:          # identical weights: the same gradient values on both sides
                assert abs(nd - nz) <= tol * nd, (nd, nz)
        # the sharded form of finish() on HIP kernels: sum, all-reduce of one float, count-1 coef
        g = zero.grad_shard
        local, shard = GradClipper(1, clip, g.device), GradClipper(1, clip, g.device)
        local.accumulate(0, g)
        shard.accumulate(0, g)
        local.finish(0.5)
        shard.finish(0.5, group=dist.group.WORLD)
        assert torch.equal(local.out, shard.out) and float(local.norm) > 0
        # checkpoint / resume with clipping on
        zero.save_checkpoint(str(tmp_path / "ck"))
        cont = [(zero.step(data[s, :, :-1], data[s, :, 1:]), zero.last_grad_norm())
                for s in range(3, 6)]
        res = ShardedTrainer(_gpt2(99, **kw), comm, lr=1e-3, bucket_mb=1, clip_grad_norm=clip)
        res.load_checkpoint(str(tmp_path / "ck"))
        again = [(res.step(data[s, :, :-1], data[s, :, 1:]), res.last_grad_norm())
                 for s in range(3, 6)]
        assert cont == again, (cont, again)
        assert torch.equal(zero.master, res.master)
    finally:
        comm.destroy()
