"""Training health on the GPU: the segmented per-tensor statistics kernels (md_tensor_stats_partial / _finish) against float64
torch, the device-side non-finite step guard (md_step_guard, md_adamw_step[_ranges]_guarded) against the unguarded pass, and both
under the Trainer: one rank without an exchange, the two exchange modes on a one-rank process group, and the promise that the
switches left off change nothing.

Tolerance of every sum of squares: 2e-5 relative.  One thread chains at most 256 fp32 terms (65536-element items, 256 threads x 8
elements per iteration), the wave / workgroup / item / tensor trees above it are about 20 levels: 276 * 2^-24 = 1.65e-5 worst case.
max |x| and the non-finite count are exact."""
import ctypes
import math
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5
NUMELS = [16, 1, 77, 65536, 3 * 65536 + 40, 1152 * 4608]      # the synthetic layout of the issue (5.57 M elements with padding)
SCALES = [1e-3, 1e3, 1e-2, 1.0, 1e2, 1e-1]                    # per-tensor scale of the N(0, 1) values


def _layout(numels, align=64):
    offs, total = [], 0
    for n in numels:
        offs.append(total)
        total += (n + align - 1) // align * align
    return offs, total


def _fill(offs, numels, total, dtype, seed, scales=SCALES):
    """Values N(0, 1) * scale inside the tensors, NaN in every padding element: only masking keeps the padding out."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.full((total,), float("nan"), device=DEV, dtype=torch.float32)
    for o, n, sc in zip(offs, numels, scales):
        buf[o:o + n] = torch.randn(n, device=DEV, generator=g) * sc
    return buf.to(dtype)


def _reference(buf, offs, numels):
    """float64 torch on the stored values: (sumsq, absmax, nonfinite) per tensor over the FINITE elements."""
    out = []
    for o, n in zip(offs, numels):
        x = buf[o:o + n].double()
        fin = torch.isfinite(x)
        xf = x[fin]
        out.append((float((xf * xf).sum()), float(xf.abs().max()) if xf.numel() else 0.0, int((~fin).sum())))
    return out


def _run(offs, numels, sources):
    from micro_diffusion_amd.trainer import _StatsPlan
    out_f, out_i = _StatsPlan(offs, numels, sources, torch.device(DEV)).run()
    torch.cuda.synchronize()
    return out_f.clone(), out_i.clone()


def _check(out_f, out_i, ref, what=""):
    for t, (ss, mx, nf) in enumerate(ref):
        got_ss, got_mx, got_nf = float(out_f[0, t]), float(out_f[1, t]), int(out_i[t])
        print(f"{what} tensor {t}: sumsq {got_ss:.9g} vs {ss:.9g} rel {abs(got_ss - ss) / max(ss, 1e-300):.3g}  absmax {got_mx:.9g}  nonfinite {got_nf}")
        assert got_nf == nf, (t, got_nf, nf)
        assert got_mx == mx, (t, got_mx, mx)
        assert abs(got_ss - ss) <= TOL * ss, (t, got_ss, ss)


def _inject(buf, offs):
    """+Inf at the first element of the 65536-element tensor, NaN at the last element of the 77-element tensor (inside the masked
    tail vector), -Inf in the middle of the 81-item tensor."""
    buf[offs[3]] = float("inf")
    buf[offs[2] + 76] = float("nan")
    buf[offs[5] + NUMELS[5] // 2 + 3] = float("-inf")
    return buf


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_tensor_stats_against_torch(hip, dtype):
    offs, total = _layout(NUMELS)
    buf = _fill(offs, NUMELS, total, dtype, 5)
    a = _run(offs, NUMELS, [(buf, [(0, total, 0)])])
    b = _run(offs, NUMELS, [(buf, [(0, total, 0)])])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "two calls on the same data must be bit-identical"
    ref = _reference(buf, offs, NUMELS)
    assert all(r[2] == 0 for r in ref)
    _check(a[0], a[1], ref, str(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_tensor_stats_count_and_exclude_non_finite_elements(hip, dtype):
    offs, total = _layout(NUMELS)
    buf = _inject(_fill(offs, NUMELS, total, dtype, 6), offs)
    out_f, out_i = _run(offs, NUMELS, [(buf, [(0, total, 0)])])
    assert out_i.tolist() == [0, 0, 1, 1, 0, 1]
    _check(out_f, out_i, _reference(buf, offs, NUMELS), str(dtype))


def test_tensor_stats_bad_arguments(hip):
    L, st = hip.lib(), hip.stream_ptr()
    x = torch.zeros(64, device=DEV)
    it = torch.zeros(2, dtype=torch.int64, device=DEV)
    o = torch.zeros(8, device=DEV)
    oi = torch.zeros(8, device=DEV, dtype=torch.int32)
    ok = (x.data_ptr(), 0, it.data_ptr(), 1, o.data_ptr(), o.data_ptr(), oi.data_ptr(), st)
    for i, bad in [(0, None), (2, None), (4, None), (5, None), (6, None), (3, 0), (0, x.data_ptr() + 4)]:
        args = list(ok)
        args[i] = bad
        assert L.md_tensor_stats_partial(*args) == -1, (i, bad)
    okf = (o.data_ptr(), o.data_ptr(), oi.data_ptr(), oi.data_ptr(), 1, o.data_ptr(), o.data_ptr(), oi.data_ptr(), st)
    for i, bad in [(0, None), (1, None), (2, None), (3, None), (5, None), (6, None), (7, None), (4, 0)]:
        args = list(okf)
        args[i] = bad
        assert L.md_tensor_stats_finish(*args) == -1, (i, bad)
    assert L.md_step_guard(None, oi.data_ptr(), st) == -1 and L.md_step_guard(o.data_ptr(), None, st) == -1


def test_tensor_stats_of_four_simulated_ranks_combine_to_the_whole(hip):
    """The sharded exchange at world 4 on one GPU: every rank's items on a packed copy of its chunks plus the small-region items,
    the four tables combined as the Trainer combines them (trainer.combine_rank_tables) -- against the whole-buffer pass."""
    from micro_diffusion_amd.trainer import combine_rank_tables, shard_plan
    world = 4
    # matrix-shaped tensors first, in two buckets on 1024-element boundaries; the three short tensors form the small region
    numels = [NUMELS[3], NUMELS[4], NUMELS[5], NUMELS[0], NUMELS[1], NUMELS[2]]
    scales = [SCALES[3], SCALES[4], SCALES[5], SCALES[0], SCALES[1], SCALES[2]]
    up = lambda v, a: (v + a - 1) // a * a
    offs = [0, up(numels[0], 64)]
    b1 = up(offs[1] + up(numels[1], 64), 1024)
    offs.append(b1)
    b2 = up(b1 + up(numels[2], 64), 1024)
    offs += [b2, b2 + 64, b2 + 128]
    total = up(b2 + 128 + up(numels[5], 64), 1024)
    buf = _fill(offs, numels, total, torch.bfloat16, 7, scales)
    buf[offs[0]] = float("inf")
    buf[offs[5] + 76] = float("nan")
    buf[offs[2] + numels[2] // 2 + 3] = float("-inf")
    whole_f, whole_i = _run(offs, numels, [(buf, [(0, total, 0)])])
    assert whole_i.tolist() == [1, 0, 1, 0, 0, 1]
    plan, small, own = shard_plan([("a", 0, b1), ("b", b1, b2), ("small", b2, total)], world)
    table = torch.zeros(world, 3, len(numels), device=DEV)
    for r in range(world):
        packed = torch.cat([buf[lo + r * chunk: lo + (r + 1) * chunk] for _, lo, hi, chunk, _ in plan])
        assert packed.numel() == own
        present = [(lo + r * chunk, chunk, olo) for _, lo, hi, chunk, olo in plan]
        f, i = _run(offs, numels, [(packed, present), (buf, [(small[0], small[1] - small[0], small[0])])])
        table[r, :2], table[r, 2] = f, i.float()
    comb = combine_rank_tables(table, torch.tensor([o >= small[0] for o in offs], device=DEV))
    assert torch.equal(comb[1], whole_f[1]), "max |x| of the combined ranks must equal the whole-buffer pass exactly"
    assert torch.equal(comb[2].to(torch.int32), whole_i)
    for t in range(len(numels)):
        a, b = float(comb[0, t]), float(whole_f[0, t])
        print(f"tensor {t}: combined {a:.9g} whole {b:.9g} rel {abs(a - b) / b:.3g}")
        assert abs(a - b) <= TOL * b, (t, a, b)
    _check(comb[:2], comb[2].to(torch.int32), _reference(buf, offs, numels), "combined")


def test_step_guard_flag_and_counter(hip):
    L, st = hip.lib(), hip.stream_ptr()
    state = torch.zeros(4, device=DEV, dtype=torch.int32)
    seen = []
    for v in (3.5, float("inf"), float("nan")):
        ss = torch.full((1,), v, device=DEV)
        hip.check(L.md_step_guard(ss.data_ptr(), state.data_ptr(), st), "md_step_guard")
        seen.append(state.tolist())
    assert seen == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0]], seen


def _adamw_case(hip, n, gbf16, ema_mode, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda: torch.randn(n, device=DEV, generator=g)
    st0 = {"p": rn(), "m": rn() * 0.1, "v": torch.rand(n, device=DEV, generator=g) * 0.01, "g": rn(), "ema": rn() * 0.5}
    gb = rn().to(torch.bfloat16) if gbf16 else None
    src = gb.float() if gbf16 else st0["g"]
    ss = torch.full((1,), float((src.double() ** 2).sum()), device=DEV)

    def run(call):
        t = {k: v.clone() for k, v in st0.items()}
        t["s"] = torch.zeros(n, device=DEV, dtype=torch.bfloat16)
        a = hip.AdamWArgs(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["s"].data_ptr(), ss.data_ptr(),
                          gb.data_ptr() if gbf16 else None, t["ema"].data_ptr() if ema_mode else None, n, 1e-3, 0.9, 0.999, 1e-8, 0.1,
                          1 - 0.9 ** 3, 1 - 0.999 ** 3, 0.25, 0.125, 0.99, 1, ema_mode)
        hip.check(call(ctypes.byref(a)), "adamw")
        torch.cuda.synchronize()
        return t
    return st0, run


@pytest.mark.parametrize("ema_mode", [0, 1, 2])
@pytest.mark.parametrize("gbf16", [False, True], ids=["g_fp32", "g_bf16"])
def test_adamw_step_guarded(hip, gbf16, ema_mode):
    L, st = hip.lib(), hip.stream_ptr()
    n = 3 * 1024 + 4
    st0, run = _adamw_case(hip, n, gbf16, ema_mode, 40 + ema_mode)
    go, stop = torch.tensor([1, 0, 0, 0], device=DEV, dtype=torch.int32), torch.zeros(4, device=DEV, dtype=torch.int32)
    base = run(lambda a: L.md_adamw_step(a, st))
    assert not torch.equal(base["p"], st0["p"])
    for name, guard in (("flag 1", go.data_ptr()), ("null guard", None)):
        got = run(lambda a: L.md_adamw_step_guarded(a, guard, st))
        for k in ("p", "m", "v", "s", "ema", "g"):
            assert torch.equal(got[k], base[k]), (name, k)
    got = run(lambda a: L.md_adamw_step_guarded(a, stop.data_ptr(), st))
    for k in ("p", "m", "v"):
        assert torch.equal(got[k], st0[k]), k
    assert float(got["g"].abs().max()) == 0.0
    assert torch.equal(got["s"], st0["p"].to(torch.bfloat16))
    assert torch.equal(got["ema"], st0["p"] if ema_mode == 1 else st0["ema"])


@pytest.mark.parametrize("ema_mode", [0, 1, 2])
def test_adamw_step_ranges_guarded(hip, ema_mode):
    """The range table of tests/test_kernels_gpu.py::test_adamw_step_ranges (packed bf16 gradient and bf16 weight output)."""
    L, st = hip.lib(), hip.stream_ptr()
    n = 64 * 700
    ranges = [(64 * 3, 64 * 10), (64 * 40, 64 * 100), (64 * 300, 64 * 7), (64 * 600, 64 * 100)]
    packed = sum(c for _, c in ranges)
    g = torch.Generator(device=DEV).manual_seed(50 + ema_mode)
    p0, m0 = torch.randn(n, device=DEV, generator=g), torch.randn(n, device=DEV, generator=g) * 0.1
    v0, e0 = torch.rand(n, device=DEV, generator=g) * 0.01, torch.randn(n, device=DEV, generator=g) * 0.5
    gpk = torch.randn(packed, device=DEV, generator=g).to(torch.bfloat16)
    ss = torch.full((1,), float((gpk.double() ** 2).sum()), device=DEV)
    off = (ctypes.c_int64 * len(ranges))(*[o for o, _ in ranges])
    cnt = (ctypes.c_int64 * len(ranges))(*[c for _, c in ranges])
    touched = torch.zeros(n, dtype=torch.bool, device=DEV)
    for o, c in ranges:
        touched[o:o + c] = True

    def run(call):
        t = {"p": p0.clone(), "m": m0.clone(), "v": v0.clone(), "ema": e0.clone(), "g": torch.zeros(n, device=DEV),
             "s": torch.zeros(packed, device=DEV, dtype=torch.bfloat16)}
        a = hip.AdamWArgs(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["s"].data_ptr(), ss.data_ptr(),
                          gpk.data_ptr(), t["ema"].data_ptr() if ema_mode else None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1 - 0.9 ** 3,
                          1 - 0.999 ** 3, 0.25, 0.125, 0.99, 0, ema_mode)
        hip.check(call(ctypes.byref(a)), "adamw ranges")
        torch.cuda.synchronize()
        return t
    go, stop = torch.tensor([1, 0, 0, 0], device=DEV, dtype=torch.int32), torch.zeros(4, device=DEV, dtype=torch.int32)
    base = run(lambda a: L.md_adamw_step_ranges(a, off, cnt, len(ranges), st))
    assert not torch.equal(base["p"][touched], p0[touched]) and torch.equal(base["p"][~touched], p0[~touched])
    for name, guard in (("flag 1", go.data_ptr()), ("null guard", None)):
        got = run(lambda a: L.md_adamw_step_ranges_guarded(a, off, cnt, len(ranges), guard, st))
        for k in ("p", "m", "v", "s", "ema"):
            assert torch.equal(got[k], base[k]), (name, k)
    got = run(lambda a: L.md_adamw_step_ranges_guarded(a, off, cnt, len(ranges), stop.data_ptr(), st))
    assert torch.equal(got["p"], p0) and torch.equal(got["m"], m0) and torch.equal(got["v"], v0)
    assert torch.equal(got["s"], torch.cat([p0[o:o + c] for o, c in ranges]).to(torch.bfloat16))
    want_ema = e0.clone()
    if ema_mode == 1:
        want_ema[touched] = p0[touched]
    assert torch.equal(got["ema"], want_ema)


# ---------------------------------------------------------------------------------------------------- under the Trainer
def _product(cfg, sd, ratio=0.75):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd)
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), train_mask_ratio=ratio)
    m.train()
    return m


def _step(model, tr, cfg, B, seed):
    from oracle import microdit_ref as orc
    batch, rnd, epsn, mnoise = orc.synth_batch(cfg, B, seed)
    mb = tr.microbatch_size
    chunks = [(rnd[i:i + mb].cuda(), epsn[i:i + mb].cuda(), mnoise[i:i + mb].cuda()) for i in range(0, B, mb)]
    model._noise_fn = lambda b, c=chunks: c.pop(0)
    loss = tr.train_step({k: t.cuda() for k, t in batch.items()})
    torch.cuda.synchronize()
    return loss


def _close(a, b, tol):
    return abs(a - b) <= tol * abs(b) if b != 0 else a == 0


def test_trainer_monitor_and_skipped_step_on_one_rank(hip):
    from oracle import microdit_ref as orc
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    cfg = orc.tiny_config()
    model = _product(cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 33)))
    opt = FusedAdamW(model.dit, lr=2.4e-4, skip_nonfinite=True)
    tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2, monitor_interval=1)
    f = model.dit.flat_buffers()
    names = list(f["P"])
    assert tr.tensor_stats() == {}
    # ---- step 1: finite
    before = {n: v.detach().clone() for n, v in f["P"].items()}
    _step(model, tr, cfg, 4, 500)
    stats = tr.tensor_stats()
    for n in names:
        for key in ("l2_norm/grad/", "l2_norm/param/", "absmax/grad/", "nonfinite/grad/"):
            assert key + n in stats, key + n
        assert stats["nonfinite/grad/" + n] == 0
        want = float(torch.linalg.norm(before[n].double().flatten()))
        assert _close(stats["l2_norm/param/" + n], want, TOL), (n, stats["l2_norm/param/" + n], want)
    glob = stats["l2_norm/grad/global"]
    gn = float(opt.grad_norm())
    print("global grad norm: monitor %.9g  optimizer %.9g" % (glob, gn))
    assert glob > 0 and _close(glob, gn, TOL), (glob, gn)
    assert _close(glob, math.sqrt(sum(stats["l2_norm/grad/" + n] ** 2 for n in names)), 1e-6)
    assert opt.skipped_steps() == 0
    assert not torch.equal(f["P"][names[0]], before[names[0]])
    # ---- step 2: +Inf in one element of one accumulator; the backward accumulates onto it
    bad = next(n for n, v in f["P"].items() if v.dim() == 2 and n.startswith("blocks.0."))
    f["G"][bad].view(-1)[5] = float("inf")
    p, m, v, s = f["p"].clone(), opt.m.clone(), opt.v.clone(), f["s"].clone()
    loss = _step(model, tr, cfg, 4, 501)
    assert bool(torch.isfinite(loss))
    assert torch.equal(f["p"], p) and torch.equal(opt.m, m) and torch.equal(opt.v, v) and torch.equal(f["s"], s)
    assert opt.skipped_steps() == 1
    stats = tr.tensor_stats()
    assert {n for n in names if stats["nonfinite/grad/" + n] != 0} == {bad} and stats["nonfinite/grad/" + bad] == 1
    assert math.isfinite(stats["l2_norm/grad/" + bad]) and not bool(torch.isfinite(opt.grad_norm()))
    assert float(f["g"].abs().max()) == 0.0
    # ---- step 3: finite again
    _step(model, tr, cfg, 4, 502)
    assert not torch.equal(f["p"], p) and opt.skipped_steps() == 1
    assert all(tr.tensor_stats()["nonfinite/grad/" + n] == 0 for n in names)


def test_defaults_change_nothing(hip, monkeypatch):
    """One step without the new arguments and a twin with both switches on, from the same state and noise, in deterministic mode:
    bit-equal weights, moments and bf16 shadow."""
    from oracle import microdit_ref as orc
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    monkeypatch.setenv("MD_DETERMINISTIC", "1")
    cfg = orc.tiny_config()
    sd = orc.dezero_state_dict(orc.synth_state_dict(cfg, 35))
    ends = []
    for on in (False, True):
        model = _product(cfg, sd)
        opt = FusedAdamW(model.dit, lr=2.4e-4, skip_nonfinite=True) if on else FusedAdamW(model.dit, lr=2.4e-4)
        tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2, **({"monitor_interval": 1} if on else {}))
        assert model.dit.engine.deterministic is True
        _step(model, tr, cfg, 4, 510)
        f = model.dit.flat_buffers()
        ends.append((f["p"].clone(), opt.m.clone(), opt.v.clone(), f["s"].clone()))
        assert (opt.guard_state is not None) == on and bool(tr._stats_plans) == on
    for a, b in zip(*ends):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- exchange paths, one rank
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _exchange_main(port, dp_mode, out_path):
    """One rank over backend "nccl" with single_rank_exchange (the recipe of tests/test_dp_gpu.py): the statistics pass reads the
    bf16 buffers the exchange mode holds."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from oracle import microdit_ref as orc
        from micro_diffusion_amd.trainer import FusedAdamW, LRSchedule, Trainer
        cfg = orc.tiny_config()
        model = _product(cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 61)))
        opt = FusedAdamW(model.dit, lr=2.4e-4)
        tr = Trainer(model, opt, LRSchedule("constant", alpha=1.0), clip_norm=0.25, microbatch_size=4, exchange="bf16",
                     single_rank_exchange=True, dp_mode=dp_mode, monitor_interval=1)
        assert tr.sync.enabled and tr.sync.mode == dp_mode and tr.sharded == (dp_mode == "sharded")
        held, inner = {}, tr.collect_tensor_stats

        def capture():                     # what the mode holds right before the optimiser pass
            held["gbf"] = tr.sync.gbf.clone()
            if dp_mode == "sharded":
                held["gred"] = tr.sync.gred.clone()
            inner()
        tr.collect_tensor_stats = capture
        _step(model, tr, cfg, 8, 62)
        stats = tr.tensor_stats()
        f = model.dit.flat_buffers()
        worst = 0.0
        for n, view in f["P"].items():
            o, cnt = f["offs"][n], view.numel()
            src = held["gbf"][o:o + cnt]
            if dp_mode == "sharded" and not (tr.sync.small is not None and o >= tr.sync.small[0]):
                _, lo, hi, chunk, olo = next(b for b in tr.sync.plan if b[1] <= o < b[2])
                src = held["gred"][olo + (o - lo): olo + (o - lo) + cnt]
            want = float(torch.linalg.norm(src.double()))
            got = stats["l2_norm/grad/" + n]
            assert _close(got, want, TOL), (n, got, want)
            assert stats["nonfinite/grad/" + n] == 0
            worst = max(worst, abs(got - want) / want if want else 0.0)
        glob, gn = stats["l2_norm/grad/global"], float(opt.grad_norm())
        assert glob > 0 and _close(glob, gn, TOL), (glob, gn)
        tr.sync.wait_gather()
        torch.cuda.synchronize()
        torch.save({"ok": True, "worst": worst, "global": glob, "grad_norm": gn}, out_path)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dp_mode", ["allreduce", "sharded"])
def test_trainer_monitor_on_the_exchange_paths(hip, dp_mode):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "r.pt")
        proc = mp.get_context("spawn").Process(target=_exchange_main, args=(_free_port(), dp_mode, out))
        proc.start()
        proc.join(600)
        assert proc.exitcode == 0, f"one-rank exchange process failed: {proc.exitcode}"
        r = torch.load(out)
    print(dp_mode, r)
    assert r["ok"]
