"""Post-hoc EMA on the GPU: md_ema_power_update[_ranges] against float64 torch, the guard, the range form and the argument checks;
then FusedAdamW(posthoc_sigma_rels=...) under the Trainer -- one rank, a skipped step, two sharded ranks, save / resume -- and the
whole chain train.py snapshots -> scripts/posthoc_ema.py -> dit.load_state_dict.

Tolerances.  One update e' = beta * e + (1.f - beta) * p in fp32 is one rounding of (1.f - beta), two products and one sum, which the
compiler may contract into an FMA either way: |got - ref| <= 2^-22 * max(|e|, |p|) against the same expression in fp64.  t chained
updates (the optimiser tests) add up to t * 2^-22 * the largest max(|e|, |p|) seen on the way (beta < 1 only damps earlier errors): 8
steps -> 8 * 2^-22.  Everything else is compared bit for bit.  The end-to-end bound is the one of tests/test_posthoc_ema_cpu.py:
|| rec - tracked || / || tracked - theta_final || <= 0.01."""
import ctypes
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -22
N = 3 * 1024 + 4          # more than one workgroup iteration's worth for a small grid, a ragged last workgroup
PAD = 64                  # canary elements on both sides (a multiple of 4: the payload stays 16-byte aligned)
SIGMA_RELS = (0.05, 0.10)


# ---------------------------------------------------------------------------------------------------- raw buffers
def _case(K, seed):
    """p and K profiles, each inside its own canary frame; betas that differ per profile."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(N + 2 * PAD, device=DEV, generator=g)
    es = [torch.randn(N + 2 * PAD, device=DEV, generator=g) * (0.5 + k) for k in range(K)]
    for e in es:
        e[:PAD] = 12345.0
        e[-PAD:] = -54321.0
    betas = [0.9, 0.999, 0.37, 0.99999][:K]
    return p, es, betas


def _ref(p, e, beta):
    """The kernel's expression evaluated in fp64 on the fp32 operands (beta and 1.f - beta as the fp32 numbers the kernel holds)."""
    b = torch.tensor(beta, dtype=torch.float32)
    return b.double().item() * e.double() + (torch.tensor(1.0) - b).double().item() * p.double()


def _canaries_ok(e):
    return bool((e[:PAD] == 12345.0).all()) and bool((e[-PAD:] == -54321.0).all())


@pytest.mark.parametrize("K", [1, 2, 4])
def test_kernel_against_torch(hip, K):
    p, es, betas = _case(K, 10 + K)
    before = [e.clone() for e in es]
    hip.ema_power_update(p[PAD:], [e[PAD:] for e in es], betas, N)
    torch.cuda.synchronize()
    for k in range(K):
        got, ref = es[k][PAD:PAD + N].double(), _ref(p[PAD:PAD + N], before[k][PAD:PAD + N], betas[k])
        bound = EPS * torch.maximum(before[k][PAD:PAD + N].abs(), p[PAD:PAD + N].abs()).double()
        worst = float(((got - ref).abs() / bound).max())
        print(f"K {K} profile {k} beta {betas[k]}: worst |got - ref| / (2^-22 max(|e|, |p|)) = {worst:.3f}")
        assert worst <= 1.0
        assert not torch.equal(es[k], before[k]) and _canaries_ok(es[k])


@pytest.mark.parametrize("K", [1, 2, 4])
def test_beta_zero_copies_the_weights_over_nan(hip, K):
    p, es, _ = _case(K, 20 + K)
    for e in es:
        e[PAD:PAD + N] = float("nan")
    betas = [0.0] * K
    if K > 1:
        betas[1] = 0.5                # a live profile next to first-step ones: its NaN stays NaN, the others are exact copies
    hip.ema_power_update(p[PAD:], [e[PAD:] for e in es], betas, N)
    torch.cuda.synchronize()
    for k in range(K):
        if betas[k] == 0.0:
            assert torch.equal(es[k][PAD:PAD + N], p[PAD:PAD + N]), k
        else:
            assert bool(torch.isnan(es[k][PAD:PAD + N]).all())
        assert _canaries_ok(es[k])


def test_guard(hip):
    p, es, betas = _case(4, 31)
    before = [e.clone() for e in es]
    stop = torch.zeros(4, device=DEV, dtype=torch.int32)
    go = torch.tensor([1, 0, 0, 0], device=DEV, dtype=torch.int32)
    hip.ema_power_update(p[PAD:], [e[PAD:] for e in es], betas, N, guard=stop)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(es, before)), "guard 0 must leave every profile untouched"
    hip.ema_power_update(p[PAD:], [e[PAD:] for e in es], betas, N, guard=go)
    plain = [e.clone() for e in before]
    hip.ema_power_update(p[PAD:], [e[PAD:] for e in plain], betas, N)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(es, plain)), "guard 1 must equal the unguarded launch"
    assert not torch.equal(es[0], before[0])


def test_ranges(hip):
    n = 64 * 700
    ranges = [(64 * 3, 64 * 10), (64 * 40 + 4, 64 * 100 + 8), (64 * 600, 64 * 100 - 4)]         # gaps between and around them
    g = torch.Generator(device=DEV).manual_seed(41)
    p = torch.randn(n + 2 * PAD, device=DEV, generator=g)
    es = [torch.randn(n + 2 * PAD, device=DEV, generator=g) for _ in range(3)]
    for e in es:
        e[:PAD] = 12345.0
        e[-PAD:] = -54321.0
    betas = [0.9, 0.0, 0.999]
    before = [e.clone() for e in es]
    flat = [e.clone() for e in es]
    hip.ema_power_update(p[PAD:], [e[PAD:] for e in flat], betas, n)
    hip.ema_power_update(p[PAD:], [e[PAD:] for e in es], betas, 0, flat_off=[o for o, _ in ranges], count=[c for _, c in ranges])
    torch.cuda.synchronize()
    touched = torch.zeros(n + 2 * PAD, dtype=torch.bool, device=DEV)
    for o, c in ranges:
        touched[PAD + o:PAD + o + c] = True
    for k in range(3):
        assert torch.equal(es[k][touched], flat[k][touched]), k
        assert torch.equal(es[k][~touched], before[k][~touched]), k
        assert not torch.equal(es[k][touched], before[k][touched]) and _canaries_ok(es[k])
    # the guard of the range form
    stop = torch.zeros(4, device=DEV, dtype=torch.int32)
    again = [e.clone() for e in es]
    hip.ema_power_update(p[PAD:], [e[PAD:] for e in again], betas, 0, guard=stop, flat_off=[o for o, _ in ranges], count=[c for _, c in ranges])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, es))


def test_bad_arguments_launch_nothing(hip):
    p, es, betas = _case(2, 51)
    before = [e.clone() for e in es]
    ptrs = [e[PAD:] for e in es]
    call = lambda *a, **k: hip.ema_power_update(*a, expect=None, **k)
    assert call(None, ptrs, betas, N) == -1
    assert call(p[PAD:], [ptrs[0], None], betas, N) == -1
    assert call(p[PAD:], ptrs, betas, N + 2) == -1
    assert call(p[PAD:], ptrs, betas, 0) == -1
    assert call(p[PAD:], [], [], N) == -1
    assert call(p[PAD:], ptrs * 3, betas * 3, N) == -1            # 6 profiles
    for b in (1.0, -0.5, float("nan")):
        assert call(p[PAD:], ptrs, [0.5, b], N) == -1, b
    assert call(p[PAD:], ptrs, betas, 0, flat_off=[0, 66], count=[32, 32]) == -1
    assert call(p[PAD:], ptrs, betas, 0, flat_off=[0, 64], count=[32, 0]) == -1
    assert call(p[PAD:], ptrs, betas, 0, flat_off=[0] * 65, count=[4] * 65) == -1
    L = hip.lib()
    ev, bv = (ctypes.c_void_p * 2)(*[e.data_ptr() for e in ptrs]), (ctypes.c_float * 2)(*betas)
    assert L.md_ema_power_update(p.data_ptr(), None, bv, 2, N, None, hip.stream_ptr()) == -1
    assert L.md_ema_power_update(p.data_ptr(), ev, None, 2, N, None, hip.stream_ptr()) == -1
    assert L.md_ema_power_update_ranges(p.data_ptr(), ev, bv, 2, None, None, 1, None, hip.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(es, before))


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


class _Replay:
    """Host replay of the averages over recorded masters: fp64, beta as the fp32 number the kernel receives; `scale` keeps the
    largest max(|e|, |p|) met on the way (the unit of the accumulated rounding bound)."""

    def __init__(self, sigma_rels):
        from micro_diffusion_amd import posthoc_ema as ph
        self.gammas, self.t, self.e, self.scale = [ph.sigma_rel_to_gamma(s) for s in sigma_rels], 0, None, None

    def add(self, p):
        from micro_diffusion_amd import posthoc_ema as ph
        p = p.detach().double().cpu()
        self.t += 1
        if self.e is None:
            self.e, self.scale = [p.clone() for _ in self.gammas], [p.abs() for _ in self.gammas]
        for k, g in enumerate(self.gammas):
            b = torch.tensor(ph.power_beta(self.t, g), dtype=torch.float32)
            if float(b) != 0.0:
                self.scale[k] = torch.maximum(self.scale[k], torch.maximum(self.e[k].abs(), p.abs()))
                self.e[k] = b.double().item() * self.e[k] + (torch.tensor(1.0) - b).double().item() * p
            else:
                self.e[k] = p.clone()

    def worst(self, k, got):
        """max |got - replay| in units of 2^-22 * scale (elements whose scale is 0 -- alignment padding -- must be equal)."""
        d = (got.detach().double().cpu() - self.e[k]).abs()
        s = self.scale[k]
        assert bool((d[s == 0] == 0).all())
        return float((d[s > 0] / (EPS * s[s > 0])).max())


def _train(cfg, sd, steps, sigma_rels, first_seed=700, resume=None, **opt_kw):
    """`steps` deterministic Tiny steps; returns what the tests compare.  resume = (model state, optimiser state) continues a run."""
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    model = _product(cfg, sd)
    kw = dict(posthoc_sigma_rels=sigma_rels) if sigma_rels else {}
    opt = FusedAdamW(model.dit, lr=2.4e-4, **kw, **opt_kw)
    if resume is not None:
        model.dit.load_state_dict(resume[0])
        opt.load_state_dict(resume[1])
    tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2)
    assert model.dit.engine.deterministic is True
    f = model.dit.flat_buffers()
    masters = []
    for i in range(steps):
        _step(model, tr, cfg, 4, first_seed + opt.step_count)
        masters.append(f["p"].clone())
    return {"model": model, "opt": opt, "tr": tr, "masters": masters, "p": f["p"].clone(), "m": opt.m.clone(), "v": opt.v.clone(),
            "s": f["s"].clone(), "posthoc": [e.clone() for e in opt.posthoc]}


@pytest.fixture(scope="module")
def runs(hip):
    """The 8-step run with the profiles (0.05, 0.10) and its twin without them, in deterministic mode (bit-reproducible gradients),
    computed once for the tests below; plus the state saved after step 4 of a third, identical run."""
    from oracle import microdit_ref as orc
    old = os.environ.get("MD_DETERMINISTIC")
    os.environ["MD_DETERMINISTIC"] = "1"
    try:
        cfg = orc.tiny_config()
        sd = orc.dezero_state_dict(orc.synth_state_dict(cfg, 71))
        on = _train(cfg, sd, 8, SIGMA_RELS)
        off = _train(cfg, sd, 8, None)
        half = _train(cfg, sd, 4, SIGMA_RELS)
        saved = ({k: v.detach().cpu().clone() for k, v in half["model"].dit.state_dict().items()},
                 _to_cpu(half["opt"].state_dict()))
        del half
        resumed = _train(cfg, sd, 4, SIGMA_RELS, resume=saved)
        yield {"cfg": cfg, "sd": sd, "on": on, "off": off, "resumed": resumed, "saved": saved}
    finally:
        if old is None:
            os.environ.pop("MD_DETERMINISTIC", None)
        else:
            os.environ["MD_DETERMINISTIC"] = old


def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if isinstance(x, dict):
        return {k: _to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_cpu(v) for v in x)
    return x


def test_optimizer_tracks_the_profiles_and_changes_nothing_else(runs):
    on, off = runs["on"], runs["off"]
    for k in ("p", "m", "v", "s"):
        assert torch.equal(on[k], off[k]), f"{k} differs between the run with and the run without the profiles"
    assert all(torch.equal(a, b) for a, b in zip(on["masters"], off["masters"]))
    assert off["opt"].posthoc == [] and "posthoc" not in off["opt"].state_dict()
    assert len(on["opt"].posthoc) == 2 and on["opt"].step_count == 8
    rp = _Replay(SIGMA_RELS)
    for p in on["masters"]:
        rp.add(p)
    for k in range(2):
        worst = rp.worst(k, on["posthoc"][k])
        print(f"profile {k} (sigma_rel {SIGMA_RELS[k]}): worst deviation from the host replay = {worst:.3f} x 2^-22 x scale (bound 8)")
        assert worst <= 8.0
        assert not torch.equal(on["posthoc"][k], on["p"])
    assert not torch.equal(on["posthoc"][0], on["posthoc"][1])
    sd = on["opt"].state_dict()["posthoc"]
    assert sd["sigma_rels"] == list(SIGMA_RELS) and len(sd["ema"]) == 2
    names = set(on["model"].dit.flat_buffers()["P"])
    assert set(sd["ema"][0]) == names == set(on["opt"].posthoc_state_dict(1))
    f = on["model"].dit.flat_buffers()
    for n, v in on["opt"].posthoc_state_dict(1).items():
        assert v.shape == f["P"][n].shape
        o = f["offs"][n]
        assert torch.equal(v.reshape(-1), on["posthoc"][1][o:o + v.numel()])


def test_swap_ema_evaluates_on_a_profile(runs):
    on = runs["on"]
    opt, f = on["opt"], on["model"].dit.flat_buffers()
    with opt.swap_ema() as active:            # default argument: the fixed-length EMA, which this run does not configure
        assert active is False and torch.equal(f["p"], on["p"])
    with opt.swap_ema(profile=1) as active:
        assert active is True
        assert torch.equal(f["p"], on["posthoc"][1]) and torch.equal(f["s"], on["posthoc"][1].to(torch.bfloat16))
    torch.cuda.synchronize()
    assert torch.equal(f["p"], on["p"]) and torch.equal(opt.posthoc[1], on["posthoc"][1]) and torch.equal(f["s"], on["s"])
    with pytest.raises(IndexError):
        opt.swap_ema(profile=2).__enter__()


def test_save_and_resume_continue_the_profiles(runs):
    on, re_ = runs["on"], runs["resumed"]
    assert "posthoc" in runs["saved"][1] and re_["opt"].step_count == 8
    assert torch.equal(re_["p"], on["p"]) and torch.equal(re_["m"], on["m"])
    for k in range(2):
        assert torch.equal(re_["posthoc"][k], on["posthoc"][k]), f"profile {k} differs after save at step 4 + resume"


def test_load_state_dict_checks_the_profile_list(runs, monkeypatch):
    from micro_diffusion_amd.trainer import FusedAdamW
    monkeypatch.setenv("MD_DETERMINISTIC", "1")
    model = _product(runs["cfg"], runs["sd"])
    with pytest.raises(RuntimeError, match="post-hoc EMA profiles"):
        FusedAdamW(model.dit, posthoc_sigma_rels=(0.05, 0.10, 0.15)).load_state_dict(runs["saved"][1])
    with pytest.warns(UserWarning, match="sigma_rels"):
        FusedAdamW(model.dit, posthoc_sigma_rels=(0.05, 0.12)).load_state_dict(runs["saved"][1])
    with pytest.warns(UserWarning, match="dropped"):
        FusedAdamW(model.dit).load_state_dict(runs["saved"][1])
    with pytest.raises(ValueError):
        FusedAdamW(model.dit, posthoc_sigma_rels=(0.05, 0.06, 0.07, 0.08, 0.09))


def test_non_finite_step_leaves_the_profiles_alone(hip, monkeypatch):
    from oracle import microdit_ref as orc
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    monkeypatch.setenv("MD_DETERMINISTIC", "1")
    cfg = orc.tiny_config()
    model = _product(cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 72)))
    opt = FusedAdamW(model.dit, lr=2.4e-4, skip_nonfinite=True, posthoc_sigma_rels=SIGMA_RELS)
    tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2)
    f = model.dit.flat_buffers()
    _step(model, tr, cfg, 4, 800)
    _step(model, tr, cfg, 4, 801)
    assert opt.skipped_steps() == 0 and not torch.equal(opt.posthoc[0], f["p"])
    before, p = [e.clone() for e in opt.posthoc], f["p"].clone()
    bad = next(n for n, v in f["P"].items() if v.dim() == 2 and n.startswith("blocks.0."))
    f["G"][bad].view(-1)[5] = float("nan")
    _step(model, tr, cfg, 4, 802)
    assert opt.skipped_steps() == 1 and opt.step_count == 3 and torch.equal(f["p"], p)
    assert all(torch.equal(a, b) for a, b in zip(opt.posthoc, before)), "a skipped step must not move the averages"
    _step(model, tr, cfg, 4, 803)
    assert opt.skipped_steps() == 1 and not torch.equal(opt.posthoc[0], before[0])


# ---------------------------------------------------------------------------------------------------- two sharded ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, out_path):
    """Two processes on cuda:0, gloo rendezvous (the pattern of tests/test_dp_gpu.py): 3 sharded steps, consolidating after each."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import microdit_ref as orc
        from micro_diffusion_amd.trainer import FusedAdamW, LRSchedule, Trainer
        cfg = orc.tiny_config()
        model = _product(cfg, orc.synth_state_dict(cfg, 61))
        opt = FusedAdamW(model.dit, lr=2.4e-4, posthoc_sigma_rels=SIGMA_RELS)
        tr = Trainer(model, opt, LRSchedule("constant", alpha=1.0), clip_norm=0.25, microbatch_size=4, exchange="bf16", dp_mode="sharded")
        assert tr.world == world and tr.sharded
        f = model.dit.flat_buffers()
        rp = _Replay(SIGMA_RELS)
        for i in range(3):
            batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 8, 900 + i)
            lo = rank * 4
            model._noise_fn = lambda b, lo=lo: (rnd[lo:lo + 4].cuda(), epsn[lo:lo + 4].cuda(), mnoise[lo:lo + 4].cuda())
            tr.train_step({k: v[lo:lo + 4].cuda() for k, v in batch.items()})
            assert tr.stale_foreign_chunks
            tr.consolidate()
            torch.cuda.synchronize()
            rp.add(f["p"])
        mine = torch.stack([e.detach().cpu() for e in opt.posthoc] + [f["p"].detach().cpu()])
        gathered = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
        if rank == 0:
            torch.save({"identical": all(torch.equal(gathered[0], g) for g in gathered),
                        "worst": [rp.worst(k, opt.posthoc[k]) for k in range(2)],
                        "moved": not torch.equal(opt.posthoc[0], f["p"]), "ranges": len(tr.sync.plan), "small": tr.sync.small is not None},
                       out_path)
    finally:
        dist.destroy_process_group()


def test_two_sharded_ranks_keep_identical_profiles(hip):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rank0.pt")
        ctx = mp.get_context("spawn")
        port = _free_port()
        procs = [ctx.Process(target=_rank_main, args=(r, 2, port, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
        codes = [p.exitcode for p in procs]
        assert codes == [0, 0], f"rank processes failed: {codes}"
        r = torch.load(out)
    print(r)
    assert r["identical"], "the ranks' consolidated profiles (or masters) differ"
    assert r["moved"] and r["ranges"] >= 3 and r["small"]
    assert max(r["worst"]) <= 3.0, r["worst"]           # 3 chained updates


# ---------------------------------------------------------------------------------------------------- end to end
def test_snapshots_to_reconstruction_end_to_end(hip, monkeypatch, tmp_path):
    """256 Tiny steps tracking (0.05, 0.075, 0.10); the first and the third are snapshotted every 16 steps the way train.py does it;
    scripts/posthoc_ema.py --sigma-rel 0.075 must give back the second, which no snapshot holds."""
    import train
    from oracle import microdit_ref as orc
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    cfg = orc.tiny_config()
    model = _product(cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 73)))
    opt = FusedAdamW(model.dit, lr=2.4e-4, posthoc_sigma_rels=(0.05, 0.075, 0.10))
    tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2)
    draws = []
    for i in range(8):                           # eight recorded batches, visited in turn
        batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 2, 1000 + i)
        draws.append(({k: t.cuda() for k, t in batch.items()}, (rnd.cuda(), epsn.cuda(), mnoise.cuda())))
    folder = str(tmp_path / "posthoc")
    for step in range(1, 257):
        batch, noise = draws[step % 8]
        model._noise_fn = lambda b, n=noise: n
        tr.train_step(batch)
        if step % 16 == 0:
            tr.consolidate()
            train.save_posthoc_snapshots(opt, folder, step, profiles=(0, 2))
    torch.cuda.synchronize()
    names = sorted(os.listdir(folder))
    assert len(names) == 32 and names[0] == "ema-00000016-0.050.pt" and names[-1] == "ema-00000256-0.100.pt", names[:3]
    out = str(tmp_path / "ema_0.075.pt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "posthoc_ema.py"), "--snapshots", folder, "--sigma-rel", "0.075",
                        "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    sd = torch.load(out, map_location="cpu")
    want = model.dit.state_dict()
    assert set(sd) == set(want) and all(sd[k].shape == want[k].shape for k in want)
    tracked = {k: v.detach().cpu().double() for k, v in opt.posthoc_state_dict(1).items()}
    final = {k: want[k].detach().cpu().double() for k in tracked}
    num = sum(float(((sd[k].double() - tracked[k]) ** 2).sum()) for k in tracked) ** 0.5
    den = sum(float(((tracked[k] - final[k]) ** 2).sum()) for k in tracked) ** 0.5
    away = [sum(float(((opt.posthoc_state_dict(j)[k].detach().cpu().double() - tracked[k]) ** 2).sum()) for k in tracked) ** 0.5 / den
            for j in (0, 2)]
    print(f"reconstruction of sigma_rel 0.075: error {num / den:.3g} of || tracked - theta_final || = {den:.3g}; the snapshotted "
          f"profiles lie {away[0]:.3g} and {away[1]:.3g} away")
    assert num / den <= 0.01
    model.dit.load_state_dict(sd)                # strict: every key, every shape
