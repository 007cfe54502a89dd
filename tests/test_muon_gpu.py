"""Muon as an optimiser (muon.Muon) on the GPU, Tiny widths: the AdamW part is the unchanged kernel on the unchanged
values, the Muon part moves every targeted matrix along the Newton-Schulz direction of tests/muon_ref.py, the step guard, save / resume,
the refusals, three Trainer steps on MicroDiT_Tiny_2 and two data-parallel ranks.

Most tests plant a synthetic gradient in the flat accumulator and call opt.step() directly: both optimisers then see identical bits.
The gradient of a targeted matrix is built like the Newton-Schulz test inputs of tests/muon_ref.py (Gaussian for the non-square shapes,
prescribed singular values for the square ones), so that the first step's X = u / ||u|| stays in the converged regime -- asserted per
matrix before the error bound is applied.

Update direction: with decay and lr * s known exactly, D = (p * decay - p') / (lr * s) recovers O up to the rounding of p' (2^-24 |p|
against an update of about 1e-5: a relative 1e-5, three orders below the bound).  With R = ns_fp64(X) the rule of the kernel test holds:
||D - R|| / ||R|| <= 2 e_emu, e_emu the distance of the CPU emulation (bf16 after A, B and X) from R."""
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import muon_ref as ref

pytestmark = pytest.mark.gpu
LR, WD = 2.0 ** -12, 0.125            # decay = 1 - 2^-15 exactly, fused or not


def _product(cfg, sd, ratio=0.75):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd)
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), train_mask_ratio=ratio)
    m.train()
    return m


@pytest.fixture(scope="module")
def tiny(hip):
    from oracle import microdit_ref as orc
    cfg = orc.tiny_config()
    return cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 81))


def _grad(dit, seed):
    """A flat synthetic gradient: Gaussian on every parameter (the alignment padding stays zero), the square targeted matrices replaced
    by matrices of prescribed singular values."""
    from micro_diffusion_amd import muon
    f = dit.flat_buffers()
    gen = torch.Generator().manual_seed(seed)
    g = torch.zeros(f["total"])
    for name, view in f["P"].items():
        o = f["offs"][name]
        g[o:o + view.numel()] = torch.randn(view.numel(), generator=gen) * 1e-2
    specs = muon.resolve_targets(dit._table, muon.DEFAULT_TARGETS)
    for k, (o, r, c, _) in enumerate(muon.matrices_of(specs, f["offs"])):
        if r == c:
            g[o:o + r * c] = ref.ns_input(r, c, seed * 1000 + k).float().reshape(-1) * 1e-2
    return g.cuda()


def _pair(tiny, seed, **kw):
    """A Muon and a FusedAdamW optimiser on two models of identical weights with the same planted gradient."""
    from micro_diffusion_amd.muon import Muon
    from micro_diffusion_amd.trainer import FusedAdamW
    cfg, sd = tiny
    ma, mb = _product(cfg, sd), _product(cfg, sd)
    mu, ad = Muon(ma.dit, lr=LR, weight_decay=WD, **kw), FusedAdamW(mb.dit, lr=LR, weight_decay=WD, **kw)
    g = _grad(ma.dit, seed)
    for m in (ma, mb):
        m.dit.flat_buffers()["g"].copy_(g)
    return ma, mu, mb, ad, g


def _targeted_mask(opt):
    m = torch.zeros(opt.m.numel(), dtype=torch.bool, device=opt.m.device)
    for o, r, c, _ in opt.matrices:
        m[o:o + r * c] = True
    return m


# ---------------------------------------------------------------------------------------------------- the AdamW part
@pytest.mark.parametrize("variant", ["plain", "clipped", "skip_nonfinite", "ema"])
def test_adamw_tensors_are_unchanged(tiny, variant):
    kw = {"skip_nonfinite": dict(skip_nonfinite=True), "ema": dict(ema_smoothing=0.99)}.get(variant, {})
    max_norm = 1e-3 if variant == "clipped" else 0.0
    ma, mu, mb, ad, g = _pair(tiny, 5, **kw)
    for steps in range(2):                    # the second step runs the live-EMA form and non-zero moments
        for m, o in ((ma, mu), (mb, ad)):
            if steps:
                m.dit.flat_buffers()["g"].copy_(g * 0.5)
            o.step(max_norm=max_norm)
    torch.cuda.synchronize()
    if variant == "clipped":
        assert float(mu.grad_norm()) > 10 * max_norm and torch.equal(mu.sumsq, ad.sumsq)
    fa, fb = ma.dit.flat_buffers(), mb.dit.flat_buffers()
    keep = ~_targeted_mask(mu)
    bufs = [("master", fa["p"], fb["p"]), ("m", mu.m, ad.m), ("v", mu.v, ad.v), ("shadow", fa["s"], fb["s"]), ("g", fa["g"], fb["g"])]
    if variant == "ema":
        bufs.append(("ema", mu.ema, ad.ema))
    for name, a, b in bufs:
        assert torch.equal(ref.bits(a)[keep], ref.bits(b)[keep]), f"{variant}: {name} of the non-targeted tensors differs from FusedAdamW's"
    for n in fa["P"]:                         # and tensor by tensor, as the issue words it
        if mu.rules[n] == "adamw":
            assert torch.equal(fa["P"][n], fb["P"][n]) and torch.equal(fa["S"][n], fb["S"][n]), n
    assert int((mu.v[~keep] != 0).sum()) == 0, "v stays zero on the targeted tensors"
    assert not torch.equal(fa["p"][~keep], fb["p"][~keep]) and int((fa["g"] != 0).sum()) == 0
    assert torch.equal(ref.bits(fa["s"]), ref.bits(fa["p"].to(torch.bfloat16))), "the shadow is bf16(master) everywhere"
    if variant == "ema":
        tm = ~keep
        assert mu.ema_live and not torch.equal(mu.ema[tm], fa["p"][tm])
        assert int((mu.ema[tm] == 0).sum()) < 10, "the EMA of the targeted tensors is live"


# ---------------------------------------------------------------------------------------------------- the Muon part
@pytest.mark.parametrize("adjust,nesterov", [("rms", True), ("spectral", False)])
def test_update_direction(tiny, adjust, nesterov):
    from micro_diffusion_amd import muon
    from micro_diffusion_amd.muon import Muon
    cfg, sd = tiny
    model = _product(cfg, sd)
    opt = Muon(model.dit, lr=LR, weight_decay=WD, adjust=adjust, nesterov=nesterov)
    f = model.dit.flat_buffers()
    g = _grad(model.dit, 7)
    f["g"].copy_(g)
    p0 = f["p"].clone()
    opt.step()
    torch.cuda.synchronize()
    p0, p1, g, m1 = p0.cpu(), f["p"].cpu(), g.cpu(), opt.m.cpu()
    decay = torch.tensor(ref.decay_of(LR, WD), dtype=torch.float32)
    worst = 0.0
    for k, (o, r, c, name) in enumerate(opt.matrices):
        sl = slice(o, o + r * c)
        m_ref, u = ref.momentum_ref(g[sl], torch.zeros(r * c), 1.0, 0.95, nesterov)
        assert torch.equal(ref.bits(m1[sl]), ref.bits(m_ref)), f"{name}: the momentum is not the reference's"
        nrm, inv, x = ref.normalise_ref(u)
        assert abs(float(opt.norms[k]) - nrm) <= 1e-12 * nrm
        x = x.view(r, c)
        R, emu = ref.ns_fp64(x), ref.ns_bf16_emulated(x)
        sv = torch.linalg.svdvals(R)
        assert float(sv.min()) >= 0.5 and float(sv.max()) <= 1.3, f"{name} [{r} x {c}]: the test input left the converged regime"
        s = muon.shape_scale(adjust, r, c)
        D = ((p0[sl] * decay).double() - p1[sl].double()).view(r, c) / (float(torch.tensor(LR, dtype=torch.float32)) * s)
        e_gpu, e_emu = ref.rel_err(D, R), ref.rel_err(emu, R)
        worst = max(worst, e_gpu / e_emu)
        assert e_gpu <= 2 * e_emu, f"{name} [{r} x {c}]: e_gpu {e_gpu:.4e} > 2 x e_emu {e_emu:.4e}"
    print(f"{adjust}, nesterov={nesterov}: {len(opt.matrices)} matrices, worst e_gpu / e_emu = {worst:.3f}")
    # no gradient and no momentum: the update is the decay alone, exactly
    f["g"].zero_()
    opt.m.zero_()
    p1 = f["p"].clone()
    opt.step()
    torch.cuda.synchronize()
    tm = _targeted_mask(opt)
    assert torch.equal(f["p"][tm], (p1 * decay.cuda())[tm]), "with u = 0 a targeted weight is fl(p * decay) bit for bit"


def test_skip_nonfinite(tiny):
    from micro_diffusion_amd.muon import Muon
    cfg, sd = tiny
    model = _product(cfg, sd)
    opt = Muon(model.dit, lr=LR, weight_decay=WD, skip_nonfinite=True, ema_smoothing=0.99)
    f = model.dit.flat_buffers()
    g = _grad(model.dit, 9)
    f["g"].copy_(g)
    opt.step(max_norm=0.25)
    assert opt.skipped_steps() == 0 and int((f["g"] != 0).sum()) == 0
    p, m, v, e, s = f["p"].clone(), opt.m.clone(), opt.v.clone(), opt.ema.clone(), f["s"].clone()
    f["g"].copy_(g)
    name = opt.specs[3].name
    f["G"][name].view(-1)[17] = float("inf")
    opt.step(max_norm=0.25)
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 and opt.step_count == 2
    for what, a, b in (("masters", f["p"], p), ("momentum / m", opt.m, m), ("v", opt.v, v), ("ema", opt.ema, e), ("shadow", f["s"], s)):
        assert torch.equal(ref.bits(a), ref.bits(b)), f"{what} moved on a skipped step"
    assert int((f["g"] != 0).sum()) == 0 and not bool(torch.isnan(f["g"]).any()), "the gradients are zeroed on a skipped step"
    f["g"].copy_(g)
    opt.step(max_norm=0.25)
    assert opt.skipped_steps() == 1 and not torch.equal(f["p"], p) and bool(torch.isfinite(f["p"]).all())


def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if isinstance(x, dict):
        return {k: _to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_cpu(v) for v in x)
    return x


def test_save_and_resume(tiny):
    from micro_diffusion_amd.muon import Muon
    from micro_diffusion_amd.trainer import FusedAdamW
    cfg, sd = tiny
    kw = dict(lr=LR, weight_decay=WD, ema_smoothing=0.99, ema_start=1)
    whole = _product(cfg, sd)
    a = Muon(whole.dit, **kw)
    grads = [_grad(whole.dit, 20 + i) for i in range(3)]
    for g in grads:
        whole.dit.flat_buffers()["g"].copy_(g)
        a.step(max_norm=0.25)
    first = _product(cfg, sd)
    b = Muon(first.dit, **kw)
    for g in grads[:2]:
        first.dit.flat_buffers()["g"].copy_(g)
        b.step(max_norm=0.25)
    saved = ({k: v.detach().cpu().clone() for k, v in first.dit.state_dict().items()}, _to_cpu(b.state_dict()))
    assert saved[1]["muon"]["rules"] == b.rules and saved[1]["step"] == 2
    second = _product(cfg, sd)
    second.dit.load_state_dict(saved[0])
    c = Muon(second.dit, **kw)
    c.load_state_dict(saved[1])
    second.dit.flat_buffers()["g"].copy_(grads[2])
    c.step(max_norm=0.25)
    torch.cuda.synchronize()
    fw, fs = whole.dit.flat_buffers(), second.dit.flat_buffers()
    for what, x, y in (("masters", fw["p"], fs["p"]), ("m", a.m, c.m), ("v", a.v, c.v), ("ema", a.ema, c.ema), ("shadow", fw["s"], fs["s"])):
        assert torch.equal(ref.bits(x), ref.bits(y)), f"{what} differs after save at step 2 + resume"
    # a plain FusedAdamW checkpoint, or another target list, is refused
    plain = FusedAdamW(_product(cfg, sd).dit, lr=LR)
    with pytest.raises(RuntimeError, match="rule table"):
        c.load_state_dict(_to_cpu(plain.state_dict()))
    with pytest.raises(RuntimeError, match="rule table"):
        Muon(second.dit, targets=[r"attn\.proj\.weight$"], **kw).load_state_dict(saved[1])


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(tiny):
    from micro_diffusion_amd.lora import LoRA
    from micro_diffusion_amd.muon import Muon
    from micro_diffusion_amd.trainer import Trainer
    cfg, sd = tiny
    model = _product(cfg, sd)
    f = model.dit.flat_buffers()
    opt = Muon(model.dit, lr=LR)
    model.dit.refresh_shadow(force=True)
    p, s = f["p"].clone(), f["s"].clone()
    with pytest.raises(NotImplementedError, match="sharded"):
        Trainer(model, opt, None, dp_mode="sharded")
    with pytest.raises(NotImplementedError, match="sharded"):
        opt.step_sharded(None)
    adapter = LoRA(model.dit, rank=4).attach()
    s_lora = f["s"].clone()
    try:
        with pytest.raises(NotImplementedError, match="LoRA"):
            Muon(model.dit, lr=LR)
        f["g"].fill_(1.0)
        with pytest.raises(NotImplementedError, match="LoRA"):
            opt.step()
        torch.cuda.synchronize()
        assert torch.equal(f["s"], s_lora) and bool((f["g"] == 1.0).all())
    finally:
        adapter.detach()
    torch.cuda.synchronize()
    assert torch.equal(f["p"], p) and torch.equal(f["s"], s) and opt.step_count == 0 and int((opt.m != 0).sum()) == 0
    assert opt._ws is None, "nothing is allocated before the first step"
    tr = Trainer(model, opt, None)                 # "auto" resolves to the all-reduce form
    assert tr.sharded is False and tr.sync.mode == "allreduce"


# ---------------------------------------------------------------------------------------------------- under the Trainer
def _tiny2_run(model, p0, steps=3):
    from oracle import microdit_ref as orc
    from micro_diffusion_amd.muon import Muon
    from micro_diffusion_amd.trainer import Trainer
    f = model.dit.flat_buffers()
    f["p"].copy_(p0)
    f["g"].zero_()
    model.dit.refresh_shadow(force=True)
    opt = Muon(model.dit, lr=2.4e-4)
    tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2)
    assert model.dit.engine.deterministic is True
    losses, versions = [], [model.dit.engine.weights_version]
    cfg = model.dit.config
    for i in range(steps):
        batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 4, 300 + i)
        chunks = [(rnd[j:j + 2].cuda(), epsn[j:j + 2].cuda(), mnoise[j:j + 2].cuda()) for j in range(0, 4, 2)]
        model._noise_fn = lambda b, c=chunks: c.pop(0)
        losses.append(tr.train_step({k: t.cuda() for k, t in batch.items()}))
        versions.append(model.dit.engine.weights_version)
    torch.cuda.synchronize()
    return [float(x) for x in losses], versions, f["p"].clone(), opt


def test_three_trainer_steps_on_tiny_2(hip, monkeypatch):
    from oracle import microdit_ref as orc
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    monkeypatch.setenv("MD_DETERMINISTIC", "1")
    torch.manual_seed(3)
    d = mdit.MicroDiT_Tiny_2()
    d.load_state_dict(orc.dezero_state_dict({k: v.detach().clone() for k, v in d.state_dict().items()}))
    model = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), train_mask_ratio=0.75)
    model.train()
    f = model.dit.flat_buffers()
    p0 = f["p"].clone()
    losses, versions, p_a, opt = _tiny2_run(model, p0)
    print("losses", losses, "matrices", len(opt.matrices), "GEMM launches per step", opt.last_gemm_launches)
    assert all(torch.isfinite(torch.tensor(losses))) and len(set(versions)) == 4, (losses, versions)
    assert torch.equal(ref.bits(f["s"]), ref.bits(f["p"].to(torch.bfloat16))), "the shadow is bf16(master) everywhere"
    assert bool(torch.isfinite(f["p"]).all()) and not torch.equal(p_a, p0)
    tm = _targeted_mask(opt)
    assert int((opt.v[tm] != 0).sum()) == 0 and int((opt.m[tm] != 0).sum()) > 0.5 * int(tm.sum())
    assert opt.last_gemm_launches <= 15 * len(opt.matrices)
    losses_b, _, p_b, _ = _tiny2_run(model, p0)
    assert losses_b == losses and torch.equal(ref.bits(p_a), ref.bits(p_b)), "two deterministic runs must give identical masters"


# ---------------------------------------------------------------------------------------------------- two data-parallel ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, out_path):
    """Two processes on cuda:0, gloo rendezvous (the pattern of tests/test_dp_gpu.py): 2 all-reduce steps under Muon."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import microdit_ref as orc
        from micro_diffusion_amd.muon import Muon
        from micro_diffusion_amd.trainer import LRSchedule, Trainer
        cfg = orc.tiny_config()
        model = _product(cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 61)))
        opt = Muon(model.dit, lr=2.4e-4)
        tr = Trainer(model, opt, LRSchedule("constant", alpha=1.0), clip_norm=0.25, microbatch_size=4, dp_mode="allreduce")
        assert tr.world == world and not tr.sharded
        f = model.dit.flat_buffers()
        p0 = f["p"].clone()
        sync = []
        for i in range(2):
            batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 8, 900 + i)
            lo = rank * 4
            model._noise_fn = lambda b, lo=lo: (rnd[lo:lo + 4].cuda(), epsn[lo:lo + 4].cuda(), mnoise[lo:lo + 4].cuda())
            tr.train_step({k: v[lo:lo + 4].cuda() for k, v in batch.items()})
            sync.append(tr.replicas_in_sync())
        torch.cuda.synchronize()
        mine = torch.stack([f["p"].detach().cpu(), opt.m.detach().cpu()])
        gathered = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
        if rank == 0:
            torch.save({"sync": sync, "identical": all(torch.equal(gathered[0], g) for g in gathered),
                        "moved": not torch.equal(f["p"], p0), "finite": bool(torch.isfinite(f["p"]).all())}, out_path)
    finally:
        dist.destroy_process_group()


def test_two_allreduce_ranks_stay_in_sync(hip):
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
    assert r["sync"] == [True, True] and r["identical"] and r["moved"] and r["finite"]
