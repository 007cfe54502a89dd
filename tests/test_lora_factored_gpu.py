"""LoRA with the factored backward (LoRA(backward="factored")) on MicroDiT_Tiny: the engine's backward(param_grads="lora"),
LoRAAdamW's step without projection, the Trainer's data-parallel path, train.py.  The recipe of tests/test_lora_gpu.py: MD_DETERMINISTIC,
recorded noise, the zero-initialised tensors perturbed, B randomised with std 0.05 so that dA != 0.

Bounds, per element, against the fp64 chain (lora.ref_wgrad_factored) on the operands every targeted lin_wgrad call was given
(u = 2^-9, U = 2^-24, c = scale; summed over the microbatches):
    factored   |dB^ - dB|[n, j] <= c (2 u + (M + K + 8) U) sum_m |dy[m, n]| sum_k |x[m, k]| |A[j, k]|
               |dA^ - dA|[j, k] <= c (2 u + (M + N + 8) U) sum_m (sum_n |dy[m, n]| |B[n, j]|) |x[m, k]|
    projected  (cols + 4) U c sum |G| |A| for dB, (rows + 4) U c sum |B| |G| for dA, G the fp32 gradient the engine accumulated
               (tests/test_lora_kernels_gpu.py)."""
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from micro_diffusion_amd import lora

pytestmark = pytest.mark.gpu

u, U = 2.0 ** -9, 2.0 ** -24
LR = 1e-3
DENSE = [r"^blocks\.0\.mlp\.w[12]\.weight$", r"^patch_mixer\.0\.mlp\.w[12]\.weight$"]


@pytest.fixture(autouse=True)
def _deterministic(monkeypatch):
    monkeypatch.setenv("MD_DETERMINISTIC", "1")


@pytest.fixture(scope="module")
def base():
    from oracle import microdit_ref as orc
    cfg = orc.tiny_config()
    return cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 83))


def _product(base, train=True):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    cfg, sd = base
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd)
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), train_mask_ratio=0.75,
                        latent_res=cfg.input_size)
    m.train(train)
    return m


def _batch(base, B, seed, mb, lo=0, hi=None):
    from oracle import microdit_ref as orc
    batch, rnd, epsn, mnoise = orc.synth_batch(base[0], B, seed)
    hi = B if hi is None else hi
    chunks = [(rnd[i:i + mb].cuda(), epsn[i:i + mb].cuda(), mnoise[i:i + mb].cuda()) for i in range(lo, hi, mb)]
    return {k: t[lo:hi].cuda() for k, t in batch.items()}, chunks


def _step(model, tr, base, seed, B=4, lo=0, hi=None):
    batch, chunks = _batch(base, B, seed, tr.microbatch_size, lo, hi)
    model._noise_fn = lambda b, c=chunks: c.pop(0)
    loss = tr.train_step(batch)
    torch.cuda.synchronize()
    return loss.clone()


def _randomise_b(ad, seed, std=0.05):
    g = torch.Generator().manual_seed(seed)
    for n in ad.names:
        ad.B(n).copy_(torch.randn(ad.B(n).shape, generator=g) * std)
    if ad.attached:
        ad.dit.refresh_shadow(force=True)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _setup(base, *, backward="factored", rank=8, alpha=4, seed=5, targets=lora.DEFAULT_TARGETS, mb=2, clip=0.0, bseed=6, **optkw):
    from micro_diffusion_amd.trainer import Trainer
    model = _product(base)
    ad = lora.LoRA(model.dit, rank=rank, alpha=alpha, seed=seed, targets=targets, backward=backward)
    opt = lora.LoRAAdamW(ad, lr=LR, **optkw)
    tr = Trainer(model, opt, None, clip_norm=clip, microbatch_size=mb)
    if bseed is not None:
        _randomise_b(ad, bseed)
    return model, ad, opt, tr


def _logical(t, ld, off, M, C):
    """The [M, C] operand a lin_wgrad call addresses inside tensor t (row pitch ld, column offset off), as a CPU copy."""
    flat = t.reshape(-1)              # (as_strided counts its offset from the start of the storage, and t may be a piece of an arena)
    return torch.as_strided(flat, (M, C), (ld, 1), flat.storage_offset() + off).cpu().clone()


def _spy_wgrad(model, ad, calls, nan_when=None):
    """Record the operands of every lin_wgrad call on a target of the adapter; nan_when(): set one element of the first target's dy to NaN."""
    eng = model.dit.engine
    inner = eng.lin_wgrad

    def lin_wgrad(dy, x, wname, M, N, K, *, lddy=None, ldx=None, dyoff=0, xoff=0, **kw):
        name = wname + ".weight"
        if ad.is_target(name) and eng._lora_grads:
            if nan_when is not None and nan_when() and name == ad.names[0]:
                dy.reshape(-1)[dyoff + 5] = float("nan")
            calls.append(dict(name=name, M=M, N=N, K=K, dy=_logical(dy, lddy or N, dyoff, M, N), x=_logical(x, ldx or K, xoff, M, K)))
        return inner(dy, x, wname, M, N, K, lddy=lddy, ldx=ldx, dyoff=dyoff, xoff=xoff, **kw)
    eng.lin_wgrad = lin_wgrad


def _spy_step(ad, opt, rec):
    """Keep adapter.g as the optimiser pass finds it."""
    inner = opt.step

    def step(*a, **kw):
        rec["g"] = ad.g.clone()
        return inner(*a, **kw)
    opt.step = step


def _chain(ad, calls, w):
    """{name: (dA, dB, bound dA, bound dB)} in fp64 from the recorded operands (summed over the calls) and the adapter values w."""
    out = {}
    r, c = ad.rank, ad.scale
    for cl in calls:
        n, k = ad._shape_of[cl["name"]]
        a, b = ad.offs[cl["name"]]
        A, B = w[a:a + r * k].view(r, k), w[b:b + n * r].view(n, r)
        dA, dB = lora.ref_wgrad_factored(cl["dy"], cl["x"], A, B, c)
        xa, dya, M = cl["x"].double().abs(), cl["dy"].double().abs(), cl["M"]
        bB = c * (2 * u + (M + k + 8) * U) * (dya.t() @ (xa @ A.double().abs().t()))
        bA = c * (2 * u + (M + n + 8) * U) * ((dya @ B.double().abs()).t() @ xa)
        if cl["name"] in out:
            o = out[cl["name"]]
            out[cl["name"]] = (o[0] + dA, o[1] + dB, o[2] + bA, o[3] + bB)
        else:
            out[cl["name"]] = (dA, dB, bA, bB)
    return out


def _worst(err, bound):
    """max err / bound over the elements, inf if any element is past its bound (a zero bound -- an all-zero row of dy -- allows no error)."""
    if not bool((err <= bound).all()):
        return float("inf")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def _views(ad, g, name):
    n, k = ad._shape_of[name]
    a, b = ad.offs[name]
    return g[a:a + ad.rank * k].view(ad.rank, k).double(), g[b:b + n * ad.rank].view(n, ad.rank).double()


@pytest.mark.parametrize("targets", [lora.DEFAULT_TARGETS, tuple(lora.DEFAULT_TARGETS) + tuple(DENSE)], ids=["default", "with-dense-swiglu"])
def test_adapter_gradient_of_two_microbatches(hip, base, targets):
    model, ad, opt, tr = _setup(base, targets=targets)
    eng = model.dit.engine
    eng.keep_last_tape = True
    calls, rec = [], {}
    _spy_wgrad(model, ad, calls)
    _spy_step(ad, opt, rec)
    w0 = ad.w.clone().cpu()
    _step(model, tr, base, 910)
    tp = eng.last_tape
    # every target once per microbatch, with the row count of its stream
    assert sorted(c["name"] for c in calls) == sorted(list(ad.names) * 2)
    for c in calls:
        want = 2 * 77 if "kv_linear" in c["name"] else 2 * (tp.T if c["name"].startswith("patch_mixer") else tp.Tk)
        assert c["M"] == want and (c["N"], c["K"]) == ad._shape_of[c["name"]], (c["name"], c["M"], want)
    if len(targets) > len(lora.DEFAULT_TARGETS):
        assert any(c["name"].endswith("mlp.w2.weight") for c in calls), "the lddy = 2 f / dyoff = f call"
    g = rec["g"].cpu()
    assert bool(torch.isfinite(g).all())
    worst = 0.0
    for name, (dA, dB, bA, bB) in _chain(ad, calls, w0).items():
        gA, gB = _views(ad, g, name)
        wA, wB = _worst((gA - dA).abs(), bA), _worst((gB - dB).abs(), bB)
        worst = max(worst, wA, wB)
        assert wA <= 1.0 and wB <= 1.0 and bool(dA.any()) and bool(dB.any()), (name, wA, wB)
    print(f"{len(ad.names)} targets: max |adapter.g - fp64 chain| / bound = {worst:.4f}")
    assert not ad.g.any(), "the optimiser pass clears adapter.g"


def test_the_full_gradient_is_never_formed(hip, base):
    model, ad, opt, tr = _setup(base)
    f = model.dit.flat_buffers()
    sentinel = (torch.arange(f["total"], device="cuda", dtype=torch.float32) % 251) - 125.0
    f["g"].copy_(sentinel)
    grads0 = {n: (None if p.grad is None else p.grad.clone()) for n, p in model.dit.named_parameters()}
    p0, s0, w0 = f["p"].clone(), f["s"].clone(), ad.w.clone()
    _step(model, tr, base, 910)
    assert torch.equal(_bits(f["g"]), _bits(sentinel)), "flat g was written"
    for n, p in model.dit.named_parameters():
        assert (p.grad is None) == (grads0[n] is None) and (p.grad is None or torch.equal(_bits(p.grad), _bits(grads0[n]))), n
    assert torch.equal(_bits(f["p"]), _bits(p0)), "the masters moved"
    assert not torch.equal(ad.w, w0), "the adapter did not move"
    keep = torch.ones(f["total"], dtype=torch.bool, device="cuda")
    for s in ad.specs:
        o = ad.flat_offs[s.name]
        keep[o:o + s.shape[0] * s.shape[1]] = False
    assert torch.equal(_bits(f["s"])[keep], _bits(s0)[keep]), "the shadow of a non-target tensor changed"
    assert not torch.equal(_bits(f["s"])[~keep], _bits(s0)[~keep]), "the shadow of the targets is the merge of the updated adapter"
    # the engine refuses the mode without a factored adapter
    ad.detach()
    with pytest.raises(RuntimeError, match="factored"):
        model.dit.engine.backward(None, None, param_grads="lora")
    with pytest.raises(ValueError, match="param_grads"):
        model.dit.engine.backward(None, None, param_grads="adapter")


def test_factored_and_projected_agree(hip, base):
    out = {}
    for mode in ("factored", "projected"):
        model, ad, opt, tr = _setup(base, backward=mode)
        calls, rec = [], {}
        if mode == "factored":
            _spy_wgrad(model, ad, calls)
            _spy_step(ad, opt, rec)
        else:
            inner = ad.project_grad

            def project(grad_scale=1.0, ad=ad, inner=inner, rec=rec):
                rec["G"] = ad.dit.flat_buffers()["g"].clone()
                inner(grad_scale)
                rec["g"] = ad.g.clone()
            ad.project_grad = project
        w0 = ad.w.clone().cpu()
        loss = _step(model, tr, base, 910, B=2)                   # one microbatch
        out[mode] = dict(ad=ad, calls=calls, g=rec["g"].cpu(), G=rec.get("G"), w0=w0, loss=loss)
    fa, pr = out["factored"], out["projected"]
    assert torch.equal(_bits(fa["loss"]), _bits(pr["loss"])), "the forward is the same"
    assert torch.equal(fa["w0"], pr["w0"])
    ad, G = fa["ad"], pr["G"].cpu()
    worst = 0.0
    for name, (dA, dB, bA, bB) in _chain(ad, fa["calls"], fa["w0"]).items():
        n, k = ad._shape_of[name]
        o, (a, b) = ad.flat_offs[name], ad.offs[name]
        Gw = G[o:o + n * k].view(n, k).double().abs()
        A, B = fa["w0"][a:a + ad.rank * k].view(ad.rank, k).double().abs(), fa["w0"][b:b + n * ad.rank].view(n, ad.rank).double().abs()
        pA = (n + 4) * U * ad.scale * (B.t() @ Gw)
        pB = (k + 4) * U * ad.scale * (Gw @ A.t())
        fA, fB = _views(ad, fa["g"], name)
        qA, qB = _views(ad, pr["g"], name)
        wA, wB = _worst((fA - qA).abs(), bA + pA), _worst((fB - qB).abs(), bB + pB)
        worst = max(worst, wA, wB)
        assert wA <= 1.0 and wB <= 1.0 and bool(qA.any()) and bool(qB.any()), (name, wA, wB)
    print(f"max |factored - projected| / (sum of the two bounds) = {worst:.4f}")


def test_determinism_and_poison(hip, base):
    runs = []
    for poison in (False, False, True):
        model, ad, opt, tr = _setup(base, clip=0.25)
        model.dit.engine.poison = poison
        rec = {}
        _spy_step(ad, opt, rec)
        _step(model, tr, base, 910)
        runs.append((rec["g"].clone(), ad.w.clone()))
    assert bool(runs[0][0].any()) and bool(torch.isfinite(runs[0][0]).all())
    assert torch.equal(_bits(runs[0][1]), _bits(runs[1][1])), "two identical steps, different adapter weights"
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0]))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[2][0])), "poisoned allocations changed the adapter's gradient"


def test_twenty_steps_fit_guard_and_frozen_base(hip, base):
    model, ad, opt, tr = _setup(base, rank=16, alpha=None, seed=7, clip=0.25, bseed=None, skip_nonfinite=True)
    f = model.dit.flat_buffers()
    p0 = f["p"].clone()
    rec, calls, poison = {}, [], {"on": False}
    _spy_wgrad(model, ad, calls, nan_when=lambda: poison["on"])
    _spy_step(ad, opt, rec)
    losses = []
    for _ in range(21):                                               # one fixed batch, fixed draws: loss i is taken BEFORE update i
        losses.append(float(_step(model, tr, base, 920)))
        calls.clear()
    print(f"loss before the first update {losses[0]:.6f}, after 20 updates {losses[20]:.6f}")
    assert losses[20] < losses[0]
    assert opt.skipped_steps() == 0 and torch.equal(_bits(f["p"]), _bits(p0)), "the base moved"
    assert bool(torch.isfinite(opt.grad_norm())) and float(opt.grad_norm()) > 0
    keep = (ad.w.clone(), opt.m.clone(), opt.v.clone())
    poison["on"] = True
    _step(model, tr, base, 920)
    poison["on"] = False
    assert not bool(torch.isfinite(rec["g"]).all()), "the NaN must reach the adapter's gradient"
    assert opt.skipped_steps() == 1 and opt.step_count == 22
    for nm, a, b in zip("wmv", (ad.w, opt.m, opt.v), keep):
        assert torch.equal(_bits(a), _bits(b)), f"{nm} moved on a skipped step"
    assert not f["g"].any() and not ad.g.any(), "adapter.g is cleared on a skipped step too (flat g was never written)"
    assert torch.equal(_bits(f["p"]), _bits(p0))
    _step(model, tr, base, 920)
    assert opt.skipped_steps() == 1 and not torch.equal(ad.w, keep[0]) and bool(torch.isfinite(ad.w).all())


def test_checkpoint_interchange(hip, base):
    model, ad, opt, tr = _setup(base)
    _step(model, tr, base, 910)
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ad.state_dict().items()}
    assert "backward" not in sd
    other = _product(base, False)
    ad2 = lora.LoRA.from_state_dict(other.dit, sd, backward="projected").attach()
    assert ad2.backward == "projected" and ad.backward == "factored" and torch.equal(ad2.w, ad.w)
    assert lora.LoRA.from_state_dict(other.dit, sd, device="cpu").backward == "projected"
    g = torch.Generator().manual_seed(17)
    cfg = base[0]
    lat = torch.randn(2, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g).cuda()
    y = torch.randn(2, 1, 77, cfg.caption_channels, generator=g).cuda()
    model.eval()
    a = model.edm_sampler_loop(lat, y, steps=4, cfg=3.0)
    b = other.edm_sampler_loop(lat, y, steps=4, cfg=3.0)
    assert torch.equal(a, b)
    attached = model.dit.flat_buffers()["s"].clone()
    ad.fuse()
    assert torch.equal(_bits(model.dit.flat_buffers()["s"]), _bits(attached)), "fuse() keeps the bf16 bits the adapter ran on"
    ad2.fuse()
    assert torch.equal(_bits(other.dit.flat_buffers()["s"]), _bits(attached))


# ---------------------------------------------------------------------------------------------------- data parallelism
DP_BATCH, DP_SEED = 4, 940


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_base():
    from oracle import microdit_ref as orc
    cfg = orc.tiny_config()
    return cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 83))


def _dp_rank_main(rank, world, port, out_path):
    from micro_diffusion_amd.trainer import Trainer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), MD_DETERMINISTIC="1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        base = _dp_base()
        per = DP_BATCH // world
        model = _product(base)
        # the projected backward has nothing it could exchange; the factored one has nothing to shard
        proj = lora.LoRA(model.dit, rank=8, alpha=4, seed=5)
        refused = 0
        try:
            Trainer(model, lora.LoRAAdamW(proj, lr=LR), None, microbatch_size=per)
        except NotImplementedError:
            refused += 1
        proj.detach()
        ad = lora.LoRA(model.dit, rank=8, alpha=4, seed=5, backward="factored")
        opt = lora.LoRAAdamW(ad, lr=LR)
        try:
            Trainer(model, opt, None, microbatch_size=per, dp_mode="sharded")
        except NotImplementedError:
            refused += 1
        tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=per)
        _randomise_b(ad, 6)
        f = model.dit.flat_buffers()
        p0 = f["p"].clone()
        assert tr.world == world and tr.sync.gbf is None and not tr.sharded and tr.sync.mode == "allreduce"
        _step(model, tr, base, DP_SEED, B=DP_BATCH, lo=rank * per, hi=(rank + 1) * per)
        same = True
        for t in (ad.w, opt.m, opt.v):
            mine = t.cpu()
            got = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(got, mine)
            same = same and all(torch.equal(_bits(got[0]), _bits(x)) for x in got)
        in_sync = tr.replicas_in_sync()
        if rank == 0:
            torch.save({"w": ad.w.cpu(), "gnorm": float(opt.grad_norm()), "same": same, "in_sync": in_sync, "refused": refused,
                        "base_untouched": torch.equal(_bits(f["p"]), _bits(p0)), "g_untouched": not bool(f["g"].any()),
                        "gbf": tr.sync.gbf is None, "slots": tr.sync.finish()}, out_path)
    finally:
        dist.destroy_process_group()


def test_two_ranks_match_one_rank(hip, base):
    model, ad, opt, tr = _setup(base, mb=DP_BATCH // 2, clip=0.25)
    w0 = ad.w.clone()
    _step(model, tr, base, DP_SEED, B=DP_BATCH)
    g1, w1 = float(opt.grad_norm()), ad.w.cpu()
    del model, ad, opt, tr
    torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rank0.pt")
        ctx = mp.get_context("spawn")
        port = _free_port()
        procs = [ctx.Process(target=_dp_rank_main, args=(r, 2, port, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
        codes = [p.exitcode for p in procs]
        assert codes == [0, 0], f"rank processes failed: {codes}"
        r = torch.load(out)
    assert r["same"] and r["in_sync"], "replicas diverged within one step"
    assert r["refused"] == 2, "projected LoRA with two ranks and dp_mode='sharded' must raise NotImplementedError"
    assert r["base_untouched"] and r["g_untouched"] and r["gbf"] and r["slots"] == 0
    print(f"adapter gradient norm: one rank {g1:.8f}, two ranks {r['gnorm']:.8f}")
    assert g1 > 0 and abs(r["gnorm"] - g1) <= 1e-4 * g1, (r["gnorm"], g1)
    # the first AdamW update moves every element by about lr: the same update up to the sign of elements with |g| near 0
    moved = (r["w"] - w1).abs()
    assert float((moved > 1e-5).float().mean()) <= 1e-2 and not torch.equal(r["w"], w0.cpu())


# ---------------------------------------------------------------------------------------------------- train.py end to end
def test_train_py_factored_checkpoints_and_autoresume(hip, tmp_path, capsys, monkeypatch):
    import json
    import math
    import train as train_mod
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    target = "micro_diffusion.datasets.latents_loader.build_streaming_latents_dataloader"
    folder, base_path = os.path.join(tmp_path, "run"), os.path.join(tmp_path, "base.pt")
    gen = torch.Generator().manual_seed(3)
    base_sd = {"dit.final_layer.linear.weight": torch.randn(16, 512, generator=gen) * 0.02}
    for blk in [f"patch_mixer.{i}" for i in range(4)] + [f"blocks.{i}" for i in range(16)]:
        base_sd[f"dit.{blk}.adaLN_modulation.1.bias"] = torch.randn(6 * 512, generator=gen) * 0.1
    torch.save({"state": {"model": base_sd}}, base_path)

    def cfg(max_ba, misc=None, **trainer):
        return {
            "seed": 18,
            "model": {"_target_": "micro_diffusion.models.model.create_latent_diffusion", "dit_arch": "MicroDiT_Tiny_2", "latent_res": 32,
                      "in_channels": 4, "pos_interp_scale": 1.0, "dtype": "bfloat16", "precomputed_latents": True, "p_mean": -0.6,
                      "p_std": 1.2, "train_mask_ratio": 0.75, "vae_name": "x", "text_encoder_name": "openclip:hf-hub:apple/DFN5B-CLIP-ViT-H-14-378"},
            "optimizer": {"_target_": "torch.optim.AdamW", "lr": 1e-3, "weight_decay": 0.1, "eps": 1e-8, "betas": [0.9, 0.999]},
            "scheduler": {"_target_": "composer.optim.ConstantScheduler", "alpha": 1.0},
            "algorithms": {"gradient_clipping": {"clip_norm": 0.25, "clipping_type": "norm"}},
            "dataset": {"image_size": 256, "train_batch_size": 8, "eval_batch_size": 8, "cap_drop_prob": 0.1,
                        "train": {"_target_": target, "datadir": "synthetic"}},
            "trainer": dict({"max_duration": f"{max_ba}ba", "device_train_microbatch_size": 4, "save_interval": "1ba", "save_folder": folder,
                             "load_path": base_path, "load_strict_model_weights": False}, **trainer),
            "misc": dict({"log_interval": 1, "lora_rank": 4, "lora_alpha": 8, "skip_nonfinite_steps": True, "lora_backward": "factored"},
                         **(misc or {})),
        }
    with pytest.raises(ValueError, match="lora_backward"):
        train_mod.train(cfg(1, misc={"lora_backward": "fused"}))
    capsys.readouterr()
    tr = train_mod.train(cfg(2))
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    logged = [l for l in lines if "loss" in l]
    assert [l["batch"] for l in logged] == [1, 2] and all(math.isfinite(l["loss"]) and l["skipped_steps"] == 0 for l in logged)
    opt, dit = tr.opt, tr.model.dit
    ad = opt.adapter
    assert ad.backward == "factored" and tr.lora_factored and dit._lora is ad and opt.step_count == 2
    assert any(bool(ad.B(n).any()) for n in ad.names) and not bool(dit.flat_buffers()["g"].any())
    for k, v in base_sd.items():
        assert torch.equal(dit.state_dict()[k[len("dit."):]].cpu(), v), f"{k}: the base is what trainer.load_path holds, and frozen"
    assert sorted(os.listdir(folder)) == ["latest.pt", "lora-1.pt", "lora-2.pt"]
    ck = torch.load(os.path.join(folder, "latest.pt"), map_location="cpu")
    assert ck["batch"] == 2 and ck["optimizer"]["step"] == 2 and "backward" not in ck["lora"]
    assert torch.equal(ck["lora"]["blocks.0.attn.qkv.lora_B.weight"], ad.B("blocks.0.attn.qkv.weight").cpu())
    tr2 = train_mod.train(cfg(3, autoresume=True))
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert any(l.get("resumed_from") for l in out) and [l["batch"] for l in out if "loss" in l] == [3]
    ad2 = tr2.opt.adapter
    assert ad2.backward == "factored" and tr2.opt.step_count == 3 and tr2.batches_seen == 3 and bool(tr2.opt.m.any())
    saved_b = ck["lora"]["blocks.0.attn.qkv.lora_B.weight"]
    moved = (ad2.B("blocks.0.attn.qkv.weight").cpu() - saved_b).abs().max()
    assert 0 < float(moved) <= 1.5e-3 * 3
    assert sorted(os.listdir(folder)) == ["latest.pt", "lora-1.pt", "lora-2.pt", "lora-3.pt"]
