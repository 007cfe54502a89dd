"""LoRA on MicroDiT_Tiny: attach / detach / scale / fuse against the plain model bit for bit, one Trainer step with
LoRAAdamW against the fp64 restatements, a short fit, the step guard, save / resume.  The zero-initialised tensors of the model are
perturbed (oracle.dezero_state_dict), or the network would contribute almost nothing.

Bounds (U = 2^-24): the adapter gradients as in tests/test_lora_kernels_gpu.py ((cols + 4) U c sum |G| |A| for dB, (rows + 4) U c
sum |B| |G| for dA, c = scale * grad_scale).  The AdamW step is compared with loss_weighting.ref_adamw(as_kernel=True) on the measured
gradients, with the tolerance tests/test_loss_weighting_gpu.py uses for md_adamw_step -- 16 U lr for the update's own fp32 arithmetic
-- plus U |w|: there w starts at zero, here A holds values near 1 / sqrt(K), so the fp32 rounding of the stored weight itself is the
larger term.  The moments after the first step are (1 - beta) g and (1 - beta2) g^2, two fp32 products each: 4 U |ref|."""
import pytest
import torch

from micro_diffusion_amd import lora
from micro_diffusion_amd import loss_weighting as lwm

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LR = 1e-3


@pytest.fixture(autouse=True)
def _deterministic(monkeypatch):
    monkeypatch.setenv("MD_DETERMINISTIC", "1")       # bit-reproducible backward: save / resume and the two-run comparisons need it


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


def _batch(base, B, seed, mb):
    from oracle import microdit_ref as orc
    batch, rnd, epsn, mnoise = orc.synth_batch(base[0], B, seed)
    chunks = [(rnd[i:i + mb].cuda(), epsn[i:i + mb].cuda(), mnoise[i:i + mb].cuda()) for i in range(0, B, mb)]
    return {k: t.cuda() for k, t in batch.items()}, chunks


def _microbatch_loss(model, base, seed=900):
    batch, chunks = _batch(base, 2, seed, 2)
    model._noise_fn = lambda b, c=chunks: c.pop(0)
    loss = model.train_microbatch(batch)
    torch.cuda.synchronize()
    return loss.clone()


def _step(model, tr, base, seed, B=4):
    batch, chunks = _batch(base, B, seed, tr.microbatch_size)
    model._noise_fn = lambda b, c=chunks: c.pop(0)
    loss = tr.train_step(batch)
    torch.cuda.synchronize()
    return float(loss)


def _sampler_inputs(base, seed=17):
    cfg = base[0]
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(2, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g).cuda()
    y = torch.randn(2, 1, 77, cfg.caption_channels, generator=g).cuda()
    return lat, y


def _randomise_b(ad, seed, std=0.05):
    g = torch.Generator().manual_seed(seed)
    for n in ad.names:
        ad.B(n).copy_(torch.randn(ad.B(n).shape, generator=g) * std)
    if ad.attached:
        ad.dit.refresh_shadow(force=True)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _forward(model, base, seed=31):
    lat, y = _sampler_inputs(base, seed)
    with torch.no_grad():
        out = model.dit.forward_without_cfg(lat, torch.tensor([0.3, -0.7], device="cuda"), y)["sample"]
    torch.cuda.synchronize()
    return out.clone()


def test_fresh_adapter_and_detach_leave_the_model_alone(hip, base):
    model = _product(base)
    f = model.dit.flat_buffers()
    lat, y = _sampler_inputs(base)
    loss0 = _microbatch_loss(model, base)
    model.eval()
    sample0 = model.edm_sampler_loop(lat, y, steps=4, cfg=3.0)
    model.train()
    shadow0, version0 = f["s"].clone(), model.dit.engine.weights_version
    ad = lora.LoRA(model.dit, rank=8, seed=1).attach()
    assert model.dit._lora is ad and ad.active and model.dit.engine.weights_version != version0
    assert not any(bool(ad.B(n).any()) for n in ad.names) and all(bool(ad.A(n).any()) for n in ad.names)
    assert torch.equal(_bits(f["s"]), _bits(shadow0)), "B = 0: the merge must leave bf16(p)"
    assert torch.equal(_microbatch_loss(model, base), loss0)
    model.eval()
    assert torch.equal(model.edm_sampler_loop(lat, y, steps=4, cfg=3.0), sample0)
    _randomise_b(ad, 2)
    assert not torch.equal(_bits(f["s"]), _bits(shadow0)), "a non-zero B must reach the shadow"
    version1 = model.dit.engine.weights_version
    ad.detach()
    assert model.dit._lora is None and not ad.active and model.dit.engine.weights_version != version1
    assert torch.equal(_bits(f["s"]), _bits(shadow0)), "detach() restores the plain shadow"
    with pytest.raises(RuntimeError, match="GPU"):
        lora.LoRA(model.dit, rank=8, device="cpu").attach()


def test_attached_equals_fused_and_scale(hip, base):
    plain, att, fus = _product(base, False), _product(base, False), _product(base, False)
    ad = lora.LoRA(att.dit, rank=16, alpha=8, seed=3).attach()
    _randomise_b(ad, 4)
    ad2 = lora.LoRA.from_state_dict(fus.dit, ad.state_dict()).attach()
    assert ad2.scale == 0.5 and torch.equal(ad2.w, ad.w)
    p_before = fus.dit.flat_buffers()["p"].clone()
    ad2.fuse()
    assert fus.dit._lora is None and not ad2.attached
    assert not torch.equal(fus.dit.flat_buffers()["p"], p_before), "fuse() writes the masters"
    assert set(fus.dit.state_dict()) == set(plain.dit.state_dict()), "a fused model saves a plain checkpoint"
    assert torch.equal(_bits(att.dit.flat_buffers()["s"]), _bits(fus.dit.flat_buffers()["s"])), "attached and fused run on the same bf16 bits"
    out_plain, out_att, out_fus = _forward(plain, base), _forward(att, base), _forward(fus, base)
    assert torch.equal(out_att, out_fus) and not torch.equal(out_att, out_plain)
    lat, y = _sampler_inputs(base)
    for cache in (False, True):
        a = att.edm_sampler_loop(lat, y, steps=4, cfg=3.0, sampler="heun", cond_cache=cache)
        b = fus.edm_sampler_loop(lat, y, steps=4, cfg=3.0, sampler="heun", cond_cache=cache)
        assert torch.equal(a, b), f"cond_cache={cache}"
    # a fused model loads like any other checkpoint
    again = _product((base[0], {k: v.cpu() for k, v in fus.dit.state_dict().items()}), False)
    assert torch.equal(_forward(again, base), out_fus)
    # scale: 0 is the base bit for bit, and any change invalidates a Conditioning encoded before it
    cond = att.dit.encode_condition(y)
    x, t = lat, torch.tensor([0.1], device="cuda")
    att.dit.engine.forward(x, t, None, cond=cond)
    ad.scale = 0.0
    assert not ad.active and torch.equal(_forward(att, base), out_plain)
    with pytest.raises(RuntimeError, match="weight version"):
        att.dit.engine.forward(x, t, None, cond=cond)
    ad.scale = 0.5
    assert torch.equal(_forward(att, base), out_att)
    ad.enabled = False
    assert torch.equal(_forward(att, base), out_plain)
    ad.enabled = True
    cond = att.dit.encode_condition(y)
    ad.scale = 0.6
    with pytest.raises(RuntimeError, match="weight version"):
        att.dit.engine.forward(x, t, None, cond=cond)
    assert not torch.equal(_forward(att, base), out_att)


def _spy(ad, record, poison=None):
    """Keep a copy of flat g as md_lora_grad sees it and of the adapter gradient it leaves; `poison`: an element of flat g to set to NaN."""
    inner = ad.project_grad

    def project(grad_scale=1.0):
        f = ad.dit.flat_buffers()
        if poison is not None and poison():
            f["g"][ad.flat_offs[ad.names[0]] + 5] = float("nan")
        record["G"] = f["g"].clone()
        record["d_before"] = ad.g.clone()
        inner(grad_scale)
        record["d"] = ad.g.clone()
        record["grad_scale"] = grad_scale
    ad.project_grad = project


def test_one_trainer_step(hip, base):
    from micro_diffusion_amd.trainer import FusedAdamW, Trainer
    model = _product(base)
    f = model.dit.flat_buffers()
    ad = lora.LoRA(model.dit, rank=8, alpha=4, seed=5)
    opt = lora.LoRAAdamW(ad, lr=LR)
    tr = Trainer(model, opt, None, clip_norm=0.0, microbatch_size=2)
    assert ad.attached and model.dit._lora is ad
    _randomise_b(ad, 6)
    rec = {}
    _spy(ad, rec)
    p0, w0 = f["p"].clone(), ad.w.clone()
    _step(model, tr, base, 910)
    # nothing of the base's size is held by the optimiser
    held = [v for obj in (ad, opt) for v in vars(obj).values() if torch.is_tensor(v)]
    assert len(held) >= 8 and sum(t.numel() for t in held) < f["total"] // 4, (sum(t.numel() for t in held), f["total"])
    assert lora.allocated_floats(opt) < f["total"] // 4 and opt.ema is None and opt.posthoc == []
    # the projection: measured adapter gradients against ref_grad of the gradient the pass consumed
    assert not rec["d_before"].any() and rec["grad_scale"] == 1.0 and bool(torch.isfinite(rec["G"]).all()) and bool(rec["G"].any())
    G, d, wc = rec["G"].cpu(), rec["d"].cpu(), w0.cpu()
    for s in ad.specs:
        n, k = s.shape
        o, (a, b) = ad.flat_offs[s.name], ad.offs[s.name]
        Gw, A, B = G[o:o + n * k].view(n, k), wc[a:a + 8 * k].view(8, k), wc[b:b + n * 8].view(n, 8)
        rA, rB = lora.ref_grad(Gw, A, B, 0.5, 1.0)
        bA = (n + 4) * U * 0.5 * (B.double().abs().t() @ Gw.double().abs())
        bB = (k + 4) * U * 0.5 * (Gw.double().abs() @ A.double().abs().t())
        wA = float(((d[a:a + 8 * k].view(8, k).double() - rA).abs() / bA).max())
        wB = float(((d[b:b + n * 8].view(n, 8).double() - rB).abs() / bB).max())
        print(f"{s.name}: max |dA - ref| / bound = {wA:.3f}, max |dB - ref| / bound = {wB:.3f}")
        assert wA <= 1.0 and wB <= 1.0 and bool(rA.any()) and bool(rB.any())
    # both accumulators are cleared, the base is untouched, the shadow is the merge of the UPDATED adapter
    assert not f["g"].any() and not ad.g.any()
    assert torch.equal(_bits(f["p"]), _bits(p0))
    assert not torch.equal(ad.w, w0)
    want = torch.empty_like(f["s"])
    hip.check(hip.lib().md_cast_f32_bf16(f["p"].data_ptr(), want.data_ptr(), f["total"], None, hip.stream_ptr()), "md_cast_f32_bf16")
    plain = want.clone()
    ad.merge_into(want, False)
    torch.cuda.synchronize()
    assert torch.equal(_bits(f["s"]), _bits(want)) and not torch.equal(_bits(want), _bits(plain))
    name = ad.names[0]
    o, (n, k) = ad.flat_offs[name], ad._spec(name).shape
    ref = lora.ref_merge(f["P"][name].cpu(), ad.A(name).cpu(), ad.B(name).cpu(), 0.5)
    got = f["s"][o:o + n * k].view(n, k).float().cpu().double()
    assert bool(((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-7).all()), "bf16 rounding of the merged weight"
    # AdamW on the adapter: step 1 from zero moments, no clipping, no decay
    w_ref, m_ref, v_ref = lwm.ref_adamw(w0.cpu(), d, torch.zeros_like(d), torch.zeros_like(d), 1, LR, as_kernel=True)
    for nm, got, ref, tol in (("w", ad.w, w_ref, 16 * U * LR + U * w_ref.abs()), ("m", opt.m, m_ref, 4 * U * m_ref.abs()),
                              ("v", opt.v, v_ref, 4 * U * v_ref.abs())):
        err = (got.cpu().double() - ref).abs()
        print(f"AdamW {nm}: max error / tolerance = {float((err / tol.clamp(min=1e-300)).max()):.3f}")
        assert bool((err <= tol).all()), nm
    assert opt.step_count == 1 and opt.skipped_steps() == 0
    # the optimiser of the full model refuses a DiT that carries an adapter; the adapter's refuses an exchanged gradient
    with pytest.raises(RuntimeError, match="LoRA adapter attached"):
        FusedAdamW(model.dit)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        opt.step(g_bf16=torch.zeros(8, device="cuda", dtype=torch.bfloat16))
    ad.detach()
    full = FusedAdamW(model.dit)
    ad.attach()
    with pytest.raises(RuntimeError, match="LoRA adapter attached"):
        full.step()


def test_twenty_steps_fit_guard_and_frozen_base(hip, base):
    from micro_diffusion_amd.trainer import Trainer
    model = _product(base)
    f = model.dit.flat_buffers()
    ad = lora.LoRA(model.dit, rank=16, seed=7)
    opt = lora.LoRAAdamW(ad, lr=LR, skip_nonfinite=True)
    tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2)
    p0 = f["p"].clone()
    rec, poison = {}, {"on": False}
    _spy(ad, rec, poison=lambda: poison["on"])
    losses = [_step(model, tr, base, 920) for _ in range(21)]        # one fixed batch, fixed draws: loss i is taken BEFORE update i
    print(f"loss before the first update {losses[0]:.6f}, after 20 updates {losses[20]:.6f}")
    assert losses[20] < losses[0]
    assert opt.skipped_steps() == 0 and torch.equal(_bits(f["p"]), _bits(p0)), "the base moved"
    assert bool(torch.isfinite(opt.grad_norm())) and float(opt.grad_norm()) > 0
    # the guard: one NaN in the gradient of a targeted matrix -> the adapter and its moments stay as they are, the step is counted
    keep = (ad.w.clone(), opt.m.clone(), opt.v.clone())
    poison["on"] = True
    _step(model, tr, base, 920)
    poison["on"] = False
    assert not bool(torch.isfinite(rec["d"]).all()), "the NaN must reach the adapter's gradient"
    assert opt.skipped_steps() == 1 and opt.step_count == 22
    for nm, a, b in zip("wmv", (ad.w, opt.m, opt.v), keep):
        assert torch.equal(_bits(a), _bits(b)), f"{nm} moved on a skipped step"
    assert not f["g"].any() and not ad.g.any(), "both accumulators are cleared on a skipped step too"
    assert torch.equal(_bits(f["p"]), _bits(p0))
    _step(model, tr, base, 920)
    assert opt.skipped_steps() == 1 and not torch.equal(ad.w, keep[0]) and bool(torch.isfinite(ad.w).all())


def test_save_load_then_one_more_step(hip, base):
    from micro_diffusion_amd.trainer import Trainer

    def run(steps, resume=None):
        model = _product(base)
        if resume is None:
            ad = lora.LoRA(model.dit, rank=4, seed=9)
        else:
            ad = lora.LoRA.from_state_dict(model.dit, resume["lora"])
        opt = lora.LoRAAdamW(ad, lr=LR, weight_decay=0.01)
        if resume is not None:
            opt.load_state_dict(resume["optimizer"])
        tr = Trainer(model, opt, None, clip_norm=0.25, microbatch_size=2)
        ck = None
        for _ in range(steps):
            _step(model, tr, base, 930 + opt.step_count)
            if opt.step_count == 2:
                ck = {"lora": {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ad.state_dict().items()},
                      "optimizer": {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}}
        return ad, opt, ck, model

    ad1, opt1, ck, m1 = run(3)
    ad2, opt2, _, m2 = run(1, resume=ck)
    assert opt2.step_count == 3
    for nm, a, b in (("w", ad1.w, ad2.w), ("m", opt1.m, opt2.m), ("v", opt1.v, opt2.v)):
        assert torch.equal(_bits(a), _bits(b)), f"{nm} differs after save at step 2 + resume"
    assert torch.equal(_bits(m1.dit.flat_buffers()["s"]), _bits(m2.dit.flat_buffers()["s"]))
    assert bool(opt1.m.any()) and any(bool(ad1.B(n).any()) for n in ad1.names)


# ---------------------------------------------------------------------------------------------------- train.py end to end
def test_train_py_adapter_checkpoints_and_autoresume(hip, tmp_path, capsys, monkeypatch):
    """train.py with misc.lora_rank on synthetic data: the base comes from trainer.load_path and stays as loaded, the checkpoints are
    adapters (lora-<batch>.pt, latest.pt) with their optimiser state, autoresume continues from them, and what cannot be honoured is
    refused before anything is built."""
    import json
    import math
    import os
    import train as train_mod
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    target = "micro_diffusion.datasets.latents_loader.build_streaming_latents_dataloader"
    folder, base_path = os.path.join(tmp_path, "run"), os.path.join(tmp_path, "base.pt")
    # a partial base (strict off) that un-zeroes what the reference zero-initialises on the way of the gradient: with the
    # final projection and every block's gates at zero no gradient reaches the attention projections and B would stay zero
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
            "misc": dict({"log_interval": 1, "lora_rank": 4, "lora_alpha": 8, "skip_nonfinite_steps": True}, **(misc or {})),
        }
    with pytest.raises(ValueError, match="load_path"):
        train_mod.train(cfg(1, load_path=None))
    bad = cfg(1)
    bad["algorithms"]["ema"] = {"smoothing": 0.999}
    with pytest.raises(ValueError, match="algorithms.ema"):
        train_mod.train(bad)
    capsys.readouterr()
    tr = train_mod.train(cfg(2))
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    logged = [l for l in lines if "loss" in l]
    assert [l["batch"] for l in logged] == [1, 2] and all(math.isfinite(l["loss"]) and l["skipped_steps"] == 0 for l in logged)
    opt, dit = tr.opt, tr.model.dit
    ad = opt.adapter
    assert isinstance(opt, lora.LoRAAdamW) and dit._lora is ad and ad.rank == 4 and ad.scale == 2.0 and opt.weight_decay == 0.0
    assert opt.step_count == 2 and len(ad.specs) == 5 * (16 + 4) and any(bool(ad.B(n).any()) for n in ad.names)
    for k, v in base_sd.items():
        assert torch.equal(dit.state_dict()[k[len("dit."):]].cpu(), v), f"{k}: the base is what trainer.load_path holds, and frozen"
    assert sorted(os.listdir(folder)) == ["latest.pt", "lora-1.pt", "lora-2.pt"]
    ck = torch.load(os.path.join(folder, "latest.pt"), map_location="cpu")
    assert ck["batch"] == 2 and ck["base_path"] == base_path and "model" not in ck["state"] and ck["optimizer"]["step"] == 2
    assert os.path.getsize(os.path.join(folder, "latest.pt")) < 4 * 4 * ad.total + (1 << 20), "an adapter checkpoint, not a full one"
    assert torch.equal(ck["lora"]["blocks.0.attn.qkv.lora_B.weight"], ad.B("blocks.0.attn.qkv.weight").cpu())
    first = torch.load(os.path.join(folder, "lora-1.pt"), map_location="cpu")
    assert first["batch"] == 1 and not torch.equal(first["lora"]["blocks.0.attn.qkv.lora_B.weight"], ck["lora"]["blocks.0.attn.qkv.lora_B.weight"])
    loaded = lora.LoRA.from_state_dict(dit, first["lora"], device="cpu")
    assert loaded.rank == 4 and loaded.scale == 2.0
    assert torch.equal(loaded.B("blocks.0.attn.qkv.weight"), first["lora"]["blocks.0.attn.qkv.lora_B.weight"])
    tr2 = train_mod.train(cfg(3, autoresume=True))
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert any(l.get("resumed_from") for l in out) and [l["batch"] for l in out if "loss" in l] == [3]
    ad2 = tr2.opt.adapter
    assert tr2.opt.step_count == 3 and tr2.batches_seen == 3 and bool(tr2.opt.m.any())
    saved_b = ck["lora"]["blocks.0.attn.qkv.lora_B.weight"]
    moved = (ad2.B("blocks.0.attn.qkv.weight").cpu() - saved_b).abs().max()
    # one more AdamW step from the restored state moves a weight by about lr: a restart from B = 0 or from zero moments would not
    assert 0 < float(moved) <= 1.5e-3 * 3
    assert sorted(os.listdir(folder)) == ["latest.pt", "lora-1.pt", "lora-2.pt", "lora-3.pt"]
