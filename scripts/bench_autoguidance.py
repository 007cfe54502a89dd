"""Autoguidance against classifier-free guidance (`edm_sampler_loop(..., guide=...)`): MicroDiT_XL_2 with random weights,
B = 64 images, 30 steps of dpmpp_2m (30 network evaluations) and of heun (59), cond_cache on, guidance weight 5.  Three configurations
are timed in one process on one GPU:
  cfg_2b       classifier-free guidance by batch doubling: one network at batch 2B per evaluation (the baseline)
  auto_same    autoguidance with a guide of the main architecture (other random weights): two networks at batch B
  auto_small   autoguidance with a small guide (--guide-arch, MicroDiT_Tiny_2): main at batch B + the small network at batch B
Every configuration is warmed up once per solver (code objects, allocator), then the three alternate for --repeats rounds; each run is
bracketed by device events and ends in a synchronise.  The spread (max - min) of the baseline runs is the noise floor.  No ratio is
asserted: another guide returns another sample, so nothing is compared but time.
Launches per evaluation are the C-ABI calls (one kernel each on this path) counted through a proxy around the library in two short extra
runs (3 and 5 Heun evaluations: the difference isolates the per-evaluation part from the one-off encodes); torch's own fill kernel for
the timestep tensor (1 per evaluation) is not in the count.
Extra resident bytes of a guide: its weights (the bf16 shadow the forward pass reads; the module as built also holds fp32 masters and
an fp32 gradient buffer, reported separately) plus its conditioning cache at batch B; the baseline's cache is encoded at batch 2B.
Writes profiles/autoguidance.json.
Usage: python scripts/bench_autoguidance.py [--batch 64] [--steps 30] [--guidance 5] [--repeats 3] [--arch MicroDiT_XL_2]
                                            [--guide-arch MicroDiT_Tiny_2] [--sampler dpmpp_2m heun] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import dit as mdit, hip, samplers  # noqa: E402
from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--repeats", type=int, default=3, help="timed runs per configuration and solver (>= 2: the noise floor is the spread of the baseline)")
ap.add_argument("--arch", default="MicroDiT_XL_2")
ap.add_argument("--guide-arch", default="MicroDiT_Tiny_2")
ap.add_argument("--sampler", nargs="+", default=["dpmpp_2m", "heun"], choices=list(samplers.SAMPLERS))
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autoguidance.json"))
args = ap.parse_args()
assert args.repeats >= 2 and args.steps >= 3 and args.guidance > 1.0
assert torch.cuda.is_available(), "bench_autoguidance.py measures on the GPU; there is no CPU path"


class _CountingLib:
    """Proxy around the loaded library: counts every call of an entry point."""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls += 1
            return fn(*a)
        return call


def make(arch, seed):
    torch.manual_seed(seed)
    d = getattr(mdit, arch)().to("cuda")
    d.flat_buffers()["p"].normal_(0.0, 0.02, generator=torch.Generator(device="cuda").manual_seed(seed + 1))   # random weights: the
    d.refresh_shadow(force=True)                                                                               # reference's init zeroes
    return d                                                                                                   # the output layers


main = make(args.arch, 0)
guides = {"cfg_2b": None, "auto_same": make(args.arch, 10), "auto_small": make(args.guide_arch, 20)}
model = LatentDiffusion(main, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=main.input_size)
model.eval()
B = args.batch
g = torch.Generator(device="cuda").manual_seed(100 + B)
lat = torch.randn(B, main.in_channels, main.input_size, main.input_size, device="cuda", generator=g)
y = torch.randn(B, 1, 77, main.config.caption_channels, device="cuda", generator=g)


def run(config, sampler, steps=args.steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = model.edm_sampler_loop(lat, y, steps=steps, cfg=args.guidance, cond_cache=True, sampler=sampler, guide=guides[config])
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def count_launches(config):
    """(C-ABI calls per evaluation, one-off calls per run) of the Heun loop: 2 and 3 steps are 3 and 5 evaluations."""
    real = hip.lib()
    proxy = _CountingLib(real)
    engines = [d.engine for d in (main, guides[config]) if d is not None]
    hip._lib = proxy
    for e in engines:
        e.L = proxy
    try:
        n = []
        for steps in (2, 3):
            proxy.calls = 0
            run(config, "heun", steps)
            n.append(proxy.calls)
    finally:
        hip._lib = real
        for e in engines:
            e.L = real
    assert (n[1] - n[0]) % 2 == 0
    per_eval = (n[1] - n[0]) // 2
    return per_eval, n[0] - 3 * per_eval


def resident(config):
    """Bytes a configuration keeps on the device next to the main network's weights: conditioning cache(s) and the guide."""
    guide = guides[config]
    if guide is None:
        cond = main.encode_condition(torch.cat([y, torch.zeros_like(y)], 0))
        return {"main_conditioning_nbytes": cond.nbytes, "guide_conditioning_nbytes": 0, "guide_weight_nbytes": 0,
                "guide_module_nbytes": 0, "extra_over_unguided_nbytes": cond.nbytes // 2}
    cm, cg = main.encode_condition(y), guide.encode_condition(y)
    f = guide.flat_buffers()
    shadow = f["s"].numel() * f["s"].element_size()
    module = sum(f[k].numel() * f[k].element_size() for k in ("p", "g", "s"))
    return {"main_conditioning_nbytes": cm.nbytes, "guide_conditioning_nbytes": cg.nbytes, "guide_weight_nbytes": shadow,
            "guide_module_nbytes": module, "extra_over_unguided_nbytes": shadow + cg.nbytes}


res = {"device": torch.cuda.get_device_name(0), "arch": args.arch, "guide_arch": args.guide_arch, "batch": B, "steps": args.steps,
       "guidance": args.guidance, "repeats": args.repeats, "cond_cache": True,
       "timing": "device events around edm_sampler_loop, one run each, the three configurations alternating after one warm-up run of each",
       "parameters": {"main": main.flat_buffers()["total"], "auto_same": guides["auto_same"].flat_buffers()["total"],
                      "auto_small": guides["auto_small"].flat_buffers()["total"]},
       "solvers": {}}
for sampler in args.sampler:
    ec = model.edm_config
    n_eval = len(samplers.evaluation_sigmas(sampler, samplers.edm_schedule(args.steps, ec.sigma_min, ec.sigma_max, ec.rho)))
    finite = {}
    for config in guides:                          # warm-up of every configuration at this shape
        finite[config] = bool(torch.isfinite(run(config, sampler)[0]).all())
    ms = {config: [] for config in guides}
    for _ in range(args.repeats):
        for config in guides:
            ms[config].append(run(config, sampler)[1])
    med = {config: statistics.median(v) for config, v in ms.items()}
    base = med["cfg_2b"]
    r = {"evaluations": n_eval, "network_batches": {"cfg_2b": [2 * B], "auto_same": [B, B], "auto_small": [B, B]}, "finite": finite,
         "ms": ms, "median_ms": med, "ms_per_image": {c: v / B for c, v in med.items()},
         "ratio_to_cfg_2b": {c: v / base for c, v in med.items()},
         "cfg_2b_noise_floor_rel": (max(ms["cfg_2b"]) - min(ms["cfg_2b"])) / base}
    res["solvers"][sampler] = r
    print(f"{sampler:9s} B={B}  " + "  ".join(f"{c} {med[c]:9.1f} ms ({med[c] / base:.4f})" for c in guides) +
          f"  noise {r['cfg_2b_noise_floor_rel']:.4f}", flush=True)
res["launches_per_evaluation"], res["one_off_launches"], res["resident"] = {}, {}, {}
for config in guides:
    per_eval, one_off = count_launches(config)
    res["launches_per_evaluation"][config], res["one_off_launches"][config] = per_eval, one_off
    res["resident"][config] = resident(config)
    print(f"{config:10s} launches/eval {per_eval}  one-off {one_off}  extra resident "
          f"{res['resident'][config]['extra_over_unguided_nbytes'] / 2**20:.1f} MiB", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"out": args.out, "ratios": {s: r["ratio_to_cfg_2b"] for s, r in res["solvers"].items()}}))
