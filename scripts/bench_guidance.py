"""Guidance modes against plain classifier-free guidance (`edm_sampler_loop(..., guidance_mode=)`): MicroDiT_XL_2 with
random weights, B = 64 images, 30 Heun steps, cond_cache on, guidance 5.  Four series are timed in one process on one GPU:
  cfg            the default combine inside the update kernel (59 guided network evaluations at batch 2B)
  cfg_again      the same call once more: the ratio of the two medians and the spread of all cfg runs are the noise floor
  rescale        guidance_mode="rescale", guidance_rescale = 0.7
  apg            guidance_mode="apg", apg_eta = 0, apg_norm_threshold = 15, apg_momentum = -0.5 (the paper's settings for a 4-channel
                 latent space are of this order; the threshold only changes a coefficient, never the work)
The two modes run the same network evaluations and, per guided evaluation, md_guidance_prepare_tok (one workgroup per sample: M, five
moments, two coefficients) in front of the _coef form of the update kernel: one launch and a few passes over about 1 MB of state more.
Every series is warmed up once (code objects, allocator), then the four alternate for --repeats rounds; each run is bracketed by device
events and ends in a synchronise.  No ratio is asserted.
Launches per run are the C-ABI calls (one kernel each on this path) counted through a proxy around the library in one extra run per
series, with the guidance entry points listed separately; torch's own kernels (the timestep fill) are not in the count.
Writes profiles/guidance_modes.json.
Usage: python scripts/bench_guidance.py [--batch 64] [--steps 30] [--guidance 5] [--repeats 3] [--arch MicroDiT_XL_2] [--out FILE]"""
import argparse
import collections
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import dit as mdit, hip  # noqa: E402
from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--repeats", type=int, default=3, help="timed runs per series (>= 2)")
ap.add_argument("--arch", default="MicroDiT_XL_2")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_modes.json"))
args = ap.parse_args()
assert args.repeats >= 2 and args.steps >= 3
assert torch.cuda.is_available(), "bench_guidance.py measures on the GPU; there is no CPU path"


class _CountingLib:
    """Proxy around the loaded library: counts every call of an entry point, by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] += 1
            return fn(*a)
        return call


torch.manual_seed(0)
dit = getattr(mdit, args.arch)().to("cuda")
dit.flat_buffers()["p"].normal_(0.0, 0.02, generator=torch.Generator(device="cuda").manual_seed(1))       # random weights: the reference's
dit.refresh_shadow(force=True)                                                                            # init zeroes the output layers
model = LatentDiffusion(dit, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=dit.input_size)
model.eval()
B, R = args.batch, dit.input_size
g = torch.Generator(device="cuda").manual_seed(100 + B)
lat = torch.randn(B, dit.in_channels, R, R, device="cuda", generator=g)
y = torch.randn(B, 1, 77, dit.config.caption_channels, device="cuda", generator=g)
SERIES = {"cfg": {}, "cfg_again": {},
          "rescale": dict(guidance_mode="rescale", guidance_rescale=0.7),
          "apg": dict(guidance_mode="apg", apg_eta=0.0, apg_norm_threshold=15.0, apg_momentum=-0.5)}
GUIDANCE_CALLS = ("md_guidance_prepare_tok", "md_edm_heun_update_coef_tok", "md_edm_heun_update_tok")


def run(series):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = model.edm_sampler_loop(lat, y, steps=args.steps, cfg=args.guidance, cond_cache=True, **SERIES[series])
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def count_launches(series):
    real = hip.lib()
    proxy = _CountingLib(real)
    hip._lib, dit.engine.L = proxy, proxy
    try:
        run(series)
    finally:
        hip._lib, dit.engine.L = real, real
    return dict({"total": sum(proxy.calls.values())}, **{k: proxy.calls[k] for k in GUIDANCE_CALLS})


res = {"device": torch.cuda.get_device_name(0), "arch": args.arch, "batch": B, "steps": args.steps, "sampler": "heun",
       "guidance": args.guidance, "repeats": args.repeats, "cond_cache": True, "evaluations": 2 * args.steps - 1,
       "series": {s: {k: v for k, v in kw.items()} for s, kw in SERIES.items()},
       "timing": "device events around edm_sampler_loop, one run each, the four series alternating after one warm-up run of each"}
finite, outs = {}, {}
for s in SERIES:                                  # warm-up of every series at this shape
    outs[s] = run(s)[0]
    finite[s] = bool(torch.isfinite(outs[s]).all())
ms = {s: [] for s in SERIES}
for _ in range(args.repeats):
    for s in SERIES:
        ms[s].append(run(s)[1])
med = {s: statistics.median(v) for s, v in ms.items()}
base = med["cfg"]
both = ms["cfg"] + ms["cfg_again"]
std = lambda t: t.double().flatten(1).std(dim=1).mean().item()      # noqa: E731
res.update({"finite": finite, "ms": ms, "median_ms": med, "ms_per_image": {s: v / B for s, v in med.items()},
            "ratio_to_cfg": {s: v / base for s, v in med.items()},
            "cfg_spread_rel": (max(both) - min(both)) / base,
            "extra_ms_per_guided_evaluation": {s: (med[s] - base) / (2 * args.steps - 1) for s in ("rescale", "apg")},
            "mean_sample_std": {s: std(outs[s]) for s in SERIES if s != "cfg_again"},
            "launches_per_run": {s: count_launches(s) for s in SERIES if s != "cfg_again"}})
for s in SERIES:
    print(f"{s:10s} B={B}  {med[s]:9.1f} ms  ratio {med[s] / base:.4f}", flush=True)
print(f"spread of the {len(both)} cfg runs: {res['cfg_spread_rel']:.4f} of their median;  launches per run {res['launches_per_run']}", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"out": args.out, "ratio_to_cfg": res["ratio_to_cfg"], "cfg_spread_rel": res["cfg_spread_rel"]}))
