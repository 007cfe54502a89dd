"""Image-conditioned sampling against the plain run (`edm_sampler_loop(..., init_latents=, inpaint_mask=, resample=)`):
MicroDiT_XL_2 with random weights, B = 64 images, 30 Heun steps, cond_cache on, guidance 5.  Four series are timed in one process on one
GPU:
  plain          the run from pure noise (59 network evaluations)
  plain_again    the same call once more: the ratio of the two medians and their spread are the run-to-run noise of this measurement
  inpaint_r1     init_latents + a centred half-size mask (1 inside the hole): one draw and one md_edm_blend_known launch per step more,
                 plus the initialisation and the final paste; the same 59 evaluations
  inpaint_r2     the same with resample = 2: 2 * 2 * 29 + 1 = 117 evaluations, and one draw + md_edm_churn per repeated step
Every series is warmed up once (code objects, allocator), then the four alternate for --repeats rounds; each run is bracketed by device
events and ends in a synchronise.  No ratio is asserted; the expectation written down with the result is inpaint_r1 / plain within the
noise and inpaint_r2 / plain about 117 / 59.
The timed interval of the two inpaint series includes what edm_sampler_loop does once per run with its operands: init_latents to fp64 and
the mask to fp32 (two small copies); the mask is passed as bool, so its range check, which synchronises with the host, does not run.
The plain series pay for neither: that is part of what inpaint_r1 / plain compares.
Launches per run are the C-ABI calls (one kernel each on this path) counted through a proxy around the library in one extra run per
series, with the calls of md_edm_blend_known and md_edm_churn listed separately; torch's own kernels (the draws, the timestep fill) are
not in the count.
Writes profiles/edit_sampler.json.
Usage: python scripts/bench_edit_sampler.py [--batch 64] [--steps 30] [--guidance 5] [--repeats 3] [--arch MicroDiT_XL_2] [--out FILE]"""
import argparse
import collections
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
ap.add_argument("--repeats", type=int, default=3, help="timed runs per series (>= 2)")
ap.add_argument("--arch", default="MicroDiT_XL_2")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_sampler.json"))
args = ap.parse_args()
assert args.repeats >= 2 and args.steps >= 3
assert torch.cuda.is_available(), "bench_edit_sampler.py measures on the GPU; there is no CPU path"


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
init = torch.randn(B, dit.in_channels, R, R, device="cuda", generator=g) * 0.5
mask = torch.zeros(R, R, device="cuda", dtype=torch.bool)
mask[R // 4:R // 4 + R // 2, R // 4:R // 4 + R // 2] = True             # centred, half the size: a quarter of the image is generated
SERIES = {"plain": {}, "plain_again": {},
          "inpaint_r1": dict(init_latents=init, inpaint_mask=mask),
          "inpaint_r2": dict(init_latents=init, inpaint_mask=mask, resample=2)}


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
    return {"total": sum(proxy.calls.values()), "md_edm_blend_known": proxy.calls["md_edm_blend_known"],
            "md_edm_churn": proxy.calls["md_edm_churn"]}


evaluations = {s: samplers.edit_evaluations("heun", args.steps, 1.0, kw.get("resample", 1)) for s, kw in SERIES.items()}
res = {"device": torch.cuda.get_device_name(0), "arch": args.arch, "batch": B, "steps": args.steps, "sampler": "heun",
       "guidance": args.guidance, "repeats": args.repeats, "cond_cache": True, "mask": f"centred {R // 2} x {R // 2} hole in {R} x {R}",
       "timing": "device events around edm_sampler_loop, one run each, the four series alternating after one warm-up run of each",
       "evaluations": evaluations}
finite, kept = {}, {}
for s in SERIES:                                  # warm-up of every series at this shape
    out = run(s)[0]
    finite[s] = bool(torch.isfinite(out).all())
    if "inpaint_mask" in SERIES[s]:
        keep = (~mask).expand(out.shape)
        kept[s] = bool(torch.equal(out[keep], init[keep]))
ms = {s: [] for s in SERIES}
for _ in range(args.repeats):
    for s in SERIES:
        ms[s].append(run(s)[1])
med = {s: statistics.median(v) for s, v in ms.items()}
base = med["plain"]
both = ms["plain"] + ms["plain_again"]
res.update({"finite": finite, "kept_region_exact": kept, "ms": ms, "median_ms": med, "ms_per_image": {s: v / B for s, v in med.items()},
            "ratio_to_plain": {s: v / base for s, v in med.items()},
            "plain_spread_rel": (max(both) - min(both)) / base,
            "expected_ratio": {"inpaint_r1": 1.0, "inpaint_r2": evaluations["inpaint_r2"] / evaluations["plain"]},
            "launches_per_run": {s: count_launches(s) for s in SERIES if s != "plain_again"}})
for s in SERIES:
    print(f"{s:12s} B={B}  {med[s]:9.1f} ms  ratio {med[s] / base:.4f}  evaluations {evaluations[s]}", flush=True)
print(f"spread of the {len(both)} plain runs: {res['plain_spread_rel']:.4f} of their median;  launches per run {res['launches_per_run']}", flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"out": args.out, "ratio_to_plain": res["ratio_to_plain"], "plain_spread_rel": res["plain_spread_rel"]}))
