"""Cost and numerical distance of the step cache (`edm_sampler_loop(..., step_cache=StepCache(...))`): MicroDiT_XL_2 with
random weights, B = 64 images, 30 Heun steps (59 network evaluations), guidance 5 (network batch 2B), cond_cache on.
Variants: plain (no step cache), plain_again (the same run again: what two identical series differ by), interval=2, interval=3, and two
thresholds chosen here from the distances the plain schedule records -- a run with threshold=0 is full everywhere, so its probe measures
the plain trajectory: the thresholds are the sums of 2 and of 3 median distances, about what interval=2 / 3 would accumulate.
All variants alternate inside one process after one warm-up run of each; every run is bracketed by device events and ends in a
synchronise.  Reported per variant: the latency ratio to plain next to the spread of the plain runs, the full / reused evaluation counts,
and the relative L2 difference of the final latents from the plain run.  With random weights that difference is a numerical distance --
how far reuse moves the result of this network -- not a quality measure: there is no trained model behind it.
One full and one reused engine evaluation at the run's network batch are timed on their own as well; "reused_slower_than_full" records
whether a reused evaluation measured slower than a full one.
Writes profiles/step_cache.json.
Usage: python scripts/bench_step_cache.py [--batch 64] [--steps 30] [--guidance 5] [--repeats 3] [--arch MicroDiT_XL_2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import dit as mdit  # noqa: E402
from micro_diffusion_amd.engine import ResidualCache  # noqa: E402
from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub  # noqa: E402
from micro_diffusion_amd.step_cache import StepCache  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--repeats", type=int, default=3, help="timed runs per variant (>= 2: the noise floor is the spread of the plain ones)")
ap.add_argument("--arch", default="MicroDiT_XL_2")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_cache.json"))
args = ap.parse_args()
assert args.repeats >= 2 and args.steps >= 3
assert torch.cuda.is_available(), "bench_step_cache.py measures on the GPU; there is no CPU path"

torch.manual_seed(0)
dit = getattr(mdit, args.arch)().to("cuda")
flat = dit.flat_buffers()
flat["p"].normal_(0.0, 0.02, generator=torch.Generator(device="cuda").manual_seed(1))     # random weights: the reference's init zeroes
dit.refresh_shadow(force=True)                                                            # the adaLN and output layers
model = LatentDiffusion(dit, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=dit.input_size)
model.eval()
eng = dit.engine
B = args.batch
g = torch.Generator(device="cuda").manual_seed(100 + B)
lat = torch.randn(B, dit.in_channels, dit.input_size, dit.input_size, device="cuda", generator=g)
y = torch.randn(B, 1, 77, dit.config.caption_channels, device="cuda", generator=g)


def run(sc):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = model.edm_sampler_loop(lat, y, steps=args.steps, cfg=args.guidance, cond_cache=True, step_cache=sc)
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


# the distances of the plain trajectory: every evaluation full, the probe running
probe = StepCache(threshold=0.0)
run(probe)
dist = [d for d in probe.stats.distances if d is not None]
med = statistics.median(dist)
thresholds = [2.0 * med, 3.0 * med]
variants = {"plain": None, "plain_again": None, "interval=2": StepCache(interval=2), "interval=3": StepCache(interval=3)}
for t in thresholds:
    variants[f"threshold={t:.4g}"] = StepCache(threshold=t)

final, ms = {}, {k: [] for k in variants}
for k, sc in variants.items():                      # warm-up of every variant (code objects, allocator) + the result that is compared
    final[k] = run(sc)[0]
for _ in range(args.repeats):
    for k, sc in variants.items():
        ms[k].append(run(sc)[1])

ref = final["plain"].double()
med_ms = {k: statistics.median(v) for k, v in ms.items()}
report = {}
for k, sc in variants.items():
    r = {"ms": ms[k], "median_ms": med_ms[k], "ms_per_image": med_ms[k] / B, "ratio_to_plain": med_ms[k] / med_ms["plain"],
         "finite": bool(torch.isfinite(final[k]).all()), "bit_identical_to_plain": bool(torch.equal(final[k], final["plain"])),
         "rel_l2_to_plain": float(((final[k].double() - ref).pow(2).sum().sqrt() / ref.pow(2).sum().sqrt()).item())}
    if sc is not None:
        s = sc.stats
        r.update({"evaluations": s.evaluations, "full": s.full, "reused": s.reused,
                  "decisions": "".join("F" if d else "r" for d in s.decisions),
                  "policy": {"interval": sc.interval, "threshold": sc.threshold, "warmup": sc.warmup, "tail": sc.tail}})
    report[k] = r
    print(f"{k:22s} {med_ms[k]:9.1f} ms  ratio {r['ratio_to_plain']:.4f}  full/reused {r.get('full', '-')}/{r.get('reused', '-')}  "
          f"rel L2 to plain {r['rel_l2_to_plain']:.3e}", flush=True)


def time_evaluation(reuse, rc, cond, patches, t, n=10):
    """Median milliseconds of one engine evaluation (full with the delta store, or reused) at the run's network batch."""
    out = []
    for i in range(n + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.forward(None, t, None, cond=cond, patches=patches, step_cache=rc, reuse=reuse)
        e1.record()
        e1.synchronize()
        if i >= 2:
            out.append(e0.elapsed_time(e1))
    return statistics.median(out)


Bn = 2 * B if args.guidance > 1.0 else B
cond = dit.encode_condition(torch.cat([y, torch.zeros_like(y)], 0) if args.guidance > 1.0 else y)
patches = torch.randn(Bn * dit.config.tokens, dit.config.patch_vec, device="cuda", generator=g).to(torch.bfloat16)
t = torch.full((Bn,), 0.1, device="cuda")
per_eval = {}
for name, with_probe in (("fixed", False), ("adaptive", True)):
    rc = ResidualCache(probe=with_probe)
    full_ms = time_evaluation(False, rc, cond, patches, t)
    reused_ms = time_evaluation(True, rc, cond, patches, t)
    per_eval[name] = {"full_ms": full_ms, "reused_ms": reused_ms, "reused_over_full": reused_ms / full_ms, "cache_nbytes": rc.nbytes}
    print(f"one evaluation at batch {Bn} ({name}): full {full_ms:.2f} ms  reused {reused_ms:.2f} ms  ratio {reused_ms / full_ms:.4f}", flush=True)

res = {"device": torch.cuda.get_device_name(0), "arch": args.arch, "batch": B, "network_batch": Bn, "steps": args.steps, "sampler": "heun",
       "guidance": args.guidance, "cond_cache": True, "repeats": args.repeats, "evaluations": probe.stats.evaluations,
       "timing": "device events around edm_sampler_loop, one run each, the variants alternating after one warm-up run of each",
       "plain_distances": {"min": min(dist), "median": med, "max": max(dist), "all": dist},
       "thresholds": thresholds, "plain_spread_rel": (max(ms["plain"]) - min(ms["plain"])) / med_ms["plain"],
       "rel_l2_note": "random weights: a numerical distance of the final latents from the plain run, not a quality measure",
       "variants": report, "one_evaluation": per_eval,
       "reused_slower_than_full": bool(any(v["reused_ms"] > v["full_ms"] for v in per_eval.values()))}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"out": args.out, "plain_spread_rel": res["plain_spread_rel"], "reused_slower_than_full": res["reused_slower_than_full"]}))
