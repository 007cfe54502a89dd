"""Cost of measurement-guided sampling on an MI355X: XL/2, 32 x 32 latents, caption length 77, B = 64, 30 steps, cfg 5
(every evaluation runs the network at batch 128), conditioning cache on unless stated:
  * guided / plain latency of edm_sampler_loop for heun and dpmpp_2m (4 x 4 super-resolution measurement), same process, runs in
    alternating order, each run between two device events;
  * the guided heun run with the conditioning cache against the one without;
  * the backward of one guided evaluation with the early return (input_grads=("x",)) against the full dgrad-only backward
    (("x", "t", "y")), forward excluded;
  * the four kernels alone: time per call, bytes moved, fraction of the 8 TB/s HBM3E peak.
No threshold is set anywhere: the numbers are recorded as measured.
`--parent-bench FILE` / `--head-bench FILE` (repeatable): files holding the JSON result line bench.py printed at the parent commit and at
this one in the same session, in run order; their headlines are recorded next to the measurements.
Writes a JSON file (default profiles/measurement_guidance.json).
Usage: python scripts/bench_measurement_guidance.py [--batch 64] [--steps 30] [--rounds 2] [--parent-bench FILE]... [--head-bench FILE]... [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from micro_diffusion_amd import hip  # noqa: E402
from micro_diffusion_amd import dit as mdit  # noqa: E402
from micro_diffusion_amd.inverse import LinearMeasurement  # noqa: E402
from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub  # noqa: E402

HBM_PEAK_TBS = 8.0

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--cfg", type=float, default=5.0)
ap.add_argument("--kernel-groups", type=int, default=10)
ap.add_argument("--parent-bench", action="append", default=[])
ap.add_argument("--head-bench", action="append", default=[])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measurement_guidance.json"))
args = ap.parse_args()

torch.cuda.set_device(0)
dev = torch.device("cuda")
B, C, H, p, s = args.batch, 4, 32, 2, 4
out = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "model": "MicroDiT_XL_2",
       "setting": {"batch": B, "latent": H, "tokens": (H // p) ** 2, "caption_len": 77, "steps": args.steps, "cfg": args.cfg, "pool": s,
                   "measurement_scale": 1.0}, "hbm_peak_tbs": HBM_PEAK_TBS}
L = hip.lib()
st = torch.cuda.current_stream().cuda_stream


def timed(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n          # ms per call


# ---- the four kernels alone (the guided half of a doubled batch: has_uncond = 1)
PER = 20
n, T, pv = B * C * H * H, (H // p) ** 2, C * p * p
x64 = torch.randn(B, C, H, H, device=dev, dtype=torch.float64)
tok = torch.randn(2 * B * T, pv, device=dev).to(torch.bfloat16)
Fimg = torch.randn(2 * B, C, H, H, device=dev)
D, q, meas = torch.randn(B, C, H, H, device=dev), torch.empty(B, C, H, H, device=dev), torch.randn(B, C, H // s, H // s, device=dev)
mask = (torch.rand(B, (H // s) ** 2, device=dev) < 0.6).float()
Lb, dtok, dx = torch.ones(B, device=dev, dtype=torch.float64), torch.empty(2 * B * T, pv, device=dev, dtype=torch.bfloat16), torch.randn(2 * B, C, H, H, device=dev)
kernels = {
    "md_edm_denoised": (lambda: L.md_edm_denoised(x64.data_ptr(), Fimg.data_ptr(), D.data_ptr(), B, C * H * H, args.cfg, 1, 1.0, 0.9, st),
                        n * (8 + 4 + 4 + 4)),
    "md_edm_denoised_tok": (lambda: L.md_edm_denoised_tok(x64.data_ptr(), tok.data_ptr(), D.data_ptr(), B, C, H, H, p, args.cfg, 1, 1.0, 0.9, st),
                            n * (8 + 2 + 2 + 4)),
    "md_measure_residual": (lambda: L.md_measure_residual(D.data_ptr(), meas.data_ptr(), mask.data_ptr(), B, q.data_ptr(), Lb.data_ptr(), B, C, H,
                                                          H, s, st), n * (4 + 4) + (n // (s * s)) * 4 + B * (H // s) ** 2 * 4),
    "md_guide_cotangent_tok": (lambda: L.md_guide_cotangent_tok(q.data_ptr(), dtok.data_ptr(), B, C, H, H, p, args.cfg, 1, 1.0, 0.9, st),
                               n * (4 + 2 + 2)),
    "md_edm_guide_apply": (lambda: L.md_edm_guide_apply(x64.data_ptr(), q.data_ptr(), dx.data_ptr(), Lb.data_ptr(), B, C * H * H, 1, 1e-3, 1.0,
                                                        0.9, st), n * (8 + 8 + 4 + 4 + 4)),
}
out["kernels_alone"] = {}
for name, (call, nbytes) in kernels.items():
    assert call() == 0, name
    timed(call, 3)
    times = [1e3 * timed(call, PER) for _ in range(args.kernel_groups)]
    med = statistics.median(times)
    out["kernels_alone"][name] = {"bytes": nbytes, "median_us_per_call": med, "min_us": min(times), "max_us": max(times),
                                  "launches_per_group": PER, "groups": len(times), "tbs": nbytes / med / 1e6,
                                  "frac_of_hbm_peak": nbytes / med / 1e6 / HBM_PEAK_TBS, "roofline_us_at_hbm_peak": nbytes / HBM_PEAK_TBS / 1e6}
    print(name, json.dumps(out["kernels_alone"][name]), flush=True)

# ---- the sampler
net = mdit.MicroDiT_XL_2().to(dev)
model = LatentDiffusion(net, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"))
model.eval()
g = torch.Generator(device="cpu").manual_seed(B)
lat = torch.randn(B, C, H, H, generator=g).to(dev)
y = torch.randn(B, 1, 77, 1024, generator=g).to(dev)
truth = (0.5 * torch.randn(B, C, H, H, generator=g)).to(dev)
lm = LinearMeasurement(F.avg_pool2d(truth, s), s)


def run(sampler, guided, cache=True):
    kw = dict(measurement=lm, measurement_scale=1.0) if guided else {}
    return lambda: model.edm_sampler_loop(lat, y, steps=args.steps, cfg=args.cfg, fused=True, cond_cache=cache, sampler=sampler, **kw)


sides = {"heun_plain": run("heun", False), "heun_guided": run("heun", True), "dpmpp_2m_plain": run("dpmpp_2m", False),
         "dpmpp_2m_guided": run("dpmpp_2m", True), "heun_guided_uncached": run("heun", True, False), "heun_plain_uncached": run("heun", False, False)}
ms = {k: [] for k in sides}
run("euler", True)()                         # warm-up: every kernel of both paths has run once
run("euler", True, False)()
torch.cuda.synchronize()
for rnd in range(args.rounds):
    order = list(sides.items())
    for name, fn in (order if rnd % 2 == 0 else order[::-1]):
        ms[name].append(timed(fn))
        print(name, rnd, ms[name][-1], flush=True)
med = {k: statistics.median(v) for k, v in ms.items()}
out["sampler"] = {"ms_per_run": ms, "median_ms": med,
                  "guided_over_plain": {"heun": med["heun_guided"] / med["heun_plain"], "dpmpp_2m": med["dpmpp_2m_guided"] / med["dpmpp_2m_plain"]},
                  "guided_heun_cached_over_uncached": med["heun_guided"] / med["heun_guided_uncached"],
                  "plain_heun_cached_over_uncached": med["heun_plain"] / med["heun_plain_uncached"]}
print("sampler", json.dumps(out["sampler"]), flush=True)

# ---- the backward of one guided evaluation, with and without the early return (batch 2B, uncached tape: both forms exist on it)
eng = net.engine
net.requires_grad_(False)
x2 = torch.randn(2 * B, C, H, H, device=dev)
t2 = torch.full((2 * B,), 0.1, device=dev)
y2 = torch.cat([y, torch.zeros_like(y)], 0)
dt2 = torch.randn(2 * B * T, pv, device=dev).to(torch.bfloat16)
res = {}
for name, want in (("to_the_image", ("x",)), ("dgrad_only_all_inputs", ("x", "t", "y"))):
    times, count = [], None
    for i in range(2 + 2 * args.rounds):
        tape = eng.forward(x2, t2, y2, record_tape=True)
        eng.gemm_log = [] if i == 0 else None
        t_ms = timed(lambda: eng.backward(tape, dt2, input_grads=want, param_grads=False))
        if i == 0:
            count, eng.gemm_log = len(eng.gemm_log), None
        elif i >= 2:
            times.append(t_ms)
    res[name] = {"ms": times, "median_ms": statistics.median(times), "gemm_launches": count}
res["to_the_image_over_all_inputs"] = res["to_the_image"]["median_ms"] / res["dgrad_only_all_inputs"]["median_ms"]
out["backward_one_evaluation"] = res
print("backward", json.dumps(res), flush=True)

for key, paths in (("parent_commit_bench", args.parent_bench), ("this_commit_bench", args.head_bench)):
    runs = []
    for path_ in paths:
        with open(path_) as fh:
            line = [ln for ln in fh.read().splitlines() if ln.startswith("{")][-1]
        pb = json.loads(line)
        runs.append({k: pb[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup") if k in pb})
    if runs:
        out[key] = runs
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
