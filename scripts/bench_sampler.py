"""A/B of the sampler's conditioning cache (`edm_sampler_loop(..., cond_cache=True)`): MicroDiT_XL_2 with random weights, 30 Heun
steps (59 network evaluations), guidance 5 (the batch is doubled), at B = 4, 16 and 64 images.
Cached and uncached runs alternate inside one process after a warm-up of each; every run is bracketed by device events and ends
in a synchronise.  The spread (max - min) of the uncached runs is the noise floor: the cached path passes a size when its median is
not slower than the uncached median by more than that.  The two paths must also return identical bits.
Launches per evaluation are the C-ABI calls (one kernel each on this path) counted through a proxy around the library in short
extra runs (3 and 5 evaluations: the difference isolates the per-evaluation part from the one-off encode); torch's own fill / copy
kernels around them (the timestep tensor: 2 per evaluation uncached, 1 cached) are not in the count.
Solvers (`--sampler`, `--guidance-interval`): every named solver other than the default run (Heun, no interval) is timed against that
default run in the same way -- same process, same inputs and cache setting, the two alternating, device events around whole runs -- and
reported under "solvers" with its evaluation count, its guided evaluations and the network samples per image (evaluations + guided
evaluations: a guided one runs the doubled batch); the counts follow from the schedule (samplers.evaluation_sigmas / is_guided).  There
is no bar on these: another solver returns another sample, so nothing is compared but time.
Writes profiles/sampler_cache.json.  Exit status 1 when a size loses by more than the noise floor or the results differ.
Usage: python scripts/bench_sampler.py [--sizes 4 16 64] [--steps 30] [--guidance 5] [--repeats 3] [--arch MicroDiT_XL_2] [--out FILE]
                                       [--sampler heun euler dpmpp_2m] [--guidance-interval LO HI] [--solver-cache 0 1]"""
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
ap.add_argument("--sizes", type=int, nargs="+", default=[4, 16, 64])
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--repeats", type=int, default=3, help="timed runs per side and size (>= 2: the noise floor is the spread of the uncached ones)")
ap.add_argument("--arch", default="MicroDiT_XL_2")
ap.add_argument("--sampler", nargs="+", default=["heun"], choices=list(samplers.SAMPLERS),
                help="solvers to time against the default Heun run (heun itself is timed only together with --guidance-interval)")
ap.add_argument("--guidance-interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                help="guide only while LO <= sigma <= HI (applies to the solvers of --sampler, not to the default run they are compared with)")
ap.add_argument("--solver-cache", type=int, nargs="+", default=[1], choices=[0, 1], help="cond_cache settings of the solver comparison")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_cache.json"))
args = ap.parse_args()
assert args.repeats >= 2 and args.steps >= 2
assert torch.cuda.is_available(), "bench_sampler.py measures on the GPU; there is no CPU path"


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


torch.manual_seed(0)
dit = getattr(mdit, args.arch)().to("cuda")
flat = dit.flat_buffers()
flat["p"].normal_(0.0, 0.02, generator=torch.Generator(device="cuda").manual_seed(1))     # random weights: the reference's init zeroes
dit.refresh_shadow(force=True)                                                            # the adaLN and output layers
model = LatentDiffusion(dit, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=dit.input_size)
model.eval()
eng = dit.engine
n_eval = 2 * args.steps - 1


def run(lat, y, cached, steps=args.steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = model.edm_sampler_loop(lat, y, steps=steps, cfg=args.guidance, cond_cache=cached)
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def run_solver(lat, y, cached, sampler, interval):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = model.edm_sampler_loop(lat, y, steps=args.steps, cfg=args.guidance, cond_cache=cached, sampler=sampler, guidance_interval=interval)
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def evaluation_counts(sampler, interval):
    ec = model.edm_config
    levels = samplers.evaluation_sigmas(sampler, samplers.edm_schedule(args.steps, ec.sigma_min, ec.sigma_max, ec.rho))
    guided = sum(samplers.is_guided(s, args.guidance, interval) for s in levels)
    return {"evaluations": len(levels), "guided_evaluations": guided, "network_samples_per_image": len(levels) + guided}


def bench_solvers(lat, y, B):
    """{variant: {...}} for every (solver, interval) other than the default run, each alternating with the default Heun run."""
    interval = samplers.guidance_interval_bounds(args.guidance_interval)
    out = {}
    for sampler in args.sampler:
        if sampler == "heun" and interval is None:
            continue                                # the default run itself
        for cached in args.solver_cache:
            cached = bool(cached)
            run_solver(lat, y, cached, "heun", None)            # warm-up of both at this shape
            res_s, _ = run_solver(lat, y, cached, sampler, interval)
            tb, ts = [], []
            for _ in range(args.repeats):
                tb.append(run_solver(lat, y, cached, "heun", None)[1])
                ts.append(run_solver(lat, y, cached, sampler, interval)[1])
            mb, ms = statistics.median(tb), statistics.median(ts)
            key = sampler + ("" if interval is None else f"[{interval[0]:g},{interval[1]:g}]") + ("/cached" if cached else "/uncached")
            out[key] = {"sampler": sampler, "guidance_interval": interval, "cond_cache": cached, "finite": bool(torch.isfinite(res_s).all()),
                        "heun_ms": tb, "solver_ms": ts, "heun_median_ms": mb, "solver_median_ms": ms, "solver_ms_per_image": ms / B,
                        "solver_over_heun": ms / mb, "heun_noise_floor_rel": (max(tb) - min(tb)) / mb,
                        "heun_counts": evaluation_counts("heun", None), "solver_counts": evaluation_counts(sampler, interval)}
            print(f"B={B:3d}  {key:34s} {ms:9.1f} ms  default heun {mb:9.1f} ms  ratio {ms / mb:.4f}  "
                  f"evaluations {out[key]['solver_counts']['evaluations']} vs {out[key]['heun_counts']['evaluations']}", flush=True)
    return out


def count_launches(lat, y, cached):
    """(C-ABI calls per evaluation, one-off calls per run)."""
    real = hip.lib()
    proxy = _CountingLib(real)
    hip._lib, eng.L = proxy, proxy
    try:
        n = []
        for steps in (2, 3):                    # 3 and 5 evaluations
            proxy.calls = 0
            run(lat, y, cached, steps)
            n.append(proxy.calls)
    finally:
        hip._lib, eng.L = real, real
    per_eval = (n[1] - n[0]) // 2
    assert (n[1] - n[0]) % 2 == 0
    return per_eval, n[0] - 3 * per_eval


res = {"device": torch.cuda.get_device_name(0), "arch": args.arch, "steps": args.steps, "evaluations": n_eval, "guidance": args.guidance,
       "repeats": args.repeats, "timing": "device events around edm_sampler_loop, one run each, cached / uncached alternating", "sizes": {}}
ok = True
for B in args.sizes:
    g = torch.Generator(device="cuda").manual_seed(100 + B)
    lat = torch.randn(B, dit.in_channels, dit.input_size, dit.input_size, device="cuda", generator=g)
    y = torch.randn(B, 1, 77, dit.config.caption_channels, device="cuda", generator=g)
    ref, _ = run(lat, y, False)                 # warm-up of both paths at this shape (code objects, allocator) + the bit comparison
    out, _ = run(lat, y, True)
    same = bool(torch.equal(ref, out))
    tu, tc = [], []
    for _ in range(args.repeats):
        tu.append(run(lat, y, False)[1])
        tc.append(run(lat, y, True)[1])
    lu, lc = count_launches(lat, y, False), count_launches(lat, y, True)
    Bn = 2 * B if args.guidance > 1.0 else B
    cond = dit.encode_condition(torch.cat([y, torch.zeros_like(y)], 0) if args.guidance > 1.0 else y)
    mu, mc = statistics.median(tu), statistics.median(tc)
    noise = max(tu) - min(tu)
    r = {"network_batch": Bn, "bit_identical": same,
         "uncached_ms": tu, "cached_ms": tc, "uncached_median_ms": mu, "cached_median_ms": mc,
         "uncached_ms_per_image": mu / B, "cached_ms_per_image": mc / B,
         "noise_floor_ms": noise, "noise_floor_rel": noise / mu, "cached_over_uncached": mc / mu,
         "cached_not_slower_than_noise": bool(mc <= mu + noise),
         "launches_per_evaluation": {"uncached": lu[0], "cached": lc[0]}, "one_off_launches": {"uncached": lu[1], "cached": lc[1]},
         "conditioning_nbytes": cond.nbytes}
    del cond
    solvers = bench_solvers(lat, y, B)
    if solvers:
        r["solvers"] = solvers
    ok = ok and same and r["cached_not_slower_than_noise"]
    res["sizes"][str(B)] = r
    print(f"B={B:3d}  uncached {mu:9.1f} ms  cached {mc:9.1f} ms  ratio {mc / mu:.4f}  noise {noise / mu:.4f}  launches/eval {lu[0]} -> {lc[0]}  "
          f"cond {r['conditioning_nbytes'] / 2**20:.1f} MiB  identical {same}", flush=True)
res["pass"] = bool(ok)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"out": args.out, "pass": res["pass"]}))
sys.exit(0 if ok else 1)
