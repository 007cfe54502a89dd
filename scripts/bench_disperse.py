"""Cost of the dispersive loss on an MI355X:
  * its launches alone at one bench.py microbatch (B = 1024 samples, Tk = 64 kept tokens, dim = 1024: Z is 1024 x 65,536 bf16): the Gram
    (split-K GEMM + md_splitk_reduce), md_disperse_pairs and the injection GEMM, each timed in groups of launches between two events, with
    the kernel the GEMM family chose for each product (engine.gemm_log) -- the launch to look at when the step ratio is above the estimate
    of 2 B^2 Tk dim flops per product;
  * the full optimisation step at the bench.py shape (bench.Stage, res_256_pretrain, XL/2, 2048 images in 1024-image microbatches) with the
    term on (weight 0.5, tau 0.5, block depth // 4) against the same step with it off: same process, same model, same box, rounds in
    alternating order.  With the switch off the step issues the launches of the parent commit.  The on / off ratio is recorded next to the
    spread of the off rounds.
`--parent-bench FILE` / `--head-bench FILE`: files holding the JSON result line bench.py printed at the parent commit and at this one in
the same session; their ms / step are recorded next to the two sides.
Writes a JSON file (default profiles/disperse.json).
Usage: python scripts/bench_disperse.py [--steps 3] [--rounds 3] [--microbatch 1024] [--skip-step] [--parent-bench FILE] [--head-bench FILE]
       [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import hip  # noqa: E402
from micro_diffusion_amd.disperse import DisperseLoss  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--groups", type=int, default=10)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--microbatch", type=int, default=1024)
ap.add_argument("--skip-step", action="store_true", help="only the launches alone")
ap.add_argument("--parent-bench", default=None)
ap.add_argument("--head-bench", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disperse.json"))
args = ap.parse_args()

torch.cuda.set_device(0)
dev = torch.device("cuda")
out = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "launches_alone": {}}

st = bench.Stage("res_256_pretrain", "MicroDiT_XL_2", 2048, args.microbatch, 1, 0)
tr, model = st.trainer, st.model
eng = model.dit.engine
names = {v: k for k, v in hip.GEMM_VARIANT_NAMES.items()}

# ---- the three launches alone, on buffers of their own (nothing of the step is alive yet)
B = args.microbatch
Tk = int(eng.cfg.tokens * (1 - model.train_mask_ratio)) if model.train_mask_ratio > 0 else eng.cfg.tokens
K = Tk * eng.cfg.dim
ld = (B + 7) // 8 * 8
z = (0.7 * torch.randn(B, K, device=dev)).to(torch.bfloat16)
dx = (1e-3 * torch.randn(B, K, device=dev)).to(torch.bfloat16)
G = torch.empty(B, ld, device=dev, dtype=torch.float32)
W = torch.empty(B, ld, device=dev, dtype=torch.bfloat16)
res = torch.zeros(4, device=dev, dtype=torch.float64)
tau, coef = 0.5, 4.0 * 0.5 * 0.5 / (0.5 * K)
PER = 10
launches = (("gram", lambda: eng.disperse_gram(z, B, K, G, ld), 2.0 * B * B * K),
            ("md_disperse_pairs", lambda: eng.disperse_pairs(G, ld, B, K, tau, coef, W, ld, res), 0.0),
            ("injection", lambda: eng.disperse_apply(W, ld, z, dx, B, K), 2.0 * B * B * K))
for name, fn, flops in launches:
    eng.gemm_log, eng.disperse_log = [], []
    fn()
    torch.cuda.synchronize()
    chosen, path = [names[g[0]] for g in eng.gemm_log], [p[1] for p in eng.disperse_log]
    eng.gemm_log = eng.disperse_log = None
    times = []
    for i in range(args.groups + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(PER):
            fn()
        e1.record()
        e1.synchronize()
        if i >= 2:
            times.append(1e3 * e0.elapsed_time(e1) / PER)
    med = statistics.median(times)
    out["launches_alone"][name] = {"B": B, "K": K, "median_us_per_call": med, "min_us": min(times), "max_us": max(times),
                                   "launches_per_group": PER, "groups": len(times), "gemm_variant": chosen, "path": path,
                                   **({"tflops": flops / med / 1e6} if flops else {})}
    print(name, json.dumps(out["launches_alone"][name]), flush=True)
out["disperse_result_block"] = dict(zip(("loss", "mean_dist", "mean_offdiag_p_b2", "S"), res.tolist()))
out["estimate_ms_per_microbatch"] = {"flops_per_product": 2.0 * B * B * K, "at_0.47_of_2.5_pflops_ms": 2 * 2.0 * B * B * K / (0.47 * 2.5e15) * 1e3}
del z, dx, G, W

if not args.skip_step:
    dl = DisperseLoss(weight=0.5, tau=0.5, block=None)
    dl.resolve_block(len(eng.backbone))
    sides = {"off": [], "on": []}
    for rnd in range(args.rounds):
        for name in (("off", "on") if rnd % 2 == 0 else ("on", "off")):
            tr.disperse = model.disperse = dl if name == "on" else None      # the switch train_step and train_microbatch look at
            if name == "on" and not sides["on"]:
                # the armed state is a new shape key of the tape arena: its first pass measures with plain allocations, and at this shape
                # they do not fit next to the unarmed key's 156 GB buffer (a run that starts armed never holds both)
                eng._tape_arena.buf = None
                torch.cuda.empty_cache()
            e, loss = st.timed(args.steps, 1, 1)
            sides[name].append(1e3 * e / args.steps)
            stats = tr.disperse_stats() if name == "on" else None
            print(f"{name:4s} round {rnd}: {1e3 * e / args.steps:8.2f} ms / step  loss {loss:.5f}  {stats}", flush=True)
    off, on = statistics.median(sides["off"]), statistics.median(sides["on"])
    out["full_step"] = {"stage": "res_256_pretrain", "global_batch": 2048, "microbatch": args.microbatch, "steps_per_round": args.steps,
                        "block": dl.resolve_block(len(eng.backbone)), "weight": dl.weight, "tau": dl.tau,
                        "ms_per_step": sides, "median_off_ms": off, "median_on_ms": on, "overhead_ms": on - off, "on_over_off": on / off,
                        "off_spread_ms": max(sides["off"]) - min(sides["off"]), "off_spread_frac": (max(sides["off"]) - min(sides["off"])) / off,
                        "last_disperse_stats": tr.disperse_stats() if tr.disperse is not None else stats}
    for key, path in (("parent_commit_bench", args.parent_bench), ("this_commit_bench", args.head_bench)):
        if path:
            with open(path) as fh:
                line = [ln for ln in fh.read().splitlines() if ln.startswith("{")][-1]
            pb = json.loads(line)
            out[key] = {k: pb[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup") if k in pb}
    print("full step", json.dumps(out["full_step"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
