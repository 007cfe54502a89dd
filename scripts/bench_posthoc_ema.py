"""Cost of the post-hoc EMA pass (md_ema_power_update) on an MI355X:
  * the pass alone on synthetic buffers of the size of the MicroDiT_XL_2 masters, K = 1, 2, 4 profiles: device time per call and
    algorithmic bandwidth ((4 + 8 K) bytes per parameter: p read once, every profile read and written once);
  * the full optimisation step (bench.Stage, res_256_pretrain, XL/2, 2048 images) with K = 2 profiles against the same step with the
    feature off: same process, same model, same box, rounds in alternating order as scripts/ab_step.py does.
Writes a JSON file (default profiles/posthoc_ema.json).
Usage: python scripts/bench_posthoc_ema.py [--repeats 30] [--steps 3] [--rounds 2] [--microbatch 256] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import hip, posthoc_ema  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--microbatch", type=int, default=256)
ap.add_argument("--skip-step", action="store_true", help="only the pass alone (the model is still built: its flat layout gives the size)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posthoc_ema.json"))
args = ap.parse_args()

torch.cuda.set_device(0)
dev = torch.device("cuda")
st = bench.Stage("res_256_pretrain", "MicroDiT_XL_2", 2048, args.microbatch, 1, 0)
total = st.model.dit.flat_buffers()["total"]
out = {"layout": "MicroDiT_XL_2 flat buffers", "elements": total, "parameters": sum(v.numel() for v in st.model.dit.flat_buffers()["P"].values()),
       "device": torch.cuda.get_device_name(0),
       "arch": torch.cuda.get_device_properties(0).gcnArchName, "pass_alone": {}}

p = torch.randn(total, device=dev) * 0.02
profiles = [torch.zeros(total, device=dev) for _ in range(4)]
for K in (1, 2, 4):
    betas = [posthoc_ema.power_beta(1000, posthoc_ema.sigma_rel_to_gamma(s)) for s in (0.05, 0.10, 0.15, 0.20)[:K]]
    times = []
    for i in range(args.warmup + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.ema_power_update(p, profiles[:K], betas, total)
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            times.append(e0.elapsed_time(e1))
    nbytes = total * (4 + 8 * K)
    med = statistics.median(times)
    out["pass_alone"][f"K{K}"] = {"median_ms": med, "min_ms": min(times), "max_ms": max(times), "repeats": len(times), "bytes": nbytes,
                                  "median_TB_per_s": nbytes / med / 1e9}
    print(f"K {K}", json.dumps(out["pass_alone"][f"K{K}"]), flush=True)
del p, profiles
torch.cuda.empty_cache()

if not args.skip_step:
    opt = st.trainer.opt
    f = st.model.dit.flat_buffers()
    opt.posthoc_sigma_rels = (0.05, 0.10)
    opt.posthoc_gammas = tuple(posthoc_ema.sigma_rel_to_gamma(s) for s in opt.posthoc_sigma_rels)
    bufs = [f["p"].clone() for _ in opt.posthoc_sigma_rels]
    res = {"off": [], "K2": []}
    for rnd in range(args.rounds):
        for name in (("off", "K2") if rnd % 2 == 0 else ("K2", "off")):
            opt.posthoc = bufs if name == "K2" else []            # the only switch FusedAdamW.step() looks at
            e, loss = st.timed(args.steps, 1, 1)
            res[name].append(1e3 * e / args.steps)
            print(f"{name:4s} round {rnd}: {1e3 * e / args.steps:8.2f} ms / step  loss {loss:.5f}", flush=True)
    off, on = statistics.median(res["off"]), statistics.median(res["K2"])
    out["full_step"] = {"stage": "res_256_pretrain", "global_batch": 2048, "microbatch": args.microbatch, "steps_per_round": args.steps,
                        "ms_per_step": res, "median_off_ms": off, "median_K2_ms": on, "overhead_ms": on - off, "overhead_frac": (on - off) / off}
    print("full step", json.dumps(out["full_step"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
