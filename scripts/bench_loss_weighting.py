"""Cost of the learned loss weighting on an MI355X:
  * the two new kernels alone at one bench.py microbatch (B = 1024 samples, C = 128): device time per launch, timed in groups of 100
    launches between two events (a single launch is shorter than an event pair resolves);
  * the full optimisation step at the bench.py shape (bench.Stage, res_256_pretrain, XL/2, 2048 images in 1024-image microbatches) with the
    switch on against the same step with it off: same process, same model, same box, rounds in alternating order as
    scripts/bench_posthoc_ema.py does.  With the switch off the step issues the launches of the parent commit.
`--parent-bench FILE`: a file holding the JSON result line bench.py printed at the parent commit on the same box; its ms / step is
recorded next to the two sides.
Writes a JSON file (default profiles/loss_weighting.json).
Usage: python scripts/bench_loss_weighting.py [--steps 3] [--rounds 2] [--microbatch 1024] [--skip-step] [--parent-bench FILE] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd.loss_weighting import LossWeighting  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--groups", type=int, default=20)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--microbatch", type=int, default=1024)
ap.add_argument("--channels", type=int, default=128)
ap.add_argument("--skip-step", action="store_true", help="only the kernels alone")
ap.add_argument("--parent-bench", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_weighting.json"))
args = ap.parse_args()

torch.cuda.set_device(0)
dev = torch.device("cuda")
out = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "channels": args.channels,
       "kernels_alone": {}}

B, PER = args.microbatch, 100
lw = LossWeighting(channels=args.channels, device=dev)
lw.w.normal_(0, 0.1)
c = 0.3 * torch.randn(B, device=dev)
L = torch.exp(-2 * c + 0.5)


def pair():
    lw.forward(c)
    lw.backward(c, L, 1.0)


for name, fn in (("md_logvar_fwd", lambda: lw.forward(c)), ("fwd_plus_bwd", pair)):
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
    out["kernels_alone"][name] = {"B": B, "median_us_per_call": statistics.median(times), "min_us": min(times), "max_us": max(times),
                                  "launches_per_group": PER, "groups": len(times), "note": "back-to-back launches from Python: launch-bound"}
    print(name, json.dumps(out["kernels_alone"][name]), flush=True)
lw.g.zero_()

if not args.skip_step:
    st = bench.Stage("res_256_pretrain", "MicroDiT_XL_2", 2048, args.microbatch, 1, 0)
    tr = st.trainer
    lw = LossWeighting(channels=args.channels, device=dev)
    res = {"off": [], "on": []}
    for rnd in range(args.rounds):
        for name in (("off", "on") if rnd % 2 == 0 else ("on", "off")):
            tr.loss_weighting = st.model.loss_weighting = lw if name == "on" else None      # the switch train_step and _edm_forward look at
            tr._objective = None
            e, loss = st.timed(args.steps, 1, 1)
            res[name].append(1e3 * e / args.steps)
            print(f"{name:4s} round {rnd}: {1e3 * e / args.steps:8.2f} ms / step  loss {loss:.5f}", flush=True)
    off, on = statistics.median(res["off"]), statistics.median(res["on"])
    out["full_step"] = {"stage": "res_256_pretrain", "global_batch": 2048, "microbatch": args.microbatch, "steps_per_round": args.steps,
                        "ms_per_step": res, "median_off_ms": off, "median_on_ms": on, "overhead_ms": on - off, "overhead_frac": (on - off) / off,
                        "w_moved": bool(lw.w.any())}
    if args.parent_bench:
        with open(args.parent_bench) as fh:
            line = [ln for ln in fh.read().splitlines() if ln.startswith("{")][-1]
        pb = json.loads(line)
        out["parent_commit_bench"] = {k: pb[k] for k in ("value", "unit", "ms_per_step") if k in pb}
    print("full step", json.dumps(out["full_step"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
