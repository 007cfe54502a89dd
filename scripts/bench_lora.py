"""Cost of LoRA training on an MI355X, MicroDiT_XL_2, default targets, rank 16, one GPU, one process:
  * LoRAAdamW.step alone and split into its four passes -- projection (md_lora_grad), clear of the accumulator (md_fill_zero), norm +
    AdamW on the adapter (md_sumsq, md_sumsq_finish, md_adamw_step), merge (md_lora_merge) -- device events around each, on a synthetic
    gradient of the size of the flat buffers;
  * FusedAdamW.step (the pass it replaces: norm, clip, AdamW over 1.165 G elements, bf16 emit) on the same buffers;
  * the full optimisation step (bench.Stage, res_256_pretrain, 2048 images) with each optimiser: same process, same model, rounds in
    alternating order (the adapter is detached for the full optimiser's rounds and attached again for its own);
  * bytes each optimiser holds, and the bytes each pass moves by the algorithm (from the shapes).
Writes a JSON file (default profiles/lora.json).
Usage: python scripts/bench_lora.py [--rank 16] [--repeats 20] [--steps 3] [--rounds 2] [--microbatch 256] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import hip, lora  # noqa: E402
from micro_diffusion_amd.trainer import Trainer  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--microbatch", type=int, default=256)
ap.add_argument("--skip-step", action="store_true", help="only the optimiser passes, not the full 2048-image steps")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora.json"))
args = ap.parse_args()

torch.cuda.set_device(0)
st = bench.Stage("res_256_pretrain", "MicroDiT_XL_2", 2048, args.microbatch, 1, 0)
dit = st.model.dit
f = dit.flat_buffers()
full_tr, full = st.trainer, st.trainer.opt
clip = full_tr.clip_norm
ad = lora.LoRA(dit, rank=args.rank, seed=18)
with torch.no_grad():                       # a trained adapter: B is not zero
    for n in ad.names:
        ad.B(n).normal_(0.0, 0.01)
opt = lora.LoRAAdamW(ad, lr=full.lr)         # attaches the adapter
lora_tr = Trainer(st.model, opt, full_tr.schedule, clip_norm=clip, microbatch_size=args.microbatch)
lora_tr.batches_seen = full_tr.batches_seen
targeted = sum(s.shape[0] * s.shape[1] for s in ad.specs)
strips = sum((s.shape[0] + 63) // 64 * s.shape[1] for s in ad.specs) * args.rank
out = {"model": "MicroDiT_XL_2", "rank": args.rank, "targets": len(ad.specs), "device": torch.cuda.get_device_name(0),
       "arch": torch.cuda.get_device_properties(0).gcnArchName, "flat_elements": f["total"], "targeted_elements": targeted,
       "adapter_elements": ad.total,
       "optimizer_bytes": {"FusedAdamW": 4 * (full.m.numel() + full.v.numel() + full.partials.numel() + 1),
                           "LoRAAdamW": 4 * lora.allocated_floats(opt)},
       # what each pass has to move: the projection reads the targeted gradient once and writes + reads its dA slices; the merge reads
       # the targeted masters and writes bf16; FusedAdamW reads g (norm), then reads g, p, m, v and writes g, p, m, v, bf16
       "algorithmic_bytes": {"projection": 4 * targeted + 8 * strips, "clear": 4 * f["total"], "adamw": 4 * ad.total * 8,
                             "merge": 6 * targeted, "FusedAdamW": f["total"] * (4 + 16 + 16 + 2)}}


def timed(fn, prepare=None):
    times = []
    for i in range(args.warmup + args.repeats):
        if prepare is not None:
            prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            times.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "repeats": len(times)}


L = hip.lib()
grad = torch.randn(f["total"], device="cuda") * 1e-3


def fill():
    f["g"].copy_(grad)


def adamw_only():
    stp = hip.stream_ptr()
    hip.check(L.md_sumsq(ad.g.data_ptr(), 0, ad.total, opt.partials.data_ptr(), stp), "md_sumsq")
    hip.check(L.md_sumsq_finish(opt.partials.data_ptr(), hip.SUMSQ_PARTIALS, opt.sumsq.data_ptr(), stp), "md_sumsq_finish")
    a = hip.AdamWArgs(ad.w.data_ptr(), ad.g.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr(), None, opt.sumsq.data_ptr(), None, None, ad.total,
                      1e-5, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, clip, 1.0, 0.0, 1, 0)
    from ctypes import byref
    hip.check(L.md_adamw_step(byref(a), stp), "md_adamw_step")


parts = {"projection": timed(lambda: ad.project_grad(1.0), fill),
         "clear": timed(lambda: hip.check(L.md_fill_zero(f["g"].data_ptr(), 4 * f["total"], hip.stream_ptr()), "md_fill_zero")),
         "adamw": timed(adamw_only, lambda: ad.project_grad(1.0)),
         "merge": timed(ad.apply_to_shadow),
         "LoRAAdamW.step": timed(lambda: opt.step(lr=1e-5, max_norm=clip), fill)}
ad.detach()
parts["FusedAdamW.step"] = timed(lambda: full.step(lr=1e-5, max_norm=clip), fill)
ad.attach()
for k, v in parts.items():
    if k in out["algorithmic_bytes"]:
        v["TB_per_s"] = out["algorithmic_bytes"][k] / v["median_ms"] / 1e9
    print(k, json.dumps(v), flush=True)
out["passes"] = parts
out["optimizer_phase_ratio"] = parts["LoRAAdamW.step"]["median_ms"] / parts["FusedAdamW.step"]["median_ms"]
del grad
torch.cuda.empty_cache()

if not args.skip_step:
    res = {"full": [], "lora": []}
    for rnd in range(args.rounds):
        for name in (("full", "lora") if rnd % 2 == 0 else ("lora", "full")):
            if name == "full":
                ad.detach()
                st.trainer = full_tr
            else:
                ad.attach()
                st.trainer = lora_tr
            e, loss = st.timed(args.steps, 1, 1)
            res[name].append(1e3 * e / args.steps)
            print(f"{name:4s} round {rnd}: {1e3 * e / args.steps:8.2f} ms / step  loss {loss:.5f}", flush=True)
    a, b = statistics.median(res["full"]), statistics.median(res["lora"])
    out["full_step"] = {"stage": "res_256_pretrain", "global_batch": 2048, "microbatch": args.microbatch, "steps_per_round": args.steps,
                        "ms_per_step": res, "median_full_ms": a, "median_lora_ms": b, "lora_over_full": b / a}
    print("full step", json.dumps(out["full_step"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
