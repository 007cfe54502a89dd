"""Cost of the training-health kernels on the MicroDiT_XL_2 flat layout (synthetic buffers, no model):
  * md_tensor_stats_partial + _finish over the fp32 / bf16 gradient buffer  vs  md_sumsq + md_sumsq_finish over the same buffer
    (the existing kernel that reads the same bytes once);
  * md_adamw_step_guarded with the go flag at 1  vs  md_adamw_step.
Device events around every single call, A and B alternating inside one loop (same thermal / clock state), warm-up first; medians and
the min .. max spread of each side go to a JSON file (default profiles/optimizer_monitor.json).
Usage: python scripts/bench_monitor.py [--repeats 30] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from micro_diffusion_amd import hip  # noqa: E402
from micro_diffusion_amd.arch import DiTConfig, param_table  # noqa: E402
from micro_diffusion_amd.dit import flat_layout  # noqa: E402
from micro_diffusion_amd.trainer import _StatsPlan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_monitor.json"))
args = ap.parse_args()
assert args.repeats >= 20, "at least 20 repeats per side"

L, st, dev = hip.lib(), hip.stream_ptr(), torch.device("cuda")
table = [s for s in param_table(DiTConfig()) if not s.buffer]          # DiTConfig defaults = MicroDiT_XL_2
offs_by_name, total = flat_layout(table)
table.sort(key=lambda s: offs_by_name[s.name])
offs, numels = [offs_by_name[s.name] for s in table], [int(np.prod(s.shape)) for s in table]


def ab(a, b):
    """Per-call device times (ms) of a() and b(), alternating."""
    for _ in range(args.warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(args.repeats):
        for fn, acc in ((a, ta), (b, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return ta, tb


def summary(t, nbytes):
    med = statistics.median(t)
    return {"median_ms": med, "min_ms": min(t), "max_ms": max(t), "repeats": len(t), "bytes": nbytes, "median_TB_per_s": nbytes / med / 1e9}


out = {"layout": "MicroDiT_XL_2 flat buffers", "tensors": len(offs), "elements": total, "device": torch.cuda.get_device_name(0)}
partials = torch.zeros(hip.SUMSQ_PARTIALS, device=dev)
ss = torch.zeros(1, device=dev)
for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
    g = (torch.randn(total, device=dev) * 1e-3).to(dtype)
    plan = _StatsPlan(offs, numels, [(g, [(0, total, 0)])], dev)

    def sumsq():
        hip.check(L.md_sumsq(g.data_ptr(), 1 if dtype == torch.bfloat16 else 0, total, partials.data_ptr(), st), "md_sumsq")
        hip.check(L.md_sumsq_finish(partials.data_ptr(), hip.SUMSQ_PARTIALS, ss.data_ptr(), st), "md_sumsq_finish")
    ta, tb = ab(plan.run, sumsq)
    # same data, two kernels: the per-tensor sums must add up to the whole-buffer sum (padding is zero here)
    rel = abs(float(plan.out_f[0].double().sum()) - float(ss)) / float(ss)
    nbytes = total * g.element_size()
    out["stats_" + name] = {"tensor_stats": summary(ta, nbytes), "md_sumsq": summary(tb, nbytes), "items": int(plan.items.shape[0]),
                            "ratio_stats_over_sumsq": statistics.median(ta) / statistics.median(tb), "sumsq_rel_diff": rel}
    print(name, json.dumps(out["stats_" + name]), flush=True)
    del g, plan

p, m, v = torch.randn(total, device=dev) * 0.02, torch.zeros(total, device=dev), torch.zeros(total, device=dev)
g = torch.randn(total, device=dev) * 1e-3
s = torch.zeros(total, device=dev, dtype=torch.bfloat16)
go = torch.tensor([1, 0, 0, 0], device=dev, dtype=torch.int32)
a = hip.AdamWArgs(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), s.data_ptr(), None, None, None, total, 2.4e-4, 0.9, 0.999, 1e-8,
                  0.1, 1 - 0.9 ** 10, 1 - 0.999 ** 10, 0.0, 1.0, 0.0, 0, 0)       # zero_grad 0: every repeat sees the same gradient
ta, tb = ab(lambda: hip.check(L.md_adamw_step_guarded(ctypes.byref(a), go.data_ptr(), st), "guarded"),
            lambda: hip.check(L.md_adamw_step(ctypes.byref(a), st), "unguarded"))
nbytes = total * (4 * 7 + 2)          # p, m, v read + write, g read, bf16 shadow write
out["adamw"] = {"guarded_flag_1": summary(ta, nbytes), "md_adamw_step": summary(tb, nbytes),
                "ratio_guarded_over_unguarded": statistics.median(ta) / statistics.median(tb)}
print("adamw", json.dumps(out["adamw"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
