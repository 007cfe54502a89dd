"""Cost of the Muon optimiser (muon.Muon) on an MI355X, MicroDiT_XL_2, headline shape (2048 images, microbatch 1024):
  * Muon.step against FusedAdamW.step on the same model and a planted gradient, device events, alternating in one process;
  * the split of the Muon step into momentum, complement AdamW, Newton-Schulz and apply (the same launches, timed one group at a time),
    the Newton-Schulz rate against the counted FLOPs, the GEMM launch count and the workspace;
  * the whole optimisation step (bench.Stage) with Muon against the same step with FusedAdamW, rounds in alternating order;
  * e_gpu / e_emu of the kernel test's Newton-Schulz inputs (tests/muon_ref.py).
Writes a JSON file (default profiles/muon.json).  No convergence or quality claim: there is no dataset behind it.
Usage: python scripts/bench_muon.py [--repeats 10] [--steps 3] [--rounds 2] [--microbatch 1024] [--skip-step] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import hip  # noqa: E402
from micro_diffusion_amd.muon import Muon  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--microbatch", type=int, default=1024)
ap.add_argument("--skip-step", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "muon.json"))
args = ap.parse_args()

torch.cuda.set_device(0)
st = bench.Stage("res_256_pretrain", "MicroDiT_XL_2", 2048, args.microbatch, 1, 0)
dit = st.model.dit
f = dit.flat_buffers()
adamw = st.trainer.opt
muon = Muon(dit, lr=adamw.lr, betas=adamw.betas, eps=adamw.eps, weight_decay=adamw.weight_decay)
host, dev, n = muon._items()
flops = sum(muon.ns_steps * (4 * min(r, c) ** 2 * max(r, c) + 2 * min(r, c) ** 3) for _, r, c, _ in muon.matrices)
out = {"model": "MicroDiT_XL_2", "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
       "tensors": len(muon.specs), "matrices": n, "targeted_parameters": sum(r * c for _, r, c, _ in muon.matrices),
       "complement_runs": len(muon.runs), "workspace_bytes": muon.ws_bytes, "ns_steps": muon.ns_steps, "ns_flop": flops}
gen = torch.Generator(device="cuda").manual_seed(1)
grad = torch.randn(f["total"], device="cuda", generator=gen) * 1e-3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


# ---- the optimiser step alone, alternating
res = {"adamw": [], "muon": []}
for i in range(args.warmup + args.repeats):
    for name, opt in (("adamw", adamw), ("muon", muon)) if i % 2 == 0 else (("muon", muon), ("adamw", adamw)):
        f["g"].copy_(grad)
        t = timed(lambda: opt.step(max_norm=0.25))
        if i >= args.warmup:
            res[name].append(t)
out["step_alone_ms"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "repeats": len(v)} for k, v in res.items()}
out["gemm_launches"] = muon.last_gemm_launches
print("optimiser step alone", json.dumps(out["step_alone_ms"]), "GEMM launches", muon.last_gemm_launches, flush=True)

# ---- the split: the same launches, one group at a time
L, s = hip.lib(), hip.stream_ptr()
a, b, c = muon.ns_coeffs
parts = {"momentum": [], "complement_adamw": [], "newton_schulz": [], "apply": []}
muon.step_count += 1
for i in range(args.warmup + args.repeats):
    f["g"].copy_(grad)
    t = [timed(lambda: hip.check(L.md_muon_momentum(f["g"].data_ptr(), None, muon.m.data_ptr(), dev.data_ptr(), host, n, muon.momentum, 1, 1.0,
                                                    None, 0.0, 1, None, muon._ws.data_ptr(), muon._partials.data_ptr(), muon.norms.data_ptr(), s),
                                 "md_muon_momentum")),
         timed(lambda: [muon._launch(off, cnt, muon.lr, 0.0, 1.0, None, None, f["s"].data_ptr() + 2 * off, 1, 0) for off, cnt in muon.runs]),
         timed(lambda: hip.check(L.md_muon_newton_schulz(host, n, muon.ns_steps, a, b, c, muon._ws.data_ptr(), None, s), "md_muon_newton_schulz")),
         timed(lambda: hip.check(L.md_muon_apply(f["p"].data_ptr(), f["s"].data_ptr(), None, dev.data_ptr(), host, n, muon.lr, muon.weight_decay, 0,
                                                 0.0, None, muon._ws.data_ptr(), s), "md_muon_apply"))]
    if i >= args.warmup:
        for k, v in zip(parts, t):
            parts[k].append(v)
out["split_ms"] = {k: statistics.median(v) for k, v in parts.items()}
out["newton_schulz_tflops"] = flops / out["split_ms"]["newton_schulz"] / 1e9
print("split", json.dumps(out["split_ms"]), "Newton-Schulz TFLOP/s", round(out["newton_schulz_tflops"], 1), flush=True)

# ---- the kernel test's inputs
from tests import muon_ref as ref  # noqa: E402
items, _ = ref.layout()
table = (hip.MuonItem * len(items))(*[hip.MuonItem(o, r, cc, 0, 1.0, 0) for o, r, cc in items])
need = ctypes.c_int64(0)
hip.check(L.md_muon_ws_bytes(table, len(items), ctypes.byref(need)), "md_muon_ws_bytes")
ws = torch.zeros(need.value // 2, dtype=torch.bfloat16)
xs = ref.ns_inputs()
for it, x in zip(table, xs):
    ws[it.ws_off:it.ws_off + x.numel()] = x.reshape(-1)
wsd = ws.cuda()
hip.check(L.md_muon_newton_schulz(table, len(items), 5, a, b, c, wsd.data_ptr(), None, s), "md_muon_newton_schulz")
torch.cuda.synchronize()
got = wsd.cpu()
out["kernel_test_errors"] = []
for it, x in zip(table, xs):
    R = ref.ns_fp64(x)
    O = got[it.ws_off:it.ws_off + x.numel()].view(x.shape)
    out["kernel_test_errors"].append({"shape": list(x.shape), "e_gpu": ref.rel_err(O, R), "e_emu": ref.rel_err(ref.ns_bf16_emulated(x), R)})
print("kernel test", json.dumps(out["kernel_test_errors"]), flush=True)

# ---- the whole step
if not args.skip_step:
    res = {"off": [], "muon": []}
    for rnd in range(args.rounds):
        for name in (("off", "muon") if rnd % 2 == 0 else ("muon", "off")):
            st.trainer.opt = muon if name == "muon" else adamw
            e, loss = st.timed(args.steps, 1, 1)
            res[name].append(1e3 * e / args.steps)
            print(f"{name:5s} round {rnd}: {1e3 * e / args.steps:8.2f} ms / step  loss {loss:.5f}", flush=True)
    st.trainer.opt = adamw
    off, on = statistics.median(res["off"]), statistics.median(res["muon"])
    out["full_step"] = {"stage": "res_256_pretrain", "global_batch": 2048, "microbatch": args.microbatch, "steps_per_round": args.steps,
                        "ms_per_step": res, "median_off_ms": off, "median_muon_ms": on, "ratio": on / off,
                        "spread_off": (max(res["off"]) - min(res["off"])) / off}
    print("full step", json.dumps(out["full_step"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
