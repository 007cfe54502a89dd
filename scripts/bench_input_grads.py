"""Cost of the input-gradient backward on an MI355X, XL/2 at the 256-px geometry (32 x 32 latents, 256 tokens, caption
length 77, no masking), B = 64 and B = 256:
  * forward + full backward (parameters require grad, no input does: the path the package had before) against forward + dgrad-only
    backward with dx (parameters frozen, x requires grad), through DiT.forward_without_cfg and autograd: same process, same module,
    rounds in alternating order, each round a group of passes between two device events;
  * md_patch_embed_dgrad alone at the same two shapes: time per call, the bytes of dtok it reads and the achieved fraction of the
    8 TB/s HBM3E peak (the read of dtok is the roofline: DESIGN.md 4.17).
No threshold is set anywhere: the numbers are recorded as measured.
`--parent-bench FILE` / `--head-bench FILE`: files holding the JSON result line bench.py printed at the parent commit and at this one in
the same session; their headline is recorded next to the measurements.
Writes a JSON file (default profiles/input_grads.json).
Usage: python scripts/bench_input_grads.py [--batches 64,256] [--passes 5] [--rounds 3] [--parent-bench FILE] [--head-bench FILE] [--out FILE]"""
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
from micro_diffusion_amd import dit as mdit  # noqa: E402

HBM_PEAK_TBS = 8.0

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,256")
ap.add_argument("--passes", type=int, default=5, help="forward + backward passes per timed group")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--kernel-groups", type=int, default=10)
ap.add_argument("--parent-bench", default=None)
ap.add_argument("--head-bench", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_grads.json"))
args = ap.parse_args()

torch.cuda.set_device(0)
dev = torch.device("cuda")
out = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "model": "MicroDiT_XL_2",
       "geometry": {"latent": 32, "tokens": 256, "caption_len": 77, "mask_ratio": 0.0}, "hbm_peak_tbs": HBM_PEAK_TBS, "kernel_alone": {},
       "forward_backward": {}}
L = hip.lib()
st = torch.cuda.current_stream().cuda_stream


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n          # ms per call


# ---- md_patch_embed_dgrad alone
PER = 20
for B in (int(b) for b in args.batches.split(",")):
    M, D, C, H, p = B * 256, 1024, 4, 32, 2
    dtok = torch.randn(M, D, device=dev).to(torch.bfloat16)
    w = (0.25 * torch.randn(D, C * p * p, device=dev)).to(torch.bfloat16)
    scale = torch.rand(B, device=dev) + 0.5
    dx = torch.empty(B, C, H, H, device=dev)
    path = ctypes.c_int32(-1)

    def call():
        hip.check(L.md_patch_embed_dgrad(dtok.data_ptr(), D, w.data_ptr(), scale.data_ptr(), dx.data_ptr(), B, C, H, H, p, D, ctypes.byref(path),
                                         st), "md_patch_embed_dgrad")
    timed(call, 3)
    times = [1e3 * timed(call, PER) for _ in range(args.kernel_groups)]
    med = statistics.median(times)
    nbytes = 2.0 * M * D
    out["kernel_alone"][f"B{B}"] = {"rows": M, "D": D, "patch_vec": C * p * p, "path": "mfma" if path.value == 1 else "fma",
                                    "dtok_bytes": nbytes, "dx_bytes": 4.0 * B * C * H * H, "median_us_per_call": med, "min_us": min(times),
                                    "max_us": max(times), "launches_per_group": PER, "groups": len(times), "dtok_tbs": nbytes / med / 1e6,
                                    "frac_of_hbm_peak": nbytes / med / 1e6 / HBM_PEAK_TBS, "roofline_us_at_hbm_peak": nbytes / HBM_PEAK_TBS / 1e6}
    print("md_patch_embed_dgrad", B, json.dumps(out["kernel_alone"][f"B{B}"]), flush=True)
    del dtok, w, dx

# ---- forward + backward through the autograd surface
net = mdit.MicroDiT_XL_2().to(dev)
net.train()
eng = net.engine
for B in (int(b) for b in args.batches.split(",")):
    g = torch.Generator(device="cpu").manual_seed(B)
    x = torch.randn(B, 4, 32, 32, generator=g).to(dev)
    t = (torch.rand(B, generator=g) * 3.2 - 2.0).to(dev)
    y = torch.randn(B, 1, 77, 1024, generator=g).half().to(dev)
    cot = torch.randn(B, 4, 32, 32, generator=g).to(dev)

    def full():
        (net.forward_without_cfg(x, t, y)["sample"] * cot).sum().backward()

    def dgrad_only():
        xs = x.detach().requires_grad_(True)
        (net.forward_without_cfg(xs, t, y)["sample"] * cot).sum().backward()

    def forward_only():
        with torch.no_grad():
            net.forward_without_cfg(x, t, y)

    sides = {"full": [], "dgrad_only_dx": [], "forward_only": []}
    counts = {}
    for name, fn, frozen in (("full", full, False), ("dgrad_only_dx", dgrad_only, True)):
        net.requires_grad_(not frozen)
        eng.gemm_log = []
        fn()
        torch.cuda.synchronize()
        counts[name], eng.gemm_log = len(eng.gemm_log), None
        timed(fn, 2)
    for rnd in range(args.rounds):
        order = (("full", full, False), ("dgrad_only_dx", dgrad_only, True), ("forward_only", forward_only, True))
        for name, fn, frozen in (order if rnd % 2 == 0 else order[::-1]):
            net.requires_grad_(not frozen)
            sides[name].append(timed(fn, args.passes))
    net.requires_grad_(True)
    med = {k: statistics.median(v) for k, v in sides.items()}
    out["forward_backward"][f"B{B}"] = {
        "ms_per_pass": sides, "median_ms": med, "passes_per_group": args.passes, "gemm_launches_per_pass": counts,
        "backward_ms_full": med["full"] - med["forward_only"], "backward_ms_dgrad_only_dx": med["dgrad_only_dx"] - med["forward_only"],
        "dgrad_only_over_full": med["dgrad_only_dx"] / med["full"],
        "backward_dgrad_only_over_full": (med["dgrad_only_dx"] - med["forward_only"]) / (med["full"] - med["forward_only"]),
        "full_spread_frac": (max(sides["full"]) - min(sides["full"])) / med["full"]}
    print("forward + backward", B, json.dumps(out["forward_backward"][f"B{B}"]), flush=True)

for key, path_ in (("parent_commit_bench", args.parent_bench), ("this_commit_bench", args.head_bench)):
    if path_:
        with open(path_) as fh:
            line = [ln for ln in fh.read().splitlines() if ln.startswith("{")][-1]
        pb = json.loads(line)
        out[key] = {k: pb[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup") if k in pb}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
