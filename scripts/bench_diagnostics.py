"""Cost of the model diagnostics at the routing shapes of one MicroDiT_XL_2 microbatch (synthetic tapes, no model):
every routed layer's md_moe_route on random logits -- the existing work over the same tensors -- with the diagnostics OFF, against the
same launches plus one md_moe_route_stats per routed layer and one md_loss_sigma_hist with them ON (what a monitored microbatch
adds).  Patch-mixer layers route all T tokens of a sample, backbone layers the tokens kept by the mask.
Device events around each side, ON and OFF alternating inside one loop (same thermal / clock state), warm-up first; medians, the
min .. max spread and the difference go to a JSON file (default profiles/diagnostics.json).
Usage: python scripts/bench_diagnostics.py [--microbatch 256] [--mask-ratio 0.75] [--repeats 30] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import hip  # noqa: E402
from micro_diffusion_amd.arch import DiTConfig, plan_blocks  # noqa: E402
from micro_diffusion_amd.diagnostics import LossBySigma, RouteStats  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--microbatch", type=int, default=256)
ap.add_argument("--mask-ratio", type=float, default=0.75)
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--bins", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnostics.json"))
args = ap.parse_args()
assert args.repeats >= 20, "at least 20 repeats per side"

L, st, dev = hip.lib(), hip.stream_ptr(), torch.device("cuda")
cfg = DiTConfig()                                                       # defaults = MicroDiT_XL_2
mixer, backbone = plan_blocks(cfg)
B, E = args.microbatch, cfg.num_experts
ldl = 8 if E <= 8 else 16
Tk = int(cfg.tokens * (1 - args.mask_ratio))
rs = RouteStats(SimpleNamespace(mixer=mixer, backbone=backbone, cfg=cfg, dev=dev))
lbs = LossBySigma(args.bins)


def tape(S):
    """slot / probs / gval of one routed layer over B samples of S tokens, from the real md_moe_route on random logits."""
    k = int(cfg.expert_capacity * S / E)
    t = SimpleNamespace(S=S, k=k, logits=torch.randn(B * S, ldl, device=dev), probs=torch.empty(B * S, ldl, device=dev),
                        rowidx=torch.empty(E, B * k, device=dev, dtype=torch.int32), gval=torch.empty(E, B * k, device=dev),
                        slot=torch.empty(B * S, E, device=dev, dtype=torch.int32))
    t.bytes = t.slot.numel() * 4 + B * S * E * 4 + t.gval.numel() * 4   # what md_moe_route_stats reads
    return t


tapes = {S: tape(S) for S in {cfg.tokens, Tk}}
layers = [(bp.name, tapes[cfg.tokens]) for bp in mixer if bp.moe] + [(bp.name, tapes[Tk]) for bp in backbone if bp.moe]
sigma = torch.exp(torch.randn(B, device=dev) * 1.2 - 0.6)
lps = torch.rand(B, device=dev)


def route(t):
    hip.check(L.md_moe_route(t.logits.data_ptr(), t.probs.data_ptr(), ldl, B, t.S, E, t.k, t.rowidx.data_ptr(), t.gval.data_ptr(),
                             t.slot.data_ptr(), st), "md_moe_route")


def off():
    for _, t in layers:
        route(t)


def on():
    for name, t in layers:
        route(t)
        rs.record(name, t.slot, t.probs, ldl, t.gval, B, t.S, t.k)
    lbs.accumulate(sigma, lps, True)


for _ in range(args.warmup):
    on()
    off()
torch.cuda.synchronize()
t_on, t_off = [], []
for _ in range(args.repeats):
    for fn, acc in ((on, t_on), (off, t_off)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        acc.append(e0.elapsed_time(e1))


def summary(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "repeats": len(t)}


out = {"layout": "MicroDiT_XL_2 routing shapes, one microbatch", "microbatch": B, "mask_ratio": args.mask_ratio, "experts": E,
       "routed_layers": len(layers), "device": torch.cuda.get_device_name(0),
       "tokens_per_layer": {n: B * t.S for n, t in layers}, "stats_bytes_per_layer": {n: t.bytes for n, t in layers},
       "launches_added": {"md_moe_route_stats calls (partial + finish kernel each)": len(layers), "md_loss_sigma_hist": 1},
       "on": summary(t_on), "off": summary(t_off),
       "added_ms_median": statistics.median(t_on) - statistics.median(t_off),
       "added_us_per_routed_layer": 1e3 * (statistics.median(t_on) - statistics.median(t_off)) / len(layers)}
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
