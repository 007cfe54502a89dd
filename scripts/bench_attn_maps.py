"""Cost of recording cross-attention maps (`edm_sampler_loop(..., attn_maps=AttentionMaps())`).

1. md_attn_probs alone at the MicroDiT_XL_2 shapes: B = 64 and 128 samples, S = 256 tokens, Lc = 77 caption positions, hx = 1024
   (16 heads of 64), packed rows as DiTEngine._block_fwd hands them over.  Its time against the HBM floor of its algorithmic bytes --
   q and k read once, out read and written once -- at the 8 TB/s peak.  The launches rotate over operand sets that together exceed the
   256 MB last-level cache, so no launch finds its operands there; every launch is bracketed by device events.
2. The XL/2 sampler (random weights, B = 64, 30 Heun steps = 59 evaluations, guidance 5 = network batch 2B, cond_cache) with every
   block recorded against the plain run: both in one process, alternating rounds after one warm-up run of each, device events around
   edm_sampler_loop.  Reported: the latency ratio next to the spread of the plain rounds, and whether the latents are bit-identical.
Writes profiles/attn_maps.json.
Usage: python scripts/bench_attn_maps.py [--batch 64] [--steps 30] [--guidance 5] [--repeats 3] [--arch MicroDiT_XL_2] [--out FILE]"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import dit as mdit  # noqa: E402
from micro_diffusion_amd import hip  # noqa: E402
from micro_diffusion_amd.attn_maps import AttentionMaps  # noqa: E402
from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub  # noqa: E402

HBM_PEAK_TBS = 8.0

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--repeats", type=int, default=3, help="timed rounds per variant (>= 2: the noise floor is the spread of the plain ones)")
ap.add_argument("--arch", default="MicroDiT_XL_2")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_maps.json"))
args = ap.parse_args()
assert args.repeats >= 2 and args.steps >= 3
assert torch.cuda.is_available(), "bench_attn_maps.py measures on the GPU; there is no CPU path"
L, st = hip.lib(), torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------- 1: the kernel alone
def bench_kernel(B, S=256, Lc=77, hx=1024, hd=64, launches=40):
    H, ldo = hx // hd, (Lc + 3) // 4 * 4
    nbytes = 2 * B * S * hx + 2 * B * Lc * hx + 2 * 4 * B * S * Lc           # q, k read once; out read and written once
    alloc = 2 * B * S * hx + 2 * B * Lc * 2 * hx + 4 * B * S * ldo           # what one operand set occupies (k inside [K | V] rows)
    sets = max(2, math.ceil(2 * (256 << 20) / alloc))                        # twice the last-level cache
    g = torch.Generator(device="cuda").manual_seed(B)
    ops = []
    for _ in range(sets):
        q = torch.randn(B * S, hx, device="cuda", generator=g).to(torch.bfloat16)
        kv = torch.randn(B * Lc, 2 * hx, device="cuda", generator=g).to(torch.bfloat16)
        out = torch.zeros(B * S, ldo, device="cuda")
        a = hip.AttnArgs()
        a.q, a.k, a.B, a.H, a.Sq, a.Skv = q.data_ptr(), kv.data_ptr(), B, H, S, Lc
        a.ldq, a.ldk, a.sq, a.sk, a.scale, a.hd = hx, 2 * hx, S * hx, Lc * 2 * hx, 1.0 / math.sqrt(hd), hd
        ops.append((q, kv, out, a))
    us = []
    for i in range(launches + sets):
        q, kv, out, a = ops[i % sets]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.check(L.md_attn_probs(ctypes.byref(a), out.data_ptr(), ldo, None, st), "md_attn_probs")
        e1.record()
        e1.synchronize()
        if i >= sets:                                                        # the first pass over the sets is the warm-up
            us.append(1e3 * e0.elapsed_time(e1))
    med = statistics.median(us)
    floor_us = nbytes / (HBM_PEAK_TBS * 1e12) * 1e6
    row_sum = float(ops[0][2][:, :Lc].sum(1).mean()) / len(range(0, launches + sets, sets))       # set 0 took that many launches
    r = {"B": B, "S": S, "Lc": Lc, "hx": hx, "hd": hd, "heads": H, "algorithmic_bytes": nbytes, "operand_sets": sets, "launches": launches,
         "median_us": med, "min_us": min(us), "max_us": max(us), "hbm_floor_us": floor_us, "achieved_tbs": nbytes / med / 1e6,
         "frac_of_hbm_floor": floor_us / med, "bound": "hbm (bytes over the 8 TB/s peak; the MFMA work, 2 * B * H * S * Lc * hd flop, is far below)",
         "mean_row_sum_per_launch": row_sum}
    print(f"md_attn_probs B={B}: median {med:.1f} us (min {min(us):.1f}), HBM floor {floor_us:.1f} us -> {100 * floor_us / med:.1f} % of it, "
          f"{r['achieved_tbs']:.2f} TB/s", flush=True)
    return r


kernel = [bench_kernel(64), bench_kernel(128)]
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------- 2: the sampler
torch.manual_seed(0)
dit = getattr(mdit, args.arch)().to("cuda")
flat = dit.flat_buffers()
flat["p"].normal_(0.0, 0.02, generator=torch.Generator(device="cuda").manual_seed(1))     # random weights: the reference's init zeroes
dit.refresh_shadow(force=True)                                                            # the adaLN and output layers
model = LatentDiffusion(dit, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=dit.input_size)
model.eval()
B = args.batch
g = torch.Generator(device="cuda").manual_seed(100 + B)
lat = torch.randn(B, dit.in_channels, dit.input_size, dit.input_size, device="cuda", generator=g)
y = torch.randn(B, 1, 77, dit.config.caption_channels, device="cuda", generator=g)
am = AttentionMaps()


def run(recorder):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = model.edm_sampler_loop(lat, y, steps=args.steps, cfg=args.guidance, cond_cache=True, attn_maps=recorder)
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


variants = {"plain": None, "recorded": am}
final = {k: run(v)[0] for k, v in variants.items()}                    # warm-up of both + the results that are compared
ms = {k: [] for k in variants}
for _ in range(args.repeats):
    for k, v in variants.items():
        ms[k].append(run(v)[1])
med_ms = {k: statistics.median(v) for k, v in ms.items()}
mass = am.token_mass()
n_blocks, evals = len(am.names), max(am.counts.values())
sampler = {"arch": args.arch, "batch": B, "network_batch": 2 * B if args.guidance > 1.0 else B, "steps": args.steps, "sampler": "heun",
           "guidance": args.guidance, "cond_cache": True, "repeats": args.repeats, "blocks_recorded": n_blocks, "evaluations": evals,
           "probe_launches_per_run": sum(am.counts.values()), "buffer_bytes": am.buf.numel() * 4,
           "timing": "device events around edm_sampler_loop, plain and recorded alternating after one warm-up run of each",
           "ms": ms, "median_ms": med_ms, "ratio_recorded_to_plain": med_ms["recorded"] / med_ms["plain"],
           "plain_spread_rel": (max(ms["plain"]) - min(ms["plain"])) / med_ms["plain"],
           "added_us_per_probe_launch": 1e3 * (med_ms["recorded"] - med_ms["plain"]) / sum(am.counts.values()),
           "latents_bit_identical_to_plain": bool(torch.equal(final["plain"], final["recorded"])),
           "token_mass_row_sums": {"min": float(mass.sum(1).min()), "max": float(mass.sum(1).max())}}
print(f"sampler: plain {med_ms['plain']:.1f} ms, recorded {med_ms['recorded']:.1f} ms, ratio {sampler['ratio_recorded_to_plain']:.4f} "
      f"(plain spread {sampler['plain_spread_rel']:.4f}), {sampler['probe_launches_per_run']} probe launches, "
      f"bit-identical latents: {sampler['latents_bit_identical_to_plain']}", flush=True)

res = {"device": torch.cuda.get_device_name(0), "hbm_peak_tbs": HBM_PEAK_TBS, "kernel": kernel, "sampler": sampler}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"out": args.out, "ratio_recorded_to_plain": sampler["ratio_recorded_to_plain"], "plain_spread_rel": sampler["plain_spread_rel"]}))
