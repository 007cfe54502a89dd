"""Cost of prompt control (`edm_sampler_loop(..., caption_weights=, negative=)`).

1. md_attn_fwd_kbias against md_attn_fwd at the MicroDiT_XL_2 cross-attention shapes: B = 64 and 128 samples, 16 heads of 64, Sq = 256
   tokens, Skv = 77 caption positions, packed rows as DiTEngine._block_fwd hands them over.  Both in one process, alternating launch by
   launch over operand sets that together exceed the 256 MB last-level cache, every launch bracketed by device events.  The yardstick
   is the plain md_attn_fwd of the same session; the spread of its launches (interquartile range over the median) is the noise.
2. The XL/2 sampler (random weights, B = 64, 30 Heun steps = 59 evaluations, guidance 5 = network batch 2B, cond_cache): plain rounds
   against rounds with caption_weights and a negative prompt, alternating after one warm-up run of each, device events around
   edm_sampler_loop.  The spread of the plain rounds is the noise.
No ratio is fixed in advance.  Writes profiles/prompt_control.json.
Usage: python scripts/bench_prompt_control.py [--batch 64] [--steps 30] [--guidance 5] [--repeats 3] [--arch MicroDiT_XL_2] [--out FILE]"""
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
from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--repeats", type=int, default=3, help="timed rounds per variant (>= 2: the noise floor is the spread of the plain ones)")
ap.add_argument("--arch", default="MicroDiT_XL_2")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_control.json"))
args = ap.parse_args()
assert args.repeats >= 2 and args.steps >= 3
assert torch.cuda.is_available(), "bench_prompt_control.py measures on the GPU; there is no CPU path"
L, st = hip.lib(), torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------- 1: the kernel against the plain one
def bench_kernel(B, S=256, Lc=77, hx=1024, hd=64, launches=60):
    H, ldb = hx // hd, (Lc + 3) // 4 * 4
    nbytes = 2 * (2 * B * S * hx + 2 * B * Lc * hx)                          # q read, o written, k and v read: bf16
    alloc = 2 * (2 * B * S * hx + B * Lc * 2 * hx) + 4 * B * H * S           # one operand set: q, o, [K | V] rows, lse
    sets = max(2, math.ceil(2 * (256 << 20) / alloc))                        # twice the last-level cache
    g = torch.Generator(device="cuda").manual_seed(B)
    ops = []
    for _ in range(sets):
        q = torch.randn(B * S, hx, device="cuda", generator=g).to(torch.bfloat16)
        kv = torch.randn(B * Lc, 2 * hx, device="cuda", generator=g).to(torch.bfloat16)
        o = torch.empty(B * S, hx, device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(B, H, S, device="cuda")
        w = torch.rand(B, ldb, device="cuda", generator=g) * 2
        w[:, 60:] = 0                                                        # the padding of a short caption removed
        bias = torch.log(w)
        bias[:, Lc:] = 0
        a = hip.AttnArgs()
        a.q, a.k, a.v, a.o, a.lse = q.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * hx, o.data_ptr(), lse.data_ptr()
        a.B, a.H, a.Sq, a.Skv = B, H, S, Lc
        a.ldq, a.ldk, a.ldv, a.ldo, a.sq, a.sk, a.sv, a.so = hx, 2 * hx, 2 * hx, hx, S * hx, Lc * 2 * hx, Lc * 2 * hx, S * hx
        a.scale, a.hd = 1.0 / math.sqrt(hd), hd
        ops.append((q, kv, o, lse, bias, a))
    us = {"plain": [], "kbias": []}
    for i in range(launches + sets):
        q, kv, o, lse, bias, a = ops[i % sets]
        order = ("plain", "kbias") if i % 2 == 0 else ("kbias", "plain")     # each form follows the other equally often
        for form in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if form == "plain":
                hip.check(L.md_attn_fwd(ctypes.byref(a), st), "md_attn_fwd")
            else:
                hip.check(L.md_attn_fwd_kbias(ctypes.byref(a), bias.data_ptr(), ldb, st), "md_attn_fwd_kbias")
            e1.record()
            e1.synchronize()
            if i >= sets:                                                    # the first pass over the sets is the warm-up
                us[form].append(1e3 * e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in us.items()}
    quart = statistics.quantiles(us["plain"], n=4)
    r = {"B": B, "H": H, "Sq": S, "Skv": Lc, "hd": hd, "algorithmic_bytes": nbytes, "added_bias_bytes": 4 * Lc * B, "operand_sets": sets,
         "launches_per_form": launches, "median_us": med, "min_us": {k: min(v) for k, v in us.items()},
         "ratio_kbias_to_plain": med["kbias"] / med["plain"], "plain_iqr_rel": (quart[2] - quart[0]) / med["plain"],
         "plain_spread_rel": (max(us["plain"]) - min(us["plain"])) / med["plain"], "achieved_tbs": {k: nbytes / v / 1e6 for k, v in med.items()}}
    print(f"B={B}: md_attn_fwd {med['plain']:.1f} us, md_attn_fwd_kbias {med['kbias']:.1f} us, ratio {r['ratio_kbias_to_plain']:.4f} "
          f"(plain interquartile range {r['plain_iqr_rel']:.4f}, full spread {r['plain_spread_rel']:.4f})", flush=True)
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
neg = torch.randn(1, 1, 77, dit.config.caption_channels, device="cuda", generator=g)
weights = torch.rand(B, 77, device="cuda", generator=g) * 2
weights[:, 60:] = 0
variants = {"plain": {}, "controlled": dict(caption_weights=weights, negative=neg)}


def run(kw):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = model.edm_sampler_loop(lat, y, steps=args.steps, cfg=args.guidance, cond_cache=True, **kw)
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


final = {k: run(v)[0] for k, v in variants.items()}                    # warm-up of both
ms = {k: [] for k in variants}
for _ in range(args.repeats):
    for k, v in variants.items():
        ms[k].append(run(v)[1])
med_ms = {k: statistics.median(v) for k, v in ms.items()}
blocks = len(dit.engine.mixer) + len(dit.engine.backbone)
evals = 2 * args.steps - 1
sampler = {"arch": args.arch, "batch": B, "network_batch": 2 * B if args.guidance > 1.0 else B, "steps": args.steps, "sampler": "heun",
           "guidance": args.guidance, "cond_cache": True, "repeats": args.repeats, "evaluations": evals,
           "biased_attention_launches_per_run": blocks * evals,
           "timing": "device events around edm_sampler_loop, plain and controlled alternating after one warm-up run of each",
           "ms": ms, "median_ms": med_ms, "ratio_controlled_to_plain": med_ms["controlled"] / med_ms["plain"],
           "plain_spread_rel": (max(ms["plain"]) - min(ms["plain"])) / med_ms["plain"],
           "added_us_per_attention_launch": 1e3 * (med_ms["controlled"] - med_ms["plain"]) / (blocks * evals),
           "latents_finite": bool(torch.isfinite(final["controlled"]).all()),
           "latents_differ_from_plain": not torch.equal(final["plain"], final["controlled"])}
print(f"sampler: plain {med_ms['plain']:.1f} ms, controlled {med_ms['controlled']:.1f} ms, ratio {sampler['ratio_controlled_to_plain']:.4f} "
      f"(plain spread {sampler['plain_spread_rel']:.4f})", flush=True)

res = {"device": torch.cuda.get_device_name(0), "kernel": kernel, "sampler": sampler}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps({"out": args.out, "kernel_ratios": [k["ratio_kbias_to_plain"] for k in kernel],
                  "ratio_controlled_to_plain": sampler["ratio_controlled_to_plain"], "plain_spread_rel": sampler["plain_spread_rel"]}))
