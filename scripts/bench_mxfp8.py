#!/usr/bin/env python
"""MXFP8 sampling measured on one MI355X; writes profiles/mxfp8.json.

Per class of block linear at XL/2 sampler shapes (B = 64 guided: M = 128 * 256 token rows; the experts: 8 x 8192 routed rows): the MX
GEMM alone, the quantisation of its input alone (md_mx_quant_rows; for w3 the MX-writing SwiGLU against the bf16 SwiGLU it replaces), and
their sum over the bf16 launch on the same operands.  Then the 30-step Heun sampler at B = 64, cfg 5, cond_cache on: MX-to-plain latency
and the relative L2 distance of the final latents (random weights: a numerical distance, not a quality measure), and MXWeights.nbytes.
Protocol: device events around `iters` back-to-back launches, MX and bf16 alternating over `rounds` rounds in one process, medians; the
spread (max - min) / median of the bf16 rounds is the noise floor.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from micro_diffusion_amd import hip  # noqa: E402

FP8_PEAK, BF16_PEAK = 5.0e15, 2.5e15
M_ROWS, EXPERTS, EXPERT_ROWS = 128 * 256, 8, 8192
# class -> (M, N, K, batch, epilogue): the widest backbone block of XL/2 (dim 1024, ffn 2816; expert ffn 3840)
CLASSES = {
    "qkv": (M_ROWS, 3072, 1024, 1, "store"),
    "proj": (M_ROWS, 1024, 1024, 1, "gated"),
    "q_linear": (M_ROWS, 1024, 1024, 1, "store"),
    "cross_attn.proj": (M_ROWS, 1024, 1024, 1, "residual"),
    "[w1; w2]": (M_ROWS, 5632, 1024, 1, "store"),
    "w3": (M_ROWS, 1024, 2816, 1, "gated"),
    "expert fc1": (EXPERT_ROWS, 3840, 1024, EXPERTS, "gelu"),
    "expert fc2": (EXPERT_ROWS, 1024, 3840, EXPERTS, "store"),
}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_class(name, M, N, K, batch, epi, rounds, iters):
    g = torch.Generator().manual_seed(len(name))
    dev = "cuda"
    x = torch.randn(batch, M, K, generator=g).to(torch.bfloat16).to(dev)
    expert = batch > 1
    # nn.Linear weight [N, K] (K-contiguous), or an expert tensor [E, K, N] (K-strided)
    w = (torch.randn(batch, K, N, generator=g) * 0.03).to(torch.bfloat16).to(dev) if expert else \
        (torch.randn(1, N, K, generator=g) * 0.03).to(torch.bfloat16).to(dev)
    out = torch.empty(batch, M, N, dtype=torch.bfloat16, device=dev)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev) if epi in ("gated", "residual") else None
    gate = torch.randn(M // 256, N, generator=g).to(torch.bfloat16).to(dev) if epi == "gated" else None
    mode = hip.EPI_RESIDUAL if res is not None else hip.EPI_STORE_BF16
    act = hip.ACT_GELU_ERF if epi == "gelu" else hip.ACT_NONE
    xq = torch.empty(batch, M, K, dtype=torch.uint8, device=dev)
    xs = torch.empty(batch, M, K // 32, dtype=torch.uint8, device=dev)
    wq = torch.empty(batch, N, K, dtype=torch.uint8, device=dev)
    ws = torch.empty(batch, N, K // 32, dtype=torch.uint8, device=dev)
    hip.mx_quant_rows(w, wq, ws, N, K, ld=N if expert else K, ldd=K, lds=K // 32, src_kcontig=not expert, batch=batch, sSrc=K * N,
                      sDst=N * K, sScale=N * (K // 32))

    def quant():
        hip.mx_quant_rows(x, xq, xs, M, K, ld=K, ldd=K, lds=K // 32, batch=batch, sSrc=M * K, sDst=M * K, sScale=M * (K // 32))

    def mx():
        hip.gemm_mxfp8(xq, xs, wq, ws, out, M, N, K, lda=K, ldb=K, ldsa=K // 32, ldsb=K // 32, ldc=N, mode=mode, act=act, res=res, ldr=N,
                       gate=gate, ldg=N, rows_per_sample=256 if gate is not None else 0, batch=batch, sA=M * K, sB=N * K,
                       sScaleA=M * (K // 32), sScaleB=N * (K // 32), sC=M * N)

    def bf16():
        hip.gemm(x, w, out, M, N, K, lda=K, ldb=N if expert else K, ldc=N, b_kcontig=not expert, mode=mode, act=act, res=res, ldr=N,
                 gate=gate, ldg=N, rows_per_sample=256 if gate is not None else 0, batch=batch, sA=M * K, sB=K * N, sC=M * N)

    quant_extra = None
    if name == "w3":   # the input of w3 comes from the SwiGLU: MX-writing against bf16-writing, not a separate quantisation pass
        h12 = torch.randn(M, 2 * K, generator=g).to(torch.bfloat16).to(dev)
        a = torch.empty(M, K, dtype=torch.bfloat16, device=dev)
        L = hip.lib()

        def swiglu_mx():
            hip.check(L.md_swiglu_fwd_mx(h12.data_ptr(), 2 * K, xq.data_ptr(), K, xs.data_ptr(), K // 32, M, K, hip.stream_ptr()), "swiglu_mx")

        def swiglu():
            hip.check(L.md_swiglu_fwd(h12.data_ptr(), 2 * K, a.data_ptr(), K, M, K, hip.stream_ptr()), "swiglu")
        quant_extra = (swiglu_mx, swiglu)
    quant()
    for fn in (mx, bf16, quant):
        timed(fn, 3)
    t = {"mx": [], "bf16": [], "quant": [], "swiglu_mx": [], "swiglu": []}
    for _ in range(rounds):
        t["mx"].append(timed(mx, iters))
        t["bf16"].append(timed(bf16, iters))
        t["quant"].append(timed(quant, iters))
        if quant_extra:
            t["swiglu_mx"].append(timed(quant_extra[0], iters))
            t["swiglu"].append(timed(quant_extra[1], iters))
    med = {k: statistics.median(v) for k, v in t.items() if v}
    flops = 2.0 * M * N * K * batch
    q_ms = med["quant"] if not quant_extra else med["swiglu_mx"] - med["swiglu"]     # w3: what the fused SwiGLU costs over the bf16 one
    r = {"M": M, "N": N, "K": K, "batch": batch, "epilogue": epi, "mx_gemm_ms": med["mx"], "quant_ms": q_ms, "bf16_ms": med["bf16"],
         "mx_sum_over_bf16": (med["mx"] + q_ms) / med["bf16"], "mx_gemm_over_bf16": med["mx"] / med["bf16"],
         "mx_gemm_fraction_of_fp8_peak": flops / (med["mx"] * 1e-3) / FP8_PEAK,
         "bf16_fraction_of_bf16_peak": flops / (med["bf16"] * 1e-3) / BF16_PEAK,
         "bf16_noise_floor": (max(t["bf16"]) - min(t["bf16"])) / med["bf16"], "rounds_ms": t}
    if quant_extra:
        r["standalone_quant_ms"] = med["quant"]
    return r


def bench_sampler(steps, B, cfg, rounds):
    from micro_diffusion_amd.dit import MicroDiT_XL_2
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    from micro_diffusion_amd.mxfp8 import ALL_TARGETS, MXWeights
    torch.manual_seed(0)
    d = MicroDiT_XL_2()
    with torch.no_grad():       # zero-initialised output layers would make every output zero: give them the body's scale
        for n, p in d.named_parameters():
            if p.dim() >= 2 and float(p.abs().max()) == 0.0:
                p.normal_(std=0.02)
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=32)
    m.eval()
    mx = MXWeights(m.dit, targets=ALL_TARGETS)      # every quantisable linear, whatever the default set leaves out
    g = torch.Generator().manual_seed(1)
    lat = torch.randn(B, 4, 32, 32, generator=g).cuda()
    y = torch.randn(B, 1, 77, 1024, generator=g).cuda()

    def run(**kw):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = m.edm_sampler_loop(lat, y, steps=steps, cfg=cfg, cond_cache=True, **kw)
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1)
    run()
    run(mxfp8=mx)
    t = {"plain": [], "mx": []}
    for _ in range(rounds):
        plain, ms = run()
        t["plain"].append(ms)
        q, ms = run(mxfp8=mx)
        t["mx"].append(ms)
    mp, mq = statistics.median(t["plain"]), statistics.median(t["mx"])
    rel = float((q.double() - plain.double()).norm() / plain.double().norm())
    return {"steps": steps, "B": B, "cfg": cfg, "plain_ms": mp, "mx_ms": mq, "mx_over_plain": mq / mp,
            "plain_noise_floor": (max(t["plain"]) - min(t["plain"])) / mp, "final_latents_relative_l2": rel, "finite": bool(torch.isfinite(q).all()),
            "mx_weights_nbytes": mx.nbytes, "mx_targets": len(mx.entries), "mx_skipped": mx.skipped, "rounds_ms": t}


def tiny_forward_distance(B=3):
    """Relative L2 of one MXFP8 forward (every quantisable linear) against the bf16 forward: Tiny widths, 8 x 8 latents, random weights."""
    from micro_diffusion_amd.dit import MicroDiT_Tiny_2
    from micro_diffusion_amd.mxfp8 import ALL_TARGETS, MXWeights
    torch.manual_seed(0)
    d = MicroDiT_Tiny_2(input_size=8)
    with torch.no_grad():
        for n, p in d.named_parameters():
            if p.dim() >= 2 and float(p.abs().max()) == 0.0:
                p.normal_(std=0.02)
    d = d.to("cuda")
    mx = MXWeights(d, targets=ALL_TARGETS)
    g = torch.Generator().manual_seed(2)
    x, t = torch.randn(B, 4, 8, 8, generator=g).cuda(), (torch.rand(B, generator=g) * 2 + 0.1).cuda()
    y = torch.randn(B, 1, 77, 1024, generator=g).cuda()
    with torch.no_grad():
        plain = d.forward_without_cfg(x, t, y)["sample"].double()
        d.engine.mx = mx
        try:
            q = d.forward_without_cfg(x, t, y)["sample"].double()
        finally:
            d.engine.mx = None
    return {"B": B, "relative_l2": float((q - plain).norm() / plain.norm()), "targets": len(mx.entries), "skipped": mx.skipped}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sampler-rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--no-sampler", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp8.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "source_hash": hip._gemm_source_hash(), "classes": {}}
    for name, (M, N, K, batch, epi) in CLASSES.items():
        res["classes"][name] = r = bench_class(name, M, N, K, batch, epi, a.rounds, a.iters)
        print(f"{name:16s} mx {r['mx_gemm_ms']:.3f} ms ({r['mx_gemm_fraction_of_fp8_peak']:.3f} of fp8 peak) + quant {r['quant_ms']:.3f} ms "
              f"vs bf16 {r['bf16_ms']:.3f} ms: {r['mx_sum_over_bf16']:.3f}  (noise {r['bf16_noise_floor']:.3f})", flush=True)
    res["tiny_forward"] = tf = tiny_forward_distance()
    print(f"Tiny forward, MXFP8 against bf16: relative L2 {tf['relative_l2']:.4f} ({tf['targets']} linears, {len(tf['skipped'])} not eligible)", flush=True)
    if not a.no_sampler:
        res["sampler"] = s = bench_sampler(a.steps, 64, 5.0, a.sampler_rounds)
        print(f"sampler: plain {s['plain_ms']:.0f} ms, mx {s['mx_ms']:.0f} ms: {s['mx_over_plain']:.3f}; rel L2 {s['final_latents_relative_l2']:.4f}; "
              f"MXWeights {s['mx_weights_nbytes'] / 2 ** 20:.0f} MiB", flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
