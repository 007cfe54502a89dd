"""LoRA's factored backward against the projected one on an MI355X, MicroDiT_XL_2, default targets, one GPU, one process:
  * md_lora_wgrad alone on the XL/2 shapes (M = 16384 and 65536; (N, K) of the backbone's and the mixer's attention projections): time,
    algorithmic bytes 2 M (N + K) over time as a fraction of the HBM peak, and next to it what it replaces -- the full weight-gradient
    GEMM of the same operands into an fp32 [N, K] accumulator plus md_lora_grad on that one matrix;
  * LoRAAdamW.step in both modes (device events, a gradient filled in before every repeat);
  * the full optimisation step (bench.Stage, res_256_pretrain, 2048 images) in both modes: same process, same model and adapter, rounds
    in alternating order; the ratio is reported next to the spread of the projected rounds;
  * peak device memory of a step in each mode (both include the bench stage's FusedAdamW state, which a LoRA run would not allocate).
Writes a JSON file (default profiles/lora_factored.json).
Usage: python scripts/bench_lora_factored.py [--rank 16] [--repeats 20] [--steps 3] [--rounds 3] [--microbatch 256] [--skip-step] [--out FILE]"""
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
from micro_diffusion_amd import hip, lora  # noqa: E402
from micro_diffusion_amd.trainer import Trainer  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--microbatch", type=int, default=256)
ap.add_argument("--skip-step", action="store_true", help="only the kernel and the optimiser passes, not the full 2048-image steps")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_factored.json"))
args = ap.parse_args()

torch.cuda.set_device(0)
L = hip.lib()
R = args.rank
SHAPES = [("blocks qkv", 3072, 1024), ("blocks proj / q_linear", 1024, 1024), ("blocks kv_linear", 2048, 1024), ("1536 x 1024", 1536, 1024),
          ("mixer qkv", 2304, 768), ("mixer proj / q_linear", 768, 768)]


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


st = bench.Stage("res_256_pretrain", "MicroDiT_XL_2", 2048, args.microbatch, 1, 0)
dit = st.model.dit
eng = dit.engine
f = dit.flat_buffers()
full_tr = st.trainer
clip = full_tr.clip_norm
out = {"model": "MicroDiT_XL_2", "rank": R, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
       "hbm_peak_TBps": bench.HBM_PEAK_TBS, "kernel": []}

# ---------------------------------------------------------------------------------------------------- md_lora_wgrad alone
for M in (16384, 65536):
    for label, N, K in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(M + N + K)
        dy = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
        x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
        A = torch.randn(R, K, device="cuda", generator=g) / K ** 0.5
        B = torch.randn(N, R, device="cuda", generator=g) * 0.01
        dA, dB = torch.zeros_like(A), torch.zeros_like(B)
        need, strip, groups = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
        hip.check(L.md_lora_wgrad_ws_floats(M, N, K, R, ctypes.byref(need)), "md_lora_wgrad_ws_floats")
        hip.check(L.md_lora_wgrad_geometry(M, N, K, R, ctypes.byref(strip), ctypes.byref(groups)), "md_lora_wgrad_geometry")
        ws = torch.empty(need.value, device="cuda")
        fact = timed(lambda: hip.check(L.md_lora_wgrad(dy.data_ptr(), N, x.data_ptr(), K, M, N, K, A.data_ptr(), B.data_ptr(), R, 1.0,
                                                       dA.data_ptr(), dB.data_ptr(), ws.data_ptr(), ws.numel(), hip.stream_ptr()), "md_lora_wgrad"))
        # what it replaces: G [N, K] += dy^T x (the engine's split-K weight-gradient GEMM), then this matrix's share of md_lora_grad
        G = torch.zeros(N, K, device="cuda")
        gemm = timed(lambda: eng._acc_each(G.data_ptr(), N, K, M, [(dy.data_ptr(), x.data_ptr())], lda=N, ldb=K, a_kcontig=0))
        pad = lambda n: (n + 7) // 8 * 8
        item = (hip.LoraItem * 1)(hip.LoraItem(0, 0, pad(R * K), 0, N, K))
        pneed = ctypes.c_int64(0)
        hip.check(L.md_lora_grad_ws_floats(item, 1, R, ctypes.byref(pneed)), "md_lora_grad_ws_floats")
        item_dev = torch.from_numpy(np.frombuffer(item, dtype=np.uint8).copy()).cuda()
        adp = torch.zeros(pad(R * K) + pad(N * R), device="cuda")
        adp[:R * K] = A.reshape(-1)
        adp[pad(R * K):pad(R * K) + N * R] = B.reshape(-1)
        dadp, pws = torch.zeros_like(adp), torch.empty(max(pneed.value, 4), device="cuda")
        proj = timed(lambda: hip.check(L.md_lora_grad(G.data_ptr(), adp.data_ptr(), item_dev.data_ptr(), item, 1, R, 1.0, 1.0, dadp.data_ptr(),
                                                      pws.data_ptr(), pws.numel(), hip.stream_ptr()), "md_lora_grad"))
        nbytes = 2 * M * (N + K)
        row = {"shape": label, "M": M, "N": N, "K": K, "strip_rows": strip.value, "row_groups": groups.value, "ws_bytes": 4 * need.value,
               "md_lora_wgrad": fact, "algorithmic_bytes": nbytes, "TB_per_s": nbytes / fact["median_ms"] / 1e9,
               "fraction_of_hbm_peak": nbytes / fact["median_ms"] / 1e9 / bench.HBM_PEAK_TBS,
               "wgrad_gemm": gemm, "md_lora_grad_one_matrix": proj,
               "replaced_ms": gemm["median_ms"] + proj["median_ms"],
               "factored_over_replaced": fact["median_ms"] / (gemm["median_ms"] + proj["median_ms"])}
        out["kernel"].append(row)
        print(json.dumps(row), flush=True)
        del dy, x, G, ws
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------- the optimiser pass, both modes
ad = lora.LoRA(dit, rank=R, seed=18)
with torch.no_grad():                       # a trained adapter: B is not zero
    for n in ad.names:
        ad.B(n).normal_(0.0, 0.01)
opt = lora.LoRAAdamW(ad, lr=full_tr.opt.lr)  # attaches the adapter
lora_tr = Trainer(st.model, opt, full_tr.schedule, clip_norm=clip, microbatch_size=args.microbatch)
lora_tr.batches_seen = full_tr.batches_seen
out["targets"], out["adapter_elements"], out["flat_elements"] = len(ad.specs), ad.total, f["total"]
grad = torch.randn(f["total"], device="cuda") * 1e-3
agrad = torch.randn(ad.total, device="cuda") * 1e-3
ad.backward = "projected"
out["LoRAAdamW.step"] = {"projected": timed(lambda: opt.step(lr=1e-5, max_norm=clip), lambda: f["g"].copy_(grad))}
ad.backward = "factored"
out["LoRAAdamW.step"]["factored"] = timed(lambda: opt.step(lr=1e-5, max_norm=clip), lambda: ad.g.copy_(agrad))
print("LoRAAdamW.step", json.dumps(out["LoRAAdamW.step"]), flush=True)
del grad, agrad
f["g"].zero_()
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------- the 2048-image step, both modes
if not args.skip_step:
    st.trainer = lora_tr
    res, peak = {"projected": [], "factored": []}, {}
    for rnd in range(args.rounds):
        for mode in (("projected", "factored") if rnd % 2 == 0 else ("factored", "projected")):
            ad.backward = mode
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            e, loss = st.timed(args.steps, 1, 1)
            peak[mode] = max(peak.get(mode, 0), torch.cuda.max_memory_allocated())
            res[mode].append(1e3 * e / args.steps)
            print(f"{mode:9s} round {rnd}: {1e3 * e / args.steps:8.2f} ms / step  loss {loss:.5f}", flush=True)
    a, b = statistics.median(res["projected"]), statistics.median(res["factored"])
    out["full_step"] = {"stage": "res_256_pretrain", "global_batch": 2048, "microbatch": args.microbatch, "steps_per_round": args.steps,
                        "ms_per_step": res, "median_projected_ms": a, "median_factored_ms": b, "factored_over_projected": b / a,
                        "projected_spread": (max(res["projected"]) - min(res["projected"])) / a}
    wsb = 0 if ad._wgrad_ws is None else 4 * ad._wgrad_ws.numel()
    out["peak_device_bytes"] = dict(peak, wgrad_workspace=wsb, adapter_and_optimizer=4 * lora.allocated_floats(opt) - wsb)
    print("full step", json.dumps(out["full_step"]), flush=True)
    print("memory", json.dumps(out["peak_device_bytes"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", args.out)
