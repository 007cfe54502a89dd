"""Per-kernel A/B of two builds of libmicrodit_hip.so on the sampler's twelve update entry points (md_edm_{heun,solver}_update[_guide|_coef]
[_tok]).  These kernels are memory-bound and tiny next to the network: scripts/bench_sampler.py and scripts/bench_guidance.py cannot see
them, so they are timed alone, at the shapes a user runs: latents [64, 4, 64, 64] and [64, 4, 32, 32], patch 2, guidance on.

Both libraries are loaded into one process (ctypes) and warmed; then windows alternate A B A B ..., at least five per side.  A window is
as many back-to-back launches as last 100 ms (counted once per entry point on library A, the same count for both), bracketed by device
events and ended by a synchronise; its figure is microseconds per launch.  Per entry point and shape, B passes when its median is not
above A's median by more than A's own spread (max - min of its windows).  The two must also return the same bytes.
Writes the medians, spreads and verdicts to profiles/sampler_kernels_ab.json; exit status 1 when an entry point loses or the bytes differ.
Usage: python scripts/ab_sampler_kernels.py LIB_A LIB_B [--windows 5] [--window-ms 100] [--out FILE]   (park the builds under
scratch_libs/ as scripts/ab_libs.sh describes; A is the parent)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import hip, native  # noqa: E402
from tests import sampler_bits as sb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("lib_a")
ap.add_argument("lib_b")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_kernels_ab.json"))
args = ap.parse_args()
assert args.windows >= 5 and args.window_ms >= 100.0, "at least five windows of at least 100 ms per side"

SHAPES = [(64, 4, 64, 64), (64, 4, 32, 32)]
libs = {"A": native.load(args.lib_a, hip._SIGS, "md_abi_version", hip.ABI_VERSION),
        "B": native.load(args.lib_b, hip._SIGS, "md_abi_version", hip.ABI_VERSION)}
st = torch.cuda.current_stream().cuda_stream


def window(L, call, count):
    """Milliseconds of `count` launches between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        call(L)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


results, failed = [], False
for shape in SHAPES:
    inp = sb.Inputs(shape)
    for step in sb.STEPS:
        for source in sb.SOURCES:
            for layout in sb.LAYOUTS:
                name = sb.entry_name(step, source, layout)
                state, x_next = inp.state0.clone(), inp.fresh()

                a = sb.update_args(inp, step, source, layout, state, x_next, st)    # built once: a window is launches, not Python

                def call(L, a=a, name=name):
                    code = getattr(L, name)(*a)
                    assert code == 0, (name, code)

                # the bytes: each library on fresh outputs
                out = {}
                for k, L in libs.items():
                    s, x = inp.state0.clone(), inp.fresh()
                    assert sb.launch_update(L, inp, step, source, layout, s, x, st) == 0, name
                    torch.cuda.synchronize()
                    out[k] = (sb.digest(s), sb.digest(x))
                same = out["A"] == out["B"]
                # warm both, size the window on A
                for L in libs.values():
                    window(L, call, 200)
                count = 200
                while True:
                    ms = window(libs["A"], call, count)
                    if ms >= 1.5 * args.window_ms:
                        break
                    count = int(count * max(1.5, 1.6 * args.window_ms / max(ms, 1e-3))) + 1
                for attempt in range(4):                # a window that came in short: more launches, all windows again
                    us = {"A": [], "B": []}
                    shortest = float("inf")
                    for _ in range(args.windows):
                        for k, L in libs.items():
                            ms = window(L, call, count)
                            shortest = min(shortest, ms)
                            us[k].append(ms * 1e3 / count)
                    if shortest >= args.window_ms:
                        break
                    count *= 2
                assert shortest >= args.window_ms, (name, shortest)
                med = {k: statistics.median(v) for k, v in us.items()}
                spread_a = max(us["A"]) - min(us["A"])
                ok = same and med["B"] <= med["A"] + spread_a
                failed |= not ok
                results.append({"entry": name, "shape": list(shape), "launches_per_window": count, "us_a_median": round(med["A"], 4),
                                "us_b_median": round(med["B"], 4), "us_a_spread": round(spread_a, 4),
                                "us_b_spread": round(max(us["B"]) - min(us["B"]), 4), "us_a": [round(v, 4) for v in us["A"]],
                                "us_b": [round(v, 4) for v in us["B"]], "equal_bytes": same, "pass": ok})
                print(f"{name:36s} {str(shape):18s} A {med['A']:8.3f} us (spread {spread_a:.3f})  B {med['B']:8.3f} us  bytes "
                      f"{'equal' if same else 'DIFFER'}  {'ok' if ok else 'LOSES'}", flush=True)

report = {"what": "microseconds per launch of the sampler update entry points, library B against library A (the parent), windows alternating "
                  "in one process; pass: median B <= median A + (max - min of A's windows), and equal output bytes",
          "device": torch.cuda.get_device_name(0), "windows_per_side": args.windows, "window_ms_min": args.window_ms,
          "source_hash_b": hip._source_hash(), "verdict": "fail" if failed else "pass", "results": results}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
    f.write("\n")
print(f"verdict: {report['verdict']} -> {args.out}")
sys.exit(1 if failed else 0)
