"""Record the bits of the sampler's elementwise kernels: runs the case list of tests/sampler_bits.py on the loaded library (MICRODIT_LIB
names another build) and writes {case id: {buffer: sha256}} as JSON.  Run it on the build whose results are to be kept BEFORE changing a
kernel; tests/test_sampler_kernel_bits_gpu.py then holds every later build to them.
Usage: python scripts/record_sampler_bits.py [--out tests/golden/sampler_kernel_bits.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import hip  # noqa: E402
from tests import sampler_bits  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sampler_kernel_bits.json"))
args = ap.parse_args()

assert torch.cuda.is_available(), "recording needs the GPU"
bits = sampler_bits.compute(hip.lib(), torch.cuda.current_stream().cuda_stream)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(bits, f, indent=0, sort_keys=True)
    f.write("\n")
print(f"{len(bits)} cases, {sum(len(v) for v in bits.values())} digests -> {args.out}")
