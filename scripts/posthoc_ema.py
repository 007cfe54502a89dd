"""Synthesise the EMA of any length from the post-hoc EMA snapshots a run wrote (train.py: misc.posthoc_ema_sigma_rels,
misc.posthoc_ema_snapshot_interval; files <save_folder>/posthoc/ema-<step>-<sigma_rel>.pt):

    python scripts/posthoc_ema.py --snapshots ./trained_models/run1/posthoc --sigma-rel 0.075 [--step 200000] --out ema_0.075.pt

writes a state_dict that `dit.load_state_dict` accepts: the synthesised parameters plus the buffers (pos_embed) the snapshots carry.
Host only: fp64 sums on the CPU, no GPU is touched."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from micro_diffusion_amd import posthoc_ema  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--snapshots", required=True, help="folder of ema-<step>-<sigma_rel>.pt files")
    ap.add_argument("--sigma-rel", type=float, required=True, help="relative width of the wanted average, inside (0, 0.28)")
    ap.add_argument("--step", type=int, default=None, help="training step of the wanted average (default: the last snapshot's)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    files = posthoc_ema.list_snapshots(a.snapshots)
    if not files:
        raise SystemExit(f"no ema-*.pt snapshot under {a.snapshots}")
    sd = posthoc_ema.reconstruct(files, a.sigma_rel, a.step)
    tmp = a.out + ".tmp"
    torch.save(sd, tmp)
    os.replace(tmp, a.out)
    print(json.dumps({"snapshots": len(files), "sigma_rel": a.sigma_rel, "gamma": posthoc_ema.sigma_rel_to_gamma(a.sigma_rel),
                      "step": a.step, "tensors": len(sd), "out": a.out}))


if __name__ == "__main__":
    main()
