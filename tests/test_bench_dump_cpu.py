"""`bench.py --dump-outputs DIR`: the loss and one seeded sample, shared by the three arrays, of the fp32 weights and both AdamW
moments as float32 .npy files.  No GPU: the flat buffers are stand-ins laid out by the library's own flat_layout."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head():
    from micro_diffusion_amd import dit as mdit
    from oracle import microdit_ref as orc
    dit = mdit.DiT(**orc.tiny_config().__dict__)
    offs, total = mdit.flat_layout(dit._table)
    p = torch.arange(total, dtype=torch.float32)           # each value names its own position (total < 2^24)
    assert total < 1 << 24
    dit.flat_buffers = lambda: {"offs": offs, "p": p}
    return SimpleNamespace(model=SimpleNamespace(dit=dit), trainer=SimpleNamespace(opt=SimpleNamespace(m=p * 2, v=p * p))), offs, p


def test_dump_outputs_samples_the_training_state(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    head, offs, p = _head()
    bench.dump_outputs(head, 0.5, str(tmp_path / "a"))
    bench.dump_outputs(head, 0.5, str(tmp_path / "b"))
    names = ["adamw_exp_avg.npy", "adamw_exp_avg_sq.npy", "loss.npy", "params.npy"]
    assert sorted(os.listdir(tmp_path / "a")) == names
    out = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float32 for a in out.values())
    assert all(np.array_equal(out[n], np.load(tmp_path / "b" / n)) for n in names)      # a fixed sample
    assert out["loss.npy"].tolist() == [0.5]
    params = out["params.npy"]
    assert np.array_equal(out["adamw_exp_avg.npy"], params * 2) and np.array_equal(out["adamw_exp_avg_sq.npy"], params * params)
    i = 0
    for name, t in head.model.dit.named_parameters():                  # each tensor's segment: distinct elements of that tensor
        k = min(t.numel(), bench.DUMP_PER_TENSOR)
        pos = params[i:i + k].astype(np.int64) - offs[name]
        assert pos.min() >= 0 and pos.max() < t.numel() and len(np.unique(pos)) == k, name
        i += k
    assert i == params.size < p.numel()                                 # the larger tensors were sampled, not copied
