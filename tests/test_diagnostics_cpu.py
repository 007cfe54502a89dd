"""Model diagnostics, host side: config switches, the rank-order combine (alone and under a 2-process gloo group),
the logged keys, the ln sigma bin edges, and the compiled resources of the new kernels."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from micro_diffusion_amd import config as mdcfg
from micro_diffusion_amd import diagnostics as dg
from micro_diffusion_amd import hip, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ["res_256_pretrain", "res_256_finetune", "res_512_pretrain", "res_512_finetune"]


@pytest.mark.parametrize("stage", STAGES)
def test_config_keys_default_off_and_parse(stage):
    path = os.path.join(ROOT, "configs")
    plain = mdcfg.load_config(path, stage + ".yaml")
    assert mdcfg.diagnostics_options(plain) == {"diagnostics_interval": 0, "loss_by_sigma_bins": 0, "moe_routing": False}
    on = mdcfg.load_config(path, stage + ".yaml", ["+misc.diagnostics_interval=50", "+misc.loss_by_sigma_bins=16",
                                                   "+misc.moe_routing_monitor=true"])
    assert mdcfg.diagnostics_options(on) == {"diagnostics_interval": 50, "loss_by_sigma_bins": 16, "moe_routing": True}
    # the stage config itself is unaffected: everything but the three added keys parses to what it parsed to before
    misc = dict(on.get("misc") or {})
    for k in ("diagnostics_interval", "loss_by_sigma_bins", "moe_routing_monitor"):
        misc.pop(k)
    assert misc == (plain.get("misc") or {})
    assert {k: v for k, v in on.items() if k != "misc"} == {k: v for k, v in plain.items() if k != "misc"}


def test_trainer_signature_has_the_switches_off():
    import inspect
    from micro_diffusion_amd.trainer import Trainer
    p = inspect.signature(Trainer.__init__).parameters
    assert p["diagnostics_interval"].default == 0 and p["loss_by_sigma_bins"].default == 0 and p["moe_routing"].default is False


def _fabricated(world, n=7, k=5, seed=3):
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(0, 1000, (world, n), generator=g, dtype=torch.int64)
    # magnitudes 1e-8 .. 1e8: fp64 addition in another order gives other bits
    sums = torch.randn(world, k, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-8, 9, (world, k), generator=g).double()
    return counts, sums


def test_combine_is_rank_ordered():
    counts, sums = _fabricated(5)
    c, s = dg.combine_rank_diagnostics(counts, sums)
    assert torch.equal(c, counts.sum(0))
    want = sums[0].clone()
    for r in range(1, 5):
        want = want + sums[r]
    assert torch.equal(s, want), "sums must be added in rank order, starting from rank 0"
    rev = sums[4].clone()
    for r in (3, 2, 1, 0):
        rev = rev + sums[r]
    assert not torch.equal(rev, want), "the fabricated table must be order-sensitive, or the check above shows nothing"
    assert torch.equal(counts, _fabricated(5)[0]) and torch.equal(sums, _fabricated(5)[1]), "inputs are left alone"
    one_c, one_s = dg.combine_rank_diagnostics(counts[:1], sums[:1])
    assert torch.equal(one_c, counts[0]) and torch.equal(one_s, sums[0])
    with pytest.raises(ValueError):
        dg.combine_rank_diagnostics(counts.int(), sums)
    with pytest.raises(ValueError):
        dg.combine_rank_diagnostics(counts, sums.float())


def test_gather_without_a_process_group_is_the_identity():
    counts, sums = _fabricated(1)
    c, s = dg.gather_rank_diagnostics(counts[0], sums[0])
    assert torch.equal(c, counts[0]) and torch.equal(s, sums[0])


def _gloo_rank(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        counts, sums = _fabricated(world)
        c, s = dg.gather_rank_diagnostics(counts[rank], sums[rank])
        torch.save((c, s), os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_gather_and_combine_under_two_gloo_ranks(tmp_path):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_gloo_rank, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    assert [p.exitcode for p in procs] == [0, 0]
    counts, sums = _fabricated(2)
    want_c, want_s = dg.combine_rank_diagnostics(counts, sums)
    for r in range(2):
        c, s = torch.load(tmp_path / f"r{r}.pt")
        assert torch.equal(c, want_c) and torch.equal(s, want_s), f"rank {r}: the combined tables must have identical bits on every rank"


def test_route_keys_on_a_fabricated_table():
    E = 4
    hist = [10, 70, 15, 4, 1]                       # 100 tokens; chosen entries = 70 + 30 + 12 + 4 = 116 -> 29 per expert
    f = [120.0, 40.0, 30.0, 20.0, 10.0, 14.5, 8.7, 5.8, 2.9]
    out = dg.format_route_stats("blocks.3", hist, f)
    assert set(out) == {"moe/blocks.3/" + k for k in ("coverage", "dropped_frac", "router_entropy", "expert_prob_mean", "expert_gate_mean")}
    cov = out["moe/blocks.3/coverage"]
    assert len(cov) == E + 1 and abs(sum(cov) - 1.0) < 1e-15
    assert out["moe/blocks.3/dropped_frac"] == cov[0] == 0.1
    assert out["moe/blocks.3/router_entropy"] == 1.2
    assert out["moe/blocks.3/expert_prob_mean"] == [0.4, 0.3, 0.2, 0.1]
    assert out["moe/blocks.3/expert_gate_mean"] == [14.5 / 29, 8.7 / 29, 5.8 / 29, 2.9 / 29]
    assert all(type(v) in (float, list) for v in out.values())
    assert dg.format_route_stats("blocks.3", [0] * 5, [0.0] * 9) == {}
    with pytest.raises(ValueError):
        dg.format_route_stats("blocks.3", hist, f[:-1])


def test_loss_by_sigma_keys_on_a_fabricated_table():
    edges = dg.sigma_bin_edges(-1.0, 1.0, 4)
    out = dg.format_loss_by_sigma("eval", edges, [3.0, 0.0, 1.0, 8.0], [2, 0, 4, 4], 3)
    assert out == {"loss_by_sigma/eval/ln_sigma_edges": [-1.0, -0.5, 0.0, 0.5, 1.0], "loss_by_sigma/eval/count": [2, 0, 4, 4],
                   "loss_by_sigma/eval/mean_loss": [1.5, None, 0.25, 2.0], "loss_by_sigma/eval/nonfinite": 3}
    import json
    json.dumps(out)


def test_bin_edges_follow_p_mean_and_p_std():
    lbs = dg.LossBySigma(16, p_mean=-0.6, p_std=1.2)
    assert lbs.log_lo == pytest.approx(-0.6 - 3.6, abs=1e-12) and lbs.log_hi == pytest.approx(-0.6 + 3.6, abs=1e-12)
    assert len(lbs.edges) == 17 and lbs.edges[0] == lbs.log_lo and lbs.edges[-1] == lbs.log_hi
    w = [b - a for a, b in zip(lbs.edges, lbs.edges[1:])]
    assert max(w) - min(w) < 1e-12 and math.isclose(w[0], 7.2 / 16)
    assert lbs.edges[8] == pytest.approx(-0.6, abs=1e-12), "the middle edge is P_mean"
    other = dg.LossBySigma(4, p_mean=0.0, p_std=0.5, log_lo=-2.0)          # the constructor can override either end
    assert (other.log_lo, other.log_hi) == (-2.0, 1.5)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            dg.LossBySigma(bad)
    with pytest.raises(ValueError):
        dg.LossBySigma(4, log_lo=1.0, log_hi=1.0)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_new_kernels_compile_without_scratch_at_the_partial_kernels_occupancy(tmp_path):
    res = native.resource_usage("stats.hip", hip.HIPCC_FLAGS, tmp_path / "stats.o")
    floor = min(v["occ"] for k, v in res.items() if "stats_partial_kernel" in k and "route" not in k)
    new = {k: v for k, v in res.items() if any(t in k for t in ("loss_sigma_hist_kernel", "route_stats_partial_kernel",
                                                               "route_stats_finish_kernel"))}
    assert len(new) == 5, sorted(res)               # the histogram, three expert widths of the partial kernel, the finish
    for k, v in new.items():
        print(k, v)
        assert v["scratch"] == 0 and v["spill"] == 0, (k, v)
        assert v["occ"] >= floor, f"{k}: {v['vgprs']} VGPRs, {v['lds']} B LDS -> {v['occ']} waves / SIMD, md_tensor_stats_partial has {floor}"
