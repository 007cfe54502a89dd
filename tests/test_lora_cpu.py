"""LoRA, host side: target resolution, the item table, the state dict, the config switches and the fp64 restatements
the GPU tests compare the kernels with.  No GPU."""
import math
import os
import re

import pytest
import torch

from micro_diffusion_amd import config as mdcfg
from micro_diffusion_amd import dit as mdit
from micro_diffusion_amd import hip, lora, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return mdit.MicroDiT_Tiny()


def _blocks(d):
    return d.config.depth + d.config.patch_mixer_depth


def test_default_targets_on_tiny_and_xl2(tiny):
    from micro_diffusion_amd.arch import DiTConfig, param_table
    specs = lora.resolve_targets(tiny._table, lora.DEFAULT_TARGETS)
    assert len(specs) == 5 * _blocks(tiny) == 20
    assert all(len(s.shape) == 2 and s.ctor == "linear_w" and s.name.split(".")[0] in ("blocks", "patch_mixer") for s in specs)
    assert [s.name for s in specs] == [s.name for s in tiny._table if s in specs], "table order"
    import numpy as np
    xl = DiTConfig(32, 2, 4, 1024, 28, 64, 256, 1024, 1.0, 1e-6, True, tuple(np.linspace(0.5, 1.0, 28)), tuple(np.linspace(0.5, 4.0, 28)),
                   True, 6, 768, 1.0, 4.0, False, 8, 2.0, 2)
    xs = lora.resolve_targets(param_table(xl), lora.DEFAULT_TARGETS)
    assert len(xs) == 5 * (28 + 6)
    assert all(s.shape[1] % 8 == 0 for s in xs)


@pytest.mark.parametrize("pattern", [r"patch_mixer\.1\.mlp\.w1$",       # 3-D expert tensor of a MoE block
                                     r"patch_mixer\.1\.mlp\.w2$",
                                     r"x_embedder\.proj\.weight",       # conv-shaped
                                     r"blocks\.0\.norm1\.weight",       # 1-D
                                     r"t_embedder\.mlp\.0\.bias",
                                     r"pos_embed"])                     # a buffer
def test_targets_of_another_kind_raise(tiny, pattern):
    assert any(re.search(pattern, s.name) for s in tiny._table), "the pattern must select something for this test to mean anything"
    with pytest.raises(ValueError, match="only 2-D linear"):
        lora.resolve_targets(tiny._table, [pattern])


def test_unmatched_pattern_and_bad_arguments_raise(tiny):
    with pytest.raises(ValueError, match="matches no parameter"):
        lora.resolve_targets(tiny._table, [r"attn\.qkv", r"no_such_module"])
    with pytest.raises(ValueError):
        lora.resolve_targets(tiny._table, [])
    for bad in (0, 3, 12, 128, True, 16.0):
        with pytest.raises(ValueError, match="rank"):
            lora.LoRA(tiny, rank=bad, device="cpu")


def test_item_table_matches_the_flat_layout(tiny):
    ad = lora.LoRA(tiny, rank=8, device="cpu")
    offs, total = mdit.flat_layout(tiny._table)
    rows = ad.item_rows()
    assert len(rows) == 20
    end = 0
    for (w, a, b, n, k), spec in zip(rows, ad.specs):
        assert w == offs[spec.name] and (n, k) == tuple(spec.shape)
        assert w % 8 == 0 and a % 4 == 0 and b % 4 == 0 and w + n * k <= total
        assert a >= end and b >= a + 8 * k, "A then B, no overlap"
        end = b + n * 8
    assert end <= ad.total and ad.total % 8 == 0
    # what ctypes hands the library is the header's struct: 4 x int64 + 2 x int32
    assert ctypes_sizeof(hip.LoraItem) == 40
    header = open(os.path.join(ROOT, "include", "microdit_hip.h")).read()
    body = re.search(r"typedef struct md_lora_item \{(.*?)\} md_lora_item;", header, flags=re.S).group(1)
    declared = [n.strip() for line in re.findall(r"^\s*int(?:64|32)_t\s+([\w, ]+);", body, flags=re.M) for n in line.split(",")]
    assert declared == [f[0] for f in hip.LoraItem._fields_]


def ctypes_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


def test_init_is_reproducible_and_b_is_zero(tiny):
    a, b, c = lora.LoRA(tiny, rank=16, seed=5, device="cpu"), lora.LoRA(tiny, rank=16, seed=5, device="cpu"), lora.LoRA(tiny, rank=16, seed=6, device="cpu")
    assert torch.equal(a.w, b.w) and not torch.equal(a.w, c.w)
    assert a.alpha == 16.0 and a.scale == 1.0 and lora.LoRA(tiny, rank=8, alpha=4, device="cpu").scale == 0.5
    gen = torch.Generator().manual_seed(5)
    for s in a.specs:
        ref = torch.empty(16, s.shape[1])
        torch.nn.init.kaiming_uniform_(ref, a=math.sqrt(5), generator=gen)          # per target, in table order
        assert torch.equal(a.A(s.name), ref)
        assert a.A(s.name).abs().max() <= 1 / math.sqrt(s.shape[1]) and bool(a.A(s.name).any())
        assert not a.B(s.name).any()
    assert not a.g.any()


def test_state_dict_layout_and_round_trip(tiny):
    ad = lora.LoRA(tiny, rank=4, alpha=8, targets=[r"blocks\.\d+\.attn\.proj\.weight$", r"patch_mixer\.0\.cross_attn\.kv_linear"], seed=1,
                   device="cpu")
    gen = torch.Generator().manual_seed(9)
    ad.w.copy_(torch.randn(ad.total, generator=gen))
    sd = ad.state_dict()
    tens = {k: v for k, v in sd.items() if torch.is_tensor(v)}
    assert sorted(tens) == sorted(m + s for m in ("blocks.0.attn.proj", "blocks.1.attn.proj", "patch_mixer.0.cross_attn.kv_linear")
                                  for s in (".lora_A.weight", ".lora_B.weight"))
    assert tuple(sd["blocks.0.attn.proj.lora_A.weight"].shape) == (4, 256) and tuple(sd["blocks.0.attn.proj.lora_B.weight"].shape) == (256, 4)
    assert tuple(sd["patch_mixer.0.cross_attn.kv_linear.lora_B.weight"].shape) == (256, 4)
    assert sd["rank"] == 4 and sd["alpha"] == 8.0 and sd["targets"] == ad.targets
    back = lora.LoRA.from_state_dict(tiny, sd, device="cpu")
    assert back.rank == 4 and back.scale == 2.0 and back.names == ad.names
    for n in ad.names:
        assert torch.equal(back.A(n), ad.A(n)) and torch.equal(back.B(n), ad.B(n))
    # another model's shapes, another rank, other targets: refused
    other = lora.LoRA(tiny, rank=4, targets=[r"blocks\.\d+\.attn\.qkv\.weight$", r"patch_mixer\.0\.cross_attn\.kv_linear"], device="cpu")
    with pytest.raises(RuntimeError, match="do not match"):
        other.load_state_dict(sd)
    wrong = dict(sd)
    wrong["blocks.0.attn.proj.lora_A.weight"] = torch.zeros(4, 128)
    with pytest.raises(RuntimeError, match="this model needs"):
        ad.load_state_dict(wrong)
    with pytest.raises(RuntimeError, match="rank"):
        lora.LoRA(tiny, rank=8, targets=ad.targets, device="cpu").load_state_dict(sd)


def test_attach_needs_a_gpu(tiny):
    with pytest.raises(RuntimeError, match="GPU"):
        lora.LoRA(tiny, rank=4, device="cpu").attach()


def _cfg(**misc):
    return {"misc": misc, "algorithms": {"gradient_clipping": {"clip_norm": 0.25}}}


def test_lora_options_parsing():
    off = mdcfg.lora_options({}, world=1)
    assert off["enabled"] is False and off["rank"] == 0
    assert mdcfg.lora_options(_cfg(lora_rank=0), world=8)["enabled"] is False, "off: nothing is refused"
    o = mdcfg.lora_options(_cfg(lora_rank=16), world=1)
    assert o == {"enabled": True, "rank": 16, "alpha": None, "targets": list(lora.DEFAULT_TARGETS), "weight_decay": 0.0, "load_path": None}
    o = mdcfg.lora_options(_cfg(lora_rank=8, lora_alpha=4, lora_targets=[r"attn\.qkv"], lora_weight_decay=0.01, lora_load_path="a.pt"), world=1)
    assert (o["rank"], o["alpha"], o["targets"], o["weight_decay"], o["load_path"]) == (8, 4.0, [r"attn\.qkv"], 0.01, "a.pt")
    assert mdcfg.lora_options(_cfg(lora_rank=8, lora_targets=r"attn\.proj"), world=1)["targets"] == [r"attn\.proj"]
    for bad in (dict(lora_rank=12), dict(lora_rank=True), dict(lora_rank="16"), dict(lora_rank=16, lora_alpha="x"),
                dict(lora_rank=16, lora_targets=[]), dict(lora_rank=16, lora_targets=["("]), dict(lora_rank=16, lora_weight_decay=-1),
                dict(lora_alpha=8), dict(lora_targets=["a"]), dict(lora_load_path="a.pt"), dict(lora_rank=0, lora_weight_decay=0.1)):
        with pytest.raises(ValueError, match="lora_"):
            mdcfg.lora_options(_cfg(**bad), world=1)


def test_lora_options_refuse_what_is_not_covered(monkeypatch):
    with pytest.raises(ValueError, match="single-GPU"):
        mdcfg.lora_options(_cfg(lora_rank=16), world=2)
    monkeypatch.setenv("WORLD_SIZE", "4")
    with pytest.raises(ValueError, match="WORLD_SIZE = 4"):
        mdcfg.lora_options(_cfg(lora_rank=16))
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert mdcfg.lora_options(_cfg(lora_rank=16))["enabled"]
    c = _cfg(lora_rank=16)
    c["algorithms"]["ema"] = {"smoothing": 0.999}
    with pytest.raises(ValueError, match="algorithms.ema"):
        mdcfg.lora_options(c, world=1)
    with pytest.raises(ValueError, match="posthoc_ema_sigma_rels"):
        mdcfg.lora_options(_cfg(lora_rank=16, posthoc_ema_sigma_rels=[0.05]), world=1)
    with pytest.raises(ValueError, match="posthoc_ema_snapshot_interval"):
        mdcfg.lora_options(_cfg(lora_rank=16, posthoc_ema_snapshot_interval="100ba"), world=1)
    with pytest.raises(ValueError, match="optimizer_monitor_interval"):
        mdcfg.lora_options(_cfg(lora_rank=16, optimizer_monitor_interval=10), world=1)
    assert mdcfg.lora_options(_cfg(lora_rank=16, optimizer_monitor_interval=0, loss_uncertainty_weighting=True, diagnostics_interval=5),
                              world=1)["enabled"], "loss weighting and the diagnostics stay available"


@pytest.mark.parametrize("rows,cols,rank", [(8, 128, 4), (200, 192, 8), (1, 64, 32)])
def test_ref_functions_against_autograd(rows, cols, rank):
    g = torch.Generator().manual_seed(rows + cols)
    p, G = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    A = torch.randn(rank, cols, generator=g, dtype=torch.float64, requires_grad=True)
    B = torch.randn(rows, rank, generator=g, dtype=torch.float64, requires_grad=True)
    scale, gs = 0.75, 0.5
    W = p.double() + scale * (B @ A)
    assert torch.equal(lora.ref_merge(p, A.detach(), B.detach(), scale), W.detach())
    ((gs * G.double()) * W).sum().backward()
    dA, dB = lora.ref_grad(G, A.detach(), B.detach(), scale, gs)
    assert dA.dtype == torch.float64 and tuple(dA.shape) == (rank, cols) and tuple(dB.shape) == (rows, rank)
    for name, a, b in (("dA", dA, A.grad), ("dB", dB, B.grad)):
        err = float((a - b).abs().max())
        print(f"{name} {rows}x{cols} r{rank}: max |ref - autograd| = {err:.3g} (bound 1e-12 * max |ref|)")
        assert err <= 1e-12 * float(b.abs().max())


def test_ws_floats_checks_the_table_on_the_host():
    """md_lora_grad_ws_floats is host code: it runs without a GPU.  It fixes the workspace layout (one [rank, cols] slice per strip of 64
    rows) and refuses the shapes the kernels do not take."""
    import ctypes
    L = hip.lib()

    def ask(items, rank):
        arr = (hip.LoraItem * len(items))(*[hip.LoraItem(*it) for it in items])
        out = ctypes.c_int64(-1)
        return L.md_lora_grad_ws_floats(arr, len(items), rank, ctypes.byref(out)), out.value, arr

    rc, n, arr = ask([(0, 0, 512, 0, 8, 128), (1024, 1024, 2048, 0, 200, 192), (65536, 8192, 16384, 0, 64, 64)], 4)
    assert rc == 0 and n == 1 * 4 * 128 + 4 * 4 * 192 + 1 * 4 * 64
    assert [a.ws_off for a in arr] == [0, 512, 512 + 3072]
    for rank in (0, 2, 12, 128):
        assert ask([(0, 0, 512, 0, 8, 128)], rank)[0] == -1
    for item in [(0, 0, 512, 0, 8, 100), (0, 0, 512, 0, 8, 4), (0, 0, 512, 0, 0, 128), (4, 0, 512, 0, 8, 128), (0, 2, 512, 0, 8, 128),
                 (0, 0, 514, 0, 8, 128), (-8, 0, 512, 0, 8, 128)]:
        assert ask([item], 8)[0] == -1, item
    assert L.md_lora_grad_ws_floats(None, 1, 8, ctypes.byref(ctypes.c_int64())) == -1


def test_source_is_built_hashed_and_spill_free(tmp_path):
    assert os.path.join(native.CSRC, "lora.hip") in hip._hashed_files()
    for name in ("md_lora_merge", "md_lora_grad_ws_floats", "md_lora_grad"):
        assert name in hip.exported_symbols()
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    res = native.resource_usage("lora.hip", hip.HIPCC_FLAGS, tmp_path / "lora.o")
    assert len(res) == 16, sorted(res)            # merge: 5 ranks x {bf16, f32}; grad: 5 ranks; the finish
    for name, v in res.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (name, v)
        assert v["lds"] <= 64 * 1024 and v["occ"] >= 3, (name, v)


def test_fused_adamw_and_trainer_surface():
    """What the Trainer reads from an optimiser exists on LoRAAdamW (checked without constructing one: that needs a GPU)."""
    for member in ("step", "ensure_norm_slots", "skipped_steps", "state_dict", "load_state_dict", "swap_ema", "ema_state_dict", "grad_norm"):
        assert callable(getattr(lora.LoRAAdamW, member))
