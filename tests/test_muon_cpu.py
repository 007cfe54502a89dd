"""Muon, host side: the config switches, target resolution and the split of the flat buffers between Muon and AdamW,
the shape factors, the state dict, the plumbing of the new symbols, and the reference models the GPU tests compare the kernels with.
No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

from micro_diffusion_amd import config as mdcfg
from micro_diffusion_amd import dit as mdit
from micro_diffusion_amd import hip, muon
from micro_diffusion_amd.arch import DiTConfig, param_table
from tests import muon_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("md_muon_ws_bytes", "md_muon_momentum", "md_muon_newton_schulz", "md_muon_apply", "md_muon_axpby")


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return mdit.MicroDiT_Tiny()


def _xl2_table():
    return param_table(DiTConfig(32, 2, 4, 1024, 28, 64, 256, 1024, 1.0, 1e-6, True, tuple(np.linspace(0.5, 1.0, 28)),
                                 tuple(np.linspace(0.5, 4.0, 28)), True, 6, 768, 1.0, 4.0, False, 8, 2.0, 2))


def _tiny2_table():
    return param_table(DiTConfig(32, 2, 4, 512, 16, 32, 256, 1024, 1.0, 1e-6, True, tuple(np.linspace(0.5, 1.0, 16)),
                                 tuple(np.linspace(0.5, 4.0, 16)), True, 4, 512, 1.0, 1.0, False, 8, 2.0, 2))


# ---------------------------------------------------------------------------------------------------- options
def _cfg(**misc):
    return {"misc": misc}


def test_options_default_to_off_and_parse():
    off = mdcfg.muon_options({})
    assert off["enabled"] is False and mdcfg.muon_options(_cfg(muon=False))["enabled"] is False
    assert mdcfg.muon_options(_cfg(muon=None))["enabled"] is False
    on = mdcfg.muon_options(_cfg(muon=True))
    assert on == {"enabled": True, "momentum": 0.95, "nesterov": True, "ns_steps": 5, "adjust": "rms",
                  "targets": list(muon.DEFAULT_TARGETS), "adamw_lr": None}
    full = mdcfg.muon_options(_cfg(muon=True, muon_momentum=0.9, muon_nesterov=False, muon_ns_steps=3, muon_adjust="spectral",
                                   muon_targets=r"attn\.qkv\.weight$", muon_adamw_lr=1e-4))
    assert full == {"enabled": True, "momentum": 0.9, "nesterov": False, "ns_steps": 3, "adjust": "spectral",
                    "targets": [r"attn\.qkv\.weight$"], "adamw_lr": 1e-4}


@pytest.mark.parametrize("misc", [
    dict(muon="yes"), dict(muon=1),
    dict(muon_momentum=0.9), dict(muon_nesterov=True), dict(muon_ns_steps=5), dict(muon_adjust="rms"), dict(muon_targets=["x"]),
    dict(muon_adamw_lr=1e-4), dict(muon=False, muon_ns_steps=5),
    dict(muon=True, muon_momentum=1.0), dict(muon=True, muon_momentum=-0.1), dict(muon=True, muon_momentum="0.9"),
    dict(muon=True, muon_momentum=True), dict(muon=True, muon_nesterov=1), dict(muon=True, muon_ns_steps=0),
    dict(muon=True, muon_ns_steps=9), dict(muon=True, muon_ns_steps=5.0), dict(muon=True, muon_adjust="frobenius"),
    dict(muon=True, muon_targets=[]), dict(muon=True, muon_targets=[3]), dict(muon=True, muon_targets=["("]),
    dict(muon=True, muon_adamw_lr=-1.0), dict(muon=True, muon_adamw_lr=float("inf")), dict(muon=True, lora_rank=8),
])
def test_option_misuse_raises(misc):
    with pytest.raises(ValueError, match="muon"):
        mdcfg.muon_options(_cfg(**misc))


def test_reference_yamls_parse_unchanged_and_leave_muon_off():
    for name in ("res_256_pretrain", "res_256_finetune", "res_512_pretrain", "res_512_finetune"):
        cfg = mdcfg.load_config(os.path.join(ROOT, "configs"), name)
        assert mdcfg.muon_options(cfg)["enabled"] is False
        assert not any(k.startswith("muon") for k in (cfg.get("misc") or {}))
        on = mdcfg.load_config(os.path.join(ROOT, "configs"), name, ["misc.muon=true", "misc.muon_ns_steps=4"])
        assert mdcfg.muon_options(on)["enabled"] is True and mdcfg.muon_options(on)["ns_steps"] == 4


def test_train_py_builds_muon_behind_the_switch():
    src = open(os.path.join(ROOT, "train.py")).read()
    assert "mdcfg.muon_options(cfg)" in src and re.search(r'elif muon\["enabled"\]:\s*\n(.*\n){0,6}\s*opt = Muon\(model\.dit', src)


# ---------------------------------------------------------------------------------------------------- targets and the split
def _split(table):
    specs = muon.resolve_targets(table, muon.DEFAULT_TARGETS)
    offs, total = mdit.flat_layout(table)
    return specs, muon.matrices_of(specs, offs), muon.complement_runs(specs, offs, total), offs, total


def _assert_tiles_once(table, specs, mats, runs, offs, total):
    cover = np.zeros(total, dtype=np.int8)
    for o, r, c, _ in mats:
        assert o % 8 == 0 and r % 64 == 0 and c % 64 == 0
        cover[o:o + r * c] += 1
    for o, n in runs:
        assert o % 4 == 0 and n % 4 == 0 and n > 0
        cover[o:o + n] += 1
    assert int(cover.min()) == 1 == int(cover.max()), "targets and complement runs must tile the flat buffers exactly once"
    assert all(a + n < b for (a, n), (b, _) in zip(runs, runs[1:])), "adjacent runs must be merged"
    targeted = {s.name for s in specs}
    for s in table:                      # every non-targeted parameter lies inside one run
        if s.buffer or s.name in targeted:
            continue
        o, n = offs[s.name], int(np.prod(s.shape))
        assert any(a <= o and o + n <= a + cnt for a, cnt in runs), s.name


def test_default_targets_on_xl2():
    table = _xl2_table()
    specs, mats, runs, offs, total = _split(table)
    assert len(specs) == 256 and len(mats) == 480 and len(runs) == 18
    assert sum(r * c for _, r, c, _ in mats) == 937_426_944
    assert all(r % 128 == 0 and c % 128 == 0 for _, r, c, _ in mats)
    _assert_tiles_once(table, specs, mats, runs, offs, total)
    for s in specs:
        assert re.match(r"(patch_mixer|blocks)\.\d+\.(attn\.(qkv|proj)|cross_attn\.(q_linear|kv_linear|proj)|mlp\.w[123])(\.weight)?$", s.name)
    names = {s.name for s in specs}
    for s in table:
        if any(k in s.name for k in ("mlp.gate", "adaLN_modulation", "embedder", "y_emb_preprocess", "pooled_y_emb_process", "final_layer",
                                     "patch_mixer_map")) or len(s.shape) == 1:
            assert s.name not in names, s.name


def test_default_targets_on_tiny_2_and_tiny(tiny):
    table = _tiny2_table()
    specs, mats, runs, offs, total = _split(table)
    assert len(mats) == len(specs) + 7 * sum(len(s.shape) == 3 for s in specs)
    _assert_tiles_once(table, specs, mats, runs, offs, total)
    o = muon.Muon(tiny, device="cpu")
    _assert_tiles_once(tiny._table, o.specs, o.matrices, o.runs, *mdit.flat_layout(tiny._table))
    assert set(o.rules.values()) == {"muon", "adamw"} and sum(v == "muon" for v in o.rules.values()) == len(o.specs)


def test_bad_targets_raise(tiny):
    t = tiny._table
    for bad, why in (([r"nothing_like_this"], "matches no parameter"), ([r"^pos_embed$"], "buffer"), ([r"x_embedder\.proj\.weight"], "only 2-D"),
                     ([r"blocks\.0\.norm1\.weight"], "only 2-D"), ([r"t_embedder\.mlp\.0\.bias"], "only 2-D"), ([], "non-empty"),
                     ("attn", "non-empty")):
        with pytest.raises(ValueError, match=why):
            muon.resolve_targets(t, bad)
    # a matrix dimension that is not a multiple of 64: the router [experts, dim] and the final projection [patch_vec, dim]
    for bad in ([r"mlp\.gate\.weight"], [r"final_layer\.linear\.weight"]):
        with pytest.raises(ValueError, match="multiples of 64"):
            muon.resolve_targets(t, bad)
    with pytest.raises(ValueError, match="multiples of 64"):
        muon.Muon(tiny, targets=[r"mlp\.gate\.weight"], device="cpu")


def test_constructor_refusals_come_first(tiny):
    for kw in (dict(momentum=1.0), dict(nesterov=1), dict(ns_steps=0), dict(ns_steps=9), dict(adjust="x"), dict(adamw_lr=-1)):
        with pytest.raises(ValueError, match="muon"):
            muon.Muon(tiny, device="cpu", **kw)
    tiny._lora = object()
    try:
        with pytest.raises(NotImplementedError, match="LoRA"):
            muon.Muon(tiny, device="cpu")
    finally:
        tiny._lora = None
    o = muon.Muon(tiny, device="cpu")
    assert o.shardable is False
    with pytest.raises(NotImplementedError, match="sharded"):
        o.step_sharded(None)
    with pytest.raises(RuntimeError, match="GPU"):
        o.step()


# ---------------------------------------------------------------------------------------------------- shape factors
@pytest.mark.parametrize("rows,cols", [(256, 1024), (1024, 256), (512, 512)])
def test_scale_formulas(rows, cols, tiny):
    assert muon.shape_scale("rms", rows, cols) == pytest.approx(0.2 * math.sqrt(max(rows, cols)), rel=1e-15)
    assert muon.shape_scale("spectral", rows, cols) == pytest.approx(math.sqrt(max(1.0, rows / cols)), rel=1e-15)
    assert muon.shape_scale("spectral", 256, 1024) == 1.0 and muon.shape_scale("spectral", 1024, 256) == 2.0
    assert muon.shape_scale("rms", 1024, 256) == muon.shape_scale("rms", 256, 1024) == pytest.approx(6.4)
    with pytest.raises(ValueError):
        muon.shape_scale("other", rows, cols)
    o = muon.Muon(tiny, ns_steps=3, adjust="spectral", device="cpu")
    assert o.item_scale(rows, cols) == muon.shape_scale("spectral", rows, cols)


# ---------------------------------------------------------------------------------------------------- state
def test_state_dict_round_trip_and_rule_table(tiny):
    a = muon.Muon(tiny, momentum=0.9, ns_steps=4, ema_smoothing=0.99, posthoc_sigma_rels=(0.05,), device="cpu")
    gen = torch.Generator().manual_seed(3)
    a.m.copy_(torch.randn(a.m.shape, generator=gen))
    a.ema.copy_(torch.randn(a.m.shape, generator=gen))
    a.posthoc[0].copy_(torch.randn(a.m.shape, generator=gen))
    a.step_count, a.ema_live = 7, True
    sd = a.state_dict()
    assert sd["format"] == "by_name" and set(sd["m"]) == {s.name for s in tiny._table if not s.buffer} == set(sd["muon"]["rules"])
    assert sd["muon"]["momentum"] == 0.9 and sd["muon"]["ns_steps"] == 4 and sd["muon"]["adjust"] == "rms" and sd["muon"]["nesterov"] is True
    name = a.specs[0].name
    assert sd["muon"]["rules"][name] == "muon" and sd["muon"]["rules"]["final_layer.linear.weight"] == "adamw"
    assert sd["m"][name].shape == tuple(a.specs[0].shape)
    b = muon.Muon(tiny, momentum=0.9, ns_steps=4, ema_smoothing=0.99, posthoc_sigma_rels=(0.05,), device="cpu")
    b.load_state_dict(sd)
    assert b.step_count == 7 and b.ema_live
    for fa, fb in ((a.m, b.m), (a.v, b.v), (a.ema, b.ema), (a.posthoc[0], b.posthoc[0])):      # (the alignment padding is no state)
        va, vb = a._by_name(fa), b._by_name(fb)
        assert all(torch.equal(va[n], vb[n]) for n in va)
    assert not torch.equal(b._by_name(b.m)[name], torch.zeros_like(sd["m"][name]))
    # other targets: another rule table
    other = muon.Muon(tiny, targets=[r"attn\.qkv\.weight$"], device="cpu")
    with pytest.raises(RuntimeError, match="rule table"):
        other.load_state_dict(sd)
    # a plain FusedAdamW state carries none
    plain = {k: v for k, v in sd.items() if k != "muon"}
    with pytest.raises(RuntimeError, match="rule table"):
        b.load_state_dict(plain)
    with pytest.warns(UserWarning, match="momentum continues"):
        muon.Muon(tiny, momentum=0.8, ns_steps=4, device="cpu").load_state_dict({k: v for k, v in sd.items() if k not in ("ema", "posthoc")})


# ---------------------------------------------------------------------------------------------------- plumbing
def test_symbols_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "microdit_hip.h")).read()
    for name in SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared"
        assert name in hip.exported_symbols(), f"{name} is not bound in hip._SIGS"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(hip._SIGS[name][1]), name
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6
    assert re.search(r"#define MD_MUON_NORM_PARTS 16\b", header) and hip.MUON_NORM_PARTS == 16 == ref.NORM_PARTS
    import ctypes
    assert ctypes.sizeof(hip.MuonItem) == 32
    assert "4.20" in open(os.path.join(ROOT, "DESIGN.md")).read() and "Muon" in open(os.path.join(ROOT, "README.md")).read()


# ---------------------------------------------------------------------------------------------------- the reference models
def test_fma32_is_one_rounding():
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(20000, generator=gen)
    x = torch.randn(20000, generator=gen)
    y = -(a.double() * x.double()).float() * (1 + torch.randn(20000, generator=gen) * 1e-3)        # heavy cancellation
    got = ref.fma32(a, x, y)
    from fractions import Fraction

    def round32(fr):                    # the fp32 neighbour of float(fr) nearest to the exact rational, a tie to the even mantissa
        c = np.float32(float(fr))
        cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
        return float(min(cands, key=lambda v: (abs(Fraction(float(v)) - fr), int(np.float32(v).view(np.uint32)) & 1)))

    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(x[i])) + Fraction(float(y[i]))
        assert float(got[i]) == round32(exact), i
    assert torch.equal(ref.fma32(0.5, x, torch.zeros_like(x)), 0.5 * x)
    # the fp64 sum lands exactly on an fp32 tie, the exact sum just below it: 1 + 2^-23 + 2^-24 - 2^-70 rounds DOWN to 1 + 2^-23, where
    # rounding the fp64 sum (a tie, to even) would give 1 + 2^-22
    a1, x1, y1 = torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([(1.0 - 2.0 ** -23) * 2.0 ** -24]), torch.tensor([1.0 + 2.0 ** -23])
    assert float((a1.double() * x1.double() + y1.double()).float()) == 1.0 + 2.0 ** -22
    assert float(ref.fma32(a1, x1, y1)) == 1.0 + 2.0 ** -23
    assert float(ref.fma32(a1, -x1, -y1)) == -(1.0 + 2.0 ** -23)


def test_newton_schulz_inputs_stay_in_the_converged_regime():
    xs = ref.ns_inputs()
    assert [tuple(x.shape) for x in xs] == list(ref.SHAPES)
    assert torch.equal(xs[2], xs[1].t())                      # the tall input is the transpose of the wide one
    for x in xs:
        sv = torch.linalg.svdvals(ref.ns_fp64(x))
        print(tuple(x.shape), "singular values of ns_fp64 in", [round(float(sv.min()), 3), round(float(sv.max()), 3)])
        assert float(sv.min()) >= 0.5 and float(sv.max()) <= 1.3
        e = ref.rel_err(ref.ns_bf16_emulated(x), ref.ns_fp64(x))
        print("   e_emu", e)
        assert 1e-3 < e < 3e-2
    # what must NOT be used for the error bound: a Gaussian square matrix leaves the regime
    g = torch.Generator().manual_seed(1)
    sq = torch.randn(64, 64, generator=g, dtype=torch.float64)
    assert float(torch.linalg.svdvals(ref.ns_fp64(sq / sq.norm())).min()) < 0.5
    # orientation: the tall form is the transpose of the wide one
    assert ref.rel_err(ref.ns_bf16_emulated(xs[2], 1), ref.ns_bf16_emulated(xs[1], 1).t()) < 1e-2
    assert torch.allclose(ref.ns_fp64(xs[2]), ref.ns_fp64(xs[1]).t())


def test_reference_momentum_and_apply_restate_the_formulas():
    gen = torch.Generator().manual_seed(9)
    g, m, p = (torch.randn(4096, generator=gen) for _ in range(3))
    coef = ref.clip_coef(0.5, 37.0, 0.25)
    assert coef == pytest.approx(0.5 * 0.25 / (math.sqrt(37.0) * 0.5 + 1e-6), rel=1e-6) and ref.clip_coef(0.5) == 0.5
    mn, u = ref.momentum_ref(g, m, coef, 0.95, True)
    assert torch.allclose(mn.double(), 0.95 * m.double() + coef * g.double(), rtol=1e-6, atol=1e-7)
    assert torch.allclose(u.double(), coef * g.double() + 0.95 * mn.double(), rtol=1e-6, atol=1e-7)
    assert torch.equal(ref.momentum_ref(g, m, coef, 0.95, False)[1], mn)
    nrm, inv, x = ref.normalise_ref(u)
    assert abs(float(x.double().norm()) - 1.0) < 5e-3 and inv == pytest.approx(1 / math.sqrt(nrm), rel=1e-6)
    o = torch.randn(4096, generator=gen).to(torch.bfloat16)
    assert ref.decay_is_unambiguous(2.0 ** -10, 0.25)
    pn, sh, e = ref.apply_ref(p, o, 2.0 ** -10, 0.25, 6.4, 2, 0.75, g)
    want = p.double() * (1 - 2.0 ** -12) - 2.0 ** -10 * 6.4 * o.double()
    assert torch.allclose(pn.double(), want, rtol=1e-6, atol=1e-7) and torch.equal(sh, pn.to(torch.bfloat16))
    assert torch.allclose(e.double(), 0.75 * g.double() + 0.25 * pn.double(), rtol=1e-6, atol=1e-7)
    assert torch.equal(ref.apply_ref(p, o, 2.0 ** -10, 0.25, 6.4, 1)[2], pn)
    items, total = ref.layout()
    assert all(o % 8 == 0 for o, _, _ in items) and all(a[0] + a[1] * a[2] <= b[0] for a, b in zip(items, items[1:]))
    assert items[4][0] + 64 * 128 == items[5][0], "the two experts are adjacent"
