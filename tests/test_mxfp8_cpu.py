"""MXFP8 sampling, the parts that need no GPU: the reference's own properties, the ABI, the sampler's refusals, the
compiled resources of the two new files and the target selection."""
import os
import re

import pytest
import torch

from micro_diffusion_amd import hip, native, samplers
from tests import mx_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("md_mx_quant_rows", "md_gemm_mxfp8", "md_swiglu_fwd_mx")


# ------------------------------------------------------------------------------------------------------------------ reference
def _roundtrip(x):
    q, s = mx_ref.mx_quantize(x.to(torch.bfloat16))
    return mx_ref.mx_dequantize(q, s), q, s


def test_reference_powers_of_two_and_small_integers_round_trip():
    p2 = torch.exp2(torch.arange(-40, 40).float()).reshape(-1, 1) * torch.ones(1, 32)         # one power of two per block
    assert torch.equal(_roundtrip(p2)[0], p2.double())
    mixed = torch.exp2(torch.arange(-3, 5).float()).repeat(4).reshape(1, 32)                   # 2^-3 ... 2^4 in one block: 8 octaves
    assert torch.equal(_roundtrip(mixed)[0], mixed.double())
    ints = torch.arange(-16, 16).float().reshape(1, 32)
    assert torch.equal(_roundtrip(ints)[0], ints.double())
    ints = torch.arange(1, 17).float().repeat(2).reshape(1, 32) * 2.0 ** 20                    # ... at another scale
    assert torch.equal(_roundtrip(ints)[0], ints.double())


def test_reference_error_bound_per_block():
    """|x - deq| <= 2^-4 * 2^floor(log2 amax) per block: with X = floor(log2 amax) - 8 the scaled values lie below 2^9, where e4m3 steps
    by at most 32, so rounding errs by at most 16 * 2^X.  The bound cannot hold for an element the rule's clamp saturates -- a scaled
    magnitude in (464, 512) goes to 448, up to 64 * 2^X = 2^-2 * 2^floor(log2 amax) away -- so those elements (only ones within a factor
    1.1 of amax can be) are held to that figure instead; every other element is held to the 2^-4 bound."""
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 8, 32, generator=g) * torch.exp2(torch.randint(-30, 30, (64, 8, 1), generator=g).float())).to(torch.bfloat16)
    deq, q, s = _roundtrip(x.reshape(64, 256))
    xb = x.double()
    amax = xb.abs().amax(-1, keepdim=True)
    step = torch.exp2(torch.floor(torch.log2(amax)))
    err = (xb - deq.reshape(64, 8, 32)).abs()
    saturated = xb.abs() > 464.0 * step / 256.0
    assert bool(saturated.any()) and bool((~saturated).any())
    assert bool((err[~saturated] <= (2.0 ** -4 * step).expand_as(err)[~saturated]).all())
    assert bool((err[saturated] < (2.0 ** -2 * step).expand_as(err)[saturated]).all())
    assert not bool(torch.isnan(q.float()).any())


@pytest.mark.parametrize("j", (-20, -1, 0, 7, 30))
def test_reference_saturation_case(j):
    x = torch.zeros(1, 32)
    x[0, 3], x[0, 4], x[0, 9] = 460.0 * 2.0 ** j, -460.0 * 2.0 ** j, 500.0 * 2.0 ** j
    x[0, 9] = float(torch.tensor(500.0 * 2.0 ** j).to(torch.bfloat16))                       # 500 -> 500 (bf16: 1.953125 * 2^8)
    deq, q, s = _roundtrip(x)
    assert int(s[0, 0]) == 127 + j                                                             # floor(log2 amax) = 8 + j
    assert not bool(torch.isnan(q.float()).any())
    assert deq[0, 3] == 448.0 * 2.0 ** j and deq[0, 4] == -448.0 * 2.0 ** j and deq[0, 9] == 448.0 * 2.0 ** j


def test_reference_zero_block():
    x = torch.randn(2, 64)
    x[1, 32:] = 0
    deq, q, s = _roundtrip(x)
    assert int(s[1, 1]) == 0 and bool((q.view(torch.uint8)[1, 32:] == 0).all()) and bool((deq[1, 32:] == 0).all())
    assert int(s[1, 0]) != 0


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_header_declares_and_binding_matches():
    header = open(os.path.join(ROOT, "include", "microdit_hip.h")).read()
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6
    for name in SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in the header"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in hip._SIGS, f"{name} is not bound in hip.py"
        assert len(hip._SIGS[name][1]) == n_args, (name, n_args, len(hip._SIGS[name][1]))
    # md_gemm_mx_args: the ctypes structure has the header's fields, in order
    body = re.search(r"typedef struct md_gemm_mx_args \{(.*?)\} md_gemm_mx_args;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip().lstrip("*") for f in re.sub(r"^(const\s+)?\w+\s*\*?\s*", "", decl, count=1).split(",")]
    assert fields == [f[0] for f in hip.GemmMxArgs._fields_], fields


# ------------------------------------------------------------------------------------------------------------------ sampler
class _FakeMX:
    entries = {}

    def check_fresh(self, v):
        pass

    def requantize(self):
        return self


def test_check_mxfp8_accepts_and_refuses():
    assert samplers.check_mxfp8(None) is False
    assert samplers.check_mxfp8(None, measurement=object()) is False
    assert samplers.check_mxfp8(True) is True
    assert samplers.check_mxfp8(_FakeMX()) is True
    for bad in (False, 1, "yes", object(), {"entries": {}}):
        with pytest.raises(ValueError):
            samplers.check_mxfp8(bad)
    with pytest.raises(ValueError, match="measurement"):
        samplers.check_mxfp8(True, measurement=object())
    with pytest.raises(ValueError, match="guidance_loss"):
        samplers.check_mxfp8(_FakeMX(), guidance_loss=lambda d: d)


def test_request_carries_mxfp8_and_checks_it():
    from micro_diffusion_amd import sampling
    assert sampling.Request().mxfp8 is None
    import inspect
    from micro_diffusion_amd.model import LatentDiffusion
    for fn in (LatentDiffusion.edm_sampler_loop, LatentDiffusion.generate):
        assert inspect.signature(fn).parameters["mxfp8"].default is None


# ------------------------------------------------------------------------------------------------------------------ resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_kernel_resources(tmp_path):
    res = {}
    for f in ("gemm_mxfp8.hip", "mx_quant.hip"):
        res.update(native.resource_usage(f, hip.HIPCC_FLAGS, tmp_path / (f + ".o")))
    assert len(res) == 4, sorted(res)                     # the GEMM, the two quantisers, the MX-writing SwiGLU
    for name, v in res.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (name, v)
    gemm = next(v for k, v in res.items() if "gemm_mxfp8_kernel" in k)
    assert gemm["lds"] <= 64 * 1024 and gemm["occ"] >= 1


# ------------------------------------------------------------------------------------------------------------------ targets
def _tiny_config():
    from micro_diffusion_amd.dit import MicroDiT_Tiny_2
    return MicroDiT_Tiny_2(input_size=8).config


def test_targets_name_the_block_linears_and_nothing_else():
    """The quantisable set (targets=ALL_TARGETS) is the linears of every patch-mixer and backbone block.  The default set is that set
    minus the classes that lost their measurement by more than the noise floor (mxfp8.DEFAULT_EXCLUDED, with the numbers): a subset,
    and never one of the excluded layers."""
    from micro_diffusion_amd import mxfp8
    from micro_diffusion_amd.arch import param_table, plan_blocks
    cfg = _tiny_config()
    names = mxfp8.target_names(cfg, mxfp8.ALL_TARGETS)
    default = mxfp8.target_names(cfg)
    assert set(default) <= set(names) and default == [n for n in names if not mxfp8.DEFAULT_EXCLUDED.search(n)]
    mixer, backbone = plan_blocks(cfg)
    want = []
    for bp in list(mixer) + list(backbone):
        want += [bp.name + s for s in (".attn.qkv", ".attn.proj", ".cross_attn.q_linear", ".cross_attn.proj")]
        want += [bp.name + ".mlp.w1", bp.name + ".mlp.w2"] + ([] if bp.moe else [bp.name + ".mlp.w3"])
    assert sorted(names) == sorted(want)
    table = {s.name for s in param_table(cfg)}
    for n in names:                                           # every name is a weight of the model: a linear's or an expert tensor
        assert (n + ".weight") in table or n in table
    for n in names:
        for never in ("adaLN_modulation", "gate", "kv_linear", "y_embedder", "y_emb_preprocess", "pooled_y_emb_process", "x_embedder",
                      "t_embedder", "final_layer", "norm"):
            assert never not in n, n


def test_targets_is_a_regular_expression_over_the_quantisable_set():
    from micro_diffusion_amd import mxfp8
    cfg = _tiny_config()
    assert mxfp8.target_names(cfg, r"$^") == []
    qkv = mxfp8.target_names(cfg, r"attn\.qkv$")
    assert qkv and all(n.endswith(".attn.qkv") for n in qkv)
    # a pattern that also matches excluded layers still selects none of them
    everything = mxfp8.target_names(cfg, r".")
    assert everything == mxfp8.target_names(cfg, mxfp8.ALL_TARGETS) and not any("kv_linear" in n or "adaLN" in n or ".gate" in n for n in everything)
    assert mxfp8.eligible(512, 512) and not mxfp8.eligible(512, 320) and not mxfp8.eligible(8, 512)
