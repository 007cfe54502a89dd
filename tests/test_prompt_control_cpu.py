"""Prompt control, host side (no GPU): every request check_prompt_control refuses and that both public functions refuse
before anything runs, the log of the weights and the layout of a run's bias buffer, the surface (signatures, header, binding, library)
and the compiled resources of the kernels the feature adds or touches."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from micro_diffusion_amd import hip, native, samplers, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("md_attn_fwd_kbias", "md_attn_probs_kbias")
B, LC, DC = 3, 77, 16
Y_SHAPE = (B, 1, LC, DC)


def _ok_weights():
    w = torch.ones(B, LC)
    w[:, 60:] = 0
    return w


# ------------------------------------------------------------------------------------------------ what is defined, what is refused
def test_check_accepts_what_is_defined():
    chk = samplers.check_prompt_control
    assert chk() is False
    assert chk(True, cfg=3.0) is False                                        # a negative prompt alone arms no bias
    assert chk(False, _ok_weights(), cfg=1.0, y_shape=Y_SHAPE) is True        # weights do not need guidance
    neg = torch.zeros(Y_SHAPE)
    for w in (_ok_weights(), _ok_weights()[:1], _ok_weights()[0], _ok_weights().bool(), _ok_weights().half(), _ok_weights().double(),
              _ok_weights().to(torch.bfloat16)):
        assert chk(False, w, w, 3.0, negative=neg, y_shape=Y_SHAPE) is True
    assert chk(negative=neg[:1], cfg=3.0, y_shape=Y_SHAPE) is False           # a leading 1 is broadcast
    assert chk(True, cfg=3.0, measurement=object()) is False                  # a negative prompt composes with measurement guidance
    assert chk(True, cfg=3.0, guidance_loss=lambda d: d) is False
    assert chk(False, will_weight=True) is True                               # generate's mask_padding before it has a mask


@pytest.mark.parametrize("kw,match", [
    (dict(caption_weights=torch.ones(B, LC + 1), y_shape=Y_SHAPE), "shape"),
    (dict(caption_weights=torch.ones(B + 1, LC), y_shape=Y_SHAPE), "shape"),
    (dict(caption_weights=torch.ones(1, B, LC), y_shape=Y_SHAPE), "shape"),
    (dict(caption_weights=torch.ones(B, LC, dtype=torch.int64), y_shape=Y_SHAPE), "bool or floating"),
    (dict(caption_weights=[1.0] * LC, y_shape=Y_SHAPE), "tensor"),
    (dict(caption_weights=torch.full((B, LC), -0.5)), ">= 0"),
    (dict(caption_weights=torch.full((LC,), float("nan"))), "finite"),
    (dict(caption_weights=torch.full((LC,), float("inf"))), "finite"),
    (dict(caption_weights=torch.cat([torch.ones(2, LC), torch.zeros(1, LC)])), "at least one weight > 0"),
    (dict(caption_weights=torch.zeros(LC, dtype=torch.bool)), "at least one weight > 0"),
    (dict(has_negative=True, cfg=1.0), "cfg > 1"),
    (dict(negative=torch.zeros(Y_SHAPE), cfg=0.5), "cfg > 1"),
    (dict(negative_weights=torch.ones(LC), cfg=3.0), "needs negative"),
    (dict(negative=torch.zeros(B, 1, LC + 1, DC), cfg=3.0, y_shape=Y_SHAPE), "negative has shape"),
    (dict(negative=torch.zeros(2, 1, LC, DC), cfg=3.0, y_shape=Y_SHAPE), "negative has shape"),
    (dict(negative=torch.zeros(B, LC, DC), cfg=3.0, y_shape=Y_SHAPE), "negative has shape"),
    (dict(has_negative=True, cfg=3.0, negative_weights=torch.full((LC,), -1.0)), ">= 0"),
    (dict(has_negative=True, cfg=3.0, guide=object()), "guide"),
    (dict(caption_weights=torch.ones(LC), guide=object()), "guide"),
    (dict(has_negative=True, cfg=3.0, negative_weights=torch.ones(LC), guide=object()), "guide"),
    (dict(caption_weights=torch.ones(LC), measurement=object()), "measurement"),
    (dict(caption_weights=torch.ones(LC), guidance_loss=lambda d: d), "measurement"),
    (dict(has_negative=True, cfg=3.0, negative_weights=torch.ones(LC), measurement=object()), "measurement"),
    (dict(will_weight=True, measurement=object()), "measurement"),
])
def test_check_refuses(kw, match):
    with pytest.raises(ValueError, match=match):
        samplers.check_prompt_control(**kw)


def test_requests_are_refused_before_anything_runs():
    """Both public functions check the request first: no parameters, device, tokenizer or text encoder is touched (self is not a model)."""
    from micro_diffusion_amd.model import LatentDiffusion

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    class Stub:
        edm_config = Cfg(S_churn=0, num_steps=4)
        dit = None
    x, y = torch.zeros(B, 4, 8, 8), torch.zeros(Y_SHAPE)
    loop = [(dict(caption_weights=torch.ones(LC + 3)), "shape"), (dict(caption_weights=-torch.ones(LC)), ">= 0"),
            (dict(caption_weights=torch.zeros(LC)), "at least one weight > 0"), (dict(negative=torch.zeros(2, 1, LC, DC)), "negative has shape"),
            (dict(negative_weights=torch.ones(LC)), "needs negative"), (dict(caption_weights=torch.ones(LC), guidance_loss=lambda d: d), "measurement")]
    for kw, match in loop:
        with pytest.raises(ValueError, match=match):
            LatentDiffusion.edm_sampler_loop(Stub(), x, y, 4, 3.0, **kw)
    with pytest.raises(ValueError, match="cfg > 1"):
        LatentDiffusion.edm_sampler_loop(Stub(), x, y, 4, 1.0, negative=torch.zeros(Y_SHAPE))
    gen = [(dict(caption_weights=-torch.ones(LC)), ">= 0"), (dict(negative_weights=torch.ones(LC)), "needs negative"),
           (dict(negative_prompt=["blurry"], guidance_scale=1.0), "cfg > 1"),
           (dict(negative_tokenized_prompts=torch.zeros(1, LC, dtype=torch.long), guidance_scale=0.0), "cfg > 1"),
           (dict(mask_padding=True, guidance_loss=lambda d: d), "measurement"),
           (dict(mask_padding=True, tokenized_prompts=torch.zeros(1, LC, dtype=torch.long)), "attention_mask"),
           (dict(mask_padding=True, negative_tokenized_prompts=torch.zeros(1, LC, dtype=torch.long)), "attention_mask")]
    for kw, match in gen:
        with pytest.raises(ValueError, match=match):
            LatentDiffusion.generate(Stub(), ["a prompt"], **kw)


def test_request_check_passes_the_caption_shape_on():
    from types import SimpleNamespace
    model = SimpleNamespace(edm_config=SimpleNamespace(S_churn=0.0), dit=SimpleNamespace(config=None))
    sampling.Request(caption_weights=torch.ones(LC)).check(model, None, 1.0)
    sampling.Request(caption_weights=torch.ones(LC)).check(model, (B, 4, 8, 8), 1.0, y_shape=Y_SHAPE)
    with pytest.raises(ValueError, match="shape"):
        sampling.Request(caption_weights=torch.ones(LC)).check(model, (B, 4, 8, 8), 1.0, y_shape=(B, 1, LC + 1, DC))
    with pytest.raises(ValueError, match="cfg > 1"):
        sampling.Request().check(model, None, 1.0, has_negative=True)


def test_bias_context_puts_back_what_the_engine_held():
    from types import SimpleNamespace
    by_hand, run_bias = torch.zeros(B, 80), torch.ones(2 * B, 80)
    for before in (None, by_hand):
        dit = SimpleNamespace(engine=SimpleNamespace(caption_bias=before))
        with sampling.caption_bias(dit, run_bias):
            assert dit.engine.caption_bias is run_bias
        assert dit.engine.caption_bias is before
        with pytest.raises(RuntimeError, match="boom"):
            with sampling.caption_bias(dit, run_bias):
                raise RuntimeError("boom")
        assert dit.engine.caption_bias is before
        with sampling.caption_bias(dit, None):                                # a run without weights touches nothing
            assert dit.engine.caption_bias is before


# ------------------------------------------------------------------------------------------------ the bias
def test_log_of_the_weights_and_broadcasting():
    w = torch.tensor([1.0, 0.0, 2.0, 0.5] + [1.0] * (LC - 4))
    for form in (w, w[None], w[None].expand(B, LC), w.double(), w.half()):
        b = samplers.caption_log_bias(form, B, LC)
        assert b.shape == (B, LC) and b.dtype == torch.float32
        assert torch.equal(b, torch.log(w.to(torch.float32))[None].expand(B, LC))
    b = samplers.caption_log_bias(w, B, LC)
    assert b[0, 0] == 0 and b[0, 1] == float("-inf") and abs(float(b[0, 2]) - math.log(2.0)) < 1e-7
    assert float(b[0, 3]) == -float(b[0, 2])
    keep = torch.arange(LC) < 20
    bb = samplers.caption_log_bias(keep, B, LC)                               # bool: 0 where kept, -inf where removed
    assert bool((bb[:, :20] == 0).all()) and bool((bb[:, 20:] == float("-inf")).all())
    per_sample = torch.rand(B, LC) + 0.1
    assert torch.equal(samplers.caption_log_bias(per_sample, B, LC), torch.log(per_sample))


def test_layout_of_the_bias_buffer():
    cw, nw = torch.rand(B, LC) + 0.5, torch.rand(1, LC) + 0.5
    cw[1, 70:] = 0
    for Lc in (LC, 76, 5):
        ldb = (Lc + 3) // 4 * 4
        c, n = cw[:, :Lc].contiguous(), nw[:, :Lc].contiguous()
        both = samplers.caption_bias_buffer(c, n, B, Lc, True)
        assert both.shape == (2 * B, ldb) and both.dtype == torch.float32 and both.is_contiguous() and ldb % 4 == 0 and ldb - Lc < 4
        assert torch.equal(both[:B, :Lc], torch.log(c)) and torch.equal(both[B:, :Lc], torch.log(n).expand(B, Lc))
        assert bool((both[:, Lc:] == 0).all()), "the pad columns hold 0"
        only_c = samplers.caption_bias_buffer(c, None, B, Lc, True)
        assert torch.equal(only_c[:B], both[:B]) and bool((only_c[B:] == 0).all()), "a second half without weights holds 0"
        only_n = samplers.caption_bias_buffer(None, n, B, Lc, True)
        assert bool((only_n[:B] == 0).all()) and torch.equal(only_n[B:], both[B:])
        single = samplers.caption_bias_buffer(c, n, B, Lc, False)              # nothing is doubled: the first half alone
        assert single.shape == (B, ldb) and torch.equal(single, both[:B])


# ------------------------------------------------------------------------------------------------ the surface
def test_signatures_and_defaults():
    from micro_diffusion_amd.dit import DiT
    from micro_diffusion_amd.model import LatentDiffusion
    loop = dict(negative=None, caption_weights=None, negative_weights=None)
    gen = dict(negative_prompt=None, negative_tokenized_prompts=None, negative_attention_mask=None, caption_weights=None,
               negative_weights=None, mask_padding=False)
    for fn, want in ((LatentDiffusion.edm_sampler_loop, loop), (LatentDiffusion.generate, gen), (DiT.forward_with_cfg, dict(negative=None))):
        p = inspect.signature(fn).parameters
        for name, default in want.items():
            assert name in p, f"{fn.__name__} lacks {name}"
            assert p[name].default is default, (fn.__name__, name, p[name].default)
            assert p[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert [k for k, v in p.items() if v.kind is inspect.Parameter.VAR_KEYWORD] == ["kwargs"]
    req = sampling.Request()
    assert req.negative is None and req.caption_weights is None and req.negative_weights is None
    # generate hands vars(request) to edm_sampler_loop: every field must be one of its named parameters
    assert set(vars(req)) <= set(inspect.signature(LatentDiffusion.edm_sampler_loop).parameters)


def _declaration(header, name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/microdit_hip.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "microdit_hip.h")).read()
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6, "two symbols added, none changed: the ABI version stays"
    for name in NAMES:
        declared = _declaration(header, name)
        assert name in hip.exported_symbols() and name in hip._SIGS, f"{name} is not bound in hip._SIGS"
        restype, argtypes = hip._SIGS[name]
        assert len(declared) == len(argtypes), (name, len(declared), len(argtypes))
        assert declared[-1].split()[0] == "hipStream_t"
        for text, ctype in zip(declared, argtypes):
            if "*" in text or "hipStream_t" in text:
                assert ctype is ctypes.c_void_p or ctype is ctypes.POINTER(hip.AttnArgs), (name, text)
            else:
                assert {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}[text.split()[-2]] is ctype, (name, text)
    assert hip.ATTN_KBIAS_MAX_KEYS == 256


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_built_library_exports_the_entry_points():
    lib = ctypes.CDLL(hip.build())
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert lib.md_abi_version() == 6


# ------------------------------------------------------------------------------------------------ compiled resources
# VGPRs of attn_fwd_kernel<HD, MAXIT> at the parent commit: the plain forward must not pay for the bias form
PLAIN_VGPRS = {(32, 1): 76, (32, 2): 98, (32, 4): 120, (64, 1): 92, (64, 2): 122, (64, 4): 142}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_forward_kernel_resources(tmp_path):
    res = native.resource_usage("attention.hip", hip.HIPCC_FLAGS, tmp_path / "attn.o")
    for (hd, it), vgprs in PLAIN_VGPRS.items():
        plain = [v for k, v in res.items() if f"attn_fwd_kernelILi{hd}ELi{it}EE" in k]
        biased = [v for k, v in res.items() if f"attn_fwd_kbias_kernelILi{hd}ELi{it}EE" in k]
        assert len(plain) == 1 and len(biased) == 1, (hd, it, sorted(res))
        p, b = plain[0], biased[0]
        print(hd, it, "plain", p, "kbias", b)
        lds = 2 * 32 * (hd + 8) * 2                                            # the K and V staging tiles
        assert p["vgprs"] == vgprs and p["lds"] == lds and p["spill"] == 0 and p["scratch"] == 0, (hd, it, p)
        assert b["spill"] == 0 and b["scratch"] == 0, (hd, it, b)
        assert b["lds"] == lds + 256 * 4, (hd, it, b)                          # plus the sample's 256 biases
        assert b["occ"] >= 2, (hd, it, b)
    assert len([k for k in res if "attn_fwd_kbias_kernel" in k]) == 6


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_probe_kernel_resources(tmp_path):
    """The bias form of the probe is the same two kernels (a wave-uniform branch on the bias pointer) and keeps the biases in the
    padding of the K rows already in LDS: no new instantiation, no more LDS, three workgroups per CU as before."""
    res = native.resource_usage("attn_probe.hip", hip.HIPCC_FLAGS, tmp_path / "probe.o")
    assert len(res) == 2, sorted(res)
    for hd in (32, 64):
        (v,) = [v for k, v in res.items() if f"attn_probs_kernelILi{hd}E" in k]
        print(hd, v)
        assert v["spill"] == 0 and v["scratch"] == 0 and v["lds"] == 2 * 128 * (hd + 8) * 2 and v["occ"] >= 3, (hd, v)
