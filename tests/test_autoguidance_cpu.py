"""Autoguidance, host side (no GPU): the four two-pointer update entry points are declared in the header, exported by
the built library and bound with matching argument counts, the ABI version stays, the public arguments default to no guide, and every
request the sampler cannot run is refused with a ValueError before anything touches a device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from micro_diffusion_amd import samplers, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of arguments: the existing counterpart's, has_uncond replaced by the second pointer
NEW = {"md_edm_heun_update_guide": 14, "md_edm_solver_update_guide": 14, "md_edm_heun_update_guide_tok": 18,
       "md_edm_solver_update_guide_tok": 18}


def _header():
    return open(os.path.join(ROOT, "include", "microdit_hip.h")).read()


def test_guide_entry_points_are_declared_and_bound():
    from micro_diffusion_amd import hip
    header = _header()
    for name, nargs in NEW.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/microdit_hip.h"
        assert name in hip.exported_symbols(), f"{name} is not bound in hip._SIGS"
        declared = [a for a in m.group(1).split(",") if a.strip()]
        restype, argtypes = hip._SIGS[name]
        assert len(declared) == len(argtypes) == nargs, (name, len(declared), len(argtypes))
        assert declared[-1].split()[0] == "hipStream_t"
        assert "has_uncond" not in m.group(1) and "guide" in m.group(1)
        # the counterpart has the same number of arguments: one int flag became one pointer
        assert len(hip._SIGS[name.replace("_guide", "")][1]) == nargs
    declared = set(re.findall(r"^int\s+(md_\w+)\s*\(", header, flags=re.M))
    assert set(hip.exported_symbols()) == declared
    assert "BOTH token pointers are 16-byte aligned" in header and "has_uncond = 1 on the concatenation" in header


def test_abi_version_stays():
    from micro_diffusion_amd import hip
    assert re.search(r"#define MD_ABI_VERSION 6\b", _header()) and hip.ABI_VERSION == 6, "four symbols added, none changed"


def test_guide_entry_points_are_exported_by_the_built_library():
    from micro_diffusion_amd import hip
    lib = ctypes.CDLL(hip.build())
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert lib.md_abi_version() == 6


def test_guide_entry_points_are_in_the_documents():
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in NEW:
            assert name in text, (doc, name)
    assert "4.11" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_defaults_are_no_guide():
    from micro_diffusion_amd.model import LatentDiffusion
    for fn in (LatentDiffusion.edm_sampler_loop, LatentDiffusion.generate):
        p = inspect.signature(fn).parameters
        assert p["guide"].default is None and p["guide_captions"].default == "same"
    assert samplers.GUIDE_CAPTIONS == ("same", "null")


# ------------------------------------------------------------------------------------------------ refusals
KW = dict(input_size=8, dim=64, depth=2, head_dim=32, caption_channels=32, multiple_of=32, patch_mixer_depth=1, patch_mixer_dim=64,
          num_experts=2)


def _dit(**over):
    from micro_diffusion_amd import dit as mdit
    return mdit.DiT(**{**KW, **over})


@pytest.fixture(scope="module")
def cpu_model():
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    return LatentDiffusion(_dit(), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=8)


class _Elsewhere(torch.nn.Module):
    """A stand-in guide with main's geometry whose parameters live on another device (the meta device: no storage anywhere)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.w = torch.nn.Parameter(torch.empty(1, device="meta"))

    def forward_without_cfg(self, *a, **k):
        raise AssertionError("a refused guide must never be evaluated")

    encode_condition = forward_without_cfg


def _never(*a, **k):
    raise AssertionError("the request must be refused before any network evaluation")


def _bad_requests(model):
    yield "in_channels", dict(guide=_dit(in_channels=8))
    yield "patch_size", dict(guide=_dit(patch_size=4))
    yield "caption_channels", dict(guide=_dit(caption_channels=64))
    yield "same device", dict(guide=_Elsewhere(model.dit.config))
    yield "unknown guide_captions", dict(guide=_dit(), guide_captions="zero")
    yield "unknown guide_captions", dict(guide_captions="uncond")
    yield "needs a guide", dict(guide_captions="null")


def test_refusals_raise_before_anything_runs(cpu_model, monkeypatch):
    m = cpu_model
    x, y = torch.randn(1, 4, 8, 8), torch.randn(1, 1, 5, 32)
    monkeypatch.setattr(m.dit, "forward_without_cfg", _never)
    monkeypatch.setattr(m.dit, "encode_condition", _never)
    monkeypatch.setattr(sampling, "FusedRun", _never)                  # the fused loop's entry point: its constructor
    n = 0
    for match, kw in _bad_requests(m):
        for fused in (None, False, True):
            for cfg in (1.0, 3.0):                      # refused whether or not the guide would ever be evaluated
                with pytest.raises(ValueError, match=match):
                    m.edm_sampler_loop(x, y, steps=3, cfg=cfg, fused=fused, **kw)
        with pytest.raises(ValueError, match=match):     # generate: before the tokenizer / text encoder stubs (which raise RuntimeError)
            m.generate(prompt=["a"], **kw)
        n += 1
    assert n == 7


def test_check_guide_accepts_what_is_legal(cpu_model):
    d = cpu_model.dit
    samplers.check_guide(d, None, "same")
    samplers.check_guide(d, d, "same")                  # main as its own guide: legal (the result does not depend on w)
    samplers.check_guide(d, d, "null")                  # classifier-free guidance as two batch-B launches
    samplers.check_guide(d, _dit(dim=32, depth=1), "same")      # narrower and shallower: what a guide is
    samplers.check_guide(d, _dit(dim=32, depth=1), "null")


def test_autoguided_forward_combines_in_fp32(cpu_model):
    """The tensor-op loop's forward function: fg + w * (fm - fg) in fp32, the guide with its own captions."""
    class Net:
        def __init__(self, k):
            self.k, self.seen = k, []

        def forward_without_cfg(self, x, t, y, **kw):
            self.seen.append(y)
            return {"sample": (self.k * x).to(torch.float64), "mask": None}
    main, guide = Net(2.0), Net(0.5)
    holder = type("H", (), {"dit": main})()
    y, yg = torch.ones(2, 1, 3, 4), torch.zeros(2, 1, 3, 4)
    fwd = sampling.autoguided_forward(holder, guide, yg, 2.5)
    x = torch.randn(2, 4, 8, 8)
    out = fwd(x, torch.zeros(1), y, mask_ratio=0)["sample"]
    assert out.dtype == torch.float32
    assert torch.equal(out, 0.5 * x + 2.5 * (2.0 * x - 0.5 * x))
    assert main.seen[0] is y and guide.seen[0] is yg
