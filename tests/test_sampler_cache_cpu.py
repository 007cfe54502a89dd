"""The cached sampling path, host side (no GPU): the two token-space entry points are declared and bound with matching argument
counts, the ABI version stays, and the `cond_cache` switch of the sampler defaults to off and refuses what the fused loop refuses."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("md_edm_sampler_patchify", "md_edm_heun_update_tok")


def _header():
    return open(os.path.join(ROOT, "include", "microdit_hip.h")).read()


def test_token_space_entry_points_are_declared_and_bound():
    from micro_diffusion_amd import hip
    header = _header()
    for name in NEW:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/microdit_hip.h"
        assert name in hip.exported_symbols(), f"{name} is not bound in hip._SIGS"
        declared = [a for a in m.group(1).split(",") if a.strip()]
        restype, argtypes = hip._SIGS[name]
        assert len(declared) == len(argtypes), (name, len(declared), len(argtypes))
        assert declared[-1].split()[0] == "hipStream_t"
    assert len(hip._SIGS["md_edm_sampler_patchify"][1]) == 11 and len(hip._SIGS["md_edm_heun_update_tok"][1]) == 18
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6, "two symbols added, none changed: the ABI version stays"


def test_entry_points_are_in_the_integration_notes():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in text


def _cpu_model():
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(input_size=8, dim=64, depth=2, head_dim=32, caption_channels=32, multiple_of=32, patch_mixer_depth=1, patch_mixer_dim=64,
                 num_experts=2)
    return LatentDiffusion(d, _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=8)


def test_cond_cache_defaults_to_off(monkeypatch):
    from micro_diffusion_amd import model
    monkeypatch.delenv("MD_SAMPLER_CACHE", raising=False)
    assert model.sampler_cache_enabled(None) is False
    assert model.sampler_cache_enabled(True) is True and model.sampler_cache_enabled(False) is False
    monkeypatch.setenv("MD_SAMPLER_CACHE", "1")
    assert model.sampler_cache_enabled(None) is True and model.sampler_cache_enabled(False) is False
    monkeypatch.setenv("MD_SAMPLER_CACHE", "0")
    assert model.sampler_cache_enabled(None) is False


def test_cond_cache_needs_the_fused_loop(monkeypatch):
    monkeypatch.delenv("MD_SAMPLER_CACHE", raising=False)
    m = _cpu_model()
    x, y = torch.randn(1, 4, 8, 8), torch.randn(1, 1, 5, 32)
    m.edm_config.S_churn = 10
    with pytest.raises(RuntimeError, match="cond_cache needs the fused sampler"):
        m.edm_sampler_loop(x, y, steps=3, cond_cache=True)
    m.edm_config.S_churn = 0
    with pytest.raises(RuntimeError, match="cond_cache needs the fused sampler"):     # CPU tensors
        m.edm_sampler_loop(x, y, steps=3, cond_cache=True)
    with pytest.raises(RuntimeError, match="cond_cache needs the fused sampler"):     # an extra forward argument
        m.edm_sampler_loop(x, y, steps=3, cond_cache=True, foo=1)
    monkeypatch.setenv("MD_SAMPLER_CACHE", "1")                                       # the environment switch goes the same way
    with pytest.raises(RuntimeError, match="cond_cache needs the fused sampler"):
        m.edm_sampler_loop(x, y, steps=3)
