"""Input gradients, host side: the ABI additions, the argument checks of md_patch_embed_dgrad (they run on the host in
front of the launch) and LearnedCaption on CPU tensors.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"md_patch_embed_dgrad": 13, "md_timestep_embed_bwd": 6, "md_cast_rows_from_bf16": 8}


def test_library_exports_the_entry_points():
    from micro_diffusion_amd import hip
    with open(os.path.join(ROOT, "include", "microdit_hip.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(hip.build())
    for name, nargs in NEW.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/microdit_hip.h"
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
        assert name in hip.exported_symbols(), f"{name} is not bound in hip._SIGS"
        declared = [a for a in m.group(1).split(",") if a.strip()]
        assert len(declared) == len(hip._SIGS[name][1]) == nargs, (name, len(declared))
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6 == lib.md_abi_version(), "symbols added, none changed"
    assert re.search(r"#define MD_PATCH_EMBED_DGRAD_MAX_PV 64\b", header) and hip.PATCH_EMBED_DGRAD_MAX_PV == 64


def test_bad_arguments_are_refused_before_any_launch():
    """Fake addresses: a call that got past the checks would fault, so every one of these must return MD_BAD_ARG from the host."""
    from micro_diffusion_amd import hip
    L = hip.lib()
    a, w, o = 1 << 20, 2 << 20, 3 << 20
    good = dict(dtok=a, ld=128, w=w, scale=None, dx=o, B=2, C=4, H=8, W=8, p=2, D=128)

    def call(**kw):
        g = dict(good, **kw)
        return L.md_patch_embed_dgrad(g["dtok"], g["ld"], g["w"], g["scale"], g["dx"], g["B"], g["C"], g["H"], g["W"], g["p"], g["D"], None, None)
    for kw in (dict(dtok=None), dict(w=None), dict(dx=None), dict(B=0), dict(C=0), dict(H=0), dict(W=-2), dict(p=0), dict(D=0), dict(H=7),
               dict(W=9), dict(D=124, ld=124), dict(ld=120), dict(C=17), dict(C=4, p=8, H=8, W=8)):
        assert call(**kw) == -1, kw
    assert L.md_timestep_embed_bwd(None, a, o, 2, 512, None) == -1 and L.md_timestep_embed_bwd(a, a, o, 0, 512, None) == -1
    assert L.md_timestep_embed_bwd(a, a, o, 2, 511, None) == -1 and L.md_timestep_embed_bwd(a, a, None, 2, 512, None) == -1
    assert L.md_cast_rows_from_bf16(None, o, 1, 4, 8, None, 2, None) == -1 and L.md_cast_rows_from_bf16(a, o, 2, 4, 8, None, 2, None) == -1
    assert L.md_cast_rows_from_bf16(a, o, 1, 0, 8, None, 2, None) == -1 and L.md_cast_rows_from_bf16(a, o, 1, 4, 8, a, 0, None) == -1


def test_engine_backward_signature():
    """The Trainer's call -- backward(tape, dtok, on_segment) -- is still valid and means what it meant: no input gradient, all
    parameter gradients."""
    import inspect
    from micro_diffusion_amd.engine import DiTEngine, InputGrads
    sig = inspect.signature(DiTEngine.backward)
    assert list(sig.parameters)[:4] == ["self", "tp", "dtok", "on_segment"]
    assert sig.parameters["input_grads"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["input_grads"].default == ()
    assert sig.parameters["param_grads"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["param_grads"].default is True
    assert DiTEngine._param_grads is True
    g = InputGrads()
    assert g.dx is None and g.dt is None and g.dy is None


@pytest.mark.parametrize("shape", [(3, 7, 16), (2, 1, 7, 16)])
def test_learned_caption_replaces_rows_and_gets_their_gradient(shape):
    from micro_diffusion_amd.prompt_tuning import LearnedCaption
    torch.manual_seed(5)
    y = torch.randn(*shape)
    init = torch.randn(2, 16)
    lc = LearnedCaption(2, 16, init=init)
    assert [n for n, _ in lc.named_parameters()] == ["tokens"] and lc.tokens.dtype == torch.float32 and torch.equal(lc.tokens.detach(), init)
    pos = torch.tensor([5, 1])
    y0 = y.clone()
    y.requires_grad_(True)
    out = lc(y, pos)
    assert out.shape == y.shape and out.dtype == y.dtype and torch.equal(y.detach(), y0), "the input must not be modified"
    exp = y0.clone()
    exp[..., 5, :] = init[0]
    exp[..., 1, :] = init[1]
    assert torch.equal(out.detach(), exp)
    cot = torch.randn(*shape)
    (out * cot).sum().backward()
    lead = tuple(range(len(shape) - 2))
    g = torch.stack([cot[..., 5, :].sum(dim=lead), cot[..., 1, :].sum(dim=lead)])
    assert torch.allclose(lc.tokens.grad, g, rtol=1e-6, atol=1e-6), "each token gets its row's gradient summed over the batch"
    gy = cot.clone()
    gy[..., 5, :] = 0
    gy[..., 1, :] = 0
    assert torch.equal(y.grad, gy), "replaced rows of y get no gradient, the others the cotangent"


def test_learned_caption_half_input_and_validation():
    from micro_diffusion_amd.prompt_tuning import LearnedCaption
    lc = LearnedCaption(1, 8)
    assert float(lc.tokens.detach().abs().max()) == 0.0
    y = torch.ones(2, 1, 4, 8, dtype=torch.float16)
    out = lc(y, [2])
    assert out.dtype == torch.float16 and float(out[:, :, 2].abs().max()) == 0.0 and float(out[:, :, 3].min()) == 1.0
    out.float().sum().backward()
    assert lc.tokens.grad.shape == (1, 8) and lc.tokens.grad.dtype == torch.float32
    for bad in ([4], [-1], [0, 1]):
        with pytest.raises(ValueError):
            lc(y, bad)
    with pytest.raises(ValueError):
        LearnedCaption(2, 8)(y, [1, 1])
    with pytest.raises(ValueError):
        lc(torch.ones(2, 4, 9), [0])
    with pytest.raises(ValueError):
        LearnedCaption(2, 8, init=torch.zeros(3, 8))
