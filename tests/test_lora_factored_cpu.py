"""The host side of LoRA's factored backward: the config switch, the constructor argument, the fp64 restatement and
the C ABI's new symbols -- everything that needs no GPU."""
import ctypes
import os
import re

import pytest
import torch

from micro_diffusion_amd import config as mdcfg
from micro_diffusion_amd import hip, lora, native


def _cfg(**misc):
    return {"misc": dict(misc), "algorithms": {}}


def test_lora_backward_option():
    assert mdcfg.lora_backward_option({}) == "projected"
    assert mdcfg.lora_backward_option(_cfg(lora_rank=16)) == "projected"
    assert mdcfg.lora_backward_option(_cfg(lora_rank=16, lora_backward="projected")) == "projected"
    assert mdcfg.lora_backward_option(_cfg(lora_rank=16, lora_backward="factored")) == "factored"
    for bad in ("fused", "", 1, True, ["factored"]):
        with pytest.raises(ValueError, match="lora_backward"):
            mdcfg.lora_backward_option(_cfg(lora_rank=16, lora_backward=bad))
    for rank in ({}, {"lora_rank": 0}):
        with pytest.raises(ValueError, match="lora_backward needs misc.lora_rank"):
            mdcfg.lora_backward_option(_cfg(lora_backward="factored", **rank))


def test_lora_options_world_and_keys(monkeypatch):
    keys = {"enabled", "rank", "alpha", "targets", "weight_decay", "load_path"}
    with pytest.raises(ValueError, match="single-GPU"):
        mdcfg.lora_options(_cfg(lora_rank=16), world=2)
    with pytest.raises(ValueError, match="single-GPU"):
        mdcfg.lora_options(_cfg(lora_rank=16, lora_backward="projected"), world=2)
    got = mdcfg.lora_options(_cfg(lora_rank=16, lora_backward="factored"), world=2)
    assert got["enabled"] and set(got) == keys
    assert set(mdcfg.lora_options(_cfg(lora_rank=16), world=1)) == keys and set(mdcfg.lora_options(_cfg())) == keys
    monkeypatch.setenv("WORLD_SIZE", "4")
    assert mdcfg.lora_options(_cfg(lora_rank=8, lora_backward="factored"))["rank"] == 8
    with pytest.raises(ValueError, match="lora_backward"):
        mdcfg.lora_options(_cfg(lora_rank=8, lora_backward="x"))


def test_constructor_argument():
    from oracle import microdit_ref as orc
    from micro_diffusion_amd import dit as mdit
    d = mdit.DiT(**orc.tiny_config().__dict__)
    assert lora.LoRA(d, rank=4, device="cpu").backward == "projected"
    ad = lora.LoRA(d, rank=4, device="cpu", backward="factored")
    assert ad.backward == "factored" and not ad.factored, "factored counts only while the adapter is attached and active"
    for bad in ("x", None, "Factored"):
        with pytest.raises(ValueError, match="backward"):
            lora.LoRA(d, rank=4, device="cpu", backward=bad)
    sd = ad.state_dict()
    assert "backward" not in sd
    assert lora.LoRA.from_state_dict(d, sd, device="cpu").backward == "projected"
    assert lora.LoRA.from_state_dict(d, sd, device="cpu", backward="factored").backward == "factored"
    assert ad.is_target("blocks.0.attn.qkv.weight") and not ad.is_target("blocks.0.mlp.w1.weight")


@pytest.mark.parametrize("M,N,K,r", [(7, 24, 16, 4), (300, 40, 72, 16)])
def test_ref_wgrad_factored_is_ref_grad_of_the_full_gradient(M, N, K, r):
    g = torch.Generator().manual_seed(M + N)
    dy, x = torch.randn(M, N, generator=g).to(torch.bfloat16), torch.randn(M, K, generator=g).to(torch.bfloat16)
    A, B = torch.randn(r, K, generator=g), torch.randn(N, r, generator=g)
    dA, dB = lora.ref_wgrad_factored(dy, x, A, B, 0.375)
    rA, rB = lora.ref_grad(dy.double().t() @ x.double(), A, B, 0.75, 0.5)
    assert dA.dtype == torch.float64 and tuple(dA.shape) == (r, K) and tuple(dB.shape) == (N, r)
    for name, a, b in (("dA", dA, rA), ("dB", dB, rB)):
        err = float((a - b).abs().max())
        print(f"{name}: max |factored - ref_grad(dy^T x)| = {err:.3g} (bound 1e-12 * max |ref|)")
        assert err <= 1e-12 * float(b.abs().max())


def test_symbols_header_and_host_checks():
    header = open(os.path.join(native.INCLUDE, "microdit_hip.h")).read()
    for name in ("md_lora_wgrad_ws_floats", "md_lora_wgrad_geometry", "md_lora_wgrad"):
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in the header"
        assert name in hip.exported_symbols() and name in hip._SIGS
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6
    assert os.path.join(native.CSRC, "lora_wgrad.hip") in hip._hashed_files()
    # the two host functions run without a GPU
    L = hip.lib()
    need, strip, groups = ctypes.c_int64(-1), ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.md_lora_wgrad_ws_floats(16384, 3072, 1024, 16, ctypes.byref(need)) == 0
    assert L.md_lora_wgrad_geometry(16384, 3072, 1024, 16, ctypes.byref(strip), ctypes.byref(groups)) == 0
    M, N, K, r = 16384, 3072, 1024, 16
    # shares [groups][r][N + K] fp32, the bf16 adapter operands [r][N + K], P^T and Q^T as bf16 [2 r][M]: nothing of N * K elements
    assert need.value == groups.value * r * (N + K) + r * (N + K) // 2 + r * M and need.value < N * K
    assert strip.value > 0 and 1 <= groups.value <= -(-M // strip.value)
    for args in ((M, N, K, 12), (M, N, 60, r), (M, N, 0, r), (0, N, K, r), (M, 0, K, r)):
        assert L.md_lora_wgrad_ws_floats(*args, ctypes.byref(need)) == -1, args
        assert L.md_lora_wgrad_geometry(*args, ctypes.byref(strip), ctypes.byref(groups)) == -1, args
    assert L.md_lora_wgrad_ws_floats(M, N, K, r, None) == -1


def test_kernels_are_spill_free(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    res = native.resource_usage("lora_wgrad.hip", hip.HIPCC_FLAGS, tmp_path / "lora_wgrad.o")
    assert len(res) == 8, sorted(res)              # prep, finish, and {projection, reduction} x {16, 32, 64} padded ranks
    for name, v in res.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (name, v)
        assert v["lds"] <= 64 * 1024, (name, v)
