"""Dispersive loss, the kernels alone: md_disperse_pairs on a Gram computed in fp64 on the host and rounded to fp32, the
Gram product on both of its paths (the GEMM family's split-K for B % 8 == 0, md_disperse_gram_small otherwise) and the injection
dx += W' Z through the family's residual epilogue, each against disperse.reference / fp64.

Bounds.  L and the mean distance: fp32 evaluation of exp / log on arguments of the size used -> relative 1e-5, absolute floor 1e-6.
W': one bf16 rounding, relative 2^-8 per entry with an absolute floor of 2^-8 times the largest |W'| of the row.  Injection: the family's
residual epilogue rounds the product to bf16 and then the sum to bf16 (as every data gradient of the engine that adds into dx does), so
|out - ref| <= 2^-8 |W'Z| + 2^-8 |ref| + B 2^-24 sum_j |W'_aj Z_jc| (fp32 accumulation of B terms)."""
import json

import pytest
import torch

from micro_diffusion_amd import disperse as dsp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 2, 3, 8, 9, 64, 65, 257]
K = 256
REPORT = {}


def _pad8(n):
    return (n + 7) // 8 * 8


def _close(got, want, what):
    assert abs(got - want) <= 1e-5 * abs(want) + 1e-6, f"{what}: {got} vs {want}"


def _pairs(hip, G64, B, Kdim, tau, coef, accum=None, weight=0.0):
    """Launch md_disperse_pairs on the fp32 rounding of G64; pad columns of G are NaN (they must not be read).  -> (result[4], W[B, ldw])"""
    ld = _pad8(B)
    G = torch.full((B, ld), float("nan"), device=DEV, dtype=torch.float32)
    G[:, :B] = G64.to(DEV).float()
    W = torch.full((B, ld), float("nan"), device=DEV, dtype=torch.bfloat16)
    res = torch.full((4,), float("nan"), device=DEV, dtype=torch.float64)
    ws = torch.full((2 * B,), float("nan"), device=DEV, dtype=torch.float64)
    la = None if accum is None else accum[0:1].data_ptr()
    da = None if accum is None else accum[1:2].data_ptr()
    hip.check(hip.lib().md_disperse_pairs(G.data_ptr(), ld, B, Kdim, tau, coef, W.data_ptr(), ld, res.data_ptr(), ws.data_ptr(), 2 * B,
                                          la, da, weight, hip.stream_ptr()), "md_disperse_pairs")
    torch.cuda.synchronize()
    return res.cpu(), W.cpu()


def _check_weights(W, Wref, coef, B, what):
    want = coef * Wref
    got = W[:, :B].double()
    floor = 2.0 ** -8 * want.abs().amax(dim=1, keepdim=True)
    err = (got - want).abs()
    # relative 2^-8 per entry, absolute floor 2^-8 x the row's largest |W'| -- an entry passes when it meets either
    ok = (err <= 2.0 ** -8 * want.abs()) | (err <= floor)
    assert bool(ok.all()), f"{what}: W' off by {float(err.max())} (largest |W'| {float(want.abs().max())})"
    assert not W[:, B:].any() and bool(torch.isfinite(W.float()).all()), f"{what}: the pad columns are exactly zero"


@pytest.mark.parametrize("B", SIZES)
def test_pairs_against_reference(hip, B):
    torch.manual_seed(B)
    z = torch.randn(B, K, dtype=torch.float64)
    tau, lam, gs = 0.5, 0.5, 0.25
    coef = 4.0 * lam * gs / (tau * K)
    G64 = z @ z.t()
    res, W = _pairs(hip, G64, B, K, tau, coef)
    L, _, md = dsp.reference(z, tau)
    Wref, _, _ = dsp.reference_weights(G64, K, tau)
    print(json.dumps({"B": B, "L": float(res[0]), "L_ref": float(L), "mean_D": float(res[1]), "mean_D_ref": float(md),
                      "mean_offdiag_p_B2": float(res[2]), "S": float(res[3])}))
    _close(float(res[0]), float(L), f"L at B = {B}")
    _close(float(res[1]), float(md), f"mean distance at B = {B}")
    if B == 1:
        assert float(res[0]) == 0.0 and float(res[1]) == 0.0 and float(res[2]) == 0.0 and not W.any()
        return
    off = ~torch.eye(B, dtype=torch.bool)
    _close(float(res[2]), float(Wref[off].mean() * B * B), f"mean off-diagonal p B^2 at B = {B}")
    _check_weights(W, Wref, coef, B, f"B = {B}")
    # the rows of W' sum to zero up to its bf16 roundings: the diagonal is the negative off-diagonal row sum
    assert float(W[:, :B].double().sum(dim=1).abs().max()) <= B * 2.0 ** -8 * float(W.double().abs().max())
    res2, W2 = _pairs(hip, G64, B, K, tau, coef)
    assert torch.equal(res.view(torch.int64), res2.view(torch.int64)) and torch.equal(W.view(torch.int16), W2.view(torch.int16)), \
        "two launches on the same Gram give identical bits"


@pytest.mark.parametrize("B", [2, 9, 65])
def test_saturated_and_identical_rows(hip, B):
    import math
    torch.manual_seed(B)
    z = torch.randn(B, K, dtype=torch.float64)
    coef = 4.0 * 0.5 / (0.5 * K)
    res, W = _pairs(hip, (30.0 * z) @ (30.0 * z).t(), B, K, 0.5, coef)
    _close(float(res[0]), math.log(1.0 / B), "saturated L")
    assert not W.any() and bool(torch.isfinite(res).all()), "saturated: the weights are exactly 0, nothing is NaN"
    assert float(res[3]) == float(B) and float(res[2]) == 0.0
    same = z[:1].expand(B, K)
    G64 = torch.full((B, B), float((same[0] ** 2).sum()), dtype=torch.float64)        # the Gram of B identical rows
    res, W = _pairs(hip, G64, B, K, 0.5, coef)
    assert float(res[0]) == 0.0 and float(res[1]) == 0.0 and abs(float(res[2]) - 1.0) <= 1e-12
    Wref, _, _ = dsp.reference_weights(G64, K, 0.5)
    _check_weights(W, Wref, coef, B, "identical rows")
    # the gradient W' Z = (row sum of W') z: zero up to the bf16 rounding of the diagonal entry
    # (one rounding of the diagonal, one of the B - 1 equal off-diagonal entries: each at most 2^-8 |W'_aa|)
    assert float(W[:, :B].double().sum(dim=1).abs().max()) <= 2 * 2.0 ** -8 * float(W.double().abs().max())


def test_pairs_accumulates_on_the_device(hip):
    torch.manual_seed(5)
    z = torch.randn(5, K, dtype=torch.float64)
    acc = torch.tensor([1.5, -2.0], device=DEV)
    res, _ = _pairs(hip, z @ z.t(), 5, K, 0.5, 1.0, accum=acc, weight=0.25)
    want = torch.tensor([1.5 + 0.25 * float(res[0]), -2.0 + 0.25 * float(res[1])])
    assert float((acc.cpu() - want).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ the two products
@pytest.fixture(scope="module")
def engine(hip):
    from oracle import microdit_ref as orc
    from micro_diffusion_amd import dit as mdit
    cfg = orc.tiny_config()
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(orc.synth_state_dict(cfg, 3))
    return d.to(DEV).engine


@pytest.mark.parametrize("B,Kdim,path", [(2, 256, "small"), (8, 1024, "gemm"), (9, 1024, "small"), (64, 4096, "gemm"), (65, 512, "small")])
def test_gram_on_both_paths(hip, engine, B, Kdim, path):
    torch.manual_seed(B + Kdim)
    z = torch.randn(B, Kdim, device=DEV).to(torch.bfloat16)
    ld = _pad8(B)
    G = torch.full((B, ld), float("nan"), device=DEV, dtype=torch.float32)
    engine.disperse_log, engine.gemm_log = [], []
    engine.disperse_gram(z, B, Kdim, G, ld)
    torch.cuda.synchronize()
    log, glog, engine.disperse_log, engine.gemm_log = engine.disperse_log, engine.gemm_log, None, None
    assert log == [("gram", path, B, Kdim)], log
    assert (len(glog) == 1) == (path == "gemm"), glog
    REPORT[f"gram B={B} K={Kdim}"] = {"path": path, "gemm_variant": [g[0] for g in glog]}
    print(json.dumps(REPORT[f"gram B={B} K={Kdim}"]))
    ref = z.double() @ z.double().t()
    # fp32 accumulation of K products of bf16 values (exact in fp32): |err| <= K 2^-24 sum_k |z_ik z_jk|
    bound = Kdim * 2.0 ** -24 * (z.double().abs() @ z.double().abs().t())
    assert bool(((G[:, :B].double() - ref).abs() <= bound).all())
    if path == "small":
        assert bool(torch.isnan(G[:, B:]).all()), "columns >= B are not written"
    G2 = torch.empty_like(G)
    engine.disperse_gram(z, B, Kdim, G2, ld)
    torch.cuda.synchronize()
    assert torch.equal(G[:, :B], G2[:, :B]), "two launches give identical bits"


@pytest.mark.parametrize("B,Kdim", [(2, 256), (5, 384), (9, 1024), (65, 512), (256, 49152)])
def test_injection_against_fp64(hip, engine, B, Kdim):
    """dx_out = dx + W' Z.  (256, 49152) is the smallest shape the AUTO rule hands to the 4-wave 256 x 256 kernel (192 tiles, whole
    interior tiles, contraction a multiple of 128): the kernel the XL/2 microbatch runs on."""
    torch.manual_seed(B * 7 + Kdim)
    ld = _pad8(B)
    z = torch.randn(B, Kdim, device=DEV).to(torch.bfloat16)
    dx = torch.randn(B, Kdim, device=DEV).to(torch.bfloat16)
    W = torch.zeros(B, ld, device=DEV, dtype=torch.bfloat16)
    W[:, :B] = (torch.randn(B, B, device=DEV) / B ** 0.5).to(torch.bfloat16)
    acc = W[:, :B].double() @ z.double()
    ref = dx.double() + acc
    out = dx.clone()
    engine.disperse_log, engine.gemm_log = [], []
    engine.disperse_apply(W, ld, z, out, B, Kdim)
    torch.cuda.synchronize()
    log, glog, engine.disperse_log, engine.gemm_log = engine.disperse_log, engine.gemm_log, None, None
    assert log == [("apply", "gemm", B, Kdim)] and len(glog) == 1 and glog[0][1:] == (B, Kdim, B, 1), (log, glog)
    names = {v: k for k, v in hip.GEMM_VARIANT_NAMES.items()}
    REPORT[f"apply B={B} K={Kdim}"] = {"path": "gemm", "gemm_variant": names[glog[0][0]]}
    print(json.dumps(REPORT[f"apply B={B} K={Kdim}"]))
    if (B, Kdim) == (256, 49152):
        assert names[glog[0][0]] == "w4", "the large case is there for the 4-wave kernel"
    bound = 2.0 ** -8 * acc.abs() + 2.0 ** -8 * ref.abs() + B * 2.0 ** -24 * (W[:, :B].double().abs() @ z.double().abs())
    err = (out.double() - ref).abs()
    assert bool((err <= bound).all()), f"max err {float(err.max())}, worst excess {float((err - bound).max())}"
    assert float((out.double() - dx.double()).abs().max()) > 0, "the launch wrote dx"
