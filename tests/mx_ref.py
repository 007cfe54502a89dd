"""Reference of the MXFP8 format (OCP MX, e4m3fn elements, one e8m0 scale per 32 consecutive elements along the last dimension), pure
torch on the CPU.  For a block with largest magnitude amax (fp32, from bf16 inputs):

    X = clamp(floor(log2 amax) - 8, -127, 127);  scale byte = X + 127;  amax = 0: scale byte 0 and zero elements
    element = e4m3_rne(clamp(v * 2^-X, -448, 448))        (the scaling is exact: a power of two)

The clamp is part of the rule: a block with amax in (448 * 2^X, 512 * 2^X) would otherwise overflow, and torch's cast then gives NaN.
Inputs are finite.
"""
import torch

BLOCK = 32


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for integer e in [-126, 127], built from the encoding (no transcendental)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def mx_quantize(x_bf16: torch.Tensor):
    """x [..., K] bf16 with K % 32 == 0 -> (fp8 [..., K] float8_e4m3fn, scale bytes uint8 [..., K / 32])."""
    assert x_bf16.dtype == torch.bfloat16 and x_bf16.shape[-1] % BLOCK == 0
    x = x_bf16.detach().cpu().to(torch.float32)
    blocks = x.reshape(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    amax = blocks.abs().amax(-1)
    _, e = torch.frexp(amax)                              # amax = m * 2^e, m in [0.5, 1): floor(log2 amax) = e - 1 (subnormals too)
    X = (e.to(torch.int32) - 1 - 8).clamp(-127, 127)
    X = torch.where(amax == 0, torch.full_like(X, -127), X)
    # floor(log2 amax) <= 127 gives X in [-127, 119]: the factor 2^-X lies in [2^-119, 2^127], a normal fp32 number
    scaled = blocks * _pow2(-X).unsqueeze(-1)
    q = scaled.clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.reshape(x.shape), (X + 127).to(torch.uint8)


def mx_dequantize(q: torch.Tensor, scale_bytes: torch.Tensor) -> torch.Tensor:
    """fp64 [..., K] of elements [..., K] (float8_e4m3fn, or their uint8 encodings) and scale bytes [..., K / 32]."""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    v = q.detach().cpu().to(torch.float32).to(torch.float64)
    s = torch.ldexp(torch.ones((), dtype=torch.float64), scale_bytes.detach().cpu().to(torch.int32) - 127)
    return (v.reshape(*v.shape[:-1], v.shape[-1] // BLOCK, BLOCK) * s.unsqueeze(-1)).reshape(v.shape)
