"""ctypes binding of libmicrodit_hip.so (the C ABI declared in include/microdit_hip.h).

This is the only place Python touches the HIP kernels.  There is deliberately NO fallback: if the shared
library is missing or a launch fails, a RuntimeError is raised (the product path never routes through the
CPU oracle or through PyTorch ops).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_float, c_int, c_int32, c_int64, c_void_p, POINTER, Structure, byref

from . import native

_CSRC = native.CSRC
_HEADER = os.path.join(native.INCLUDE, "microdit_hip.h")
LIB_PATH = os.path.join(os.path.dirname(_CSRC), "libmicrodit_hip.so")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
               "-Wno-unused-result", "-Wno-inline-asm"]   # (inline-asm: gemm_w4's literal v[128:255] clobbers are "reserved" by design)

# enums (mirror include/microdit_hip.h)
ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU = 0, 1, 2, 3
EPI_STORE_BF16, EPI_RESIDUAL, EPI_STORE_F32, EPI_ACCUM_F32, EPI_ATOMIC_F32, EPI_DACT, EPI_SWIGLU_BWD = 0, 1, 2, 3, 4, 5, 6
DET_GATE_BWD, DET_LN_BWD, DET_COLSUM = 0, 1, 2      # md_det_kind
GEMM_AUTO, GEMM_REG128, GEMM_DMA128, GEMM_PACED256, GEMM_PP256, GEMM_W4 = 0, 1, 2, 3, 4, 5
GEMM_VARIANT_NAMES = {"auto": 0, "reg128": 1, "dma128": 2, "paced256": 3, "pp256": 4, "w4": 5}
# md_attn_args.bwd_split: backward kernel selector (0 = the library's rule; the others force a kernel: tests, A/B runs)
ATTN_BWD_AUTO, ATTN_BWD_FUSED_1PHASE, ATTN_BWD_FUSED_2PHASE, ATTN_BWD_FUSED_2PHASE_SPLIT, ATTN_BWD_STREAM_PAIR = 0, 2, 3, 4, 5   # (1: removed)


def _hashed_files():
    """What the build reads: every file directly under csrc/ (headers and generated includes too), and the public header."""
    return [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if os.path.isfile(os.path.join(_CSRC, f))] + [_HEADER]


def _gemm_source_hash() -> str:
    """Hash of what determines the GEMM kernels alone (gemm*.hip, their headers and generated includes, md_common.h, the public header,
    the compiler flags): the key of profiles/*_gemm_traffic.json, so that an edit of attention.hip does not void a GEMM measurement."""
    files = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC))
             if f.endswith((".hip", ".h", ".inc")) and (f.startswith("gemm") or f == "md_common.h")]
    return native.source_hash(files + [_HEADER], HIPCC_FLAGS)


def _source_hash() -> str:
    return native.source_hash(_hashed_files(), HIPCC_FLAGS)


def build(force: bool = False, verbose: bool = True) -> str:
    """Compile every .hip under csrc/ for gfx950 in parallel into csrc/build/<name>.o (scripts/build_*_variant.sh link against
    those objects) and link libmicrodit_hip.so in-tree (idempotent)."""
    def make(tmp):
        hipcc = native.hipcc()
        objdir = os.path.join(_CSRC, "build")
        os.makedirs(objdir, exist_ok=True)
        srcs = sorted(f for f in os.listdir(_CSRC) if f.endswith(".hip"))
        objs = [os.path.join(objdir, f[:-4] + ".o") for f in srcs]
        native.run(*([hipcc, *HIPCC_FLAGS, "-I", native.INCLUDE, "-c", os.path.join(_CSRC, f), "-o", o] for f, o in zip(srcs, objs)),
                   verbose=verbose)
        native.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", tmp])
    return native.build(LIB_PATH, _source_hash(), make, force)


class GemmProblem(Structure):
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("lda", c_int64), ("ldb", c_int64), ("M", c_int64), ("N", c_int64), ("c_off", c_int64)]


GEMM_MAX_PROBLEMS = 8
NUM_CU = 256            # MI355X; md_gemm_args.cu_limit is counted against it


class GemmArgs(Structure):
    _fields_ = [
        ("A", c_void_p), ("B", c_void_p), ("C", c_void_p), ("C2", c_void_p), ("bias", c_void_p),
        ("res", c_void_p), ("gate", c_void_p), ("aux", c_void_p),
        ("M", c_int64), ("N", c_int64), ("K", c_int64),
        ("lda", c_int64), ("ldb", c_int64), ("ldc", c_int64), ("ldc2", c_int64), ("ldr", c_int64),
        ("ldg", c_int64), ("ldaux", c_int64),
        ("sA", c_int64), ("sB", c_int64), ("sC", c_int64), ("sC2", c_int64), ("sBias", c_int64),
        ("sAux", c_int64), ("sSplit", c_int64),
        ("rows_per_sample", c_int64),
        ("batch", c_int32), ("ksplit", c_int32), ("a_kcontig", c_int32), ("b_kcontig", c_int32),
        ("mode", c_int32), ("act", c_int32), ("alpha", c_float), ("variant", c_int32), ("raster_group_n", c_int32),
        ("timeline", c_void_p), ("chosen_variant", c_void_p), ("A_list", c_void_p), ("B_list", c_void_p), ("list_segments", c_int32),
        ("problems", c_void_p), ("n_problems", c_int32), ("cu_limit", c_int32),
        ("tail_ws", c_void_p), ("tail_ws_bytes", c_int64), ("tail_mode", c_int32), ("tail_used", c_void_p),
        ("dact_cached", c_int32),
    ]


_lib = None
ABI_VERSION = 6        # MD_ABI_VERSION of include/microdit_hip.h this binding was written against


def lib() -> ctypes.CDLL:
    """Load (once) the in-tree shared library; raise loudly when it is absent."""
    global _lib
    if _lib is None:
        path = os.environ.get("MICRODIT_LIB")       # experiments only: load an explicitly named build
        if not path:
            stale = not native.up_to_date(LIB_PATH, _source_hash())
            if stale and (os.path.exists("/opt/rocm/bin/hipcc") or os.environ.get("HIPCC")):
                build()                      # sources changed since the last build: never run a stale library
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} is missing: the MicroDiT HIP extension has not been built. "
                    "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                    "There is no CPU / PyTorch fallback for the training path.")
            path = LIB_PATH
        _lib = native.load(path, _SIGS, "md_abi_version", ABI_VERSION)
    return _lib


NOT_ELIGIBLE = -2      # MD_NOT_ELIGIBLE: the forced kernel variant does not cover the problem (nothing was launched)


def check(code: int, what: str) -> None:
    if code != 0:
        why = {-1: "bad argument", NOT_ELIGIBLE: "forced kernel variant not eligible for this problem"}.get(code, "hipError_t")
        raise RuntimeError(f"{what} failed with code {code} ({why})")


# name -> (restype, argtypes); every launch function returns int and takes the stream last.
_SIGS = {"md_abi_version": (c_int, [])}


def _sig(name, *argtypes):
    _SIGS[name] = (c_int, list(argtypes))


P, I64, I32, F32 = c_void_p, c_int64, c_int32, c_float

class LnArgs(Structure):
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("shift", c_void_p), ("scale", c_void_p), ("pos", c_void_p),
                ("out", c_void_p), ("mean", c_void_p), ("rstd", c_void_p),
                ("rows", c_int64), ("C", c_int64), ("ldx", c_int64), ("ldo", c_int64), ("ldmod", c_int64),
                ("rows_per_sample", c_int64), ("pos_rows", c_int64), ("eps", c_float), ("act", c_int32)]


class LnBwdArgs(Structure):
    _fields_ = [("dz", c_void_p), ("dx", c_void_p), ("dscale", c_void_p), ("dshift", c_void_p), ("dw", c_void_p),
                ("lddz", c_int64), ("lddx", c_int64), ("ldg", c_int64), ("rows_per_block", c_int64),
                ("accumulate", c_int32), ("dscale_is_output", c_int32)]


class AttnArgs(Structure):
    _fields_ = [("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("o", c_void_p), ("lse", c_void_p),
                ("d_o", c_void_p), ("dq", c_void_p), ("dk", c_void_p), ("dv", c_void_p), ("delta", c_void_p),
                ("B", c_int64), ("H", c_int64), ("Sq", c_int64), ("Skv", c_int64),
                ("ldq", c_int64), ("ldk", c_int64), ("ldv", c_int64), ("ldo", c_int64),
                ("sq", c_int64), ("sk", c_int64), ("sv", c_int64), ("so", c_int64),
                ("lddq", c_int64), ("lddk", c_int64), ("lddv", c_int64), ("lddo", c_int64),
                ("sdq", c_int64), ("sdk", c_int64), ("sdv", c_int64), ("sdo", c_int64),
                ("scale", c_float), ("hd", c_int32), ("bwd_split", c_int32),
                ("hsq", c_int64), ("hsk", c_int64), ("hsv", c_int64), ("hso", c_int64),      # ABI 6: per-tensor head strides
                ("hsdq", c_int64), ("hsdk", c_int64), ("hsdv", c_int64), ("hsdo", c_int64)]  # (0 = hd: heads packed in the row)


class AdamWArgs(Structure):
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("shadow", c_void_p),
                ("sumsq", c_void_p), ("g_bf16", c_void_p), ("ema", c_void_p), ("n", c_int64),
                ("lr", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float),
                ("bias_corr1", c_float), ("bias_corr2", c_float), ("max_norm", c_float), ("grad_scale", c_float),
                ("ema_smoothing", c_float), ("zero_grad", c_int32), ("ema_mode", c_int32)]


SUMSQ_PARTIALS = 1024    # MD_SUMSQ_PARTIALS
STATS_ITEM_MAX = 65536   # MD_STATS_ITEM_MAX


class StatsItem(Structure):
    """md_stats_item: one piece (<= STATS_ITEM_MAX elements) of one tensor inside the buffer md_tensor_stats_partial reads."""
    _fields_ = [("src_off", c_int64), ("count", c_int32), ("tensor", c_int32)]


class LoraItem(Structure):
    """md_lora_item: one targeted matrix W [rows, cols] of the flat buffers and its A [rank, cols] / B [rows, rank] inside the adapter's
    flat buffer (offsets in elements); ws_off is written by md_lora_grad_ws_floats."""
    _fields_ = [("w_off", c_int64), ("a_off", c_int64), ("b_off", c_int64), ("ws_off", c_int64), ("rows", c_int32), ("cols", c_int32)]


class MuonItem(Structure):
    """md_muon_item: one targeted matrix W [rows, cols] of the flat buffers under Muon; ws_off is written by md_muon_ws_bytes, scale is
    the shape factor of the update."""
    _fields_ = [("flat_off", c_int64), ("rows", c_int32), ("cols", c_int32), ("ws_off", c_int64), ("scale", c_float), ("reserved", c_int32)]


_sig("md_gemm_bf16", POINTER(GemmArgs), P)
_sig("md_splitk_reduce_flat", P, P, I64, I64, I32, I32, P)
_sig("md_splitk_reduce", P, P, I64, I64, I64, I64, I32, I32, I32, P)
_sig("md_ln_fwd", POINTER(LnArgs), P)
_sig("md_ln_bwd", POINTER(LnArgs), POINTER(LnBwdArgs), P)
_sig("md_qkln_fwd", P, I64, I64, I64, I64, I32, I64, P, F32, P)
_sig("md_qkln_bwd", P, I64, I64, P, I64, I64, I64, I64, I32, I64, I64, P, P)
_sig("md_qkln_fwd_hm", P, I64, I64, I64, I64, I32, I64, P, I64, I64, I32, P, F32, P)
_sig("md_qkln_bwd_hm", P, I64, P, I64, P, I64, I64, I64, I64, I64, I32, I64, I32, P, P)
_sig("md_attn_fwd", POINTER(AttnArgs), P)
_sig("md_attn_fwd_kbias", POINTER(AttnArgs), P, I64, P)      # args, kbias fp32 [B, ldb], ldb
_sig("md_attn_bwd", POINTER(AttnArgs), P)
_sig("md_swiglu_fwd", P, I64, P, I64, I64, I64, P)
_sig("md_swiglu_bwd", P, I64, P, I64, P, I64, I64, I64, P)
_sig("md_gate_bwd", P, P, P, I64, P, P, I64, I64, I64, I64, I64, P)
_sig("md_act_fwd", P, P, I64, I32, P)
_sig("md_act_bwd", P, P, P, I64, I32, P)
_sig("md_colsum", P, I32, I64, P, I64, I64, P)
_sig("md_cast_f32_bf16", P, P, I64, P, P)
_sig("md_cast_f32_bf16_clear", P, P, I64, P)
_sig("md_cast_rows_bf16", P, I32, P, I64, I64, P, I64, P)
_sig("md_mean_tokens", P, P, I64, I64, I64, P)
_sig("md_mean_tokens_bwd", P, P, I64, I64, I64, P)
_sig("md_add_bf16", P, P, P, I64, P)
_sig("md_fill_zero", P, I64, P)
_sig("md_get_mask", P, I64, I64, I64, P, P, P, P)
_sig("md_gather_rows", P, I64, P, P, I64, I64, I64, P)
_sig("md_scatter_rows", P, I64, P, P, I64, I64, I64, P)
_sig("md_moe_route", P, P, I64, I64, I64, I32, I32, P, P, P, P)
_sig("md_moe_combine", P, P, P, P, P, I64, P, P, I64, I64, I32, I32, I64, P)
_sig("md_moe_combine_bwd", P, P, P, P, P, P, I64, I64, P)
_sig("md_moe_dispatch_bwd", P, P, P, P, I64, P, P, I64, I64, I64, I32, I32, I64, P)
# masked-expert pruning of the last patch-mixer block: compact lists of the routed rows whose token survives the mask
_sig("md_moe_compact_kept", P, P, P, I64, I64, I64, I32, I32, P, P, P, P, P, I64, P)
_sig("md_moe_gather_compact", P, I64, P, P, I32, I64, I64, I64, P)
_sig("md_moe_combine_abs", P, P, P, P, P, I64, P, P, I64, I64, I32, I64, I64, P)
_sig("md_moe_combine_bwd_compact", P, P, P, P, P, P, I32, I64, I64, I64, P)
_sig("md_moe_dispatch_bwd_abs", P, P, P, P, I64, P, P, I64, I64, I64, I32, I64, I64, P)
_sig("md_edm_prepare", P, P, P, P, P, P, P, I64, I64, F32, F32, F32, P)
_sig("md_edm_prepare_f16", P, P, P, P, P, P, P, P, I64, I64, F32, F32, F32, P)
_sig("md_patchify", P, P, P, I64, I32, I32, I32, I32, P)
_sig("md_timestep_embed", P, P, I64, I32, P)
_sig("md_unpatchify", P, P, I64, P, P, I64, I32, I32, I32, I32, P)
_sig("md_edm_loss", P, P, P, P, P, P, P, P, I64, I64, I32, I32, I32, I32, F32, P)
_sig("md_edm_loss_train", P, P, P, P, P, P, P, P, F32, P, F32, I64, I64, I32, I32, I32, I32, F32, P)
# learned per-noise-level loss weighting (loss_weighting.py): u / exp(-u) per sample, the EDM loss with a per-sample gradient factor,
# the gradient of the weighted objective w.r.t. the C feature weights
_sig("md_logvar_fwd", P, P, P, P, P, P, I64, I32, P)
_sig("md_edm_loss_train_weighted", P, P, P, P, P, P, P, P, F32, P, F32, I64, I64, I32, I32, I32, I32, F32, P, P)
_sig("md_logvar_bwd", P, P, P, P, P, F32, P, P, P, F32, I64, I32, P)
_sig("md_edm_sampler_input", P, P, I64, F32, F32, I32, P)
_sig("md_edm_heun_update", P, P, P, P, P, I64, F32, I32, ctypes.c_double, ctypes.c_double, ctypes.c_double, F32, I32, P)
# token-space forms (the cached sampling path): no fp32 image between the fp64 sampler state and the network's bf16 rows
_sig("md_edm_sampler_patchify", P, P, I64, I32, I32, I32, I32, F32, F32, I32, P)
_sig("md_edm_heun_update_tok", P, P, P, P, P, I64, I32, I32, I32, I32, F32, I32, ctypes.c_double, ctypes.c_double, ctypes.c_double, F32, I32, P)
# opt-in sampler solvers: one linear-multistep update (Euler, DPM-Solver++(2M)) in image and token space, and the churn step
_sig("md_edm_solver_update", P, P, P, P, I64, F32, I32, ctypes.c_double, F32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, P)
_sig("md_edm_solver_update_tok", P, P, P, P, I64, I32, I32, I32, I32, F32, I32, ctypes.c_double, F32, ctypes.c_double, ctypes.c_double,
     ctypes.c_double, ctypes.c_double, P)
_sig("md_edm_churn", P, P, P, I64, ctypes.c_double, P)
# image-conditioned sampling (img2img, inpainting): blend the known latents, at the state's noise level, into the fp64 state (edit.hip)
_sig("md_edm_blend_known", P, P, P, P, I64, I32, I64, I32, ctypes.c_double, P)
# autoguidance: the two-pointer forms of the four update entry points (the second network's output in a buffer of its own)
_sig("md_edm_heun_update_guide", P, P, P, P, P, P, I64, F32, ctypes.c_double, ctypes.c_double, ctypes.c_double, F32, I32, P)
_sig("md_edm_solver_update_guide", P, P, P, P, P, I64, F32, ctypes.c_double, F32, ctypes.c_double, ctypes.c_double, ctypes.c_double,
     ctypes.c_double, P)
_sig("md_edm_heun_update_guide_tok", P, P, P, P, P, P, I64, I32, I32, I32, I32, F32, ctypes.c_double, ctypes.c_double, ctypes.c_double, F32,
     I32, P)
_sig("md_edm_solver_update_guide_tok", P, P, P, P, P, I64, I32, I32, I32, I32, F32, ctypes.c_double, F32, ctypes.c_double, ctypes.c_double,
     ctypes.c_double, ctypes.c_double, P)
# guidance modes (CFG rescale, APG): per-sample moments and coefficients, then the update kernels with D = alpha_b * D_c + gamma_b * M
GUIDANCE_RESCALE, GUIDANCE_APG = 1, 2       # MD_GUIDANCE_*
F64 = ctypes.c_double
_sig("md_guidance_prepare", P, P, P, P, P, P, I64, I64, F64, F32, I32, F64, F64, F64, I32, F64, F64, I32, P)
_sig("md_guidance_prepare_tok", P, P, P, P, P, P, I64, I32, I32, I32, I32, F64, F32, I32, F64, F64, F64, I32, F64, F64, I32, P)
_sig("md_edm_heun_update_coef", P, P, P, P, P, P, P, I64, I64, F64, F64, F64, F32, I32, P)
_sig("md_edm_solver_update_coef", P, P, P, P, P, P, I64, I64, F64, F32, F64, F64, F64, F64, P)
_sig("md_edm_heun_update_coef_tok", P, P, P, P, P, P, P, I64, I32, I32, I32, I32, F64, F64, F64, F32, I32, P)
_sig("md_edm_solver_update_coef_tok", P, P, P, P, P, P, I64, I32, I32, I32, I32, F64, F32, F64, F64, F64, F64, P)
_sig("md_sumsq", P, I32, I64, P, P)
_sig("md_sumsq_finish", P, I64, P, P)
_sig("md_checksum_u16", P, I64, P, P)
_sig("md_adamw_step", POINTER(AdamWArgs), P)
_sig("md_adamw_step_ranges", POINTER(AdamWArgs), P, P, I32, P)
# training health: per-tensor statistics (optimizer monitor) and the device-side non-finite step guard
_sig("md_tensor_stats_partial", P, I32, P, I64, P, P, P, P)
_sig("md_tensor_stats_finish", P, P, P, P, I32, P, P, P, P)
_sig("md_step_guard", P, P, P)
_sig("md_adamw_step_guarded", POINTER(AdamWArgs), P, P)
_sig("md_adamw_step_ranges_guarded", POINTER(AdamWArgs), P, P, I32, P, P)
# deterministic (atomic-free) forms of the three column reductions; md_det_ws_floats sizes their workspace
_sig("md_det_ws_floats", I32, I64, I64, I64, I64, POINTER(c_int64))
_sig("md_ln_bwd_det", POINTER(LnArgs), POINTER(LnBwdArgs), P, I64, P)
_sig("md_gate_bwd_det", P, P, P, I64, P, P, I64, I64, I64, I64, I64, P, I64, P)
_sig("md_colsum_det", P, I32, I64, P, I64, I64, P, I64, P)
# model diagnostics: loss by noise level, expert-choice routing statistics (md_moe_route_stats_ws_floats sizes the workspace)
_sig("md_loss_sigma_hist", P, P, I64, F32, F32, I32, P, P, P, P)
_sig("md_moe_route_stats_ws_floats", I64, I64, I32, POINTER(c_int64))
_sig("md_moe_route_stats", P, P, I64, P, I64, I64, I32, I32, P, I64, P, P, P)
# post-hoc EMA: up to EMA_MAX_PROFILES power-function averages of the masters in one pass (host arrays of pointers / betas)
_sig("md_ema_power_update", P, P, P, I32, I64, P, P)
_sig("md_ema_power_update_ranges", P, P, P, I32, P, P, I32, P, P)
# LoRA: merge the adapters into the bf16 shadow (or the fp32 masters), project the accumulated gradient onto them (lora.py)
_sig("md_lora_merge", P, P, P, P, I32, I32, F32, P, I32, P)
_sig("md_lora_grad_ws_floats", P, I32, I32, POINTER(c_int64))
_sig("md_lora_grad", P, P, P, P, I32, I32, F32, F32, P, P, I64, P)
# ... and the factored backward: dA, dB of one targeted linear straight from dy and x (lora.LoRA.wgrad)
_sig("md_lora_wgrad_ws_floats", I32, I32, I32, I32, POINTER(c_int64))
_sig("md_lora_wgrad_geometry", I32, I32, I32, I32, POINTER(c_int32), POINTER(c_int32))
_sig("md_lora_wgrad", P, I32, P, I32, I32, I32, I32, P, P, I32, F32, P, P, P, I64, P)
# dispersive loss (disperse.py): the pairwise stage between the Gram and the injection GEMM, and the bounds-checked Gram
_sig("md_disperse_ws_doubles", I64, POINTER(c_int64))
_sig("md_disperse_pairs", P, I64, I64, I64, F32, F64, P, I64, P, P, I64, P, P, F32, P)
_sig("md_disperse_gram_small", P, I64, I64, I64, P, I64, P)
# input gradients: embedded-token gradient -> image gradient, timestep-feature gradient -> dt, bf16 caption rows -> f32 | f16
_sig("md_patch_embed_dgrad", P, I64, P, P, P, I64, I32, I32, I32, I32, I32, POINTER(c_int32), P)
_sig("md_timestep_embed_bwd", P, P, P, I64, I32, P)
_sig("md_cast_rows_from_bf16", P, P, I32, I64, I64, P, I64, P)
PATCH_EMBED_DGRAD_MAX_PV = 64   # MD_PATCH_EMBED_DGRAD_MAX_PV
# measurement-guided sampling: the denoised prediction, the residual / its gradient / the per-sample loss, the cotangent of
# the network output in token rows, and the correction of the fp64 state
_sig("md_edm_denoised", P, P, P, I64, I64, F32, I32, F64, F32, P)
_sig("md_edm_denoised_tok", P, P, P, I64, I32, I32, I32, I32, F32, I32, F64, F32, P)
_sig("md_measure_residual", P, P, P, I32, P, P, I64, I32, I32, I32, I32, P)
_sig("md_guide_cotangent_tok", P, P, I64, I32, I32, I32, I32, F32, I32, F64, F32, P)
_sig("md_edm_guide_apply", P, P, P, P, I64, I64, I32, F64, F64, F32, P)
GUIDE_TINY = 1e-30              # MD_GUIDE_TINY
# step cache: the residual contribution of a run of blocks (the apply step is md_add_bf16), and the two-stage fp64
# distance probe of the adaptive policy (md_step_probe_ws_doubles sizes its workspace)
_sig("md_residual_delta", P, P, P, I64, P)
_sig("md_step_probe_ws_doubles", I64, I64, POINTER(c_int64))
_sig("md_step_probe", P, P, I64, I64, P, P)
_sig("md_step_probe_finish", P, I64, P, P, P)
# Muon (muon.py): workspace layout, momentum + normalise, the Newton-Schulz driver (a C loop over md_gemm_bf16), apply
_sig("md_muon_ws_bytes", P, I32, POINTER(c_int64))
_sig("md_muon_momentum", P, P, P, P, P, I32, F32, I32, F32, P, F32, I32, P, P, P, P, P)
_sig("md_muon_newton_schulz", P, I32, I32, F32, F32, F32, P, P, P)
_sig("md_muon_apply", P, P, P, P, P, I32, F32, F32, I32, F32, P, P, P)
_sig("md_muon_axpby", P, P, P, F32, F32, I64, P)
# cross-attention probe (attn_maps.py): head-averaged probabilities of a short key set added into fp32 rows
_sig("md_attn_probs", POINTER(AttnArgs), P, I64, P, P)
_sig("md_attn_probs_kbias", POINTER(AttnArgs), P, I64, P, I64, P, P)     # args, kbias, ldb, out, ldo, out_rows
# MXFP8 (mxfp8.py): the quantisers, the MX-writing SwiGLU and the block-scaled fp8 GEMM
_sig("md_mx_quant_rows", P, I64, I32, P, I64, P, I64, I64, I64, I32, I64, I64, I64, P)
_sig("md_swiglu_fwd_mx", P, I64, P, I64, P, I64, I64, I64, P)


class GemmMxArgs(Structure):
    """md_gemm_mx_args."""
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("scaleA", c_void_p), ("scaleB", c_void_p), ("C", c_void_p), ("C2", c_void_p),
                ("bias", c_void_p), ("res", c_void_p), ("gate", c_void_p),
                ("M", c_int64), ("N", c_int64), ("K", c_int64),
                ("lda", c_int64), ("ldb", c_int64), ("ldsa", c_int64), ("ldsb", c_int64), ("ldc", c_int64), ("ldc2", c_int64),
                ("ldr", c_int64), ("ldg", c_int64),
                ("sA", c_int64), ("sB", c_int64), ("sScaleA", c_int64), ("sScaleB", c_int64), ("sC", c_int64), ("sC2", c_int64),
                ("sBias", c_int64), ("rows_per_sample", c_int64),
                ("batch", c_int32), ("mode", c_int32), ("act", c_int32), ("reserved", c_int32)]


_sig("md_gemm_mxfp8", POINTER(GemmMxArgs), P)
MX_BLOCK = 32                   # elements per e8m0 scale
ATTN_KBIAS_MAX_KEYS = 256       # Skv of md_attn_fwd_kbias
ATTN_PROBS_MAX_KEYS = 128       # Skv of md_attn_probs
MUON_NORM_PARTS = 16            # MD_MUON_NORM_PARTS
STEP_DELTA_MAX_BLOCKS = 2048    # MD_STEP_DELTA_MAX_BLOCKS
STEP_PROBE_CHUNKS = 1024        # MD_STEP_PROBE_CHUNKS
DISPERSE_MAX_B = 4096    # MD_DISPERSE_MAX_B
LORA_RANKS = (4, 8, 16, 32, 64)
EMA_MAX_PROFILES = 4     # MD_EMA_MAX_PROFILES
ADAMW_MAX_RANGES = 64    # MD_ADAMW_MAX_RANGES


def ema_power_update(p, emas, betas, n, guard=None, flat_off=None, count=None, stream=None, expect=0):
    """md_ema_power_update (or, with flat_off / count -- ctypes int64 arrays or sequences --, its _ranges form).  p / emas / guard:
    ints (device addresses) or torch tensors; betas: Python floats.  expect=None returns the code instead of raising."""
    k = len(emas)
    ev = (c_void_p * max(k, 1))(*[_ptr(e) for e in emas])
    bv = (c_float * max(k, 1))(*[float(b) for b in betas])
    st = stream if stream is not None else stream_ptr()
    if flat_off is None:
        rc = lib().md_ema_power_update(_ptr(p), ev, bv, k, n, _ptr(guard), st)
    else:
        if not isinstance(flat_off, ctypes.Array):
            flat_off, count = (c_int64 * len(flat_off))(*flat_off), (c_int64 * len(count))(*count)
        rc = lib().md_ema_power_update_ranges(_ptr(p), ev, bv, k, flat_off, count, len(flat_off), _ptr(guard), st)
    if expect is None:
        return rc
    check(rc, "md_ema_power_update")


def exported_symbols():
    """Names the header declares (used by the CPU-side ABI test)."""
    return list(_SIGS)


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _ptr(x):
    """A device address from an int, a torch tensor or None."""
    if x is None:
        return None
    return x if isinstance(x, int) else x.data_ptr()


def adamw_step(w, g, m, v, n, *, lr, betas, eps, weight_decay, step, shadow=None, sumsq=None, g_bf16=None, ema=None, ema_smoothing=0.0,
               max_norm=0.0, grad_scale=1.0, zero_grad=1, ema_mode=0, guard=None, ranges=None, stream=None):
    """One AdamW launch: md_adamw_step, with `guard` (the md_step_guard state) its _guarded form, with `ranges` = (flat offsets,
    counts) as ctypes int64 arrays its _ranges form (`n` is then unused), with both md_adamw_step_ranges_guarded.  The only place that
    fills md_adamw_args.  w / g / m / v / shadow / sumsq / g_bf16 / ema / guard: ints (device addresses) or torch tensors; `step`
    (counted from 1) gives the bias corrections 1 - beta ** step."""
    b1, b2 = betas
    a = AdamWArgs(p=_ptr(w), g=_ptr(g), m=_ptr(m), v=_ptr(v), shadow=_ptr(shadow), sumsq=_ptr(sumsq), g_bf16=_ptr(g_bf16), ema=_ptr(ema),
                  n=n, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=weight_decay, bias_corr1=1 - b1 ** step, bias_corr2=1 - b2 ** step,
                  max_norm=max_norm or 0.0, grad_scale=grad_scale, ema_smoothing=ema_smoothing or 0.0, zero_grad=zero_grad, ema_mode=ema_mode)
    name = "md_adamw_step" + ("_ranges" if ranges is not None else "") + ("_guarded" if guard is not None else "")
    args = [byref(a)] + ([ranges[0], ranges[1], len(ranges[0])] if ranges is not None else []) + ([_ptr(guard)] if guard is not None else [])
    check(getattr(lib(), name)(*args, stream if stream is not None else stream_ptr()), name)


def grad_sumsq(partials, out, *, src=None, src_is_bf16=False, n=0, count=SUMSQ_PARTIALS, guard=None, stream=None):
    """The gradient-norm tail: md_sumsq of `src` (n elements, fp32 or bf16) into `partials` when `src` is given, md_sumsq_finish over
    `count` partial sums into `out`, md_step_guard on `out` when `guard` (its state) is given."""
    L, st = lib(), stream if stream is not None else stream_ptr()
    if src is not None:
        check(L.md_sumsq(_ptr(src), 1 if src_is_bf16 else 0, n, _ptr(partials), st), "md_sumsq")
    check(L.md_sumsq_finish(_ptr(partials), count, _ptr(out), st), "md_sumsq_finish")
    if guard is not None:
        check(L.md_step_guard(_ptr(out), _ptr(guard), st), "md_step_guard")


def gemm(A, B, C, M, N, K, *, lda, ldb, ldc, a_kcontig=True, b_kcontig=True, mode=EPI_STORE_BF16,
         act=ACT_NONE, alpha=1.0, bias=None, res=None, ldr=0, gate=None, ldg=0, rows_per_sample=0,
         aux=None, ldaux=0, C2=None, ldc2=0, batch=1, sA=0, sB=0, sC=0, sC2=0, sBias=0, sAux=0, sSplit=0, ksplit=1,
         variant=GEMM_AUTO, raster_group_n=0, timeline=None, stream=None, expect=0, A_list=None, B_list=None, list_segments=0, chosen=None, cu_limit=0,
         tail_ws=None, tail_mode=0, tail_used=None, dact_cached=0):
    """Raw-pointer GEMM launch.  A/B/C/... are ints (device addresses) or torch tensors.  tail_ws: a torch tensor used as the
    workspace of the whole-rounds + split-K-tail form (md_gemm_args.tail_ws); tail_used: list that receives the split it ran with (0 = not used)."""
    a = GemmArgs(_ptr(A), _ptr(B), _ptr(C), _ptr(C2), _ptr(bias), _ptr(res), _ptr(gate), _ptr(aux),
                 M, N, K, lda, ldb, ldc, ldc2, ldr, ldg, ldaux, sA, sB, sC, sC2, sBias, sAux, sSplit,
                 rows_per_sample, batch, ksplit, int(a_kcontig), int(b_kcontig), mode, act, alpha, variant, raster_group_n,
                 _ptr(timeline), None, _ptr(A_list), _ptr(B_list), list_segments, None, 0, cu_limit,
                 _ptr(tail_ws), (tail_ws.numel() * tail_ws.element_size()) if tail_ws is not None else 0, tail_mode, None, dact_cached)
    ch, tu = ctypes.c_int32(-1), ctypes.c_int32(-1)
    a.chosen_variant = ctypes.addressof(ch)
    a.tail_used = ctypes.addressof(tu)
    rc = lib().md_gemm_bf16(byref(a), stream if stream is not None else stream_ptr())
    if chosen is not None:
        chosen.append(ch.value)
    if tail_used is not None:
        tail_used.append(tu.value)
    if expect is None:
        return rc
    check(rc, "md_gemm_bf16")


def mx_quant_rows(src, dst, scales, rows, K, *, ld, ldd, lds, src_kcontig=True, batch=1, sSrc=0, sDst=0, sScale=0, stream=None, expect=0):
    """md_mx_quant_rows: bf16 [rows, K] (K-contiguous, or K-strided with src_kcontig=False) -> fp8 elements + e8m0 scales.  src / dst /
    scales: ints (device addresses) or torch tensors.  expect=None returns the code instead of raising."""
    rc = lib().md_mx_quant_rows(_ptr(src), ld, int(src_kcontig), _ptr(dst), ldd, _ptr(scales), lds, rows, K, batch, sSrc, sDst, sScale,
                                stream if stream is not None else stream_ptr())
    if expect is None:
        return rc
    check(rc, "md_mx_quant_rows")


def gemm_mxfp8(A, scaleA, B, scaleB, C, M, N, K, *, lda, ldb, ldsa, ldsb, ldc, mode=EPI_STORE_BF16, act=ACT_NONE, bias=None, res=None,
               ldr=0, gate=None, ldg=0, rows_per_sample=0, C2=None, ldc2=0, batch=1, sA=0, sB=0, sScaleA=0, sScaleB=0, sC=0, sC2=0, sBias=0,
               stream=None, expect=0):
    """Raw-pointer md_gemm_mxfp8 launch (operands: ints or torch tensors).  expect=None returns the code (NOT_ELIGIBLE: nothing ran)."""
    a = GemmMxArgs(_ptr(A), _ptr(B), _ptr(scaleA), _ptr(scaleB), _ptr(C), _ptr(C2), _ptr(bias), _ptr(res), _ptr(gate), M, N, K,
                   lda, ldb, ldsa, ldsb, ldc, ldc2, ldr, ldg, sA, sB, sScaleA, sScaleB, sC, sC2, sBias, rows_per_sample, batch, mode, act, 0)
    rc = lib().md_gemm_mxfp8(byref(a), stream if stream is not None else stream_ptr())
    if expect is None:
        return rc
    check(rc, "md_gemm_mxfp8")
