"""Hardware-semantics probes (tests only): tests/probes/hw_probes.hip -> tests/probes/libmd_probes.so, bound with ctypes.
Kept out of the product library and its header; `__graft_entry__.build()` compiles it so it travels to the GPU box."""
import ctypes
import os
from ctypes import c_int32, c_int64, c_void_p as P

from micro_diffusion_amd import native

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "hw_probes.hip")
_HASHED = [_SRC, os.path.join(native.CSRC, "md_common.h")]       # hw_probes.hip includes md_common.h
LIB_PATH = os.path.join(_HERE, "libmd_probes.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared"]
_SIGS = {"mdp_tr_probe": (c_int32, [P, P, P]), "mdp_mfma_probe": (c_int32, [P, P, P, P]),
         "mdp_vmcnt_order_probe": (c_int32, [P, c_int64, P, P, c_int32, P]), "mdp_cu_hog": (c_int32, [c_int32, c_int64, P, P])}


def build(force: bool = False) -> str:
    return native.build(LIB_PATH, native.source_hash(_HASHED, FLAGS),
                        lambda tmp: native.run([native.hipcc(), *FLAGS, _SRC, "-o", tmp]), force)


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = native.load(build(), _SIGS)
    return _lib
