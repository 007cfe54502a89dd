"""Masked-expert pruning, host side: the new entry points are declared, bound and exported under ABI 6, and the new
kernels of routing.hip compile for gfx950 without scratch or spills."""
import ctypes
import os
import re
import subprocess

import pytest

from micro_diffusion_amd import hip, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["md_moe_compact_kept", "md_moe_gather_compact", "md_moe_combine_abs", "md_moe_combine_bwd_compact", "md_moe_dispatch_bwd_abs"]
NEW_KERNELS = ["fill_i32_kernel", "moe_compact_count_kernel", "moe_compact_write_kernel", "gather_rows_compact_kernel", "moe_combine_bwd_compact_kernel"]
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def _declaration(header, name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/microdit_hip.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "microdit_hip.h")).read()
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6, "symbols added, none changed: the ABI version stays"
    for name in NAMES:
        declared = _declaration(header, name)
        assert name in hip.exported_symbols() and name in hip._SIGS, f"{name} is not bound in hip._SIGS"
        restype, argtypes = hip._SIGS[name]
        assert restype is ctypes.c_int and len(declared) == len(argtypes), (name, len(declared), len(argtypes))
        assert declared[-1].split()[0] == "hipStream_t"
        for text, ctype in zip(declared, argtypes):             # pointers and integers line up
            kind = "P" if "*" in text or "hipStream_t" in text else text.split()[-2]
            assert {"P": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[kind] is ctype, (name, text)


def test_the_old_routing_entry_points_keep_their_signatures():
    header = open(os.path.join(ROOT, "include", "microdit_hip.h")).read()
    for name, n in (("md_moe_route", 11), ("md_moe_combine", 14), ("md_moe_combine_bwd", 9), ("md_moe_dispatch_bwd", 14)):
        assert len(_declaration(header, name)) == n == len(hip._SIGS[name][1]), name


@needs_hipcc
def test_built_library_exports_the_entry_points():
    path = hip.build()
    lib = ctypes.CDLL(path)
    assert lib.md_abi_version() == 6
    dyn = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in dyn.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in exported and hasattr(lib, name), f"{name} is not exported by the built library"


@needs_hipcc
def test_new_kernels_compile_without_scratch_or_spills(tmp_path):
    res = native.resource_usage("routing.hip", hip.HIPCC_FLAGS, tmp_path / "routing.o")
    for kern in NEW_KERNELS:
        hits = {k: v for k, v in res.items() if kern in k}
        assert len(hits) == 1, (kern, sorted(res))
        for k, v in hits.items():
            print(k, v)
            assert v["scratch"] == 0 and v["spill"] == 0, (k, v)
    # the absolute-position entry points launch the existing combine / scatter-sum / softmax-backward kernels (k = 0): no new variants
    assert sum("moe_combine_kernel" in k for k in res) == 2 and sum("moe_scatter_sum_kernel" in k for k in res) == 2, sorted(res)
