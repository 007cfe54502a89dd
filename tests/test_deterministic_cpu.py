"""Deterministic mode, host side (no GPU): the four entry points are declared and bound, and md_det_ws_floats -- a host-only function
of libmicrodit_hip.so -- answers the workspace sizes include/microdit_hip.h documents:
  gate_bwd  samples * chunks * C             (0 with one chunk per sample),  chunks = ceil(rows_per_sample / rows_per_block)
  ln_bwd    2 * samples * chunks * C         (0 with one chunk) + ceil(samples / 16) * C  (0 with one group of 16 samples)
  colsum    blocks * C                       (0 with one row block), blocks from the library's own rows-per-workgroup rule
"""
import ctypes
import os
import re

import pytest

from micro_diffusion_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["md_det_ws_floats", "md_gate_bwd_det", "md_ln_bwd_det", "md_colsum_det"]


def test_header_declares_and_binding_lists_the_entry_points():
    with open(os.path.join(ROOT, "include", "microdit_hip.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"^int\s+(md_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared, f"{name} is not declared at the start of a line of microdit_hip.h"
        assert name in hip.exported_symbols(), f"{name} is missing from hip._SIGS"
    assert re.search(r"enum md_det_kind \{ MD_DET_GATE_BWD = 0, MD_DET_LN_BWD = 1, MD_DET_COLSUM = 2 \};", header)
    assert (hip.DET_GATE_BWD, hip.DET_LN_BWD, hip.DET_COLSUM) == (0, 1, 2)
    assert re.search(r"#define MD_ABI_VERSION 6\b", header), "the change only adds symbols: the ABI version stays"


def _floats(L, kind, rows, rps, rpb, C):
    out = ctypes.c_int64(-7)
    rc = L.md_det_ws_floats(kind, rows, rps, rpb, C, ctypes.byref(out))
    return rc, out.value


@pytest.fixture(scope="module")
def L():
    return hip.lib()


# (rows, rows_per_sample, rows_per_block, C) -> floats
GATE = [((150, 50, 16, 384), 3 * 4 * 384),        # rows_per_sample not divisible by rows_per_block: ceil(50 / 16) = 4 chunks
        ((128, 64, 16, 1024), 2 * 4 * 1024),
        ((128, 64, 4, 1152), 2 * 16 * 1152),
        ((64, 16, 16, 768), 0),                   # one chunk: no workspace
        ((64, 16, 64, 768), 0)]
LN = [((150, 50, 16, 384), 2 * 3 * 4 * 384),
      ((128, 64, 4, 1152), 2 * 2 * 16 * 1152),
      ((320, 8, 4, 256), 2 * 40 * 2 * 256 + 3 * 256),     # 40 samples: three groups of 16 for the weight gradient
      ((320, 8, 8, 256), 3 * 256),                        # one chunk, three groups
      ((64, 0, 16, 256), 2 * 1 * 4 * 256),                # rows_per_sample 0: one sample of 64 rows
      ((64, 16, 16, 768), 0)]
# (rows, C) -> floats, with the rule of md_colsum: 128 rows per workgroup, halved down to 8 while there are fewer than 512 workgroups
COLSUM = [((1000, 520), 125 * 520), ((300, 48), 38 * 48), ((4096, 264), 256 * 264), ((65536, 1152), 512 * 1152), ((8, 64), 0)]


@pytest.mark.parametrize("shape,want", GATE)
def test_ws_floats_gate_bwd(L, shape, want):
    assert _floats(L, hip.DET_GATE_BWD, *shape) == (0, want)


@pytest.mark.parametrize("shape,want", LN)
def test_ws_floats_ln_bwd(L, shape, want):
    assert _floats(L, hip.DET_LN_BWD, *shape) == (0, want)


@pytest.mark.parametrize("shape,want", COLSUM)
def test_ws_floats_colsum(L, shape, want):
    rows, C = shape
    assert _floats(L, hip.DET_COLSUM, rows, 0, 0, C) == (0, want)
    assert _floats(L, hip.DET_COLSUM, rows, 77, 5, C) == (0, want), "rows_per_sample / rows_per_block are ignored for colsum"


def test_ws_floats_bad_arguments(L):
    assert L.md_det_ws_floats(hip.DET_GATE_BWD, 128, 64, 16, 1024, None) == -1
    assert L.md_det_ws_floats(hip.DET_COLSUM, 128, 0, 0, 1024, None) == -1
    for kind in (hip.DET_GATE_BWD, hip.DET_LN_BWD):
        assert _floats(L, kind, 128, 64, 16, 100) == (-1, -7), "C % 8 != 0"
        assert _floats(L, kind, 128, 64, 0, 1024) == (-1, -7), "rows_per_block 0"
        assert _floats(L, kind, 128, 64, -4, 1024) == (-1, -7), "rows_per_block < 0"
        assert _floats(L, kind, 130, 64, 16, 1024) == (-1, -7), "rows not a multiple of rows_per_sample"
    assert _floats(L, 3, 128, 64, 16, 1024) == (-1, -7), "unknown kind"
    assert _floats(L, hip.DET_COLSUM, 0, 0, 0, 64) == (-1, -7)
