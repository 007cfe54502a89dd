"""CPU guard of tests/test_kernel_geometry_gpu.py: the launch-heuristic constants are read out of the kernel sources, and every GPU
case must still land in the branch its id names.  A retune of a heuristic fails here instead of moving a GPU test silently off the
production path."""
import os
import re

import pytest

from tests import kernel_geometry as kg

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "micro_diffusion_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _body(src, head):
    """The text of the function / kernel whose definition starts with `head`, up to its closing brace at column 0."""
    i = src.index(head)
    return src[i:src.index("\n}", i)]


def _one(pattern, text, what):
    hits = re.findall(pattern, text)
    assert len(hits) == 1, f"{what}: expected one match of {pattern!r}, found {hits}"
    return int(hits[0])


def _cap(src, fn):
    """The workgroup cap of a flat grid helper `inline int fn(int64_t ...) { ... if (g > N) g = N; ... }`."""
    body = _body(src, f"inline int {fn}(")
    n = _one(r"if \(g > (\d+)\) g = \1;", body, fn)
    assert "+ 255) / 256" in body or "+ 3) / 4" in body, f"{fn}: the per-workgroup work changed"
    return n


@pytest.fixture(scope="module")
def K():
    norm, ew, edm, rt = _src("norm.hip"), _src("elementwise.hip"), _src("edm.hip"), _src("routing.hip")
    fwd = _body(norm, 'extern "C" int md_ln_fwd(')
    div = _one(r"rpw = \(a->rows \+ (\d+)\) / (?:\d+);", fwd, "md_ln_fwd rows per wave")
    assert f"(a->rows + {div}) / {div + 1};" in fwd, "md_ln_fwd: rows per wave is no longer ceil(rows / N)"
    finish = _body(norm, "__global__ __launch_bounds__(256) void ln_bwd_finish_kernel(")
    chunk = _one(r"blockIdx\.y \* (\d+);", finish, "ln_bwd_finish_kernel chunk")
    assert f"float sv[{chunk}], mv[{chunk}];" in finish
    bwd = _body(norm, 'extern "C" int md_ln_bwd(')
    assert f"(nsmp + {chunk - 1}) / {chunk}" in bwd, "md_ln_bwd: the finish grid no longer uses the kernel's chunk"
    lf = _body(edm, "__global__ __launch_bounds__(64) void edm_loss_finish_kernel(")
    stride = _one(r"b < B; b \+= (\d+)\)", lf, "edm_loss_finish_kernel stride")
    assert "int64_t b = threadIdx.x;" in lf
    for launch in re.findall(r"edm_loss_finish_kernel, dim3\(1\), dim3\((\d+)\)", edm):
        assert int(launch) == stride, "edm_loss_finish_kernel launched with a different lane count than its stride"
    k = {"ln_rpw_rows": div + 1,
         "ln_rpw_max": _one(r"if \(rpw > (\d+)\) rpw = \1;", fwd, "md_ln_fwd rows-per-wave cap"),
         "ln_grid_max": _cap(norm, "ln_grid"),
         "ew_grid_max": _cap(ew, "ew_grid"),
         "egrid_max": _cap(edm, "egrid"),
         "rgrid_max": _cap(rt, "rgrid"),
         "finish_chunk": chunk,
         "loss_finish_stride": stride}
    # the NCH template choice of the row kernels (kg.nch)
    for text in (fwd, bwd, _body(ew, 'extern "C" int md_gate_bwd(')):
        assert re.search(r"C <= 512\) \w+\(1(, \w+)?\); else if \(C <= 1024\) \w+\(2", text.replace("a->", "")), text[:80]
    return k


def test_constants_read(K):
    """The values the cases were sized for (a retune must re-size the cases, not just pass this)."""
    assert K == {"ln_rpw_rows": 16384, "ln_rpw_max": 8, "ln_grid_max": 4096, "ew_grid_max": 8192, "egrid_max": 8192,
                 "rgrid_max": 8192, "finish_chunk": 16, "loss_finish_stride": 64}


@pytest.mark.parametrize("case", kg.LN_FWD, ids=[c.id for c in kg.LN_FWD])
def test_ln_fwd_geometry(K, case):
    rpw = kg.ln_fwd_rpw(case.rows, K)
    assert rpw == case.rpw, (case.id, rpw)
    assert f"rpw{rpw}" in case.id
    assert case.rows % case.rps == 0
    assert f"nch{kg.nch(case.C)}" in case.id or kg.nch(case.C) < 4
    assert ("crosses-samples" in case.id) == (case.rps % rpw != 0 and case.mod), "a case whose waves straddle samples must say so"
    if case.act or case.pos:
        assert case.rows > K["ln_rpw_rows"], "the generic path must run past one row per wave"


def test_ln_fwd_coverage():
    assert {c.rpw for c in kg.LN_FWD} >= {4, 5, 8}
    assert {kg.nch(c.C) for c in kg.LN_FWD} == {1, 2, 4}
    assert any(c.act == 1 for c in kg.LN_FWD) and any(c.pos for c in kg.LN_FWD)


@pytest.mark.parametrize("case", kg.LN_BWD, ids=[c.id for c in kg.LN_BWD])
def test_ln_bwd_geometry(K, case):
    from micro_diffusion_amd.engine import DiTEngine
    rps = case.rps if case.rps > 0 else case.rows
    assert case.rows % rps == 0
    rpb = DiTEngine._rows_per_block(case.rows, rps, 1024)
    assert f"rpb{rpb}-" in case.id, (case.id, rpb)
    samples = case.rows // rps
    chunks, last = kg.finish_chunks(samples, K)
    if "chunks64" in case.id:
        assert chunks == 64
    if "3chunks-partial" in case.id:
        assert chunks == 3 and last < K["finish_chunk"]
    if "partial-chunk" in case.id:
        assert chunks >= 3 and last < K["finish_chunk"]
    assert (case.rps == 0) == (case.form == "rps0")


def test_ln_bwd_coverage(K):
    from micro_diffusion_amd.engine import DiTEngine
    assert {c.form for c in kg.LN_BWD} == {"mod", "scratch", "rps0"}
    assert {c.accumulate for c in kg.LN_BWD} == {0, 1}
    assert any(DiTEngine._rows_per_block(c.rows, c.rps or c.rows, 1024) == 64 for c in kg.LN_BWD), "rpb 64 = 16 rows per wave"
    assert any(kg.finish_chunks(c.rows // c.rps, K)[0] >= 3 and kg.finish_chunks(c.rows // c.rps, K)[1] < K["finish_chunk"]
               for c in kg.LN_BWD if c.rps and c.rows // c.rps >= 33)


@pytest.mark.parametrize("case", kg.QKLN, ids=[c.id for c in kg.QKLN])
def test_qkln_geometry(K, case):
    passes = kg.ln_grid_passes(case.rows * 2, K)          # q and k: two work items per row
    assert passes == 5 and f"{passes}-passes" in case.id
    assert (case.rows * 2) % (4 * K["ln_grid_max"]) != 0, "the last pass must be partial"
    assert case.rows % case.S == 0 and case.width % case.hd == 0


def test_elementwise_geometry(K):
    n8 = kg.EW_N // 8
    assert kg.flat_grid_passes(n8, K, "ew_grid_max") == (2, 37)
    assert kg.flat_grid_passes(kg.EW_SMALL // 8, K, "ew_grid_max") == (1, 1)
    rows, C = kg.CAST_ROWS
    passes, tail = kg.flat_grid_passes(rows * C // 8, K, "ew_grid_max")
    assert passes == 2 and tail % 256 != 0
    B, L, C = kg.MEAN_TOKENS
    assert kg.flat_grid_passes(B * C // 8, K, "ew_grid_max")[0] == 2
    assert kg.flat_grid_passes(B * L * C // 8, K, "ew_grid_max")[0] >= 2
    n, C = kg.GATHER
    assert kg.flat_grid_passes(n * C // 8, K, "rgrid_max")[0] == 2


def test_edm_geometry(K):
    B, C, HW, p = kg.EDM_B, kg.EDM_C, kg.EDM_HW, kg.EDM_P
    items = B * C * HW * HW
    passes, _ = kg.flat_grid_passes(items, K, "egrid_max")
    assert passes == 2, "prepare / patchify / unpatchify must take a second grid-stride pass"
    per = C * HW * HW
    assert any(b * per >= 256 * K["egrid_max"] for b in range(B)), "some sample's sigma must be written in the second pass"
    assert kg.loss_finish_strides(B, K) == 3
    assert (HW // p) ** 2 == 1024


@pytest.mark.parametrize("case", kg.GATE_BWD, ids=[c.id for c in kg.GATE_BWD])
def test_gate_bwd_geometry(case):
    assert f"nch{kg.nch(case.C)}-" in case.id and case.rpb == 64


def test_gate_bwd_coverage():
    assert {kg.nch(c.C) for c in kg.GATE_BWD} == {1, 2, 4}
    assert any(c.C == 1024 for c in kg.GATE_BWD), "NCH = 2 fully used"
    assert {c.rps for c in kg.GATE_BWD} == {64, 77}
