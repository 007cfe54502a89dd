"""CPU guard of tests/test_kernel_geometry_gpu.py and tests/test_moe_geometry_gpu.py: the launch-heuristic constants are read out of the kernel sources, and every GPU
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


def _wgrid_cap(rt):
    """wgrid: one wave per row, four rows per workgroup, capped."""
    body = _body(rt, "inline int wgrid(")
    assert "(rows + 3) / 4" in body, "wgrid: the per-workgroup work changed"
    return _one(r"if \(g > (\d+)\) g = \1;", body, "wgrid")


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
         "wgrid_max": _wgrid_cap(rt),
         "compact_chunk": _one(r"constexpr int CK = (\d+);", rt, "compaction chunk"),
         "finish_chunk": chunk,
         "loss_finish_stride": stride}
    # the NCH template choice of the row kernels (kg.nch)
    for text in (fwd, bwd, _body(ew, 'extern "C" int md_gate_bwd(')):
        assert re.search(r"C <= 512\) \w+\(1(, \w+)?\); else if \(C <= 1024\) \w+\(2", text.replace("a->", "")), text[:80]
    return k


def test_constants_read(K):
    """The values the cases were sized for (a retune must re-size the cases, not just pass this)."""
    assert K == {"ln_rpw_rows": 16384, "ln_rpw_max": 8, "ln_grid_max": 4096, "ew_grid_max": 8192, "egrid_max": 8192,
                 "rgrid_max": 8192, "wgrid_max": 8192, "compact_chunk": 1024, "finish_chunk": 16, "loss_finish_stride": 64}


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


# ---------------------------------------------------------------------------------------------------------------- MoE routing
def test_moe_emax_split():
    """The four launchers pick the <8> instance for E <= 8 and <16> otherwise, through wgrid: what kg.emax and the EMAX cases assume."""
    rt = _src("routing.hip")
    for fn, kernel in (("md_moe_combine", "moe_combine_kernel"), ("md_moe_combine_abs", "moe_combine_kernel"),
                       ("md_moe_dispatch_bwd", "moe_scatter_sum_kernel"), ("md_moe_dispatch_bwd_abs", "moe_scatter_sum_kernel")):
        body = _body(rt, f'extern "C" int {fn}(')
        assert re.search(rf"if \(E <= 8\)\s+hipLaunchKernelGGL\({kernel}<8>, dim3\(wgrid\((B \* S|M)\)\).*?else\s+hipLaunchKernelGGL\({kernel}<16>, "
                         rf"dim3\(wgrid\((B \* S|M)\)\)", body, re.S), fn
        assert "E > 16" in body, f"{fn}: E above the largest instance must be refused"
    assert kg.emax(8) == 8 and kg.emax(9) == 16
    for fn in ("md_moe_combine_bwd(", "md_moe_combine_bwd_compact("):
        assert "dim3(wgrid(" in _body(rt, f'extern "C" int {fn}'), fn
    assert len(re.findall(r"for \(int c = lane \* 8; c < C; c \+= 512\)", rt)) == 4, "the column loops kg.col_trips restates"


@pytest.mark.parametrize("case", kg.MOE_TABLES, ids=[c.id for c in kg.MOE_TABLES])
def test_moe_table_geometry(K, case):
    M = case.B * case.S
    passes, last = kg.wave_grid_passes(M, K)
    if "second-pass" in case.id:
        assert M == kg.MOE_SECOND_PASS_M and passes == 2 and 0 < last < 4 * K["wgrid_max"], "exactly two passes, the last partial"
        assert last < case.S, "the rows of the second pass belong to the last sample"
    else:
        assert passes == 1
    assert ("emax16" in case.id) == (kg.emax(case.E) == 16)
    trips = kg.col_trips(case.C)
    assert f"trips{trips}" in case.id or trips == 1
    if "one-lane" in case.id:
        assert case.C % 512 == 8, "the last trip has lane 0 alone"
    assert case.E <= case.ldo <= 16 and case.E <= case.ldp and case.k < case.S and case.C % 8 == 0


def test_moe_table_coverage(K):
    cs = [c.C for c in kg.MOE_TABLES]
    assert any(0 < c <= 512 for c in cs) and any(512 < c <= 1024 for c in cs) and any(c > 1024 for c in cs)
    assert {kg.emax(c.E) for c in kg.MOE_TABLES if "second-pass" in c.id} == {8, 16}
    assert {(c.ldp, c.ldo) for c in kg.MOE_TABLES} >= {(8, 8), (16, 16), (24, 16)}
    assert any(c.E == 16 and (c.ldp, c.ldo) == (16, 16) for c in kg.MOE_TABLES), "E = 16: dlogits without padding"
    assert any(c.E < c.ldo for c in kg.MOE_TABLES) and any(c.E % 2 == 1 for c in kg.MOE_TABLES)
    passes, last = kg.wave_grid_passes(kg.MOE_BWD_SECOND_PASS, K)
    assert passes == 2 and 0 < last < 4 * K["wgrid_max"]


def test_moe_compact_geometry(K):
    ck = K["compact_chunk"]
    rt = _src("routing.hip")
    assert "for (int j = tid; j < nchunk; j += 256)" in _body(rt, "void moe_compact_write_kernel("), "the chunk-prefix loop changed"
    by_id = {c.id: c for c in kg.MOE_COMPACT}
    c = by_id["chunk-prefix-second-trip-E1"]
    assert kg.compact_chunks(c.B, c.k, K) > 256, "the chunk-prefix loop must take a second trip"
    c = by_id["Bk2048-exact-chunks"]
    assert c.B * c.k == 2 * ck
    assert any(kg.emax(c.E) == 16 for c in kg.MOE_COMPACT)
    for c in kg.MOE_COMPACT:
        assert c.k <= c.S and 0 < c.len_keep <= c.S and c.B * c.S < 2 ** 31 and kg.compact_chunks(c.B, c.k, K) <= 65535
        if c.dead is not None:
            assert c.k <= c.S - c.len_keep and c.dead < c.E, "an expert can only keep nothing if k dropped tokens exist"


def test_moe_route_and_mask_cases():
    rt = _src("routing.hip")
    smax = _one(r"k > S \|\| S > (\d+)\)", _body(rt, 'extern "C" int md_moe_route('), "md_moe_route's largest S")
    tmax = _one(r"len_keep > T \|\| T > (\d+)\)", _body(rt, 'extern "C" int md_get_mask('), "md_get_mask's largest T")
    assert smax == tmax == 16384 and smax * 4 == 64 * 1024, "the accepted maximum is 64 KiB of dynamic LDS"
    assert any(c.S == smax for c in kg.MOE_ROUTE) and any(c.T == tmax for c in kg.MOE_MASK)
    assert any(c.S % 256 for c in kg.MOE_ROUTE) and any(c.k == c.S for c in kg.MOE_ROUTE) and any(c.k == 1 for c in kg.MOE_ROUTE)
    assert any(c.E == 1 for c in kg.MOE_ROUTE) and any(c.E % 2 and c.E > 8 for c in kg.MOE_ROUTE) and any(c.ld > 16 for c in kg.MOE_ROUTE)
    assert sum(c.special for c in kg.MOE_ROUTE) == 1
    assert any(c.len_keep == c.T for c in kg.MOE_MASK) and any(c.len_keep == 1 for c in kg.MOE_MASK)
    for c in kg.MOE_ROUTE:
        assert c.E <= c.ld and c.k <= c.S
