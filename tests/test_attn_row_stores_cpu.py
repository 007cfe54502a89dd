"""Host model of the LINES store form of csrc/attention.hip (store_lines), no GPU needed -- in the style of
test_two_phase_lds_choreography (tests/test_attn_static_cpu.py).

A wave parks its 32 x hd result rows as bf16 in its own 32-row part of a dead LDS image (8 bytes per lane and column group, lane <-> row),
reads them back row-contiguously (16 bytes per lane, hd / 8 lanes per row) and stores whole head slices.  Checked per kernel family,
workgroup size and head_dim: the parked bytes of a wave tile its 32-row region without overlap, the regions of the waves do not overlap
and never reach past the image, every byte read back was written by the same wave, and element (row, column) of the accumulator tile
arrives at dst0 + row * ld + column exactly once for rows < nvalid and never otherwise."""
import pytest

STG = 32


def _park(lane, hd):
    """(byte offset in the wave's region, row, first column) of the 8-byte LDS writes of one lane: acc[di][4 g .. 4 g + 3]."""
    pk, hh = (hd + 8) * 2, lane >> 5
    for di in range(hd // 32):
        for g in range(4):
            col = di * 32 + 8 * g + 4 * hh
            yield (lane & 31) * pk + col * 2, lane & 31, col


def _read_back(lane, hd):
    """(byte offset, row, first column) of the 16-byte LDS reads of one lane; the global store goes to dst0 + row * ld + column."""
    pk, cpr = (hd + 8) * 2, hd // 8
    rpi = 64 // cpr
    for it in range(32 // rpi):
        r, c = it * rpi + lane // cpr, lane % cpr
        yield r * pk + c * 16, r, c * 8


# (family, rows of the dead image, waves of the workgroup): every wave w uses rows [32 w, 32 w + 32) of the image
def _images():
    for nw in (1, 2):
        yield "attn_fwd_kernel: K / V staging tiles", 2 * STG, nw
    for sch, nws in ((128, (6, 7, 8)), (64, (3, 4))):
        for nw in nws:
            yield f"attn_bwd_dkv_stream_kernel: Q / dO chunk tiles, {sch}-row chunks", 2 * sch, nw
    for skp in (64, 96, 256):
        yield "attn_bwd_fused_kernel: K tile (dK), V tile (dV)", skp, skp // 32
    for sqp, skp in ((64, 64), (64, 96), (96, 64), (96, 96)):
        yield "attn_bwd_fused2_kernel: tile A (dK), tile B (dV)", max(sqp, skp), skp // 32


@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("family,image_rows,nwaves", list(_images()))
def test_lines_regions_inside_the_image(family, image_rows, nwaves, hd):
    pk = (hd + 8) * 2
    seen = set()
    for w in range(nwaves):
        region = range(w * 32 * pk, (w + 1) * 32 * pk)
        assert region.stop <= image_rows * pk, f"{family}: wave {w} reaches past the image"
        assert not (seen & set(region))
        seen |= set(region)


@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("nvalid", [32, 13, 1, 0])
def test_lines_route(hd, nvalid):
    pk = (hd + 8) * 2
    lds = {}                                  # byte -> (row, column) of the accumulator element whose bf16 it holds
    for lane in range(64):
        for off, row, col in _park(lane, hd):
            assert off % 8 == 0 and off + 8 <= 32 * pk
            for e in range(4):
                for byte in (0, 1):
                    assert off + 2 * e + byte not in lds, "two lanes park into the same byte"
                    lds[off + 2 * e + byte] = (row, col + e)
    assert len(lds) == 32 * hd * 2            # the wave's 32 x hd tile, nothing of the pitch padding
    stored = {}
    for lane in range(64):
        for off, r, c0 in _read_back(lane, hd):
            assert off % 16 == 0 and off + 16 <= 32 * pk
            for e in range(8):
                assert lds[off + 2 * e] == lds[off + 2 * e + 1] == (r, c0 + e), "read back from bytes another element was parked in"
                if r < nvalid:
                    assert (r, c0 + e) not in stored
                    stored[(r, c0 + e)] = lds[off + 2 * e]
    assert stored == {(r, c): (r, c) for r in range(nvalid) for c in range(hd)}


@pytest.mark.parametrize("hd", [64, 32])
def test_wide_route(hd):
    """WIDE (store_rows): after the half-wave exchange of groups (g, g + 1), lane L stores columns di 32 + 8 g + 8 hh .. + 7 of row L & 31
    as (a0, a1, b0, b1): lower half-wave keeps its a (group g), takes the partner's a as b; upper keeps its b, takes the partner's b as a."""
    stored = {}
    for lane in range(64):
        hh, partner = lane >> 5, lane ^ 32
        for di in range(hd // 32):
            for g in (0, 2):
                own = lambda L, grp: [(L & 31, di * 32 + 8 * grp + 4 * (L >> 5) + e) for e in range(4)]
                # v_permlane32_swap(a, b): a of the upper half <-> b of the lower half
                a = own(lane, g) if hh == 0 else own(partner, g + 1)
                b = own(partner, g) if hh == 0 else own(lane, g + 1)
                col0 = di * 32 + 8 * g + 8 * hh
                for e, src in enumerate(a + b):
                    assert src == (lane & 31, col0 + e)
                    assert src not in stored
                    stored[src] = True
    assert len(stored) == 32 * hd
