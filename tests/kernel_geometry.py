"""The shapes of tests/test_kernel_geometry_gpu.py and tests/test_moe_geometry_gpu.py and the launch geometry each one is meant to reach.

Each case names the heuristic branch it exists for.  The GPU tests run the shapes; tests/test_kernel_geometry_cpu.py reads the
heuristic constants out of the kernel sources and checks, through the functions below, that every shape still lands in the branch
it claims.  A retune of a heuristic then fails on a CPU instead of quietly moving a GPU test off the production path.

The functions restate the launch code of csrc/ with its constants as parameters (K: the dict the CPU test parses)."""
from collections import namedtuple

# ---------------------------------------------------------------------------------------------------------------- heuristics


def nch(C):
    """Chunks of 512 columns per lane: the template instance the LN / qkln / gate_bwd launchers pick (1, 2 or 4)."""
    return 1 if C <= 512 else 2 if C <= 1024 else 4


def ln_fwd_rpw(rows, K):
    """md_ln_fwd: consecutive rows per wave."""
    return max(1, min(K["ln_rpw_max"], -(-rows // K["ln_rpw_rows"])))


def ln_grid_passes(items, K):
    """md_qkln_*: grid-stride passes over `items` waves' worth of rows (4 waves per workgroup, at most ln_grid_max workgroups)."""
    waves = 4 * max(1, min(K["ln_grid_max"], -(-items // 4)))
    return -(-items // waves)


def flat_grid_passes(items, K, key):
    """ew_grid / egrid / rgrid: grid-stride passes over `items` threads' work (256 per workgroup, at most K[key] workgroups)."""
    threads = 256 * max(1, min(K[key], -(-items // 256)))
    return -(-items // threads), items % threads


def finish_chunks(samples, K):
    """ln_bwd_finish_kernel: sample chunks (gridDim.y) and the size of the last one."""
    n = K["finish_chunk"]
    return -(-samples // n), samples - (-(-samples // n) - 1) * n


def loss_finish_strides(B, K):
    """edm_loss_finish_kernel: how many lane-strided steps lane 0 takes over the batch."""
    return -(-B // K["loss_finish_stride"])


# ---------------------------------------------------------------------------------------------------------------- the cases
LnFwd = namedtuple("LnFwd", "id rows rps C mod act pos rpw")           # rpw: rows per wave the case is for
LN_FWD = [
    LnFwd("rpw4-mb1024-C1024-mod", 65536, 64, 1024, True, 0, False, 4),
    LnFwd("rpw4-mb1024-C512-plain", 65536, 64, 512, False, 0, False, 4),
    LnFwd("rpw4-mb1024-C2048-mod-nch4", 65536, 64, 2048, True, 0, False, 4),
    LnFwd("rpw5-crosses-samples-C1024-mod", 78848, 77, 1024, True, 0, False, 5),
    LnFwd("rpw5-crosses-samples-C512-mod", 78848, 77, 512, True, 0, False, 5),
    LnFwd("rpw5-captions-C1024-plain", 78848, 77, 1024, False, 0, False, 5),
    LnFwd("rpw8-C1024-mod", 131072, 256, 1024, True, 0, False, 8),
    LnFwd("rpw8-C512-plain", 131072, 256, 512, False, 0, False, 8),
    LnFwd("rpw2-generic-gelu-tanh-C1024", 16448, 64, 1024, False, 1, False, 2),
    LnFwd("rpw2-generic-pos-C512", 16448, 64, 512, False, 0, True, 2),
]

# form: "mod" (dscale / dshift into a 6 C stride, dscale_is_output), "scratch" (plain: zeroed [samples, C] scratch + dw),
# "rps0" (plain, one sample: rows_per_sample = 0)
LnBwd = namedtuple("LnBwd", "id rows rps C form accumulate")
LN_BWD = [
    LnBwd("mod-rpb64-mb1024-chunks64-acc1", 65536, 64, 1024, "mod", 1),
    LnBwd("mod-rpb64-B40-3chunks-partial-acc0", 65600, 1640, 1024, "mod", 0),
    LnBwd("scratch-dw-rpb32-B520-partial-chunk-acc0", 40040, 77, 512, "scratch", 0),
    LnBwd("scratch-dw-rpb64-B1024-C2048-acc1", 78848, 77, 2048, "scratch", 1),
    LnBwd("rps0-dw-rpb64-acc1", 65536, 0, 1024, "rps0", 1),
]

QkLn = namedtuple("QkLn", "id rows width hd S")
QKLN = [
    QkLn("grid-stride-5-passes-w1152-nch4", 40192, 1152, 64, 256),
    QkLn("grid-stride-5-passes-w512-hd32", 40000, 512, 32, 64),
]

EW_N = 2 ** 24 + 8 * 37          # 2^21 + 37 16-byte items: the second grid-stride pass of ew_grid runs 37 threads
EW_SMALL = 8
Ew = namedtuple("Ew", "id n")
EW = [Ew("second-pass-ragged", EW_N), Ew("n8", EW_SMALL)]
# (rows, C) of the row-shaped elementwise kernels: > 2^21 16-byte items, last pass partial
CAST_ROWS = (77 * 213, 1024)
MEAN_TOKENS = (14564, 2, 1152)    # B, L, C: B * C / 8 = 2^21 + 64 items
GATHER = (16400, 1024)            # rows moved, C: 2^21 + 2048 items (rgrid)

EDM_B, EDM_C, EDM_HW, EDM_P = 130, 4, 64, 2      # 64 x 64 latents (res 512): T = 1024 tokens; 130 * 16384 items > 2^21

GateBwd = namedtuple("GateBwd", "id B rps C rpb")
GATE_BWD = [GateBwd(f"nch{nch(C)}-C{C}-rps{rps}-rpb64", 128, rps, C, 64) for C in (256, 1024, 2048) for rps in (64, 77)]


# ---------------------------------------------------------------------------------------------------------------- MoE routing
# The cases of tests/test_moe_geometry_gpu.py (csrc/routing.hip).
def wave_grid_passes(rows, K):
    """wgrid: grid-stride passes of the wave-per-row kernels over `rows` rows (4 waves per workgroup, at most wgrid_max workgroups),
    and the rows of the last pass."""
    waves = 4 * max(1, min(K["wgrid_max"], -(-rows // 4)))
    return -(-rows // waves), rows - (-(-rows // waves) - 1) * waves


def col_trips(C):
    """Trips of the `for (c = lane * 8; c < C; c += 512)` loops taken by lane 0 (the most any lane takes)."""
    return -(-C // 512)


def emax(E):
    """The template instance of moe_combine_kernel / moe_scatter_sum_kernel the launchers pick."""
    return 8 if E <= 8 else 16


def compact_chunks(B, k, K):
    """md_moe_compact_kept: chunks of compact_chunk list entries per expert (gridDim.x; the chunk-prefix loop strides by 256)."""
    return -(-B * k // K["compact_chunk"])


MoeRoute = namedtuple("MoeRoute", "id B S E k ld special")         # special: sentinel / saturated rows written over the first tokens
MOE_ROUTE = [
    MoeRoute("S100-E4-k25-sentinel-rows", 3, 100, 4, 25, 8, True),
    MoeRoute("S257-E3-k1", 2, 257, 3, 1, 8, False),
    MoeRoute("S300-E16-k-is-S", 2, 300, 16, 300, 16, False),
    MoeRoute("E1", 2, 64, 1, 7, 8, False),
    MoeRoute("S130-E9-odd", 2, 130, 9, 29, 16, False),
    MoeRoute("ld24", 2, 64, 8, 16, 24, False),
    MoeRoute("S16384-lds-64KiB", 1, 16384, 2, 4096, 8, False),
]

# combine / combine backward / dispatch backward on synthetic tables; ldp / ldo: row lengths of probs and dlogits
MoeTable = namedtuple("MoeTable", "id B S E k C ldp ldo")
MOE_SECOND_PASS_M = 5 * 6557                                       # 32768 + 17 token rows
MOE_TABLES = [
    MoeTable("one-lane-E8-C8", 2, 24, 8, 6, 8, 8, 8),
    MoeTable("trips2-one-lane-active-E8-C520", 2, 24, 8, 6, 520, 16, 16),
    MoeTable("trips3-emax16-E12-C1032", 2, 24, 12, 5, 1032, 24, 16),
    MoeTable("emax16-E16-C128", 2, 24, 16, 3, 128, 16, 16),
    MoeTable("odd-E5-C128", 2, 23, 5, 9, 128, 8, 8),
    MoeTable("second-pass-E8-C8", 5, 6557, 8, 1639, 8, 8, 8),
    MoeTable("second-pass-emax16-E12-C8", 5, 6557, 12, 1092, 8, 24, 16),
]
MOE_BWD_SECOND_PASS = 32768 + 17                                   # R of md_moe_combine_bwd, cap of md_moe_combine_bwd_compact (C = 8)

MoeCompact = namedtuple("MoeCompact", "id B S E k len_keep dead")  # dead: an expert all of whose tokens are dropped, or None
MOE_COMPACT = [
    MoeCompact("E16", 3, 32, 16, 8, 8, None),
    MoeCompact("E5-one-expert-keeps-nothing", 3, 32, 5, 8, 8, 2),
    MoeCompact("Bk2048-exact-chunks", 4, 1024, 2, 512, 256, None),
    MoeCompact("chunk-prefix-second-trip-E1", 17, 16384, 1, 16384, 4096, None),
]

MoeMask = namedtuple("MoeMask", "id B T len_keep")
MOE_MASK = [
    MoeMask("T100-keep25", 3, 100, 25),
    MoeMask("T257-keep1", 2, 257, 1),
    MoeMask("T300-keep-all", 2, 300, 300),
    MoeMask("T16384-lds-64KiB", 1, 16384, 4096),
]
