"""Split-K planning for the GEMMs whose output is too small to fill the chip (weight gradients, skinny data gradients, the grouped
launches of a backward): pure arithmetic on shapes -- no torch, no ctypes, no engine.  DiTEngine asks a plan here, builds the ctypes
table and launches; tests/test_splitk_plan_cpu.py holds the plans of the real shapes.  The cost model is the one of the persistent
256 x 256 kernel (pp256): tiles x splits work items are dealt out to the CUs, a workgroup pays per 64-deep k-tile and per fp32 slice
it writes, and the slice reduction moves (ks + 2) x the output once."""
from typing import NamedTuple

NUM_CU = 256                 # MI355X: one persistent workgroup per CU
K_TILE = 64                  # contraction depth of one k-tile of pp256
K_TILE_US = 1.9              # a workgroup's time per k-tile (profiles/r2_wgrad_splitk_pp256.txt)
SLICE_US = 5.0               # ... and to write one 256 x 256 fp32 slice (profiles/r2_wgrad_splitk_pp256.txt)
HBM_BYTES_PER_US = 4e6       # ~4 TB/s: the slice reduction's rate (profiles/r2_wgrad_splitk_pp256.txt)
K_UNIT = 128                 # pp256 takes a contraction per split that is a multiple of this
PP256_MIN_ITEMS = 192        # md_gemm_bf16's AUTO rule sends launches with fewer work items to the 2-stage kernels
MAX_SPLITS = 64
SHORT_K, SHORT_K_MIN_TILES = 512, 64     # a contraction this short into this many tiles is pure output traffic: accumulate in place
TILE128_MIN_K = 512          # the round-1 rule for the 2-stage 128 x 128 kernels: at least this much k per split


def tiles(rows, cols, edge=256):
    return ((rows + edge - 1) // edge) * ((cols + edge - 1) // edge)


def pp256_cost_us(t256, ks, k_per_split, out_elems):
    """Microseconds of a pp256 launch of t256 output tiles split ks ways plus the reduction of its fp32 slices."""
    rounds = -(-t256 * ks // NUM_CU)
    return rounds * (k_per_split / K_TILE * K_TILE_US + SLICE_US) + (ks + 2) * (out_elems * 4 / HBM_BYTES_PER_US)


def choose_ksplit(out_rows, out_cols, contraction, batch=1, *, ws_floats, target_blocks=768, min_items=PP256_MIN_ITEMS, short_k_accum=True):
    """Split-K factor of one fp32-output GEMM; 1: none (accumulate epilogue); -1: none, but one slice through the workspace on pp256.
    Preferred: the cheapest factor pp256 accepts that deals at least `min_items` work items.  ks = 1 is a candidate too: a launch
    with enough tiles of its own (the 8-expert weight gradients) writes ONE slice and the reduction adds it to the accumulator -- 3
    passes over the output instead of the 2 slices + 4 passes of the smallest split.  Otherwise (ragged contraction, tiny outputs)
    the round-1 rule: ~3 workgroups of 128 x 128 per CU (`target_blocks`), >= 512 k per split."""
    out_elems = out_rows * out_cols * batch
    ws_cap = max(1, ws_floats // out_elems)
    t256 = tiles(out_rows, out_cols) * batch
    if short_k_accum and contraction <= SHORT_K and t256 >= SHORT_K_MIN_TILES:
        return 1             # (the adaLN weight gradients: 256 tokens into 6144 x 1024) one read + one write instead of slices + a pass
    if contraction % K_UNIT == 0 and out_cols % 8 == 0:
        units = contraction // K_UNIT
        best, best_cost = None, None
        for ks in range(1, min(MAX_SPLITS, ws_cap, units) + 1):
            if units % ks or t256 * ks < min_items:
                continue
            cost = pp256_cost_us(t256, ks, contraction // ks, out_elems)
            if best_cost is None or cost < best_cost:
                best, best_cost = ks, cost
        if best is not None:
            return best if best > 1 else -1
    ks = max(1, target_blocks // (tiles(out_rows, out_cols, 128) * batch))
    ks = min(ks, max(1, contraction // TILE128_MIN_K))
    return max(1, min(ks, ws_cap))


class WgradPlan(NamedTuple):
    ks: int              # split factor over the tokens
    span: int            # fp32 elements of one slice: it mirrors the gradient tensors' layout, gaps included
    offsets: tuple       # per problem: elements from the slice's start
    runs: tuple          # (offset, elements) of every contiguous run of tensors: one flat reduction each


def plan_wgrad_group(problems, tokens, ws_floats):
    """One grouped pp256 launch for weight gradients that contract over the same `tokens` (a multiple of 128).  problems: (byte
    address of the fp32 output, rows, cols) in address order.  Their tiles share the 256 workgroups, so the split only has to fill
    what ALL of them leave empty.  None: run them one by one (a single problem, or a slice does not fit the workspace)."""
    if len(problems) < 2:
        return None
    base = problems[0][0]
    span = (max(out + 4 * m * n for out, m, n in problems) - base) // 4
    units = tokens // K_UNIT
    t256 = sum(tiles(m, n) for _, m, n in problems)
    out_elems = sum(m * n for _, m, n in problems)
    best, best_cost = None, None
    for ks in range(1, min(MAX_SPLITS, ws_floats // span, units) + 1):
        if units % ks:
            continue
        cost = pp256_cost_us(t256, ks, tokens // ks, out_elems)
        if t256 * ks < PP256_MIN_ITEMS:
            cost *= float(PP256_MIN_ITEMS) / (t256 * ks)      # an under-filled chip: the round costs the same with fewer tiles done
        if best_cost is None or cost < best_cost:
            best, best_cost = ks, cost
    if best is None:
        return None
    runs, lo, hi = [], base, base
    for out, m, n in problems:
        if out != hi:                        # a gap (a tensor that is not in the group): the run ends
            runs.append(((lo - base) // 4, (hi - lo) // 4))
            lo = out
        hi = out + 4 * m * n
    runs.append(((lo - base) // 4, (hi - lo) // 4))
    return WgradPlan(best, span, tuple((out - base) // 4 for out, _, _ in problems), tuple(runs))


def plan_dycond(G, Mc, d, K, ws_floats):
    """out[Mc, d] += sum over G layers of a [Mc, K] x [K, d] product as one launch over operand lists: (ks, segments per split) --
    split only as far as whole rounds of the CUs need it.  None: layer by layer (not a shape of pp256, or no room for one slice)."""
    if K % K_UNIT or d % 8 or Mc * d > ws_floats:
        return None
    t256 = tiles(Mc, d)
    best, best_cost = 1, None
    for ks in range(1, G + 1):
        if G % ks or ks * Mc * d > ws_floats:
            continue
        cost = pp256_cost_us(t256, ks, (G // ks) * K, Mc * d)
        if best_cost is None or cost < best_cost:
            best, best_cost = ks, cost
    return best, G // best


def plan_adaln_dgrad(G, B, N, D, ws_floats):
    """dgc[B, D] += sum over G layers of dmod_l[B, N] W_l[N, D] as one launch: every (layer, k-part) is a work item with a slice of
    its own.  (parts per layer, contraction per part, ks = G * parts): the fewest parts that fill the chip.  None: layer by layer."""
    t256 = tiles(B, D)
    parts = 1
    for c in (1, 2, 3, 4, 6, 8, 12):
        if N % c == 0 and (N // c) % K_UNIT == 0 and (N // c) >= K_UNIT:
            parts = c
            if t256 * G * c >= PP256_MIN_ITEMS:
                break
    kspan, ks = N // parts, G * parts
    if ks * B * D > ws_floats or kspan % K_UNIT:
        return None
    return parts, kspan, ks
