"""Training health (per-tensor optimizer monitor + device-side non-finite step guard), the parts that need no GPU: the C ABI
surface, the host-side work-item builder of md_tensor_stats_partial and the compiled resources of the new kernels."""
import os
import re

import pytest

from micro_diffusion_amd import hip, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NEW = ["md_tensor_stats_partial", "md_tensor_stats_finish", "md_step_guard", "md_adamw_step_guarded", "md_adamw_step_ranges_guarded"]
NUMELS = [16, 1, 77, 65536, 3 * 65536 + 40, 1152 * 4608]


def synthetic_layout(numels=NUMELS, align=64):
    """Offsets of tensors padded to `align` elements, as dit.flat_layout pads them."""
    offs, total = [], 0
    for n in numels:
        offs.append(total)
        total += (n + align - 1) // align * align
    return offs, total


def test_header_binding_and_abi():
    with open(os.path.join(ROOT, "include", "microdit_hip.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"^int (md_\w+)\(", header, flags=re.M))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/microdit_hip.h"
        assert name in hip.exported_symbols(), f"{name} is not bound in hip._SIGS"
    assert "#define MD_ABI_VERSION 6" in header and hip.ABI_VERSION == 6
    assert "#define MD_STATS_ITEM_MAX 65536" in header and hip.STATS_ITEM_MAX == 65536
    import ctypes
    assert ctypes.sizeof(hip.StatsItem) == 16 and hip.StatsItem.count.offset == 8 and hip.StatsItem.tensor.offset == 12


def _covered(items, numels):
    """{tensor: sorted [(source offset, count)]} with the per-item invariants checked."""
    per = {t: [] for t in range(len(numels))}
    for so, c, t in items:
        assert 1 <= c <= hip.STATS_ITEM_MAX and so % 8 == 0, (so, c, t)
        per[t].append((so, c))
    return per


def test_stats_items_tile_every_tensor_of_the_whole_buffer():
    from micro_diffusion_amd.trainer import stats_items
    offs, total = synthetic_layout()
    items, begin = stats_items(offs, NUMELS, [(0, total, 0)])
    assert [t for _, _, t in items] == sorted(t for _, _, t in items), "items must be sorted by tensor"
    assert len(begin) == len(NUMELS) + 1 and begin[0] == 0 and begin[-1] == len(items)
    per = _covered(items, NUMELS)
    for t, n in enumerate(NUMELS):
        assert [x[2] for x in items[begin[t]:begin[t + 1]]] == [t] * (begin[t + 1] - begin[t])
        pos = offs[t]
        for so, c in per[t]:                               # in order, back to back, starting at the tensor: no gap, no overlap
            assert so == pos
            pos += c
        assert pos == offs[t] + n, f"tensor {t}: items cover {pos - offs[t]} of {n} elements"
    assert begin[5] - begin[4] == 4 and begin[6] - begin[5] == 81     # 3 * 65536 + 40 -> 4 items, 1152 * 4608 -> 81 items
    small, _ = stats_items(offs, NUMELS, [(0, total, 0)], item_max=24)
    assert max(c for _, c, _ in small) == 24 and sum(c for _, c, _ in small) == sum(NUMELS)
    with pytest.raises(ValueError):
        stats_items(offs, NUMELS, [(0, total, 4)])         # a source offset that breaks the 16-byte alignment


@pytest.mark.parametrize("world", [1, 2, 4, 8, 16])
def test_stats_items_of_the_ranks_cover_the_tiny_table_once(world):
    """The sharded exchange: rank r holds chunk r of every matrix-shaped bucket packed back to back, every rank the small region.
    Mapped back to flat indices, the ranks' items are disjoint and, with the small-region items, cover every element of every
    tensor of the real Tiny layout exactly once."""
    import numpy as np
    from oracle import microdit_ref as orc
    from micro_diffusion_amd.dit import DiT, bucket_ranges, flat_layout
    from micro_diffusion_amd.trainer import shard_plan, stats_items
    table = DiT(**orc.tiny_config().__dict__)._table
    offs_by_name, total = flat_layout(table)
    specs = sorted((s for s in table if not s.buffer), key=lambda s: offs_by_name[s.name])
    offs, numels = [offs_by_name[s.name] for s in specs], [int(np.prod(s.shape)) for s in specs]
    plan, small, own = shard_plan(bucket_ranges(table, offs_by_name, total), world)
    seen = np.zeros(total, dtype=np.int32)
    for rank in range(world):
        present = [(lo + rank * chunk, chunk, olo) for _, lo, hi, chunk, olo in plan]
        items, begin = stats_items(offs, numels, present)
        assert begin[-1] == len(items)
        _covered(items, numels)
        for so, c, t in items:
            assert so + c <= own
            j = max(i for i, (_, _, olo) in enumerate(present) if olo <= so)      # packed offset -> flat index
            flo, cnt, olo = present[j]
            assert so + c <= olo + cnt, "an item must not straddle two chunks"
            a = flo + (so - olo)
            assert offs[t] <= a and a + c <= offs[t] + numels[t], "an item must lie inside its tensor"
            seen[a:a + c] += 1
    items, _ = stats_items(offs, numels, [(small[0], small[1] - small[0], small[0])])
    for so, c, t in items:
        assert offs[t] <= so and so + c <= offs[t] + numels[t]
        seen[so:so + c] += 1
    want = np.zeros(total, dtype=np.int32)
    for o, n in zip(offs, numels):
        want[o:o + n] = 1
    assert np.array_equal(seen, want), "every element of every tensor exactly once, padding never"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_new_kernels_have_no_spills_no_scratch_and_adamw_keeps_its_occupancy(tmp_path):
    res = native.resource_usage("stats.hip", hip.HIPCC_FLAGS, tmp_path / "stats.o")
    assert any("stats_partial_kernelILb0E" in k for k in res) and any("stats_partial_kernelILb1E" in k for k in res)
    assert any("stats_finish_kernel" in k for k in res)
    opt = native.resource_usage("optim.hip", hip.HIPCC_FLAGS, tmp_path / "optim.o")
    assert any("step_guard_kernel" in k for k in opt)
    for name, v in {**res, **opt}.items():
        assert v["spill"] == 0 and v["scratch"] == 0, (name, v)
    hits = [k for k in opt if "adamw_kernel" in k]
    assert len(hits) >= 9, hits
    for k in hits:
        assert opt[k]["occ"] >= 8, f"{k}: {opt[k]['vgprs']} VGPRs -> {opt[k]['occ']} waves / SIMD"
