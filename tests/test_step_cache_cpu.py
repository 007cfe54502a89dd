"""Step cache, the part that needs no GPU: the policy's decisions against hand-written plans, the constructor's and the
sampler's refusals, and the ABI of the three launch functions and the workspace-size function."""
import ctypes
import math
import os
import re

import pytest

from micro_diffusion_amd import samplers
from micro_diffusion_amd.step_cache import StepCache, StepCacheStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, R = True, False            # full, reused


def _run(sc, n, valid=None, distances=None):
    sc.reset(n)
    out = [sc.step(True if valid is None else valid[e], None if distances is None else distances[e]) for e in range(n)]
    assert out == sc.stats.decisions
    return out


# ------------------------------------------------------------------------------------------------ fixed schedule
@pytest.mark.parametrize("interval, warmup, tail, want", [
    (1, 1, 1, [F] * 11),
    (2, 1, 1, [F, R, F, R, F, R, F, R, F, R, F]),
    (3, 1, 1, [F, R, R, F, R, R, F, R, R, F, F]),
    (2, 2, 2, [F, F, R, F, R, F, R, F, R, F, F]),
    (3, 2, 2, [F, F, R, R, F, R, R, F, R, F, F]),
    (3, 1, 2, [F, R, R, F, R, R, F, R, R, F, F]),
    (2, 2, 1, [F, F, R, F, R, F, R, F, R, F, F]),
])
def test_fixed_interval_plans_at_eleven_evaluations(interval, warmup, tail, want):
    sc = StepCache(interval=interval, warmup=warmup, tail=tail)
    assert _run(sc, 11) == want
    s = sc.stats
    assert (s.evaluations, s.full, s.reused) == (11, want.count(F), want.count(R))
    assert s.distances == [None] * 11
    assert sc.plan(11) == s and isinstance(s, StepCacheStats)
    assert _run(sc, 11) == want, "reset() starts the same run again"


def test_a_batch_change_in_the_middle_forces_a_full_evaluation():
    valid = [True] * 11
    valid[5] = False                                # e.g. the network batch goes from 2B to B here
    sc = StepCache(interval=3)
    #                               0  1  2  3  4  5* 6  7  8  9  10
    assert _run(sc, 11, valid) == [F, R, R, F, R, F, R, R, F, R, F]
    assert sc.plan(11, valid=valid).decisions == sc.stats.decisions
    valid[6] = False                                # and back one evaluation later
    assert _run(sc, 11, valid) == [F, R, R, F, R, F, F, R, R, F, F]


def test_tail_zero_and_short_runs():
    assert _run(StepCache(interval=2, tail=0), 4) == [F, R, F, R]
    assert _run(StepCache(interval=2), 1) == [F]
    assert _run(StepCache(interval=4, warmup=3, tail=3), 5) == [F] * 5
    assert _run(StepCache(interval=2), 0) == []


# ------------------------------------------------------------------------------------------------ adaptive state machine
DIST = [None, 0.25, 0.25, 0.5, 0.125, 0.125, 0.125, 1.0, 0.0625, 0.0625, 0.0625]      # exact in binary: the sums below are exact


def test_adaptive_accumulates_until_the_threshold():
    sc = StepCache(threshold=0.5)
    # acc:                          -  .25 .5* .5* .125 .25 .375 1.375* .0625 .125 (tail)
    assert _run(sc, 11, None, DIST) == [F, R, F, F, R, R, R, F, R, R, F]
    assert sc.stats.distances == DIST
    assert (sc.stats.full, sc.stats.reused) == (5, 6)
    assert sc.plan(11, distances=DIST) == sc.stats
    sc = StepCache(threshold=0.375, warmup=2, tail=2)
    # acc:                          -  (f) .25 .75* .125 .25 .375* 1.0* .0625 (tail) (tail)
    assert _run(sc, 11, None, DIST) == [F, F, R, F, R, R, F, F, R, F, F]


def test_adaptive_threshold_zero_is_all_full_and_infinity_only_the_forced_ones():
    assert _run(StepCache(threshold=0.0), 11, None, DIST) == [F] * 11
    assert _run(StepCache(threshold=0.0), 11, None, [None] + [0.0] * 10) == [F] * 11
    assert _run(StepCache(threshold=math.inf), 11, None, DIST) == [F] + [R] * 9 + [F]
    valid = [True] * 11
    valid[4] = False
    dist = list(DIST)
    dist[4] = None                                  # the probe restarts with the batch
    assert _run(StepCache(threshold=math.inf, warmup=2), 11, valid, dist) == [F, F, R, R, F, R, R, R, R, R, F]


def test_adaptive_forced_evaluations_clear_the_accumulator_and_odd_distances_are_never_close():
    valid = [True] * 6
    valid[2] = False
    assert _run(StepCache(threshold=0.5, tail=0), 6, valid, [None, 0.25, 0.125, 0.25, 0.125, 0.125]) == [F, R, F, R, R, F]
    assert _run(StepCache(threshold=0.5, tail=0), 4, None, [None, 0.25, None, 0.25]) == [F, R, F, R], "no distance: full"
    assert _run(StepCache(threshold=math.inf, tail=0), 4, None, [None, 0.25, math.inf, 0.25]) == [F, R, F, R], "a zero reference"
    assert _run(StepCache(threshold=1e30, tail=0), 3, None, [None, math.nan, 0.0]) == [F, F, R]


# ------------------------------------------------------------------------------------------------ constructor
@pytest.mark.parametrize("kwargs", [
    dict(interval=2, threshold=0.1), dict(), dict(interval=0), dict(interval=2, warmup=0), dict(interval=2.0), dict(interval=True),
    dict(threshold=-0.1), dict(threshold=math.nan), dict(threshold="0.1"), dict(interval=2, tail=-1), dict(interval=2, warmup=1.5),
    dict(interval=2, blocks=(2, 2)), dict(interval=2, blocks=(-1, 2)), dict(interval=2, blocks=(0, 1, 2)),
])
def test_constructor_refuses(kwargs):
    with pytest.raises(ValueError):
        StepCache(**kwargs)


def test_constructor_accepts():
    assert StepCache(interval=1).adaptive is False and StepCache(threshold=0).adaptive is True
    assert StepCache(threshold=math.inf, warmup=3, tail=0, blocks=(1, 5)).blocks == (1, 5)
    with pytest.raises(ValueError):
        StepCache(interval=2).reset(-1)


# ------------------------------------------------------------------------------------------------ sampler checks
def test_check_step_cache_refuses_guide_and_measurement_guidance():
    sc = StepCache(interval=2)
    assert samplers.check_step_cache(None) is False
    assert samplers.check_step_cache(None, guide=object(), measurement=object(), guidance_loss=len) is False    # nothing to refuse
    assert samplers.check_step_cache(sc) is True
    with pytest.raises(ValueError, match="guide"):
        samplers.check_step_cache(sc, guide=object())
    with pytest.raises(ValueError, match="measurement"):
        samplers.check_step_cache(sc, measurement=object())
    with pytest.raises(ValueError, match="guidance_loss"):
        samplers.check_step_cache(sc, guidance_loss=lambda D: D.flatten(1).sum(1))
    with pytest.raises(ValueError, match="StepCache"):
        samplers.check_step_cache(2)


def test_evaluation_counts_the_loop_resets_with_match_the_schedule_helpers():
    """The fused loop counts repetitions * (2 for heun but on the last step); samplers.edit_evaluations / evaluation_sigmas say the same."""
    for sampler in samplers.SAMPLERS:
        for n, strength, resample in ((5, 1.0, 1), (6, 0.5, 1), (5, 1.0, 3), (7, 0.4, 2)):
            if resample > 1 and sampler not in samplers.RESAMPLE_SAMPLERS:
                continue
            t = samplers.edm_schedule(n)
            i0 = samplers.edit_start_index(n, strength)
            reps = samplers.edit_repetitions(t, i0, resample)
            heun = sampler == "heun"
            count = sum(r * (2 if heun and i < n - 1 else 1) for i, r in zip(range(i0, n), reps))
            assert count == samplers.edit_evaluations(sampler, n, strength, resample)
            if strength == 1.0 and resample == 1:
                assert count == len(samplers.evaluation_sigmas(sampler, t))


# ------------------------------------------------------------------------------------------------ ABI
NAMES = ("md_residual_delta", "md_step_probe", "md_step_probe_finish", "md_step_probe_ws_doubles")


def test_abi_symbols_are_declared_bound_and_exported_and_the_version_stays():
    from micro_diffusion_amd import hip
    header = open(os.path.join(ROOT, "include", "microdit_hip.h")).read()
    lib = ctypes.CDLL(hip.build(verbose=False))
    for name in NAMES:
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), f"{name} is not declared in the header"
        assert name in hip.exported_symbols() and name in hip._SIGS, f"{name} is not bound in hip._SIGS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert len(hip._SIGS["md_step_probe_finish"][1]) == 5, "md_step_probe_finish(ws, B, rel, rel_max, stream)"
    assert re.search(r"#define MD_ABI_VERSION 6\b", header) and hip.ABI_VERSION == 6 == lib.md_abi_version(), "symbols added, none changed"
    for macro, value in (("MD_STEP_DELTA_MAX_BLOCKS", hip.STEP_DELTA_MAX_BLOCKS), ("MD_STEP_PROBE_CHUNKS", hip.STEP_PROBE_CHUNKS)):
        assert re.search(r"#define " + macro + r" " + str(value) + r"\b", header), f"{macro} differs between the header and hip.py"


def test_workspace_size_and_argument_checks_run_on_the_host():
    """Nothing is launched for a bad argument, so the refusals are observable without a GPU (non-null dummy addresses are never read)."""
    from micro_diffusion_amd import hip
    lib = ctypes.CDLL(hip.build(verbose=False))
    lib.md_step_probe_ws_doubles.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    out = ctypes.c_int64(-7)
    chunks = hip.STEP_PROBE_CHUNKS
    for B, per, groups in ((3, 8 * 37, 1), (2, 8 * chunks, 1), (2, 8 * chunks + 8, 2), (64, 256 * 1024, 32)):
        assert lib.md_step_probe_ws_doubles(B, per, ctypes.byref(out)) == 0 and out.value == 2 + 2 * B * groups
    for B, per in ((0, 64), (2, 12), (2, 0), (65536, 64)):
        assert lib.md_step_probe_ws_doubles(B, per, ctypes.byref(out)) == -1
    assert lib.md_step_probe_ws_doubles(2, 64, None) == -1
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    lib.md_residual_delta.argtypes = [P, P, P, I64, P]
    a, b, c = 0x10000, 0x20000, 0x30000
    assert lib.md_residual_delta(a, b, c, 12, None) == -1, "n % 8"
    assert lib.md_residual_delta(a, b, c, 0, None) == -1
    assert lib.md_residual_delta(None, b, c, 8, None) == -1
    assert lib.md_residual_delta(a, b, a, 64, None) == -1 and lib.md_residual_delta(a, b, b, 64, None) == -1, "delta aliases an input"
    assert lib.md_residual_delta(a, b, a + 64, 64, None) == -1, "delta overlaps an input"
    assert lib.md_residual_delta(a, b, c + 2, 64, None) == -1, "alignment"
    lib.md_step_probe.argtypes = [P, P, I64, I64, P, P]
    assert lib.md_step_probe(a, a, 2, 64, c, None) == -1, "x and ref alias"
    assert lib.md_step_probe(a, b, 2, 12, c, None) == -1 and lib.md_step_probe(a, b, 0, 64, c, None) == -1
    assert lib.md_step_probe(a, b, 2, 64, None, None) == -1
    lib.md_step_probe_finish.argtypes = [P, I64, P, P, P]
    assert lib.md_step_probe_finish(None, 2, b, c, None) == -1 and lib.md_step_probe_finish(a, 0, b, c, None) == -1
