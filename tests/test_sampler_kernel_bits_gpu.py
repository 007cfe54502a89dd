"""The sampler's elementwise kernels return the bits recorded in tests/golden/sampler_kernel_bits.json (tests/sampler_bits.py says what
the cases are and why a digest is a fair check), and the twelve update entry points refuse a time that is not positive."""
import json
import os

import pytest
import torch

from tests import sampler_bits as sb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_kernel_bits.json")


def _st():
    return torch.cuda.current_stream().cuda_stream


def test_every_case_returns_the_recorded_bits(hip):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = sb.compute(hip.lib(), _st())
    assert sorted(got) == sorted(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))      # no case lost, none unrecorded
    differ = [cid for cid in got if got[cid] != want[cid]]
    assert not differ, f"{len(differ)} of {len(got)} cases differ from the recorded bits; first: {differ[:8]}"


def test_update_entry_points_refuse_a_time_that_is_not_positive(hip):
    """NaN and zero t_in: the bad-argument code from all twelve forms, nothing launched, the outputs as they were."""
    L, inp = hip.lib(), sb.Inputs(sb.SHAPES[0])
    state, x_next = inp.state0.clone(), inp.fresh()
    for step in sb.STEPS:
        for source in sb.SOURCES:
            for layout in sb.LAYOUTS:
                for t_in in (float("nan"), 0.0):
                    code = sb.launch_update(L, inp, step, source, layout, state, x_next, _st(), t_in=t_in)
                    assert code == sb.BAD_ARG, (sb.entry_name(step, source, layout), t_in, code)
    torch.cuda.synchronize()
    assert torch.equal(state, inp.state0) and bool((x_next == sb.SENTINEL).all())
