"""The bump allocator of the engine (`engine._Arena`) against a model of live intervals, on the CPU.

The model: an allocation is a byte interval [off, off + nbytes) that is live from its `alloc` until a `release(mark)` with
mark <= off (the bump pointer drops below it).  `top` is the bump pointer, rounded up to ALIGN after every allocation; the peak
is the largest `top` a pass reached.  Every statement about the arena below is one about this model.

Measured pass: the recorded peak is the model's peak.  Served pass of the same sequence: every view has the asked shape and dtype,
its offset is a multiple of ALIGN, it lies inside `buf`, it overlaps no allocation the model says is live, and a write through one
view changes no other live view.  Keys: a second key with a larger peak re-allocates at `begin` and only there, a smaller one
does not, the buffer holds max(peaks) + ALIGN bytes, a pass ended with end(ok=False) is not recorded and measures again, and one
allocation more than measured raises the overflow error and returns nothing."""
import random

import pytest
import torch

from micro_diffusion_amd.engine import _Arena

ALIGN = _Arena.ALIGN
DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int32, torch.uint8]


def _esize(dt):
    return torch.empty((), dtype=dt).element_size()


def _up(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


class Model:
    """Live intervals of a bump allocator with mark / release."""

    def __init__(self):
        self.top = self.peak = 0
        self.live = []                  # (off, nbytes, index of the op that allocated it)

    def alloc(self, nbytes, i):
        off = self.top
        self.top = _up(off + nbytes)
        self.peak = max(self.peak, self.top)
        self.live.append((off, nbytes, i))
        return off

    def release(self, mark):
        self.top = mark
        self.live = [a for a in self.live if a[0] < mark]


def _shape(rng, dt):
    """Shapes whose byte size is zero, tiny, or one element under / at / over a multiple of ALIGN (for uint8: one BYTE)."""
    es = _esize(dt)
    kind = rng.randrange(6)
    if kind == 0:
        return rng.choice([(0,), (3, 0), (0, 7)])
    if kind == 1:
        return (rng.randrange(1, 9),)
    per = ALIGN // es
    n = rng.randrange(1, 5) * per + rng.choice([-1, 0, 1])
    if kind == 2 and n % 2 == 0:
        return (2, n // 2)
    if kind == 3 and n % 3 == 0:
        return (n // 3, 1, 3)
    return (n,)


def _sequence(seed, n_ops=60):
    """Random program of ("alloc", shape, dtype) / ("mark",) / ("release",): releases are nested (they pop the marks in turn)."""
    rng = random.Random(seed)
    ops, depth = [], 0
    for _ in range(n_ops):
        r = rng.random()
        if r < 0.15:
            ops.append(("mark",))
            depth += 1
        elif r < 0.30 and depth:
            ops.append(("release",))
            depth -= 1
        else:
            dt = rng.choice(DTYPES)
            ops.append(("alloc", _shape(rng, dt), dt))
    return ops


def _nbytes(shape, dt):
    n = 1
    for d in shape:
        n *= d
    return n * _esize(dt)


def _run(arena, ops, check=None):
    """Drive the arena and the model through `ops`; check(i, view, off, model, views) after every served allocation."""
    m, marks, views = Model(), [], {}
    for i, op in enumerate(ops):
        if op[0] == "mark":
            marks.append((arena.mark(), m.top))
            assert marks[-1][0] == marks[-1][1]
        elif op[0] == "release":
            am, mm = marks.pop()
            arena.release(am)
            m.release(mm)
        else:
            off = m.alloc(_nbytes(op[1], op[2]), i)
            v = arena.alloc(op[1], op[2])
            views[i] = v
            if check is not None:
                check(i, v, off, m, views)
        assert arena.top == m.top and arena.peak == m.peak
    return m


SEEDS = list(range(12))


@pytest.mark.parametrize("seed", SEEDS)
def test_measured_peak_is_the_models_peak(seed):
    ops = _sequence(seed)
    a = _Arena("cpu")
    a.begin("k")
    assert a.measuring and a.buf is None
    m = _run(a, ops)
    a.end()
    assert a.peaks == {"k": m.peak}
    assert a.buf is None, "the buffer is allocated at the next begin(), never at the end of the measuring pass"
    assert m.peak % ALIGN == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_served_pass_gives_disjoint_aligned_views_inside_the_buffer(seed):
    ops = _sequence(seed)
    a = _Arena("cpu")
    a.begin("k")
    m0 = _run(a, ops)
    a.end()
    a.begin("k")
    assert not a.measuring and a.buf is not None and a.buf.numel() == m0.peak + ALIGN and a.buf.dtype == torch.uint8
    base, size = a.buf.data_ptr(), a.buf.numel()
    a.buf.fill_(0xEE)
    tags = {}

    def tag_of(i, dt):
        return (i % 100) + 1            # 1 .. 100: exact in every dtype used, and never the 0xEE background byte pattern

    def check(i, v, off, m, views):
        _, shape, dt = ops[i]
        assert tuple(v.shape) == tuple(shape) and v.dtype == dt
        nb = _nbytes(shape, dt)
        assert v.numel() * v.element_size() == nb
        if nb:
            assert v.is_contiguous()
            assert v.data_ptr() - base == off, "the served offset is the model's"
            assert (v.data_ptr() - base) % ALIGN == 0
            assert 0 <= off and off + nb <= size
        for (o2, n2, j) in m.live:
            if j != i and nb and n2:
                assert off + nb <= o2 or o2 + n2 <= off, f"allocation {i} [{off}, {off + nb}) overlaps live allocation {j} [{o2}, {o2 + n2})"
        v.fill_(tag_of(i, dt))
        tags[i] = tag_of(i, dt)
        for (_, _, j) in m.live:        # a write through one view changes no other live view
            assert bool((views[j] == tags[j]).all()), f"the write through allocation {i} changed live allocation {j}"

    m1 = _run(a, ops, check)
    a.end()
    assert m1.peak == m0.peak and a.peaks == {"k": m0.peak}


def test_keys_reallocate_at_begin_and_only_for_a_larger_peak():
    a = _Arena("cpu")
    a.begin("small")
    a.alloc((1000,), torch.float32)                 # 4000 bytes -> 4096
    a.end()
    assert a.buf is None and a.peaks == {"small": 4096}
    a.begin("small")
    assert a.buf.numel() == 4096 + ALIGN
    first = a.buf
    a.alloc((1000,), torch.float32)
    a.end()
    # a second, larger key: its measuring pass leaves the buffer alone, its first served begin() re-allocates
    a.begin("large")
    assert a.measuring and a.buf is first
    a.alloc((1000,), torch.float32)
    a.alloc((3000,), torch.bfloat16)                # 6000 bytes -> top 10240
    assert a.buf is first
    a.end()
    assert a.buf is first and a.peaks == {"small": 4096, "large": 10240}
    a.begin("small")                                # the old buffer still serves the small key: no re-allocation here
    assert a.buf is first and not a.measuring
    a.end()
    a.begin("large")
    assert a.buf is not first and a.buf.numel() == max(a.peaks.values()) + ALIGN == 10240 + ALIGN
    second = a.buf
    a.alloc((1000,), torch.float32)
    a.alloc((3000,), torch.bfloat16)
    a.end()
    # a third, smaller key never re-allocates: not while measuring, not when served
    a.begin("tiny")
    a.alloc((5,), torch.float64)
    a.end()
    assert a.buf is second and a.peaks["tiny"] == 256
    a.begin("tiny")
    assert a.buf is second and not a.measuring
    v = a.alloc((5,), torch.float64)
    assert v.data_ptr() == second.data_ptr()
    a.end()
    a.begin("small")
    assert a.buf is second
    a.end()
    assert a.buf.numel() == max(a.peaks.values()) + ALIGN


def test_a_failed_pass_is_not_recorded_and_measures_again():
    a = _Arena("cpu")
    a.begin("k")
    a.alloc((1024,), torch.float32)
    a.end(ok=False)
    assert a.peaks == {} and a.buf is None
    a.begin("k")
    assert a.measuring, "the key of a failed pass measures again"
    a.alloc((1024,), torch.float32)
    a.alloc((4096,), torch.float32)
    a.end(ok=True)
    assert a.peaks == {"k": 4096 + 16384} and a.buf is None
    # a failed SERVED pass changes nothing either
    a.begin("k")
    a.alloc((1024,), torch.float32)
    a.end(ok=False)
    assert a.peaks == {"k": 4096 + 16384} and a.buf.numel() == 4096 + 16384 + ALIGN


def test_one_allocation_more_than_measured_raises_and_returns_nothing():
    a = _Arena("cpu")
    a.begin("k")
    a.alloc((100,), torch.float32)                  # 400 -> 512
    a.alloc((64,), torch.float32)                   # 256 -> 768
    a.end()
    a.begin("k")
    a.alloc((100,), torch.float32)
    a.alloc((64,), torch.float32)
    got = None
    with pytest.raises(RuntimeError, match="activation arena overflow"):
        got = a.alloc((100,), torch.float32)        # the first allocation once more: 768 + 512 > 768 + ALIGN
    assert got is None
    a.end()
    assert a.peaks == {"k": 768}, "a served pass never changes the recorded peak"
    # the buffer holds peak + ALIGN bytes, so an extra allocation of at most ALIGN bytes still lies inside it; the next one cannot
    a.begin("k")
    a.alloc((100,), torch.float32)
    a.alloc((64,), torch.float32)
    extra = a.alloc((ALIGN,), torch.uint8)
    assert extra.data_ptr() + ALIGN == a.buf.data_ptr() + a.buf.numel()
    with pytest.raises(RuntimeError, match="activation arena overflow"):
        got = a.alloc((1,), torch.uint8)
    assert got is None
    a.end()


def test_release_makes_the_region_reusable_and_keeps_what_is_below_the_mark():
    a = _Arena("cpu")
    for _ in range(2):
        a.begin("k")
        keep = a.alloc((300,), torch.uint8)         # [0, 300) -> top 512
        mk = a.mark()
        t1 = a.alloc((255,), torch.uint8)           # [512, 767) -> 768
        a.release(mk)
        t2 = a.alloc((257,), torch.uint8)           # [512, 769) -> 1024
        a.end()
    assert mk == 512 and a.peaks == {"k": 1024}
    assert t1.data_ptr() == t2.data_ptr() == a.buf.data_ptr() + 512, "a released region is handed out again"
    assert keep.data_ptr() == a.buf.data_ptr()
    keep.fill_(7)
    t2.fill_(9)
    assert bool((keep == 7).all())
