"""The layer that hands the kernels their memory: DiTEngine.empty() / zeros() / fresh(), the two bump arenas with their mark / release
discipline, and the split-K / tail workspace -- poisoned (DiTEngine.poison, MD_POISON=1) and arena-backed passes must give the bits of
the plain allocator pass.

Why a poisoned pass: with the arena every buffer of a microbatch sits at the same address in every pass, so a launch that reads a buffer
(or its padding) before anything wrote it finds what the previous, identical pass left there -- the right answer.  With the switch on,
empty() hands out NaN (floating dtypes) or 0 (integer dtypes: every integer buffer is an index table, and 0 is always inside it) and
the 512 MiB workspace is NaN at the start of every forward() and backward(): such a read now gives NaN, or another bit pattern.

Reference R0 of a case: deterministic mode, torch allocator, poison off -- the path test_engine_gpu.py and test_oracle_golden.py hold to
the oracle.  Compared with it, torch.equal on the loss and every named gradient (all finite):
  P1  allocator, poison on
  P2  arena, poison on, the served (second) pass of the key
  P3  arena, poison on, keys A, B, A, B, A (A: a batch of 4, B: a batch of 2): passes 3 and 5 against R0 of A, pass 4 (the served
      pass of B) against R0 of B; the gradient buffer is zeroed between passes
ROWS is the table of engine switches that change which buffers exist or how large they are.  Every row runs in deterministic mode (none
of the switches turned out to need the atomic split-K form the mode refuses).  The x-only backward of an input_tape cannot run from the
arena (cond= / patches= are refused with arena=True): that row runs P1 alone.

Default (atomic) mode, the three base rows: P1 and P2 finite, the flat gradient within 1e-5 of the unpoisoned allocator run
(test_arena_on_off_same_gradients_with_ragged_microbatch) and every gradient tensor within 1e-2 (test_deterministic_equals_default_mode).

Inference: edm_sampler_loop on the tiny network, poison on against off, bit-equal final latents.  Trainer: three train_steps of two
microbatches, poison on (through MD_POISON) against off: shadow checksum, masters, both moments, losses.

The comparisons are shown to bite by two host-side mutations of an engine instance (floating buffers only, every address stays inside
the arena): (1) the fp32 accumulator dgc of _backward comes from empty() instead of zeros() -> P1 reports non-finite gradients;
(2) one floating allocation inside a block's backward is handed the offset of the previous floating allocation of the same byte size
in the scratch arena (an aliased temporary) -> P2 differs from R0.

The torch.empty sites outside empty(): ResidualCache (delta, ref, _ws, _rel, _rel_max) and InputGrads (dx, dt, dy) in engine.py and
the loss glue of model.py (xn, sigma, cin, cnoise, x0, lps, loss, dtok, dtb) go through ResidualCache._new / DiTEngine.fresh, which
obey the switch."""
import collections

import pytest
import torch

from oracle import microdit_ref as orc
from tests.test_deterministic_gpu import _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ the table
def _sw(**attrs):
    def setup(m):
        for k, v in attrs.items():
            assert hasattr(m.dit.engine, k), k
            setattr(m.dit.engine, k, v)
    return setup


def _arm_disperse(m):
    from micro_diffusion_amd import disperse as dsp
    m.disperse = dsp.DisperseLoss(weight=0.5, tau=0.5, block=0)
    m.disperse_accum = torch.zeros(2, device=DEV)


def _arm_loss_weighting(m):
    from micro_diffusion_amd import loss_weighting as lwm
    lw = lwm.LossWeighting(channels=128, seed=3, device=DEV)
    g = torch.Generator().manual_seed(5)
    lw.w.copy_((0.05 * torch.randn(128, generator=g)).to(DEV))        # (w = 0 would make every weight exactly 1)
    m.loss_weighting = lw


# kind: "train" = LatentDiffusion.train_microbatch; otherwise (input_grads, param_grads, input_tape) of a direct
# DiTEngine.forward(record_tape=True) + backward under a fixed cotangent
Row = collections.namedtuple("Row", "id cfgf ratio cap setup kind")
TRAIN = "train"
ROWS = [
    Row("tiny_mask0", orc.tiny_config, 0.0, 77, _sw(), TRAIN),
    Row("tiny_mask50", orc.tiny_config, 0.5, 77, _sw(), TRAIN),
    Row("tiny_mask75", orc.tiny_config, 0.75, 77, _sw(), TRAIN),
    Row("micro_mask50_cap20", orc.micro_config, 0.5, 20, _sw(), TRAIN),
    Row("prune_off", orc.tiny_config, 0.75, 77, _sw(prune_masked_experts=False), TRAIN),
    Row("qk_head_major", orc.tiny_config, 0.75, 77, _sw(qk_head_major=True), TRAIN),
    Row("grouped_off", orc.tiny_config, 0.75, 77, _sw(group_wgrad=False, group_dycond=False, group_adaln=False), TRAIN),
    Row("batch_adaln_off", orc.tiny_config, 0.75, 77, _sw(batch_adaln=False), TRAIN),
    Row("moe_cache_dact_off", orc.tiny_config, 0.75, 77, _sw(moe_cache_dact=False), TRAIN),
    Row("gemm_tail_always", orc.tiny_config, 0.75, 77, _sw(gemm_tail_mode=2), TRAIN),
    Row("disperse_armed", orc.tiny_config, 0.75, 77, _arm_disperse, TRAIN),
    Row("loss_weighting", orc.tiny_config, 0.75, 77, _arm_loss_weighting, TRAIN),
    Row("input_grads_xty", orc.tiny_config, 0.5, 8, _sw(), (("x", "t", "y"), True, False)),
    Row("param_grads_off", orc.tiny_config, 0.5, 8, _sw(), (("y",), False, False)),
    Row("x_only", orc.tiny_config, 0.0, 8, _sw(), (("x",), False, False)),
    Row("x_only_input_tape", orc.tiny_config, 0.0, 8, _sw(), (("x",), False, True)),        # P1 alone: no arena with cond= / patches=
    Row("res512_mask75", orc.tiny512_config, 0.75, 77, _sw(), TRAIN),
]
BASE = ROWS[:3]
ARENA_ROWS = [r for r in ROWS if not (r.kind != TRAIN and r.kind[2])]
IDS = lambda rows: [r.id for r in rows]     # noqa: E731

_SD, _INPUTS, _R0 = {}, {}, {}


def _sd(row):
    if row.cfgf not in _SD:
        cfg = row.cfgf()
        _SD[row.cfgf] = (cfg, orc.dezero_state_dict(orc.synth_state_dict(cfg, 61)))     # dezero: no gradient is trivially zero
    return _SD[row.cfgf]


def _inputs(row, B):
    """The microbatch of B samples of a row (key A: B = 4, key B: B = 2; res512: 2 and 1), computed once and left unchanged."""
    key = (row.cfgf, row.cap, row.kind == TRAIN, B)
    if key not in _INPUTS:
        cfg, _ = _sd(row)
        if row.kind == TRAIN:
            batch, rnd, epsn, mnoise = orc.synth_batch(cfg, B, 100 + B, cap_len=row.cap)
            _INPUTS[key] = ({k: t.cuda() for k, t in batch.items()}, (rnd.cuda(), epsn.cuda(), mnoise.cuda()))
        else:
            g = torch.Generator().manual_seed(200 + B)
            S, p = cfg.input_size, cfg.patch_size
            T = (S // p) ** 2
            x = torch.randn(B, cfg.in_channels, S, S, generator=g)
            t = torch.rand(B, generator=g) * 3.2 - 2.0
            y = torch.randn(B, 1, row.cap, cfg.caption_channels, generator=g)
            cot = torch.randn(B * T, cfg.in_channels * p * p, generator=g)
            mnoise = torch.rand(B, T, generator=g)
            _INPUTS[key] = tuple(v.cuda() for v in (x, t, y, cot, mnoise))
    return _INPUTS[key]


def _sizes(row):
    return (2, 1) if row.cfgf is orc.tiny512_config else (4, 2)


def _new_model(row, *, det=True, poison=False, arena=False):
    cfg, sd = _sd(row)
    m = _model(cfg, sd, row.ratio)
    eng = m.dit.engine
    eng.deterministic, eng.poison, eng.use_arena = det, poison, arena
    row.setup(m)
    return m


def _pass(m, row, B):
    """One forward + backward of the row's microbatch of B samples on model m, from a zeroed gradient buffer.
    -> {name: tensor} in forward order (the loss or the network output first)."""
    dit = m.dit
    eng = dit.engine
    dit.refresh_shadow()
    dit.attach_grads()
    dit.flat_buffers()["g"].zero_()
    out = {}
    if row.kind == TRAIN:
        gb, noise = _inputs(row, B)
        if row.ratio == 0:
            noise = (noise[0], noise[1], None)
        m._noise_fn = lambda b: noise
        if m.disperse_accum is not None:
            m.disperse_accum.zero_()
        if m.loss_weighting is not None:
            m.loss_weighting.g.zero_()
        out["loss"] = m.train_microbatch(gb).detach().clone()
        if m.disperse is not None:
            out["disperse_accum"] = m.disperse_accum.clone()
        if m.loss_weighting is not None:
            out["loss_weighting.g"] = m.loss_weighting.g.clone()
    else:
        want, pgrad, input_tape = row.kind
        x, t, y, cot, mnoise = _inputs(row, B)
        if input_tape:
            cond = dit.encode_condition(y)
            tape = eng.forward(x, t, None, cond=cond, input_tape=True)
        else:
            kw = dict(mask_ratio=row.ratio, mask_noise=mnoise) if row.ratio > 0 else {}
            tape = eng.forward(x, t, y, record_tape=True, arena=eng.use_arena, **kw)
            assert tape.arena == eng.use_arena
        out["out_tok"] = tape.out_tok.clone()
        dtok = cot if tape.keep_rows is None else cot[tape.keep_rows.long()]
        res = eng.backward(tape, dtok.to(BF16).contiguous(), input_grads=want, param_grads=pgrad)
        for k in ("dx", "dt", "dy"):
            if k[1] in want:
                out[k] = getattr(res, k).clone()
    torch.cuda.synchronize()
    out.update({k: p.grad.clone() for k, p in dit.named_parameters()})
    return out


def _r0(row, B, det=True):
    key = (row.id, B, det)
    if key not in _R0:
        _R0[key] = _pass(_new_model(row, det=det), row, B)
        bad = [k for k, v in _R0[key].items() if not bool(torch.isfinite(v).all())]
        assert not bad, f"the reference run itself is not finite: {bad[:4]}"
    return _R0[key]


def _assert_bits(got, ref, what):
    """All finite, then bit-equal; reports the first offenders in forward order (as test_two_runs_are_bit_identical does)."""
    assert list(got) == list(ref)
    bad = [k for k in got if not bool(torch.isfinite(got[k]).all())]
    assert not bad, (f"{what}: {len(bad)} of {len(got)} outputs are not finite (a buffer read before it was written?), "
                     f"first (in forward order): {bad[:4]}")
    differ = [k for k in ref if not torch.equal(got[k], ref[k])]
    assert not differ, (f"{what}: {len(differ)} of {len(ref)} outputs differ from the unpoisoned allocator run, "
                        f"first (in forward order): {differ[:4]}")


def _served(eng):
    return (not eng._tape_arena.measuring and not eng._scratch_arena.measuring
            and eng._tape_arena.buf is not None and eng._scratch_arena.buf is not None)


# ------------------------------------------------------------------------------------------------ the switch itself
def test_poison_fills_what_the_engine_hands_out(hip):
    """empty() / fresh() / zeros() with the switch on: NaN for bf16 / fp16 / fp32 / fp64, 0 for integers, zeros() still zero -- from
    the allocator, from a measuring arena pass and from a served one (whose memory is pre-filled with finite garbage here); the
    workspace is NaN after a forward.  With the switch off the arena's memory comes back as it was left: nothing is launched."""
    row = ROWS[0]
    m = _new_model(row, poison=True)
    eng = m.dit.engine
    assert eng.poison is True

    def check():
        for dt in (BF16, torch.float16, F32, torch.float64):
            t = eng.empty(3, 37, dtype=dt)
            assert t.dtype == dt and t.shape == (3, 37) and bool(torch.isnan(t).all())
        i = eng.empty(129, dtype=torch.int32)
        assert i.dtype == torch.int32 and not bool(i.any())
        assert eng.empty(0, 5).shape == (0, 5)
        z = eng.zeros(5, 300)
        assert z.dtype == F32 and not bool(z.any())
        zb = eng.zeros(7, 9, dtype=BF16)
        assert zb.dtype == BF16 and not bool(zb.any())
    check()
    assert bool(torch.isnan(eng.fresh(2, 3)).all()) and not bool(eng.fresh(4, dtype=torch.int32).any())
    arena = eng._scratch_arena
    for served in (False, True):
        arena.begin("k")
        assert arena.measuring is (not served)
        if served:
            arena.buf.fill_(0x3C)
        eng._arena = arena
        try:
            check()
        finally:
            eng._arena = None
        arena.end()
    # off: the served memory is handed out untouched
    eng.poison = False
    arena.begin("k")
    arena.buf.fill_(0x3C)
    eng._arena = arena
    try:
        t = eng.empty(3, 37, dtype=F32)
        assert bool((t.view(torch.uint8) == 0x3C).all())
    finally:
        eng._arena = None
    arena.end()
    eng.poison = True
    eng.ws.zero_()
    _pass(m, row, 2)
    # the forward and the backward each filled the workspace; what remains finite is what the last backward's launches wrote
    assert bool(torch.isnan(eng.ws[-(1 << 20):]).all()), "the end of the 512 MiB workspace is beyond every tiny launch: still NaN"


def test_poison_is_off_by_default_and_follows_the_environment(hip, monkeypatch):
    monkeypatch.delenv("MD_POISON", raising=False)
    row = ROWS[2]
    cfg, sd = _sd(row)
    eng = _model(cfg, sd, row.ratio).dit.engine
    assert eng.poison is False
    monkeypatch.setenv("MD_POISON", "1")
    assert _model(cfg, sd, row.ratio).dit.engine.poison is True


# ------------------------------------------------------------------------------------------------ P1 - P3, deterministic mode
@pytest.mark.parametrize("row", ROWS, ids=IDS(ROWS))
def test_p1_allocator_poisoned(hip, row):
    B = _sizes(row)[0]
    got = _pass(_new_model(row, poison=True), row, B)
    _assert_bits(got, _r0(row, B), f"{row.id} P1")


@pytest.mark.parametrize("row", ARENA_ROWS, ids=IDS(ARENA_ROWS))
def test_p2_arena_poisoned_served_pass(hip, row):
    B = _sizes(row)[0]
    m = _new_model(row, poison=True, arena=True)
    eng = m.dit.engine
    first = _pass(m, row, B)                # the measuring pass of the key: allocator memory, poisoned
    assert eng._tape_arena.buf is None and eng._scratch_arena.buf is None
    _assert_bits(first, _r0(row, B), f"{row.id} P2, measuring pass")
    got = _pass(m, row, B)
    assert _served(eng)
    _assert_bits(got, _r0(row, B), f"{row.id} P2, served pass")


@pytest.mark.parametrize("row", ARENA_ROWS, ids=IDS(ARENA_ROWS))
def test_p3_arena_poisoned_alternating_keys(hip, row):
    A, Bk = _sizes(row)
    m = _new_model(row, poison=True, arena=True)
    eng = m.dit.engine
    for i, B in enumerate((A, Bk, A, Bk, A)):
        got = _pass(m, row, B)
        if i >= 2:
            assert _served(eng), f"pass {i + 1} must be served from the arena"
            _assert_bits(got, _r0(row, B), f"{row.id} P3, pass {i + 1} (batch {B})")
    assert len(eng._tape_arena.peaks) == 2 and len(eng._scratch_arena.peaks) == 2


# ------------------------------------------------------------------------------------------------ default (atomic) mode
@pytest.mark.parametrize("row", BASE, ids=IDS(BASE))
def test_default_mode_poisoned(hip, row):
    """What production runs: float atomics in four column reductions, so two runs differ by the order of fp32 sums.  Flat gradient
    within 1e-5, every tensor within 1e-2 of the unpoisoned allocator run; everything finite; the loss (no backward precedes it) equal.

    Measured on an MI355X (tiny_mask75, B = 4, every pass on a fresh model, against the deterministic run): 96 of 100 passes lie at
    6e-9 or 1.9e-6 of the flat gradient, whether poisoned or not (the 1.9e-6 state is one bf16 element of the condition-vector
    gradient rounding the other way: blocks.0.adaLN_modulation.1.weight 9.3e-6, t_embedder.mlp.2 1.3e-6).  4 of 100 allocator passes
    -- 1 of 40 poisoned, 3 of 40 unpoisoned, none of 20 arena passes -- land in ONE other state, the same bits each time: flat
    gradient 1.541e-3, worst tensor y_embedder.y_proj.fc1.weight 2.66e-3, only the tensors behind the pooled-caption MLP differ
    (pooled_y_emb_process.norm.weight in the single element of column 4, fc1.bias in 4 columns, then every caption-path tensor),
    all finite, the loss equal.  Captured against the deterministic run: the fp32 condition-vector gradient dgc differs by at most
    1.7e-7 (the atomics' summation order), which rounds ONE more element of its bf16 cast dc the other way ([3, 216], one bf16 ulp);
    behind pooled_y_emb_process.fc2 that moves one element of the [4, 256] data gradient by one bf16 ulp ([3, 4]), the LayerNorm
    backward turns it into 4 elements, fc1's data gradient into 66, and the caption path carries it on: rounding noise of the
    atomic mode (it never appears in deterministic mode: every pass of P1 - P3 above is bit-equal), not memory -- poison does not change its
    rate or its bits.  It is the size of the 1.2e-3 once recorded for test_arena_on_off_same_gradients_with_ragged_microbatch.
    The 1e-5 bound on the flat gradient is the one that test sets and stays; a run that meets that state fails here (about one
    pass in 25 at mask 0.75; not seen at mask 0 and 0.5), and the message names the tensors."""
    B = _sizes(row)[0]
    ref = _r0(row, B, det=False)
    runs = {"P1": _pass(_new_model(row, det=False, poison=True), row, B)}
    m = _new_model(row, det=False, poison=True, arena=True)
    _pass(m, row, B)
    runs["P2"] = _pass(m, row, B)
    assert _served(m.dit.engine)
    names = [k for k in ref if k != "loss"]
    flat_ref = torch.cat([ref[k].double().flatten() for k in names])
    for tag, got in runs.items():
        bad = [k for k in got if not bool(torch.isfinite(got[k]).all())]
        assert not bad, f"{row.id} {tag}: not finite, first (in forward order): {bad[:4]}"
        assert torch.equal(got["loss"], ref["loss"]), (tag, got["loss"], ref["loss"])
        flat = torch.cat([got[k].double().flatten() for k in names])
        rel = float((flat - flat_ref).norm() / flat_ref.norm())
        per = {k: float((got[k].double() - ref[k].double()).norm()) / (float(ref[k].double().norm()) + 1e-30) for k in names}
        worst = max(per, key=per.get)
        print(f"{row.id} {tag}: flat gradient rel {rel:.3e}, worst tensor {per[worst]:.3e} ({worst})")
        off = [f"{k} {per[k]:.2e}" for k in names if per[k] > 1e-5]
        assert rel <= 1e-5, (f"{row.id} {tag}: flat gradient differs from the unpoisoned allocator run by {rel:.3e}; "
                             f"{len(off)} of {len(names)} tensors beyond 1e-5, in forward order: {off}")
        for k in names:
            a, b = got[k].double(), ref[k].double()
            assert float((a - b).norm()) <= 1e-2 * float(b.norm()) + 1e-12, (row.id, tag, k, float((a - b).norm()), float(b.norm()))


# ------------------------------------------------------------------------------------------------ the tests bite
def test_mutation_unzeroed_accumulator_is_reported_by_p1(hip):
    """Mutation 1: the first zeros() of _backward -- dgc, the fp32 [B, D] sum of every adaLN data gradient -- is served by empty()."""
    row = ROWS[2]
    B = _sizes(row)[0]
    m = _new_model(row, poison=True)
    eng = m.dit.engine
    state = {"armed": False, "hit": None}
    inner_bwd, inner_zeros = eng._backward, eng.zeros

    def _backward(*a, **k):
        state["armed"] = True
        try:
            return inner_bwd(*a, **k)
        finally:
            state["armed"] = False

    def zeros(*shape, dtype=F32):
        if state["armed"] and state["hit"] is None:
            state["hit"] = (tuple(shape), dtype)
            return eng.empty(*shape, dtype=dtype)
        return inner_zeros(*shape, dtype=dtype)
    eng._backward, eng.zeros = _backward, zeros
    got = _pass(m, row, B)
    assert state["hit"] == ((B, eng.cfg.dim), F32), state["hit"]
    with pytest.raises(AssertionError, match="P1: .* outputs are not finite"):
        _assert_bits(got, _r0(row, B), f"{row.id} P1")
    # the same mutation without poison: what the allocator happens to return decides -- that is the gap the switch closes


def _alias_one_scratch_allocation(eng, which=0):
    """Mutation 2 on an engine instance: inside a block's backward, the `which`-th floating allocation of the served scratch arena
    that has a predecessor of the same byte size in the same block is handed that predecessor's offset (the real bump allocation
    still happens, so every other address is the unmutated one).  -> state, state["hit"] = (shape, dtype, own offset, aliased offset)."""
    arena = eng._scratch_arena
    state = {"in_block": False, "seen": {}, "n": 0, "hit": None}
    inner_block, inner_alloc = eng._block_bwd, arena.alloc

    def _block_bwd(*a, **k):
        state["in_block"], state["seen"] = True, {}
        try:
            return inner_block(*a, **k)
        finally:
            state["in_block"] = False

    def alloc(shape, dtype):
        off = arena.top
        t = inner_alloc(shape, dtype)
        if not (state["in_block"] and not arena.measuring and dtype.is_floating_point and t.numel()):
            return t
        nbytes = t.numel() * t.element_size()
        prev = state["seen"].get(nbytes)
        state["seen"][nbytes] = off
        if prev is not None and state["hit"] is None:
            if state["n"] == which:
                state["hit"] = (tuple(shape), dtype, off, prev)
                assert 0 <= prev and prev + nbytes <= arena.buf.numel()
                return arena.buf[prev:prev + nbytes].view(dtype).view(*shape)
            state["n"] += 1
        return t
    eng._block_bwd, arena.alloc = _block_bwd, alloc
    return state


def test_mutation_aliased_temporary_is_reported_by_p2(hip):
    row = ROWS[2]
    B = _sizes(row)[0]
    m = _new_model(row, poison=True, arena=True)
    eng = m.dit.engine
    _pass(m, row, B)                                    # measuring pass, unmutated
    state = _alias_one_scratch_allocation(eng)
    got = _pass(m, row, B)
    assert _served(eng) and state["hit"] is not None, "the mutation must have found an allocation to alias"
    print("aliased:", state["hit"])
    with pytest.raises(AssertionError, match="P2, served pass: .* outputs (are not finite|differ)"):
        _assert_bits(got, _r0(row, B), f"{row.id} P2, served pass")


# ------------------------------------------------------------------------------------------------ inference
@pytest.fixture(scope="module")
def sampler_net(hip):
    from micro_diffusion_amd.inverse import LinearMeasurement
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    cfg = orc.tiny_config()
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(orc.synth_state_dict(cfg, 41))
    m = LatentDiffusion(d.to(DEV), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), latent_res=cfg.input_size)
    m.eval()
    m.dit.engine.deterministic = True                   # the guided run's backward to the image: no atomic order between two runs
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(2, 4, 32, 32, generator=g).cuda()
    y = torch.randn(2, 1, 77, 1024, generator=g).cuda()
    truth = (torch.randn(2, 4, 32, 32, generator=g) * 0.5).cuda()
    mask = (torch.rand(2, 1, 16, 16, generator=g) < 0.6).cuda()
    lm = LinearMeasurement(torch.nn.functional.avg_pool2d(truth, 2), 2, mask)
    return m, lat, y, lm


def _step_cache():
    from micro_diffusion_amd.step_cache import StepCache
    return StepCache(interval=2)


SAMPLER_CASES = {
    "cfg1": lambda lm: dict(cfg=1.0, cond_cache=False),
    "cfg1_cond_cache": lambda lm: dict(cfg=1.0, cond_cache=True),
    "cfg3": lambda lm: dict(cfg=3.0, cond_cache=False),
    "cfg3_cond_cache": lambda lm: dict(cfg=3.0, cond_cache=True),
    "cfg3_step_cache": lambda lm: dict(cfg=3.0, cond_cache=True, step_cache=_step_cache()),
    "cfg3_step_cache_uncached_captions": lambda lm: dict(cfg=3.0, cond_cache=False, step_cache=_step_cache()),
    "cfg3_measurement_guided": lambda lm: dict(cfg=3.0, cond_cache=True, measurement=lm, measurement_scale=2.0),
}


@pytest.mark.parametrize("case", list(SAMPLER_CASES))
def test_sampler_poisoned_equals_plain(sampler_net, case):
    """Four sampler steps on the real tiny network, B = 2: the final latents with poison on are the bits of the run with it off."""
    m, lat, y, lm = sampler_net
    eng = m.dit.engine
    out = {}
    try:
        for poison in (False, True):
            eng.poison = poison
            out[poison] = m.edm_sampler_loop(lat, y, steps=4, **SAMPLER_CASES[case](lm))       # (a fresh StepCache per run)
            torch.cuda.synchronize()
    finally:
        eng.poison = False
    assert bool(torch.isfinite(out[False]).all()) and float(out[False].abs().max()) > 0
    assert bool(torch.isfinite(out[True]).all()), "poisoned run: the latents are not finite (a buffer read before it was written?)"
    assert torch.equal(out[True], out[False]), f"max |difference| {float((out[True] - out[False]).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------ Trainer
def test_three_trainer_steps_poisoned_equal_plain(hip, monkeypatch):
    """test_three_trainer_steps_are_bit_identical with the switch on (MD_POISON=1) in one of the two runs: arenas on, two
    microbatches per step, the optimizer tail behind them."""
    from micro_diffusion_amd.trainer import FusedAdamW, LRSchedule, Trainer
    monkeypatch.setenv("MD_DETERMINISTIC", "1")
    cfg = orc.tiny_config()
    sd = orc.dezero_state_dict(orc.synth_state_dict(cfg, 71))
    L, st = hip.lib(), hip.stream_ptr()
    ends = []
    for poison in (False, True):
        monkeypatch.setenv("MD_POISON", "1" if poison else "0")
        model = _model(cfg, sd, 0.75)
        sched = LRSchedule("cosine_with_warmup", t_warmup=10, t_max=1000, alpha_f=0.33)
        opt = FusedAdamW(model.dit, lr=2.4e-4)
        tr = Trainer(model, opt, sched, clip_norm=0.25, microbatch_size=2)
        eng = model.dit.engine
        assert eng.deterministic is True and eng.poison is poison and eng.use_arena is True
        tr.batches_seen = 3
        losses = []
        for step in range(3):
            batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 4, 170 + step)
            chunks = [(rnd[i:i + 2].cuda(), epsn[i:i + 2].cuda(), mnoise[i:i + 2].cuda()) for i in range(0, 4, 2)]
            model._noise_fn = lambda b, c=chunks: c.pop(0)
            losses.append(tr.train_step({k: t.cuda() for k, t in batch.items()}).detach().clone().reshape(()))
        assert _served(eng)
        f = model.dit.flat_buffers()
        cs = torch.zeros(2, device=DEV, dtype=torch.int64)
        hip.check(L.md_checksum_u16(f["s"].data_ptr(), f["s"].numel(), cs.data_ptr(), st), "md_checksum_u16")
        torch.cuda.synchronize()
        ends.append((cs.cpu(), f["p"].clone(), opt.m.clone(), opt.v.clone(), torch.stack(losses)))
    a, b = ends
    assert all(bool(torch.isfinite(t).all()) for t in b[1:]), "poisoned run: masters, moments or losses are not finite"
    assert torch.equal(a[4], b[4]), ("losses", a[4], b[4])
    assert torch.equal(a[0], b[0]), "bf16 shadow checksum"
    assert torch.equal(a[1], b[1]), "fp32 masters"
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), "AdamW moments"
    assert not torch.equal(a[1], _model(cfg, sd, 0.75).dit.flat_buffers()["p"]), "the steps must have moved the weights"
