"""The optimiser tail makes the launches it made before it was gathered into hip.adamw_step / hip.grad_sumsq and optim.py.

tests/optim_launch_table.json was recorded at the commit before optim.py existed (`python tests/test_optim_launches_cpu.py --record`;
it runs against any commit that has the optimisers).  The harness: a fake DiT with the real flat layout of the tiny configuration on
CPU tensors, `hip._lib` replaced by a recorder that returns 0 and notes the symbol and every argument, torch.cuda.current_stream
stubbed.  Arguments are canonical: a byref struct field by field, a ctypes array as a list, an address as [buffer name, byte
offset], a float as the bits of the c_float / c_double the library receives (so the bias corrections 1 - b ** step are compared
exactly).  Every case records two consecutive steps.  The table keeps per case the symbols in order and one SHA-256 over the
canonical entries; `--record FULL.json` also writes every entry, so two such files from two commits name the call that differs.

Cases: FusedAdamW.step over clip x guard x EMA state x post-hoc profiles x gradient source; FusedAdamW.step_sharded at world 4 rank 1
(guarded and not, chunk_of=8, and a plan of more buckets than the range table holds); LoRAAdamW.step projected and factored;
LossWeighting.step.  Muon steps on the GPU only: scripts/engine_fingerprint.py --cases step covers it.

Also here: hip.adamw_step picks each of the four entry points and fills AdamWArgs by name; GradSync.last_microbatch disarms the
engine when its body raises."""
import ctypes
import hashlib
import itertools
import json
import os
import struct
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micro_diffusion_amd import hip                                                 # noqa: E402
from micro_diffusion_amd.arch import DiTConfig, param_table                         # noqa: E402
from micro_diffusion_amd.dit import bucket_ranges, flat_layout                      # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "optim_launch_table.json")
_BYREF = type(ctypes.byref(ctypes.c_int()))
ADDRESS = 1 << 32                 # an integer argument at or above this is an address of one of the named buffers


# ------------------------------------------------------------------------------------------------ the harness
class FakeDiT:
    """CPU flat buffers with the layout of the tiny configuration: what the optimisers read of a DiT."""

    def __init__(self):
        import numpy as np
        from oracle import microdit_ref as orc
        self._table = param_table(DiTConfig(**orc.tiny_config().__dict__))
        offs, total = flat_layout(self._table)
        p, g, s = torch.zeros(total), torch.zeros(total), torch.zeros(total, dtype=torch.bfloat16)
        P = {sp.name: p[offs[sp.name]:offs[sp.name] + int(np.prod(sp.shape))].view(sp.shape) for sp in self._table if not sp.buffer}
        self._flat = {"p": p, "g": g, "s": s, "offs": offs, "total": total, "P": P, "buckets": bucket_ranges(self._table, offs, total)}
        self._lora = None
        self.fresh = 0

    def flat_buffers(self):
        return self._flat

    def mark_shadow_fresh(self):
        self.fresh += 1


class Recorder:
    """Stands in for hip._lib: every call returns 0 and lands in `log` in canonical form.  `named()` -> {name: tensor}: the buffers
    an address may point into."""

    def __init__(self, named):
        self.named, self.log = named, []

    def where(self, v):
        if v is None or v < ADDRESS:
            return v
        for name, t in self.named().items():
            if t is not None and t.data_ptr() <= v < t.data_ptr() + max(t.numel() * t.element_size(), 1):
                return [name, v - t.data_ptr()]
        raise AssertionError(f"address {v:#x} is in none of the named buffers")

    def canon(self, typ, v):
        if isinstance(v, _BYREF):
            v = v._obj
            if not isinstance(v, ctypes.Structure):
                return "out"
            return {name: self.canon(ft, getattr(v, name)) for name, ft in v._fields_}
        if isinstance(v, ctypes.Array):
            et = v._type_
            if issubclass(et, ctypes.Structure):
                return [[self.canon(ft, getattr(e, name)) for name, ft in et._fields_] for e in v]
            return [self.canon(et, e) for e in v]
        if typ is ctypes.c_float:
            return struct.pack("<f", v).hex()
        if typ is ctypes.c_double:
            return struct.pack("<d", v).hex()
        if typ is ctypes.c_void_p:
            return self.where(v)
        assert v is None or isinstance(v, int), (typ, v)
        return v

    def __getattr__(self, name):
        argtypes = hip._SIGS[name][1]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            self.log.append([name] + [self.canon(t, a) for t, a in zip(argtypes, args)])
            return 0
        return call


class _Stream:
    cuda_stream = 0


@pytest.fixture
def recording(monkeypatch):
    """record(named) -> Recorder installed as hip._lib for the rest of the test."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream())

    def install(named):
        rec = Recorder(named)
        monkeypatch.setattr(hip, "_lib", rec)
        return rec
    return install


def _opt_buffers(dit, opt, extra=None):
    def named():
        f = dit.flat_buffers()
        d = {"p": f["p"], "g": f["g"], "s": f["s"], "m": opt.m, "v": opt.v, "ema": getattr(opt, "ema", None), "sumsq": opt.sumsq,
             "partials": opt.partials, "guard": opt.guard_state}
        d.update({f"posthoc{i}": e for i, e in enumerate(getattr(opt, "posthoc", ()) or ())})
        d.update(extra() if callable(extra) else (extra or {}))
        return d
    return named


# ------------------------------------------------------------------------------------------------ the cases
EMA_STATES = ("none", "before_start", "first", "live")
STEP_AXES = list(itertools.product((0.0, 0.25), (False, True), EMA_STATES, (0, 2), ("fp32", "bf16_partials")))
STEP_EXTRA = [(0.25, False, "none", 0, "bf16"), (0.0, True, "first", 2, "bf16"), (None, False, "live", 0, "fp32")]


def _fused(dit, guard, ema, posthoc):
    from micro_diffusion_amd.trainer import FusedAdamW
    kw = {} if ema == "none" else {"ema_smoothing": 0.99975, "ema_start": 10 if ema == "before_start" else 0}
    opt = FusedAdamW(dit, lr=2.4e-4, skip_nonfinite=guard, posthoc_sigma_rels=(0.05, 0.1) if posthoc else None, **kw)
    if ema == "live":
        opt.ema_live = True
    return opt


def run_step(install, clip, guard, ema, posthoc, grad):
    dit = FakeDiT()
    opt = _fused(dit, guard, ema, posthoc)
    gbf = torch.zeros(dit._flat["total"], dtype=torch.bfloat16)
    rec = install(_opt_buffers(dit, opt, {"gbf": gbf}))
    for i in range(2):
        kw = {"lr": 2.4e-4 * (0.5 + 0.25 * i), "grad_scale": 0.25} if clip is not None else {}      # clip None: every default
        if grad != "fp32":
            kw.update(g_bf16=gbf, norm_partials=3 * hip.SUMSQ_PARTIALS if grad == "bf16_partials" else 0)
        opt.step(max_norm=clip, **kw) if clip is not None else opt.step(**kw)
    assert dit.fresh == 2 and opt.step_count == 2
    return rec.log


def _fake_sync(dit, world, rank, plan=None):
    """What step_sharded reads of a GradSync, on CPU buffers; finish_sharded_norm is GradSync's own, gather_shadows a marker."""
    from micro_diffusion_amd.trainer import GradSync, shard_plan
    p, small, own = shard_plan(dit._flat["buckets"], world)
    if plan is not None:
        p, own = plan, sum(r[3] for r in plan)
    total = dit._flat["total"]
    ns = types.SimpleNamespace(rank=rank, world=world, plan=p, small=small, gbf=torch.zeros(total, dtype=torch.bfloat16),
                               gred=torch.zeros(max(own, 8), dtype=torch.bfloat16), ssend=torch.zeros(max(own, 8), dtype=torch.bfloat16),
                               fin=torch.zeros(hip.SUMSQ_PARTIALS + 8), norm_partials=None, log=None)
    ns._all_reduce = lambda buf: None
    ns.all_reduce_now = lambda buf: None
    ns.finish_sharded_norm = types.MethodType(GradSync.finish_sharded_norm, ns)
    ns.gather_shadows = lambda: ns.log.append(["gather_shadows"])
    return ns


def many_buckets_plan(dit, world, n=70, chunk=64):
    """More matrix-shaped buckets than the kernel's range table holds: the first bucket cut into `n` of world * chunk elements."""
    key, lo, hi = next(b for b in dit._flat["buckets"] if b[0] != "small")
    assert hi - lo >= n * world * chunk
    return [(f"{key}.{i}", lo + i * world * chunk, lo + (i + 1) * world * chunk, chunk, i * chunk) for i in range(n)]


def run_sharded(install, guard, chunk_of=None, many=False, clip=0.25, posthoc=2, ema="first"):
    dit = FakeDiT()
    opt = _fused(dit, guard, ema, posthoc)
    sync = _fake_sync(dit, 4, 1, many_buckets_plan(dit, 4) if many else None)
    sync.norm_partials = opt.partials
    rec = install(_opt_buffers(dit, opt, {"gbf": sync.gbf, "gred": sync.gred, "ssend": sync.ssend, "fin": sync.fin}))
    sync.log = rec.log
    for i in range(2):
        opt.step_sharded(sync, lr=1e-4 * (i + 1), max_norm=clip, grad_scale=0.25, norm_slots=5, chunk_of=chunk_of)
    assert dit.fresh == 2
    return rec.log


def run_lora(install, backward, guard, clip):
    from micro_diffusion_amd import lora
    dit = FakeDiT()
    ad = lora.LoRA(dit, rank=4, device="cpu", backward=backward)
    ad.attached, dit._lora = True, ad                    # attach() needs a GPU (it merges into the shadow): only its bookkeeping here
    opt = lora.LoRAAdamW(ad, lr=1e-4, weight_decay=0.01, skip_nonfinite=guard)
    extra = lambda: {"lora_w": ad.w, "lora_g": ad.g, "lora_items": ad._items_dev, "lora_ws": ad._ws}
    rec = install(_opt_buffers(dit, opt, extra))
    for i in range(2):
        opt.step(lr=1e-4 * (i + 1), max_norm=clip, grad_scale=0.5)
    assert dit.fresh == 2
    return rec.log


def run_loss_weighting(install, guard):
    from micro_diffusion_amd.loss_weighting import LossWeighting
    lw = LossWeighting(channels=64, device="cpu")
    gs = torch.zeros(4, dtype=torch.int32) if guard else None
    rec = install(lambda: {"w": lw.w, "g": lw.g, "m": lw.m, "v": lw.v, "guard": gs})
    for i in range(2):
        lw.step(3e-4 * (i + 1), grad_scale=0.125, guard_state=gs)
    return rec.log


def cases():
    """name -> a function of the recording fixture that returns the log."""
    out = {}
    for clip, guard, ema, ph, grad in STEP_AXES + STEP_EXTRA:
        name = f"step/clip={clip}/guard={int(guard)}/ema={ema}/posthoc={ph}/grad={grad}"
        out[name] = lambda ins, a=(clip, guard, ema, ph, grad): run_step(ins, *a)
    for guard in (False, True):
        out[f"sharded/guard={int(guard)}"] = lambda ins, g=guard: run_sharded(ins, g)
        out[f"sharded/guard={int(guard)}/many_buckets"] = lambda ins, g=guard: run_sharded(ins, g, many=True)
        out[f"loss_weighting/guard={int(guard)}"] = lambda ins, g=guard: run_loss_weighting(ins, g)
        for backward, clip in itertools.product(("projected", "factored"), (0.0, 0.5)):
            out[f"lora/{backward}/guard={int(guard)}/clip={clip}"] = lambda ins, a=(backward, guard, clip): run_lora(ins, *a)
    out["sharded/chunk_of=8"] = lambda ins: run_sharded(ins, True, chunk_of=8)
    out["sharded/plain"] = lambda ins: run_sharded(ins, False, clip=0.0, posthoc=0, ema="none")
    return out


# ------------------------------------------------------------------------------------------------ record
def digest(log):
    """What the table keeps of one case: the symbols in order (runs as name*n) and ONE SHA-256 over the canonical entries."""
    runs = []
    for e in log:
        if runs and runs[-1][0] == e[0]:
            runs[-1][1] += 1
        else:
            runs.append([e[0], 1])
    lines = "\n".join(json.dumps(e, separators=(",", ":")) for e in log)
    return {"symbols": " ".join(n if c == 1 else f"{n}*{c}" for n, c in runs), "sha256": hashlib.sha256(lines.encode()).hexdigest()}


def record(full_path=None):
    """Write the table; `full_path`: also every entry of every case (two such files from two commits name the call that differs)."""
    mp = pytest.MonkeyPatch()
    mp.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream())

    def install(named):
        rec = Recorder(named)
        mp.setattr(hip, "_lib", rec)
        return rec
    try:
        logs = {name: fn(install) for name, fn in cases().items()}
    finally:
        mp.undo()
    with open(TABLE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(digest(log))}" for n, log in logs.items()) + "\n}\n")
    if full_path:
        with open(full_path, "w") as f:
            json.dump(logs, f, indent=0)
    print(f"{TABLE}: {len(logs)} cases, {sum(map(len, logs.values()))} calls, {os.path.getsize(TABLE)} bytes")


# ------------------------------------------------------------------------------------------------ tests
def _table():
    with open(TABLE) as f:
        return json.load(f)


def test_table_and_harness_hold_every_entry_point_and_case(recording):
    """A table that lost its hard rows, or a harness that no longer reaches them, cannot pass quietly."""
    tab = _table()
    assert sorted(tab) == sorted(cases())
    seen = {r.split("*")[0] for c in tab.values() for r in c["symbols"].split()}
    assert {"md_sumsq", "md_sumsq_finish", "md_step_guard", "md_adamw_step", "md_adamw_step_guarded", "md_adamw_step_ranges",
            "md_adamw_step_ranges_guarded", "md_ema_power_update", "md_ema_power_update_ranges", "md_lora_grad", "md_lora_merge",
            "md_fill_zero"} <= seen
    assert "md_adamw_step_guarded*71" in tab["sharded/guard=1/many_buckets"]["symbols"], "one launch per chunk and one for the small region"
    # what the hashes cover, read from the harness itself: every EMA mode, both bias corrections, the packed gradient, a step without a norm
    logs = [cases()[n](recording) for n in ("step/clip=0.0/guard=0/ema=first/posthoc=0/grad=fp32", "sharded/guard=0")]
    args = [c[1] for log in logs for c in log if c[0].startswith("md_adamw_step")]
    assert {a["ema_mode"] for a in args} == {1, 2} and {a["zero_grad"] for a in args} == {0, 1}
    assert len({a["bias_corr1"] for a in args}) == 2, "two consecutive steps: two bias corrections"
    assert any(a["g_bf16"] is not None and a["g_bf16"][0] == "gred" for a in args) and any(a["sumsq"] is None for a in args)


@pytest.mark.parametrize("prefix", ["step/clip=0.0", "step/clip=0.25", "step/clip=None", "sharded", "lora", "loss_weighting"])
def test_head_reproduces_every_recorded_launch(recording, prefix):
    tab = _table()
    todo = {n: fn for n, fn in cases().items() if n.startswith(prefix)}
    assert todo
    for name, fn in todo.items():
        log = fn(recording)
        got = digest(log)
        assert got["symbols"] == tab[name]["symbols"], f"{name}: other launches\n  recorded: {tab[name]['symbols']}\n  head:     {got['symbols']}"
        assert got["sha256"] == tab[name]["sha256"], f"{name}: the same symbols with other arguments; the head's calls:\n" + "\n".join(map(json.dumps, log[:12]))


def _fields(a):
    return {name: getattr(a, name) for name, _ in a._fields_}


@pytest.mark.parametrize("guard,ranges,symbol", [(False, False, "md_adamw_step"), (True, False, "md_adamw_step_guarded"),
                                                 (False, True, "md_adamw_step_ranges"), (True, True, "md_adamw_step_ranges_guarded")])
def test_adamw_step_picks_the_entry_point_and_fills_every_field_by_name(monkeypatch, guard, ranges, symbol):
    made = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: made.append((name, a)) or 0
    monkeypatch.setattr(hip, "_lib", Lib())
    t = {k: torch.zeros(16) for k in ("w", "g", "m", "v", "ema", "sumsq")}
    t.update(shadow=torch.zeros(16, dtype=torch.bfloat16), gbf=torch.zeros(16, dtype=torch.bfloat16), guard=torch.zeros(4, dtype=torch.int32))
    off, cnt = (ctypes.c_int64 * 2)(0, 8), (ctypes.c_int64 * 2)(8, 8)
    hip.adamw_step(t["w"], t["g"].data_ptr() + 4, t["m"], t["v"], 12, lr=3e-4, betas=(0.9, 0.95), eps=1e-6, weight_decay=0.1, step=3,
                   shadow=t["shadow"], sumsq=t["sumsq"], g_bf16=t["gbf"], ema=t["ema"], ema_smoothing=0.999, max_norm=0.5, grad_scale=0.25,
                   zero_grad=0, ema_mode=2, guard=t["guard"] if guard else None, ranges=(off, cnt) if ranges else None, stream=77)
    (name, args), = made
    assert name == symbol
    want = hip.AdamWArgs(p=t["w"].data_ptr(), g=t["g"].data_ptr() + 4, m=t["m"].data_ptr(), v=t["v"].data_ptr(), shadow=t["shadow"].data_ptr(),
                         sumsq=t["sumsq"].data_ptr(), g_bf16=t["gbf"].data_ptr(), ema=t["ema"].data_ptr(), n=12, lr=3e-4, beta1=0.9, beta2=0.95,
                         eps=1e-6, weight_decay=0.1, bias_corr1=1 - 0.9 ** 3, bias_corr2=1 - 0.95 ** 3, max_norm=0.5, grad_scale=0.25,
                         ema_smoothing=0.999, zero_grad=0, ema_mode=2)
    assert _fields(args[0]._obj) == _fields(want)
    rest = list(args[1:])
    assert rest == ([off, cnt, 2] if ranges else []) + ([t["guard"].data_ptr()] if guard else []) + [77]
    made.clear()                                         # the defaults: null pointers, zero_grad on, the current stream
    monkeypatch.setattr(hip, "stream_ptr", lambda: 55)
    hip.adamw_step(t["w"], t["g"], t["m"], t["v"], 16, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)
    (name, (a, st)), = made
    want = hip.AdamWArgs(p=t["w"].data_ptr(), g=t["g"].data_ptr(), m=t["m"].data_ptr(), v=t["v"].data_ptr(), n=16, lr=1e-3, beta1=0.9,
                         beta2=0.999, eps=1e-8, bias_corr1=1 - 0.9 ** 1, bias_corr2=1 - 0.999 ** 1, grad_scale=1.0, zero_grad=1)
    assert (name, st) == ("md_adamw_step", 55) and _fields(a._obj) == _fields(want)


def test_grad_sumsq_runs_the_tail_in_order(monkeypatch):
    made = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: made.append((name, a)) or 0
    monkeypatch.setattr(hip, "_lib", Lib())
    part, out, src, guard = torch.zeros(hip.SUMSQ_PARTIALS), torch.zeros(1), torch.zeros(40, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.int32)
    hip.grad_sumsq(part, out, src=src, src_is_bf16=True, n=40, guard=guard, stream=9)
    assert made == [("md_sumsq", (src.data_ptr(), 1, 40, part.data_ptr(), 9)),
                    ("md_sumsq_finish", (part.data_ptr(), hip.SUMSQ_PARTIALS, out.data_ptr(), 9)),
                    ("md_step_guard", (out.data_ptr(), guard.data_ptr(), 9))]
    made.clear()
    hip.grad_sumsq(part, out, count=3 * hip.SUMSQ_PARTIALS, stream=9)
    assert made == [("md_sumsq_finish", (part.data_ptr(), 3 * hip.SUMSQ_PARTIALS, out.data_ptr(), 9))]


def test_last_microbatch_disarms_when_the_body_raises():
    """GradSync.last_microbatch: a body that raises (an OOM, the engine's "two weight gradients for one tensor") leaves the engine's
    bf16 store disarmed and the exchange inactive, and the exception propagates."""
    from micro_diffusion_amd.gradsync import GradSync
    dit = FakeDiT()
    dit.engine = types.SimpleNamespace(wgrad_bf16="stale")
    sync = GradSync(dit)
    # the sharded one-microbatch step of a GPU run, as far as begin_backward reads it
    sync.enabled, sync.mode, sync.gbf = True, "sharded", types.SimpleNamespace(is_cuda=True, data_ptr=lambda: 1 << 40)
    g = dit._flat["g"]
    with pytest.raises(RuntimeError, match="two weight gradients"):
        with sync.last_microbatch(True):
            assert sync.active is True
            armed = dit.engine.wgrad_bf16
            assert armed["g_lo"] == g.data_ptr() and armed["gbf"] == 1 << 40 and armed["written"] == {}
            armed["written"][g.data_ptr()] = 64
            raise RuntimeError("two weight gradients for one tensor")
    assert dit.engine.wgrad_bf16 is None and sync.active is False and sync.last_stored == 1
    with sync.last_microbatch(False):                    # more than one microbatch: active, nothing armed
        assert sync.active is True and dit.engine.wgrad_bf16 is None
    assert sync.active is False and sync.last_stored == 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3:
        record(*sys.argv[2:])
    else:
        sys.exit("usage: python tests/test_optim_launches_cpu.py --record [FULL.json]")
