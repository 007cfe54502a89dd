"""Fingerprint of the engine's host side: WHICH launches a training microbatch makes, with which scalar arguments, and the bits they
leave behind.  A refactor of engine.py that changes nothing on the GPU gives the same file before and after.

    python scripts/engine_fingerprint.py --out full_head.json --digest-out profiles/engine_fingerprint_head.json
    python scripts/engine_fingerprint.py --compare profiles/engine_fingerprint_parent.json profiles/engine_fingerprint_head.json

Cases (deterministic mode, batch 4 -- those of tests/test_deterministic_gpu.py::test_two_runs_are_bit_identical): tiny / mask 0.75 /
caption length 77, tiny / mask 0, micro / mask 0.5 / caption length 20, each once on the torch allocator and once in the fixed-address
arenas (two microbatches: the first one measures the arena, the second runs in it); and one Trainer.train_step of a single microbatch
on a one-rank sharded bf16 exchange, so that the weight gradients take the bf16 store path (DiTEngine.wgrad_bf16).

`--cases step` (profiles/step_fingerprint_*.json) fingerprints the training step instead: three Trainer.train_steps of two microbatches
each on tiny / mask 0.75 / batch 4 under FusedAdamW (EMA, post-hoc EMA, step guard, clipping), the same on the one-rank sharded bf16
exchange followed by consolidate(), Muon, LoRAAdamW projected and factored, and FusedAdamW with the learned loss weighting.  There the
recorder also stands in for hip._lib, so the optimisers' own launches are traced; the hashes are the loss of every step, the masters,
the bf16 shadow, both moments, the EMA, every post-hoc profile and the adapter's / loss weighting's weights.

Per case the file holds
  trace   the ordered list of every call made through `eng.L` (a recording proxy stands in for it): symbol, return code, the integer
          and float arguments, for byref structs their non-pointer fields in order, trailing zeros dropped (pointer fields as p = set / 0 = null), for
          grouped GEMMs each problem's lda, ldb, M, N, c_off.  An integer >= 2^40 is an address: "ptr"; None: "null".  The entries are
          interned: `calls` is the table of distinct entries, `trace` indexes it.
  sha256  of the loss, and one digest over the SHA-256 of every gradient tensor's bytes in parameter order (Trainer case: of the
          fp32 masters after the step).
The full file (~65 KB) names the first differing call when two of them are compared; profiles/ keeps its digest (digest()), which
--compare takes as well.  The tool touches `eng.L` and public entry points only, so the same file runs against any commit of the project."""
import argparse
import ctypes
import hashlib
import json
import os
import socket
import sys

os.environ["MD_DETERMINISTIC"] = "1"            # before the package is imported: the engine reads it when it is built
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ADDRESS = 1 << 40
_BYREF = type(ctypes.byref(ctypes.c_int()))


def _scalar(v):
    if v is None:
        return "null"
    if isinstance(v, bool):
        return int(v)
    if isinstance(v, int):
        return "ptr" if v >= ADDRESS else v
    if isinstance(v, float):
        return v
    raise TypeError(f"unexpected launch argument {v!r}")


def _struct(s):
    from micro_diffusion_amd import hip
    if not isinstance(s, ctypes.Structure):
        return "out"                             # byref(c_int32 / c_int64): a value the library writes
    ptrs, vals = "", []
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is ctypes.c_void_p:
            ptrs += "p" if v else "0"
        else:
            vals.append(_scalar(v))
    while vals and not vals[-1]:
        vals.pop()
    rec = [type(s).__name__, ptrs, vals]
    if isinstance(s, hip.GemmArgs) and s.problems and s.n_problems > 0:
        table = (hip.GemmProblem * s.n_problems).from_address(s.problems)
        rec.append([[g.lda, g.ldb, g.M, g.N, g.c_off] for g in table])
    return rec


def _array(a):
    """A host table the optimisers pass (range tables, EMA pointers and betas, Muon / LoRA items): its elements in order."""
    if issubclass(a._type_, ctypes.Structure):
        return [_struct(e) for e in a]
    if a._type_ is ctypes.c_void_p:
        return "".join("p" if e else "0" for e in a)
    return [_scalar(e) for e in a]


class Recorder:
    """Stands in for DiTEngine.L (and, in the step cases, for hip._lib): records every call, then makes it."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            entry = [name, None] + [_struct(a._obj) if isinstance(a, _BYREF) else _array(a) if isinstance(a, ctypes.Array) else _scalar(a)
                                    for a in args]
            rc = fn(*args)
            entry[1] = rc
            self._log.append(json.dumps(entry, separators=(",", ":")))
            return rc
        return call


def _sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _model(cfg, sd, ratio, pm=-0.6, ps=1.2):
    from micro_diffusion_amd import dit as mdit
    from micro_diffusion_amd.model import LatentDiffusion, _FrozenStub
    d = mdit.DiT(**cfg.__dict__)
    d.load_state_dict(sd)
    m = LatentDiffusion(d.to("cuda"), _FrozenStub("vae"), _FrozenStub("te"), _FrozenStub("tok"), p_mean=pm, p_std=ps, train_mask_ratio=ratio)
    m.train()
    return m


def _microbatch_case(cfgf, seed, ratio, pm, ps, cap, arena):
    import torch
    from oracle import microdit_ref as orc
    cfg = cfgf()
    sd = orc.dezero_state_dict(orc.synth_state_dict(cfg, seed))
    batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 4, seed + 1, cap_len=cap)
    gb = {k: t.cuda() for k, t in batch.items()}
    noise = (rnd.cuda(), epsn.cuda(), mnoise.cuda() if ratio > 0 else None)
    m = _model(cfg, sd, ratio, pm, ps)
    eng, log = m.dit.engine, []
    assert eng.deterministic is True
    eng.L = Recorder(eng.L, log)
    eng.use_arena = arena
    m._noise_fn = lambda b: noise
    for _ in range(2 if arena else 1):
        loss = m.train_microbatch(gb)
    torch.cuda.synchronize()
    grads = hashlib.sha256("".join(f"{k}:{_sha(p.grad)}\n" for k, p in m.dit.named_parameters()).encode()).hexdigest()
    return log, {"loss": _sha(loss), "gradients": grads}


def _trainer_case():
    import torch
    import torch.distributed as dist
    from oracle import microdit_ref as orc
    from micro_diffusion_amd.trainer import FusedAdamW, LRSchedule, Trainer
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        cfg = orc.tiny_config()
        sd = orc.dezero_state_dict(orc.synth_state_dict(cfg, 71))
        batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 4, 72)
        m = _model(cfg, sd, 0.75)
        m._noise_fn = lambda b: (rnd.cuda(), epsn.cuda(), mnoise.cuda())
        opt = FusedAdamW(m.dit, lr=2.4e-4)
        tr = Trainer(m, opt, LRSchedule("constant", alpha=1.0), clip_norm=0.25, microbatch_size=4, exchange="bf16", single_rank_exchange=True,
                     dp_mode="sharded")
        eng, log = m.dit.engine, []
        eng.L = Recorder(eng.L, log)
        loss = tr.train_step({k: t.cuda() for k, t in batch.items()})
        tr.sync.wait_gather()
        torch.cuda.synchronize()
        assert tr.sync.last_stored > 0, "the step was meant to store its weight gradients as bf16"
        return log, {"loss": _sha(loss), "masters": _sha(m.dit.flat_buffers()["p"]), "stored": str(tr.sync.last_stored)}
    finally:
        dist.destroy_process_group()


STEP_CASES = ("adamw", "adamw_sharded", "muon", "lora_projected", "lora_factored", "adamw_loss_weighting")


def _step_case(kind):
    """Three Trainer.train_steps of two microbatches each (tiny, batch 4) under one optimiser; the recorder also stands in for
    hip._lib, so the optimiser's own launches are in the trace.  Hashes: the loss of every step and the state the steps leave."""
    import torch
    import torch.distributed as dist
    from oracle import microdit_ref as orc
    from micro_diffusion_amd import hip
    from micro_diffusion_amd.trainer import FusedAdamW, LRSchedule, Trainer
    sharded = kind == "adamw_sharded"
    if sharded:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    real = hip.lib()
    try:
        cfg = orc.tiny_config()
        sd = orc.dezero_state_dict(orc.synth_state_dict(cfg, 81))
        batch, rnd, epsn, mnoise = orc.synth_batch(cfg, 4, 82)
        m = _model(cfg, sd, 0.75)
        # one fixed draw per microbatch of two samples (the same in every step)
        m._noise_fn = lambda b: (rnd.cuda()[:2], epsn.cuda()[:2], mnoise.cuda()[:2])
        adamw = dict(lr=2.4e-4, ema_smoothing=0.999, ema_start=1, skip_nonfinite=True, posthoc_sigma_rels=(0.05, 0.1))
        adapter = lw = None
        if kind == "muon":
            from micro_diffusion_amd.muon import Muon
            opt = Muon(m.dit, **adamw)
        elif kind.startswith("lora"):
            from micro_diffusion_amd import lora
            adapter = lora.LoRA(m.dit, rank=8, alpha=4, seed=5, backward=kind[5:])
            opt = lora.LoRAAdamW(adapter, lr=1e-3, skip_nonfinite=True)
        else:
            opt = FusedAdamW(m.dit, **adamw)
        kw = dict(exchange="bf16", single_rank_exchange=True, dp_mode="sharded") if sharded else {}
        if kind == "adamw_loss_weighting":
            from micro_diffusion_amd.loss_weighting import LossWeighting
            lw = kw["loss_weighting"] = LossWeighting(channels=64, seed=3)
        tr = Trainer(m, opt, LRSchedule("constant", alpha=1.0), clip_norm=0.25, microbatch_size=2, **kw)
        log = []
        rec = hip._lib = m.dit.engine.L = Recorder(real, log)
        gb = {k: t.cuda() for k, t in batch.items()}
        sha = {}
        for i in range(3):
            sha[f"loss{i}"] = _sha(tr.train_step(gb))
        if sharded:
            tr.consolidate()
            tr.sync.wait_gather()
        torch.cuda.synchronize()
        assert rec is hip._lib
        f = m.dit.flat_buffers()
        sha.update(p=_sha(f["p"]), s=_sha(f["s"]), m=_sha(opt.m), v=_sha(opt.v))
        if getattr(opt, "ema", None) is not None:
            sha["ema"] = _sha(opt.ema)
        for k, e in enumerate(getattr(opt, "posthoc", None) or ()):
            sha[f"posthoc{k}"] = _sha(e)
        if adapter is not None:
            sha["adapter_w"] = _sha(adapter.w)
        if lw is not None:
            sha["lw_w"] = _sha(lw.w)
        sha["skipped"] = str(opt.skipped_steps())
        return log, sha
    finally:
        hip._lib = real
        if sharded:
            dist.destroy_process_group()


def run(out_path, digest_path=None, which="engine"):
    from oracle import microdit_ref as orc
    from micro_diffusion_amd import hip
    specs = [("tiny_mask75", orc.tiny_config, 61, 0.75, -0.6, 1.2, 77), ("tiny_mask0", orc.tiny_config, 62, 0.0, -0.6, 1.2, 77),
             ("micro_mask50", orc.micro_config, 63, 0.5, 0.0, 0.6, 20)]
    calls, index, cases = [], {}, {}

    def keep(name, log, sha):
        trace = []
        for e in log:
            if e not in index:
                index[e] = len(calls)
                calls.append(json.loads(e))
            trace.append(index[e])
        cases[name] = {"trace": trace, "sha256": sha}
        print(f"{name}: {len(trace)} calls", flush=True)

    if which == "step":
        for kind in STEP_CASES:
            keep("step_" + kind, *_step_case(kind))
    else:
        for name, *spec in specs:
            for arena in (False, True):
                keep(name + ("+arena" if arena else ""), *_microbatch_case(*spec, arena))
        keep("trainer_one_microbatch", *_trainer_case())
    doc = {"library_source_hash": hip._source_hash(), "calls": calls, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    if digest_path:
        write_digest(digest(doc), digest_path)
    print(f"wrote {out_path}: {len(calls)} distinct calls")


def write_digest(d, path):
    with open(path, "w") as f:                       # one line per case
        f.write('{"library_source_hash": "%s", "cases": {\n' % d["library_source_hash"])
        f.write(",\n".join(f'"{name}": {json.dumps(c)}' for name, c in d["cases"].items()) + "\n}}\n")


def digest(doc):
    """The small form of a fingerprint (what profiles/ keeps): per case the number of calls, the calls per symbol, ONE SHA-256 over the
    ordered trace entries and the hashes of the results.  Equal digests: equal traces; which call differs takes the two full files."""
    if "calls" not in doc:
        return doc
    cases = {}
    for name, c in doc["cases"].items():
        entries = [json.dumps(doc["calls"][i], separators=(",", ":")) for i in c["trace"]]
        symbols = {}
        for i in c["trace"]:
            symbols[doc["calls"][i][0]] = symbols.get(doc["calls"][i][0], 0) + 1
        cases[name] = {"calls": len(entries), "trace_sha256": hashlib.sha256("\n".join(entries).encode()).hexdigest(),
                       "symbols": dict(sorted(symbols.items())), "sha256": c["sha256"]}
    return {"library_source_hash": doc["library_source_hash"], "cases": cases}


def compare(pa, pb):
    a, b = (json.load(open(p)) for p in (pa, pb))
    if a["library_source_hash"] != b["library_source_hash"]:
        print(f"native library sources differ: {a['library_source_hash']} vs {b['library_source_hash']}")
        return 1
    if sorted(a["cases"]) != sorted(b["cases"]):
        print(f"cases differ: {sorted(a['cases'])} vs {sorted(b['cases'])}")
        return 1
    full = "calls" in a and "calls" in b
    da, db = digest(a), digest(b)
    for name in a["cases"]:
        ca, cb = da["cases"][name], db["cases"][name]
        if full:                           # two full files: the first call that differs
            ta, tb = ([d["calls"][i] for i in d["cases"][name]["trace"]] for d in (a, b))
            for i, (x, y) in enumerate(zip(ta, tb)):
                if x != y:
                    print(f"{name}: call {i} differs\n  A: {json.dumps(x)}\n  B: {json.dumps(y)}")
                    return 1
            if len(ta) != len(tb):
                longer, which = (ta, "A") if len(ta) > len(tb) else (tb, "B")
                print(f"{name}: {len(ta)} vs {len(tb)} calls; first call only in {which}: {json.dumps(longer[min(len(ta), len(tb))])}")
                return 1
        elif (ca["calls"], ca["symbols"], ca["trace_sha256"]) != (cb["calls"], cb["symbols"], cb["trace_sha256"]):
            counts = {s: (ca["symbols"].get(s, 0), cb["symbols"].get(s, 0)) for s in sorted(set(ca["symbols"]) | set(cb["symbols"]))
                      if ca["symbols"].get(s) != cb["symbols"].get(s)}
            print(f"{name}: the traces differ ({ca['calls']} vs {cb['calls']} calls; per symbol: {counts or 'equal counts, other arguments'}); "
                  "two full files name the call")
            return 1
        for k in sorted(set(ca["sha256"]) | set(cb["sha256"])):
            if ca["sha256"].get(k) != cb["sha256"].get(k):
                print(f"{name}: same launches, but the bits of {k} differ ({ca['sha256'].get(k)} vs {cb['sha256'].get(k)})")
                return 1
    n = sum(c["calls"] for c in da["cases"].values())
    h = sum(len(c["sha256"]) for c in da["cases"].values())
    print(f"identical: {len(da['cases'])} cases, {n} calls, {h} hashes")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="engine_fingerprint.json", help="the full fingerprint: every call with its arguments")
    ap.add_argument("--digest-out", default=None, help="also write the small form (see digest())")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"), help="full files or digests; prints the first difference")
    ap.add_argument("--cases", choices=("engine", "step"), default="engine",
                    help="engine: the microbatch cases above; step: three optimiser steps under every optimiser (profiles/step_fingerprint_*.json)")
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run(args.out, args.digest_out, args.cases))
