"""The split-K planner (micro_diffusion_amd/splitk.py) gives the plans the engine gave before the planning was moved out of it.

tests/splitk_plan_table.json was recorded from DiTEngine._ksplit, _wgrad_flush, _dycond_grouped and _adaln_dgrad_grouped at the commit
before splitk.py existed (`python tests/test_splitk_plan_cpu.py --record` drives those methods of a half-built engine whose _gemm, L, ws
and gemm_f32_acc are recording stubs; it runs against any commit that has the methods).  Inputs: a host walk over the backward of XL/2
at microbatch 256 and 1024, mask ratio 0 and 0.75, caption length 77, and of the tiny and micro configurations at batch 4 -- every
shape the walk hands to gemm_f32_acc, the weight-gradient groups of both flush points of a selection of dense and MoE blocks, the
caption-token and condition-vector groups of both stacks -- plus the shapes of test_splitk_factor_fills_whole_rounds, ragged
contractions and a few synthetic groups (a workspace too small: the one-by-one fall-back).  A ksplit row is a shape and its factor
under three settings of the A/B switches (KSPLIT_SWITCHES): the defaults, ksplit_min_items = 128, short_k_accum = False.

Two tests: the pure planner reproduces every row, and so do the engine methods that now ask it (planner + ctypes table + launches)."""
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from micro_diffusion_amd import hip                                                 # noqa: E402
from micro_diffusion_amd.arch import DiTConfig, caption_ffn_hidden, param_table, plan_blocks   # noqa: E402
from micro_diffusion_amd.dit import flat_layout                                     # noqa: E402
from micro_diffusion_amd.engine import DiTEngine                                    # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "splitk_plan_table.json")
WS_FLOATS = 128 << 20
WS_BASE, G_BASE, S_BASE, BUF_BASE, W_BASE = 1 << 40, 1 << 41, 1 << 42, 1 << 43, 1 << 44
INT_KEYS = ("ksplit", "sSplit", "K", "list_segments", "n_problems", "M", "N", "ldc", "sC")


# ------------------------------------------------------------------------------------------------ a half-built engine that records
class T:
    """A tensor stand-in: address and element count."""
    dtype = None

    def __init__(self, ptr, numel=0, item=0):
        self.ptr, self.n, self.item = ptr, numel, item

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n

    def __getitem__(self, i):
        return T(self.ptr + i * self.item)


class Group(dict):
    """The per-stack state of a grouped data gradient as the engine methods read it: by key or by attribute."""

    def __init__(self, buf, w):
        super().__init__(buf=buf, w=w)
        self.buf, self.w = buf, w


def stub_engine(cfg=None, ws_floats=WS_FLOATS, min_items=192, short_k=True):
    """(engine, calls): a DiTEngine without __init__ whose launches land in `calls` as canonical records."""
    calls = {"gemm": None, "c_off": None, "lists": [], "reduce": [], "acc": []}

    def gemm(**kw):
        calls["gemm"] = {k: int(kw[k]) for k in INT_KEYS if k in kw}
        if kw.get("problems"):
            table = (hip.GemmProblem * kw["n_problems"]).from_address(kw["problems"])
            calls["c_off"] = [g.c_off for g in table]
        return True

    def reduce_flat(ws, out, n, stride, ks, mode, st):
        calls["reduce"].append(["flat", ws - WS_BASE, out - G_BASE, n, stride, ks, mode])
        return 0

    def reduce_2d(ws, out, M, N, ldo, sOut, ks, batch, mode, st):
        calls["reduce"].append(["2d", ws - WS_BASE, M, N, ldo, sOut, ks, batch, mode])
        return 0

    def ptr_list(ptrs):
        calls["lists"].append([p - (BUF_BASE if p < W_BASE else W_BASE) for p in ptrs])
        return T(0)

    eng = DiTEngine.__new__(DiTEngine)
    eng.cfg = cfg
    eng.ws = T(WS_BASE, ws_floats)
    eng.L = type("L", (), {"md_splitk_reduce_flat": staticmethod(reduce_flat), "md_splitk_reduce": staticmethod(reduce_2d)})()
    eng.kernel_profile = eng.gemm_profile = eng.wgrad_bf16 = eng._wgroup = None
    eng.group_wgrad = eng.single_slice_ws = True
    eng.splitk_force_pp = eng.deterministic = False
    eng.gemm_prefer = hip.GEMM_AUTO
    eng.wgrad_target_blocks, eng.ksplit_min_items, eng.short_k_accum = 768, min_items, short_k
    eng._st = lambda: 0
    eng._gemm = gemm
    eng._ptr_list = ptr_list
    eng._colsum = lambda *a: None
    eng.gemm_f32_acc = lambda **kw: calls["acc"].append([kw["M"], kw["N"], kw["K"], kw.get("batch", 1)])
    eng.P = eng.S = eng.G = {}
    if cfg is not None:
        table = [s for s in param_table(cfg) if not s.buffer]
        offs, _ = flat_layout(param_table(cfg))
        numel = {s.name: int(np.prod(s.shape)) for s in table}
        eng.P = {s.name: T(0) for s in table}
        eng.S = {n: T(S_BASE + 2 * o, numel[n]) for n, o in offs.items()}
        eng.G = {n: T(G_BASE + 4 * o, numel[n]) for n, o in offs.items()}
    return eng, calls


def taken(calls):
    """The canonical record of what ran since the last call, then forget it."""
    out = {"acc": calls["acc"]} if calls["gemm"] is None else {
        k: v for k, v in (("gemm", calls["gemm"]), ("c_off", calls["c_off"]), ("lists", calls["lists"]), ("reduce", calls["reduce"])) if v}
    calls.update(gemm=None, c_off=None, lists=[], reduce=[], acc=[])
    return out


# ------------------------------------------------------------------------------------------------ the rows' outputs from the ENGINE
KSPLIT_SWITCHES = ((192, True), (128, True), (192, False))     # (ksplit_min_items, short_k_accum) of a ksplit row's three results


def engine_ksplit(row):
    """[rows, cols, contraction, batch] -> the factor under each of KSPLIT_SWITCHES."""
    return [stub_engine(min_items=mi, short_k=sk)[0]._ksplit(*row[:4]) for mi, sk in KSPLIT_SWITCHES]


def engine_wgrad(row):
    eng, calls = stub_engine(ws_floats=row["ws_floats"])
    eng._wgroup = [dict(tokens=row["tokens"], A=1, lda=M, B=2, ldb=N, M=M, N=N, out=G_BASE + off, keep=None) for off, M, N in row["problems"]]
    eng._wgrad_flush()
    return taken(calls)


def _group(G, item):
    return Group(T(BUF_BASE, item=item), [W_BASE + (i << 28) for i in range(G)])


def engine_dycond(row):
    G, Mc, d, K, ws_floats = row["in"]
    eng, calls = stub_engine(ws_floats=ws_floats)
    eng._dycond_grouped(_group(G, 2 * Mc * K), Mc, d, K, T(G_BASE))
    return taken(calls)


def engine_adaln(row):
    G, B, N, D, ws_floats = row["in"]
    eng, calls = stub_engine(ws_floats=ws_floats)
    eng.cfg = DiTConfig(dim=D)
    eng._adaln_dgrad_grouped(_group(G, 2 * B * N), B, N, T(G_BASE))
    return taken(calls)


# ------------------------------------------------------------------------------------------------ ... and from the PLANNER alone
def planner_wgrad(row):
    from micro_diffusion_amd import splitk
    probs = sorted(row["problems"])
    plan = splitk.plan_wgrad_group([(G_BASE + off, M, N) for off, M, N in probs], row["tokens"], row["ws_floats"])
    if plan is None:
        return {"acc": [[M, N, row["tokens"], 1] for _, M, N in probs]}
    first = probs[0]
    return {"gemm": {"ksplit": plan.ks, "sSplit": plan.span, "K": row["tokens"], "n_problems": len(probs), "M": first[1], "N": first[2], "ldc": first[2]},
            "c_off": list(plan.offsets),
            "reduce": [["flat", 4 * off, first[0] + 4 * off, n, plan.span, plan.ks, 1] for off, n in plan.runs]}


def planner_dycond(row):
    from micro_diffusion_amd import splitk
    G, Mc, d, K, ws_floats = row["in"]
    plan = splitk.plan_dycond(G, Mc, d, K, ws_floats)
    if plan is None:
        return {"acc": [[Mc, d, K, 1]] * G}
    ks, seg = plan
    return {"gemm": {"ksplit": ks, "sSplit": Mc * d, "K": K * G, "list_segments": seg, "M": Mc, "N": d, "ldc": d, "sC": ks * Mc * d},
            "lists": [[2 * i * Mc * K for i in range(G)], [i << 28 for i in range(G)]],
            "reduce": [["2d", 0, Mc, d, d, 0, ks, 1, 1]]}


def planner_adaln(row):
    from micro_diffusion_amd import splitk
    G, B, N, D, ws_floats = row["in"]
    plan = splitk.plan_adaln_dgrad(G, B, N, D, ws_floats)
    if plan is None:
        return {"acc": [[B, D, N, 1]] * G}
    parts, kspan, ks = plan
    return {"gemm": {"ksplit": ks, "sSplit": B * D, "K": kspan * ks, "M": B, "N": D, "ldc": D, "sC": ks * B * D},
            "lists": [[2 * (i * B * N + c * kspan) for i in range(G) for c in range(parts)],
                      [(i << 28) + 2 * c * kspan * D for i in range(G) for c in range(parts)]],
            "reduce": [["2d", 0, B, D, D, 0, ks, 1, 1]]}


# ------------------------------------------------------------------------------------------------ the inputs: a host walk of _backward
def walk_backward(cfg, B, mask_ratio, Lc, blocks_kept=None):
    """Drive the recording engine through the weight-gradient and grouped-dgrad calls of DiTEngine._backward / _block_bwd (default
    switches), in their order.  Returns (shapes handed to gemm_f32_acc, wgrad rows, dycond rows, adaln rows)."""
    eng, calls = stub_engine(cfg)
    mixer, backbone = plan_blocks(cfg)
    Tn = cfg.tokens
    Tk = int(Tn * (1 - mask_ratio)) if mask_ratio > 0 else Tn
    D, Dm, pv, Dc, E = cfg.dim, cfg.patch_mixer_dim, cfg.patch_vec, cfg.caption_channels, cfg.num_experts
    Mc, X = B * Lc, T(8)
    shapes, wgrad, dycond, adaln = [], [], [], []

    def lw(name, M, N, K, **kw):
        eng.lin_wgrad(X, X, name, M, N, K, **kw)

    def acc(**kw):
        eng._param_acc(A=8, B=8, a_kcontig=0, b_kcontig=0, **kw)

    def flush(keep):
        grp = eng._wgroup or []
        row = {"tokens": grp[0]["tokens"] if grp else 0, "ws_floats": WS_FLOATS, "problems": [[g["out"] - G_BASE, g["M"], g["N"]] for g in grp]}
        shapes.extend(calls["acc"])
        calls["acc"] = []
        eng._wgrad_flush()
        row["plan"] = taken(calls)
        shapes.extend(row["plan"].get("acc", []))
        if keep and grp:
            wgrad.append(row)

    def ffn(pre, M, d, f, defer):
        lw(pre + ".w3", M, d, f, defer=defer)
        if eng._fused12(pre):
            lw(pre + ".w1", M, 2 * f, d, defer=defer)
        else:
            lw(pre + ".w1", M, f, d, lddy=2 * f, defer=defer)
            lw(pre + ".w2", M, f, d, lddy=2 * f, dyoff=f, defer=defer)

    def block(bp, S, keep, cap=None):
        n, d, h, hx, f, M = bp.name, bp.dim, bp.attn_hidden, bp.xattn_hidden, bp.ffn_hidden, B * S
        eng._wgrad_begin()
        if not bp.moe:
            ffn(n + ".mlp", M, d, f, True)
        else:
            k = int(cfg.expert_capacity * S / E)
            rows = cap or B * k
            acc(out_ptr=eng.G[n + ".mlp.w2"].data_ptr(), M=f, N=d, K=rows, ldo=d, batch=E, sOut=f * d)
            acc(out_ptr=eng.G[n + ".mlp.w1"].data_ptr(), M=d, N=f, K=rows, ldo=f, batch=E, sOut=d * f)
            lw(n + ".mlp.gate", M, E, d, lddy=8 if E <= 8 else 16)
        lw(n + ".cross_attn.proj", M, d, hx, defer=True)
        lw(n + ".cross_attn.q_linear", M, hx, d, defer=True)
        lw(n + ".cross_attn.kv_linear", Mc, 2 * hx, d)
        flush(keep)
        lw(n + ".attn.proj", M, d, h, defer=True)
        lw(n + ".attn.qkv", M, 3 * h, d, defer=True)
        flush(keep)
        eng._wgroup = None
        lw(n + ".adaLN_modulation.1", B, 6 * d, D, bias_from=X)

    def stack(blocks, S, which):
        for i, bp in reversed(list(enumerate(blocks))):
            cap = None
            if which == "m" and mask_ratio > 0 and i == len(blocks) - 1 and bp.moe:      # masked-expert pruning: whole 256-row granules
                Bk = B * int(cfg.expert_capacity * S / E)
                cap = -(-int(Bk * (1 - mask_ratio)) // 256) * 256
                cap = cap if cap < Bk else None
            block(bp, S, blocks_kept is None or (which, i) in blocks_kept, cap)
        if blocks:
            d, K = blocks[0].dim, 2 * blocks[0].xattn_hidden
            for fn, rows, item, args in ((eng._dycond_grouped, dycond, 2 * Mc * K, (Mc, d, K)), (eng._adaln_dgrad_grouped, adaln, 2 * B * 6 * d, (B, 6 * d))):
                fn(_group(len(blocks), item), *args, T(G_BASE))
                dims = [len(blocks), *args] if fn == eng._dycond_grouped else [len(blocks), B, 6 * d, D]
                rows.append({"in": dims + [WS_FLOATS], "plan": taken(calls)})

    lw("final_layer.linear", B * Tk, pv, D)
    lw("final_layer.adaLN_modulation.1", B, 2 * D, D, bias_from=X)
    eng.gemm_f32_acc(M=B, N=D, K=2 * D)
    stack(backbone, Tk, "b")
    if cfg.has_maps:
        lw("patch_mixer_map_xout.1", B * Tk, D, Dm)
    stack(mixer, Tn, "m")
    if cfg.has_maps:
        lw("patch_mixer_map_xin.1", B * Tn, Dm, D)
    acc(out_ptr=eng.G["x_embedder.proj.weight"].data_ptr(), M=D, N=pv, K=B * Tn, ldo=pv)
    lw("t_embedder.mlp.2", B, D, D)
    lw("t_embedder.mlp.0", B, D, 512)
    lw("pooled_y_emb_process.fc2", B, D, D)
    lw("pooled_y_emb_process.fc1", B, D, D)
    if cfg.has_maps:
        lw("patch_mixer_map_y.1", Mc, Dm, D)
    ffn("y_emb_preprocess.mlp", Mc, D, caption_ffn_hidden(cfg), False)
    lw("y_emb_preprocess.attn.proj", Mc, D, D)
    lw("y_emb_preprocess.attn.qkv", Mc, 3 * D, D)
    lw("y_embedder.y_proj.fc2", Mc, D, D)
    lw("y_embedder.y_proj.fc1", Mc, D, Dc)
    shapes.extend(calls["acc"])
    return shapes, wgrad, dycond, adaln


OLD_TEST_SHAPES = [(1024, 1024, 65536, 1), (2048, 1024, 78848, 1), (1024, 1024, 16384, 1), (78848, 1024, 2048, 1), (1024, 3840, 4096, 8),
                   (768, 3072, 65536, 8), (16, 1024, 65536, 1), (256, 256, 1024, 1), (1024, 8, 512, 1), (768, 768, 262144, 1),
                   (5376, 1024, 65536, 1), (3072, 1024, 16384, 1), (6144, 1024, 1024, 1), (1024, 1024, 1000, 1), (6144, 1024, 256, 1)]
RAGGED = [(1024, 1024, 308, 1), (2048, 1024, 308, 1), (1024, 1024, 1000, 1), (768, 768, 1000, 4), (256, 1024, 1024, 1), (128, 128, 308, 1)]


def record():
    from oracle import microdit_ref as orc
    xl = DiTConfig(**orc.xl2_config().__dict__)
    some = {("m", 0), ("m", 5), ("b", 0), ("b", 1), ("b", 27)}         # dense and MoE blocks of both stacks, the pruned one included
    runs = [(xl, mb, ratio, 77, some) for mb in (256, 1024) for ratio in (0.0, 0.75)]
    runs += [(DiTConfig(**orc.tiny_config().__dict__), 4, 0.75, 77, None), (DiTConfig(**orc.micro_config().__dict__), 4, 0.5, 20, None)]
    shapes, wgrad, dycond, adaln = [], [], [], []
    for run in runs:
        s, w, d, a = walk_backward(*run)
        shapes += s
        wgrad += w
        dycond += d
        adaln += a
    shapes = sorted(set(map(tuple, shapes)) | set(OLD_TEST_SHAPES) | set(RAGGED))
    ksplit = [[*s, *engine_ksplit(s)] for s in shapes]
    # synthetic groups: the group of test_grouped_wgrad_host_logic; a workspace the span does not fit (one by one); small workspaces
    MB = 1 << 20
    wgrad.append({"tokens": 16384, "ws_floats": WS_FLOATS, "problems": [[48 * MB, 1024, 2816], [16 * MB + 8 * MB + 4 * MB, 5632, 1024], [12 * MB + 8 * MB, 1024, 1024], [0, 1024, 1024]]})
    wgrad.append({"tokens": 16384, "ws_floats": WS_FLOATS, "problems": [[0, 1024, 1024], [4 * (129 << 20), 1024, 1024]]})
    wgrad.append({"tokens": 4096, "ws_floats": 3 * MB, "problems": [[0, 1024, 1024], [4 * MB, 1024, 1024], [12 * MB, 512, 1024]]})
    wgrad.append({"tokens": 1024, "ws_floats": WS_FLOATS, "problems": [[0, 768, 768]]})
    dycond += [{"in": [28, 19712, 1024, 2048, 32 * MB]}, {"in": [28, 19712, 1024, 2048, 16 * MB]}, {"in": [6, 308, 768, 1536, WS_FLOATS]},
               {"in": [4, 308, 128, 200, WS_FLOATS]}]
    adaln += [{"in": [28, 256, 6144, 1024, 2 * MB]}, {"in": [2, 1024, 6144, 1024, WS_FLOATS]}, {"in": [6, 4, 4608, 1024, WS_FLOATS]},
              {"in": [3, 8, 200, 64, WS_FLOATS]}]

    def dedupe(rows):
        seen, out = set(), []
        for r in rows:
            key = json.dumps({k: v for k, v in r.items() if k != "plan"}, sort_keys=True)
            if key not in seen:
                seen.add(key)
                out.append(r)
        return out

    wgrad, dycond, adaln = dedupe(wgrad), dedupe(dycond), dedupe(adaln)
    for rows, fn in ((wgrad, engine_wgrad), (dycond, engine_dycond), (adaln, engine_adaln)):
        for r in rows:
            plan = fn(r)
            assert r.get("plan", plan) == plan, "the walk and the replay of its inputs must agree"
            r["plan"] = plan
    with open(TABLE, "w") as f:
        per_line = [", ".join(json.dumps(r, separators=(",", ":")) for r in ksplit[i:i + 5]) for i in range(0, len(ksplit), 5)]
        f.write('{"ksplit": [\n' + ",\n".join(per_line) + "\n],\n")
        for name, rows in (("wgrad", wgrad), ("dycond", dycond), ("adaln", adaln)):
            f.write(f'"{name}": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + ("\n],\n" if name != "adaln" else "\n]}\n"))
    print(f"{TABLE}: {len(ksplit)} ksplit, {len(wgrad)} wgrad, {len(dycond)} dycond, {len(adaln)} adaln rows, {os.path.getsize(TABLE)} bytes")


# ------------------------------------------------------------------------------------------------ tests
def _table():
    with open(TABLE) as f:
        return json.load(f)


def test_table_holds_every_outcome_class():
    """A table that lost its hard rows cannot pass quietly."""
    tab = _table()
    ks = {tuple(r[:4]): r[4:] for r in tab["ksplit"]}                    # shape -> factors under KSPLIT_SWITCHES
    assert ks[(6144, 1024, 256, 1)][0] == 1 and ks[(6144, 1024, 256, 1)][2] != 1     # plain 1 by the short-contraction rule, and by nothing else
    assert ks[(78848, 1024, 2048, 1)][0] == -1
    assert ks[(1024, 1024, 65536, 1)][0] == 16                           # a pp256 factor > 1
    K = 1024                                                             # the 128 x 128 rule: pp256 cannot reach 192 items (4 tiles x 8 units)
    assert ks[(256, 1024, K, 1)][0] == min(768 // 16, K // 512) == 2
    assert any(r[4] > 1 and r[2] % (128 * r[4]) == 0 for r in tab["ksplit"]) and any(r[2] % 128 and r[4] >= 1 for r in tab["ksplit"])
    assert any(r[4] != r[5] for r in tab["ksplit"]) and any(r[4] != r[6] for r in tab["ksplit"]), "the switches must matter somewhere"
    for name in ("wgrad", "dycond", "adaln"):
        assert any("acc" in r["plan"] for r in tab[name]), f"{name}: no group that falls back to one-by-one"
        assert any("gemm" in r["plan"] for r in tab[name]), f"{name}: no grouped launch"
    assert any(len(r["problems"]) > 1 and "acc" in r["plan"] for r in tab["wgrad"])
    assert any(len(r["plan"].get("reduce", ())) > 1 for r in tab["wgrad"]), "no group with more than one contiguous run"
    assert any(r["plan"].get("gemm", {}).get("ksplit", 1) > 1 for r in tab["wgrad"])
    assert any(r["plan"].get("gemm", {}).get("list_segments", 1) > 1 for r in tab["dycond"])
    assert len(tab["ksplit"]) + len(tab["wgrad"]) + len(tab["dycond"]) + len(tab["adaln"]) < 1000 and os.path.getsize(TABLE) < 100_000


def test_planner_reproduces_every_recorded_plan():
    from micro_diffusion_amd import splitk
    tab = _table()
    for *shape, r192, r128, rlong in tab["ksplit"]:
        got = [splitk.choose_ksplit(*shape, ws_floats=WS_FLOATS, min_items=mi, short_k_accum=sk) for mi, sk in KSPLIT_SWITCHES]
        assert got == [r192, r128, rlong], (shape, got, [r192, r128, rlong])
    for name, fn in (("wgrad", planner_wgrad), ("dycond", planner_dycond), ("adaln", planner_adaln)):
        for row in tab[name]:
            assert fn(row) == row["plan"], (name, {k: v for k, v in row.items() if k != "plan"}, fn(row), row["plan"])


def test_engine_methods_reproduce_every_recorded_plan():
    """The same rows through DiTEngine._ksplit / _wgrad_flush / _dycond_grouped / _adaln_dgrad_grouped: the planner's answer, the
    ctypes problem table and the launches together."""
    tab = _table()
    for row in tab["ksplit"]:
        assert engine_ksplit(row) == row[4:], row
    for name, fn in (("wgrad", engine_wgrad), ("dycond", engine_dycond), ("adaln", engine_adaln)):
        for row in tab[name]:
            assert fn(row) == row["plan"], (name, {k: v for k, v in row.items() if k != "plan"}, fn(row), row["plan"])


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        record()
    else:
        sys.exit("usage: python tests/test_splitk_plan_cpu.py --record")
