"""The bits of the sampler's elementwise kernels, pinned: a fixed case list over the twelve md_edm_{heun,solver}_update entry points and the
kernels that share their token geometry, each case reduced to the SHA-256 of every output buffer.

The existing tests compare the forms with each other (token = image, _guide = doubled batch) and with torch fp64 under a tolerance; none of
them would notice all forms moving together by one ulp.  tests/golden/sampler_kernel_bits.json holds the digests one build of the library
gave (scripts/record_sampler_bits.py writes it); tests/test_sampler_kernel_bits_gpu.py recomputes them.  The arithmetic of these kernels
is fp32 / fp64 with every multiply-add an explicit fma (csrc/sampler_math.h), so a digest that moves is a changed kernel, not noise.

Inputs are a closed-form integer pattern (a multiplicative hash of the element index mapped to [-3, 3)), not a library random generator:
the fixture does not depend on the torch version.  fp32 and bf16 inputs are the fp64 pattern rounded once by .to().

launch_update() and Inputs are also what scripts/ab_sampler_kernels.py times, at the shapes a user runs.
"""
import hashlib

import torch

P = 2
SD = 0.9                        # sigma_data
T_IN, T_HAT, T_NEXT = 1.7, 2.1, 1.2
CFG = 3.0
SHAPES = [(3, 4, 6, 10),        # patch_vec 16: the 16-byte path, 720 elements (no multiple of 256), odd batch
          (2, 3, 6, 10),        # patch_vec 12: the element path with a ragged last segment
          (2, 16, 8, 8)]        # patch_vec 64: several segments per row
COEFS = {"no_history": (0.625, 0.375, 1.0, 0.0),       # the three sets of tests/test_guidance_modes_gpu.py
         "history": (0.625, 0.46, 1.4, 0.4),
         "last": (0.0, 1.0, 1.0, 0.0)}
APG = (2, 3.0, 0.0, 0.25, 1, 2.0, -0.5)                # mode, w, phi, eta, has_r, r, beta of md_guidance_prepare
STEPS, SOURCES, LAYOUTS = ("heun", "solver"), ("plain", "guide", "coef"), ("img", "tok")
SENTINEL = 7.0                  # what an output holds before the launch
BAD_ARG = -1


def entry_name(step, source, layout):
    return f"md_edm_{step}_update" + ("" if source == "plain" else "_" + source) + ("_tok" if layout == "tok" else "")


ENTRY_POINTS = [entry_name(s, src, lay) for s in STEPS for src in SOURCES for lay in LAYOUTS]


def pattern(n, salt):
    """n fp64 values in [-3, 3): ((i * 2654435761 + salt * 2654435769) mod 2^32) / 2^32 * 6 - 3.  Exact in fp64 (32 significant bits)."""
    i = torch.arange(n, dtype=torch.int64)
    h = (i * 2654435761 + salt * 2654435769) % (1 << 32)          # < 2^53 for every n used here: no wrap-around
    return h.double() / float(1 << 32) * 6.0 - 3.0


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


class Inputs:
    """Every operand of one shape, on `device`.  Token buffers carry 4 spare leading elements: tok_ptr(shift=True) is 8 bytes past a 16-byte
    boundary, the same values behind it."""

    def __init__(self, shape, device="cuda"):
        B, C, H, W = self.shape = shape
        self.T, self.pv, self.n = (H // P) * (W // P), C * P * P, B * C * H * W
        self.geo = (B, C, H, W, P)
        n, rows = self.n, B * self.T
        dev = lambda t: t.to(device)
        self.x_in, self.x_hat, self.state0 = (dev(pattern(n, s).view(shape)) for s in (1, 2, 3))
        self.F = dev(pattern(2 * n, 4).float().view(2 * B, C, H, W))             # the doubled batch: conditional, then unconditional
        self.F_guide = dev(pattern(n, 5).float().view(shape))
        self.M = dev(pattern(n, 6).float().view(shape))
        self.q = dev(pattern(n, 7).float().view(shape))
        self.coef = dev((pattern(2 * B, 8) / 3.0 + torch.tensor([1.0, 2.0]).double().repeat(B)).float().view(B, 2))
        self._tok = {}
        for name, salt, r in (("tok", 9, 2 * rows), ("tok_guide", 10, rows)):
            v = pattern(r * self.pv, salt).to(torch.bfloat16)
            for shift in (0, 4):
                buf = torch.zeros(r * self.pv + 4, dtype=torch.bfloat16)
                buf[shift:shift + v.numel()] = v
                self._tok[name, shift] = dev(buf)

    def tok_ptr(self, name="tok", shift=False):
        s = 4 if shift else 0
        return self._tok[name, s].data_ptr() + 2 * s

    def fresh(self, dtype=torch.float64):
        """An output buffer of the state's shape filled with the sentinel."""
        return torch.full(self.shape, SENTINEL, dtype=dtype, device=self.x_in.device)


def update_args(inp, step, source, layout, state, x_next, st, *, x_in=None, x_hat=None, has_uncond=1, second=0, coefs=COEFS["history"],
                t_in=T_IN, shift=()):
    """The arguments of one call of the entry point (step, source, layout).  state: d_cur (heun) / hist (solver), read and written in
    place.  shift: the token operands ("tok", "tok_guide") handed over 8 bytes off their 16-byte boundary."""
    B = inp.shape[0]
    x_in = inp.x_in if x_in is None else x_in
    x_hat = inp.x_hat if x_hat is None else x_hat
    tok = layout == "tok"
    ptrs = ([x_hat.data_ptr()] if step == "heun" else []) + [x_in.data_ptr()]
    ptrs.append(inp.tok_ptr("tok", "tok" in shift) if tok else inp.F.data_ptr())
    if source == "guide":
        ptrs.append(inp.tok_ptr("tok_guide", "tok_guide" in shift) if tok else inp.F_guide.data_ptr())
    if source == "coef":
        ptrs += [inp.M.data_ptr(), inp.coef.data_ptr()]
    ptrs += [state.data_ptr(), x_next.data_ptr()]
    size = inp.geo if tok else ((B, inp.n // B) if source == "coef" else (inp.n,))
    guide = {"plain": (CFG, has_uncond), "guide": (CFG,), "coef": ()}[source]
    tail = (t_in, T_HAT, T_NEXT, SD, second) if step == "heun" else (t_in, SD, *coefs)
    return (*ptrs, *size, *guide, *tail, st)


def launch_update(L, inp, step, source, layout, state, x_next, st, **kw):
    """One call; returns its code."""
    return getattr(L, entry_name(step, source, layout))(*update_args(inp, step, source, layout, state, x_next, st, **kw))


def _update_case(L, inp, st, step, source, layout, alias=None, **kw):
    state = inp.state0.clone()
    x_in, x_hat = inp.x_in.clone(), inp.x_hat.clone()
    x_next = {None: inp.fresh(), "x_in": x_in, "x_hat": x_hat}[alias]
    code = launch_update(L, inp, step, source, layout, state, x_next, st, x_in=x_in, x_hat=x_hat, **kw)
    assert code == 0, (entry_name(step, source, layout), kw, code)
    return {"x_next": x_next, "d_cur" if step == "heun" else "hist": state}


def _other_cases(L, inp, st):
    """The kernels that share the token geometry or the per-element arithmetic, once each."""
    B, n, rows, pv = inp.shape[0], inp.n, inp.shape[0] * inp.T, inp.pv
    dev = inp.x_in.device
    xp = inp.x_in.data_ptr()

    def prepare(tokens):
        M = inp.M.clone()
        coef, mom = torch.full((B, 2), SENTINEL, device=dev), torch.full((B, 5), SENTINEL, dtype=torch.float64, device=dev)
        if tokens:
            code = L.md_guidance_prepare_tok(xp, inp.tok_ptr(), inp.tok_ptr() + 2 * rows * pv, M.data_ptr(), coef.data_ptr(), mom.data_ptr(),
                                             *inp.geo, T_IN, SD, *APG, 0, st)
        else:
            code = L.md_guidance_prepare(xp, inp.F.data_ptr(), inp.F[B:].data_ptr(), M.data_ptr(), coef.data_ptr(), mom.data_ptr(), B, n // B,
                                         T_IN, SD, *APG, 0, st)
        assert code == 0, code
        return {"M": M, "coef": coef, "moments": mom}

    def denoised(tokens):
        D = inp.fresh(dtype=torch.float32)
        if tokens:
            code = L.md_edm_denoised_tok(xp, inp.tok_ptr(), D.data_ptr(), *inp.geo, CFG, 1, T_IN, SD, st)
        else:
            code = L.md_edm_denoised(xp, inp.F.data_ptr(), D.data_ptr(), B, n // B, CFG, 1, T_IN, SD, st)
        assert code == 0, code
        return {"D": D}

    def patchify():
        out = torch.full((2 * rows, pv), SENTINEL, dtype=torch.bfloat16, device=dev)
        assert L.md_edm_sampler_patchify(xp, out.data_ptr(), *inp.geo, T_IN, SD, 1, st) == 0
        return {"patches": out}

    def cotangent():
        out = torch.full((2 * rows, pv), SENTINEL, dtype=torch.bfloat16, device=dev)
        assert L.md_guide_cotangent_tok(inp.q.data_ptr(), out.data_ptr(), *inp.geo, CFG, 1, T_IN, SD, st) == 0
        return {"dtok": out}

    return {"md_guidance_prepare": lambda: prepare(False), "md_guidance_prepare_tok": lambda: prepare(True),
            "md_edm_denoised": lambda: denoised(False), "md_edm_denoised_tok": lambda: denoised(True),
            "md_edm_sampler_patchify": patchify, "md_guide_cotangent_tok": cotangent}


def cases(L, st, device="cuda"):
    """Yields (case id, thunk); the thunk launches and returns {buffer name: tensor}."""
    for si, shape in enumerate(SHAPES):
        inp = Inputs(shape, device)
        tag = "x".join(map(str, shape))

        def upd(step, source, layout, _inp=inp, **kw):
            return lambda: _update_case(L, _inp, st, step, source, layout, **kw)

        for source in SOURCES:
            for layout in LAYOUTS:
                for hu in ((0, 1) if source == "plain" else (None,)):
                    kw = {} if hu is None else {"has_uncond": hu}
                    suffix = "" if hu is None else f"-uncond{hu}"
                    for second in (0, 1):
                        yield f"{tag}/{entry_name('heun', source, layout)}{suffix}-second{second}", upd("heun", source, layout, second=second, **kw)
                    for cname, cf in COEFS.items():
                        yield f"{tag}/{entry_name('solver', source, layout)}{suffix}-{cname}", upd("solver", source, layout, coefs=cf, **kw)
        for name, thunk in _other_cases(L, inp, st).items():
            yield f"{tag}/{name}", thunk
        if si == 0:
            for layout in LAYOUTS:
                yield f"{tag}/alias-x_in/{entry_name('solver', 'plain', layout)}", upd("solver", "plain", layout, alias="x_in")
                yield f"{tag}/alias-x_hat/{entry_name('heun', 'plain', layout)}", upd("heun", "plain", layout, alias="x_hat")
            yield f"{tag}/shift8-tok/md_edm_heun_update_tok", upd("heun", "plain", "tok", shift=("tok",))
            yield f"{tag}/shift8-tok_guide/md_edm_solver_update_guide_tok", upd("solver", "guide", "tok", shift=("tok_guide",))
            yield f"{tag}/shift8-tok/md_edm_solver_update_coef_tok", upd("solver", "coef", "tok", shift=("tok",))


def compute(L, st, device="cuda"):
    """{case id: {buffer name: sha256 hex}} of every case, in case order."""
    out = {}
    for cid, thunk in cases(L, st, device):
        assert cid not in out, cid
        out[cid] = {k: digest(v) for k, v in thunk().items()}
    return out
