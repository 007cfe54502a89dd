"""Cross-attention maps without a GPU: the policy and the refusals of attn_maps.AttentionMaps and
samplers.check_attn_maps, the read-out (per_block, maps, token_mass, mask) on a synthetic buffer, the three sampler signatures, and the
compiled resources of attn_probe.hip."""
import inspect
import os

import pytest
import torch

from oracle import microdit_ref as orc
from micro_diffusion_amd import attn_maps as am_mod
from micro_diffusion_amd import hip, native, samplers, sampling
from micro_diffusion_amd.attn_maps import AttentionMaps

HIPCC = "/opt/rocm/bin/hipcc"


def _cfg():
    from micro_diffusion_amd import dit as mdit
    return mdit.DiT(**orc.micro_config().__dict__).config


# ------------------------------------------------------------------------------------------------ constructor, selection, check
def test_block_names_and_selection():
    cfg = _cfg()
    names = am_mod.block_names(cfg)
    assert names == ["patch_mixer.0", "patch_mixer.1", "blocks.0", "blocks.1", "blocks.2", "blocks.3"]
    assert am_mod.select_blocks(names, None) == names
    assert am_mod.select_blocks(names, ["blocks.2", "patch_mixer.0"]) == ["patch_mixer.0", "blocks.2"]      # forward order
    assert am_mod.select_blocks(names, r"^blocks\.[01]$") == ["blocks.0", "blocks.1"]
    assert am_mod.select_blocks(names, "mixer") == ["patch_mixer.0", "patch_mixer.1"]
    am = AttentionMaps(blocks=("blocks.3",))
    assert am.resolve(cfg) == ["blocks.3"] and am.grid == (8, 8) and am.tokens == 64 and am.patch_size == 2
    assert am.counts == {"blocks.3": 0}


@pytest.mark.parametrize("blocks", [[], (), 5, [3], ["blocks.0", 1], "blocks.(", ])
def test_constructor_refuses_a_malformed_selection(blocks):
    with pytest.raises(ValueError):
        AttentionMaps(blocks=blocks)


@pytest.mark.parametrize("rng", [(2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf")), (1.0,), "ab", 3.0, (1.0, 2.0, 3.0), (True, 2.0)])
def test_constructor_refuses_a_bad_sigma_range(rng):
    with pytest.raises(ValueError, match="sigma_range"):
        AttentionMaps(sigma_range=rng)


def test_sigma_range_is_inclusive():
    am = AttentionMaps(sigma_range=(0.5, 2))
    assert am.sigma_range == (0.5, 2.0)
    assert am.wants(0.5) and am.wants(2.0) and am.wants(1.0) and not am.wants(0.49) and not am.wants(2.01)
    assert AttentionMaps().wants(1e9) and AttentionMaps(sigma_range=(1.0, 1.0)).wants(1.0)


def test_check_attn_maps_refusals():
    cfg = _cfg()
    assert samplers.check_attn_maps(None, cfg) is False
    assert samplers.check_attn_maps(AttentionMaps(), cfg) is True
    assert samplers.check_attn_maps(AttentionMaps(blocks="blocks"), None) is True          # no model yet: the type alone
    for bad in (object(), "blocks.0", 3, {"blocks": None}):
        with pytest.raises(ValueError, match="AttentionMaps"):
            samplers.check_attn_maps(bad, cfg)
    with pytest.raises(ValueError, match="selects no block"):
        samplers.check_attn_maps(AttentionMaps(blocks=r"blocks\.9"), cfg)
    with pytest.raises(ValueError, match="not a block"):
        samplers.check_attn_maps(AttentionMaps(blocks=["blocks.12"]), cfg)
    with pytest.raises(ValueError, match="selects no block"):
        AttentionMaps(blocks="nothing").resolve(cfg)
    with pytest.raises(ValueError, match="token grid"):
        AttentionMaps().resolve(cfg, grid=(4, 8))


def test_request_check_runs_the_attention_map_check_before_anything_else_happens():
    from types import SimpleNamespace
    cfg = _cfg()
    model = SimpleNamespace(edm_config=SimpleNamespace(S_churn=0.0), dit=SimpleNamespace(config=cfg))
    sampling.Request().check(model, None, 1.0)
    sampling.Request(attn_maps=AttentionMaps(blocks=["blocks.1"])).check(model, None, 3.0)
    with pytest.raises(ValueError, match="AttentionMaps"):
        sampling.Request(attn_maps=object()).check(model, None, 1.0)
    with pytest.raises(ValueError, match="selects no block"):
        sampling.Request(attn_maps=AttentionMaps(blocks="blocks.7")).check(model, (2, 4, 16, 16), 1.0)


def test_signatures_carry_attn_maps():
    from micro_diffusion_amd.model import LatentDiffusion
    for fn in (LatentDiffusion.edm_sampler_loop, LatentDiffusion.generate):
        p = inspect.signature(fn).parameters["attn_maps"]
        assert p.default is None
    assert sampling.Request().attn_maps is None
    assert "attn_maps" in {f.name for f in sampling.Request.__dataclass_fields__.values()}
    assert "md_attn_probs" in hip.exported_symbols()


def test_recorder_skips_unselected_blocks_and_inactive_evaluations_without_touching_the_gpu():
    am = AttentionMaps(blocks=["blocks.0"], sigma_range=(1.0, 2.0))
    am.resolve(_cfg())
    am.start_run()
    am.record("blocks.1", None, 2, 64, 77, None)            # not selected: returns before anything is touched
    am.begin_evaluation(5.0, 2)
    am.record("blocks.0", None, 2, 64, 77, None)            # outside sigma_range
    am.begin_evaluation(1.5, 2)
    am.skip_evaluation()
    am.record("blocks.0", None, 2, 64, 77, None)            # a guide's forward
    assert am.counts == {"blocks.0": 0} and am.buf is None
    with pytest.raises(RuntimeError, match="nothing has been recorded"):
        am.per_block()


# ------------------------------------------------------------------------------------------------ read-out on a synthetic buffer
B, LC, LDO, GRID, PS = 2, 5, 8, (4, 6), 2
NAMES = ["patch_mixer.0", "blocks.0", "blocks.1"]


def _synthetic():
    g = torch.Generator().manual_seed(5)
    T = GRID[0] * GRID[1]
    p = torch.softmax(torch.randn(len(NAMES), B, T, LC, generator=g) * 2, -1)
    counts = [3, 2, 0]
    buf = torch.full((len(NAMES), B, T, LDO), 9.0)          # pad columns hold garbage the read-out must not see
    for i, c in enumerate(counts):
        buf[i, :, :, :LC] = p[i] * c
    return AttentionMaps.from_buffer(NAMES, buf, counts, LC, GRID, PS), p


def test_per_block_maps_and_token_mass():
    am, p = _synthetic()
    pb = am.per_block()
    assert list(pb) == NAMES[:2], "a block that was never recorded is left out"
    for i, n in enumerate(NAMES[:2]):
        assert pb[n].shape == (B, LC, *GRID) and pb[n].dtype == torch.float32
        want = p[i].permute(0, 2, 1).reshape(B, LC, *GRID)
        torch.testing.assert_close(pb[n], want, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(pb[n].sum(1), torch.ones(B, *GRID), rtol=1e-5, atol=0)
    torch.testing.assert_close(am.maps(), (pb[NAMES[0]] + pb[NAMES[1]]) / 2, rtol=1e-6, atol=1e-7)
    assert torch.equal(am.maps(["blocks.0"]), pb["blocks.0"]) and torch.equal(am.maps("mixer"), pb["patch_mixer.0"])
    with pytest.raises(RuntimeError, match="recorded"):
        am.maps(["blocks.1"])
    with pytest.raises(ValueError):
        am.maps(["blocks.5"])
    tm = am.token_mass()
    assert tm.shape == (len(NAMES), LC) and tm.dtype == torch.float32
    torch.testing.assert_close(tm[:2].sum(1), torch.ones(2), rtol=1e-5, atol=0)
    torch.testing.assert_close(tm[:2], p[:2].mean(dim=(1, 2)), rtol=1e-5, atol=1e-7)
    assert torch.isnan(tm[2]).all()
    assert am.counts == {"patch_mixer.0": 3, "blocks.0": 2, "blocks.1": 0}


def _heat_recorder(heat):
    """A recorder with one block and one caption position of weight whose map is `heat` [B, h, w] (position 1 holds the rest)."""
    b, h, w = heat.shape
    buf = torch.zeros(1, b, h * w, 4)
    buf[0, :, :, 0] = heat.reshape(b, h * w)
    buf[0, :, :, 1] = 1 - heat.reshape(b, h * w)
    return AttentionMaps.from_buffer(["blocks.0"], buf, [1], 2, (h, w), PS)


def test_mask_shape_values_threshold_and_quantile():
    g = torch.Generator().manual_seed(7)
    heat = torch.rand(3, 5, 7, generator=g) * torch.tensor([0.9, 0.5, 0.1]).view(3, 1, 1)
    am = _heat_recorder(heat)
    m = am.mask(tokens=[0], threshold=0.6)
    assert m.shape == (3, 1, 5 * PS, 7 * PS) and m.dtype == torch.float32
    assert set(m.unique().tolist()) <= {0.0, 1.0}
    norm = heat / heat.flatten(1).max(1).values.view(3, 1, 1)               # per-sample maximum: the faint third sample is not empty
    cells = (norm >= 0.6).float()
    assert torch.equal(m, cells.unsqueeze(1).repeat_interleave(PS, 2).repeat_interleave(PS, 3))
    assert (m.flatten(1).sum(1) > 0).all()
    # every patch_size x patch_size cell is constant
    assert torch.equal(m.view(3, 1, 5, PS, 7, PS).amax(dim=(3, 5)), m.view(3, 1, 5, PS, 7, PS).amin(dim=(3, 5)))
    mq = am.mask(tokens=[0], quantile=0.75)
    kept = mq[:, 0, ::PS, ::PS].flatten(1).sum(1)
    assert ((kept >= 9) & (kept <= 10)).all(), kept                         # the top quarter of 35 cells, per sample
    level = torch.quantile(norm.flatten(1), 0.75, dim=1).view(3, 1, 1)
    assert torch.equal(mq[:, 0, ::PS, ::PS], (norm >= level).float())
    assert torch.equal(am.mask(tokens=[0], quantile=0.0), torch.ones_like(m))
    # several caption positions are summed: positions 0 and 1 together are flat, everything is selected
    assert torch.equal(am.mask(tokens=[0, 1], threshold=0.99), torch.ones_like(m))


def test_mask_dilates_by_exactly_the_given_number_of_cells():
    heat = torch.zeros(1, 9, 9)
    heat[0, 4, 4] = 1.0
    heat[0, 0, 8] = 0.95                                                    # a corner: the growth is clipped at the border
    am = _heat_recorder(heat)
    for d in (0, 1, 2):
        cells = am.mask(tokens=[0], threshold=0.9, dilate=d)[0, 0, ::PS, ::PS]
        want = torch.zeros(9, 9)
        want[4 - d:4 + d + 1, 4 - d:4 + d + 1] = 1
        want[0:d + 1, 8 - d:9] = 1
        assert torch.equal(cells, want), d


def test_mask_refuses_bad_criteria():
    am = _heat_recorder(torch.rand(1, 3, 3))
    for kw in ({}, {"quantile": 0.5, "threshold": 0.5}, {"quantile": 1.5}, {"threshold": -0.1}, {"threshold": 0.5, "dilate": -1},
               {"threshold": 0.5, "dilate": 1.5}, {"threshold": True}):
        with pytest.raises(ValueError):
            am.mask(tokens=[0], **kw)
    for tokens in ([], [2], [-1]):
        with pytest.raises(ValueError, match="tokens"):
            am.mask(tokens=tokens, threshold=0.5)


# ------------------------------------------------------------------------------------------------ compiled resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_attn_probe_kernels_have_no_spills_no_scratch_and_the_stated_lds(tmp_path):
    """The design (attn_probe.hip): two K buffers of 128 rows x (hd + 8) bf16 and nothing else in LDS."""
    res = native.resource_usage("attn_probe.hip", hip.HIPCC_FLAGS, tmp_path / "attn_probe.o")
    kernels = {32: [k for k in res if "attn_probs_kernelILi32E" in k], 64: [k for k in res if "attn_probs_kernelILi64E" in k]}
    assert len(res) == 2 and all(len(v) == 1 for v in kernels.values()), list(res)
    for hd, (name,) in kernels.items():
        v = res[name]
        assert v["spill"] == 0 and v["scratch"] == 0, (name, v)
        assert v["lds"] <= 2 * 128 * (hd + 8) * 2, (name, v)
        assert v["occ"] >= 3, (name, v)              # three workgroups of four waves per CU fit by registers and by LDS
