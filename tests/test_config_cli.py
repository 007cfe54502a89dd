"""Host-side surface: the reference's YAML configs parse unchanged (no hydra / omegaconf), overrides and ${}
interpolation behave like the reference CLI (README.md:34-50), every `_target_` maps to a native implementation, and
the repo's own stage configs carry the reference's values."""
import json
import os

import pytest
import yaml

from micro_diffusion_amd import config as mdcfg
from micro_diffusion_amd.trainer import LRSchedule, parse_batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The reference's configs/*.yaml as yaml.safe_load returns them (written by `python oracle/gen_golden.py configs`)
with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")) as _fh:
    REF = json.load(_fh)


def _flat(d, p=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flat(v, p + k + "."))
        else:
            out[p + k] = v
    return out


@pytest.mark.parametrize("name", ["res_256_pretrain", "res_256_finetune", "res_512_pretrain", "res_512_finetune"])
def test_stage_configs(name):
    cfg = mdcfg.load_config(os.path.join(ROOT, "configs"), name + ".yaml",
                            ["exp_name=run1", "model.train_mask_ratio=0.5", "dataset.train_batch_size=512"])
    assert cfg["trainer"]["run_name"] == "run1" and cfg["trainer"]["save_folder"] == "./trained_models/run1/"
    assert cfg["trainer"]["seed"] == 18 and cfg["model"]["train_mask_ratio"] == 0.5
    assert isinstance(cfg["optimizer"]["lr"], float)
    for k, v in _flat(cfg).items():
        if k.endswith("_target_"):
            assert v in mdcfg.TARGETS, f"unmapped _target_ {v}"
    # same values as the reference's YAML
    ref = mdcfg.coerce_numbers(REF[name])
    mine = mdcfg.coerce_numbers(yaml.safe_load(open(os.path.join(ROOT, "configs", name + ".yaml"))))
    fr, fm = _flat(ref), _flat(mine)
    diff = {k: (fr.get(k), fm.get(k)) for k in set(fr) | set(fm)
            if fr.get(k) != fm.get(k) and "image_monitor" not in k and "wandb" not in k}
    assert not diff, diff


def test_reference_yaml_parses_unchanged(tmp_path):
    assert sorted(REF) == ["res_256_finetune", "res_256_pretrain", "res_512_finetune", "res_512_pretrain"]
    for name, raw in REF.items():
        (tmp_path / (name + ".yaml")).write_text(yaml.safe_dump(raw))
        cfg = mdcfg.load_config(str(tmp_path), name + ".yaml", ["trainer.device_train_microbatch_size=128"])
        assert cfg["trainer"]["device_train_microbatch_size"] == 128
        assert cfg["callbacks"]["image_monitor"]["seed"] == cfg["seed"]
        assert mdcfg.locate(cfg["model"]["_target_"]).__name__ == "create_latent_diffusion"


def test_schedules_and_durations():
    assert parse_batches("2500ba") == 2500
    with pytest.raises(ValueError):
        parse_batches("3ep")
    s = LRSchedule.from_target("composer.optim.CosineAnnealingWithWarmupScheduler", t_max="250000ba", t_warmup="2500ba", alpha_f=0.33)
    assert s.factor(0) == 0.0 and abs(s.factor(2500) - 1.0) < 1e-12 and abs(s.factor(250000) - 0.33) < 1e-12
    c = LRSchedule.from_target("composer.optim.ConstantWithWarmupScheduler", t_max=100, t_warmup="500ba", alpha=1.0)
    assert c.factor(250) == 0.5 and c.factor(5000) == 1.0
    assert LRSchedule.from_target("composer.optim.ConstantScheduler", t_max=1, alpha=1.0).factor(7) == 1.0


def test_import_alias_and_factory_signature():
    import inspect
    from micro_diffusion.models.model import create_latent_diffusion
    from micro_diffusion.models import dit as zoo
    sig = inspect.signature(create_latent_diffusion)
    assert list(sig.parameters) == ["vae_name", "text_encoder_name", "dit_arch", "latent_res", "in_channels",
                                    "pos_interp_scale", "dtype", "precomputed_latents", "p_mean", "p_std", "train_mask_ratio"]
    assert all(hasattr(zoo, n) for n in ("DiT", "MicroDiT_XL_2", "MicroDiT_Tiny_2"))
