"""CLIPPO (`models.proj.clippo.one_tower`) without a GPU: module path, parameter tree, loader, config, input contract."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

from big_vision_amd.models import vit
from big_vision_amd.models.proj.clippo import one_tower

REFERENCE = os.environ.get("BV_REFERENCE_ROOT", "/root/reference")
TOWER = dict(width=64, depth=2, num_heads=2, mlp_dim=128, patch_size=(16, 16), pool_type="map")
HW = (3, 3)      # 48 x 48 pixels


def _cfg(**kw):
  from big_vision_amd.compat.ml_collections import ConfigDict
  return ConfigDict(dict(image_model="vit", image=dict(TOWER), out_dim=32, temperature_init=10.0, **kw))


def test_alias_path_is_the_same_module():
  assert importlib.import_module("big_vision.models.proj.clippo.one_tower") is one_tower
  from big_vision_amd.compat.ml_collections import ConfigDict
  from big_vision_amd.trainers.proj.image_text import contrastive
  mod, model = contrastive.get_model(ConfigDict(dict(model_name="proj.clippo.one_tower", model=_cfg().to_dict())))
  assert mod is one_tower and isinstance(model, one_tower.Model)


@pytest.mark.parametrize("pool", ["map", "gap", "tok"])
def test_parameter_names_are_the_towers_plus_t(pool):
  cfg = dict(TOWER, pool_type=pool)
  model = one_tower.Model(image=cfg, out_dim=32)
  ours = [leaf for e in model.entries("", HW) for leaf, _ in e.flax_leaves()]
  tower = [leaf for e in vit.Model(num_classes=32, **cfg).entries("", HW) for leaf, _ in e.flax_leaves()]
  assert sorted(ours) == sorted([f"img/{k}" for k in tower] + ["t"])
  assert "b" not in ours and not any(k.startswith("txt/") for k in ours)
  assert "img/head/kernel" in ours                      # num_classes = out_dim: the tower carries the projection
  assert model.leaf_names((4, 48, 48, 3), (4, 48, 48, 3)) == model.leaf_names((4, 48, 48, 3))
  assert model.bias_init is None


def test_temperature_init_is_log_10():
  model = one_tower.Model(image=TOWER, out_dim=32)           # temperature_init defaults to 10 (one_tower.py:32)
  (t,) = [e for e in model.entries("", HW) if e.name == "t"]
  assert tuple(t.shape) == (1,)
  value = t.init(torch.Generator().manual_seed(0), (1,))
  assert abs(value.item() - math.log(10.0)) < 1e-6
  assert abs(one_tower.Model(image=TOWER, temperature_init=3.0).entries("", HW)[-1].init(None, (1,)).item() - math.log(3.0)) < 1e-6


def _trees(seed):
  """(checkpoint, init tree) of the model's own shapes as nested numpy dicts, from two different seeds."""
  import bv_oracle as O
  from big_vision_amd import utils as u

  def one(seed, t):
    tower = O.init_vit(torch.Generator().manual_seed(seed), (48, 48), num_classes=32, head_zeroinit=False, **TOWER)
    return {"img": u.tree_map(lambda v: v.numpy(), tower), "t": np.full((1,), t, np.float32)}
  return one(seed, 1.25), one(seed + 1, math.log(10.0))


def _same(a, b):
  from big_vision_amd import utils as u
  fa, fb = dict(u.tree_flatten_with_names(a)[0]), dict(u.tree_flatten_with_names(b)[0])
  return fa.keys() == fb.keys() and all(np.array_equal(np.asarray(fa[k]), np.asarray(fb[k])) for k in fa)


def test_load_string_and_dict_forms(tmp_path):
  from big_vision_amd import utils as u
  ckpt, init = _trees(3)
  path = str(tmp_path / "clippo.npz")
  u.save_params_npz(path, ckpt)
  tower_path = str(tmp_path / "tower.npz")
  u.save_params_npz(tower_path, ckpt["img"])
  cfg = _cfg()
  # one file: its img and t sub-trees
  got = one_tower.load(init, path, cfg)
  assert set(got) == {"img", "t"} and _same(got, ckpt)
  # dict forms, both spellings of every key; a part without an init file keeps its init value
  for img_key, t_key in (("image", "temperature"), ("img", "t")):
    got = one_tower.load(init, {img_key: tower_path, t_key: f"{path}:t"}, cfg)
    assert _same(got, ckpt)
  got = one_tower.load(init, {"image": f"{path}:img"}, cfg)
  assert _same(got["img"], ckpt["img"]) and np.array_equal(got["t"], init["t"])
  got = one_tower.load(init, {"t": f"{path}:t"}, cfg)
  assert _same(got["img"], init["img"]) and np.array_equal(got["t"], ckpt["t"])
  # img_load_kw goes to models.vit.load: the head keeps its init value
  got = one_tower.load(init, {"image": tower_path}, cfg, img_load_kw={"dont_load": ["^head/.*"]})
  assert np.array_equal(got["img"]["head"]["kernel"], init["img"]["head"]["kernel"])
  assert np.array_equal(got["img"]["embedding"]["kernel"], ckpt["img"]["embedding"]["kernel"])
  assert _same(init, _trees(3)[1]), "load() changed init_params"


def test_load_refuses_leftover_keys_and_remote_names(tmp_path):
  from big_vision_amd import utils as u
  ckpt, init = _trees(5)
  path = str(tmp_path / "clippo.npz")
  u.save_params_npz(path, ckpt)
  with pytest.raises(AssertionError, match=r"unused left in `config.model_init`.*'txt'"):
    one_tower.load(init, {"img": f"{path}:img", "txt": f"{path}:img"}, _cfg())
  with pytest.raises(AssertionError, match=r"'bias'"):
    one_tower.load(init, {"bias": path}, _cfg())
  # the reference config's own init: a vanity name of the tower, a gs:// path - refused, never fetched
  with pytest.raises(FileNotFoundError, match="remote checkpoints cannot be opened"):
    one_tower.load(init, {"image": "howto-i21k-B/16"}, _cfg())
  with pytest.raises(FileNotFoundError, match="remote checkpoints cannot be opened"):
    one_tower.load(init, {"t": "gs://bucket/ckpt.npz:t"}, _cfg())


def test_a_non_image_text_raises():
  model = one_tower.Model(image=TOWER, out_dim=32)
  image = torch.zeros((2, 48, 48, 3))
  for bad in (torch.zeros((2, 16), dtype=torch.int32), torch.zeros((2, 48, 48, 3), dtype=torch.int32),
              torch.zeros((2, 48, 48)), np.zeros((2, 48, 48, 3), np.float32)):
    with pytest.raises(ValueError, match=r"float32 tensor of shape \[n, H, W, 3\]"):
      model.apply({"params": {}}, image, bad)
  with pytest.raises(ValueError, match="share one shape"):
    model.leaf_names((2, 48, 48, 3), (2, 16))
  with pytest.raises(ValueError, match="share one shape"):
    model.leaf_names((2, 48, 48, 3), (2, 64, 64, 3))


def test_sigmoid_losses_need_a_bias_parameter():
  from big_vision_amd.compat.ml_collections import ConfigDict
  from big_vision_amd.trainers.proj.image_text import contrastive
  model = one_tower.Model(image=TOWER, out_dim=32)
  for name in ("sigmoid", "chunked_sigmoid"):
    with pytest.raises(ValueError, match="bias parameter"):
      contrastive.make_update_fn(model, ConfigDict(dict(loss_fn=name)))


def _plain(x):
  if hasattr(x, "to_dict"):
    x = x.to_dict()
  if isinstance(x, dict):
    return {k: _plain(v) for k, v in x.items()}
  if isinstance(x, (list, tuple)):
    return [_plain(v) for v in x]
  return x


def _diff(ref, ours, path=""):
  """Every field of `ref` that `ours` lacks or holds another value for."""
  if isinstance(ref, dict):
    if not isinstance(ours, dict):
      return [f"{path}: {ours!r} != {ref!r}"]
    return [d for k, v in ref.items()
            for d in (_diff(v, ours[k], f"{path}/{k}") if k in ours else [f"{path}/{k}: missing"])]
  return [] if ref == ours else [f"{path}: {ours!r} != {ref!r}"]


@pytest.mark.skipif(not os.path.isdir(f"{REFERENCE}/big_vision/configs"), reason="needs the reference checkout")
@pytest.mark.parametrize("arg", ["", "runlocal", "i1k_eval=True,res=256"])
def test_fresh_config_equals_the_reference_config(arg):
  from big_vision_amd.configs.loader import load_config
  from big_vision_amd.trainers.proj.image_text import contrastive
  sfx = f":{arg}" if arg else ""
  ref = load_config(f"{REFERENCE}/big_vision/configs/proj/clippo/train_clippo.py{sfx}", reference_root=REFERENCE)
  here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  ours = load_config(f"{here}/big_vision_amd/configs/proj/clippo/train_clippo.py{sfx}")
  assert ref.model_name == "proj.clippo.one_tower"
  assert _diff(_plain(ref), _plain(ours)) == []
  extra = set(_plain(ours)) - set(_plain(ref))
  assert extra == {"init_shapes", "init_types"}, extra       # the tensors the step consumes, stated here only
  assert set(ours.evals.keys()) == set(ref.evals.keys())
  for cfg in (ref, ours):     # either file drives the model registry
    mod, model = contrastive.get_model(cfg)
    assert mod is one_tower and model.out_dim == 768 and model.temperature_init == 10.0
    tw = model.image_tower
    assert (tw.width, tw.depth, tw.pool_type, tw.head_zeroinit, tw.num_classes) == (768, 12, "map", False, 768)
