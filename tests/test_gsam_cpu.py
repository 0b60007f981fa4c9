"""The GSAM / SAM trainer (`trainers.proj.gsam`) without a GPU: config, alias paths, the host arithmetic of the step
against an fp64 restatement of big_vision/trainers/proj/gsam/gsam.py:69-122, and the refusals."""
import importlib
import math
import os

import pytest
import torch

REFERENCE = os.environ.get("BV_REFERENCE_ROOT", "/root/reference")
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = f"{HERE}/big_vision_amd/configs/proj/gsam/vit_i1k_gsam_no_aug.py"
TINY = dict(width=128, depth=2, mlp_dim=256, num_heads=2, patch_size=(16, 16), pool_type="gap")


def _cfg(**kw):
  from big_vision_amd.compat.ml_collections import ConfigDict
  c = ConfigDict()
  c.lr, c.wd = 1e-3, 1e-4
  c.schedule = dict(warmup_steps=2, decay_type="linear", linear_end=0.01)
  c.optax_name = "scale_by_adam"
  c.grad_clip_norm = 1.0
  c.total_steps = 10
  c.model_name = "vit"
  c.model = dict(TINY)
  c.num_classes = 24
  c.gsam = dict(rho_max=0.6, rho_min=0.1, alpha=0.6, lr_max=1e-3, lr_min=1e-5)
  for k, v in kw.items():
    c[k] = v
  return c


def _plain(x):
  if hasattr(x, "to_dict"):
    x = x.to_dict()
  if isinstance(x, dict):
    return {k: _plain(v) for k, v in x.items()}
  if isinstance(x, (list, tuple)):
    return [_plain(v) for v in x]
  return x


# ------------------------------------------------------------------------------------------------ config, alias --
def test_alias_paths_are_the_same_modules():
  from big_vision_amd.trainers.proj.gsam import gsam, train
  assert importlib.import_module("big_vision.trainers.proj.gsam.gsam") is gsam
  assert importlib.import_module("big_vision.trainers.proj.gsam.train") is train
  mod = importlib.import_module("big_vision.configs.proj.gsam.vit_i1k_gsam_no_aug")
  assert mod is importlib.import_module("big_vision_amd.configs.proj.gsam.vit_i1k_gsam_no_aug")
  for name in ("get_model", "make_train_state", "make_update_fn", "make_grad_fn", "make_predict_fn", "check_finite",
               "load_init"):
    assert callable(getattr(train, name)), name
  from big_vision_amd import train as bv_train
  assert train.get_model is bv_train.get_model and train.check_finite is bv_train.check_finite
  assert train.make_predict_fn is bv_train.make_predict_fn and train.load_init is bv_train.load_init


def test_config_loads_and_gsam_tracks_lr_and_linear_end():
  from big_vision_amd.configs.loader import load_config
  c = load_config(CONFIG)
  assert c.model_name == "vit" and _plain(c.model) == dict(variant="B/32", rep_size=False, pool_type="gap")
  assert (c.loss, c.num_classes, c.init_head_bias, c.grad_clip_norm) == ("sigmoid_xent", 1000, -10.0, 1.0)
  assert (c.optax_name, _plain(c.optax), c.lr, c.wd) == ("scale_by_adam", dict(mu_dtype="float32"), 0.003, 0.001)
  assert _plain(c.schedule) == dict(warmup_steps=10_000, decay_type="linear", linear_end=0.01)
  assert _plain(c.gsam) == dict(rho_max=0.6, rho_min=0.1, alpha=0.6, lr_max=0.003, lr_min=0.01 * 0.003)
  c.lr = 0.01
  assert c.gsam.lr_max == 0.01 and c.gsam.lr_min == 0.01 * 0.01
  c.schedule.linear_end = 0.1
  assert c.gsam.lr_max == 0.01 and c.gsam.lr_min == 0.1 * 0.01
  assert dict(**c.gsam)["lr_min"] == 0.1 * 0.01            # what `**config.gsam` hands to gsam_gradient
  assert load_config(CONFIG + ":variant=S/16").model.variant == "S/16"


@pytest.mark.skipif(not os.path.isdir(f"{REFERENCE}/big_vision/configs"), reason="needs the reference checkout")
def test_fresh_config_equals_the_reference_config():
  from big_vision_amd.configs.loader import load_config
  from big_vision_amd.trainers.proj.gsam import train
  ref = load_config(f"{REFERENCE}/big_vision/configs/proj/gsam/vit_i1k_gsam_no_aug.py", reference_root=REFERENCE)
  ours = load_config(CONFIG)
  r, o = _plain(ref), _plain(ours)
  r.pop("fewshot")                       # the fewshot_lsr evaluator is not provided here: left out of the fresh file
  assert r == o, {k: (r.get(k), o.get(k)) for k in set(r) | set(o) if r.get(k) != o.get(k)}
  for cfg in (ref, ours):                # either file drives the model registry and passes the trainer's checks
    cfg.lr = 0.001                       # ... and ties gsam's end points to lr in both
    assert cfg.gsam.lr_max == 0.001 and cfg.gsam.lr_min == cfg.schedule.linear_end * 0.001
    _, model = train.get_model(cfg)
    assert (model.width, model.depth, model.pool_type, model.num_classes) == (768, 12, "gap", 1000)
    kw = train.check_config(cfg)
    assert kw == dict(rho_max=0.6, rho_min=0.1, alpha=0.6, lr_max=0.001, lr_min=1e-5, eps=1e-12, minimize_fp=True)
    train.make_update_fn(model, cfg)


# --------------------------------------------------------------------- the host arithmetic vs the reference's --
def _dual_vector(y):
  """gsam.py:19-27 on a list of fp64 leaves."""
  norm = torch.sqrt(sum(torch.sum(torch.square(e)) for e in y))
  return [e / norm for e in y], norm


def _reference_gsam(params, g_clean, g_robust, *, rho_max, rho_min, alpha, lr, lr_max, lr_min, eps=1e-12,
                    minimize_fp=True):
  """fp64 restatement of gsam.py:69-122 with the two gradients GIVEN (lists of leaves): -> (param_sam, g_gsam)."""
  _, g_clean_length = _dual_vector(g_clean)
  if lr_max == lr_min:
    sam_rho = rho_max
  else:
    sam_rho = rho_min + (rho_max - rho_min) * (lr - lr_min) / (lr_max - lr_min)
  param_sam = [a + sam_rho * b / (g_clean_length + eps) for a, b in zip(params, g_clean)]
  if minimize_fp:
    g_robust_normalized, _ = _dual_vector(g_robust)
    proj = sum(torch.vdot(p.flatten(), q.flatten()) for p, q in zip(g_robust_normalized, g_clean))
    residual = [a - proj * b for a, b in zip(g_clean, g_robust_normalized)]
    g_gsam = [a - b * alpha for a, b in zip(g_robust, residual)]
  else:
    g_clean_normalized, _ = _dual_vector(g_clean)
    proj = sum(torch.vdot(p.flatten(), q.flatten()) for p, q in zip(g_clean_normalized, g_robust))
    residual = [a - proj * b for a, b in zip(g_robust, g_clean_normalized)]
    g_gsam = [a + b * alpha for a, b in zip(g_clean, residual)]
  return param_sam, g_gsam


def _vectors(seed):
  g = torch.Generator().manual_seed(seed)
  shapes = [(37, 53), (1024,), (3, 7, 11), (1,)]
  params = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
  g_clean = [torch.randn(s, generator=g, dtype=torch.float64) * 1e-2 for s in shapes]
  # near-parallel gradients, as the two passes of one step give
  g_robust = [c * 1.3 + torch.randn(c.shape, generator=g, dtype=torch.float64) * 2e-3 for c in g_clean]
  return params, g_clean, g_robust


RTOL = 1e-12      # fp64 on both sides


def _product(params, g_clean, g_robust, *, lr, **kw):
  """The trainer's host functions on the same flat fp64 vectors: -> (param_sam, g_gsam, a, b)."""
  from big_vision_amd.trainers.proj.gsam import gsam
  hp = gsam.hparams(**kw)
  p, gc, gr = (torch.cat([t.flatten() for t in ts]) for ts in (params, g_clean, g_robust))
  rho = gsam.sam_rho(lr, hp["rho_max"], hp["rho_min"], hp["lr_max"], hp["lr_min"])
  c = gsam.perturbation_scale(rho, (gc * gc).sum().item(), hp["eps"])
  a, b = gsam.combine_coefficients(hp["alpha"], hp["minimize_fp"], (gr * gc).sum().item(), (gr * gr).sum().item(),
                                   (gc * gc).sum().item())
  return p + c * gc, a * gr + b * gc, a, b, (a * gr).abs() + (b * gc).abs()


@pytest.mark.parametrize("minimize_fp", [True, False])
@pytest.mark.parametrize("case", ["gsam", "alpha0", "sam", "lr_max_eq_lr_min", "lr_at_ends"])
def test_host_arithmetic_matches_the_reference_formulas(case, minimize_fp):
  kw = dict(rho_max=0.6, rho_min=0.1, alpha=0.6, lr_max=3e-3, lr_min=3e-5, minimize_fp=minimize_fp)
  lrs = [1.2e-3]
  if case == "alpha0":
    kw.update(alpha=0.0)
  elif case == "sam":
    kw.update(alpha=0.0, rho_max=0.3, rho_min=0.3)
  elif case == "lr_max_eq_lr_min":
    kw.update(lr_max=3e-3, lr_min=3e-3)
  elif case == "lr_at_ends":
    lrs = [3e-3, 3e-5, 0.0]
    kw.update(eps=1e-6)
  params, g_clean, g_robust = _vectors(11)
  for lr in lrs:
    p_ref, g_ref = _reference_gsam(params, g_clean, g_robust, lr=lr, **kw)
    p_ref, g_ref = (torch.cat([t.flatten() for t in ts]) for ts in (p_ref, g_ref))
    p_sam, g_gsam, a, b, terms = _product(params, g_clean, g_robust, lr=lr, **kw)
    p0, gc = (torch.cat([t.flatten() for t in ts]) for ts in (params, g_clean))
    assert ((p_sam - p_ref).abs() <= RTOL * (p0.abs() + (p_sam - p0).abs())).all()
    assert ((g_gsam - g_ref).abs() <= RTOL * terms).all(), ((g_gsam - g_ref).abs() / terms).max()
    # the perturbation has length sam_rho (up to eps)
    from big_vision_amd.trainers.proj.gsam import gsam
    rho = gsam.sam_rho(lr, kw["rho_max"], kw["rho_min"], kw["lr_max"], kw["lr_min"])
    assert abs((p_sam - p0).norm().item() - rho) <= 1e-4 * abs(rho) + 1e-15
    gr = torch.cat([t.flatten() for t in g_robust])
    if kw["alpha"] == 0.0:       # SAM (minimize_fp) / plain training (otherwise): EXACTLY one of the two gradients
      assert torch.equal(g_gsam, gr if minimize_fp else gc)
      assert (a, b) == ((1.0, -0.0) if minimize_fp else (0.0, 1.0))


def test_sam_rho_schedule():
  from big_vision_amd.trainers.proj.gsam import gsam
  kw = dict(rho_max=0.6, rho_min=0.1, lr_max=3e-3, lr_min=3e-5)
  assert gsam.sam_rho(3e-3, **kw) == pytest.approx(0.6, rel=RTOL)
  assert gsam.sam_rho(3e-5, **kw) == pytest.approx(0.1, rel=RTOL)
  mid = gsam.sam_rho(0.5 * (3e-3 + 3e-5), **kw)
  assert mid == pytest.approx(0.35, rel=RTOL) and 0.1 < mid < 0.6
  # warm-up: lr below lr_min extrapolates, as in the reference (no clamp)
  assert gsam.sam_rho(0.0, **kw) == pytest.approx(0.1 + 0.5 * (0.0 - 3e-5) / (3e-3 - 3e-5), rel=RTOL)
  # lr_max == lr_min: rho_max whatever lr is; rho_max == rho_min: that value on both sides of the branch
  assert gsam.sam_rho(1.0, rho_max=0.6, rho_min=0.1, lr_max=2e-3, lr_min=2e-3) == 0.6
  assert gsam.sam_rho(7e-4, rho_max=0.3, rho_min=0.3, lr_max=3e-3, lr_min=3e-5) == 0.3
  assert gsam.sam_rho(7e-4, rho_max=0.3, rho_min=0.3, lr_max=3e-3, lr_min=3e-3) == 0.3


# ----------------------------------------------------------------------------------------------------- refusals --
def _model(config):
  from big_vision_amd.trainers.proj.gsam import train
  return train.get_model(config)[1]


def test_adaptive_perturbation_is_refused_by_name():
  from big_vision_amd.trainers.proj.gsam import train
  config = _cfg()
  config.gsam.adaptive_perturbation = True
  with pytest.raises(NotImplementedError, match=r"gsam\.py:78-80") as e:
    train.make_update_fn(_model(config), config)
  assert "element-wise" in str(e.value) and "entry point" in str(e.value)
  config.gsam.adaptive_perturbation = False        # stated and off: accepted
  train.make_update_fn(_model(config), config)


def test_unknown_and_missing_gsam_keys_are_type_errors():
  from big_vision_amd.trainers.proj.gsam import train
  config = _cfg()
  config.gsam.rho = 0.3
  with pytest.raises(TypeError, match="rho"):
    train.make_update_fn(_model(config), config)
  config = _cfg()
  del config.gsam["lr_min"]
  with pytest.raises(TypeError, match="lr_min"):
    train.make_update_fn(_model(config), config)
  config = _cfg()
  config.gsam.update(eps=1e-8, minimize_fp=False)   # every honoured key
  assert train.check_config(config) == dict(rho_max=0.6, rho_min=0.1, alpha=0.6, lr_max=1e-3, lr_min=1e-5, eps=1e-8,
                                            minimize_fp=False)


def test_grad_accum_steps_raises_the_reference_assertion():
  from big_vision_amd.trainers.proj.gsam import train
  config = _cfg(grad_accum_steps=2)
  with pytest.raises(AssertionError, match="Grad-acc not supported anymore"):
    train.make_update_fn(_model(config), config)
  train.make_update_fn(_model(_cfg(grad_accum_steps=0)), _cfg(grad_accum_steps=0))


def test_more_than_one_schedule_is_refused():
  from big_vision_amd.trainers.proj.gsam import train
  sched = dict(warmup_steps=2, decay_type="cosine")
  config = _cfg(schedule=[("head/.*", dict(sched, mult=2.0)), (".*", sched)])
  with pytest.raises(AssertionError, match="one global learning-rate"):
    train.make_update_fn(_model(config), config)
  config = _cfg(schedule=[("head/.*", None), (".*", sched)])      # a frozen group is no schedule
  train.make_update_fn(_model(config), config)


def test_no_cpu_fallback(monkeypatch):
  """The vector stage is libbvhip or nothing: CPU tensors raise, and so does a library that is not built."""
  from big_vision_amd import _lib
  from big_vision_amd.trainers.proj.gsam import gsam
  x, y, eye = torch.ones(128), torch.ones(128), torch.eye(64)
  with pytest.raises(RuntimeError, match="GPU"):
    gsam.axpby_(y, 1.0, x, 0.5, eye)
  assert torch.equal(y, torch.ones(128))
  hip = _lib.LIBRARIES["hip"]
  monkeypatch.setattr(_lib, "_owner", {})
  monkeypatch.setattr(hip, "dll", None)
  monkeypatch.setattr(hip, "path", os.path.join(os.path.dirname(hip.path), "no_such_libbvhip.so"))
  with pytest.raises(RuntimeError, match="no CPU/eager fallback"):
    _lib.call("bv_sgemm_strided")


def test_axpby_row_ranges_fit_the_launch_grid():
  """bv_sgemm_strided launches ceil(M / 64) (VALU kernel) or ceil(M / 128) workgroups along gridDim.y, which ends at
  65535; the flat buffers are whole 1024-element chunks, so they split into rows of 64."""
  from big_vision_amd.params import ALIGN
  from big_vision_amd.trainers.proj.gsam import gsam
  assert (gsam.AXPBY_ROWS + 63) // 64 <= 65535 and ALIGN % gsam.AXPBY_COLS == 0
  assert gsam.AXPBY_ROWS * gsam.AXPBY_COLS % ALIGN == 0 and gsam.AXPBY_ROWS < 2 ** 31
