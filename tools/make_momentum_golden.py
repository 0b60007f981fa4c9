"""Golden fixtures of the SGD-momentum / SGD optimizers and the transfer configs, from the reference's own code.

  python tools/make_momentum_golden.py [out_dir]          (default tests/golden/)

Drives oracle/run_reference_optax.py as a module (its stand-ins, its `run_case`) with the cases below added to its
CASES table in memory, so `big_vision/optax.py::make` of the reference builds the chain with
`optax_name="big_vision.momentum_hp"` (optax.py:219-226: optax.trace) exactly as for the committed refoptax_* cases:

  refmomentum_<case>.npz         the layout of refoptax_<case>.npz (initial parameters, gradients, updates, final state)
  refmomentum_state_names.json   names and shapes of the state `make` builds for a two-tower and a classification ViT tree
  transfer_configs.json          configs/transfer.py resolved by big_vision_amd/configs/loader.py (settings only)

The stand-ins evaluate `decay * trace` in float64 (oracle/refshim/optax/__init__.py: trace).  Under real JAX a Python
float times a bf16 trace is weakly typed, so that product is probably rounded to bf16 before the add: one bf16 rounding
of one term, inside the tolerance the GPU tests allow for a bf16 accumulator.  JAX is not available to check it.
"""
import importlib.util
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REFERENCE = os.environ.get("BV_REFERENCE_ROOT", "/root/reference")

MOMENTUM_CASES = {
    # configs/transfer.py:149-152 with its cosine-with-warmup schedule: bf16 trace, momentum 0.9, clip 1.0, no wd
    "transfer": dict(lr=0.01, grad_clip_norm=1.0, wd=None, optax_name="big_vision.momentum_hp",
                     schedule=dict(decay_type="cosine", warmup_steps=2)),
    # every argument moved: fp32 trace, nesterov, momentum 0.8, decoupled wd and lr_mults
    "nesterov_f32": dict(lr=0.03, wd=1e-3, grad_clip_norm=0.5, optax_name="big_vision.momentum_hp",
                         optax=dict(momentum=0.8, dtype="float32", nesterov=True),
                         schedule=dict(decay_type="linear", warmup_steps=1, linear_end=0.1),
                         lr_mults=[("txt/head/.*", 2.0), (".*/bias", 0.5), (".*", 1.0)]),
    # a frozen group, two live schedules, BiT-style wd (configs/bit_i1k.py:64-70: (1e-4 / 256) * batch size)
    "frozen_bit": dict(lr=0.03, wd=(1e-4 / 256) * 512, optax_name="big_vision.momentum_hp",
                       schedule=[("img/embedding/.*", None),
                                 ("txt/.*", dict(decay_type="cosine", warmup_steps=1, mult=0.5)),
                                 (".*", dict(decay_type="cosine", warmup_steps=2))]),
}

MODEL_STATE_CASES = {
    "two_map_last_bias/momentum_hp": ("refwiring_two_map_last_bias", dict(
        lr=0.01, grad_clip_norm=1.0, wd=None, optax_name="big_vision.momentum_hp",
        schedule=dict(decay_type="cosine", warmup_steps=1))),
    "two_map_last_bias/momentum_hp_frozen_img": ("refwiring_two_map_last_bias", dict(
        lr=0.01, optax_name="big_vision.momentum_hp", optax=dict(dtype="float32"),
        schedule=[("img/.*", None), (".*", dict(decay_type="cosine"))])),
    "two_map_last_bias/sgd": ("refwiring_two_map_last_bias", dict(
        lr=0.01, wd=1e-4, optax_name="big_vision.sgd", schedule=dict(decay_type="cosine"))),
    "vit_0/momentum_hp": ("refwiring_vit_0", dict(
        lr=0.01, grad_clip_norm=1.0, wd=None, optax_name="big_vision.momentum_hp",
        schedule=dict(decay_type="cosine", warmup_steps=1))),
}

TRANSFER_ARGS = ["model=vit-i21k-augreg-b/32,dataset=cifar10", "model=vit-s16,dataset=oxford_iiit_pet",
                 "model=vit-i21k-augreg-b/32,dataset=cifar10,fsdp=True"]


def _load_runner():
  spec = importlib.util.spec_from_file_location("run_reference_optax", os.path.join(REPO, "oracle", "run_reference_optax.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def _plain(v):
  """ConfigDict / tuples -> JSON-able plain values."""
  if hasattr(v, "to_dict"):
    v = v.to_dict()
  if isinstance(v, dict):
    return {str(k): _plain(x) for k, x in v.items()}
  if isinstance(v, (list, tuple)):
    return [_plain(x) for x in v]
  return v


def transfer_configs():
  """Settings of configs/transfer.py resolved by this repository's config loader (run before the runner's import
  isolation, which points `big_vision` at the reference)."""
  sys.path.insert(0, REPO)
  from big_vision_amd.configs.loader import load_config
  path = os.path.join(REFERENCE, "big_vision", "configs", "transfer.py")
  return {arg: _plain(load_config(f"{path}:{arg}", reference_root=REFERENCE)) for arg in TRANSFER_ARGS}


def model_state_names(RO):
  import numpy as np
  import big_vision.optax as bv_optax
  import big_vision.utils as u
  out = {}
  for name, (fixture, cfg) in MODEL_STATE_CASES.items():
    z = np.load(os.path.join(REPO, "tests", "golden", f"{fixture}.npz"))
    params = RO._nest({k[len("param/"):]: np.asarray(z[k], np.float64) for k in z.files if k.startswith("param/")})
    tx, _ = bv_optax.make(RO._config(cfg), params, sched_kw=dict(RO.SCHED_KW))
    flat = u.tree_flatten_with_names(tx.init(params))[0]
    out[name] = dict(fixture=fixture, config=cfg, state=[[k, list(np.shape(v))] for k, v in flat])
  return out


def main(out_dir=None):
  out_dir = out_dir or (sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden"))
  os.makedirs(out_dir, exist_ok=True)
  configs = transfer_configs()
  RO = _load_runner()
  RO.CASES.update(MOMENTUM_CASES)
  RO._isolate_imports()
  with tempfile.TemporaryDirectory() as tmp:
    for name in MOMENTUM_CASES:
      meta = RO.run_case(name, tmp)
      shutil.move(os.path.join(tmp, f"refoptax_{name}.npz"), os.path.join(out_dir, f"refmomentum_{name}.npz"))
      print(name, meta["count"], len(meta["state_names"]), "state leaves")
  with open(os.path.join(out_dir, "refmomentum_state_names.json"), "w") as f:
    json.dump(model_state_names(RO), f, indent=1, sort_keys=True)
  with open(os.path.join(out_dir, "transfer_configs.json"), "w") as f:
    json.dump(configs, f, indent=1, sort_keys=True)


if __name__ == "__main__":
  main()
