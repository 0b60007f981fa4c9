"""Loads a model and only runs evaluators: the offline evaluation of a finished checkpoint, without a training run.

Mirrors big_vision/tools/eval_only.py.  `run(config, workdir)` does what its `main` does, in its order:
  * a config that re-initialises part of the model (`config.model.reinit`) is refused (:69-70);
  * `big_vision.models.<config.model_name>` is imported and `Model(**config.model)` built, with `num_classes` from the
    config when it has one, so classification and image-text configs both work (:71-75);
  * the parameters are initialised with rng 42 for `config.init_shapes` (default `[(1, 224, 224, 3)]`, :80-89) through
    the models' host shell (models/common.py: `make_store`, then the shell's init) and counted as `num_params` (:92-93).
    `config.init_types` is accepted and checked against the number of shapes; no layout here depends on an input's
    dtype;
  * `config.model_init`, when set, goes through the model module's `load(params, model_init, config.model,
    **config.model_load)` into the store (:96-100; `train.load_init`, which also resolves a vanity name and refuses a
    remote or missing file before anything is read);
  * `predict_fn(params, *a, **kw) = model.apply({"params": params}, *a, **kw)`: the forward that saves no context
    (:107-108).  Evaluators here call `predict_fn(train_state, batch)` with the batch DICT, so a single mapping
    argument is spread over the model's inputs first (`image`; `image` and `labels` for an image-text pair, either may
    be absent);
  * `evaluators.common.from_config(config, {"predict": predict_fn, "model": model}, ...)` with a `get_steps` that
    ignores `log_steps` (:110-114), so a config that names an evaluator this package lacks fails there with
    ModuleNotFoundError;
  * for `s in range(config.eval_repeats)` (default 1) every evaluator runs on the bare parameters - there is no
    optimizer in the state - and `prefix + key` is recorded for step `s` (:119-129).

Returned: `{step: {name: value}}`, `num_params` in step 0.  With a `workdir`, one JSON line `{"step": s, ...}` per step
is appended to `<workdir>/big_vision_metrics.txt`, the file of the reference's metric writer, and evaluators with a
`workdir` attribute (save) that is not set get this one.

Two arguments stand in for what the reference takes from elsewhere.  `batches` ({evaluator name: iterable of batch
dicts}) is assigned to `evaluator.batches` after construction: this tree has no input pipeline, an evaluator consumes
in-memory batches, and an entry of `config.evals` may carry its `batches` itself.  `predict_fns` ({name: fn(params,
batch, **pred_kw)}) adds predict functions beside `predict` and `model` for `config.evals.<name>.pred` to select: the
reference offers those two alone, which serves `type="mean"` only for a model whose `apply` returns per-example
metrics, and no model here does.

One process, one device (`device`, default the current GPU); the timing measurements and the profiler hooks of the
reference are left out.

  python -m big_vision.tools.eval_only --config big_vision_amd/configs/load_and_eval.py:name=vit_i1k,model_init=ckpt.npz --workdir /tmp/eval
"""
import argparse
import importlib
import json
import logging
import os
import sys
from collections.abc import Mapping

from big_vision_amd import train
from big_vision_amd import utils as u
from big_vision_amd.evaluators import common as eval_common
from big_vision_amd.models import common as models_common

METRICS_FILE = "big_vision_metrics.txt"


def _nested(config, dotted):
  """config["a.b"] or None (the `config.get("a.b")` of ml_collections; the offline ConfigDict's `get` takes plain keys)."""
  node = config
  for part in dotted.split("."):
    if not hasattr(node, "keys") or part not in node.keys():
      return None
    node = node[part]
  return node


def _model_inputs(model, batch):
  """The positional inputs of `model.apply` in a batch dict."""
  if isinstance(model, models_common.Pair):
    return batch.get("image"), batch.get("labels")
  return (batch["image"],)


def _plain(value):
  return value.item() if hasattr(value, "item") else value


def run(config, workdir=None, batches=None, device=None, predict_fns=None):
  """Evaluates `config.model_init` with `config.evals`; see the module docstring."""
  write_note = lambda note: logging.info("NOTE: %s", note)

  write_note(f"Initializing {config.model_name} model...")
  assert _nested(config, "model.reinit") is None, "eval_only evaluates a checkpoint: config.model.reinit must not be set"
  model_mod = importlib.import_module(f"{models_common.MODELS_PKG}.{config.model_name}")
  model_kw = dict(config.get("model", {}))
  if "num_classes" in config:
    model_kw["num_classes"] = config.num_classes
  model = model_mod.Model(**model_kw)

  shapes = [tuple(s) for s in config.get("init_shapes", [(1, 224, 224, 3)])]
  types = config.get("init_types", ["float32"] * len(shapes))
  assert len(types) == len(shapes), f"config.init_types {types} does not match config.init_shapes {shapes}"
  store = model.make_store(*shapes, device=device)
  params = model._variables(store, 42)["params"]     # pylint: disable=protected-access
  num_params = sum(int(leaf.numel()) for _, leaf in u.tree_flatten_with_names(params)[0])

  if config.get("model_init"):
    write_note(f"Initialize model from {config.model_init}...")
    train.load_init(model, store, config.model_init, config.get("model"), dict(config.get("model_load", {})),
                    key="model_init")
    store.refresh_shadow()
    params = store.tree()

  def predict_fn(params, *a, **kw):
    if len(a) == 1 and isinstance(a[0], Mapping):
      a = _model_inputs(model, a[0])
    return model.apply({"params": params}, *a, **kw)

  # every predict function runs on config.residual_stream, like the trainers' (train.make_predict_fn)
  fns = {"predict": train.in_residual_stream(config, predict_fn), "model": model}
  for name, fn in (predict_fns or {}).items():
    assert name not in fns, f"predict_fns: '{name}' is taken"
    fns[name] = train.in_residual_stream(config, fn)
  evaluators = eval_common.from_config(
      config, fns, lambda s: write_note(f"Initializing evaluator: {s}..."),
      lambda key, cfg: 1)                              # log_steps is ignored: every evaluator runs at every step
  unknown = set(batches or {}) - {name for name, *_ in evaluators}
  if unknown:
    raise ValueError(f"batches for {sorted(unknown)}: config.evals has {[name for name, *_ in evaluators]}")
  for name, evaluator, _, _ in evaluators:
    if batches and name in batches:
      evaluator.batches = batches[name]
    if workdir is not None and getattr(evaluator, "workdir", "") is None:
      evaluator.workdir = workdir

  if workdir is not None:
    os.makedirs(workdir, exist_ok=True)
  results = {}
  for s in range(config.get("eval_repeats", 1)):
    measured = results.setdefault(s, {"num_params": num_params} if s == 0 else {})
    for name, evaluator, _, prefix in evaluators:
      write_note(f"{name} evaluation step {s}...")
      for key, value in evaluator.run(params):
        measured[f"{prefix}{key}"] = _plain(value)
    if workdir is not None:
      with open(os.path.join(workdir, METRICS_FILE), "a") as f:
        f.write(json.dumps({"step": s, **measured}) + "\n")
  write_note("Done!")
  return results


def main(argv=None):
  from big_vision_amd.configs import loader
  parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
  parser.add_argument("--config", required=True, metavar="FILE[:ARG]", help="config file and its argument string")
  parser.add_argument("--workdir", default=None, help="where big_vision_metrics.txt and the evaluators' files go")
  args = parser.parse_args(argv)
  logging.basicConfig(level=logging.INFO)
  results = run(loader.load_config(args.config), workdir=args.workdir)
  for step, measured in results.items():
    print(json.dumps({"step": step, **measured}))
  return results


if __name__ == "__main__":
  main(sys.argv[1:])
