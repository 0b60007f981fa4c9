"""Utils for evaluators in general: `from_config` of big_vision/evaluators/common.py:36-88.

Kept: the handling of `type` (defaults to the evaluator's name), `pred`, `pred_kw`, `prefix`, `skip_first`, the
`log_*` keys (through `get_steps`), the `batch_size` default chain (:60), the ValueError that lists the available
predict functions (:80-82), the returned `(name, evaluator, logsteps, prefix)` tuples, and that the evaluator module is
resolved by its `big_vision.evaluators.<type>` path (the alias package maps it onto this tree; a type that has no
implementation here raises ModuleNotFoundError).

Dropped: the `devices` argument and the `API` check that tells pmap- from jit-based evaluators (:64-75).  There is
one execution model here - kernels launched on the current device's stream - so there is nothing to tell apart and
no device list to hand on.  `_CacheablePartial` exists in the reference to keep jit caches warm; a
`functools.partial` does the same job without a cache to serve.
"""
import functools
import importlib

# what from_config itself consumes of an entry of config.evals (common.py:49-56); the rest is the evaluator's
GENERIC_KEYS = ("type", "pred", "pred_kw", "prefix", "skip_first")
LOG_KEYS = ("log_steps", "log_epochs", "log_examples", "log_percent")


def _steps_from_cfg(key, cfg):
  return cfg[f"{key}_steps"]


def _batch_size(cfg, config):
  """common.py:60: the evaluator's own value, else the config's, newest spelling first."""
  for value in (cfg.get("batch_size"), config.get("batch_size_eval"), config.get("input.batch_size")):
    if value:
      return value
  return config.get("batch_size")


def from_config(config, predict_fns, write_note=lambda s: s, get_steps=_steps_from_cfg):
  """[(name, evaluator, logsteps, prefix)] for the entries of `config.evals`, in their order."""
  built = []
  for name, spec in config.get("evals", {}).items():
    write_note(name)
    cfg = spec.to_dict() if hasattr(spec, "to_dict") else dict(spec)
    generic = {k: cfg.pop(k) for k in GENERIC_KEYS if k in cfg}
    logsteps = get_steps("log", cfg)                 # sees the log_* keys; they leave right after
    for k in LOG_KEYS:
      cfg.pop(k, None)
    cfg["batch_size"] = _batch_size(cfg, config)
    module = importlib.import_module(f"big_vision.evaluators.{generic.get('type', name)}")
    pred_key = generic.get("pred", "predict")
    if pred_key not in predict_fns:
      raise ValueError(f"Unknown predict_fn '{pred_key}'. Available predict_fns are:\n" + "\n".join(predict_fns))
    predict_fn = predict_fns[pred_key]
    if generic.get("pred_kw") is not None:
      predict_fn = functools.partial(predict_fn, **dict(generic["pred_kw"]))
    built.append((name, module.Evaluator(predict_fn, **cfg), logsteps, generic.get("prefix", f"{name}/")))
  return built
