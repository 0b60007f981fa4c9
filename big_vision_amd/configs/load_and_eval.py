"""Load a model and evaluate it: the config that drives tools/eval_only.py.

Counterpart of big_vision/configs/load_and_eval.py for the accelerated hot path, written from its field values.  Same
top-level keys and defaults: the argument string selects a preset by `name` and sets `batch_size` (default 4);
`total_steps = 0`, `input = {batch_size, data = the dummy dataset of the init spec}`, `optax_name = "identity"`,
`lr = 0`, one `data` mesh axis, the fsdp sharding strategy for `params/.*`, the `act_batch` sharding rule; a preset
adds `num_classes`, `model_name`, `model`, `model_init` and its `evals`.  `eval_only = True` marks the config for tools
that tell a training config from this one.  There is no training section: no schedule, no `pp_train`, no weight decay.

Two more arguments, because tools/eval_only.py has no `--config.x` overrides: `variant` replaces the preset's ViT
variant and `model_init` names the checkpoint (a local .npz; empty = evaluate the random init, for testing).

  python -m big_vision.tools.eval_only --config big_vision_amd/configs/load_and_eval.py:name=vit_i1k,model_init=S16.npz --workdir /tmp/eval

Left out, and why:
  * `evals.fewshot` (`get_fewshot_lsr()`): the `fewshot_lsr` evaluator is not part of this package;
  * the presets `bit_paper` (the default name there) and `mlp_mixer_i1k`: `models.bit_paper` and `models.mlp_mixer` are
    not part of this package.  The default preset is `vit_i1k`; an unknown name is a KeyError that lists the presets;
  * `bit_paper`'s three evaluators with it.

Every entry of `evals` has a `type` that exists here: `classification`, `save`, `mean`.  Each preset gets, beside the
reference's classification entry, a `save_pred` entry that writes the pooled outputs (`collect=False`) of the same
split to `{workdir}/inference-{step:09d}.npz`.  `type="mean"` averages what a predict function returns per example; the
models' `apply` returns (logits, out), so an entry of that type selects a function handed to `eval_only.run(...,
predict_fns={...})` by `pred` - none is configured here.  `data` / `pp_fn` / `cache` stay what they are in the
reference: settings for its input pipeline, which is out of scope here; the evaluators consume in-memory `batches`.
"""
import big_vision.configs.common as bvcc

I1K_PP = ('decode|resize_small(256)|central_crop(224)|value_range(-1, 1)'
          '|onehot(1000, key="label", key_result="labels")|keep("image", "labels")')
I21K_PP = 'decode|resize_small(256)|central_crop(224)|value_range(-1, 1)|onehot(21843)|keep("image", "labels")'


def eval_only(config, batch_size, spec_for_init):
  """The fields that turn a trainer config into an evaluation-only one."""
  config.eval_only = True
  config.total_steps = 0
  config.input = dict(batch_size=batch_size, data=dict(name="bv:dummy", spec=spec_for_init))
  config.optax_name = "identity"
  config.lr = 0.0
  config.mesh = [("data", -1)]
  config.sharding_strategy = [("params/.*", 'fsdp(axis="data")')]
  config.sharding_rules = [("act_batch", ("data",))]
  return config


def _evals(data, pp_fn, loss_name):
  common = dict(data=data, pp_fn=pp_fn, cache="none")
  return dict(val=dict(common, type="classification", loss_name=loss_name),
              save_pred=dict(common, type="save", outfile="{workdir}/inference-{step:09d}.npz",
                             pred_kw=dict(collect=False)))


def vit_i1k(config):
  config.num_classes = 1000
  config.model_name = "vit"
  config.model = dict(variant="S/16", pool_type="gap", posemb="sincos2d", rep_size=True)
  config.evals = _evals(dict(name="imagenet2012", split="validation"), I1K_PP, "softmax_xent")


def vit_i21k(config):
  config.num_classes = 21843
  config.model_name = "vit"
  config.model = dict(variant="B/32", pool_type="tok")
  config.evals = _evals(dict(name="imagenet21k", split="full[:51200]"), I21K_PP, "sigmoid_xent")


PRESETS = {"vit_i1k": vit_i1k, "vit_i21k": vit_i21k}


def get_config(arg=""):
  config = bvcc.parse_arg(arg, name="vit_i1k", batch_size=4, variant="", model_init="")
  variant = config.variant
  del config["variant"]
  eval_only(config, config.batch_size, spec_for_init=dict(image=dict(shape=(224, 224, 3), dtype="float32")))
  if config.name not in PRESETS:
    raise KeyError(f"load_and_eval: no preset '{config.name}' (presets: {sorted(PRESETS)})")
  PRESETS[config.name](config)
  if variant:
    config.model.variant = variant
  return config
