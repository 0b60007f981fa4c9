"""ViT-B/32 on ImageNet-1k with GSAM (arXiv 2203.08065), no strong augmentation: the GSAM / SAM trainer's config.

Counterpart of big_vision/configs/proj/gsam/vit_i1k_gsam_no_aug.py for the accelerated hot path, written from its
field values: a run configured from either file builds the same model (`vit`, `variant` B/32, gap pooling, no
pre-logits, head bias -10), the same optimizer (Adam with fp32 first moment, clip norm 1, lr 0.003, wd 0.001), the
same linear schedule (10 k warm-up steps, down to 0.01 of the peak) and the same `gsam` section;
tests/test_gsam_cpu.py compares the two where a reference checkout is present.  Arguments as there: `variant`,
`runlocal`.

`gsam.lr_max` / `gsam.lr_min` are REFERENCES to `lr` and `schedule.linear_end * lr`: an override of either (a sweep,
`config.lr = ...` after loading) moves the rho schedule's end points with it.  rho_max == rho_min with alpha == 0 is
SAM.

The `pp_train` / `pp_fn` entries stay what they are in the reference: STRINGS for its input pipeline, which is out of
scope here; the step consumes `image` as float32 [n, 224, 224, 3] and one-hot `labels` [n, 1000].  The reference's
`fewshot` section names the `fewshot_lsr` evaluator, which this package does not provide, and is left out.

  big_vision.trainers.proj.gsam.train with --config big_vision/configs/proj/gsam/vit_i1k_gsam_no_aug.py
"""
import big_vision.configs.common as bvcc
from ml_collections import ConfigDict


def get_config(arg=None):
  arg = bvcc.parse_arg(arg, variant="B/32", runlocal=False)
  local = arg.runlocal
  c = ConfigDict()

  c.dataset = "imagenet2012"
  c.train_split = "train[:99%]"
  c.cache_raw = not local
  c.shuffle_buffer_size = 10 if local else 250_000
  c.num_classes = 1000
  c.loss = "sigmoid_xent"
  c.batch_size = 8 if local else 4096
  c.num_epochs = 300

  labels = lambda key: f'|value_range(-1, 1)|onehot(1000, key="{key}", key_result="labels")|keep("image", "labels")'
  c.pp_train = "decode_jpeg_and_inception_crop(224)|flip_lr|" + labels("label")     # (the empty stage is the reference's)
  pp_eval = lambda key: "decode|resize_small(256)|central_crop(224)" + labels(key)
  c.prefetch_to_host = 8
  c.prefetch_to_device = 4
  c.log_training_steps = 50
  c.checkpoint_steps = 1000

  c.model_name = "vit"
  c.model = dict(variant=arg.variant, rep_size=False, pool_type="gap")
  c.init_head_bias = -10.0

  c.grad_clip_norm = 1.0
  c.optax_name = "scale_by_adam"
  c.optax = dict(mu_dtype="float32")
  c.lr = 0.003
  c.wd = 0.001
  c.schedule = dict(warmup_steps=10_000, decay_type="linear", linear_end=0.01)

  # the rho schedule follows the learning rate between its end points (trainers/proj/gsam/gsam.py: sam_rho)
  c.gsam = dict(rho_max=0.6, rho_min=0.1, alpha=0.6, lr_max=c.get_ref("lr"),
                lr_min=c.schedule.get_ref("linear_end") * c.get_ref("lr"))

  sub = "[:16]" if local else ""
  common = dict(type="classification", dataset="imagenet2012", pp_fn=pp_eval("label"), loss_name=c.loss, log_steps=2500)
  c.evals = {}
  c.evals.train = dict(common, split="train[:2%]")
  c.evals.minival = dict(common, split="train[:16]" if local else "train[99%:]")
  c.evals.val = dict(common, split=f"validation{sub}")
  c.evals.v2 = dict(common, dataset="imagenet_v2", split=f"test{sub}")
  c.evals.real = dict(common, dataset="imagenet2012_real", split=f"validation{sub}", pp_fn=pp_eval("real_label"))
  return c
