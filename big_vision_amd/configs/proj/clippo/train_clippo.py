"""CLIPPO (CLIP with Pixels Only, arXiv 2212.08045): one ViT for photos and rendered captions, contrastive trainer.

Counterpart of big_vision/configs/proj/clippo/train_clippo.py for the accelerated hot path, written from its field
values: a run configured from either file builds the same model (`proj.clippo.one_tower`: ViT `variant` with the MAP
head, head_zeroinit False, temperature 10, out_dim 768), the same optimizer (Adafactor, clip norm 1), the same rsqrt
schedule and the same `evals` section; tests/test_clippo_cpu.py compares the two field by field where a reference
checkout is present.  Arguments as there: `res`, `runlocal`, `variant`, `test_with_coco` (default True: COCO captions,
a 400-step sanity run from the i21k B/16 checkpoint), `i1k_eval`.

The `pp` / `pp_fn` / `pp_txt` / `pp_img` entries stay what they are in the reference: STRINGS for its input pipeline.
Rendering captions with unifont (pp/proj/clippo/pp_ops.py) is out of scope here; the step consumes
`image` and `labels` as float32 [n, res, res, 3] tensors, stated in `init_shapes`.  The `fewshot` entry names the
`fewshot_lsr` evaluator, which this package does not provide: `evaluators.common.from_config` refuses it by name.
"""
import big_vision.configs.common as bvcc
from ml_collections import ConfigDict


def _render(res, inkey, outkey="labels"):
  """pp string that renders the feature `inkey` into a [-1, 1] image under `outkey`."""
  return (f'render_unifont(inkey="{inkey}", outkey="{outkey}", image_size={res}, lower=True, font_size=16, '
          f'text_brightness=0, background_brightness=127)|value_range(-1, 1, inkey="{outkey}", outkey="{outkey}")')


def _fewshot(log_steps):
  pp = 'decode|resize(256)|central_crop(224)|value_range(-1,1)|keep("image", "label")'
  return ConfigDict(dict(
      representation_layer="img/pre_logits", shots=(1, 5, 10, 25), l2_reg=2.0 ** 10, num_seeds=3, prefix="",
      log_steps=log_steps, type="fewshot_lsr",
      datasets={"caltech": ("caltech101", "train", "test"), "cars": ("cars196:2.1.0", "train", "test"),
                "cifar100": ("cifar100", "train", "test"), "dtd": ("dtd", "train", "test"),
                "pets": ("oxford_iiit_pet", "train", "test"), "uc_merced": ("uc_merced", "train[:1000]", "train[1000:]")},
      pp_train=pp, pp_eval=pp, display_first=[("imagenet", 10)]))


def get_config(arg=None):
  arg = bvcc.parse_arg(arg, res=224, runlocal=False, variant="B/16", test_with_coco=True, i1k_eval=False)
  local = arg.runlocal
  c = ConfigDict()

  if not arg.test_with_coco:
    # the TFDS catalogue has no large image / alt-text set: name yours here (and its validation split below)
    raise AssertionError("test_with_coco=False needs an image/alt-text data set: set config.input.data and the "
                         "validation data in this file")
  train_data = dict(name="coco_captions", split="train")
  val_data = dict(train_data, split="val")
  text_key = "captions/text"
  pp_image = f"decode|resize({arg.res})|value_range(-1,1)"
  pp_train_image = f"decode|resize({arg.res})|flip_lr|randaug(2,10)|value_range(-1,1)"     # augmented sanity run
  pairs = lambda pp_img, key: f'{pp_img}|flatten|{_render(arg.res, key)}|keep("image", "labels")'

  c.input = dict(data=train_data, batch_size=32 if local else 4000, shuffle_buffer_size=50 if local else 50_000)
  c.total_steps = 10 if local else 400
  c.input.pp = pp_eval = pairs(pp_train_image, text_key)
  c.pp_modules = ["ops_general", "ops_image", "ops_text", "proj.clippo.pp_ops"]
  c.init_shapes = [(1, arg.res, arg.res, 3), (1, arg.res, arg.res, 3)]
  c.init_types = ["float32", "float32"]

  c.log_training_steps = 50
  c.ckpt_steps = 1000
  c.keep_ckpt_steps = 5000
  c.loss_use_global_batch = True

  c.model_name = "proj.clippo.one_tower"
  c.model = ConfigDict()
  c.model.image_model = "vit"
  c.model.image = ConfigDict(dict(variant=arg.variant, pool_type="map", head_zeroinit=False))
  c.model.temperature_init = 10.0
  c.model.out_dim = 768
  # the sanity run starts from the ImageNet-21k checkpoint, without its head
  assert arg.variant == "B/16", arg.variant
  c.model_init = {"image": "howto-i21k-B/16"}
  c.model_load = {"img_load_kw": {"dont_load": ["^head/.*", "^MAPHead_0/.*", "cls"]}}

  c.optax_name = "big_vision.scale_by_adafactor"
  c.grad_clip_norm = 1.0
  c.lr = 0.0001
  c.wd = 0.0003
  ramp = 5 if local else 100
  c.schedule = dict(decay_type="rsqrt", timescale=100, warmup_steps=ramp, cooldown_steps=ramp)

  contrastive = dict(type="proj.image_text.contrastive", use_global_batch=c.loss_use_global_batch,
                     log_steps=5 if local else 1000)
  slow = 5 if local else 5_000
  sub = "[:4]" if local else ""
  c.evals = {}
  c.evals.val = dict(contrastive, data=val_data, pp_fn=pp_eval)
  c.evals.coco = dict(contrastive, data=dict(name="coco_captions", split=f"val{sub}"), pp_fn=pairs(pp_image, text_key))
  if arg.i1k_eval:     # needs a manually prepared ImageNet
    c.evals.imagenet = dict(contrastive, data=dict(name="imagenet2012", split=f"validation{sub}"),
                            pp_fn=f'{pp_image}|clip_i1k_label_names|{_render(arg.res, "labels")}|keep("image", "labels")')
    c.evals.disclf = dict(type="proj.image_text.discriminative_classifier", pp_txt=_render(arg.res, "texts", "labels"),
                          prefix="z/0shot/", log_steps=slow)
  c.evals.retrieval_coco = ConfigDict(dict(
      type="proj.image_text.retrieval", pp_txt=_render(arg.res, "texts"), pp_img=f"resize({arg.res})|value_range(-1, 1)",
      prefix="z/retr/coco_", dataset="coco_captions", txt_name=("captions", "text"), log_steps=slow))
  c.evals.fewshot = _fewshot(slow)

  c.seed = 0
  return c
