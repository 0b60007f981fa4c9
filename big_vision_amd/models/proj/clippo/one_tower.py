"""CLIPPO: one ViT that embeds the photo and the caption rendered as an image, behind `models.proj.clippo.one_tower`.

Mirrors big_vision/models/proj/clippo/one_tower.py: `Model(**config.model)` with fields image / image_model / out_dim /
temperature_init (:27-32); the tower is resolved by module path below `big_vision_amd.models` and built with
`num_classes=out_dim` under the name `img` (:40-42); both inputs go through THAT tower (:54-60), the embeddings are
L2-normalised with eps 1e-8 (:49-50); `t` (log-temperature) is a (1,)-shaped param (:62-67).  There is no `txt` subtree
and no bias `b`: the sigmoid losses of the contrastive trainer refuse this model.  `apply` returns `(zimg, ztxt, out)`
and accepts `image=None` or `text=None` (:35).  `text` is the rendered caption, a float32 [n, H, W, 3] tensor of the
images' geometry; rendering it is input pipeline (pp/proj/clippo/pp_ops.py) and not part of this package.

One pass over 2n rows.  The reference calls the shared tower twice.  Nothing in a ViT couples the examples of a batch,
so here the tower runs ONCE on cat([image, text]) and the rows are split afterwards: zimg / ztxt and every `img/...` /
`txt/...` entry of `out` are views of the two halves.  The backward concatenates the two cotangents (a missing one is
zeros for its half, not a second code path) and runs once, so every weight gradient is formed in one launch over 2n
rows - the sum over both uses that autograd would accumulate.  One input alone runs its n rows.

Dropout.  The kernels derive the keep bits from (site key, element index).  The 2n batch indexes its elements
0 .. 2n L D - 1, so the text half never repeats the image half's masks; no per-half key is folded.  A lone input folds
its own name ("img" / "txt") into the key, so a text-only pass does not repeat an image-only one either.

The executor is the image half of the two-tower executor (`two_towers.TwoTowersExec`) run on both inputs: the trainers
(`trainers.proj.image_text.contrastive` / `siglip`) and `make_predict_fn` drive it through the same surface.
"""
from __future__ import annotations

import importlib

import torch

from big_vision_amd import engine as E
from big_vision_amd import ops
from big_vision_amd.models import common
from big_vision_amd.models.common import MODELS_PKG
from big_vision_amd.models.proj.image_text.two_towers import TwoTowersExec
from big_vision_amd.params import ParamStore

F32 = torch.float32


def _split_rows(tree, ni, nt):
  """(image half, text half) of a tower `out` entry: tensors are split along their leading axis ([2n, ...] and
  [2n L, ...] alike: rows are ordered by example), nested dicts recursively; anything else is shared."""
  if isinstance(tree, dict):
    halves = {k: _split_rows(v, ni, nt) for k, v in tree.items()}
    return {k: v[0] for k, v in halves.items()}, {k: v[1] for k, v in halves.items()}
  if torch.is_tensor(tree) and tree.dim() > 0 and tree.shape[0] % (ni + nt) == 0:
    cut = tree.shape[0] // (ni + nt) * ni
    return tree[:cut], tree[cut:]
  return tree, tree


def _require_rendered_text(text, want=("H", "W", 3)):
  """`text` must be the caption rendered as an image: float32 [n, H, W, 3] (of the tower's geometry when known)."""
  ok = torch.is_tensor(text) and text.dtype == F32 and text.dim() == 4 and text.shape[3] == 3
  if ok and isinstance(want[0], int):
    ok = tuple(text.shape[1:]) == tuple(want)
  if not ok:
    got = f"{tuple(text.shape)} {text.dtype}" if torch.is_tensor(text) else type(text).__name__
    raise ValueError(f"one_tower: `text` is the caption rendered as an image, a float32 tensor of shape "
                     f"[n, {want[0]}, {want[1]}, 3]; got {got} (tokenised text is not supported)")


class OneTowerExec(TwoTowersExec):
  """Forward / backward of the shared tower bound to a ParamStore at `prefix`, on one batch of image + text rows."""

  def __init__(self, m: "Model", store: ParamStore, prefix: str, hw):   # pylint: disable=super-init-not-called
    self.m, self.store = m, store
    self.img = m.image_tower.executor(store, f"{prefix}img/", hw)
    self.txt = None
    self.prefix, self._ranges = prefix, {}
    self.t = E._W(store, f"{prefix}t")
    self.b = None
    self.streams = 1       # (set by the trainers from config.tower_streams: one tower has nothing to fork)

  def _check_text(self, text, image):
    ph, pw = self.m.image_tower.patch_size
    want = (self.img.hw[0] * ph, self.img.hw[1] * pw, 3)
    _require_rendered_text(text, want)
    if image is not None and (tuple(image.shape[1:]) != want or image.device != text.device):
      raise ValueError(f"one_tower: image {tuple(image.shape)} on {image.device} and text {tuple(text.shape)} on "
                       f"{text.device} must share one geometry [n, {want[0]}, {want[1]}, 3] and one device")

  def fwd(self, image, text, save=False, collect=False, drop_key=None):
    if text is not None:
      self._check_text(text, image)
    out, ctx = {}, {}
    zimg = ztxt = None
    save = E.ctx_kind(save) if self._tower_trainable("img/") else False
    ni = 0 if image is None else int(image.shape[0])
    nt = 0 if text is None else int(text.shape[0])
    if ni or nt:
      x = torch.cat([image.to(F32), text]) if ni and nt else (image if ni else text)
      kw = self._drop_kw(self.m.image_tower, "img" if ni else "txt", drop_key)
      z, o, c = self.img.fwd(x, save, collect, **kw)
      zn, norm = ops.l2norm_fwd(z)
      o = dict(o, norm=norm.view(-1, 1), normalized=zn)
      o_img, o_txt = _split_rows(o, ni, nt) if ni and nt else ((o, None) if ni else (None, o))
      if ni:
        out.update({f"img/{k}": v for k, v in o_img.items()})
        zimg = out["img/normalized"]
      if nt:
        out.update({f"txt/{k}": v for k, v in o_txt.items()})
        ztxt = out["txt/normalized"]
      ctx = {"img": (c, z, norm), "rows": (ni, nt)}
    out["t"] = torch.exp(self.t.f32)
    out["t/parameter"] = self.t.f32
    return zimg, ztxt, out, (ctx if save else None)

  def check_inputs(self):
    pass                   # (the ViT validates nothing late)

  def bwd(self, ctx, dzimg, dztxt, sync=None):
    """dzimg / dztxt: gradients w.r.t. the NORMALISED embeddings of the halves the forward ran (None = zeros for that
    half).  ONE tower backward over all rows; with `sync` (dp.GradSync) every encoder block's gradient range is handed
    to the all-reduce right after that block's backward - it is complete then, both uses of the weights included."""
    if ctx is None or ctx["img"][0] is None or (dzimg is None and dztxt is None):
      return               # a frozen tower kept no context / nothing to differentiate
    ni, nt = ctx["rows"]
    z = ctx["img"][1]
    halves = []
    for rows, dz in ((ni, dzimg), (nt, dztxt)):
      if rows:
        if dz is not None and dz.shape[0] != rows:
          raise ValueError(f"one_tower: cotangent of {dz.shape[0]} rows for a half of {rows} rows")
        halves.append(dz.to(F32) if dz is not None else z.new_zeros((rows, z.shape[1])))
    self._bwd_img(ctx, halves[0].contiguous() if len(halves) == 1 else torch.cat(halves), sync)


class Model(common.Pair):
  """Single ViT to encode regular images and text images."""
  Exec = OneTowerExec

  def __init__(self, image=None, image_model="vit", out_dim=768, temperature_init=10.0, name=None):
    self.image, self.image_model = dict(image or {}), image_model
    self.out_dim, self.temperature_init = out_dim, temperature_init
    self.bias_init = None          # (read by the contrastive trainer: no bias parameter, no sigmoid loss)
    self.image_tower = importlib.import_module(f"{MODELS_PKG}.{image_model}").Model(
        **{"num_classes": out_dim, **self.image}, name="img")
    self.towers = {"img": self.image_tower}
    self.name = name
    self._execs = {}

  def _geometry(self, image_shape, text_shape):
    """[n, H, W, 3] the tower is laid out for, from whichever input is there (both: they must agree)."""
    shapes = [tuple(s) for s in (image_shape, text_shape) if s is not None]
    if not shapes:
      raise ValueError("one_tower: neither an image nor a text shape")
    if any(len(s) != 4 or s[1:] != shapes[0][1:] for s in shapes):
      raise ValueError(f"one_tower: image and text (the caption rendered as an image) share one shape [n, H, W, 3]; "
                       f"got image {image_shape}, text {text_shape}")
    return shapes[0]

  def layout(self, image_shape, text_shape=None):
    return (self.image_tower.layout(self._geometry(image_shape, text_shape)),)

  def executor(self, store, prefix, image_shape, text_shape=None):
    return self._executor(store, prefix, *self.layout(image_shape, text_shape))

  def apply(self, variables, image, text=None, *, train=False, rngs=None, collect=True, **kw):
    """train=True: the tower's dropout (if its config asks for any) is drawn from rngs["dropout"]."""
    del kw
    drop_key = self.dropout_key(train, rngs)
    if text is not None:
      _require_rendered_text(text)
    ishape, tshape = E.input_shape(image), E.input_shape(text)
    store, prefix = self._store_for(variables["params"], lambda: self.layout(ishape, tshape))
    if image is None and text is None:     # (one_tower.py:53-69: only t is reported)
      t = store.t(f"{prefix}t")
      return None, None, {"t": torch.exp(t), "t/parameter": t}
    ex = self.executor(store, prefix, ishape, tshape)
    zimg, ztxt, out, _ = ex.fwd(image, text, save=False, collect=collect, drop_key=drop_key)
    return zimg, ztxt, out


# init-file keys of `config.model_init` -> (leaf of the param tree, default tower module or None for a plain array)
_PARTS = ((("image", "img"), "img", "image_model", "vit"), (("temperature", "t"), "t", None, None))


def load(init_params, init_files, model_cfg, img_load_kw={}):  # pylint: disable=dangerous-default-value
  """Restores the tower and the temperature (contract of one_tower.py:72-96).

  `init_files`: ONE checkpoint path (its `img` and `t` sub-trees are taken) or a dict {"image"|"img",
  "temperature"|"t"} -> path.  The tower is restored by its own module's `load` with `img_load_kw`; parts without an
  init file keep `init_params`; a key nobody consumed is refused with the reference's message (a typo in a config must
  not pass silently)."""
  todo = {k: f"{init_files}:{k}" for k in ("img", "t")} if isinstance(init_files, str) else dict(init_files)
  # (a remote source - a tower's vanity name resolves to one - is refused here the way train.load_init refuses it)
  return common.load_parts(_PARTS, init_params, todo, model_cfg, {"img": img_load_kw}, local_only=True)
