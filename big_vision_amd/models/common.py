"""What the model modules share: the Flax-like shell around an executor, and checkpoint <-> init reconciliation.

The shell.  A model class keeps what is its own - its constructor checks, `entries`, its executor class, its layout key
- and takes the rest from here: `Tower` (one input: vit, text_transformer, naflex_vit, bert) and `Pair` (image + text:
two_towers, one_tower) give it `init`, `leaf_names` / `make_store`, the executor cache and the resolution of the tree
an `apply` was handed to a store.  `model._execs` holds both the executors, keyed (id(store), prefix, <layout key>,
want_grads), and the one ad-hoc store per layout of `params.adhoc_store`, keyed ("adhoc", <layout key>, device).

Checkpoint reconciliation.  Contract (what a caller of big_vision/models/common.py:24-92 relies on): the result has
exactly the leaves of `inited`; a leaf comes from `loaded` unless one of the `dont_load` regexes full-matches its
`/`-joined name; a name that exists on one side only and is not excused by `dont_load` is an error whose text lists
both trees and the two difference sets (with the ` - ` / ` + ` markers tools grep for).  The error text is API; the
code below is ours."""
import importlib
import math

import torch

from big_vision_amd import engine as E
from big_vision_amd import utils as u
from big_vision_amd.params import Entry, ParamTree, adhoc_store, entry_leaf_names, make_store

MODELS_PKG = "big_vision_amd.models"


# ------------------------------------------------------------ shared pieces --
def check_head_dim(width, num_heads):
  """Refuses, when the model is built, a head size no attention kernel serves."""
  if width % num_heads or (width // num_heads) % 8 or width // num_heads > 128:
    raise NotImplementedError(f"attention kernels need a head_dim that is a multiple of 8 and <= 128 (64 is the "
                              f"fast path), got {width}/{num_heads}")


def head_entries(prefix, feat, num_classes, rep_size=False, head_zeroinit=True):
  """`pre_logits` (rep_size: True = as wide as its input) and `head` below `prefix`, on `feat` input features."""
  ents = []
  if rep_size:
    rs = feat if rep_size is True else rep_size
    ents += [Entry(f"{prefix}pre_logits/kernel", (feat, rs), E.init_lecun_normal(feat)),
             Entry(f"{prefix}pre_logits/bias", (rs,), E.init_zeros)]
    feat = rs
  if num_classes:
    kinit = E.init_zeros if head_zeroinit else E.init_lecun_normal(feat)
    ents += [Entry(f"{prefix}head/kernel", (feat, num_classes), kinit),
             Entry(f"{prefix}head/bias", (num_classes,), E.init_zeros)]
  return ents


def report_tail(out, t_out, x, n, L, per_token, keys=("pre_logits", "logits")):
  """Copies the `keys` a PooledTail produced from `t_out` to `out` and returns `x`; per_token (pool_type "none"):
  each of them as [n, L, .], like the reference's un-pooled x."""
  shaped = (lambda t: t.view(n, L, -1)) if per_token else (lambda t: t)
  out.update({k: shaped(t_out[k]) for k in keys if k in t_out})
  return shaped(x)


def dropout_key(rates, train, rngs):
  """The 64-bit dropout key of an `apply(..., train=, rngs=)` call, None when the call is deterministic (flax: a module
  with dropout > 0 applied with train=True and no "dropout" rng raises)."""
  if not train or not any(float(r or 0.0) > 0.0 for r in rates):
    return None
  if not rngs or "dropout" not in rngs:
    raise ValueError("train=True with dropout > 0 needs rngs={'dropout': key}")
  return E.seed_of(rngs["dropout"])


def dropout_for(rate, train, rngs):
  """engine.Dropout of a tower's `apply(..., train=, rngs=)` call, None when the call is deterministic."""
  key = dropout_key((rate,), train, rngs)
  return None if key is None else E.Dropout(rate, key)


def refuse_remote(path, what):
  """`path`, unless it is a URL: nothing is fetched.  `what` names the config field in the error."""
  if isinstance(path, str) and "://" in path:
    raise FileNotFoundError(f"{what} resolves to {path!r}: remote checkpoints cannot be opened "
                            "here; download it and pass the local .npz path")
  return path


# ---------------------------------------------------------------- the shell --
class _Shell:
  """Executor cache and store handling of a model whose `entries(prefix, *layout)` list its parameters, whose
  `Exec(model, store, prefix, *layout)` runs them and whose constructor sets `self._execs = {}`."""
  Exec = None

  def _leaf_names(self, layout):
    return entry_leaf_names(self.entries("", *layout), self.scan_prefixes())

  def _make_store(self, layout, device=None, frozen_leaves=()):
    return make_store(self.entries("", *layout), device, self.scan_prefixes(), frozen_leaves)

  @staticmethod
  def _variables(store, rng):
    store.init_random(E.seed_of(rng))
    store.refresh_shadow()
    return {"params": store.tree()}

  def _executor(self, store, prefix, *layout):
    key = (id(store), prefix, *layout, getattr(store, "want_grads", False))
    if key not in self._execs:
      self._execs[key] = self.Exec(self, store, prefix, *layout)
    return self._execs[key]

  def _store_for(self, params, layout):
    """(store, prefix) behind the tree an `apply` was handed: the store the tree is bound to, or the ad-hoc store of
    `layout()` (called for a plain tree only: a pair model may have to size an absent input from the tree) with the
    tree's values loaded; its bf16 shadow is current either way."""
    if isinstance(params, ParamTree) and params.store is not None:
      store, prefix = params.store, params.prefix
    else:
      layout = tuple(layout())
      key = layout + (torch.cuda.current_device(),)
      store = adhoc_store(self._execs, key, params, lambda: self._make_store(layout))
      prefix = ""
    store.refresh_shadow()
    return store, prefix


class Tower(_Shell):
  """Flax-like init / apply of a model with ONE input.  A tower states its executor class `Exec`, the name `encoder` of
  its scanned encoder below its prefix (None: no block is ever presented stacked), and `layout(shape)`, the key of
  everything that depends on the input's shape (default: `grid(shape)`).  `dropout` None: the tower has no dropout
  site, its `apply` ignores train / rngs and its executor's `fwd` takes no `drop`.  late_input_check: the executor
  validates its input on the device and `check_pending()` raises the verdict before the outputs are handed out."""
  encoder = None
  dropout = None
  late_input_check = False

  def layout(self, shape):
    return self.grid(shape)

  def scan_prefixes(self, prefix=""):
    """Encoders presented with stacked blocks (scan=True, vit.py:129-148)."""
    return (f"{prefix}{self.encoder}",) if self.encoder and self.scan else ()

  def leaf_names(self, shape):
    """Leaf names as presented (stacked `encoderblock` for a tower built with scan=True)."""
    return self._leaf_names((self.layout(tuple(shape)),))

  def make_store(self, shape, device=None, frozen_leaves=()):
    """The flat parameter store for inputs of `shape` (params.make_store: `device` None = the current GPU)."""
    return self._make_store((self.layout(tuple(shape)),), device, frozen_leaves)

  def init(self, rng, inputs, **kw):
    del kw
    first = inputs[0] if isinstance(inputs, (tuple, list)) else inputs     # (NaFlex: the patches of the input tuple)
    on_gpu = torch.is_tensor(first) and first.is_cuda
    return self._variables(self.make_store(E.input_shape(inputs), first.device if on_gpu else None), rng)

  def executor(self, store, prefix, layout):
    return self._executor(store, prefix, tuple(layout) if isinstance(layout, (tuple, list)) else int(layout))

  def apply(self, variables, inputs, *, train=False, rngs=None, collect=True, **kw):
    """train=True with dropout > 0 needs rngs={"dropout": key} (vit.py:228, train.py:298), as in the reference."""
    del kw
    layout = self.layout(E.input_shape(inputs))
    store, prefix = self._store_for(variables["params"], lambda: (layout,))
    ex = self.executor(store, prefix, layout)
    drop = {} if self.dropout is None else {"drop": dropout_for(self.dropout, train, rngs)}
    x, out, _ = ex.fwd(inputs, save=False, collect=collect, **drop)
    if self.late_input_check:
      ex.check_pending()        # the verdict on THIS batch, before its outputs are handed out
    return x, out


class Pair(_Shell):
  """Flax-like shell of a model of an image and a text input that end in one loss: `towers` ({"img": tower, ...} in
  parameter order) below a log-temperature `t` and, with `bias_init`, a bias `b`.  A pair model states its executor
  class `Exec` and `layout(image_shape, text_shape)`, one layout key per tower."""

  def entries(self, prefix, *layout):
    ents = [e for (name, tower), key in zip(self.towers.items(), layout) for e in tower.entries(f"{prefix}{name}/", key)]
    ents.append(Entry(f"{prefix}t", (1,), E.init_const(math.log(self.temperature_init))))
    if self.bias_init is not None:
      ents.append(Entry(f"{prefix}b", (1,), E.init_const(self.bias_init)))
    return ents

  def scan_prefixes(self, prefix=""):
    return tuple(p for name, tower in self.towers.items() for p in tower.scan_prefixes(f"{prefix}{name}/"))

  def leaf_names(self, image_shape, text_shape=None):
    """Leaf names as presented (stacked `encoderblock` for towers built with scan=True)."""
    return self._leaf_names(self.layout(image_shape, text_shape))

  def make_store(self, image_shape, text_shape=None, device=None, frozen_leaves=()):
    """Allocates the flat parameter store of the towers (+ t, b).

    `frozen_leaves`: exact Flax leaf names that get no gradient / optimizer
    state (config.schedule None entries); they are laid out last (params.make_store)."""
    return self._make_store(self.layout(image_shape, text_shape), device, frozen_leaves)

  def init(self, rng, image, text=None, **kw):
    del kw
    return self._variables(self.make_store(E.input_shape(image), E.input_shape(text)), rng)

  def dropout_key(self, train, rngs):
    """The pass's 64-bit dropout key when `train` and a tower's config asks for dropout > 0, else None."""
    return dropout_key([tower.dropout for tower in self.towers.values()], train, rngs)


def load_parts(parts, init_params, init_files, model_cfg, tower_kw, local_only=False):
  """The loop of a pair model's `load`.  parts: ((init-file keys of `config.model_init`, leaf of the param tree,
  model_cfg key of the tower's module or None for a plain array, default module), ...); init_files: {key: source},
  consumed here.  Towers are restored by their own module's `load` with `tower_kw[leaf]`; parts without an init file
  keep `init_params`; a key nobody consumed is refused with the reference's message (a typo in a config must not pass
  silently).  local_only: the towers' vanity names are resolved here and a remote source is refused."""
  restored_params = dict(init_params) if init_params else {leaf: None for _, leaf, module_key, _ in parts if module_key}
  for aliases, leaf, module_key, default_module in parts:
    found = [init_files.pop(a) for a in aliases if a in init_files]
    source = found[0] if found else None
    if not source:
      continue
    tower = module_key and importlib.import_module(f"{MODELS_PKG}.{model_cfg.get(module_key, default_module)}")
    if local_only:
      source = getattr(tower, "VANITY_NAMES", {}).get(source, source)
      source = refuse_remote(source, f"config.model_init[{aliases[0]!r}]")
    if tower:
      restored_params[leaf] = tower.load(restored_params.get(leaf), source, model_cfg.get(aliases[0]), **tower_kw[leaf])
    else:
      restored_params[leaf] = u.load_params(source)
  assert not init_files, (
      f"There's something unused left in `config.model_init`. You probably got "
      f"a typo. Here it is: {init_files}")
  return restored_params


# ------------------------------------------- checkpoint <-> init reconciliation --
_SECTIONS = (
    ("Params in checkpoint", "  "),
    ("Params in model (code)", "  "),
    ("Params in model (code) but not in checkpoint and not `dont_load`ed", " - "),
    ("Params in checkpoint but not in model (code) and not `dont_load`ed", " + "),
)


def _report(groups):
  """One block per non-empty name set: a title line, then the sorted names behind that set's marker."""
  blocks = []
  for (title, marker), names in zip(_SECTIONS, groups):
    blocks.append("\n".join([f"{title}:"] + [marker + n for n in sorted(names)]) if names else "")
  return "\n".join(blocks)


def merge_params(loaded, inited, dont_load=(), match_dtype=False):
  """`loaded` reshaped onto the structure of `inited` (see the module docstring).  `match_dtype` casts each
  taken leaf to the dtype of the init leaf it replaces."""
  if inited is None:
    return loaded
  excused = u.check_and_compile_patterns(dont_load)
  have = dict(u.tree_flatten_with_names(loaded)[0])
  want = dict(u.tree_flatten_with_names(inited)[0])
  pinned = {n for n in have.keys() | want.keys() if any(rx.fullmatch(n) for rx in excused)}

  only_model = want.keys() - have.keys() - pinned
  only_ckpt = have.keys() - want.keys() - pinned
  if only_model or only_ckpt:
    raise ValueError(_report((have.keys(), want.keys(), only_model, only_ckpt)))

  def pick(name, init_leaf):
    if name in pinned or name not in have:
      return init_leaf
    leaf = have[name]
    if match_dtype and hasattr(leaf, "dtype") and leaf.dtype != init_leaf.dtype:
      leaf = leaf.to(init_leaf.dtype) if hasattr(leaf, "to") else leaf.astype(init_leaf.dtype)
    return leaf

  names = list(want)
  return u.recover_tree(names, [pick(n, want[n]) for n in names])
