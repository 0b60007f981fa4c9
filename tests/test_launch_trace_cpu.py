"""The ORDERED launch sequence of the host path, pinned against golden traces (tests/golden/launch_trace/<case>.json
over the shared table of distinct launches _launches.json).

Same dry run as tests/test_host_dryrun_cpu.py - CPU tensors, `_lib.call` replaced, memory probes faked - but the
recorder keeps every launch in order: the entry point's name, every integer / float argument as it is, every tensor
argument as [dtype, shape] (`ops._p` is patched), host arrays and the `bv_ctx` pointer as tokens.  `ops._contexts` is
cleared before each recording, so the one-off `bv_ctx_set_workspace` of a fresh context is part of every trace and a
trace is a function of the code alone.

What a trace pins: which kernels the towers, the trainers and the optimizer launch, with which shapes, strides,
epilogues and flags, in which order.  What it cannot see: the stream a launch goes to (the dry run has one), and a
mix-up of two tensors of equal dtype and shape - the GPU parity suites see those.

Regenerate (only when a change of the launch sequence is intended):  python tests/test_launch_trace_cpu.py --write
"""
import contextlib
import ctypes
import json
import os
import sys
import tempfile
from unittest import mock

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
  sys.path.insert(0, os.path.dirname(HERE))

from big_vision_amd import _lib, engine as E, ops, train  # noqa: E402
from big_vision_amd import utils as u  # noqa: E402
from big_vision_amd.compat.ml_collections import ConfigDict  # noqa: E402
from big_vision_amd.models import vit  # noqa: E402
from big_vision_amd.models.proj.clippo import one_tower  # noqa: E402
from big_vision_amd.models.proj.flaxformer import bert  # noqa: E402
from big_vision_amd.models.proj.image_text import naflex_vit, text_transformer, two_towers  # noqa: E402
from big_vision_amd.params import ParamStore, flatten_tree  # noqa: E402
from big_vision_amd.trainers.proj.distill import distill  # noqa: E402
from big_vision_amd.trainers.proj.gsam import train as gsam_train  # noqa: E402
from big_vision_amd.trainers.proj.image_text import contrastive, siglip  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "launch_trace")

IMG = dict(width=128, depth=3, mlp_dim=256, num_heads=2, patch_size=(16, 16), pool_type="map")
TXT = dict(width=128, depth=2, mlp_dim=256, num_heads=2, vocab_size=50)
TINY = dict(width=128, depth=2, mlp_dim=256, num_heads=2)
BERT = dict(hidden_size=128, intermediate_dim=256, num_hidden_layers=2, num_attention_heads=2, vocab_size=60,
            max_length=24, num_segments=2)
LIT_SCHEDULE = [("img/.*", None), (".*", dict(decay_type="cosine", warmup_steps=2))]


# ---------------------------------------------------------------- recorder ---
def _tensor_token(t):
  if t is None:
    return None
  if isinstance(t, ops.ShiftedBase):
    return ["shifted", str(t.dtype)[6:], list(t.t.shape), t.shift]
  return [str(t.dtype)[6:], list(t.shape)]     # ("torch.bfloat16" -> "bfloat16")


def _arg_token(a, ctx_ptrs):
  if a is None or isinstance(a, (list, str, float)):
    return a
  if isinstance(a, bool):
    return int(a)
  if isinstance(a, int):
    return "ctx" if a in ctx_ptrs else a
  if isinstance(a, (ctypes.c_void_p, ctypes.Array)):
    return "host"
  raise TypeError(f"launch argument of unexpected type {type(a)}: {a!r}")


@contextlib.contextmanager
def dry_run(trace):
  """The host path on CPU tensors; every `_lib.call` is appended to `trace` instead of being made."""
  mem = {"alloc": 0}

  def fake_allocated(*a):       # every probe sees 1 GiB more "allocated": a forward "costs" 1 GiB
    mem["alloc"] += 1 << 30
    return mem["alloc"]

  def call(name, *args):
    ctx_ptrs = {c.ptr for c in ops._contexts.values()}
    if name == "bv_ctx_set_workspace":   # (ctx, the workspace's raw address, bytes)
      args = (args[0], None if args[1] is None else "workspace", args[2])
    trace.append([name] + [_arg_token(a, ctx_ptrs) for a in args])

  with contextlib.ExitStack() as st:
    for obj, attr, new in ((_lib, "call", call), (ops, "_p", _tensor_token), (ops, "_chk", lambda t, dtype, name: t),
                           (ops, "_stream", lambda: 0),
                           (torch.cuda, "mem_get_info", lambda *a: (1 << 40, 1 << 40)),
                           (torch.cuda, "memory_reserved", lambda *a: 0),
                           (torch.cuda, "memory_allocated", fake_allocated)):
      st.enter_context(mock.patch.object(obj, attr, new))
    yield


def record(case):
  """`case()` sets the workload up (its launches are not recorded) and returns the callable whose launches are."""
  trace = []
  old = E.set_residual_stream(torch.float32)
  try:
    with dry_run(trace):
      run = case()
      ops._contexts.clear()
      trace.clear()
      run()
  finally:
    E.set_residual_stream(old)
    ops._contexts.clear()
  return trace


# ------------------------------------------------------------------- cases ---
def _cfg(**kw):
  c = ConfigDict()
  c.lr, c.wd, c.optax_name, c.total_steps, c.grad_clip_norm = 1e-3, 1e-2, "scale_by_adam", 10, 1.0
  c.schedule = dict(decay_type="cosine", warmup_steps=2)
  for k, v in kw.items():
    c[k] = v
  return c


def _siglip(config, image=IMG, text=TXT, n=8, rng=None, apply_collect=False, trainer=siglip, predict=False, clippo=False,
            **model_kw):
  """One step of `trainer` (siglip | contrastive), or its predict function; clippo: on the one-tower model, whose
  caption is an image of the photo's geometry."""
  def case():
    if clippo:
      model = one_tower.Model(image=image, out_dim=64)
    else:
      model = two_towers.Model(image=image, text=text, out_dim=(None, 64), temperature_init=10.0, bias_init=-10.0,
                               **model_kw)
    images = torch.zeros((n, 32, 32, 3))
    labels = torch.zeros((n, 32, 32, 3)) if clippo else torch.ones((n, 8), dtype=torch.int32)
    state, _ = trainer.make_train_state(model, config, tuple(images.shape), tuple(labels.shape), rng=0, total_steps=10,
                                        device="cpu")
    if apply_collect:
      return lambda: model.apply({"params": state["params"]}, images, labels, train=True, collect=True,
                                 rngs={"dropout": rng})
    if predict:
      fn = trainer.make_predict_fn(model, config)
      return lambda: fn(state, {"image": images, "labels": labels})
    fn = trainer.make_update_fn(model, config)
    return lambda: fn(state, rng, {"image": images, "labels": labels})
  return case


def _gsam_read_back():
  """The GSAM vector stage reads |g_clean|^2 and (<g_robust, g_clean>, |g_robust|^2) back from fp64 accumulators,
  which a dry run leaves at zero, and divides by them: the two read-backs return fixed non-zero values instead."""
  item, tolist = torch.Tensor.item, torch.Tensor.tolist
  return (mock.patch.object(torch.Tensor, "item", lambda t: 4.0 if t.dtype == torch.float64 else item(t)),
          mock.patch.object(torch.Tensor, "tolist", lambda t: [1.0, 2.0] if t.dtype == torch.float64 else tolist(t)))


def _vit_cls(num_classes=16, cfg=None, rng=0, batch=None, trainer=train, predict=False, read_back=False, **model):
  """One step of `trainer` (train | the GSAM trainer) on the tiny ViT, or its predict function."""
  def case():
    config = _cfg(model_name="vit", num_classes=num_classes, loss="softmax_xent",
                  model=dict(patch_size=(16, 16), **TINY, **model), **(cfg or {}))
    _, m = trainer.get_model(config)
    state, _ = trainer.make_train_state(m, config, (2, 32, 32, 3), rng=0, total_steps=10, device="cpu")
    data = {"image": torch.zeros((2, 32, 32, 3)), "labels": torch.zeros((2, num_classes)), **(batch or {})}
    if predict:
      fn = trainer.make_predict_fn(m, config)
      return lambda: fn(state, data)
    fn = trainer.make_update_fn(m, config)

    def run():
      with contextlib.ExitStack() as st:
        for patch in (_gsam_read_back() if read_back else ()):
          st.enter_context(patch)
        fn(state, rng, data)
    return run
  return case


def _distill(teachers, cfg=None, rng=0, labels=True, batch=None, shapes=None, predict=None, **student):
  """One step of the distillation trainer, or the predict function named `predict`.  Teacher i is a ViT of depth 1 + i
  whose checkpoint is written to a temporary directory and loaded by make_train_state."""
  n, classes = 4, 10

  def case():
    config = _cfg(num_classes=classes, student_name="vit", student=dict(patch_size=(16, 16), **TINY, **student),
                  teachers=list(teachers), **(cfg or {}))
    for i, t in enumerate(teachers):
      config[f"{t}_name"], config[t] = "vit", dict(patch_size=(16, 16), **dict(TINY, depth=1 + i))
    models = distill.get_models(config)
    image_shapes = {"image": (n, 32, 32, 3), **(shapes or {})}
    with tempfile.TemporaryDirectory() as tmp:
      for t in teachers:
        m = models[t]
        store = ParamStore(m.entries("", m.grid(tuple(image_shapes.get(t, image_shapes["image"])))), "cpu")
        store.init_random(7)
        config[f"{t}_init"] = os.path.join(tmp, f"{t}.npz")
        u.save_params_npz(config[f"{t}_init"], {"params": store.tree()})
      state, _ = distill.make_train_state(models, config, image_shapes, rng=0, total_steps=10, device="cpu")
    data = {k: torch.zeros(s) for k, s in image_shapes.items()}
    if labels:
      data["labels"] = torch.zeros((n, classes))
    data.update(batch or {})
    if predict:
      fn = distill.make_predict_fns(models, config)[predict]
      return lambda: fn(state, data)
    fn = distill.make_update_fn(models, config)
    return lambda: fn(state, rng, data)
  return case


@contextlib.contextmanager
def _cpu_for_cuda():
  """An ad-hoc `apply` allocates its store on the current GPU: the dry run's is the CPU."""
  cpu = torch.empty(0).device
  with mock.patch.object(torch, "device", lambda *a, **k: cpu), mock.patch.object(torch.cuda, "current_device", lambda: 0):
    yield


def _plain(store):
  """The store's values as a plain numpy tree, bound to no store (what a checkpoint reader hands to `apply`)."""
  return u.tree_map(lambda v: v.numpy().copy(), dict(store.tree()))


def _apply_adhoc(m, tree, *inputs):
  with _cpu_for_cuda():
    return m.apply({"params": tree}, *inputs, collect=True)


def _tower_setup(make_model, key, inputs, scan=False):
  """(model, its initialised CPU store, the inputs of `apply`) of ONE tower."""
  m = make_model()
  store = ParamStore(m.entries("", key), "cpu", scan_prefixes=m.scan_prefixes() if scan else ())
  store.init_random(0)
  store.refresh_shadow()
  return m, store, (inputs,)


def _pair_setup(clippo=False, image=True, text=True):
  """(model, its initialised CPU store, the inputs of `apply`) of a pair model; an absent input is None."""
  if clippo:
    model = one_tower.Model(image=IMG, out_dim=64)
  else:
    model = two_towers.Model(image=IMG, text=TXT, out_dim=(None, 64), temperature_init=10.0, bias_init=-10.0)
  images = torch.zeros((2, 32, 32, 3))
  labels = torch.zeros((2, 32, 32, 3)) if clippo else torch.ones((2, 8), dtype=torch.int32)
  store = model.make_store(tuple(images.shape), tuple(labels.shape), device="cpu")
  store.init_random(0)
  store.refresh_shadow()
  return model, store, (images if image else None, labels if text else None)


def _apply(setup, adhoc=False, then_no_input=False):
  """`model.apply(..., collect=True)` on a tree bound to its store, or (adhoc) on a plain numpy tree;
  then_no_input: followed by the store-bound apply without any input (one_tower reports `t` alone)."""
  def case():
    m, store, inputs = setup()
    if adhoc:
      tree = _plain(store)
      return lambda: _apply_adhoc(m, tree, *inputs)

    def run():
      m.apply({"params": store.tree()}, *inputs, collect=True)
      if then_no_input:
        m.apply({"params": store.tree()}, None, None)
    return run
  return case


def _tower(make_model, key, inputs, collect=False, scan=False):
  """Forward + backward of ONE tower through its executor (collect: `model.apply(..., collect=True)` instead)."""
  def case():
    m, store, _ = _tower_setup(make_model, key, inputs, scan)
    if collect:
      return lambda: m.apply({"params": store.tree()}, inputs, collect=True)
    store.want_grads = True
    store.zero_grad()
    ex = m.executor(store, "", key)

    def run():
      x, _, ctx = ex.fwd(inputs, save=True)
      ex.bwd(ctx, torch.zeros_like(x))
    return run
  return case


def _text(collect=False, scan=False, **kw):
  ids = torch.ones((2, 8), dtype=torch.int32)
  return _tower(lambda: text_transformer.Model(64, **TINY, vocab_size=50, scan=scan, **kw), 8, ids, collect, scan)


def _text_setup():
  return _tower_setup(lambda: text_transformer.Model(64, **TINY, vocab_size=50), 8, torch.ones((2, 8), dtype=torch.int32))


def _bert_setup():
  return _tower_setup(lambda: bert.Model(BERT, num_classes=64), 8, torch.ones((2, 8), dtype=torch.int32))


def _naflex_setup():
  batch = _naflex_batch()
  return _tower_setup(lambda: naflex_vit.Model(16, **TINY, nposemb=4, posemb="learn_2d(16)"), int(batch[0].shape[-1]),
                      batch)


def _naflex_batch(holes=False):
  grids, N, pd = [(2, 3), (3, 3), (1, 4)], 9, 8 * 8 * 3
  patches, ptype = torch.zeros((len(grids), N, pd)), torch.zeros((len(grids), N), dtype=torch.int32)
  yabs, xabs = torch.zeros((len(grids), N), dtype=torch.int32), torch.zeros((len(grids), N), dtype=torch.int32)
  for e, (h, w) in enumerate(grids):
    ptype[e, :h * w] = 1
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    yabs[e, :h * w], xabs[e, :h * w] = yy.flatten().int(), xx.flatten().int()
  if holes:   # padding in front: a mask that is not a prefix (the executor reorders the tokens)
    patches, ptype, yabs, xabs = (t.flip(1) for t in (patches, ptype, yabs, xabs))
  return patches, ptype, yabs, xabs


def _naflex(num_classes=None, collect=False, holes=False, **kw):
  batch = _naflex_batch(holes)
  return _tower(lambda: naflex_vit.Model(num_classes, **TINY, nposemb=4, posemb="learn_2d(16)", **kw),
                int(batch[0].shape[-1]), batch, collect)


def _vit_collect(num_classes=None, **kw):
  image = torch.zeros((2, 32, 32, 3))
  m = lambda: vit.Model(num_classes, patch_size=(16, 16), **TINY, **kw)
  return _tower(m, m().grid(tuple(image.shape)), image, collect=True)


DROP = dict(image=dict(IMG, dropout=0.1), text=dict(TXT, dropout=0.1), rng=7)
MB = dict(microbatch=2)
MIXUP = dict(cfg=dict(mixup=dict(p=0.2, fold_in=None)), batch=dict(mixup_a=0.75))    # (the batch's own coefficient)
BF16 = dict(residual_stream="bfloat16")
GSAM = dict(rho_max=0.6, rho_min=0.1, alpha=0.6, lr_max=1e-3, lr_min=1e-5)

CASES = {
    # SigLIP step: one pass; two passes over 4 micro-batches with every keep / context-kind scheme
    "siglip_single": _siglip(_cfg()),
    "siglip_mb_keep_all_full": _siglip(_cfg(**MB, microbatch_keep="all", microbatch_light=False)),
    "siglip_mb_keep_all_light": _siglip(_cfg(**MB, microbatch_keep="all", microbatch_light="light")),
    "siglip_mb_keep_1_g": _siglip(_cfg(**MB, microbatch_keep=1, microbatch_light="g")),
    "siglip_mb_keep_0_full": _siglip(_cfg(**MB, microbatch_keep=0, microbatch_light=False)),
    "siglip_mb_keep_all_true_bf16": _siglip(_cfg(**MB, microbatch_keep="all", microbatch_light=True,
                                                 residual_stream="bfloat16")),
    "siglip_single_light": _siglip(_cfg(microbatch_light="light")),
    "siglip_mb_auto": _siglip(_cfg(**MB)),
    # dropout > 0 on both towers: the contexts with site keys, and the branch outputs that leave them again
    "siglip_dropout": _siglip(_cfg(), **DROP),
    "siglip_dropout_mb": _siglip(_cfg(**MB, microbatch_keep=1), **DROP),
    "two_towers_apply_train_collect_dropout": _siglip(_cfg(), apply_collect=True, **DROP),
    # LiT: the frozen image tower keeps no context and takes no backward
    "lit_frozen_image": _siglip(_cfg(schedule=LIT_SCHEDULE)),
    # ViT classification step
    "vit_cls_gap": _vit_cls(pool_type="gap"),
    "vit_cls_tok": _vit_cls(pool_type="tok"),
    "vit_cls_0": _vit_cls(pool_type="0"),
    "vit_cls_map": _vit_cls(pool_type="map"),
    "vit_cls_gap_rep12_classes10": _vit_cls(num_classes=10, pool_type="gap", rep_size=12, posemb="sincos2d"),
    "vit_cls_tok_rep_true": _vit_cls(pool_type="tok", rep_size=True),
    "vit_cls_mixup_dropout": _vit_cls(pool_type="gap", dropout=0.1, rng=7, **MIXUP),
    "vit_cls_bf16": _vit_cls(pool_type="gap", cfg=BF16),
    # distillation: one teacher with labels; two teachers, one on its own input key, mixup, student dropout, no labels
    "distill_one_teacher_kl": _distill(("prof_a",), cfg=dict(distance="kl"), pool_type="gap"),
    "distill_two_teachers_mixup_dropout": _distill(
        ("prof_a", "prof_b"), cfg=dict(mixup=dict(p=0.2, fold_in=None), distance="kl", distance_kw=dict(t=2.0)), rng=7,
        labels=False, batch=dict(mixup_a=0.75), shapes=dict(prof_b=(4, 48, 48, 3)), pool_type="gap", dropout=0.1),
    # contrastive trainer: config.loss_fn on the two-tower model, and CLIPPO's one tower
    "contrastive_softmax": _siglip(_cfg(loss_fn="softmax"), trainer=contrastive),
    "contrastive_sigmoid": _siglip(_cfg(loss_fn="sigmoid"), trainer=contrastive),
    "contrastive_chunked_sigmoid": _siglip(_cfg(loss_fn="chunked_sigmoid"), trainer=contrastive),
    "contrastive_softmax_mb": _siglip(_cfg(loss_fn="softmax", **MB), trainer=contrastive),
    "clippo_step": _siglip(_cfg(), trainer=contrastive, clippo=True),
    # GSAM (the scalars it reads back are patched, see _gsam_read_back) and SAM, which runs on a dry run's zeros
    "gsam_dropout": _vit_cls(trainer=gsam_train, cfg=dict(gsam=GSAM), pool_type="gap", dropout=0.1, rng=7,
                             read_back=True),
    "sam": _vit_cls(trainer=gsam_train, cfg=dict(gsam=dict(GSAM, rho_min=0.6, alpha=0.0)), pool_type="gap"),
    # predict functions
    "predict_cls_bf16": _vit_cls(pool_type="gap", cfg=BF16, predict=True),
    "predict_siglip_bf16": _siglip(_cfg(**BF16), predict=True),
    "predict_distill_student_teacher_ensemble": _distill(("prof_a", "prof_b"), pool_type="gap",
                                                         predict="student_teacher_ensemble_fwd"),
    # text tower
    "text_last": _text(pool_type="last"),
    "text_first": _text(pool_type="first"),
    "text_max": _text(pool_type="max"),
    "text_map": _text(pool_type="map"),
    "text_gap": _text(pool_type="gap"),
    "text_last_scan": _text(pool_type="last", scan=True),
    # NaFlex tower
    "naflex_gap": _naflex(pool_type="gap"),
    "naflex_max": _naflex(pool_type="max"),
    "naflex_map": _naflex(pool_type="map"),
    "naflex_gap_patchln_head": _naflex(num_classes=16, pool_type="gap", patchln_pre=True, patchln_post=True),
    "naflex_max_rep_head": _naflex(num_classes=10, pool_type="max", rep_size=16),
    "naflex_map_patchln_holes": _naflex(pool_type="map", patchln_pre=True, patchln_post=True, holes=True),
    # BERT text tower inside the two-tower step (LiT, as in the config that uses it, and fully trainable)
    "bert_lit_step": _siglip(_cfg(schedule=LIT_SCHEDULE), image=dict(IMG, pool_type="tok"),
                             text=dict(config=BERT), text_model="proj.flaxformer.bert"),
    "bert_step": _siglip(_cfg(), text=dict(config=BERT), text_model="proj.flaxformer.bert"),
    # the diagnostics path of model.apply
    "vit_apply_collect_tok_rep_head": _vit_collect(num_classes=10, pool_type="tok", rep_size=True),
    "vit_apply_collect_map": _vit_collect(pool_type="map"),
    "vit_apply_collect_gap_head": _vit_collect(num_classes=16, pool_type="gap"),
    "naflex_apply_collect_gap_holes": _naflex(num_classes=16, pool_type="gap", collect=True, holes=True),
    "naflex_apply_collect_map": _naflex(pool_type="map", collect=True),
    "text_apply_collect_last": _text(pool_type="last", collect=True),
    "text_apply_collect_map": _text(pool_type="map", collect=True),
    "bert_apply_collect": _apply(_bert_setup),
    "one_tower_apply_collect_then_no_input": _apply(lambda: _pair_setup(clippo=True), then_no_input=True),
    # model.apply on a plain numpy tree: the ad-hoc store of the geometry, re-loaded from the tree
    "text_apply_adhoc": _apply(_text_setup, adhoc=True),
    "naflex_apply_adhoc": _apply(_naflex_setup, adhoc=True),
    "bert_apply_adhoc": _apply(_bert_setup, adhoc=True),
    "two_towers_apply_adhoc_no_text": _apply(lambda: _pair_setup(text=False), adhoc=True),
    "two_towers_apply_adhoc_no_image": _apply(lambda: _pair_setup(image=False), adhoc=True),
    "one_tower_apply_adhoc": _apply(lambda: _pair_setup(clippo=True), adhoc=True),
}

ADHOC = {"text": _text_setup, "naflex": _naflex_setup, "bert": _bert_setup,
         "two_towers_no_text": lambda: _pair_setup(text=False), "two_towers_no_image": lambda: _pair_setup(image=False),
         "one_tower": lambda: _pair_setup(clippo=True)}


TABLE = os.path.join(GOLDEN, "_launches.json")      # every distinct launch of all cases, one per line


def _golden_path(name):
  return os.path.join(GOLDEN, f"{name}.json")


def _key(launch):
  return json.dumps(launch, separators=(",", ":"))


def _golden(name):
  """The golden trace of a case: <case>.json is the ordered list of line numbers into the shared table (a step repeats
  the same few dozen launches per block and micro-batch; spelled out, the traces were 1.3 MB)."""
  with open(TABLE) as f:
    table = json.load(f)
  with open(_golden_path(name)) as f:
    return [table[i] for i in json.load(f)]


def _write_goldens():
  """The table keeps the lines it has (a new case leaves the goldens of the others as they are) and grows at its end, in
  order of first appearance over the sorted cases; index lists wrapped at 40 numbers a line."""
  os.makedirs(GOLDEN, exist_ok=True)
  index = {}
  if os.path.exists(TABLE):
    with open(TABLE) as f:
      index = {_key(launch): i for i, launch in enumerate(json.load(f))}
  for name in sorted(CASES):
    trace = record(CASES[name])
    order = [index.setdefault(_key(launch), len(index)) for launch in trace]
    rows = [",".join(map(str, order[i:i + 40])) for i in range(0, len(order), 40)]
    with open(_golden_path(name), "w") as f:
      f.write("[" + ",\n".join(rows) + "]\n")
    print(f"{name}: {len(trace)} launches")
  with open(TABLE, "w") as f:
    f.write("[\n" + ",\n".join(index) + "\n]\n")
  print(f"{len(index)} distinct launches")


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace_matches_golden(name):
  got = [json.loads(_key(launch)) for launch in record(CASES[name])]     # (through JSON: tuples and lists compare alike)
  want = _golden(name)
  assert len(got) > 20, f"{name}: the dry run recorded only {len(got)} launches"
  for i, (g, w) in enumerate(zip(got, want)):
    assert g == w, f"{name}: launch {i} differs\n  got    {g}\n  golden {w}"
  assert len(got) == len(want), (f"{name}: {len(got)} launches, golden has {len(want)}; first unmatched: "
                                 f"{(got + want)[min(len(got), len(want))]}")


def test_siglip_traces_have_the_recorded_lengths():
  """The six SigLIP schemes, counted on the commit the goldens were recorded on."""
  names = ("siglip_single", "siglip_mb_keep_all_full", "siglip_mb_keep_all_light", "siglip_mb_keep_1_g",
           "siglip_mb_keep_0_full", "siglip_mb_keep_all_true_bf16")
  lengths = [len(_golden(name)) for name in names]
  assert lengths == [174, 594, 594, 744, 794, 650], lengths


def test_a_recording_is_a_function_of_the_code_alone():
  """Two recordings of one case in one process are equal, and each carries the one-off bv_ctx_set_workspace."""
  a, b = record(CASES["siglip_single"]), record(CASES["siglip_single"])
  assert a == b
  assert sum(launch[0] == "bv_ctx_set_workspace" for launch in a) == 1


@pytest.mark.parametrize("name", sorted(ADHOC))
def test_adhoc_apply_reloads_the_tree_every_call(name):
  """What tests/test_advice_r1_cpu.py asserts for the ViT, for every other model: two different plain trees and an
  in-place edit of one each reach the device store, and only one store per geometry is kept."""
  with dry_run([]):
    m, ref, inputs = ADHOC[name]()
    tree_a = _plain(ref)
    tree_b = u.tree_map(lambda v: v + 1.0, tree_a)
    _apply_adhoc(m, tree_a, *inputs)
    stores = [v for k, v in m._execs.items() if k[0] == "adhoc"]
    assert len(stores) == 1
    st = stores[0]
    for leaf, want in flatten_tree(tree_a).items():
      assert torch.equal(st.leaf(leaf), torch.from_numpy(want)), leaf
    _apply_adhoc(m, tree_b, *inputs)
    flat_b = flatten_tree(tree_b)
    for leaf, want in flat_b.items():
      assert torch.equal(st.leaf(leaf), torch.from_numpy(want)), leaf
    leaf = sorted(flat_b)[-1]
    flat_b[leaf][...] = 7.0
    _apply_adhoc(m, tree_b, *inputs)
    assert bool((st.leaf(leaf) == 7.0).all())
    assert len([k for k in m._execs if k[0] == "adhoc"]) == 1
  ops._contexts.clear()


def test_one_tower_apply_without_inputs_reports_only_t():
  """one_tower.py:53-69: neither an image nor a text - no embeddings, `out` holds the temperature alone."""
  with dry_run([]):
    m, store, _ = _pair_setup(clippo=True)
    zimg, ztxt, out = m.apply({"params": store.tree()}, None, None)
  ops._contexts.clear()
  assert zimg is None and ztxt is None and sorted(out) == ["t", "t/parameter"]
  assert torch.equal(out["t/parameter"], store.leaf("t")) and torch.equal(out["t"], torch.exp(store.leaf("t")))


if __name__ == "__main__":
  if "--write" in sys.argv:
    _write_goldens()
