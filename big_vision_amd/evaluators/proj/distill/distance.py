"""Distillation distances and their evaluator on the libbvdistill kernels.

Mirrors big_vision/evaluators/proj/distill/distance.py: `dist` (:35-67), `get_dist_fn` (:70-72) and `Evaluator`
(:102-151).  Kept: names, signatures and defaults of `dist` / `get_dist_fn`, the metric names `<k=v_...>/all`,
`/avg`, `/min`, `/max`, the AssertionError on an unknown kind.  New: every distance is ONE launch of
`bv_distill_dist` (include/bvdistill.h) on fp32 GPU logits; the reference reads a TFDS dataset through its input
pipeline (out of scope here) - this evaluator consumes an iterable of in-memory batches that carry `_mask`, like the
repository's other evaluators.
"""
import functools

import numpy as np
import torch

from big_vision_amd import _lib
from big_vision_amd import ops


def dist(student, teacher, kind, feat_axis=-1, epsilon=1e-12, t=1, ls=0.0, k=1):
  """Distance function used for distillation: per-example values, fp32 [b] (`agree`: 0 / 1)."""
  assert kind in _lib.DISTILL_KINDS, f"Unknown kind of distance {kind}."
  assert student.shape == teacher.shape, (tuple(student.shape), tuple(teacher.shape))
  if feat_axis not in (-1, student.dim() - 1):
    student, teacher = student.movedim(feat_axis, -1), teacher.movedim(feat_axis, -1)
  lead = student.shape[:-1]
  flat = lambda x: x.to(torch.float32).reshape(-1, x.shape[-1]).contiguous()
  rows, _ = ops.distill_dist(kind, flat(student), flat(teacher), per_row=True, t=t, ls=ls, eps=epsilon, k=k)
  return rows.view(lead)


@functools.lru_cache(None)
def get_dist_fn(**kw):
  return functools.partial(dist, **kw)


def _tree_get(tree, name):
  for part in name.split("/"):
    tree = tree[part]
  return tree


class Evaluator:
  """Distillation distance evaluator.

  student_teacher_fwd(train_state, batch) -> ((_, out_s), (_, out_t)), e.g. the trainer's `student_<teacher>_fwd`;
  batches: an iterable (re-iterated by every `run`) of dicts of tensors with a `_mask` entry [b] (1 = a real example);
  distances: a sequence of keyword dicts for `dist`, e.g. [dict(kind="kl"), dict(kind="agree", k=5)]."""

  def __init__(self, student_teacher_fwd, batches, distances, what=("logits", "logits")):
    self.fwd, self.batches, self.what = student_teacher_fwd, batches, tuple(what)
    self.dist_fns = tuple(get_dist_fn(**d) for d in distances)
    self.dist_names = ["_".join(f"{k}={v}" for k, v in d.items()) for d in distances]

  def run(self, train_state):
    """Yields (metric name, value) over the unmasked examples of all batches."""
    all_ds = [[] for _ in self.dist_names]
    for batch in self.batches:
      batch = dict(batch)
      mask = np.asarray(torch.as_tensor(batch.pop("_mask")).cpu()) == 1
      (_, out_s), (_, out_t) = self.fwd(train_state, batch)
      # non-vectors (feature maps) are flattened, b ... -> b (...)
      rs, rt = (_tree_get(o, w).flatten(1) for o, w in zip((out_s, out_t), self.what))
      for i, fn in enumerate(self.dist_fns):
        all_ds[i].append(fn(rs, rt).detach().cpu().numpy()[mask])
    stats = (("all", lambda v: v), ("avg", np.mean), ("min", np.min), ("max", np.max))
    for name, parts in zip(self.dist_names, all_ds):
      values = np.concatenate(parts)
      for stat, fn in stats:
        yield f"{name}/{stat}", fn(values)
