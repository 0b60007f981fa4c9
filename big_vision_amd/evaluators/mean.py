"""Evaluator for the mean of per-example metrics, on the `bv_dot_f32` entry point.

Mirrors big_vision/evaluators/mean.py: `predict_fn(train_state, batch)` returns a dict from metric name to per-example
values of the shape of `batch["_mask"]`, and `run(train_state)` yields `(key, sum_i mask_i metric_i / sum_i mask_i)`
for every key, in the dict's order (:64-80).  It is the generic evaluator, and the one a new evaluator inherits from:
a subclass that turns a model's outputs into per-example numbers in `predict_fn` gets the accumulation, the reduction
over the ranks and the single host copy from here.  Kept: the names, the two checks of `_run_predict_fn` (:43-48: a
result that is no mapping is an AssertionError, a leaf that is not per-example a ValueError whose text begins
"Expected per-example metrics of shape"), the order of the keys, that `predict_fn` sees the whole batch (`_mask`
included).

New: the masked sum of a batch's metric is ONE launch of `ops.dot_(metric, mask, acc[k:k + 1])`, which adds
`sum(metric * mask)` into an fp64 scalar on the device; `ops.dot_(mask, mask, acc[-1:])` counts the real examples of
the batch (the mask is 0 / 1, so its square is itself).  All accumulators are one fp64 tensor of `len(metrics) + 1`
elements that lives on the device for the whole `run`, is summed over the ranks once (`comm`, a dp.Comm) and copied to
the host once, after the last batch.  The reference keeps a dict of device scalars per batch, fetches them all
(`jax.device_get`, :74) and sums them on the host.  Metrics that arrive as bf16, fp64 or integers are cast to
contiguous fp32 on the device first: `bv_dot_f32` reads fp32.

One deviation.  The reference takes `where(mask, x, 0)` (:50), so a NaN or Inf that `predict_fn` computes for a PADDING
row is dropped; the product `x * 0` keeps it as NaN and the metric's mean becomes NaN.  No entry point of the kernel
libraries selects, and finding the case would need a host synchronisation per batch, so it is not detected: a
`predict_fn` must return finite numbers for padding rows too.

Like this repository's other evaluators, this one consumes `batches`: an iterable (re-iterated by every `run`) of
in-memory dicts of tensors with a `_mask` entry [b] (1 = a real example, 0 = padding of the last batch).
"""
from collections.abc import Mapping

import torch

from big_vision_amd import ops

# Kept for configs and tools that read it (mean.py:33); the pmap / jit distinction has no meaning here.
API = "jit"


class Evaluator:
  """Report the mean of per-example metrics computed by predict_fn."""

  def __init__(self, predict_fn, batches=(), comm=None, **kw):
    """**kw: what `common.from_config` passes on from a reference config (`data`, `pp_fn`, `batch_size`, ...): input
    pipeline settings, kept for inspection in `self.pipeline_kw` and not acted upon."""
    self.predict_fn = predict_fn
    self.batches, self.comm, self.pipeline_kw = batches, comm, kw

  def run(self, train_state):
    """Yields (key, masked mean over all batches) for every key of the dict `predict_fn` returns."""
    keys, acc = None, None                         # fp64 [len(keys) + 1] on the device: the metric sums, then nseen
    for batch in self.batches:
      metrics = self.predict_fn(train_state, batch)
      assert isinstance(metrics, Mapping), "predict_fn must return a dict"
      mask = torch.as_tensor(batch["_mask"])
      for y in metrics.values():
        if tuple(y.shape) != tuple(mask.shape):
          raise ValueError(f"Expected per-example metrics of shape {tuple(mask.shape)} found "
                           f"{ {k: tuple(v.shape) for k, v in metrics.items()} }.")
      if keys is None:
        keys = list(metrics)
        device = next((torch.as_tensor(y).device for y in metrics.values()), mask.device)
        acc = torch.zeros(len(keys) + 1, device=device, dtype=torch.float64)
      elif list(metrics) != keys:
        raise ValueError(f"predict_fn returned the metrics {list(metrics)} after {keys}")
      mask = mask.to(device=acc.device, dtype=torch.float32).contiguous()
      for k, key in enumerate(keys):
        y = torch.as_tensor(metrics[key]).to(device=acc.device, dtype=torch.float32).contiguous()
        ops.dot_(y, mask, acc[k:k + 1])
      ops.dot_(mask, mask, acc[len(keys):])
    if acc is None:
      raise ValueError("mean evaluator: `batches` is empty")
    if self.comm is not None:
      self.comm.all_reduce_scalars_(acc)           # common.process_sum
    *sums, nseen = acc.cpu().tolist()              # the evaluation's one copy to the host
    for key, value in zip(keys, sums):
      yield (key, value / nseen)
