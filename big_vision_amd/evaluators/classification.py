"""Evaluator for the classification task on the libbveval kernel.

Mirrors big_vision/evaluators/classification.py: `Evaluator(predict_fn, loss_name, label_key='labels', ...)` (:57-63)
and `run(train_state)` (:65-76), which yields ('prec@1', ncorrect / nseen) and ('loss', loss / nseen).  Kept: names,
the metric names and their order, the weight of an example (`_mask` times the row maximum of its labels, :41), the
AttributeError of `getattr(u, loss_name)` on an unknown loss.

New: the per-batch arithmetic of `_eval_fn` (:37-53: masked loss, argmax, label at the argmax, three sums) is ONE launch
of `bv_eval_classify` (include/bveval.h) that adds into an fp64 [3] accumulator on the device.  The reference fetches
three scalars per batch (`jax.device_get`, :70); here a whole evaluation copies to the host ONCE, after the last
batch, and `process_sum` over the hosts is one all-reduce of that accumulator (`comm`, a dp.Comm).

The reference reads a TFDS split through its input pipeline (`common.eval_input_pipeline`, out of scope here).  Like
this repository's other evaluators, this one consumes `batches`: an iterable (re-iterated by every `run`) of in-memory
dicts of tensors that carry the images for `predict_fn`, the labels under `label_key` ([b, C], one- or multi-hot) and
a `_mask` entry [b] (1 = a real example, 0 = padding of the last batch).
"""
import torch

from big_vision_amd import _lib
from big_vision_amd import ops

# Kept for configs and tools that read it (classification.py:28); the pmap / jit distinction has no meaning here.
API = "jit"


class Evaluator:
  """Classification evaluator."""

  def __init__(self, predict_fn, loss_name, label_key="labels", batches=(), comm=None, **kw):
    """**kw: what `common.from_config` passes on from a reference config (`data`, `pp_fn`, `batch_size`, ...): input
    pipeline settings, kept for inspection in `self.pipeline_kw` and not acted upon."""
    if loss_name not in _lib.EVAL_LOSSES:
      raise AttributeError(f"module 'big_vision.utils' has no attribute '{loss_name}' "
                           f"(losses of the evaluation kernel: {sorted(_lib.EVAL_LOSSES)})")
    self.predict_fn, self.loss_name, self.label_key = predict_fn, loss_name, label_key
    self.batches, self.comm, self.pipeline_kw = batches, comm, kw

  def run(self, train_state):
    """Yields ('prec@1', ncorrect / nseen) and ('loss', loss / nseen) over all batches."""
    acc = None                                     # fp64 [3] on the device: ncorrect, loss, nseen
    for batch in self.batches:
      inputs = {k: v for k, v in batch.items() if k not in (self.label_key, "_mask")}
      logits = self.predict_fn(train_state, inputs)[0].to(torch.float32).contiguous()
      labels, mask = (torch.as_tensor(batch[k]).to(device=logits.device, dtype=torch.float32).contiguous()
                      for k in (self.label_key, "_mask"))
      # the first launch creates the accumulator, every later one adds into it
      acc = ops.eval_classify(self.loss_name, logits, labels, mask, acc=acc)
    if acc is None:
      raise ValueError("classification evaluator: `batches` is empty")
    if self.comm is not None:
      self.comm.all_reduce_scalars_(acc)           # common.process_sum
    ncorrect, loss, nseen = acc.cpu().tolist()     # the evaluation's one copy to the host
    yield ("prec@1", ncorrect / nseen)
    yield ("loss", loss / nseen)
