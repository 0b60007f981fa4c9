"""Evaluator that saves the inputs and outputs of a prediction function.

Mirrors big_vision/evaluators/save.py: `run(train_state)` (:90-121) formats `outfile` with the work directory and the
optimizer's step count, runs `predict_fn(train_state, batch)` on every batch, keeps the rows with `_mask == 1` of every
leaf of `{"inputs": batch without _mask, "outputs": result}`, concatenates them over the batches along axis 0 and
writes ONE compressed .npz.  It yields nothing and is still a generator, so a loop over `run` drives it like any other
evaluator.  Example entry of `config.evals`:

    config.evals.save_pred = dict(type="save", outfile="{workdir}/inference-{step:09d}.npz", pred_kw=dict(collect=False))

and to look at the file:

    results = utils.load_checkpoint_np("<outfile>")
    inputs, outputs = results["inputs"], results["outputs"]

The file is written by `utils.save_params_npz`, the writer of this repository's checkpoints: keys are the `/`-joined
leaf names (`inputs/image`, `outputs/0`, `outputs/1/pre_logits`, ...; a tuple's members are named "0", "1", ...; `None`
leaves do not exist), bf16 leaves are held as 2-byte values and widen back exactly on load.  Every leaf must be
per-example, i.e. have the batch as its leading axis: ask a model for its pooled outputs only (`collect=False`).

`step` is `bv_optax.get_count(train_state["opt"])`, or 0 for a state without an optimizer (tools/eval_only.py hands
the bare parameters to `run`).  The reference reads the work directory from its command-line flags; here it is the
`workdir` argument or attribute.

Host copies.  The reference fetches every batch as soon as it is computed (`jax.device_get`, :102).  Here every leaf is
copied to pinned host memory with a non-blocking copy on the current stream, the next batch's forward is enqueued
right behind it, and the stream is synchronised ONCE, before the rows are selected and concatenated on the host.  The
pinned buffers of all batches are alive until then: an evaluation holds its whole output in host memory, as the
reference's list of fetched batches does.

Like this repository's other evaluators, this one consumes `batches`: an iterable (re-iterated by every `run`) of
in-memory dicts of tensors with a `_mask` entry [b] (1 = a real example, 0 = padding of the last batch).
"""
import torch

from big_vision_amd import optax as bv_optax
from big_vision_amd import utils as u

# Kept for configs and tools that read it (save.py:32); the pmap / jit distinction has no meaning here.
API = "jit"


def _to_host(t):
  """`t` on the host: a device tensor through a non-blocking copy into pinned memory (valid after the stream is
  synchronised), anything else as a tensor."""
  t = torch.as_tensor(t)
  if not t.is_cuda:
    return t
  host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
  return host.copy_(t, non_blocking=True)


class Evaluator:
  """Save the inputs and outputs of predict_fn for all real examples."""

  def __init__(self, predict_fn, outfile, batches=(), workdir=None, **kw):
    """**kw: what `common.from_config` passes on from a reference config (`data`, `pp_fn`, `batch_size`, ...): input
    pipeline settings, kept for inspection in `self.pipeline_kw` and not acted upon."""
    self.predict_fn, self.outfile = predict_fn, outfile
    self.batches, self.workdir, self.pipeline_kw = batches, workdir, kw

  def run(self, train_state):
    """A generator without items: the file is written when it is iterated, like every evaluator's work."""
    self.save(train_state)
    yield from ()

  def save(self, train_state):
    """Computes all predictions and saves them, with their inputs; returns the name of the file."""
    opt = train_state.get("opt") if hasattr(train_state, "get") else None
    step = 0 if opt is None else int(bv_optax.get_count(opt, jittable=True))
    outfile = self.outfile.format(workdir=self.workdir, step=step)

    names, fetched = None, []
    for batch in self.batches:
      out = {"inputs": {k: v for k, v in batch.items() if k != "_mask"}, "outputs": self.predict_fn(train_state, batch)}
      flat, _ = u.tree_flatten_with_names(out)
      if names is None:
        names = [n for n, _ in flat]
      elif [n for n, _ in flat] != names:
        raise ValueError(f"save evaluator: a batch has the leaves {[n for n, _ in flat]} after {names}")
      fetched.append((_to_host(batch["_mask"]), [_to_host(v) for _, v in flat]))
    if names is None:
      raise ValueError("save evaluator: `batches` is empty")
    if torch.cuda.is_available():
      torch.cuda.current_stream().synchronize()    # the evaluation's one wait for the device

    rows = []
    for mask, leaves in fetched:
      keep = mask.reshape(-1) == 1
      for name, leaf in zip(names, leaves):
        if leaf.dim() == 0 or leaf.shape[0] != keep.shape[0]:
          raise ValueError(f"save evaluator: leaf '{name}' of shape {tuple(leaf.shape)} is not per-example "
                           f"(batch of {keep.shape[0]})")
      rows.append([leaf[keep] for leaf in leaves])
    u.save_params_npz(outfile, u.recover_tree(names, [torch.cat(parts, 0) for parts in zip(*rows)]), compressed=True)
    return outfile
