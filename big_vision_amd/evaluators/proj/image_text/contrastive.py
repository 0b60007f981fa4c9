"""Evaluator for the contrastive task: held-out bidirectional contrastive loss and in-batch accuracy.

DON'T COMPARE ACROSS RUNS, use for training health monitoring only: `ncorrect_minibatch` is a function of the batch
size and is biased low when a batch holds the same caption twice (the reference's own warning, contrastive.py:17-25).

Mirrors big_vision/evaluators/proj/image_text/contrastive.py: `Evaluator(predict_fn, ..., use_global_batch, ...,
label_key='labels')` (:71-82) and `run(params)` (:84-99), which yields ('ncorrect_minibatch', c / nseen) and
('loss', l / nseen), with `_eval_fn` (:51-63) on `u.bidirectional_contrastive_loss(zimg, ztxt, extras["t"], mask,
reduction=False)` (utils.py:246-273).  Followed to the line:
  * the logits are t zimg ztxt^T (utils.py:249); the per-example loss is 0.5 (NLL of row i of the logits under a
    softmax over axis 1 + NLL of column i under a softmax over axis 0) (:259-261);
  * `ncorrect` counts ONE direction only: argmax over axis 1 (image -> text) equal to the example's own index (:272),
    jnp.argmax's first maximum winning a tie;
  * the mask removes a padded example from BOTH the rows and the columns: every logit whose row or column is padded
    becomes -inf (:254-256), the padded examples' losses are zeroed (:264), and the evaluator multiplies losses and
    `ncorrect` by the mask once more before it sums (contrastive.py:60-62).

Removed rows equal the masked formula.  A -inf logit contributes exp(-inf) = 0 to every log-sum-exp and never wins an
argmax against a finite logit, and a real example's row (column) keeps its own finite diagonal entry.  So for the real
examples the masked B x B problem IS the v x v problem on the real rows and columns alone - the same sets of finite
terms, hence the same values - while the padded examples contribute exactly 0.  This evaluator therefore selects the
rows with `_mask != 0` (an index select) and runs no masking arithmetic at all; tests/test_contrastive_eval_cpu.py
proves the equality in fp64 against the literal masked formula.

Device arithmetic per batch (`ops.contrastive_eval`, shared with `utils.bidirectional_contrastive_loss`): two
`bv_sgemm_strided` (t zimg ztxt^T and, operands swapped, t ztxt zimg^T: no transpose) and two `bv_eval_classify`
("softmax_xent" against a cached identity block), which add into two fp64 [3] accumulators that live on the device for
the whole `run`.  The temperature goes in as the GEMM's device-side `log_alpha` (the model's `t/parameter`), so no
batch waits for the host; the evaluation's one copy to the host is the 48 bytes of the two accumulators, at the end.

`use_global_batch` (contrastive.py:54-55 all-gathers zimg, ztxt and mask over the devices): with a `comm` of more than
one rank the embeddings are all-gathered (`dp.Comm.all_gather_rows`, the SigLIP step's path) and every rank evaluates
ITS OWN real rows against the gathered real columns, in both directions, its identity block starting at its row offset
among the real examples.  The reference computes the whole gathered problem on every device and psums it, which counts
everything `size` times in c, l and n alike; the ratios that `run` yields are the same.  The gathered masks of ALL
batches are exchanged in one collective before the first batch and read once (the shapes of the launches depend on
them), so that mode costs a second, `4 size b` bytes per batch, host copy per evaluation.  With
`use_global_batch=False` every rank's batch is its own universe; either way the accumulators are all-reduced once, at
the end.  With `comm=None` or one rank the two settings are the same thing.

The reference reads a TFDS split through its input pipeline (out of scope here).  Like this repository's other
evaluators, this one consumes `batches`: an iterable (re-iterated by every `run`) of in-memory dicts with `image`, the
tokens under `label_key` and `_mask` [b] (1 = a real example, 0 = padding).  `_mask` is host data (numpy or a CPU
tensor): it decides shapes; one held on the device is copied to the host batch by batch.
"""
import torch
import torch.distributed as dist

from big_vision_amd import ops
from big_vision_amd import utils as u

# Kept for configs and tools that read it; the reference's evaluator is pmap-based, a distinction without meaning here.
API = "jit"


class Evaluator:
  """Contrastive evaluator."""

  def __init__(self, predict_fn, use_global_batch, label_key="labels", batches=(), comm=None, **kw):
    """predict_fn(train_state, {"image": ..., "labels": ...}) -> (zimg [b, E], ztxt [b, E], out) with out["t"] (and,
    from this repository's models, out["t/parameter"] = log t), the convention of the retrieval evaluator.
    **kw: what `common.from_config` passes on from a reference config (`data`, `pp_fn`, `batch_size`, `cache_final`,
    `cache_raw`, `prefetch`): input pipeline settings, kept for inspection in `self.pipeline_kw` and not acted upon."""
    self.predict_fn, self.use_global_batch, self.label_key = predict_fn, bool(use_global_batch), label_key
    self.batches, self.comm, self.pipeline_kw = batches, comm, kw

  def _embed(self, train_state, batch):
    zimg, ztxt, out = self.predict_fn(train_state, {"image": batch["image"], "labels": batch[self.label_key]})
    zimg, ztxt = (z.to(torch.float32).contiguous() for z in (zimg, ztxt))
    return zimg, ztxt, out["t"], out.get("t/parameter")

  def run(self, train_state):
    """Yields ('ncorrect_minibatch', c / nseen) and ('loss', l / nseen) over all batches."""
    comm = self.comm
    gather = self.use_global_batch and comm is not None and comm.size > 1
    batches = self.batches
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    if gather:
      # every rank's masks of every batch in ONE collective and one read: [size * b, number of batches]
      batches = list(batches)
      if batches:
        local = torch.stack([u.host_mask(b["_mask"]) for b in batches], 1).to(torch.float32)
        if dist.get_backend(comm.group) == "nccl":   # RCCL moves device memory only
          local = local.to(device)
        masks_all = comm.all_gather_rows(local).cpu() != 0
    acc, nbatches = None, 0                          # fp64 [2, 3] on the device: (hits, loss, nseen) per direction
    for j, batch in enumerate(batches):
      nbatches += 1
      mask = u.host_mask(batch["_mask"])
      mask_cols = masks_all[:, j] if gather else mask
      if not bool(mask_cols.any()):                  # nothing real in this batch's universe: nothing is launched
        continue
      zimg, ztxt, t, log_t = self._embed(train_state, batch)
      if acc is None:
        acc = torch.zeros((2, 3), device=zimg.device, dtype=torch.float64)
      if gather:
        b = mask.numel()
        cols = tuple(u.real_rows(comm.all_gather_rows(z), mask_cols) for z in (zimg, ztxt))
        row_offset, v = int(mask_cols[:comm.rank * b].sum()), int(mask.sum())
        zimg, ztxt = (c[row_offset:row_offset + v] for c in cols)     # this rank's real rows: a contiguous run
      else:
        cols, row_offset = None, 0
        zimg, ztxt = u.real_rows(zimg, mask), u.real_rows(ztxt, mask)
      ops.contrastive_eval(zimg, ztxt, t, acc[0], acc[1], row_offset=row_offset, cols=cols, log_t=log_t)
    if nbatches == 0:
      raise ValueError("contrastive evaluator: `batches` is empty")
    if acc is None:                                  # every example of this rank was padding; others may have had some
      acc = torch.zeros((2, 3), device=device, dtype=torch.float64)
    if comm is not None:
      comm.all_reduce_scalars_(acc)                  # psum of c, l, n (contrastive.py:60-62): both accumulators, once
    (c, l_it, nseen), (_, l_ti, _) = acc.cpu().tolist()   # the evaluation's one copy of its results to the host
    l = 0.5 * (l_it + l_ti)
    yield ("ncorrect_minibatch", c / nseen if nseen else float("nan"))
    yield ("loss", l / nseen if nseen else float("nan"))
