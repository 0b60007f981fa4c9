"""fp64 restatement of the reference's bidirectional contrastive loss and of the contrastive evaluator's sums, the
inputs of the contrastive-evaluator tests, and the rounding-error bound the GPU results are held to.

The reference point is `masked64`: utils.py:246-273 of the reference at reduction=False, restated LITERALLY - the mask
turns every logit of a padded row or column into -inf (:254-256), the padded losses are zeroed (:264), `ncorrect` is
the argmax over axis 1 against the own index (:272) - never the removed-rows shortcut the product takes, and never a
kernel output.  `eval_sums64` is evaluators/proj/image_text/contrastive.py:60-62 on top of it.

Bound of a direction's loss sum (u = 2^-24, nothing fitted to GPU output):
  * a logit is an E-term fp32 dot product scaled by t: |error| <= delta = gamma_E |t| ||zi|| ||zt||,
    gamma_E = E u / (1 - E u);
  * log-sum-exp moves by at most the largest logit error of the row and the own logit by its own: a row loss moves by
    at most 2 delta (delta taken over the row's columns);
  * bv_eval_classify adds what tests/_eval_bounds.py states for it on these logits and labels (`loss_bound`, summed by
    `sum_bound`), imported from there.
"""
import torch

import _eval_bounds as B

F64 = torch.float64
U = 2.0 ** -24


def gamma(E):
  return E * U / (1.0 - E * U)


# ------------------------------------------------------- fp64 restatement ----
def masked64(zimg, ztxt, t, mask=None):
  """utils.py:246-273, reduction=False, fp64.  Returns (l [b], ncorrect bool [b], logits [b, b])."""
  zi, zt = torch.as_tensor(zimg).to(F64), torch.as_tensor(ztxt).to(F64)
  logits = zi @ zt.T * float(t)                                              # :249
  if mask is not None:
    mask = torch.as_tensor(mask) != 0
    exclude = ~mask                                                          # :254
    exclude = exclude[:, None] | exclude[None, :]                            # :255
    logits = torch.where(exclude, torch.full_like(logits, -float("inf")), logits)   # :256
  l1 = -torch.diagonal(torch.log_softmax(logits, 1))                         # :259
  l2 = -torch.diagonal(torch.log_softmax(logits, 0))                         # :260
  l = 0.5 * (l1 + l2)                                                        # :261
  if mask is not None:
    l = torch.where(mask, l, torch.zeros_like(l))                            # :264
  ncorrect = B.first_argmax(logits) == torch.arange(logits.shape[0])         # :272
  return l, ncorrect, logits


def eval_sums64(zimg, ztxt, t, mask):
  """contrastive.py:60-62 for one device: (c, l, n) = sums of ncorrect * mask, losses * mask, mask."""
  l, nc, _ = masked64(zimg, ztxt, t, mask)
  m = (torch.as_tensor(mask) != 0).to(F64)
  return float((nc.to(F64) * m).sum()), float((l * m).sum()), float(m.sum())


def removed64(zimg, ztxt, t, mask):
  """The product's route in fp64: the padded examples leave, the v x v problem carries no mask.  (c, l, n)."""
  keep = torch.as_tensor(mask) != 0
  if not bool(keep.any()):
    return 0.0, 0.0, 0.0
  l, nc, _ = masked64(torch.as_tensor(zimg)[keep], torch.as_tensor(ztxt)[keep], t)
  return float(nc.sum()), float(l.sum()), float(keep.sum())


def block64(zimg, ztxt, t, row_offset=0, cols=None):
  """One call of ops.contrastive_eval in fp64: for each direction the tests/_eval_bounds.py reference dict of
  softmax_xent on logits [v, B] against the identity block at row_offset, plus the logits.  Returns (it, ti)."""
  zi, zt = zimg.to(F64), ztxt.to(F64)
  zi_all, zt_all = (zi, zt) if cols is None else (c.to(F64) for c in cols)
  v, Bc = zi.shape[0], zi_all.shape[0]
  eye = torch.zeros((v, Bc), dtype=F64)
  eye[torch.arange(v), row_offset + torch.arange(v)] = 1.0
  out = []
  for a, b in ((zi, zt_all), (zt, zi_all)):
    logits = a @ b.T * float(t)
    ref = B.classify64("softmax_xent", logits, eye)
    ref["logits"], ref["labels"] = logits, eye
    ref["delta"] = gamma(a.shape[1]) * abs(float(t)) * a.norm(dim=1) * b.norm(dim=1).max()    # [v]
    out.append(ref)
  return out


def direction_bound(ref):
  """Bound of a direction's loss sum: 2 delta per row for the GEMM, plus the evaluation kernel's own."""
  return B.sum_bound(ref, 2.0 * ref["delta"] + B.loss_bound("softmax_xent", ref["logits"], ref["labels"]))


# ----------------------------------------------------------------- inputs ----
def unit(x):
  return x / x.norm(dim=1, keepdim=True)


def planted(v, E, seed, eps=0.05, wrong_every=0):
  """Unit-norm fp32 (zimg, ztxt): zimg[i] sits eps away from ztxt[target(i)], target(i) = i, or with wrong_every = k
  the next example for every k-th row (a confident mistake).  Random in every other respect."""
  g = torch.Generator().manual_seed(seed)
  zt = unit(torch.randn((v, E), generator=g, dtype=F64))
  target = torch.arange(v)
  if wrong_every and v > 1:
    target = torch.where(target % wrong_every == wrong_every - 1, (target + 1) % v, target)
  zi = unit(zt[target] + eps * unit(torch.randn((v, E), generator=g, dtype=F64)))
  return zi.float(), zt.float()


def margin_ok(logits, t, delta):
  """Every row's largest logit exceeds its runner-up by more than 4 delta (so by more than 4 delta / |t| in cosine): an
  argmax no rounding within the bound can move.  logits: fp64 [v, B]; delta: [v]."""
  if logits.shape[1] == 1:
    return True
  top = logits.topk(2, dim=1).values
  return bool(((top[:, 0] - top[:, 1]) > 4.0 * delta).all())


def dyadic_with_ties(v, E, seed):
  """Multiples of 1/8 in [-1/2, 1/2] (every dot product is exact in fp32 and fp64 alike, so both see the same ties),
  with every fourth caption an exact copy of its predecessor: rows i - 1 and i tie on columns i - 1 and i."""
  g = torch.Generator().manual_seed(seed)
  zt = torch.randint(-4, 5, (v, E), generator=g).float() / 8
  zt[3::4] = zt[2::4][:zt[3::4].shape[0]]
  zi = zt.clone()
  zi[::5] = torch.randint(-4, 5, zi[::5].shape, generator=g).float() / 8
  return zi, zt
