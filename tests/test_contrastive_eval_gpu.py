"""The contrastive evaluator's device side against fp64 (tests/_contrastive_bounds.py): `ops.contrastive_eval`, i.e.
two bv_sgemm_strided and two bv_eval_classify per call, then the evaluator end to end on the `mu/16` two-tower model.

Loss sums are held, per direction, to the derived bound of _contrastive_bounds.direction_bound (2 delta per row for the
fp32 GEMM, delta = gamma_E |t| ||zi|| ||zt||, plus the model tests/_eval_bounds.py states for bv_eval_classify); the
legacy rtol / atol floor of _eval_bounds is NOT granted.  Counts are exact: the inputs carry a margin of more than
4 delta between every row's best and second-best logit (checked in fp64 before the launch), or exact ties in exactly
representable arithmetic, decided by jnp.argmax's rule (the lowest index wins).

Measured on the MI355X (each case prints its figure, "[contrastive] ... err/bound"): the worst error is 1.6 % of the
bound over the kernel-level cases ((v, E) = (63, 16), t = 1, text -> image: 1.16e-5 of 7.22e-4) and 0.6 % end to end
(4.2e-6 of 7.4e-4); every count exact.
"""
import math

import pytest
import torch

import _contrastive_bounds as CB
import _eval_bounds as B

pytestmark = pytest.mark.gpu

# (v, E): below / at / above bv_sgemm_strided's MFMA thresholds (M, N >= 64, K >= 16), its 64-wide tiles and their
# remainders, a single row, and several workgroups of bv_eval_classify's wave-per-row mapping (four rows each)
SHAPES = [(1, 16), (5, 24), (63, 16), (64, 16), (67, 768), (130, 64), (257, 768)]
WORST = {"frac": 0.0}


def _launch(dev, zi, zt, t, row_offset=0, cols=None, log_t=None):
  from big_vision_amd import ops
  acc = torch.zeros((2, 3), device=dev, dtype=torch.float64)
  ops.contrastive_eval(zi.to(dev), zt.to(dev), t, acc[0], acc[1], row_offset=row_offset,
                       cols=None if cols is None else tuple(c.to(dev) for c in cols), log_t=log_t)
  return acc.cpu()


def _check_losses(got, refs, name, extra_delta=0.0):
  for k, (d, ref) in enumerate(zip(("img->txt", "txt->img"), refs)):
    bound = CB.direction_bound(dict(ref, delta=ref["delta"] + extra_delta))
    err = abs(got[k, 1].item() - ref["loss_sum"])
    frac = err / bound
    WORST["frac"] = max(WORST["frac"], frac)
    print(f"[contrastive] {name} {d}: loss sum {ref['loss_sum']:.9g}, err {err:.3e}, bound {bound:.3e}, "
          f"err/bound {frac:.3f} (worst so far {WORST['frac']:.3f})")
    assert err <= bound, (name, d, err, bound)


@pytest.mark.parametrize("t", [1.0, 10.0, 100.0])
@pytest.mark.parametrize("v,E", SHAPES)
def test_planted_positives(dev, v, E, t):
  """Every positive pair beats every other pair of its row and of its column by more than 4 delta: no row may be
  excluded from the count, which must be v in both directions; the loss sums within the derived bound."""
  zi, zt = CB.planted(v, E, seed=v * 1000 + E)
  refs = CB.block64(zi, zt, t)
  for ref in refs:
    assert CB.margin_ok(ref["logits"], t, ref["delta"]) and ref["ncorrect"] == v     # the planted margin holds in fp64
  got = _launch(dev, zi, zt, t)
  assert got[:, 0].tolist() == [v, v] and got[:, 2].tolist() == [v, v]
  _check_losses(got, refs, f"planted v={v} E={E} t={t:g}")


@pytest.mark.parametrize("v,E", SHAPES[1:])
def test_planted_mistakes(dev, v, E):
  """Every third image sits next to the WRONG caption, with the same margin: the image -> text count (the reference's
  `ncorrect`, utils.py:272) must be the fp64 count exactly, and is not v."""
  t = 10.0
  zi, zt = CB.planted(v, E, seed=v * 1000 + E + 1, wrong_every=3)
  refs = CB.block64(zi, zt, t)
  assert CB.margin_ok(refs[0]["logits"], t, refs[0]["delta"]) and 0 < refs[0]["ncorrect"] < v
  got = _launch(dev, zi, zt, t)
  assert got[0, 0].item() == refs[0]["ncorrect"] and got[:, 2].tolist() == [v, v]
  _check_losses(got, refs, f"mistakes v={v} E={E}")


def test_rank_block(dev):
  """The shape a rank launches under use_global_batch: its v rows against B > v gathered columns, the identity block
  at row_offset > 0."""
  t, Bc, off, v = 10.0, 100, 41, 37
  zi_all, zt_all = CB.planted(Bc, 24, seed=77, wrong_every=4)
  zi, zt = zi_all[off:off + v].contiguous(), zt_all[off:off + v].contiguous()
  refs = CB.block64(zi, zt, t, row_offset=off, cols=(zi_all, zt_all))
  assert CB.margin_ok(refs[0]["logits"], t, refs[0]["delta"]) and 0 < refs[0]["ncorrect"] < v
  got = _launch(dev, zi, zt, t, row_offset=off, cols=(zi_all, zt_all))
  assert got[0, 0].item() == refs[0]["ncorrect"] and got[:, 2].tolist() == [v, v]
  _check_losses(got, refs, f"rank block v={v} B={Bc} offset={off}")
  with pytest.raises(ValueError, match="outside B"):
    _launch(dev, zi, zt, t, row_offset=Bc - v + 1, cols=(zi_all, zt_all))
  z0 = torch.zeros((0, 24))
  assert _launch(dev, z0, z0, t, row_offset=3, cols=(zi_all, zt_all)).abs().sum().item() == 0     # v = 0: nothing


def _exp_delta(t, took_log=False):
  """What a device-side temperature adds to a logit's error (unit-norm embeddings): alpha = __expf(log t) carries the
  relative error (EXP0 + EXPX |log t|) u of tests/_distill_bounds.py and the product with alpha one more u; where the
  helper had to take log t itself, its fp32 rounding adds (1 + |log t|) u; all times |logit| <= |t|."""
  lt = abs(math.log(t))
  return (B.EXP0 + B.EXPX * lt + 1.0 + (1.0 + lt if took_log else 0.0)) * B.U * abs(t)


@pytest.mark.parametrize("as_log", [True, False])
def test_device_temperature(dev, as_log):
  """t on the device: as log t (the model's t/parameter, the GEMM's log_alpha) or as t itself (the helper takes its
  logarithm on the device).  Neither is read back."""
  v, E, t = 67, 768, 10.0
  zi, zt = CB.planted(v, E, seed=5, wrong_every=3)
  log_t = torch.tensor([math.log(t)], dtype=torch.float32)
  t_dev = torch.exp(log_t)
  refs = CB.block64(zi, zt, float(torch.exp(log_t.double())))
  got = (_launch(dev, zi, zt, None, log_t=log_t.to(dev)) if as_log else _launch(dev, zi, zt, t_dev.to(dev)))
  assert got[0, 0].item() == refs[0]["ncorrect"]
  _check_losses(got, refs, f"device t ({'log t' if as_log else 't'})", extra_delta=_exp_delta(t, took_log=not as_log))


def test_exact_ties(dev):
  """Dyadic embeddings (every logit exact in fp32 and fp64) with duplicated captions: the count is decided by the
  argmax order - the lowest index wins (utils.py:272, jnp.argmax) - and must be the fp64 count exactly."""
  v, E, t = 67, 16, 2.0
  zi, zt = CB.dyadic_with_ties(v, E, seed=9)
  refs = CB.block64(zi, zt, t)
  lg = refs[0]["logits"]
  ties = int(((lg == lg.max(1, keepdim=True).values).sum(1) > 1).sum())
  assert ties >= v // 4 and 0 < refs[0]["ncorrect"] < v             # ties decide rows, in both ways
  assert torch.equal(lg, (zi @ zt.T * t).double())                 # the arithmetic is exact: fp32 sees the same ties
  got = _launch(dev, zi, zt, t)
  assert got[0, 0].item() == refs[0]["ncorrect"] and got[1, 0].item() == refs[1]["ncorrect"]


# ------------------------------------------------------------- end to end ----
N, RES, SEQ, VOCAB, EMB = 8, 64, 16, 100, 32


def _model_and_state(dev):
  from big_vision_amd.compat.ml_collections import ConfigDict
  from big_vision_amd.models.proj.image_text import two_towers
  from big_vision_amd.trainers.proj.image_text import siglip
  model = two_towers.Model(image=dict(variant="mu/16", pool_type="map"), text=dict(variant="mu", vocab_size=VOCAB),
                           out_dim=(None, EMB), temperature_init=10.0, bias_init=-10.0)
  c = ConfigDict()
  c.lr, c.wd = 1e-3, 1e-2
  c.schedule = dict(decay_type="cosine", warmup_steps=2)
  c.optax_name, c.grad_clip_norm, c.total_steps = "scale_by_adam", 1.0, 10
  c.evals = {}
  c.evals.val = dict(type="proj.image_text.contrastive", use_global_batch=True, log_steps=1)
  state, _ = siglip.make_train_state(model, c, (N, RES, RES, 3), (N, SEQ), rng=0, total_steps=c.total_steps)
  store = state["params"].store
  g = torch.Generator().manual_seed(7)
  for name in store.leaf_names():                   # break the zero / unit initialisations
    if name.endswith(("bias", "scale", "cls")):
      leaf = store.leaf(name)
      leaf.add_((0.05 * torch.randn(leaf.shape, generator=g)).to(dev))
  store.mark_dirty(); store.refresh_shadow()
  return model, c, state


def test_evaluator_on_the_two_tower_model(dev):
  """Two batches of 8, the last three rows of the second masked.  The evaluator (built by from_config on the trainer's
  predict function) against the literal masked fp64 formula fed the product's own zimg / ztxt; and
  `utils.bidirectional_contrastive_loss`, batch by batch, gives the evaluator's sums bit for bit when both are handed
  the same temperature operand: they share ops.contrastive_eval, and fp64 sums of a few fp32 values of like magnitude
  are exact in any order (asserted on the values)."""
  import bv_oracle as O
  from big_vision_amd import utils as u
  from big_vision_amd.evaluators import common
  from big_vision_amd.evaluators.proj.image_text import contrastive
  from big_vision_amd.trainers.proj.image_text import siglip
  model, config, state = _model_and_state(dev)
  predict_fn = siglip.make_predict_fn(model, config)
  batches = []
  for seed, mask in ((1, torch.ones(N)), (2, torch.tensor([1.0] * (N - 3) + [0.0] * 3))):
    image, text = O.synthetic_batch(seed, N, RES, SEQ, VOCAB)
    batches.append({"image": image.to(dev), "labels": text.to(dev), "_mask": mask})
  (name, ev, logsteps, prefix), = common.from_config(config, {"predict": predict_fn})
  assert (name, logsteps, prefix) == ("val", 1, "val/") and isinstance(ev, contrastive.Evaluator)
  ev.batches = batches
  got = list(ev.run(state))
  assert [k for k, _ in got] == ["ncorrect_minibatch", "loss"]
  got = dict(got)

  # the fp64 restatement on the product's own embeddings
  c = l = n = bound = 0.0
  loose, embs = 0, []
  for b in batches:
    zimg, ztxt, out = predict_fn(state, {"image": b["image"], "labels": b["labels"]})
    assert zimg.shape == ztxt.shape == (N, EMB) and zimg.dtype == torch.float32
    t = float(torch.exp(out["t/parameter"].double().cpu().reshape(-1)[0]))
    zi, zt = zimg.cpu(), ztxt.cpu()
    embs.append((zimg, ztxt, out))
    cb, lb, nb = CB.eval_sums64(zi, zt, t, b["_mask"])
    c, l, n = c + cb, l + lb, n + nb
    keep = b["_mask"] != 0
    refs = CB.block64(zi[keep], zt[keep], t)
    for ref in refs:
      ref["delta"] = ref["delta"] + _exp_delta(t)
    bound += 0.5 * (CB.direction_bound(refs[0]) + CB.direction_bound(refs[1]))
    top = refs[0]["logits"].topk(2, dim=1).values
    loose += int(((top[:, 0] - top[:, 1]) <= 4.0 * refs[0]["delta"]).sum())     # rows rounding may decide
  assert n == 2 * N - 3
  err = abs(got["loss"] * n - l)
  print(f"[contrastive] two towers: loss {got['loss']:.7f} vs fp64 {l / n:.7f}, err of the sum {err:.3e}, bound "
        f"{bound:.3e}, err/bound {err / bound:.3f}; ncorrect {got['ncorrect_minibatch'] * n:.0f} vs {c:.0f}, "
        f"{loose} rows without margin")
  assert err <= bound
  assert abs(got["ncorrect_minibatch"] * n - c) <= loose + 1e-9

  # utils.bidirectional_contrastive_loss on the same launch sequence: the evaluator's sums, bit for bit
  def predict_t_only(train_state, batch):
    zimg, ztxt, out = predict_fn(train_state, batch)
    return zimg, ztxt, {"t": out["t"]}
  ev_t = contrastive.Evaluator(predict_t_only, False, batches=batches)
  got_t = dict(ev_t.run(state))
  ls, cs = [], []
  for b, (zimg, ztxt, out) in zip(batches, embs):
    lb, meas = u.bidirectional_contrastive_loss(zimg, ztxt, out["t"], b["_mask"], reduction=False)
    assert lb.shape == (N,) and meas["ncorrect"].shape == (N,) and meas["ncorrect"].dtype == torch.bool
    keep = (b["_mask"] != 0).to(dev)
    assert bool((lb[~keep] == 0).all())
    ls.append(lb[keep].cpu())
    cs.append(meas["ncorrect"][keep].cpu())
    lr, mr = u.bidirectional_contrastive_loss(zimg, ztxt, out["t"], b["_mask"], reduction=True)
    assert lr.item() == pytest.approx(lb.sum().item() / (keep.sum().item() + 1e-8), rel=1e-12)
    assert mr["ncorrect"].item() == pytest.approx(cs[-1].sum().item() / (keep.sum().item() + 1e-8), rel=1e-12)
  ls, cs = torch.cat(ls), torch.cat(cs)
  assert ls.min() > 0 and ls.max() / ls.min() < 2.0 ** 20        # like magnitude: every partial sum is exact in fp64
  assert got_t["loss"] == ls.sum().item() / n
  assert got_t["ncorrect_minibatch"] == cs.sum().item() / n
  assert abs(got_t["loss"] - got["loss"]) * n <= bound           # t and log t as operands differ by rounding only
