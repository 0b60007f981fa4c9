"""The classification evaluator end to end on the GPU: the tiny `mu/16` ViT (width 32, depth 1), 10 classes, 32 px
images, two batches of 8 with the last three rows of the second one masked (the padding of a last batch).

  * `train.make_predict_fn` gives, bit for bit, the logits of the training forward at train=False (the model has no
    dropout, so the two run the same kernels on the same operands);
  * the evaluator's `prec@1` and `loss` equal tests/_eval_bounds.py::classify64 applied to those logits: the counts
    exactly, the loss within max(legacy, summed rounding model) / nseen;
  * an evaluation between two training steps changes no bit of the train state (fp32 master, bf16 shadow, gradient
    buffer, optimizer state), and step + evaluation + step leaves the parameters of step + step.
"""
import pytest
import torch

import _eval_bounds as B

pytestmark = pytest.mark.gpu

N, RES, CLASSES = 8, 32, 10
MODEL = dict(variant="mu/16", pool_type="gap")


def _config(loss):
  from big_vision_amd.compat.ml_collections import ConfigDict
  c = ConfigDict()
  c.lr, c.wd = 1e-3, 1e-4
  c.schedule = dict(warmup_steps=2, decay_type="cosine")
  c.optax_name, c.optax = "scale_by_adam", dict(mu_dtype="bfloat16")
  c.grad_clip_norm, c.total_steps = 1.0, 10
  c.model_name, c.model, c.num_classes, c.loss = "vit", dict(MODEL), CLASSES, loss
  c.evals = {}
  c.evals.val = dict(type="classification", loss_name=loss, log_steps=1)
  return c


def _state(dev, config, model):
  """A train state with the zero / unit initialisations broken (the head kernel is zero-init: every logit would be 0)."""
  from big_vision_amd import train
  state, _ = train.make_train_state(model, config, (N, RES, RES, 3), rng=0, total_steps=config.total_steps)
  store = state["params"].store
  g = torch.Generator().manual_seed(3)
  for name in store.leaf_names():
    leaf = store.leaf(name)
    std = 0.5 if name.endswith("kernel") and "head" in name else (0.05 if name.endswith(("bias", "scale")) else 0.0)
    if std:
      leaf.add_((std * torch.randn(leaf.shape, generator=g)).to(dev))
  store.mark_dirty(); store.refresh_shadow()
  return state


def _batches(dev, loss):
  g = torch.Generator().manual_seed(5)
  out = []
  for mask in (torch.ones(N), torch.tensor([1.0] * (N - 3) + [0.0] * 3)):
    labels = torch.nn.functional.one_hot(torch.randint(0, CLASSES, (N,), generator=g), CLASSES).float()
    if loss == "sigmoid_xent":
      labels[1, torch.randint(0, CLASSES, (2,), generator=g)] = 1.0       # a multi-hot row
    out.append({"image": (torch.rand((N, RES, RES, 3), generator=g) * 2 - 1).to(dev), "labels": labels.to(dev),
                "_mask": mask.to(dev)})
  return out


def _snapshot(state):
  from big_vision_amd import utils as u
  store = state["params"].store
  snap = {"master": store.master.clone(), "shadow": store.shadow.clone(),
          "grad": None if store.grad is None else store.grad.clone()}
  for k, v in u.tree_flatten_with_names(state["opt"].state_tree())[0]:
    snap["opt/" + k] = torch.as_tensor(v).clone()
  return snap


@pytest.mark.parametrize("loss", ["softmax_xent", "sigmoid_xent"])
def test_evaluator_on_the_trainers_predict_fn(dev, loss):
  from big_vision_amd import train
  from big_vision_amd.evaluators import classification, common
  config = _config(loss)
  _, model = train.get_model(config)
  state = _state(dev, config, model)
  batches = _batches(dev, loss)
  predict_fn = train.make_predict_fn(model, config)
  # the predict function is the training forward at train=False
  store = state["params"].store
  logits = []
  for b in batches:
    got, out = predict_fn(state, {"image": b["image"]})
    ex = model.executor(store, "", model.grid(tuple(b["image"].shape)))
    want, _, _ = ex.fwd(b["image"], save=False)
    assert got.shape == (N, CLASSES) and torch.equal(got, want)
    assert out["logits"] is got
    logits.append(got.float().cpu())
  assert len(set(torch.cat(logits).argmax(-1).tolist())) > 1            # the logits are not degenerate
  # the evaluator, built the way the trainer builds it
  (name, ev, logsteps, prefix), = common.from_config(config, {"predict": predict_fn})
  assert (name, logsteps, prefix) == ("val", 1, "val/") and isinstance(ev, classification.Evaluator)
  ev.batches = batches
  before = _snapshot(state)
  got = dict(ev.run(state))
  after = _snapshot(state)
  assert list(got) == ["prec@1", "loss"]
  ncorrect = loss_sum = nseen = bound = 0.0
  for b, lg in zip(batches, logits):
    ref = B.classify64(loss, lg, b["labels"].cpu(), b["_mask"].cpu())
    rb = B.loss_bound(loss, lg, b["labels"].cpu())
    ncorrect, loss_sum, nseen = ncorrect + ref["ncorrect"], loss_sum + ref["loss_sum"], nseen + ref["nseen"]
    bound += B.sum_bound(ref, rb)
  assert nseen == 2 * N - 3
  assert got["prec@1"] == ncorrect / nseen
  tol = max(B.LEGACY_VALUE[1] + B.LEGACY_VALUE[0] * abs(loss_sum), bound) / nseen
  print(f"[eval step] {loss}: prec@1 {got['prec@1']:.4f}, loss {got['loss']:.6f} vs fp64 {loss_sum / nseen:.6f} (tol {tol:.2e})")
  assert abs(got["loss"] - loss_sum / nseen) <= tol
  # the evaluation changed no bit of the train state
  assert set(before) == set(after)
  for k in before:
    assert (before[k] is None and after[k] is None) or torch.equal(before[k], after[k]), k
  assert store.want_grads is True


def test_an_evaluation_between_two_steps_leaves_the_parameters_of_two_steps(dev):
  """step, evaluation, step vs step, step from the same start.  The evaluation itself changes no bit (asserted), so the
  second steps start from states that differ only by what two runs of the FIRST step differ by: the fp32 atomic adds of
  the bias / LayerNorm / column-sum gradients make a training step's result depend on arrival order.  The parameters
  are therefore compared like tests/test_bench_gpu.py compares two runs of the same steps: through their updates
  p - p0, relative L2 norm <= 2e-2 (that file's bound for arrays; it documents the measured run-to-run spread)."""
  from big_vision_amd import train
  from big_vision_amd.evaluators import classification
  loss = "softmax_xent"
  config = _config(loss)
  _, model = train.get_model(config)
  batches = _batches(dev, loss)
  update_fn = train.make_update_fn(model, config)
  step_batch = lambda b: {"image": b["image"], "labels": b["labels"]}
  finals = []
  for with_eval in (True, False):
    state = _state(dev, config, model)
    p0 = state["params"].store.master.clone()
    state, _ = update_fn(state, 0, step_batch(batches[0]))
    if with_eval:
      ev = classification.Evaluator(train.make_predict_fn(model, config), loss, batches=batches)
      before = _snapshot(state)
      results = dict(ev.run(state))
      after = _snapshot(state)
      assert 0.0 <= results["prec@1"] <= 1.0 and results["loss"] > 0
      for k in before:
        assert (before[k] is None and after[k] is None) or torch.equal(before[k], after[k]), k
    state, meas = update_fn(state, 0, step_batch(batches[1]))
    train.check_finite(meas)
    finals.append((state["params"].store.master.clone() - p0).double())
  a, b = finals
  assert a.norm() > 0
  rel = ((a - b).norm() / b.norm()).item()
  print(f"[eval step] updates with vs without the evaluation: rel L2 {rel:.3e}")
  assert rel <= 2e-2
