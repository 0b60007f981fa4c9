"""Host logic of the classification evaluator without a GPU: `ops.eval_classify` is replaced by a torch-CPU stand-in
built on the fp64 restatement of tests/_eval_bounds.py, so what is checked here is what the evaluator and
`common.from_config` do around the kernel: which batches they feed it, how often they reduce and copy to the host,
what they pass on and what they raise."""
import importlib

import numpy as np
import pytest
import torch

import _eval_bounds as B
from big_vision_amd import ops
from big_vision_amd.compat.ml_collections import ConfigDict
from big_vision_amd.evaluators import classification, common

C, D = 10, 6


class Spy(torch.Tensor):
  """The accumulator the stand-in hands out: counts every copy to the host."""
  reads = []

  def cpu(self, *a, **kw):
    Spy.reads.append("cpu")
    return torch.Tensor.cpu(self.as_subclass(torch.Tensor), *a, **kw)

  def item(self):
    Spy.reads.append("item")
    return self.as_subclass(torch.Tensor).item()

  def tolist(self):
    Spy.reads.append("tolist")
    return self.as_subclass(torch.Tensor).tolist()

  def numpy(self, *a, **kw):
    Spy.reads.append("numpy")
    return self.as_subclass(torch.Tensor).numpy(*a, **kw)


@pytest.fixture()
def kernel(monkeypatch):
  calls = []

  def eval_classify(loss_name, logits, labels, mask=None, acc=None, per_row=False):
    if loss_name not in B.LOSSES:
      raise AttributeError(loss_name)
    assert logits.dtype == labels.dtype == mask.dtype == torch.float32 and not per_row
    ref = B.classify64(loss_name, logits, labels, mask)
    if acc is None:
      acc = torch.zeros(3, dtype=torch.float64).as_subclass(Spy)
    assert isinstance(acc, Spy)
    acc += torch.tensor([ref["ncorrect"], ref["loss_sum"], ref["nseen"]], dtype=torch.float64)
    calls.append((loss_name, tuple(logits.shape)))
    return acc
  monkeypatch.setattr(ops, "eval_classify", eval_classify)
  Spy.reads = []
  return calls


class FakeComm:
  def __init__(self):
    self.calls = []

  def all_reduce_scalars_(self, t):
    assert t.dtype == torch.float64 and tuple(t.shape) == (3,)
    self.calls.append(t)
    t *= 2          # as if a second host had seen the same examples: the ratios must not move


def _data():
  g = torch.Generator().manual_seed(0)
  W = torch.randn((D, C), generator=g)
  batches = []
  for i, mask in enumerate(([1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 0, 0])):      # the last batch is padded
    img = torch.randn((4, D), generator=g)
    y = torch.nn.functional.one_hot(torch.randint(0, C, (4,), generator=g), C).float()
    if i == 1:
      y[2] = 0.0                                                              # an example without a label: dropped
    batches.append({"image": img, "labels": y, "_mask": torch.tensor(mask, dtype=torch.float32)})
  seen = []

  def predict_fn(train_state, batch, scale=1.0):
    assert set(batch) == {"image"}, set(batch)       # labels and _mask were popped (classification.py:69)
    seen.append(train_state)
    return (batch["image"] @ W) * scale, {"pre_logits": batch["image"]}
  return W, batches, predict_fn, seen


def _numpy_reference(loss_name, W, batches):
  """classification.py:37-53 and :65-76 restated with numpy, fp64."""
  ncorrect = loss = nseen = 0.0
  for b in batches:
    logits = (b["image"] @ W).double().numpy()
    labels, mask = b["labels"].double().numpy(), b["_mask"].double().numpy()
    mask = mask * labels.max(axis=1)
    if loss_name == "softmax_xent":
      s = logits - logits.max(axis=1, keepdims=True)
      nll = -np.sum(labels * (s - np.log(np.exp(s).sum(axis=1, keepdims=True))), axis=-1)
    else:
      ls = lambda x: np.minimum(x, 0) - np.log1p(np.exp(-np.abs(x)))
      nll = -np.sum(labels * ls(logits) + (1.0 - labels) * ls(-logits), axis=-1)
    top1 = np.argmax(logits, axis=1)
    correct = np.take_along_axis(labels, top1[:, None], axis=1)[:, 0]
    ncorrect += np.sum(correct * mask)
    loss += np.sum(nll * mask)
    nseen += np.sum(mask)
  assert nseen == 9.0
  return ncorrect / nseen, loss / nseen


@pytest.mark.parametrize("loss_name", ["softmax_xent", "sigmoid_xent"])
def test_evaluator_matches_the_reference_loop(kernel, loss_name):
  W, batches, predict_fn, seen = _data()
  comm = FakeComm()
  ev = classification.Evaluator(predict_fn, loss_name, batches=batches, comm=comm)
  state = {"params": object()}
  got = list(ev.run(state))
  assert [k for k, _ in got] == ["prec@1", "loss"]
  prec, loss = _numpy_reference(loss_name, W, batches)
  assert got[0][1] == pytest.approx(prec, rel=1e-12) and got[1][1] == pytest.approx(loss, rel=1e-12)
  assert kernel == [(loss_name, (4, C))] * 3 and seen == [state] * 3        # one launch per batch
  assert len(comm.calls) == 1 and isinstance(comm.calls[0], Spy)             # process_sum: once, on the accumulator
  assert len(Spy.reads) == 1, Spy.reads                                      # one copy to the host per evaluation
  # a second run iterates the batches again (they were not consumed or edited) and gives the same answer
  assert all(set(b) == {"image", "labels", "_mask"} for b in batches)
  again = list(ev.run(state))
  assert again == got and len(kernel) == 6 and len(comm.calls) == 2 and len(Spy.reads) == 2


def test_evaluator_label_key_no_comm_and_generators(kernel):
  W, batches, predict_fn, _ = _data()
  renamed = [{"image": b["image"], "lbl": b["labels"], "_mask": b["_mask"]} for b in batches]

  class Reiterable:
    def __iter__(self):
      return iter(renamed)
  got = dict(classification.Evaluator(predict_fn, "softmax_xent", label_key="lbl", batches=Reiterable()).run(None))
  prec, loss = _numpy_reference("softmax_xent", W, batches)
  assert got["prec@1"] == pytest.approx(prec, rel=1e-12) and got["loss"] == pytest.approx(loss, rel=1e-12)
  assert len(Spy.reads) == 1


def test_unknown_loss_raises_attribute_error(kernel):
  with pytest.raises(AttributeError, match="nope"):
    classification.Evaluator(lambda s, b: None, "nope")


class Recorder:
  made = []

  def __init__(self, predict_fn, **kw):
    self.predict_fn, self.kw = predict_fn, kw
    Recorder.made.append(self)


def _config():
  c = ConfigDict()
  c.batch_size = 4
  c.evals = {}
  c.evals.classification = dict(loss_name="softmax_xent", log_steps=100, data=dict(name="imagenet2012", split="val"),
                                pp_fn="decode|resize(32)")
  c.evals.minival = dict(type="classification", loss_name="sigmoid_xent", pred="scaled", pred_kw=dict(scale=2.0),
                         prefix="mini_", skip_first=True, log_epochs=1, log_percent=0.1, batch_size=8, label_key="lbl")
  return c


def test_from_config(monkeypatch):
  monkeypatch.setattr(classification, "Evaluator", Recorder)
  Recorder.made = []
  notes, asked = [], []

  def get_steps(key, cfg):
    asked.append((key, dict(cfg)))
    return cfg.get("log_steps", 7)

  def predict(train_state, batch):
    return "plain", train_state, batch

  def scaled(train_state, batch, scale=1.0):
    return "scaled", scale
  c = _config()
  evs = common.from_config(c, {"predict": predict, "scaled": scaled}, write_note=notes.append, get_steps=get_steps)
  assert [(n, ls, p) for n, _, ls, p in evs] == [("classification", 100, "classification/"), ("minival", 7, "mini_")]
  assert notes == ["classification", "minival"]
  assert [e for _, e, _, _ in evs] == Recorder.made
  first, second = Recorder.made
  # `type` defaults to the name; the default predict function; batch_size falls through to config.batch_size
  assert first.predict_fn is predict
  assert first.kw == dict(loss_name="softmax_xent", data=dict(name="imagenet2012", split="val"), pp_fn="decode|resize(32)",
                          batch_size=4)
  # pred / pred_kw; the evaluator's own batch_size wins; nothing from_config consumed reaches the constructor
  assert second.predict_fn("s", "b") == ("scaled", 2.0)
  assert second.kw == dict(loss_name="sigmoid_xent", batch_size=8, label_key="lbl")
  # get_steps saw the log_* keys (they are popped only afterwards), and none of the generic keys
  assert [k for k, _ in asked] == ["log", "log"]
  assert asked[1][1]["log_epochs"] == 1 and asked[1][1]["log_percent"] == 0.1
  assert not {"type", "pred", "pred_kw", "prefix", "skip_first"} & set(asked[1][1])
  # the rest of the batch_size chain (common.py:60)
  c.batch_size_eval = 32
  assert common.from_config(c, {"predict": predict, "scaled": scaled}, get_steps=get_steps)[0][1].kw["batch_size"] == 32
  del c["batch_size_eval"]
  c["input.batch_size"] = 16
  assert common.from_config(c, {"predict": predict, "scaled": scaled}, get_steps=get_steps)[0][1].kw["batch_size"] == 16
  # the default get_steps reads cfg["log_steps"]
  c.evals.minival.log_steps = 5
  assert [ls for _, _, ls, _ in common.from_config(c, {"predict": predict, "scaled": scaled})] == [100, 5]
  assert c.evals.minival.to_dict()["pred"] == "scaled"          # the config itself is not edited


def test_from_config_errors():
  c = _config()
  with pytest.raises(ValueError, match=r"Unknown predict_fn 'scaled'. Available predict_fns are:\npredict\nloss"):
    common.from_config(c, {"predict": lambda s, b: None, "loss": lambda s, b: None}, get_steps=lambda k, cfg: 1)
  c = ConfigDict()
  c.evals = {}
  c.evals.fewshot_lsr = dict(log_steps=1)
  with pytest.raises(ModuleNotFoundError, match="big_vision.evaluators.fewshot_lsr"):
    common.from_config(c, {"predict": lambda s, b: None})
  assert common.from_config(ConfigDict(), {}) == []


def test_from_config_builds_a_working_evaluator(kernel):
  W, batches, predict_fn, _ = _data()
  c = ConfigDict()
  c.evals = {}
  c.evals.val = dict(type="classification", loss_name="softmax_xent", log_steps=3, pred_kw=dict(scale=1.0))
  (name, ev, logsteps, prefix), = common.from_config(c, {"predict": predict_fn})
  assert (name, logsteps, prefix) == ("val", 3, "val/") and isinstance(ev, classification.Evaluator)
  assert ev.pipeline_kw == {"batch_size": None}
  ev.batches = batches
  prec, loss = _numpy_reference("softmax_xent", W, batches)
  got = dict(ev.run(None))
  assert got["prec@1"] == pytest.approx(prec, rel=1e-12) and got["loss"] == pytest.approx(loss, rel=1e-12)


def test_reference_module_paths_resolve_to_this_tree():
  assert importlib.import_module("big_vision.evaluators.classification") is classification
  assert importlib.import_module("big_vision.evaluators.common") is common
  from big_vision_amd import train
  assert callable(train.make_predict_fn)
