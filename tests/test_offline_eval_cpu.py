"""Host logic of offline evaluation without a GPU: the mean and save evaluators, tools/eval_only.py and
configs/load_and_eval.py.  `_lib.call` is replaced by a recorder (the dry run of test_bigvision_surface_cpu.py) that
also PERFORMS `bv_dot_f32` on the host addresses it is handed (`out += sum a b` in fp64, what include/bvhip.h states),
so the launch counts and the host arithmetic around the launches are both checked; the kernel itself is held to its
bound on the GPU (tests/test_offline_eval_gpu.py)."""
import collections
import ctypes
import importlib
import json
import types

import numpy as np
import pytest
import torch

from big_vision_amd.compat.ml_collections import ConfigDict

TINY = dict(width=128, depth=2, num_heads=2, mlp_dim=256, patch_size=(16, 16), pool_type="gap")


@pytest.fixture()
def dry(monkeypatch):
  from big_vision_amd import _lib, ops
  calls = collections.Counter()

  def call(name, *args):
    calls.update([name])
    if name == "bv_dot_f32":
      pa, pb, count, pout, _ = args
      a, b = (np.ctypeslib.as_array((ctypes.c_float * count).from_address(p)).astype(np.float64) for p in (pa, pb))
      out = ctypes.c_double.from_address(pout)
      out.value += float(np.dot(a, b))
  monkeypatch.setattr(_lib, "call", call)
  monkeypatch.setattr(ops, "_chk", lambda t, dtype, name: t)
  monkeypatch.setattr(ops, "_stream", lambda: 0)
  return calls


def _metric_batches(nbatches=4, b=5):
  """`nbatches` batches of `b` rows with three metrics (fp32, bf16, int32); the last batch has two padding rows."""
  g = torch.Generator().manual_seed(7)
  out = []
  for i in range(nbatches):
    mask = torch.ones(b)
    if i == nbatches - 1:
      mask[-2:] = 0
    out.append({"a": torch.rand(b, generator=g) * 10, "b": (torch.rand(b, generator=g) * 4).to(torch.bfloat16),
                "c": torch.randint(0, 100, (b,), generator=g, dtype=torch.int32), "_mask": mask})
  return out


def _metrics_fn(train_state, batch):
  return {k: batch[k] for k in ("a", "b", "c")}


def test_module_paths_resolve_to_this_tree():
  for name in ("evaluators.mean", "evaluators.save", "tools.eval_only", "configs.load_and_eval"):
    assert importlib.import_module(f"big_vision.{name}") is importlib.import_module(f"big_vision_amd.{name}"), name
  from big_vision.evaluators import mean, save
  assert mean.API == save.API == "jit"


def test_from_config_builds_both_evaluators():
  from big_vision_amd.evaluators import common, mean, save
  c = ConfigDict()
  c.batch_size = 16
  c.evals = {}
  c.evals.avg = dict(type="mean", log_steps=3, data=dict(name="imagenet2012", split="val"), pp_fn="decode")
  c.evals.dump = dict(type="save", outfile="{workdir}/p-{step:09d}.npz", pred_kw=dict(collect=False), log_steps=5,
                      data=dict(name="imagenet2012", split="val"), cache_final=False, prefix="")
  seen = []

  def predict(train_state, batch, collect=True):
    seen.append(collect)
    return {}
  (n1, avg, s1, p1), (n2, dump, s2, p2) = common.from_config(c, {"predict": predict})
  assert (n1, s1, p1) == ("avg", 3, "avg/") and (n2, s2, p2) == ("dump", 5, "")
  assert isinstance(avg, mean.Evaluator) and isinstance(dump, save.Evaluator)
  assert avg.pipeline_kw == dict(data=dict(name="imagenet2012", split="val"), pp_fn="decode", batch_size=16)
  assert dump.pipeline_kw == dict(data=dict(name="imagenet2012", split="val"), cache_final=False, batch_size=16)
  assert dump.outfile == "{workdir}/p-{step:09d}.npz" and dump.workdir is None and avg.comm is None
  dump.predict_fn(None, {})
  assert seen == [False]


def test_mean_launches_and_values(dry):
  from big_vision_amd import dp
  from big_vision_amd.evaluators import mean
  batches = _metric_batches()
  seen = []

  def predict_fn(train_state, batch):
    seen.append((train_state, set(batch)))
    return _metrics_fn(train_state, batch)

  class Comm(dp.Comm):
    def __init__(self):
      self.calls = []

    def all_reduce_scalars_(self, t):
      self.calls.append((t.dtype, tuple(t.shape)))
  comm = Comm()
  ev = mean.Evaluator(predict_fn, batches=batches, comm=comm)
  got = list(ev.run("state"))
  assert dict(dry) == {"bv_dot_f32": 4 * (3 + 1)}                       # no other entry point
  assert seen == [("state", {"a", "b", "c", "_mask"})] * 4              # predict_fn sees the whole batch
  assert comm.calls == [(torch.float64, (4,))]                          # one reduction, on the one accumulator
  assert [k for k, _ in got] == ["a", "b", "c"]
  mask = np.concatenate([b["_mask"].numpy() for b in batches]).astype(np.float64)
  assert mask.sum() == 18
  for key, value in got:
    x = np.concatenate([b[key].to(torch.float32).numpy() for b in batches]).astype(np.float64)
    assert value == pytest.approx((mask * x).sum() / mask.sum(), rel=1e-14), key
  # a second run iterates the batches again and gives the same answer
  assert list(ev.run("state")) == got and dry["bv_dot_f32"] == 32


def test_mean_checks(dry):
  from big_vision_amd.evaluators import mean
  batches = _metric_batches(2)
  with pytest.raises(AssertionError, match="predict_fn must return a dict"):
    list(mean.Evaluator(lambda s, b: (b["a"], {}), batches=batches).run(None))
  with pytest.raises(ValueError, match=r"^Expected per-example metrics of shape \(5,\) found"):
    list(mean.Evaluator(lambda s, b: {"a": b["a"], "two": torch.zeros(5, 2)}, batches=batches).run(None))
  with pytest.raises(ValueError, match="`batches` is empty"):
    list(mean.Evaluator(_metrics_fn).run(None))
  with pytest.raises(ValueError, match="`batches` is empty"):
    list(mean.Evaluator(_metrics_fn, batches=iter(())).run(None))
  assert not dry


def test_save_outfile_step_and_rows(tmp_path):
  from big_vision_amd import utils as u
  from big_vision_amd.evaluators import save
  g = torch.Generator().manual_seed(3)
  batches = [{"image": torch.rand(4, 2, 2, 3, generator=g), "id": torch.arange(4) + 4 * i,
              "_mask": torch.tensor([1, 1, 1, 1] if i == 0 else [1, 0, 1, 0])} for i in range(2)]

  def predict_fn(train_state, batch):
    pooled = batch["image"].mean((1, 2))
    return pooled, {"half": pooled.to(torch.bfloat16), "absent": None}
  ev = save.Evaluator(predict_fn, "{workdir}/p-{step:09d}.npz", batches=batches, workdir=str(tmp_path), pp_fn="decode")
  assert ev.pipeline_kw == {"pp_fn": "decode"}
  gen = ev.run({"params": {}, "opt": types.SimpleNamespace(count=1234)})
  assert isinstance(gen, types.GeneratorType) and not (tmp_path / "p-000001234.npz").exists()
  assert list(gen) == [] and (tmp_path / "p-000001234.npz").exists()     # yields nothing; the count of the stub opt
  assert list(ev.run({"w": torch.zeros(1)})) == [] and (tmp_path / "p-000000000.npz").exists()   # no "opt": step 0
  res = u.load_checkpoint_np(str(tmp_path / "p-000000000.npz"))
  assert set(res) == {"inputs", "outputs"} and set(res["inputs"]) == {"image", "id"}
  assert set(res["outputs"]) == {"0", "1"} and set(res["outputs"]["1"]) == {"half"}     # tuple -> "0", "1"; None dropped
  assert res["inputs"]["id"].tolist() == [0, 1, 2, 3, 4, 6]
  want = torch.cat([batches[0]["image"], batches[1]["image"][[0, 2]]])
  assert np.array_equal(res["inputs"]["image"], want.numpy())
  assert np.array_equal(res["outputs"]["0"], want.mean((1, 2)).numpy())
  assert np.array_equal(res["outputs"]["1"]["half"], want.mean((1, 2)).to(torch.bfloat16).float().numpy())
  with np.load(str(tmp_path / "p-000000000.npz")) as z:                     # a compressed archive
    assert all(i.compress_type != 0 for i in z.zip.infolist())
  with pytest.raises(ValueError, match="`batches` is empty"):
    list(save.Evaluator(predict_fn, "x.npz").run({}))
  with pytest.raises(ValueError, match="leaf 'outputs' of shape .* is not per-example"):
    list(save.Evaluator(lambda s, b: torch.zeros(3), str(tmp_path / "x.npz"), batches=batches).run({}))


def _eval_config(**evals):
  c = ConfigDict()
  c.model_name, c.model, c.num_classes = "vit", dict(TINY), 10
  c.init_shapes = [(1, 32, 32, 3)]
  c.evals = evals
  return c


def test_eval_only_refusals(dry, tmp_path):
  from big_vision_amd.tools import eval_only
  c = _eval_config(val=dict(type="classification", loss_name="softmax_xent"))
  c.model.reinit = ["head"]
  with pytest.raises(AssertionError, match="model.reinit"):
    eval_only.run(c, device="cpu")
  c = _eval_config(fewshot=dict(type="fewshot_lsr"))
  with pytest.raises(ModuleNotFoundError, match="big_vision.evaluators.fewshot_lsr"):
    eval_only.run(c, device="cpu")
  c = _eval_config(val=dict(type="classification", loss_name="softmax_xent"))
  with pytest.raises(ValueError, match=r"batches for \['vla'\]"):
    eval_only.run(c, device="cpu", batches={"vla": []})
  # the command line: --config FILE[:ARG] goes through configs/loader.py
  cfg = tmp_path / "cfg.py"
  cfg.write_text("import ml_collections\n"
                 "def get_config(arg=None):\n"
                 "  c = ml_collections.ConfigDict()\n"
                 "  c.model_name, c.model = 'vit', dict(variant=arg, reinit=['head'])\n"
                 "  return c\n")
  with pytest.raises(AssertionError, match="model.reinit"):
    eval_only.main(["--config", f"{cfg}:Ti/16", "--workdir", str(tmp_path / "w")])
  with pytest.raises(SystemExit):
    eval_only.main([])


def test_eval_only_runs_the_evaluators(dry, tmp_path):
  """The driver on the dry-run kernels: mean through an extra predict function (values are those of the host stand-in
  for bv_dot_f32), repeats, the metrics file, num_params."""
  from big_vision_amd.models import vit
  from big_vision_amd.tools import eval_only
  c = _eval_config(avg=dict(type="mean", pred="metrics", pred_kw=dict(scale=2.0), prefix="m_", log_steps=1000))
  c.eval_repeats = 2
  batches = _metric_batches(2)
  states = []

  def metrics(params, batch, scale):
    states.append(params)
    return {"a": batch["a"] * scale}
  res = eval_only.run(c, workdir=str(tmp_path), batches={"avg": batches}, device="cpu", predict_fns={"metrics": metrics})
  store = vit.Model(num_classes=10, **TINY).make_store((1, 32, 32, 3), "cpu")
  assert res[0]["num_params"] == sum(store.leaf(n).numel() for n in store.leaf_names()) > 0
  mask = torch.cat([b["_mask"] for b in batches]).double()
  want = float((torch.cat([b["a"] for b in batches]).double() * 2 * mask).sum() / mask.sum())
  assert res[0]["m_a"] == pytest.approx(want, rel=1e-14) and res[1] == {"m_a": res[0]["m_a"]}
  assert set(res[0]) == {"num_params", "m_a"} and dry["bv_dot_f32"] == 2 * 2 * 2
  assert all("Transformer" in p and "opt" not in p for p in states)        # run() is handed the bare parameters
  lines = [json.loads(l) for l in (tmp_path / "big_vision_metrics.txt").read_text().splitlines()]
  assert lines == [{"step": 0, **res[0]}, {"step": 1, **res[1]}]


def test_load_and_eval_config():
  cfg = importlib.import_module("big_vision.configs.load_and_eval")
  c = cfg.get_config("name=vit_i1k,batch_size=8,variant=Ti/16,model_init=/ckpt/ti16.npz")
  assert c.optax_name == "identity" and c.eval_only is True and c.total_steps == 0 and c.lr == 0.0
  assert c.sharding_strategy == [("params/.*", 'fsdp(axis="data")')] and c.mesh == [("data", -1)]
  assert c.input.batch_size == 8 and c.input.data.name == "bv:dummy"
  assert (c.model_name, c.model.variant, c.model_init, c.num_classes) == ("vit", "Ti/16", "/ckpt/ti16.npz", 1000)
  assert "variant" not in c and not any(k in c for k in ("schedule", "pp_train", "wd"))
  d = cfg.get_config()
  assert (d.name, d.batch_size, d.model.variant, d.model_init) == ("vit_i1k", 4, "S/16", "")
  assert cfg.get_config("vit_i21k").evals.val.loss_name == "sigmoid_xent"
  for conf in (c, d, cfg.get_config("vit_i21k")):
    assert len(conf.evals) >= 2
    for name, ev in conf.evals.items():
      assert ev["type"] in ("classification", "mean", "save"), name
      assert hasattr(importlib.import_module(f"big_vision.evaluators.{ev['type']}"), "Evaluator")
  with pytest.raises(KeyError, match="bit_paper"):
    cfg.get_config("name=bit_paper")
  # the same file through the loader, as `--config FILE:ARG` reads it
  from big_vision_amd.configs import loader
  assert loader.load_config(f"{cfg.__file__}:name=vit_i1k,batch_size=8,variant=Ti/16,model_init=/ckpt/ti16.npz").to_dict() \
      == c.to_dict()
