"""bench.py's plain run end to end (small batch): ONE line with the headline fields and none of the --full objects,
and --dump-outputs writing the same float arrays from the same inputs on every run."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
import bench  # noqa: E402
from big_vision_amd.models.proj.image_text import two_towers  # noqa: E402
from big_vision_amd.trainers.proj.image_text import siglip  # noqa: E402


def _run(out_dir):
  env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
  r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--global-batch", "32", "--steps", "3",
                      "--warmup", "1", "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, r.stderr[-2000:]
  lines = [l for l in r.stdout.splitlines() if l.strip()]
  assert len(lines) == 1, r.stdout[-1000:]
  return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path, dev):
  a = _run(tmp_path / "a")
  for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
    assert key in a, key
  assert a["steps"] == 3 and a["warmup"] == 1 and a["unit"] == "pairs/s" and a["higher_is_better"] is True
  assert a["ms_per_step"] > 0 and abs(a["value"] - 32 * 1e3 / a["ms_per_step"]) <= 1e-6 * a["value"]
  for key in ("roofline", "configs", "cpu_baseline", "bf16_stream", "rccl"):
    assert key not in a, key
  names = sorted(os.listdir(tmp_path / "a"))
  assert {"training_loss.npy", "l2_grads.npy", "params.npy", "opt_mu.npy", "opt_nu.npy"} <= set(names)
  arrs = {n: np.load(tmp_path / "a" / n) for n in names}
  assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in arrs.values())
  assert sum(v.nbytes for v in arrs.values()) <= 64 << 20
  assert float(arrs["training_loss.npy"]) == pytest.approx(a["config"]["final_loss"], rel=1e-6)
  # Same arguments: bit-identical inputs (seeded generators) and initial weights, but NOT bit-identical outputs - the
  # bias / LayerNorm / colsum gradients are summed with fp32 atomics, so their summation order varies from run to run.
  # The parameters therefore agree only relative to what the steps moved them: every comparison is a relative L2 norm
  # (scale-free, so tiny arrays such as nu ~ (1 - b2) g^2 are compared too), and the parameters are compared through
  # their updates p - p0 against the initial weights p0.  Measured spread over three runs on one MI355X: loss and the
  # gradient / update norms <= 5e-5, Adam moments <= 3.1e-4, parameter updates <= 1.05e-3 (the largest element
  # difference, 3.7e-6, is 12 % of the largest update, so an absolute tolerance on p itself cannot hold).  Bounds at
  # about 20x the spread: scalars 1e-3, arrays 2e-2.
  x1, x2 = bench.synthetic_batch(32, dev, seed=1), bench.synthetic_batch(32, dev, seed=1)
  assert all(torch.equal(u, v) for u, v in zip(x1, x2))
  del x1, x2
  model = two_towers.Model(image=bench.IMAGE_CFG, text=bench.TEXT_CFG, out_dim=(None, bench.EMB), temperature_init=10.0,
                           bias_init=-10.0)
  state, _ = siglip.make_train_state(model, bench.make_config(20_000), (32, bench.RES, bench.RES, 3), (32, bench.SEQ), rng=0,
                                     total_steps=20_000, device=dev)
  bench.dump_outputs(str(tmp_path / "init"), state, {})
  del state, model
  torch.cuda.empty_cache()
  p0 = np.load(tmp_path / "init" / "params.npy").astype(np.float64)
  b = _run(tmp_path / "b")
  assert sorted(os.listdir(tmp_path / "b")) == names
  other = {n: np.load(tmp_path / "b" / n) for n in names}
  for n in names:
    assert arrs[n].shape == other[n].shape, n
  x = {n: v.astype(np.float64) for n, v in arrs.items()}
  y = {n: v.astype(np.float64) for n, v in other.items()}
  x["params.npy"], y["params.npy"] = x["params.npy"] - p0, y["params.npy"] - p0      # the updates of the 5 steps
  assert p0.shape == x["params.npy"].shape and np.linalg.norm(x["params.npy"]) > 0
  for n in names:
    ref = np.linalg.norm(x[n])
    assert ref > 0, n
    err = np.linalg.norm(x[n] - y[n]) / ref
    assert err <= (1e-3 if x[n].ndim == 0 else 2e-2), (n, err)
  assert math.isclose(a["config"]["final_loss"], b["config"]["final_loss"], rel_tol=1e-3)
