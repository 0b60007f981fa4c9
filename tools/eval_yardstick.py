"""Yardstick of the fused classification-evaluation kernel (tools only, GPU): `bv_eval_classify` (one launch per batch
into a device accumulator, nothing else in the timed region) against the same three sums composed from eager torch
ops on the same GPU, for both losses at (n, C) = (1024, 1000), (1024, 21843) and (4096, 10).

Timing: one HIP-event pair around a BATCH of back-to-back calls after `--warmup` untimed calls; the figure is window
time / calls, median and best over `--iters` windows.  It is the time per call of a saturated queue: launch overhead
is included, and where the host enqueues more slowly than the GPU executes it IS the host's launch rate - it is not
kernel time (that needs a kernel trace).  The number of calls per window follows the shape (`--window-bytes` of
algorithmic traffic per window, between 200 and 20000 calls; a tenth of that for the torch composition, which is
several times slower).  The calls rotate over enough (logits, labels) sets to exceed 512 MB, twice the 256 MB
memory-side cache, so no call finds its operands cached by an earlier one.  GB/s is the algorithmic traffic
8 * n * C + 4 * n bytes (logits and labels read once, the mask read once) over that per-call time, i.e. a lower bound
of the kernel's own bandwidth; the torch composition moves several times those bytes, which is the point of the
comparison.  `again` repeats the fused measurement after the torch one (the spread of the same code in one process).

Every shape is measured in a child process of its own under a time limit; the parent never touches the GPU and stops
at the first child that fails.

  python tools/eval_yardstick.py [--iters N] [--warmup N] [--window-bytes B] [--out profiles/eval_yardstick.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((1024, 1000), (1024, 21843), (4096, 10))
LOSSES = ("softmax_xent", "sigmoid_xent")
STEP_TIMEOUT_S = 240
ROTATE_BYTES = 512 << 20   # the operand sets a measurement rotates over: twice the memory-side cache


def algorithmic_bytes(n, C):
  return 8 * n * C + 4 * n


def measure(n, C, iters, warmup, window_bytes):
  import torch
  from big_vision_amd import _lib
  dev = torch.device("cuda:0")
  torch.cuda.set_device(dev)
  g = torch.Generator(device=dev).manual_seed(0)
  nbytes = algorithmic_bytes(n, C)
  sets = max(2, -(-ROTATE_BYTES // nbytes))
  X = [3.0 * torch.randn((n, C), device=dev, generator=g) for _ in range(sets)]
  Y = [torch.nn.functional.one_hot(torch.randint(0, C, (n,), device=dev, generator=g), C).float() for _ in range(sets)]
  mask = (torch.rand((n,), device=dev, generator=g) < 0.9).float()
  acc = torch.zeros(3, device=dev, dtype=torch.float64)
  acc_t = torch.zeros(3, device=dev, dtype=torch.float64)
  stream = torch.cuda.current_stream().cuda_stream
  ptrs = [(x.data_ptr(), y.data_ptr()) for x, y in zip(X, Y)]
  accp, maskp = acc.data_ptr(), mask.data_ptr()
  calls = int(min(20000, max(200, window_bytes // nbytes)))
  out = []
  for loss in LOSSES:
    kind = _lib.EVAL_LOSSES[loss]

    def fused(i):
      xp, yp = ptrs[i % sets]
      _lib.call("bv_eval_classify", kind, xp, yp, maskp, accp, None, None, n, C, stream)

    def composed(i):
      x, y = X[i % sets], Y[i % sets]
      m = mask * y.max(1).values
      if loss == "softmax_xent":
        nll = -(y * torch.log_softmax(x, -1)).sum(-1)
      else:
        nll = -(y * torch.nn.functional.logsigmoid(x) + (1.0 - y) * torch.nn.functional.logsigmoid(-x)).sum(-1)
      correct = y.gather(1, x.argmax(1)[:, None])[:, 0]
      acc_t.add_(torch.stack([(correct * m).sum(), (nll * m).sum(), m.sum()]))

    def timeit(fn, k):
      for i in range(warmup):
        fn(i)
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      per = []
      for _ in range(iters):
        e0.record()
        for i in range(k):
          fn(i)
        e1.record(); e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / k)
      per.sort()
      return per[len(per) // 2], per[0]

    # the two compute the same thing
    acc.zero_(); acc_t.zero_()
    fused(0); composed(0)
    torch.cuda.synchronize()
    a, b = acc.tolist(), acc_t.tolist()
    assert a[0] == b[0] and a[2] == b[2] and abs(a[1] - b[1]) <= 1e-4 * abs(b[1]), (a, b)
    res = {"n": n, "C": C, "loss": loss, "device": torch.cuda.get_device_name(dev), "bytes": nbytes, "sets": sets}
    for name, fn, k in (("bv_eval_classify", fused, calls), ("torch_ops", composed, max(20, calls // 10)),
                        ("bv_eval_classify_again", fused, calls)):
      med, best = timeit(fn, k)
      res[name] = {"median_us": round(med, 2), "best_us": round(best, 2), "GBps_median": round(nbytes / med / 1e3, 1),
                   "calls_per_window": k, "window_ms_median": round(med * k / 1e3, 1)}
    res["torch_over_fused"] = round(res["torch_ops"]["median_us"] / res["bv_eval_classify"]["median_us"], 2)
    out.append(res)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=7, help="timed windows per variant")
  ap.add_argument("--warmup", type=int, default=50)
  ap.add_argument("--window-bytes", type=int, default=1 << 40, help="algorithmic traffic of one fused window")
  ap.add_argument("--out", default=None)
  ap.add_argument("--one", default=None, help="(child) measure this n,C and print one JSON line per loss")
  a = ap.parse_args()
  if a.one is not None:
    n, C = (int(v) for v in a.one.split(","))
    for r in measure(n, C, a.iters, a.warmup, a.window_bytes):
      print("RESULT " + json.dumps(r, sort_keys=True), flush=True)
    return 0
  rows = []
  for n, C in SHAPES:
    cmd = [sys.executable, os.path.abspath(__file__), "--one", f"{n},{C}", "--iters", str(a.iters), "--warmup", str(a.warmup),
           "--window-bytes", str(a.window_bytes)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=STEP_TIMEOUT_S)
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or len(lines) != len(LOSSES):
      sys.stderr.write(p.stdout)
      print(f"n={n} C={C}: the measurement failed (exit status {p.returncode}); nothing further is started", file=sys.stderr)
      return 1
    rows += [json.loads(l[len("RESULT "):]) for l in lines]
  text = "".join(json.dumps(r, sort_keys=True) + "\n" for r in rows)
  print(text, end="")
  for r in rows:
    f, t = r["bv_eval_classify"], r["torch_ops"]
    print(f"# n={r['n']} C={r['C']} {r['loss']}: fused {f['median_us']} us ({f['GBps_median']} GB/s of {r['bytes']} B), "
          f"torch {t['median_us']} us, torch / fused {r['torch_over_fused']}x", file=sys.stderr)
  if a.out:
    with open(a.out, "w") as fh:
      fh.write(text)
  return 0


if __name__ == "__main__":
  sys.exit(main())
