"""Yardstick of the fused distillation loss (tools only, GPU): `bv_distill_dist` (kl at t = 2, with the gradient, one
launch, `accumulate = 0` into a preallocated gradient, nothing else in the timed region) against the same loss and
gradient composed from torch ops on the same GPU, at C = 1000 and n = 512 / 4096.

Timing: one HIP-event pair around a BATCH of back-to-back calls (`--batch`, default 20000), after `--warmup` untimed
calls; the figure is window time / calls, median and best over `--iters` windows.  It is the time per call of a
saturated queue: launch overhead is included, and where the host enqueues more slowly than the GPU executes it IS the
host's launch rate - it is not kernel time (that needs a kernel trace).  The calls rotate over enough
(student, teacher, gradient) sets to exceed 512 MB, twice the 256 MB memory-side cache, so no call finds its operands
cached by an earlier one.  GB/s is the algorithmic traffic 3 * n * C * 4 bytes (student and teacher read once, the
gradient written once) over that per-call time, i.e. a lower bound of the kernel's own bandwidth; the torch
composition moves several times those bytes, which is the point of the comparison.

Every shape is measured in a child process of its own under a time limit; the parent never touches the GPU and stops
at the first child that fails.

  python tools/distill_yardstick.py [--iters N] [--batch N] [--warmup N] [--out profiles/distill_yardstick.md]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C = 1000
SHAPES = (512, 4096)
T = 2.0
STEP_TIMEOUT_S = 240
ROTATE_BYTES = 512 << 20   # the operand sets a measurement rotates over: twice the memory-side cache


def measure(n, iters, warmup, batch):
  import torch
  from big_vision_amd import _lib, ops
  dev = torch.device("cuda:0")
  torch.cuda.set_device(dev)
  g = torch.Generator(device=dev).manual_seed(0)
  nbytes = 3 * n * C * 4
  sets = max(2, -(-ROTATE_BYTES // nbytes))
  S = [3.0 * torch.randn((n, C), device=dev, generator=g) for _ in range(sets)]
  Tt = [3.0 * torch.randn((n, C), device=dev, generator=g) for _ in range(sets)]
  G = [torch.empty((n, C), device=dev) for _ in range(sets)]
  acc = torch.zeros(1, device=dev, dtype=torch.float64)
  stream = torch.cuda.current_stream().cuda_stream
  kl = _lib.DISTILL_KINDS["kl"]
  ptrs = [(s.data_ptr(), t.data_ptr(), gr.data_ptr()) for s, t, gr in zip(S, Tt, G)]
  accp = acc.data_ptr()

  def fused(i):
    sp, tp, gp = ptrs[i % sets]
    _lib.call("bv_distill_dist", kl, sp, tp, None, accp, gp, 0, n, C, n, T, 0.0, 1e-12, 1, stream)

  def composed(i):
    s, t = S[i % sets], Tt[i % sets]
    y = torch.softmax(t / T, -1)
    lp = torch.log_softmax(s / T, -1)
    loss = T * T * ((y * (torch.log(y.clamp_min(1e-8)) - lp)).sum(-1)).mean()
    g_ = (T / n) * (torch.exp(lp) - y)
    return loss, g_

  def timeit(fn, calls):
    for i in range(warmup):
      fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(iters):
      e0.record()
      for i in range(calls):
        fn(i)
      e1.record(); e1.synchronize()
      per.append(e0.elapsed_time(e1) * 1e3 / calls)
    per.sort()
    return per[len(per) // 2], per[0]

  # the two compute the same thing
  acc.zero_()
  fused(0)
  loss, g_ = composed(0)
  torch.cuda.synchronize()
  assert abs(acc.item() - loss.item()) <= 1e-4 * abs(loss.item()), (acc.item(), loss.item())
  assert (G[0] - g_).abs().max().item() <= 1e-6
  res = {"n": n, "C": C, "device": torch.cuda.get_device_name(dev), "bytes": nbytes, "sets": sets, "batch": batch}
  for name, fn, calls in (("bv_distill_dist", fused, batch), ("torch_ops", composed, max(1, batch // 10)),
                          ("bv_distill_dist_again", fused, batch)):
    med, best = timeit(fn, calls)
    res[name] = {"median_us": round(med, 2), "best_us": round(best, 2), "GBps_median": round(nbytes / med / 1e3, 1),
                 "calls_per_window": calls, "window_ms_median": round(med * calls / 1e3, 1)}
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=9, help="timed windows per variant")
  ap.add_argument("--batch", type=int, default=20000, help="back-to-back calls per timed window")
  ap.add_argument("--warmup", type=int, default=100)
  ap.add_argument("--out", default=None)
  ap.add_argument("--one", type=int, default=None, help="(child) measure this n and print one JSON line")
  a = ap.parse_args()
  if a.one is not None:
    print("RESULT " + json.dumps(measure(a.one, a.iters, a.warmup, a.batch), sort_keys=True), flush=True)
    return 0
  rows = []
  for n in SHAPES:
    cmd = [sys.executable, os.path.abspath(__file__), "--one", str(n), "--iters", str(a.iters), "--warmup", str(a.warmup),
           "--batch", str(a.batch)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=STEP_TIMEOUT_S)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not line:
      sys.stderr.write(p.stdout)
      print(f"n={n}: the measurement failed (exit status {p.returncode}); nothing further is started", file=sys.stderr)
      return 1
    rows.append(json.loads(line[0][len("RESULT "):]))
  out = ["# Distillation loss yardstick", "",
         f"`tools/distill_yardstick.py --iters {a.iters} --batch {a.batch} --warmup {a.warmup}` on {rows[0]['device']}: kl at "
         f"t = {T:g} with the gradient, C = 1000, fp32.", "",
         "Time per call (us, median / best over the windows) of a back-to-back batch between one HIP-event pair: launch "
         "overhead included, NOT kernel time; where the host enqueues more slowly than the GPU executes, it is the host's "
         "launch rate.  GB/s = the algorithmic 3 * n * C * 4 bytes over the median per-call time, a lower bound of the "
         "kernel's bandwidth.  The calls rotate over `sets` operand sets (> 512 MB in all), so no call reads operands an "
         "earlier call left in the memory-side cache.  `again` repeats the first measurement after the torch one (spread "
         "of the same code in the same process).  Kernel time from a trace: not measured.", "",
         "| n | bytes / call | sets | calls / window | bv_distill_dist us | GB/s | again us | GB/s | torch ops us | GB/s | torch / fused |",
         "|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in rows:
    f, fa, t = r["bv_distill_dist"], r["bv_distill_dist_again"], r["torch_ops"]
    out.append(f"| {r['n']} | {r['bytes']} | {r['sets']} | {f['calls_per_window']} / {t['calls_per_window']} (torch) "
               f"| {f['median_us']} / {f['best_us']} | {f['GBps_median']} | {fa['median_us']} / {fa['best_us']} "
               f"| {fa['GBps_median']} | {t['median_us']} / {t['best_us']} | {t['GBps_median']} | {t['median_us'] / f['median_us']:.1f}x |")
  out += ["", "Median window length, ms: " + ", ".join(
      f"n={r['n']}: fused {r['bv_distill_dist']['window_ms_median']}, torch {r['torch_ops']['window_ms_median']}" for r in rows) + "."]
  text = "\n".join(out) + "\n"
  print(text)
  if a.out:
    with open(a.out, "w") as fh:
      fh.write(text)
  return 0


if __name__ == "__main__":
  sys.exit(main())
