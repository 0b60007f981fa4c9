"""Yardstick of the fused optimizer step (tools only, GPU): bv_adam_step (fp32 moments), SGD-momentum
(bv_trace_step with a bf16 trace, big_vision.momentum_hp) and SGD (bv_trace_step without a trace, big_vision.sgd) over
the flat buffers of 203.2 M parameters (the C3 parameter count), timed with HIP events.

HBM bytes per parameter: Adam 30 (fp32 p r/w, g, mu r/w, nu r/w; bf16 shadow), momentum 18 (p r/w, g, bf16 trace r/w,
shadow), SGD 14 (p r/w, g, shadow).  Also prints a digest of the bits three Adam steps leave in p / mu / nu / shadow, so
two builds of the library can be checked for the same Adam arithmetic.

  python tools/optimizer_yardstick.py [--lib path/to/libbvhip.so] [--iters N] [--out result.json]
"""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

P = (203_200_000 + 1023) // 1024 * 1024
BYTES = {"adam": 30, "momentum": 18, "sgd": 14}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--lib", default=None, help="libbvhip.so to load instead of the in-tree build")
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  from big_vision_amd import _lib
  if args.lib:
    import ctypes
    _lib.LIBRARIES["hip"].path = os.path.abspath(args.lib)
    if not hasattr(ctypes.CDLL(_lib.LIBRARIES["hip"].path), "bv_trace_step"):   # a build from before the trace stage: Adam only
      _lib.PROTOTYPES.pop("bv_trace_step")
  from big_vision_amd import ops
  dev = torch.device("cuda:0")
  torch.cuda.set_device(dev)
  g = torch.Generator(device=dev).manual_seed(0)
  p0 = 0.02 * torch.randn(P, device=dev, generator=g)
  grad = 1e-4 * torch.randn(P, device=dev, generator=g)
  p, shadow = p0.clone(), torch.empty(P, device=dev, dtype=torch.bfloat16)
  mu, nu = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
  trace = torch.zeros(P, device=dev, dtype=torch.bfloat16)
  segs = torch.tensor([[1e-3, 1e-4, 0.0, 0.0]], dtype=torch.float32)
  segs[0, 2:3].view(torch.int32)[0] = 0
  segs = segs.to(dev)
  chunk_seg = torch.zeros(P // 1024, device=dev, dtype=torch.int32)
  # the clip norm from a deterministic reduction (bv_sqnorm's fp64 atomics may differ in the last bits between runs)
  gsq = torch.full((1,), float(grad.double().square().sum()), device=dev, dtype=torch.float64)
  stats = torch.zeros(2, device=dev, dtype=torch.float64)
  sched = [0.5]

  def adam(k=0):
    ops.adam_step_(p, grad, mu, nu, shadow, segs, chunk_seg, P, sched, gsq, 1.0, 0.9, 0.999, 1e-8,
                   1.0 - 0.9 ** (k + 1), 1.0 - 0.999 ** (k + 1), stats)

  def momentum():
    ops.trace_step_(p, grad, trace, shadow, segs, chunk_seg, P, sched, gsq, 1.0, 0.9, False, stats)

  def sgd():
    ops.trace_step_(p, grad, None, shadow, segs, chunk_seg, P, sched, gsq, 1.0, 0.0, False, stats)

  # the bits of three Adam steps from a fixed start
  for k in range(3):
    adam(k)
  torch.cuda.synchronize()
  h = hashlib.sha256()
  for t in (p, mu, nu, shadow):      # (not stats: fp64 atomics in workgroup order)
    h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
  digest = h.hexdigest()

  def timeit(fn):
    for _ in range(args.warmup):
      fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(args.iters):
      e0.record(); fn(); e1.record(); e1.synchronize()
      per.append(e0.elapsed_time(e1))
    per.sort()
    return per[len(per) // 2], per[0]

  res = {"params": P, "adam_bits_sha256": digest, "device": torch.cuda.get_device_name(dev)}
  runs = (("adam", adam), ("momentum", momentum), ("sgd", sgd), ("adam_again", adam))
  if "bv_trace_step" not in _lib.PROTOTYPES:
    runs = (("adam", adam), ("adam_again", adam))
  for name, fn in runs:
    med, best = timeit(fn)
    b = BYTES[name.split("_")[0]] * P
    res[name] = {"median_ms": round(med, 4), "best_ms": round(best, 4), "TBps_median": round(b / (med * 1e-3) / 1e12, 3)}
    print(f"{name:11s} median {med:7.4f} ms  best {best:7.4f} ms  {b / (med * 1e-3) / 1e12:5.2f} TB/s "
          f"({BYTES[name.split('_')[0]]} B/param)", flush=True)
  print("adam bits", digest)
  line = json.dumps(res, sort_keys=True)
  print(line)
  if args.out:
    with open(args.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
