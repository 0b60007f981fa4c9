"""Build libbvhip.so, libbvdistill.so and libbveval.so (hand-written HIP kernels for gfx950) in-tree with hipcc.

hipcc cross-compiles for gfx950 without a GPU, so this runs in the CPU-only
build container; the resulting big_vision_amd/libbvhip.so travels to the GPU box
with the repo snapshot.

Build-time requirements: hipcc and the ROCm headers, including <rccl/rccl.h> (csrc/comm.cpp takes the
ncclComm_t / ncclDataType_t types and the prototypes of the eight entry points it binds from it).  There
is NO link-time RCCL dependency: comm.cpp dlopen()s librccl.so at the first bv_comm_* call, so the
library loads on hosts without RCCL as long as nothing calls those entry points.
"""
import collections
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(HERE, "..", "include")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
         "-DNDEBUG"]
MAX_JOBS = 16   # compiler processes in flight at once

# One record per kernel library: its key (big_vision_amd/_lib.py binds by the same key), the shared object, the
# public header that declares its C ABI and its sources under csrc/.  Everything below iterates this table.
Lib = collections.namedtuple("Lib", "key path header sources")
LIBS = [
    Lib("hip", os.path.join(HERE, "libbvhip.so"), os.path.join(INCLUDE, "bvhip.h"),
        ["c_api.cpp", "comm.cpp", "gemm_bf16.hip", "gemm256.hip", "attention.hip", "attention3.hip", "attention5.hip",
         "attention_dh.hip", "layernorm.hip", "elementwise.hip", "loss_optim.hip", "adafactor.hip", "dropout.hip"]),
    Lib("distill", os.path.join(HERE, "libbvdistill.so"), os.path.join(INCLUDE, "bvdistill.h"), ["distill.hip"]),
    Lib("eval", os.path.join(HERE, "libbveval.so"), os.path.join(INCLUDE, "bveval.h"), ["eval.hip"]),
]


def lib(key):
  return next(r for r in LIBS if r.key == key)


def _headers():
  return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [r.header for r in LIBS]


def _stale():
  deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + _headers()
  newest = max(os.path.getmtime(d) for d in deps)
  return any(not os.path.exists(r.path) or os.path.getmtime(r.path) < newest for r in LIBS)


def build(force=False, verbose=True):
  """Compiles what is stale and links every library of LIBS; returns the path of libbvhip.so."""
  hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  if not force and not _stale():
    return lib("hip").path
  if not os.path.exists(hipcc):
    raise RuntimeError("hipcc not found: cannot build " + " / ".join(os.path.basename(r.path) for r in LIBS))
  objdir = os.path.join(HERE, "build")
  os.makedirs(objdir, exist_ok=True)
  hdr_t = max(os.path.getmtime(h) for h in _headers())
  todo = []
  for src in [src for r in LIBS for src in r.sources]:
    obj = os.path.join(objdir, os.path.splitext(src)[0] + ".o")
    # per-object staleness: only the sources that changed (or everything, after a header edit)
    if (not force and os.path.exists(obj) and
        os.path.getmtime(obj) > max(hdr_t, os.path.getmtime(os.path.join(CSRC, src)))):
      continue
    todo.append((src, [hipcc, *FLAGS, "-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]))
  running = []

  def reap(src, p):
    out, _ = p.communicate()
    if p.returncode != 0:
      sys.stderr.write(out.decode())
      raise RuntimeError(f"hipcc failed on {src}")

  for src, cmd in todo:
    if len(running) >= MAX_JOBS:
      reap(*running.pop(0))
    if verbose:
      print(" ".join(cmd), flush=True)
    running.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
  for src, p in running:
    reap(src, p)
  for r in LIBS:
    objs = [os.path.join(objdir, os.path.splitext(src)[0] + ".o") for src in r.sources]
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", r.path]
    if verbose:
      print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
  return lib("hip").path


if __name__ == "__main__":
  build(force="--force" in sys.argv)
  print("built", *[r.path for r in LIBS])
