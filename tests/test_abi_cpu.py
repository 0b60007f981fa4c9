"""What is particular to libbvhip.so on a CPU-only host (what every library must satisfy is in test_libs_cpu.py):
the size of its ABI, no process-global state, the cited call sites; the product path refuses to run without a GPU
(no CPU fallback).  No compute calls are made here."""
import ctypes
import os
import re

import pytest
import torch

from test_libs_cpu import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bvhip.h")


@pytest.fixture(scope="module")
def lib():
  from big_vision_amd import build, _lib
  build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
  return _lib.load()


def test_header_declares_entry_points():
  syms = header_symbols(HEADER)
  assert "bv_gemm_bf16" in syms and "bv_siglip_loss" in syms and "bv_adam_step" in syms
  assert len(syms) >= 20


def test_python_prototypes_cover_the_header(lib):
  from big_vision_amd import _lib
  assert len(header_symbols(HEADER)) == len(_lib.PROTOTYPES) + 1 == 71            # + bv_last_error
  assert lib.bv_version() == 2


def test_library_keeps_no_process_global_state(lib):
  """SURVEY.md 8b / VERDICT r4 #6: options, split-K workspace and launch counters live in a caller-owned `bv_ctx`;
  the header's state paragraph names the last-error string only, the old process-global setters are gone from the
  ABI, the library's data segment holds no writable globals besides the thread-local error buffer and caches, and
  two contexts do not see each other's options."""
  import subprocess
  src = open(HEADER).read()
  para = src[src.index("thread-safe per stream"):src.index("#ifndef BVHIP_H_")]
  assert "NO process-global state besides" in para and "last-error string" in para
  for gone in ("bv_gemm_tune", "bv_gemm_roll", "bv_gemm_reserve_cus", "bv_gemm_group_n", "bv_gemm_pre_issue",
               "bv_gemm_fast_path", "bv_attn_impl", "bv_attn_tune", "bv_sgemm_path", "bv_set_workspace",
               "bv_set_stream_workspace", "bv_gemm256_calls"):
    assert gone not in header_symbols(HEADER) and not hasattr(ctypes.CDLL(os.path.join(ROOT, "big_vision_amd", "libbvhip.so")), gone), gone
  # source level: no mutable namespace-scope variable in csrc besides the thread-local error buffer and the
  # one-time RCCL binding table (+ its mutex) of comm.cpp; function-local `static` caches hold device properties only
  decl = re.compile(r"^(?:static |thread_local |extern )*(?:std::\w+(?:<[^>]*>)? |unsigned |int |long |bool |float |"
                    r"double |char |void\* |\w+ )(g_\w+)\b[^()]*[;=]", re.M)
  found = {}
  csrc = os.path.join(ROOT, "big_vision_amd", "csrc")
  for f in sorted(os.listdir(csrc)):
    txt = re.sub(r"//.*", "", open(os.path.join(csrc, f)).read())
    for m in decl.finditer(txt):
      if "__device__" not in txt[max(0, m.start() - 20):m.start() + 12]:
        found.setdefault(m.group(1), f)
  assert set(found) <= {"g_err", "g_rccl", "g_mu"}, found
  statics = []
  for f in sorted(os.listdir(csrc)):
    for ln in open(os.path.join(csrc, f)):
      if re.match(r"\s+static (?!const|constexpr|_assert|inline)\w", ln) and "static_assert" not in ln:
        statics.append((f, ln.strip()))
  assert all("cus = 0" in l or "dflt" in l for _, l in statics), statics
  a, b = lib.bv_ctx_create(), lib.bv_ctx_create()
  try:
    from big_vision_amd._lib import OPTS
    assert lib.bv_ctx_get(a, OPTS["gemm_roll"]) == 1 and lib.bv_ctx_get(None, OPTS["gemm_roll"]) == 1
    assert lib.bv_ctx_set(a, OPTS["gemm_roll"], 7) == 1 and lib.bv_ctx_get(a, OPTS["gemm_roll"]) == 7
    assert lib.bv_ctx_get(b, OPTS["gemm_roll"]) == 1 and lib.bv_ctx_get(None, OPTS["gemm_roll"]) == 1
    assert lib.bv_ctx_set(a, OPTS["gemm_reserve_cus"], 500) == 0 and lib.bv_ctx_get(a, OPTS["gemm_reserve_cus"]) == 128
    assert lib.bv_ctx_set(None, OPTS["gemm_roll"], 0) < 0 and b"NULL context" in lib.bv_last_error()
    assert lib.bv_ctx_set(a, 55, 0) < 0 and lib.bv_ctx_get(a, 55) < 0
    assert lib.bv_ctx_get(a, OPTS["gemm256_calls"]) == 0
    assert lib.bv_ctx_set_workspace(a, None, 0) == 0 and lib.bv_ctx_set_workspace(None, None, 0) != 0
  finally:
    lib.bv_ctx_destroy(a); lib.bv_ctx_destroy(b)


def test_header_cites_reference_call_sites():
  src = open(HEADER).read()
  for cite in ("models/vit.py:", "trainers/proj/image_text/siglip.py:", "optax.py:",
               "models/proj/image_text/two_towers.py:", "models/proj/image_text/text_transformer.py:"):
    assert cite in src, cite


def test_product_path_has_no_cpu_fallback():
  from big_vision_amd import ops
  a = torch.zeros(8, 8, dtype=torch.bfloat16)
  with pytest.raises(RuntimeError, match="GPU"):
    ops.gemm(a, a)
  with pytest.raises(RuntimeError, match="GPU"):
    ops.layernorm_fwd(torch.zeros(4, 8), torch.ones(8), torch.zeros(8), rows=4, D=8)


def test_product_never_imports_the_oracle():
  pkg = os.path.join(ROOT, "big_vision_amd")
  for d, _, files in os.walk(pkg):
    for f in files:
      if f.endswith((".py", ".hip", ".cpp", ".h")):
        txt = open(os.path.join(d, f)).read()
        assert "bv_oracle" not in txt and "import oracle" not in txt, os.path.join(d, f)


def test_comm_layer_binds_rccl_at_run_time():
  """bv_comm_* (csrc/comm.cpp) has no link-time RCCL dependency: the library loads on a host without a GPU and the
  first call binds the RCCL that is already in the process (PyTorch's) - one RCCL per process."""
  import ctypes
  import subprocess
  from big_vision_amd import _lib
  lib = _lib.load()
  v = ctypes.c_int(0)
  assert lib.bv_comm_version(ctypes.byref(v)) == 0 and v.value >= 20000, lib.bv_last_error()
  needed = subprocess.run(["readelf", "-d", _lib.LIBRARIES["hip"].path], capture_output=True, text=True).stdout
  assert "rccl" not in needed.lower(), "libbvhip.so must not link RCCL"
  assert lib.bv_comm_init(None, 0, 1, None) != 0 and b"bad arguments" in lib.bv_last_error()


def test_python_contexts_are_per_stream_and_options_restore(lib, monkeypatch):
  """big_vision_amd.ops keeps one bv_ctx per (device, stream); `ops.option` restores the previous value; BV_CTX_OPTS
  seeds every new context (whole-program A/B runs).  Host logic only: no kernel is launched."""
  from big_vision_amd import ops
  monkeypatch.setattr(ops, "_contexts", {})
  stream = {"id": 11}
  monkeypatch.setattr(ops, "_stream", lambda: stream["id"])
  a = ops.ctx()
  assert ops.ctx() is a and a.get("gemm_roll") == 1
  with ops.option("gemm_roll", 6) as o:
    assert o.old == 1 and ops.ctx_get("gemm_roll") == 6
    stream["id"] = 12                      # another stream: its own context, default options
    b = ops.ctx()
    assert b is not a and b.get("gemm_roll") == 1
    stream["id"] = 11
  assert ops.ctx_get("gemm_roll") == 1
  with pytest.raises(KeyError):
    a.set("no_such_option", 1)
  monkeypatch.setenv("BV_CTX_OPTS", "gemm_nt=1, gemm_group_n=4")
  stream["id"] = 13
  c = ops.ctx()
  assert c.get("gemm_nt") == 1 and c.get("gemm_group_n") == 4 and a.get("gemm_nt") == 0


def test_epilogue_and_option_codes_match_the_header():
  """The ctypes side spells the epilogue / option codes as Python constants: every BV_EPI_* and BV_OPT_* of
  include/bvhip.h has the same value in big_vision_amd/_lib.py (BV_EPI_GELU_G = 9 joined in round 6)."""
  import re
  from big_vision_amd import _lib
  hdr = open(os.path.join(ROOT, "include", "bvhip.h")).read()
  epi = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define BV_EPI_(\w+)\s+(\d+)", hdr)}
  assert len(epi) >= 10 and epi["GELU_G"] == 9
  for name, val in epi.items():
    assert getattr(_lib, f"EPI_{name}") == val, name
  opt = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define BV_OPT_(\w+)\s+(\d+)", hdr) if m.group(1) != "COUNT"}
  for name, val in opt.items():
    assert _lib.OPTS[name] == val, name
