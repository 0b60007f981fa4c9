"""libbveval.so on a CPU-only host: it loads, exports exactly what include/bveval.h declares, `_lib` binds it next to
the other two libraries and routes calls by table, the entry point has its footprint rows and every kernel
instantiation a named parity test, the kernels use no scratch memory, and the other two libraries' tables are what
they were."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bveval.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _symbols(header, prefix):
  src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
  return sorted(set(re.findall(r"^(?:int|long|void|bv_ctx\*|const char\*)\s+(" + prefix + r"\w+)\s*\(", src, re.M)))


@pytest.fixture(scope="module")
def libs():
  from big_vision_amd import build, _lib
  build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
  _lib.load()
  return _lib


def test_header_equals_the_prototype_table_and_the_exports(libs):
  syms = _symbols(HEADER, "bv_eval_")
  assert sorted(list(libs.PROTOTYPES_EVAL) + ["bv_eval_last_error"]) == syms
  raw = ctypes.CDLL(libs.LIB_EVAL_PATH)
  for s in syms:
    assert hasattr(raw, s), f"libbveval.so does not export {s} (declared in include/bveval.h)"
  exported = subprocess.run(["nm", "-D", "--defined-only", libs.LIB_EVAL_PATH], stdout=subprocess.PIPE, text=True,
                            check=True).stdout if shutil.which("nm") else ""
  if exported:      # nothing else of the bv_ namespace leaves the library
    assert sorted(set(re.findall(r"\b(bv_\w+)$", exported, re.M))) == syms
  assert libs.load_eval().bv_eval_version() == 1
  hdr = open(HEADER).read()
  assert int(re.search(r"#define BVEVAL_VERSION\s+(\d+)", hdr).group(1)) == 1
  losses = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define BVE_LOSS_(\w+)\s+(\d+)", hdr) if m.group(1) != "COUNT"}
  assert losses == libs.EVAL_LOSSES == {"softmax_xent": 0, "sigmoid_xent": 1}
  codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define BVE_(OK|ERR_\w+)\s+\(?(-?\d+)\)?", hdr)}
  first = open(os.path.join(ROOT, "include", "bvhip.h")).read()
  for name, value in codes.items():     # the values of bvhip.h
    assert int(re.search(r"#define BV_" + name + r"\s+\(?(-?\d+)\)?", first).group(1)) == value, name
  assert set(codes) == {"OK", "ERR_INVALID_ARG", "ERR_UNSUPPORTED", "ERR_HIP"}
  for cite in ("evaluators/classification.py:", "utils.py:"):
    assert cite in hdr, cite
  import _eval_bounds as B
  assert int(re.search(r"#define BVE_WAVE_ROW_MAX_C\s+(\d+)", hdr).group(1)) == B.WAVE_ROW_MAX_C


def test_the_three_libraries_share_no_entry_point_and_the_others_are_unchanged(libs):
  tables = (libs.PROTOTYPES, libs.PROTOTYPES_DISTILL, libs.PROTOTYPES_EVAL)
  for i, a in enumerate(tables):
    for b in tables[i + 1:]:
      assert not set(a) & set(b)
  first = _symbols(os.path.join(ROOT, "include", "bvhip.h"), "bv_")
  assert len(first) == len(libs.PROTOTYPES) + 1 == 71
  assert not [s for s in first if s.startswith("bv_eval_")]
  assert len(libs.PROTOTYPES_DISTILL) == 4
  for path in (libs.LIB_PATH, libs.LIB_DISTILL_PATH):
    assert not hasattr(ctypes.CDLL(path), "bv_eval_classify"), path
  from big_vision_amd import build
  assert build.EVAL_SOURCES == ["eval.hip"]
  assert "eval.hip" not in build.SOURCES and "eval.hip" not in build.DISTILL_SOURCES
  assert build.LIBS[-1] == (build.LIB_EVAL, build.EVAL_SOURCES) and len(build.LIBS) == 3
  assert os.path.samefile(build.LIB_EVAL, libs.LIB_EVAL_PATH)


def test_call_routes_by_table_and_reports_the_right_librarys_error(libs, monkeypatch):
  seen = []

  class Obs:
    def begin(self, name, args):
      seen.append(name)
      return name

    def end(self, tok):
      seen.append("end:" + tok)
  monkeypatch.setattr(libs, "observer", Obs())
  with pytest.raises(RuntimeError, match=r"bv_eval_classify failed \(rc=-1\): bv_eval_classify: bad shape n=0 C=5"):
    libs.call("bv_eval_classify", 0, None, None, None, None, None, None, 0, 5, None)
  with pytest.raises(RuntimeError, match=r"bv_eval_classify failed \(rc=-1\): bv_eval_classify: unknown loss kind 7"):
    libs.call("bv_eval_classify", 7, None, None, None, None, None, None, 1, 5, None)
  with pytest.raises(RuntimeError, match=r"bv_eval_classify failed \(rc=-1\): bv_eval_classify: NULL logits or labels"):
    libs.call("bv_eval_classify", 1, None, None, None, None, None, None, 1, 5, None)
  # the other libraries still answer with their own strings
  with pytest.raises(RuntimeError, match=r"bv_distill_entropy failed \(rc=-1\): bv_distill_entropy: NULL logits"):
    libs.call("bv_distill_entropy", None, None, None, 1, 1, 1, None)
  assert seen == ["bv_eval_classify", "end:bv_eval_classify"] * 3 + ["bv_distill_entropy", "end:bv_distill_entropy"]
  assert libs.load_eval().bv_eval_last_error() == b"bv_eval_classify: NULL logits or labels"


def test_ops_wrapper_refuses_cpu_tensors_and_unknown_losses(libs):
  import torch
  from big_vision_amd import ops
  with pytest.raises(RuntimeError, match="GPU"):
    ops.eval_classify("sigmoid_xent", torch.zeros(2, 8), torch.zeros(2, 8))
  with pytest.raises(AttributeError, match="nope"):
    ops.eval_classify("nope", torch.zeros(2, 8), torch.zeros(2, 8))


def test_every_entry_point_has_a_footprint_row(libs):
  import test_eval_footprint_gpu as T
  want = {n for n in libs.PROTOTYPES_EVAL if n != "bv_eval_version"}
  have = {e for e, _, _ in T.ROWS}
  assert want == have, (sorted(want - have), sorted(have - want))
  ids = [f"{e}-{c}" for e, c, _ in T.ROWS]
  assert len(set(ids)) == len(ids), "duplicate row ids"
  for loss in libs.EVAL_LOSSES:               # every optional-pointer pattern of either loss at C = 5, 257, 1003
    for C in (5, 257, 1003):
      masks = {c for e, c, _ in T.ROWS if c.startswith(f"{loss}-C{C}-mask")}
      assert len(masks) == 14, (loss, C, masks)       # 2 (mask) x 7 (non-empty sets of the three outputs)


def test_kernel_set_equals_the_list_of_covering_tests(libs):
  sys.path.insert(0, os.path.join(ROOT, "tools"))
  import kernel_inventory as KI
  import test_eval_kernels_gpu as T
  have = set(KI.inventory(lib=libs.LIB_EVAL_PATH))
  assert have == set(T.KERNELS), (sorted(have - set(T.KERNELS)), sorted(set(T.KERNELS) - have))
  assert len(have) == 8                       # 2 losses x 2 load widths x 2 row mappings
  for name, test in T.KERNELS.items():
    assert hasattr(T, test.split("[")[0]), (name, test)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_no_spills_no_scratch(tmp_path):
  cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DNDEBUG", "-x", "hip", "-c",
         os.path.join(ROOT, "big_vision_amd", "csrc", "eval.hip"), "-o", str(tmp_path / "x.o"),
         "-Rpass-analysis=kernel-resource-usage"]
  out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
  res, name = {}, None
  for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
      name = m.group(1)
      res[name] = {}
    for key in ("VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "VGPRs"):
      m = re.search(re.escape(key) + r": (\d+)", line)
      if m and name and key not in res[name]:
        res[name][key] = int(m.group(1))
  assert len(res) == 8, sorted(res)
  for name, r in res.items():
    assert set(r) == {"VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "VGPRs"}, (name, r)   # all four remarks were parsed
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    assert r["ScratchSize [bytes/lane]"] == 0, f"{name} uses scratch memory: {r}"
    assert r["VGPRs"] <= 256, (name, r)
