"""What is particular to libbveval.so on a CPU-only host (what every library must satisfy is in test_libs_cpu.py):
its one entry point and two losses, the exact error strings `_lib.call` reports for it, its footprint rows and a named
parity test for each of its eight kernels, and kernels that use no scratch memory."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from test_libs_cpu import Observer, libs  # noqa: F401  (libs: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bveval.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_header_equals_the_prototype_table_and_the_exports(libs):
  d = libs.LIBRARIES["eval"]
  assert d.prototypes is libs.PROTOTYPES_EVAL and len(d.prototypes) == 2 and os.path.samefile(d.header, HEADER)
  assert libs.handle("eval").bv_eval_version() == 1
  from big_vision_amd import build
  assert build.lib("eval").sources == ["eval.hip"] and build.LIBS[-1].key == "eval"
  assert not [r.key for r in build.LIBS if r.key != "eval" and "eval.hip" in r.sources]
  hdr = open(HEADER).read()
  losses = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define BVE_LOSS_(\w+)\s+(\d+)", hdr) if m.group(1) != "COUNT"}
  assert losses == libs.EVAL_LOSSES == {"softmax_xent": 0, "sigmoid_xent": 1}
  for cite in ("evaluators/classification.py:", "utils.py:"):
    assert cite in hdr, cite
  import _eval_bounds as B
  assert int(re.search(r"#define BVE_WAVE_ROW_MAX_C\s+(\d+)", hdr).group(1)) == B.WAVE_ROW_MAX_C


def test_call_routes_by_table_and_reports_the_right_librarys_error(libs, monkeypatch):
  obs = Observer()
  monkeypatch.setattr(libs, "observer", obs)
  with pytest.raises(RuntimeError, match=r"bv_eval_classify failed \(rc=-1\): bv_eval_classify: bad shape n=0 C=5"):
    libs.call("bv_eval_classify", 0, None, None, None, None, None, None, 0, 5, None)
  with pytest.raises(RuntimeError, match=r"bv_eval_classify failed \(rc=-1\): bv_eval_classify: unknown loss kind 7"):
    libs.call("bv_eval_classify", 7, None, None, None, None, None, None, 1, 5, None)
  with pytest.raises(RuntimeError, match=r"bv_eval_classify failed \(rc=-1\): bv_eval_classify: NULL logits or labels"):
    libs.call("bv_eval_classify", 1, None, None, None, None, None, None, 1, 5, None)
  # the other libraries still answer with their own strings
  with pytest.raises(RuntimeError, match=r"bv_distill_entropy failed \(rc=-1\): bv_distill_entropy: NULL logits"):
    libs.call("bv_distill_entropy", None, None, None, 1, 1, 1, None)
  assert obs == ["bv_eval_classify", "end:bv_eval_classify"] * 3 + ["bv_distill_entropy", "end:bv_distill_entropy"]
  assert libs.handle("eval").bv_eval_last_error() == b"bv_eval_classify: NULL logits or labels"


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
  have = set(KI.inventory(lib=libs.LIBRARIES["eval"].path))
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
