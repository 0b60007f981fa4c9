"""What is particular to libbvdistill.so on a CPU-only host (what every library must satisfy is in test_libs_cpu.py):
its four entry points and distance kinds, the exact error strings `_lib.call` reports for it, a footprint row for
every entry point and a named parity test for every kernel instantiation, and kernels that use no scratch memory."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from test_libs_cpu import Observer, libs  # noqa: F401  (libs: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bvdistill.h")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_header_equals_the_prototype_table_and_the_exports(libs):
  d = libs.LIBRARIES["distill"]
  assert d.prototypes is libs.PROTOTYPES_DISTILL and len(d.prototypes) == 4 and os.path.samefile(d.header, HEADER)
  assert libs.handle("distill").bv_distill_version() == 1
  from big_vision_amd import build
  assert build.lib("distill").sources == ["distill.hip"]
  assert not [r.key for r in build.LIBS if r.key != "distill" and "distill.hip" in r.sources]
  hdr = open(HEADER).read()
  kinds = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define BVD_KIND_(\w+)\s+(\d+)", hdr) if m.group(1) != "COUNT"}
  assert kinds == libs.DISTILL_KINDS
  for cite in ("evaluators/proj/distill/distance.py:", "trainers/proj/distill/distill.py:", "utils.py:"):
    assert cite in hdr, cite


def test_call_routes_by_table_and_reports_the_right_librarys_error(libs, monkeypatch):
  obs = Observer()
  monkeypatch.setattr(libs, "observer", obs)
  with pytest.raises(RuntimeError, match=r"bv_distill_dist failed \(rc=-1\): bv_distill_dist: bad shape"):
    libs.call("bv_distill_dist", 2, None, None, None, None, None, 0, 0, 0, 0, 1.0, 0.0, 0.0, 1, None)
  with pytest.raises(RuntimeError, match=r"bv_distill_entropy failed \(rc=-1\): bv_distill_entropy: NULL logits"):
    libs.call("bv_distill_entropy", None, None, None, 1, 1, 1, None)
  assert obs == ["bv_distill_dist", "end:bv_distill_dist", "bv_distill_entropy", "end:bv_distill_entropy"]


def test_every_entry_point_has_a_footprint_row(libs):
  import test_distill_footprint_gpu as T
  want = {n for n in libs.PROTOTYPES_DISTILL if n != "bv_distill_version"}
  have = {e for e, _, _ in T.ROWS}
  assert want == have, (sorted(want - have), sorted(have - want))
  ids = [f"{e}-{c}" for e, c, _ in T.ROWS]
  assert len(set(ids)) == len(ids), "duplicate row ids"
  for kind in T.KIND_IDS:                      # every optional-pointer pattern of every kind at C = 5, 257, 1003
    for C in (5, 257, 1003):
      masks = {c for e, c, _ in T.ROWS if c.startswith(f"{kind}-C{C}-mask")}
      assert len(masks) >= (3 if kind == "agree" else 7), (kind, C, masks)


def test_kernel_set_equals_the_list_of_covering_tests(libs):
  sys.path.insert(0, os.path.join(ROOT, "tools"))
  import kernel_inventory as KI
  import test_distill_kernels_gpu as T
  have = set(KI.inventory(lib=libs.LIBRARIES["distill"].path))
  assert have == set(T.KERNELS), (sorted(have - set(T.KERNELS)), sorted(set(T.KERNELS) - have))
  for name, test in T.KERNELS.items():
    assert hasattr(T, test.split("[")[0]), (name, test)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_no_spills_no_scratch(tmp_path):
  cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DNDEBUG", "-x", "hip", "-c",
         os.path.join(ROOT, "big_vision_amd", "csrc", "distill.hip"), "-o", str(tmp_path / "x.o"),
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
  assert len(res) == 24, sorted(res)
  for name, r in res.items():
    assert set(r) == {"VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "VGPRs"}, (name, r)   # all four remarks were parsed
    assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
    assert r.get("ScratchSize [bytes/lane]", 0) == 0, f"{name} uses scratch memory (a run-time-indexed register cache?): {r}"
    assert r.get("VGPRs", 0) <= 256, (name, r)
