"""What holds for every kernel library on a CPU-only host, checked once over the table of libraries (build.LIBS and
the descriptors of `_lib.LIBRARIES`): each loads, exports exactly what its public header declares, `_lib` binds it and
routes calls to it by table, its status codes are bvhip.h's, and no two libraries share an entry point.  What is
particular to one library is in test_abi_cpu.py, test_distill_abi_cpu.py and test_eval_abi_cpu.py."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import pytest

from big_vision_amd import build

KEYS = [r.key for r in build.LIBS]


def header_symbols(header):
  """The entry points a public header declares (sorted)."""
  src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
  return sorted(set(re.findall(r"^(?:int|long|void|bv_ctx\*|const char\*)\s+(bv_\w+)\s*\(", src, re.M)))


@pytest.fixture(scope="module")
def libs():
  from big_vision_amd import _lib
  build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
  _lib.load()
  return _lib


class Observer(list):      # the protocol of `_lib.observer`; the list is what it saw
  def begin(self, name, args):
    self.append(name)
    return name

  def end(self, tok):
    self.append("end:" + tok)


def test_build_table_and_descriptors_name_the_same_files(libs):
  assert KEYS == list(libs.LIBRARIES) == ["hip", "distill", "eval"]     # a new library adds its key here
  for r in build.LIBS:
    d = libs.LIBRARIES[r.key]
    assert os.path.samefile(r.path, d.path) and os.path.samefile(r.header, d.header)
    assert r is build.lib(r.key) and d.dll is libs.handle(r.key)
    for src in r.sources:               # a source belongs to one library
      assert os.path.exists(os.path.join(build.CSRC, src)), src
      assert [o.key for o in build.LIBS if src in o.sources] == [r.key], src
  assert build.build(verbose=False) == build.lib("hip").path and libs.load() is libs.handle("hip")


@pytest.mark.parametrize("key", KEYS)
def test_header_equals_the_prototype_table_and_the_exports(libs, key):
  d = libs.LIBRARIES[key]
  syms = header_symbols(d.header)
  assert sorted(list(d.prototypes) + [d.last_error]) == syms
  raw = ctypes.CDLL(d.path)
  for s in syms:
    assert hasattr(raw, s), f"{d.name} does not export {s} (declared in include/{os.path.basename(d.header)})"
  exported = subprocess.run(["nm", "-D", "--defined-only", d.path], stdout=subprocess.PIPE, text=True,
                            check=True).stdout if shutil.which("nm") else ""
  if exported:      # nothing else of the bv_ namespace leaves the library
    assert sorted(set(re.findall(r"\b(bv_\w+)$", exported, re.M))) == syms
  declared = re.findall(r"#define BV\w*_VERSION\s+(\d+)", open(d.header).read())
  assert [int(v) for v in declared] == [d.version] == [getattr(libs.handle(key), d.version_fn)()]


@pytest.mark.parametrize("key", KEYS)
def test_status_codes_are_those_of_bvhip(libs, key):
  first = open(build.lib("hip").header).read()
  codes = {m.group(1): int(m.group(2)) for m in
           re.finditer(r"#define BV[A-Z]?_(OK|ERR_\w+)\s+\(?(-?\d+)\)?", open(libs.LIBRARIES[key].header).read())}
  assert set(codes) == {"OK", "ERR_INVALID_ARG", "ERR_UNSUPPORTED", "ERR_HIP"}
  for name, value in codes.items():
    assert int(re.search(r"#define BV_" + name + r"\s+\(?(-?\d+)\)?", first).group(1)) == value, name


def test_the_libraries_share_no_entry_point(libs):
  for a, b in itertools.permutations(KEYS, 2):
    da, db = libs.LIBRARIES[a], libs.LIBRARIES[b]
    assert not set(da.prototypes) & set(db.prototypes), (a, b)
    raw = ctypes.CDLL(da.path)
    assert not [n for n in list(db.prototypes) + [db.last_error] if hasattr(raw, n)], (a, b)
    prefix = db.version_fn[:-len("version")]             # bv_distill_, bv_eval_; libbvhip's is all of bv_
    if prefix != "bv_":
      assert not [s for s in header_symbols(da.header) if s.startswith(prefix)], (a, b)


def test_call_finds_every_entry_point_in_the_library_that_declares_it(libs):
  declared = {}
  for key in KEYS:
    d = libs.LIBRARIES[key]
    for name in header_symbols(d.header):
      if name != d.last_error:
        declared[name] = d
    for name in d.prototypes:
      assert libs._owner[name] is d and declared[name] is d, (key, name)
  assert set(libs._owner) == set(declared), set(libs._owner) ^ set(declared)


STUB = r"""
#include <stdio.h>
static _Thread_local char err[64] = "";
const char* bv_stub_last_error(void) { return err; }
int bv_stub_version(void) { return 1; }
int bv_stub_fail(int x) { snprintf(err, sizeof(err), "bv_stub_fail: refused %d", x); return -1; }
"""


def test_a_fourth_library_needs_only_a_record(libs, tmp_path, monkeypatch):
  """A host-only library with the three obligatory pieces (version, last error, status returns) is bound, routed,
  observed and reported by the code that serves the shipped ones: nothing but its descriptor is written here."""
  cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  (tmp_path / "stub.c").write_text(STUB)
  so = str(tmp_path / "libbvstub.so")
  subprocess.run([cc, "-shared", "-fPIC", "-x", "c", str(tmp_path / "stub.c"), "-o", so], check=True)
  stub = libs.Library(so, None, {"bv_stub_version": [], "bv_stub_fail": [ctypes.c_int]},
                      last_error="bv_stub_last_error", version_fn="bv_stub_version", version=1)
  monkeypatch.setattr(libs, "_owner", dict(libs._owner))      # what binding the stub adds goes with the test
  monkeypatch.setitem(libs.LIBRARIES, "stub", stub)
  obs = Observer()
  monkeypatch.setattr(libs, "observer", obs)
  assert libs.load() is libs.handle("hip") and libs._owner["bv_stub_fail"] is stub
  with pytest.raises(RuntimeError, match=r"^bv_stub_fail failed \(rc=-1\): bv_stub_fail: refused 7$"):
    libs.call("bv_stub_fail", 7)
  with pytest.raises(RuntimeError, match=r"^bv_ctx_set_workspace failed \(rc=-1\): bv_ctx_set_workspace: NULL context"):
    libs.call("bv_ctx_set_workspace", None, None, 0)
  assert obs == ["bv_stub_fail", "end:bv_stub_fail", "bv_ctx_set_workspace", "end:bv_ctx_set_workspace"]
  assert libs.handle("stub").bv_stub_last_error() == b"bv_stub_fail: refused 7"     # each library keeps its own
  with pytest.raises(AttributeError):
    libs.call("bv_stub_unknown")
