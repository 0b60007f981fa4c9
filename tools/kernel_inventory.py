"""Inventory of the GPU kernels compiled into big_vision_amd/libbvhip.so, and the coverage ledger built on it.

    python tools/kernel_inventory.py                       # one mangled kernel name per line, sorted
    python tools/kernel_inventory.py --trace T.csv [...]   # rewrite tests/kernel_coverage.json from kernel traces

The library is a host object with one `.hip_fatbin` section: a concatenation of clang offload bundles, one per
translation unit.  Each bundle holds the gfx950 code object of its source file; every kernel entry point there has
a `<mangled name>.kd` kernel-descriptor symbol.  Names stay mangled throughout (the bf16 type mangles as `DF16b`,
which older c++filt builds do not demangle), so they compare byte-for-byte with a `rocprofv3 -M` kernel trace.

--trace takes one or more `--kernel-trace -M -f csv` files of the per-kernel parity tests.  Each CSV may be given as
`TESTFILE=PATH` to record which test file launched its kernels; a plain PATH records the file name of the CSV.  The
ledger lists every inventory symbol as `covered` (by which test file) or `waived` (with a reason, kept from the
WAIVERS table below); a symbol that no trace launched and that has no waiver is an error.
"""
import argparse
import csv
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "big_vision_amd", "libbvhip.so")
LEDGER = os.path.join(ROOT, "tests", "kernel_coverage.json")
LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

# symbol -> reason: kernels the parity tests cannot launch by construction (none today)
WAIVERS = {}


def _tool(name):
  p = os.path.join(os.environ.get("BV_LLVM_BIN", LLVM), name)
  if not os.path.exists(p):
    raise FileNotFoundError(f"{name} not found at {p} (set BV_LLVM_BIN to the ROCm LLVM bin directory)")
  return p


def inventory(lib=LIB):
  """Sorted list of the mangled kernel names (`.kd` symbols without the suffix) in `lib`'s gfx950 code objects."""
  names = set()
  with tempfile.TemporaryDirectory() as tmp:
    fatbin = os.path.join(tmp, "fatbin")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fatbin}", lib,
                    os.path.join(tmp, "stripped")], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    blob = open(fatbin, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    if not starts:
      raise RuntimeError(f"{lib}: no clang offload bundle in .hip_fatbin")
    for i, s in enumerate(starts):
      piece = os.path.join(tmp, f"b{i}.bundle")
      with open(piece, "wb") as f:
        f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
      co = os.path.join(tmp, f"b{i}.co")
      subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                      f"--input={piece}", f"--output={co}"], check=True, stdout=subprocess.PIPE,
                     stderr=subprocess.STDOUT)
      if not os.path.getsize(co):
        continue
      out = subprocess.run([_tool("llvm-readelf"), "-s", "--wide", co], check=True, stdout=subprocess.PIPE,
                           text=True).stdout
      for line in out.splitlines():
        f = line.split()
        if len(f) >= 8 and f[-1].endswith(".kd"):
          names.add(f[-1][:-3])
  return sorted(names)


def traced_kernels(path):
  """Mangled kernel names launched in one rocprofv3 kernel-trace CSV."""
  with open(path, newline="") as f:
    rows = csv.DictReader(f)
    col = next(c for c in rows.fieldnames if c in ("Kernel_Name", "Kernel-Name", "KernelName"))
    # rocprofv3 -M reports the kernel-descriptor symbol itself (`<name>.kd`)
    return {re.sub(r"\.kd$", "", r[col].strip()) for r in rows}


def ledger(symbols, traces, waivers=WAIVERS):
  """traces: [(test file, set of launched names)].  Returns the ledger dict; raises on an uncovered symbol."""
  entries, missing = {}, []
  for s in symbols:
    by = sorted({t for t, launched in traces if s in launched})
    if by:
      entries[s] = {"status": "covered", "by": by}
    elif s in waivers:
      entries[s] = {"status": "waived", "reason": waivers[s]}
    else:
      missing.append(s)
  if missing:
    raise SystemExit("no trace launched, and no waiver names:\n  " + "\n  ".join(missing))
  return {"library": "big_vision_amd/libbvhip.so",
          "counts": {"symbols": len(symbols),
                     "covered": sum(e["status"] == "covered" for e in entries.values()),
                     "waived": sum(e["status"] == "waived" for e in entries.values())},
          "kernels": entries}


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  ap.add_argument("--lib", default=LIB)
  ap.add_argument("--trace", nargs="+", metavar="[TESTFILE=]CSV")
  ap.add_argument("--out", default=LEDGER)
  a = ap.parse_args(argv)
  syms = inventory(a.lib)
  if not a.trace:
    print("\n".join(syms))
    print(f"{len(syms)} kernels", file=sys.stderr)
    return
  traces = []
  for t in a.trace:
    name, _, path = t.rpartition("=")
    traces.append((name or os.path.basename(path), traced_kernels(path)))
  led = ledger(syms, traces)
  with open(a.out, "w") as f:
    json.dump(led, f, indent=1, sort_keys=True)
    f.write("\n")
  print(f"{a.out}: {led['counts']}")


if __name__ == "__main__":
  main()
