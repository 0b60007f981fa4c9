"""Every kernel instantiation compiled into libbvhip.so has an entry in the coverage ledger tests/kernel_coverage.json,
and every ledger entry is still in the library.  The ledger is written by `tools/kernel_inventory.py --trace` from
rocprofv3 kernel traces of the per-kernel parity files (test_kernels_gpu.py, test_gemm256_gpu.py,
test_kernel_buckets_gpu.py, test_adafactor_gpu.py, test_dropout_gpu.py, test_full_size_properties_gpu.py): a new
instantiation without a parity row and a refreshed ledger fails here, and so does a stale entry."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_inventory as KI  # noqa: E402


@pytest.fixture(scope="module")
def symbols():
  from big_vision_amd import build
  build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
  return KI.inventory()


@pytest.fixture(scope="module")
def ledger():
  with open(KI.LEDGER) as f:
    return json.load(f)


def test_inventory_equals_the_ledger(symbols, ledger):
  assert len(symbols) == len(set(symbols)) > 100
  lib, led = set(symbols), set(ledger["kernels"])
  assert not lib - led, f"instantiations without a ledger entry (add a parity row, refresh the ledger): {sorted(lib - led)}"
  assert not led - lib, f"stale ledger entries (no longer in libbvhip.so): {sorted(led - lib)}"


def test_ledger_entries_are_covered_or_waived_with_a_reason(ledger):
  counts = {"covered": 0, "waived": 0}
  for name, e in ledger["kernels"].items():
    assert e["status"] in counts, (name, e)
    counts[e["status"]] += 1
    if e["status"] == "covered":
      assert e["by"] and all(t.startswith("test_") and t.endswith("_gpu.py") for t in e["by"]), (name, e)
    else:
      assert e["reason"].strip(), name
  assert counts == {k: ledger["counts"][k] for k in counts}
  assert ledger["counts"]["symbols"] == len(ledger["kernels"])


def test_dead_instantiations_stay_out():
  """The instantiations no dispatch row can reach were removed: attn4_bwd_dkv_kernel<4, *> (launch_bwd3's 32-key-block
  branch is compile-time attn4_dkv_exists(KF): KF >= 13) and ln_bwd_bfx_kernel<false, *> (a bf16 dy takes the two-row kernel)."""
  with open(KI.LEDGER) as f:
    names = json.load(f)["kernels"]
  assert not [n for n in names if n.startswith("_ZN12_GLOBAL__N_120attn4_bwd_dkv_kernelILi4E")]
  assert not [n for n in names if n.startswith("_ZN12_GLOBAL__N_117ln_bwd_bfx_kernelILb0E")]
