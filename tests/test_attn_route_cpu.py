"""The self-attention routing has one owner, big_vision_amd/csrc/attn_route.h, and what the tests believe about it is
held to it here: the header is compiled into a host program (tests/attn_route_dump.cpp: the system C++ compiler, no
HIP, no GPU) whose table is compared with tests/_bounds.py::attn_bwd_path for every shape, with the instantiation
table of tests/test_kernel_buckets_gpu.py at its rows, and with ops.py's choice of entry point."""
import os
import shutil
import subprocess

import pytest

import _bounds as B
import test_kernel_buckets_gpu as KB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
FAMILY = {("adh", "adh"): "adh", ("attn5", "attn5"): "attn5", ("attn3", "dq+dkv"): "attn3 dq+dkv",
          ("attn3", "dq1+dkv"): "attn3 dq1+dkv", ("attn3", "dq1+dkv32"): "attn3 dq1+attn4 dkv32"}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
  assert CXX, "no host C++ compiler"
  exe = str(tmp_path_factory.mktemp("route") / "attn_route_dump")
  subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "attn_route_dump.cpp"), "-o", exe],
                 check=True)

  def run(lmax, *cfgs):
    out = subprocess.run([exe, str(lmax), *map(str, cfgs)], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
      L, Dh, masked, cfg, fkf, fwd, fam, bkf, bwd, dpp = line.split("\t")
      table[int(L), int(Dh), bool(int(masked)), int(cfg)] = (int(fkf), fwd, fam, int(bkf), bwd, bool(int(dpp)))
    assert len(table) == lmax * 16 * 2 * len(cfgs)
    return table
  return run


@pytest.fixture(scope="module")
def default_table(dump):
  return dump(2100, 0, 128)


def test_backward_family_equals_attn_bwd_path_for_every_shape(default_table):
  """Every L in 1..2100, Dh in 8, 16 .. 128, masked and unmasked, attn_cfg 0 and 128 (one-launch kernel off)."""
  bad = []
  for (L, Dh, masked, cfg), (_, _, fam, _, bwd, _) in default_table.items():
    shape = "+".join(k.split("<")[0] for k in bwd.split("+"))   # dq1<..>+dkv32<..> -> dq1+dkv32
    if FAMILY[fam, shape] != B.attn_bwd_path(L, Dh, masked, one_launch=not (cfg & 128)):
      bad.append((L, Dh, masked, cfg, fam, bwd))
  assert not bad, bad[:20]


def test_forward_and_backward_share_the_key_fragments(default_table):
  """The backward reads an lse laid out by the forward's instantiation: same KF for every shape of the LDS-resident
  kernels, and both directions leave for attention_dh.hip together."""
  for (L, Dh, masked, cfg), (fkf, fwd, fam, bkf, bwd, _) in default_table.items():
    assert fkf == bkf and (fwd == "adh") == (fam == "adh") == (Dh != 64 or L > 576), (L, Dh, masked, cfg)
    if fam != "adh":
      assert fkf * 16 >= L and all(f"<{fkf}," in k for k in [fwd] + bwd.split("+")), (L, masked, cfg, fwd, bwd)


def test_instantiations_equal_the_bucket_table(default_table):
  """The rows of test_kernel_buckets_gpu.py::ATTN64 (both sides of every threshold) name what the route returns."""
  assert len(KB.ATTN64) >= 19
  for L, fwd, bwd, fwd_m, bwd_m in KB.ATTN64:
    got, got_m = default_table[L, 64, False, 0], default_table[L, 64, True, 0]
    assert (got[1], got[4], got_m[1], got_m[4]) == (fwd, bwd, fwd_m, bwd_m), L


def test_cfg_bits_equal_the_bucket_table(dump):
  """The rows of test_kernel_buckets_gpu.py::ATTN_CFG: each names the kernel its bit selects at that shape."""
  bits = sorted({bit for _, _, bit, _ in KB.ATTN_CFG})
  table = dump(576, *bits)
  for L, masked, bit, what in KB.ATTN_CFG:
    _, fwd, _, _, bwd, dpp = table[L, 64, masked, bit]
    what = what.split(":")[-1]                       # "no-attn5:dq1<..>+dkv<..>"
    for k in ("-unmasked", "-masked", "-classic"):
      what = what.replace(k, "")
    if bit == 256:
      assert dpp and what.endswith(",BM=1>") and bwd == what.replace(",BM=1>", ">"), (L, bit, bwd)
    elif what.startswith("fwd"):
      assert fwd == what, (L, bit, fwd)
    else:
      assert what == bwd or what in bwd.split("+"), (L, masked, bit, what, bwd)
    assert not dpp or bit == 256


def test_ops_entry_points_follow_the_route(default_table):
  """ops.py chooses between the Dh = 64 entry points and attention_dh.hip's with the route's condition."""
  from big_vision_amd import ops
  for (L, Dh, masked, cfg), (_, fwd, _, _, _, _) in default_table.items():
    if cfg == 0:
      want = "_dh" if fwd == "adh" else "_masked" if masked else ""
      assert ops._self_attn_entry(L, Dh, masked) == want, (L, Dh, masked)
