"""The bf16 GEMM dispatch has one owner, big_vision_amd/csrc/gemm_route.h, and what the tests believe about it is held
to it here: the header is compiled into a host program (tests/gemm_route_dump.cpp: the system C++ compiler, no HIP, no
GPU) whose answers are compared with a restatement of include/bvhip.h's fast-path rule, with the instantiations of
tests/kernel_coverage.json, with bv_gemm_workspace_bytes of the built library, and with the dispatch that
test_footprint_gpu.py and test_kernel_buckets_gpu.py assume for their rows."""
import collections
import itertools
import json
import os
import shutil
import subprocess

import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
# BV_EPI_* (include/bvhip.h; test_epilogue_and_option_codes_match_the_header holds big_vision_amd._lib to the header)
E = dict(NONE=0, RESIDUAL=1, POS=2, GELU=3, GELU_BWD=4, ATOMIC=5, GELU_BWD_EMIT=6, GELU_GD=7, MUL=8, GELU_G=9)
FAMILIES = ("gemm_bf16_kernel", "gemm256_kernel", "gemm256r_kernel")   # GEMM_128, GEMM_256, GEMM_256R
A, B_, C, AUX, BIAS, C2 = 1, 2, 4, 8, 16, 32                           # bvgemm::GemmOperand

Call = collections.namedtuple("Call", "akm bkm M N K lda ldb ldc ldaux mis has_aux has_bias has_colsum epi f32 alpha1 split_k")
Opts = collections.namedtuple("Opts", "fast_path roll reserve skew_pct skew_mode group_n nt pre_issue ws_bytes has_ws")
Route = collections.namedtuple("Route", "family kernel splits ktiles_per_split k_chunk gx gy gz block use_slab slab_bytes "
                                        "skew_cycles skew_mode group_n multi fused")
DEFAULTS = Opts(1, 1, 0, 0, 1, 0, 0, 0, 0, 0)   # include/bvhip.h, no workspace
NEEDS_AUX = {E[k] for k in ("RESIDUAL", "POS", "GELU_BWD", "GELU_BWD_EMIT", "MUL")}


def call(akm, bkm, M, N, K, epi, f32, bias, *, pad=0, ldc=None, mis=0, colsum=0, alpha1=1, split_k=0, **ld):
  """A call with dense operands (+ pad elements per row); ld: lda / ldb / ldaux overrides."""
  aux = epi in NEEDS_AUX
  c = Call(akm, bkm, M, N, K, (K if akm else M) + pad, (K if bkm else N) + pad, (N + pad) if ldc is None else ldc,
           (N + pad) if aux else 0, mis, int(aux), int(bias), colsum, epi, f32, alpha1, split_k)
  return c._replace(**ld)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
  assert CXX, "no host C++ compiler"
  exe = str(tmp_path_factory.mktemp("route") / "gemm_route_dump")
  subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "gemm_route_dump.cpp"), "-o", exe],
                 check=True)

  def run(mode, cases=()):
    """cases: (Call, Opts) pairs.  routes -> one Route per case; kernels -> the set of instantiations; defaults -> Opts."""
    if mode == "defaults":
      return Opts(*map(int, subprocess.run([exe, mode], check=True, capture_output=True, text=True).stdout.split()))
    text = "".join(" ".join(map(str, c + o)) + "\n" for c, o in cases)
    out = subprocess.run([exe, mode], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    if mode == "kernels":
      return set(out)
    assert len(out) == len(cases)
    return [Route(*(x if i == 1 else int(x) for i, x in enumerate(line.split("\t")))) for line in out]
  return run


def grid():
  """M, N in {8, 248, 256, 264, 512, 768} x K in {8, 56, 64, 72, 128, 1024} x the four layouts x every epilogue x
  out_f32 x bias, dense and aligned; then one misaligned case each for lda, ldb, ldc, ldaux and each pointer, on calls
  that qualify otherwise."""
  dims, ks = (8, 248, 256, 264, 512, 768), (8, 56, 64, 72, 128, 1024)
  cases = [call(akm, bkm, M, N, K, epi, f32, bias)
           for M, N, K in itertools.product(dims, dims, ks) for akm in (0, 1) for bkm in (0, 1)
           for epi in range(10) for f32 in (0, 1) for bias in (0, 1)]
  res = call(1, 1, 512, 768, 128, E["RESIDUAL"], 1, 1)   # has every operand: aux, bias; C2 with GELU below
  gelu = call(1, 1, 512, 768, 128, E["GELU"], 0, 1)
  dw = call(0, 0, 512, 768, 128, E["ATOMIC"], 1, 0)
  for base in (res, dw):
    cases += [base._replace(lda=base.lda + 4), base._replace(ldb=base.ldb + 4), base._replace(ldc=base.ldc + 4),
              base._replace(mis=A), base._replace(mis=B_), base._replace(mis=C)]
  cases += [res._replace(ldaux=res.ldaux + 4), res._replace(mis=AUX), res._replace(mis=BIAS), gelu._replace(mis=C2),
            gelu._replace(mis=BIAS), gelu._replace(ldaux=4)]   # the last one has no aux: its pitch is not looked at
  return cases


def edge_calls(M, N, K):
  """The launches of test_kernel_buckets_gpu.py::test_gemm_fast_path_edges: k-major fp32 / bf16 with a bias, and dW."""
  return [call(1, 1, M, N, K, E["NONE"], 1, 1), call(1, 1, M, N, K, E["NONE"], 0, 1), call(0, 0, M, N, K, E["ATOMIC"], 1, 0)]


def takes_256(c):
  """include/bvhip.h, BV_OPT_FAST_PATH: the 256 x 256 x 64 kernels serve M, N % 256 == 0, K % 64 == 0, one layout for both
  operands, 16-byte operand chunks, and the epilogues of the layout."""
  shape = c.akm == c.bkm and c.M % 256 == 0 and c.N % 256 == 0 and c.K % 64 == 0
  epi = c.epi != E["ATOMIC"] if c.akm else c.epi == E["ATOMIC"] or (c.epi == E["NONE"] and c.f32 and not c.has_bias)
  ld = c.lda % 8 == 0 and c.ldb % 8 == 0 and c.ldc % 8 == 0 and (not c.has_aux or c.ldaux % 8 == 0)
  return bool(shape and epi and ld and c.mis == 0)


def edges():
  """EDGES of test_kernel_buckets_gpu.py; the GPU test modules are imported where their tables are read, so a fault
  in one of them fails the tests that mirror it and not this file's collection."""
  import test_kernel_buckets_gpu as KB
  return KB.EDGES


def test_qualification_equals_the_header_rule(dump):
  cases = grid() + [c for M, N, K, _ in edges() for c in edge_calls(M, N, K)]
  routes = dump("routes", [(c, DEFAULTS) for c in cases])
  bad = [(c, r.kernel) for c, r in zip(cases, routes) if (r.family != 0) != takes_256(c)]
  assert not bad, bad[:10]
  assert sum(r.family != 0 for r in routes) > 1000 and sum(r.family == 0 for r in routes) > 1000
  for c, r in zip(cases, routes):
    assert FAMILIES[r.family] == r.kernel.split("<")[0]
  off = dump("routes", [(c, DEFAULTS._replace(fast_path=0)) for c in cases[::97]])
  assert all(r.family == 0 for r in off), "fast_path = 0 sends everything to the general kernel"
  assert routes[len(grid()) - 1].family != 0, "the pitch of an absent aux disqualifies nothing"


def test_edge_table_states_the_route(dump):
  """Every row of test_kernel_buckets_gpu.py::EDGES: its `fast` column is the rule's answer, and the route's, for the
  k-major calls and the dW call that test issues."""
  assert len(edges()) >= 7
  for M, N, K, fast in edges():
    calls = edge_calls(M, N, K)
    for c, r in zip(calls, dump("routes", [(c, DEFAULTS) for c in calls])):
      assert takes_256(c) == fast and (r.family != 0) == fast, (M, N, K, c, r)


def test_routes_reach_exactly_the_compiled_instantiations(dump):
  """Over the grid x BV_OPT_GEMM_ROLL 0..15 x column sums x alpha 1 / 0.5: the instantiations the route names are the
  gemm_bf16_kernel / gemm256_kernel / gemm256r_kernel entries of tests/kernel_coverage.json, no more and no fewer."""
  filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
  cov = json.load(open(os.path.join(ROOT, "tests", "kernel_coverage.json")))["kernels"]
  mangled = [k for k in cov if any(f"{len(f)}{f}I" in k for f in FAMILIES)]
  names = subprocess.run([filt], input="\n".join(mangled), check=True, capture_output=True, text=True).stdout.splitlines()
  compiled = set()
  for n in names:   # "void (anonymous namespace)::gemm256_kernel<true, 0, 3, false>((anonymous namespace)::G256Params)"
    head = "void (anonymous namespace)::"
    assert n.startswith(head) and ">(" in n, n
    compiled.add(n[len(head):n.index(">(") + 1])
  assert len(compiled) == len(mangled) == 21   # the enumerators of bvgemm::GemmKernel
  reached = dump("kernels", [(c, DEFAULTS) for c in grid()])
  assert reached == compiled, (sorted(reached - compiled), sorted(compiled - reached))


@pytest.fixture(scope="module")
def lib():
  from big_vision_amd import build, _lib
  build.build(verbose=False)
  return _lib.load()


def test_workspace_bytes_is_the_route(dump, lib):
  """bv_gemm_workspace_bytes = the dW route's slab_bytes: exact at gemm_reserve_cus = 0, an upper bound at every other
  value, and what the library answered before the route existed (tests/golden/gemm_workspace_bytes.json)."""
  gold = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_workspace_bytes.json")))
  assert gold["m"] == gold["n"] == list(range(1, 13)) and gold["k"] == [1, 2, 7, 8, 16, 17, 48, 196]
  shapes = [(256 * m, 256 * n, 64 * k) for m in gold["m"] for n in gold["n"] for k in gold["k"]]
  want = [b for plane in gold["bytes"] for row in plane for b in row]
  got = [lib.bv_gemm_workspace_bytes(*s) for s in shapes]
  assert got == want and sum(b > 0 for b in got) > 500
  unlimited = DEFAULTS._replace(ws_bytes=2 ** 62, has_ws=1)
  for reserve in (0, 1, 4, 64, 128):
    o = unlimited._replace(reserve=reserve)
    routes = dump("routes", [(call(0, 0, *s, E["ATOMIC"], 1, 0), o) for s in shapes])
    for s, r, b in zip(shapes, routes, got):
      assert r.family == 1 and r.use_slab == (r.slab_bytes > 0) and r.slab_bytes == r.splits * (r.splits > 1) * s[0] * s[1] * 4
      assert r.slab_bytes == b if reserve == 0 else r.slab_bytes <= b, (s, reserve, r.slab_bytes, b)
  assert lib.bv_gemm_workspace_bytes(512, 760, 1024) == 0 and lib.bv_gemm_workspace_bytes(512, 768, 1000) == 0
  assert lib.bv_gemm_workspace_bytes(0, 256, 1024) == 0


def test_footprint_rows_state_the_route(dump, lib):
  """Every GEMM row of test_footprint_gpu.py: its stat = (CALLS, MULTI, FUSED) increments are what the route says for
  the row's shape, pitches (+ 8 elements), options and workspace mode, and an ATOMIC row's split count is the one its
  rounding-error bound assumes."""
  from big_vision_amd._lib import OPTS
  import test_footprint_gpu as FP
  assert FP.E == E
  rows = {k: v for k, v in FP.ARGS.items() if v[0] is FP.gemm_row}
  assert len(rows) >= 45
  cases, want = [], []
  for name, (_, (_, M, N, K, akm, bkm, f32, *epi), kw) in rows.items():
    epi = epi[0] if epi else "NONE"
    wsb = lib.bv_gemm_workspace_bytes(M, N, K) if kw.get("ws") == "exact" else 0
    o = DEFAULTS._replace(ws_bytes=wsb, has_ws=int(wsb > 0))
    for k, v in (kw.get("opts") or {}).items():
      assert k.startswith("gemm_") and k in OPTS
      o = o._replace(**{k[5:].replace("reserve_cus", "reserve"): v})
    c = call(akm, bkm, M, N, K, E[epi], f32, kw.get("bias", True), pad=FP.PAD, colsum=int(kw.get("colsum", False)),
             split_k=kw.get("split_k", 0))
    cases.append((c, o))
    want.append((name, epi, kw))
  for (name, epi, kw), (c, o), r in zip(want, cases, dump("routes", cases)):
    stat = kw.get("stat", (0, 0, 0))
    assert (int(r.family != 0), r.multi, r.fused) == stat, (name, r)
    if epi == "ATOMIC":
      assert r.splits == (kw.get("split_k", 0) or (2 if stat[0] else 1)), (name, r)
      # "exact" sizes the workspace for the automatic choice (2 splits): the explicit split_k = 3 row asks for three
      # partial tiles, does not fit, and combines with atomics
      assert r.use_slab == (kw.get("ws") == "exact" and not kw.get("split_k")), (name, r)
    if name.startswith("g256-roll"):
      assert r.family == 2 and r.kernel.endswith(", 1>") == bool(o.roll & 8), (name, r)


def test_defaults_are_the_context_defaults(dump, lib):
  """gemm_default_opts() (what bv_gemm_workspace_bytes routes under), this file's DEFAULTS and a context nobody has set
  (c_api.cpp) state the same option values."""
  from big_vision_amd._lib import OPTS
  d = dump("defaults")
  assert d == DEFAULTS
  names = dict(fast_path="fast_path", roll="gemm_roll", reserve="gemm_reserve_cus", skew_pct="gemm_skew_pct", skew_mode="gemm_skew_mode",
               group_n="gemm_group_n", nt="gemm_nt", pre_issue="gemm_pre_issue")
  ctx = lib.bv_ctx_create()
  try:
    for field, opt in names.items():
      assert getattr(d, field) == lib.bv_ctx_get(ctx, OPTS[opt]) == lib.bv_ctx_get(None, OPTS[opt]), field
  finally:
    lib.bv_ctx_destroy(ctx)
  assert set(names) | {"ws_bytes", "has_ws"} == set(Opts._fields)


def test_grid_skew_and_tile_order_of_the_256_families(dump):
  """The persistent grid is min(work items, 256 - reserved CUs) x 512 threads; the start skew is set only for a k-major
  launch with skew_pct > 0 whose work items exceed the 256 CUs, as pct % of (3600 cycles per K-tile + 12000), and the
  skew mode travels only with it; group_n reaches the k-major kernels and is 0 for the k-minor one; nt / pre_issue do
  not move the route."""
  o = DEFAULTS._replace(skew_pct=25, skew_mode=0, group_n=3, nt=3, pre_issue=2)
  km = lambda M, N, K: call(1, 1, M, N, K, E["NONE"], 0, 1)
  dw = lambda M, N, K: call(0, 0, M, N, K, E["ATOMIC"], 1, 0)
  cases = [(km(512, 512, 128), o), (km(4096, 4096, 128), o), (km(4096, 4352, 128), o), (km(4096, 4352, 1024), o._replace(skew_mode=1)),
           (km(4096, 4352, 128), o._replace(skew_pct=0)), (km(4096, 4352, 128), o._replace(reserve=4)),
           (km(4096, 4096, 128), o._replace(reserve=4)), (dw(4096, 4352, 1024), o), (dw(2816, 3072, 1024), o._replace(reserve=128))]
  want = [  # grid.x, skew_cycles, skew_mode, group_n, multi
      (4, 0, 0, 3, 0), (256, 0, 0, 3, 0), (256, (2 * 3600 + 12000) * 25 // 100, 0, 3, 1), (256, (16 * 3600 + 12000) * 25 // 100, 1, 3, 1),
      (256, 0, 0, 3, 1), (252, (2 * 3600 + 12000) * 25 // 100, 0, 3, 1), (252, 0, 0, 3, 1), (256, 0, 0, 0, 1), (128, 0, 0, 0, 1)]
  routes = dump("routes", cases)
  for (c, oo), r, w in zip(cases, routes, want):
    assert (r.gx, r.skew_cycles, r.skew_mode, r.group_n, r.multi) == w and (r.gy, r.gz, r.block) == (1, 1, 512), (c, oo, r)
    assert r.family != 0 and not r.fused
  plain = dump("routes", [(c, oo._replace(nt=0, pre_issue=0)) for c, oo in cases])
  assert plain == routes
  assert routes[-1].splits == routes[-2].splits == 1   # more tiles than CUs in use: no split


def test_general_path_splits(dump):
  """GEMM_128, EPI_ATOMIC: grid.z and k_chunk from the rule of gemm_route.h's general branch, restated: the automatic
  choice aims at >= 1024 workgroups with >= 8 K-steps of 64 per split, an explicit one is clamped to the K-steps, and
  the chunk is rounded up to whole K-steps so that no split is empty."""
  for (M, N, K), split_k in itertools.product(((64, 72, 333), (136, 136, 72)), (0, 3, 100)):
    tiles, ksteps = -(-M // 128) * -(-N // 128), -(-K // 64)
    splits = split_k or min(-(-1024 // tiles), max(ksteps // 8, 1))
    splits = min(max(splits, 1), ksteps)
    k_chunk = -(-ksteps // splits) * 64
    r, = dump("routes", [(call(0, 0, M, N, K, E["ATOMIC"], 1, 0, split_k=split_k), DEFAULTS)])
    assert r.family == 0 and r.kernel == "gemm_bf16_kernel<false, false>"
    assert (r.gx, r.gy, r.gz, r.block) == (-(-N // 128), -(-M // 128), -(-K // k_chunk), 256) and r.k_chunk == k_chunk, (M, N, K, split_k, r)
    assert r.splits == r.gz and not r.use_slab and r.slab_bytes == 0
