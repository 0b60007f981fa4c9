"""Proof that the memory-footprint harness (tests/_footprint.py) bites, in the spirit of test_tolerance_power_cpu.py:
torch "kernels" for a small pitched GEMM with a workspace and a row-wise normalisation over strided rows run on a CPU
arena.  The correct kernels pass; each of seven sabotaged kernels is flagged, and the message names the operand and the
byte offset where the kernel left its footprint."""
import re

import pytest
import torch

import _footprint as F

F32 = torch.float32
M, N, K, PAD = 5, 12, 8, 8
WS_BYTES = 4 * M * N                      # the "split-K workspace": one fp32 partial tile
ROWS, D, STRIDE, OFFSET = 3, 16, 4, 3     # normalise rows 3, 7, 11 of a [12][16] buffer


def gemm_ops():
  return [F.mat("A", F32, M, K, K + PAD), F.mat("B", F32, K, N, N + PAD), F.mat("C", F32, M, N, N + PAD, role="out"),
          F.Op("ws", torch.uint8, (WS_BYTES,), "scratch")]


def gemm(arena, sabotage=None):
  a, b, c = arena.view("A"), arena.view("B"), arena.view("C")
  ws = arena.view("ws").view(F32).view(M, N)
  ws.copy_(a @ b)                         # partial tile through the workspace, as the split-K kernels do
  rows = M - 1 if sabotage == "d" else M
  c[:rows] = ws[:rows]
  if sabotage == "a":                     # one element stored past the output's end
    flat, o0 = arena.around("C")
    flat[o0 + arena.ops["C"].alloc] = 1.0
  elif sabotage == "b":                   # one element stored into the pitch gap of row 0
    flat, o0 = arena.around("C")
    flat[o0 + N] = 1.0
  elif sabotage == "c":                   # one input element modified
    a.view(torch.int32)[2, 3] ^= 0x01010101
  elif sabotage == "f":                   # one guard element of B read and multiplied by zero into the result
    flat, o0 = arena.around("B")
    c[1, 2] += 0.0 * flat[o0 + arena.ops["B"].alloc + 5]
  elif sabotage == "g":                   # a workspace write one element past the declared size
    flat, o0 = arena.around("ws")
    flat[o0 + WS_BYTES:o0 + WS_BYTES + 4] = 0


def norm_ops():
  sel = dict(strides=(STRIDE * D, 1), offset=OFFSET * D, alloc=ROWS * STRIDE * D)
  return [F.Op("x", F32, (ROWS, D), "in", **sel), F.Op("y", F32, (ROWS, D), "out", **sel),
          F.Op("mean", F32, (ROWS,), "out")]


def norm(arena, sabotage=None):
  x = arena.view("x")
  mean = x.mean(-1)
  arena.view("mean").copy_(mean)
  arena.view("y").copy_((x - mean[:, None]) / x.std(-1, unbiased=False)[:, None])
  if sabotage == "e":                     # a skipped row of the strided output written
    flat, o0 = arena.around("y")
    flat[o0 + (OFFSET + 1) * D:o0 + (OFFSET + 2) * D] = 0.0


def test_correct_kernels_pass_and_return_their_operands():
  r = F.run("gemm", "ok", gemm_ops, gemm)
  ref = r["A"].double() @ r["B"].double()
  assert torch.allclose(r["C"].double(), ref, rtol=1e-5, atol=1e-5)
  assert r["C"].shape == (M, N) and r["A"].shape == (M, K)
  r = F.run("norm", "ok", norm_ops, norm)
  x = r["x"].double()
  assert torch.allclose(r["y"].double(), (x - x.mean(-1, keepdim=True)) / x.std(-1, unbiased=False, keepdim=True), atol=1e-5)
  assert torch.allclose(r["mean"].double(), x.mean(-1), atol=1e-6)
  # the arena is what the module says: 0xFF everywhere outside the extents, 256-byte-aligned operands, >= 64 KiB guards
  a = F.Arena(gemm_ops())
  assert bool((a.buf[a.filler_mask()] == 0xFF).all())
  assert torch.isnan(a.around("C")[0]).all()
  for o in a.ops.values():
    assert o.start % 256 == 0 and o.guard >= 64 << 10
  assert a.nbytes - (a.ops["ws"].start + WS_BYTES) >= 64 << 10


def test_guard_is_a_tile_row_block_when_that_is_larger():
  o = F.mat("A", torch.bfloat16, 4, 1024, 1032)
  assert o.guard == 256 * 1032 * 2


def test_seeded_inputs_repeat():
  assert torch.equal(F.Arena(gemm_ops(), seed=3).buf, F.Arena(gemm_ops(), seed=3).buf)
  assert not torch.equal(F.Arena(gemm_ops(), seed=3).buf, F.Arena(gemm_ops(), seed=4).buf)


LD = 4 * (N + PAD)
CASES = {
    "a": (gemm_ops, gemm, r"write outside the extent: operand 'C' \(guard band after\), byte offset (\d+), 4 byte"
          , ((M - 1) * (N + PAD) + N) * 4),
    "b": (gemm_ops, gemm, r"write outside the extent: operand 'C' \(pitch gap / unselected row\), byte offset (\d+), 4 byte",
          N * 4),
    "c": (gemm_ops, gemm, r"input modified: operand 'A' \(extent\), byte offset (\d+), 4 byte", (2 * (K + PAD) + 3) * 4),
    "d": (gemm_ops, gemm, r"not written: operand 'C' \(extent\), byte offset (\d+), 12 element", (M - 1) * LD),
    "e": (norm_ops, norm, r"write outside the extent: operand 'y' \(pitch gap / unselected row\), byte offset (\d+), 64 byte",
          (OFFSET + 1) * D * 4),
    "f": (gemm_ops, gemm, r"read outside the extent: operand 'B' \(guard band after\), byte offset (\d+), within 8 byte",
          ((K - 1) * (N + PAD) + N + 5) * 4 // 8 * 8),
    "g": (gemm_ops, gemm, r"write outside the extent: operand 'ws' \(guard band after\), byte offset (\d+), 4 byte", WS_BYTES),
}


@pytest.mark.parametrize("which", sorted(CASES))
def test_sabotaged_kernel_is_flagged_with_operand_and_offset(which):
  make_ops, kernel, pattern, offset = CASES[which]
  with pytest.raises(AssertionError) as e:
    F.run("kernel", which, make_ops, lambda a: kernel(a, which))
  text = str(e.value)
  m = re.search(pattern, text)
  assert m, text
  assert int(m.group(1)) == offset, text
  assert text.startswith(f"kernel[{which}]: ")
  if which == "f":     # ... and the element of C that took the guard value is named too
    assert re.search(r"output depends on bytes outside the input extents: operand 'C' \(extent\), byte offset "
                     + str((1 * (N + PAD) + 2) * 4) + ", 1 element", text), text
  # one finding, one cause: nothing else is reported
  assert len(text.splitlines()) == (2 if which == "f" else 1), text


def test_runs_of_one_buffer_are_one_operand():
  """An optimizer's leaves inside one parameter buffer: the extent is the union of the runs, a write between them is
  outside it and the value is their concatenation."""
  full = torch.arange(40, dtype=F32)
  ops = lambda: [F.Op("p", F32, role="inout", runs=[(4, 6), (20, 8)], alloc=40, fill=full)]

  def kernel(arena, bad=False):
    flat, o0 = arena.around("p")
    flat[o0 + 4:o0 + 10] += 1.0
    flat[o0 + 20:o0 + 28] += 1.0
    if bad:
      flat[o0 + 12] = 0.0

  r = F.run("opt", "ok", ops, kernel)
  assert torch.equal(r["p"], torch.cat([full[4:10], full[20:28]]) + 1.0)
  with pytest.raises(AssertionError, match=r"write outside the extent: operand 'p' \(pitch gap / unselected row\), byte offset 48, 4 byte"):
    F.run("opt", "bad", ops, lambda a: kernel(a, True))


def test_prepare_fills_address_tables_before_the_snapshot():
  ops = lambda: [F.Op("table", torch.int64, (2,), fill=torch.zeros(2)), F.Op("y", F32, (2,), "out")]

  def prepare(arena):
    arena.view("table").copy_(torch.tensor([arena.ptr("y"), 7]))

  r = F.run("k", "ok", ops, lambda a: a.view("y").fill_(1.0), prepare=prepare)
  assert int(r["table"][1]) == 7 and int(r["table"][0]) == r.arena.ptr("y")
  with pytest.raises(AssertionError, match="input modified: operand 'table'"):
    F.run("k", "bad", ops, lambda a: (a.view("y").fill_(1.0), a.view("table").add_(1)), prepare=prepare)


# ------------------------------------------------ the GPU table is complete ----
NOT_COMPUTE = {"bv_version", "bv_gemm_workspace_bytes"}   # host-side queries: no device operand


def test_every_compute_entry_point_has_a_footprint_row():
  """Reads the table of test_footprint_gpu.py and _lib.PROTOTYPES only: needs no GPU, so a new entry point without a
  footprint row fails the CPU suite."""
  from big_vision_amd import _lib
  import test_footprint_gpu as T
  want = {n for n in _lib.PROTOTYPES if not n.startswith(("bv_comm_", "bv_ctx_")) and n not in NOT_COMPUTE}
  have = {e for entries, _, _ in T.ROWS for e in entries}
  assert want <= have, f"entry points without a footprint row: {sorted(want - have)}"
  assert have <= want, f"rows for unknown entry points: {sorted(have - want)}"
  ids = [f"{e[0]}-{c}" for e, c, _ in T.ROWS]
  assert len(set(ids)) == len(ids), "duplicate row ids"
