"""The optimizer kernels - bv_adam_step, bv_trace_step, bv_adafactor_leaf, bv_adafactor_step, bv_sqnorm - through
ops.*_ directly (no model, no trainer), held per element to the fp64 models of the documented arithmetic in
tests/_bounds.py (adam_bounds, trace_bounds, adafactor_bounds, sqnorm_bound, clip_factor).  The cases live in
tests/_opt_cases.py as drivers over a set of step functions: here they run ops itself; tests/test_tolerance_power_cpu.py
runs the same drivers on an fp32 emulation of the kernels and proves the checker calls reject a catalogue of slips.

Every case runs two consecutive steps, the reference of each step starting from the state the kernel stored before it
(step 2 therefore starts from the kernel's own non-zero state); parameters mix p = 0, |p| ~ 1e-4, |p| ~ 1 and a few
|p| ~ 30, gradients are 1e-3-scale with exact zeros and 1e-12 elements (_bounds.opt_inputs).  Beside the elementwise
bounds: the bf16 shadow is rne(p') bit for bit, parameters under a schedule value of 0 do not move, elements outside a
strided Adafactor view are untouched, the batched Adafactor step equals the per-leaf entry bit for bit.

Max err / bound per output family.  Every check prints its own "[bounds] <case> <operand>: max err/bound" line and every
test one "[bounds] <family>: ..." line under pytest -s.  MI355X figures: not measured (no GPU was available; the file
has run only through its CPU twin).  fp32 emulation of the documented arithmetic on the same inputs
(tests/test_tolerance_power_cpu.py): adam p 0.99, mu 1.00 (a bf16 tie), nu < 1, stats 0.10; trace 1.00 (bf16 tie), p
0.98; adafactor v_row 0.91, v_col 0.98, rcm 0.05, v 0.92, mom 1.00 (bf16 tie), p 0.99, usq 0.05, stats 0.06; sqnorm
< 0.01.  A ratio above 1 on the GPU is a failure to explain from the kernel source, never a number to absorb.
"""
import pytest
import torch

import _bounds as B
import _opt_cases as OC

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _ops():
  from big_vision_amd import ops
  return ops


def _report(family, worst):
  print(f"[bounds] {family}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
  assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("mu", [F32, BF16], ids=["mu-f32", "mu-bf16"])
@pytest.mark.parametrize("clip", [0.0, 1e-2], ids=["noclip", "clip"])
@pytest.mark.parametrize("nchunks,nseg", [(1, 1), (3, 3), (4099, 2)], ids=["1chunk", "3seg", "gridstride"])
def test_adam_step(dev, nchunks, nseg, clip, mu):
  """count = 1024; 3 x 1024 with three segments (lr_eff = 0 & wd_eff > 0 at sched_idx BV_MAX_SCHED - 1, a segment whose
  schedule value is 0); 4099 x 1024 (past the 4096-workgroup grid cap: the grid-stride loop) with two segments
  alternating per chunk, the model evaluated in blocks of 2^20 elements."""
  _report("adam", OC.chain_case(_ops(), dev, "adam", nchunks, nseg, clip, mu))


@pytest.mark.parametrize("kind,nesterov,dt", [("trace", False, BF16), ("trace", False, F32), ("trace", True, BF16),
                                              ("trace", True, F32), ("identity", False, None)],
                         ids=["bf16", "f32", "nesterov-bf16", "nesterov-f32", "identity"])
def test_trace_step(dev, kind, nesterov, dt):
  _report("trace", OC.chain_case(_ops(), dev, kind, 2, 2, 1e-2, dt, nesterov=nesterov))


@pytest.mark.parametrize("which", ["zero", "at", "ulp-above", "far"])
def test_clip_threshold(dev, which):
  """gsq = 0; float32(sqrt(gsq)) == clip_norm exactly (the no-clip side); one fp32 ulp above it; gn = 1e3 clip_norm -
  through the Adam, trace and Adafactor entries (the clip factor is shared by all three)."""
  gsq = OC.clip_gsq(which, 0.5)
  c, e = B.clip_factor(gsq, 0.5)
  assert (c == 1.0 and e == 0.0) == (which in ("zero", "at")), (which, c)
  for kind in ("adam", "trace"):
    _report(f"clip {kind}", OC.chain_case(_ops(), dev, kind, 1, 1, 0.5, F32, gsq_value=gsq))
  _report("clip adafactor", OC.af_leaf_case(_ops(), dev, B.AF_SPECS[0], BF16, 0.5, gsq_value=gsq))


@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, 1024 * 257 + 3, 2048 * 256 * 4 + 4 * 256 + 1])
def test_sqnorm(dev, count):
  """The scalar tail (count % 4 != 0), count < 4, several workgroups, the grid-stride range (count / 4 > 2048 x 256)."""
  _report("sqnorm", OC.sqnorm_case(_ops(), dev, count))


def test_sqnorm_of_a_view_16_bytes_into_a_buffer(dev):
  _report("sqnorm", OC.sqnorm_case(_ops(), dev, 1023, offset=4))


@pytest.mark.parametrize("mom", [BF16, F32], ids=["mom-bf16", "mom-f32"])
@pytest.mark.parametrize("spec", B.AF_SPECS, ids=[s[0] for s in B.AF_SPECS])
def test_adafactor_leaf(dev, spec, mom):
  """bv_adafactor_leaf on every leaf of _bounds.AF_SPECS: R = 32 (the factoring threshold) in both orders, C below and
  just above a workgroup, r_fast with R != C, the query / key slices of a fused [128][3][2][64] tensor, two non-trivial
  batch axes in a padded buffer (four distinct strides, gaps untouched), unfactored leaves of 1, 100, 257 elements,
  [31][500] and [2][3][5][7], a zero gradient row / column and an all-zero gradient (state becomes eps-only, update
  and momentum finite)."""
  _report("adafactor leaf", OC.af_leaf_case(_ops(), dev, spec, mom, 1e-2))


@pytest.mark.parametrize("mom", [BF16, F32], ids=["mom-bf16", "mom-f32"])
@pytest.mark.parametrize("single", [False, True], ids=["classes", "one-class"])
@pytest.mark.parametrize("brc", [0.0, 0.7, 1e6])
def test_adafactor_batched_step(dev, brc, single, mom):
  """One table of all the leaves through bv_adafactor_step, cut into size classes by optax.af_table or run as a single
  class sized by the largest leaf (the 1-element leaf shares a launch with the 300 x 64 one), two schedule indices,
  block_rms_clip off / 0.7 / 1e6 (never clips: scale exactly 1, results bit-equal to the per-leaf entry)."""
  _report("adafactor batched", OC.af_batched_case(_ops(), dev, mom, brc, single))
