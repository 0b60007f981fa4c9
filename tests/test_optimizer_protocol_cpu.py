"""The protocol of one optimizer step, per update rule and placement: WHICH kernels and collectives `Optimizer.step()`
issues and in WHAT ORDER.  Dry run on the CPU: every libbvhip entry point and every collective is replaced by a recorder
that keeps order (no arithmetic), "rank 1 of 2" without a process group.  The table was recorded from the three
separate step bodies (replicated chain, sharded chain, Adafactor) the optimizer had before they became one `step()`: it
is that step's contract for every rule and placement."""
import pytest

from big_vision_amd import _lib, dp, ops
from big_vision_amd import optax as bv_optax
from big_vision_amd.compat.ml_collections import ConfigDict
from big_vision_amd.models.proj.image_text import two_towers

IMG = dict(width=128, depth=2, mlp_dim=256, num_heads=2, patch_size=(16, 16), pool_type="map")
TXT = dict(width=128, depth=2, mlp_dim=256, num_heads=2, vocab_size=50)
SCHED_KW = dict(total_steps=10, batch_size=8, data_size=100)

RULES = {"adam": ("scale_by_adam", None),
         "momentum_hp": ("big_vision.momentum_hp", None),
         "sgd": ("big_vision.sgd", None),
         "adafactor": ("big_vision.scale_by_adafactor", dict(momentum=0.9))}
PLACEMENTS = ("replicated", "fsdp", "fsdp_master_replicated")


class _RecordingComm(dp.Comm):
  """Rank 1 of 2 without a process group: every collective is recorded by its method name, data stays where it is."""

  def __init__(self, log):
    self.enabled, self.group, self.rank, self.size, self.log, self.active = False, None, 1, 2, log, True

  def all_gather_flat_(self, flat, lo, hi, S):
    self.log.append("all_gather_flat_")

  def broadcast_ranges_(self, flat, bounds):
    self.log.append("broadcast_ranges_")

  def all_reduce_sum_(self, flat, bucket_bytes=0):
    self.log.append("all_reduce_sum_")

  def all_reduce_scalars_(self, t):
    self.log.append("all_reduce_scalars_")


@pytest.fixture()
def log(monkeypatch):
  """The ordered record: kernel names (`_lib.call`), collective method names, "reduce" for every range the fallback of
  step() sums onto its owner (dp.GradShardSync issues those through torch.distributed directly)."""
  out = []
  monkeypatch.setattr(_lib, "call", lambda name, *a: out.append(name))
  monkeypatch.setattr(ops, "_chk", lambda t, dtype, name: t)
  monkeypatch.setattr(ops, "_stream", lambda: 0)
  monkeypatch.setattr(dp.dist, "reduce", lambda t, dst, group=None: out.append("reduce"))
  return out


def _optimizer(log, rule, placement, frozen_prefix=None):
  model = two_towers.Model(image=IMG, text=TXT, out_dim=(None, 32), temperature_init=10.0, bias_init=-10.0)
  frozen = [n for n in model.leaf_names((2, 32, 32, 3), (2, 8)) if frozen_prefix and n.startswith(frozen_prefix)]
  store = model.make_store((2, 32, 32, 3), (2, 8), device="cpu", frozen_leaves=frozen)
  store.init_random(0)
  store.ensure_grad()
  name, okw = RULES[rule]
  schedule = dict(decay_type="cosine", warmup_steps=2)
  if frozen_prefix:
    schedule = [(frozen_prefix + ".*", None), (".*", schedule)]
  cfg = ConfigDict(dict(lr=1e-3, wd=1e-2, optax_name=name, grad_clip_norm=1.0, schedule=schedule))
  if okw is not None:
    cfg.optax = okw
  if placement == "fsdp_master_replicated":
    cfg.fsdp_shard_params = False
  sharded = placement != "replicated"
  opt, _ = bv_optax.make(cfg, store, sched_kw=SCHED_KW, comm=_RecordingComm(log) if sharded else None, shard=sharded)
  assert store.master_sharded == (placement == "fsdp")
  return opt


def _two_steps(log, opt):
  """Step 1 on gradients stamped as reduced, step 2 without a new stamp."""
  out = []
  opt.mark_grads_reduced()
  for _ in range(2):
    log.clear()
    meas = opt.step()
    assert set(meas) == {"l2_grads", "l2_params", "l2_updates"}
    out.append(list(log))
  assert opt.count == 2
  return out


# (rule, placement) -> [step 1, step 2].  Step 1 runs on gradients stamped as reduced; nobody stamps step 2, so under "fsdp"
# both owners' ranges are summed first ("reduce" twice).  Then: the clip norm over the own range and its all-reduce, the
# rule's kernels (Adafactor: one call per size class of its leaf table - six for the whole toy model, five for the second
# rank's run of tensors), the all-reduce of the norm statistics, and the parameter exchange: the bf16 shadow (all-gather of
# equal slices for the chain, one broadcast per owner for Adafactor's unequal runs) followed by the all-reduce of the small
# replicated entries - or, with a replicated fp32 master, its broadcast and the bf16 cast of the one non-empty foreign range.
AF = "bv_adafactor_step"
PROTOCOL = {
    ("adam", "replicated"): [
        ["bv_sqnorm", "bv_adam_step"],
        ["bv_sqnorm", "bv_adam_step"]],
    ("adam", "fsdp"): [
        ["bv_sqnorm", "all_reduce_scalars_", "bv_adam_step", "all_reduce_scalars_", "all_gather_flat_", "all_reduce_sum_"],
        ["reduce", "reduce", "bv_sqnorm", "all_reduce_scalars_", "bv_adam_step", "all_reduce_scalars_", "all_gather_flat_",
         "all_reduce_sum_"]],
    ("adam", "fsdp_master_replicated"): [
        ["bv_sqnorm", "all_reduce_scalars_", "bv_adam_step", "all_reduce_scalars_", "broadcast_ranges_", "bv_cast_bf16"],
        ["reduce", "reduce", "bv_sqnorm", "all_reduce_scalars_", "bv_adam_step", "all_reduce_scalars_", "broadcast_ranges_",
         "bv_cast_bf16"]],
    ("momentum_hp", "replicated"): [
        ["bv_sqnorm", "bv_trace_step"],
        ["bv_sqnorm", "bv_trace_step"]],
    ("momentum_hp", "fsdp"): [
        ["bv_sqnorm", "all_reduce_scalars_", "bv_trace_step", "all_reduce_scalars_", "all_gather_flat_", "all_reduce_sum_"],
        ["reduce", "reduce", "bv_sqnorm", "all_reduce_scalars_", "bv_trace_step", "all_reduce_scalars_", "all_gather_flat_",
         "all_reduce_sum_"]],
    ("momentum_hp", "fsdp_master_replicated"): [
        ["bv_sqnorm", "all_reduce_scalars_", "bv_trace_step", "all_reduce_scalars_", "broadcast_ranges_", "bv_cast_bf16"],
        ["reduce", "reduce", "bv_sqnorm", "all_reduce_scalars_", "bv_trace_step", "all_reduce_scalars_", "broadcast_ranges_",
         "bv_cast_bf16"]],
    ("sgd", "replicated"): [
        ["bv_sqnorm", "bv_trace_step"],
        ["bv_sqnorm", "bv_trace_step"]],
    ("sgd", "fsdp"): [
        ["bv_sqnorm", "all_reduce_scalars_", "bv_trace_step", "all_reduce_scalars_", "all_gather_flat_", "all_reduce_sum_"],
        ["reduce", "reduce", "bv_sqnorm", "all_reduce_scalars_", "bv_trace_step", "all_reduce_scalars_", "all_gather_flat_",
         "all_reduce_sum_"]],
    ("sgd", "fsdp_master_replicated"): [
        ["bv_sqnorm", "all_reduce_scalars_", "bv_trace_step", "all_reduce_scalars_", "broadcast_ranges_", "bv_cast_bf16"],
        ["reduce", "reduce", "bv_sqnorm", "all_reduce_scalars_", "bv_trace_step", "all_reduce_scalars_", "broadcast_ranges_",
         "bv_cast_bf16"]],
    ("adafactor", "replicated"): [
        ["bv_sqnorm", AF, AF, AF, AF, AF, AF],
        ["bv_sqnorm", AF, AF, AF, AF, AF, AF]],
    ("adafactor", "fsdp"): [
        ["bv_sqnorm", "all_reduce_scalars_", AF, AF, AF, AF, AF, "all_reduce_scalars_", "broadcast_ranges_", "all_reduce_sum_"],
        ["reduce", "reduce", "bv_sqnorm", "all_reduce_scalars_", AF, AF, AF, AF, AF, "all_reduce_scalars_", "broadcast_ranges_",
         "all_reduce_sum_"]],
    ("adafactor", "fsdp_master_replicated"): [
        ["bv_sqnorm", "all_reduce_scalars_", AF, AF, AF, AF, AF, "all_reduce_scalars_", "broadcast_ranges_", "bv_cast_bf16"],
        ["reduce", "reduce", "bv_sqnorm", "all_reduce_scalars_", AF, AF, AF, AF, AF, "all_reduce_scalars_", "broadcast_ranges_",
         "bv_cast_bf16"]],
}


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("rule", sorted(RULES))
def test_step_issues_the_recorded_kernels_and_collectives_in_order(log, rule, placement):
  opt = _optimizer(log, rule, placement)
  assert _two_steps(log, opt) == PROTOCOL[(rule, placement)]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("rule", sorted(RULES))
def test_a_second_step_without_a_new_stamp_reduces_again(log, rule, placement):
  """The stamp of mark_grads_reduced() / grad_sync().finish() is good for ONE step."""
  opt = _optimizer(log, rule, placement)
  first, second = _two_steps(log, opt)
  assert "reduce" not in first
  assert second == (["reduce", "reduce"] if opt.sharded else []) + first
  opt.mark_grads_reduced()
  log.clear()
  opt.step()
  assert log == first


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("rule", ["adam", "adafactor"])
def test_frozen_tensors_add_one_norm_launch_to_the_first_step_only(log, rule, placement):
  """l2_params covers the frozen tensors: their square norm is taken once, lazily, when the first step builds its
  measurements (after everything else), and kept."""
  opt = _optimizer(log, rule, placement, frozen_prefix="img/")
  first, second = _two_steps(log, opt)
  kernel = {"adam": ["bv_adam_step"], "adafactor": [AF] * 5}[rule]     # (the text tower alone: five size classes)
  step = {"replicated": ["bv_sqnorm"] + kernel,
          "fsdp": ["bv_sqnorm", "all_reduce_scalars_"] + kernel + ["all_reduce_scalars_"]
                  + [{"adam": "all_gather_flat_", "adafactor": "broadcast_ranges_"}[rule], "all_reduce_sum_"],
          "fsdp_master_replicated": ["bv_sqnorm", "all_reduce_scalars_"] + kernel
                                    + ["all_reduce_scalars_", "broadcast_ranges_", "bv_cast_bf16"]}[placement]
  assert first == step + ["bv_sqnorm"]
  assert second == (["reduce", "reduce"] if opt.sharded else []) + step
