"""The cases of tests/test_optimizer_kernels_gpu.py as drivers over a set of step functions `fns` with the signatures
of big_vision_amd.ops (adam_step_, trace_step_, adafactor_leaf_, adafactor_step_, sqnorm_): the GPU file passes ops
itself, tests/test_tolerance_power_cpu.py passes its fp32 emulations of the kernels' operation sequences - so the
models of _bounds.py are proved on the CPU against the very inputs, steps and checker calls the GPU runs.

Every case runs two consecutive steps; the reference of each step starts from the state the step function stored
before it (the kernel is held per step, no fp64-versus-bf16 drift enters); the first step already starts from
non-zero state (except the zero-gradient Adafactor leaves, whose state must become eps-only).  Each driver returns
{operand: worst max err / bound over its steps}."""
import ctypes
import math

import numpy as np
import torch

import _bounds as B

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SEG = np.dtype([("lr", np.float32), ("wd", np.float32), ("si", np.int32), ("pad", np.int32)])   # struct bv_adam_seg
MAX_SCHED = 8                                                                                   # BV_MAX_SCHED
SCHED = [[0.3, 1.0, 0.55, 0.0, 0.8, 0.25, 0.9, 0.7], [0.35, 0.95, 0.5, 0.0, 0.75, 0.2, 0.85, 0.65]]   # per step
ADAM = dict(b1=0.9, b2=0.999, eps=1e-8)
STEPS = (3, 4)          # the optimizer's step counter at the two steps (bias corrections 1 - b^(k + 1))
# segment tables: 1 segment; 2 alternating per chunk; 3 with lr_eff = 0 & wd_eff > 0 (at sched_idx BV_MAX_SCHED - 1),
# and a segment whose schedule value is 0 (index 3)
SEGS = {1: [(1e-2, 1e-4, 1, 0)], 2: [(1e-2, 1e-4, 0, 0), (5e-3, 0.0, 6, 0)],
        3: [(1e-2, 1e-4, 2, 0), (0.0, 1e-3, MAX_SCHED - 1, 0), (5e-3, 1e-4, 3, 0)]}
AF = dict(eps=1e-30, momentum=0.9)


def af_decay(k, rate=0.8, cap=0.999):
  return min(cap, 1.0 - (float(k) + 1.0) ** (-rate))


def _merge(w, d):
  for k, v in d.items():
    w[k] = max(w.get(k, 0.0), v)


def seg_setup(nchunks, nseg, dev):
  arr = np.array(SEGS[nseg], SEG)
  segs = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)
  cs = (torch.arange(nchunks) % nseg).to(torch.int32)
  el = lambda a: torch.from_numpy(np.ascontiguousarray(a))[cs.long()].repeat_interleave(1024).to(dev)
  return segs, cs.to(dev), el(arr["lr"]), el(arr["wd"]), el(arr["si"]).long()


def chain_case(fns, dev, kind, nchunks, nseg, clip_norm, acc_dtype, nesterov=False, seed=100, gsq_value=None, name=None):
  """kind "adam" | "trace" | "identity"; acc_dtype: dtype of mu / the trace; gsq_value: use this fp64 sum of squares
  instead of sqnorm_ of the gradient (the clip-threshold cases)."""
  count = nchunks * 1024
  name = name or f"{kind} {nchunks}x1024 {nseg}seg clip={clip_norm} {acc_dtype}"
  segs, chunk_seg, lr_t, wd_t, si_t = seg_setup(nchunks, nseg, dev)
  p, _ = B.opt_inputs(count, dev, seed)
  acc = None if kind == "identity" else B.rnd((count,), dev, seed + 2, 1e-3).to(acc_dtype)
  nu = (B.rnd((count,), dev, seed + 3, 1e-3) ** 2) if kind == "adam" else None
  shadow = torch.empty(count, device=dev, dtype=BF16)
  worst = {}
  for i, k in enumerate(STEPS):
    _, g = B.opt_inputs(count, dev, seed + 10 * (i + 1))
    gsq = torch.zeros(1, device=dev, dtype=F64)
    if gsq_value is None:
      fns.sqnorm_(g, gsq)
    else:
      gsq[0] = gsq_value
    sc_t = torch.tensor(SCHED[i], dtype=F32, device=dev)[si_t]
    stats = torch.zeros(2, device=dev, dtype=F64)
    if kind == "adam":
      before = dict(p=p.clone(), g=g, mu=acc.clone(), nu=nu.clone())
      hp = dict(ADAM, bc1=1 - ADAM["b1"] ** (k + 1), bc2=1 - ADAM["b2"] ** (k + 1))
      fns.adam_step_(p, g, acc, nu, shadow, segs, chunk_seg, count, SCHED[i], gsq, clip_norm, hp["b1"], hp["b2"],
                     hp["eps"], hp["bc1"], hp["bc2"], stats)
      new = dict(p=p, mu=acc, nu=nu)
    else:
      before = dict(p=p.clone(), g=g, trace=None if acc is None else acc.clone())
      hp = dict(beta=0.9, nesterov=nesterov)
      fns.trace_step_(p, g, acc, shadow, segs, chunk_seg, count, SCHED[i], gsq, clip_norm, 0.9, nesterov, stats)
      new = dict(p=p, trace=acc)
    w = B.check_chain_step("adam" if kind == "adam" else "trace", new, before, lr_t, wd_t, sc_t, gsq.item(), clip_norm,
                           hp, f"{name} step {k}", stats=stats)
    _merge(worst, w)
    assert torch.equal(shadow, p.to(BF16)), f"{name}: the bf16 shadow is not rne(p')"
    still = sc_t == 0
    assert torch.equal(p[still], before["p"][still]), f"{name}: a parameter under schedule value 0 moved"
  return worst


def clip_gsq(which, clip_norm):
  """The four sums of squares of the clip cases: 0; float32(sqrt(gsq)) == clip_norm exactly (no clip); one fp32 ulp
  above it (clips); gn = 1e3 clip_norm."""
  cn = np.float32(clip_norm)
  return {"zero": 0.0, "at": float(np.float64(cn) ** 2), "ulp-above": float(np.float64(np.nextafter(cn, np.float32(2) * cn)) ** 2),
          "far": float((np.float64(cn) * 1e3) ** 2)}[which]


def sqnorm_case(fns, dev, count, offset=0):
  x = B.rnd((count + offset,), dev, 300 + count % 97, 3.0)
  if count >= 5:
    x[-1] = 100.0                 # the last element (the scalar tail when count % 4 != 0) is visible in the sum
  v = x[offset:]
  out = torch.zeros(1, device=dev, dtype=F64)
  fns.sqnorm_(v, out)
  ref, bnd = B.sqnorm_bound(v)
  return {"sqnorm": B.check(out[0], ref, bnd, (1e-6, 0.0), f"sqnorm count={count} offset={offset}")}


# ------------------------------------------------------------------ Adafactor ----
def af_leaf_record(spec, seed, dev, flat_off=0, soff=0, sched=0, lr_eff=1e-2, wd=1e-4):
  """Inputs and the kernel view of one AF_SPECS leaf, derived the way optax.Adafactor._init_state derives them."""
  from big_vision_amd import optax as bvo
  p, g, shape, strides, off = B.af_leaf_inputs(spec, dev, seed)
  fd = bvo.factored_dims(shape, 32)
  B1, B2, R, C, sB1, sB2, sR, sC, _ = bvo.af_view(spec[0], shape, strides, fd)
  Bn = B1 * B2
  n_state = (Bn * R + Bn * C + Bn) if fd is not None else Bn * R * C
  view = (ctypes.c_long * 9)(flat_off + off, B1, B2, R, C, sB1, sB2, sR, sC)
  assert Bn * R * C == math.prod(shape), (spec[0], shape, tuple(view))
  zero = spec[3] is not None
  state = torch.zeros(n_state, device=dev) if zero else (B.rnd((n_state,), dev, seed + 4, 1e-3) ** 2 + 1e-9)
  return dict(leaf=spec[0], spec=spec, p=p, g=g, view=view, factored=fd is not None, soff=soff, n_state=n_state,
              sched=sched, lr_eff=lr_eff, wd=wd, B=Bn, R=R, C=C, state=state, zero=zero)


def _af_gap(view, n, dev):
  mask = torch.ones(n, dtype=torch.bool, device=dev)
  B.af_views([mask], view)[0].fill_(False)
  return mask


def af_leaf_case(fns, dev, spec, mom_dtype, clip_norm, seed=500, gsq_value=None):
  lf = af_leaf_record(spec, seed, dev)
  name = f"adafactor leaf {spec[0]} {mom_dtype} clip={clip_norm}"
  p, n = lf["p"], lf["p"].numel()
  mom = B.rnd((n,), dev, seed + 5, 0.3).to(mom_dtype)
  state = lf["state"]
  shadow = torch.zeros(n, device=dev, dtype=BF16)
  gap = _af_gap(lf["view"], n, dev)
  worst = {}
  for i, k in enumerate(STEPS):
    g = lf["g"] if i == 0 else B.af_leaf_inputs(spec, dev, seed + 10)[1]
    gsq = torch.zeros(1, device=dev, dtype=F64)
    if gsq_value is None:
      fns.sqnorm_(g, gsq)
    else:
      gsq[0] = gsq_value
    hp = dict(AF, decay=af_decay(k), lr_eff=lf["lr_eff"], wd=lf["wd"], sched=SCHED[i][0])
    before = dict(p=p.clone(), g=g, mom=mom.clone(), state=state.clone())
    stats = torch.zeros(2, device=dev, dtype=F64)
    fns.adafactor_leaf_(p, g, mom, shadow, lf["view"], state, lf["factored"], gsq, clip_norm, hp["decay"], hp["eps"],
                        hp["momentum"], hp["lr_eff"], hp["wd"], hp["sched"], stats)
    w, _ = B.check_af_leaf(dict(p=p, mom=mom, state=state), before, lf["view"], lf["factored"], gsq.item(), clip_norm,
                           hp, f"{name} step {k}", stats=stats)
    _merge(worst, w)
    assert torch.equal(p[gap], before["p"][gap]) and torch.equal(mom[gap], before["mom"][gap]) and \
        not bool(shadow[gap].any()), f"{name}: elements outside the view were written"
    assert torch.equal(shadow[~gap], p[~gap].to(BF16)), f"{name}: the bf16 shadow is not rne(p')"
    assert bool(torch.isfinite(p).all() and torch.isfinite(mom.float()).all() and torch.isfinite(state).all()), name
  return worst


def af_batched_case(fns, dev, mom_dtype, block_rms_clip, single_class, clip_norm=1e-2, seed=700):
  """All AF_SPECS leaves in one flat buffer and one device table through adafactor_step_: sorted and cut into size
  classes by optax.af_table (as Adafactor._init_state does), or as ONE class sized by the largest leaf.  Against the
  model per leaf, and bit for bit against adafactor_leaf_ leaf by leaf when block_rms_clip == 0 (or never clips)."""
  from big_vision_amd import optax as bvo
  name = f"adafactor batched {mom_dtype} block_rms_clip={block_rms_clip} {'one class' if single_class else 'classes'}"
  leaves, off, soff = [], 0, 0
  for j, spec in enumerate(B.AF_SPECS):
    lf = af_leaf_record(spec, seed + j, dev, flat_off=off, soff=soff, sched=j % 2, lr_eff=(1e-2, 5e-3, 2e-2)[j % 3],
                        wd=(1e-4, 0.0)[j % 2])
    lf["base"], lf["n"] = off, lf["p"].numel()
    leaves.append(lf)
    off += lf["n"] + 3                                  # leaves start at odd offsets, 3 untouched elements between them
    soff += (lf["n_state"] + 3) // 4 * 4
  N = off
  cat = lambda key, fill: torch.cat([torch.cat([lf[key], torch.full((3,), fill, device=dev)]) for lf in leaves])
  p = cat("p", 7.0)
  state = torch.zeros(soff, device=dev)
  for lf in leaves:
    state[lf["soff"]:lf["soff"] + lf["n_state"]] = lf["state"]
  mom = B.rnd((N,), dev, seed + 50, 0.3).to(mom_dtype)
  shadow = torch.zeros(N, device=dev, dtype=BF16)
  gap = torch.ones(N, dtype=torch.bool, device=dev)
  for lf in leaves:
    B.af_views([gap], lf["view"])[0].fill_(False)
  by_base = leaves
  tab, classes, leaves = bvo.af_table(leaves)           # `leaves`: the records in table order from here on
  if single_class:
    classes = [dict(first=0, n=len(leaves), rows=max(c["rows"] for c in classes), cols=max(c["cols"] for c in classes),
                    b=max(c["b"] for c in classes), total=max(c["total"] for c in classes))]
  else:
    assert len(classes) >= 3 and any(c["n"] > 1 for c in classes), classes
  table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev).view(-1, bvo.AF_LEAF.itemsize)
  p2, mom2, state2, shadow2 = p.clone(), mom.clone(), state.clone(), shadow.clone()
  worst = {}
  for i, k in enumerate(STEPS):
    g = cat("g", 9.0) if i == 0 else torch.cat(
        [torch.cat([B.af_leaf_inputs(lf["spec"], dev, seed + 100 + j)[1], torch.full((3,), 9.0, device=dev)])
         for j, lf in enumerate(by_base)])
    gsq = torch.zeros(1, device=dev, dtype=F64)
    fns.sqnorm_(g, gsq)
    decay = af_decay(k)
    before = dict(p=p.clone(), g=g, mom=mom.clone(), state=state.clone())
    stats = torch.zeros(2, device=dev, dtype=F64)
    usq_all = {}
    for c in classes:
      usq = torch.zeros(c["n"], device=dev, dtype=F64) if block_rms_clip > 0 else None
      fns.adafactor_step_(p, g, mom, shadow, table[c["first"]:c["first"] + c["n"]], c["n"], c["rows"], c["cols"], c["b"],
                          c["total"], state, gsq, clip_norm, decay, AF["eps"], AF["momentum"], SCHED[i], stats,
                          block_rms_clip=block_rms_clip, block_usq=usq)
      for j in range(c["n"]):
        usq_all[c["first"] + j] = None if usq is None else usq[j]
    sref, sbnd = 0.0, 0.0
    for j, lf in enumerate(leaves):
      hp = dict(AF, decay=decay, lr_eff=lf["lr_eff"], wd=lf["wd"], sched=SCHED[i][lf["sched"]])
      sl = slice(lf["soff"], lf["soff"] + lf["n_state"])
      w, m = B.check_af_leaf(dict(p=p, mom=mom, state=state[sl]), dict(before, state=before["state"][sl]), lf["view"],
                             lf["factored"], gsq.item(), clip_norm, hp, f"{name} step {k} {lf['leaf']}",
                             block_rms_clip=block_rms_clip, usq=usq_all[j], grid_cap=1024)
      _merge(worst, w)
      sref, sbnd = sref + m["stats"][0], sbnd + m["stats"][1]
      if block_rms_clip >= 1e6:
        assert m["scale"] == (1.0, 0.0), (name, lf["leaf"], m["scale"])   # never clips: the scale is exactly 1
    _merge(worst, {"stats": B.check_stats(stats, sref, sbnd, f"{name} step {k} stats")})
    assert torch.equal(p[gap], before["p"][gap]) and torch.equal(mom[gap], before["mom"][gap]) and \
        not bool(shadow[gap].any()), f"{name}: elements outside the leaves were written"
    assert torch.equal(shadow[~gap], p[~gap].to(BF16)), f"{name}: the bf16 shadow is not rne(p')"
    if block_rms_clip == 0 or block_rms_clip >= 1e6:
      for lf in leaves:
        fns.adafactor_leaf_(p2, g, mom2, shadow2, lf["view"], state2[lf["soff"]:lf["soff"] + lf["n_state"]],
                            lf["factored"], gsq, clip_norm, decay, AF["eps"], AF["momentum"], lf["lr_eff"], lf["wd"],
                            SCHED[i][lf["sched"]], None)
      assert torch.equal(p, p2) and torch.equal(mom, mom2) and torch.equal(state, state2) and \
          torch.equal(shadow, shadow2), f"{name} step {k}: the batched step differs from the per-leaf entry"
  return worst
