"""Memory-footprint harness: runs ONE call of a kernel entry point on operands carved out of a single guarded arena and
holds the call to the extents include/bvhip.h states for them.

The contract ("Memory footprint"):
  1. writes    no byte changes outside the declared extent of an `out` / `inout` / `scratch` operand: inputs stay
               bit-identical, pitch-gap columns and unselected rows belong to no extent, neither do the guard bands;
  2. reads     no output element depends on a byte outside the declared extent of an input operand;
  3. coverage  every element of an `out` operand is written;
  4. value     left to the caller: `run` returns the operands as CPU tensors for the suite's fp64 checks.

How: the arena is one uint8 tensor of 0xFF bytes (a NaN in fp32 and bf16, -1 in int32, 255 in uint8).  Every operand
sits at a 256-byte-aligned offset between two guard bands of its own (>= 64 KiB, or one tile-row block of the operand
when that is larger), so an overrun of a few rows or of "the next tile" lands in memory the test owns.  `in` operands
are filled from a seeded CPU generator, `inout` operands with a finite base, `out` / `scratch` operands keep the 0xFF
fill.  After the call the whole arena is compared with its pre-call snapshot under the mask of the write extents (1);
an `out` element that is still 0xFF was never written (3); a non-finite output element has either never been written
or has taken a 0xFF byte from outside an input extent (2) - the harness tells the two apart, and finds the bytes that
were read, by re-running the call on fresh arenas in which chosen 0xFF bytes are zeroed (failure path only).

Device-agnostic, plain torch: the GPU rows pass pointers into a device arena to `_lib.call`; the CPU proof
(test_footprint_cpu.py) drives the same code with torch "kernels" on a CPU arena.
"""
import torch

GUARD = 64 << 10      # minimum guard band, bytes
ALIGN = 256
WORD = 8              # granularity of the read-dependence search: no element of any dtype used here straddles a word

ROLES = ("in", "out", "inout", "scratch")


def _up(x, a=ALIGN):
  return (x + a - 1) // a * a


class Op:
  """One operand.  `shape` / `strides` / `offset` (elements) describe its EXTENT inside an allocation of `alloc`
  elements whose first element is what the kernel gets as pointer: a pitched matrix is shape (rows, cols), strides
  (ld, 1); the rows a strided LayerNorm selects are shape (rows, D), strides (row_stride * D, 1), offset row_offset * D.
  role: "in" (read extent, must stay bit-identical), "out" (write extent, every element must be written), "inout"
  (read and write: accumulated in place), "scratch" (write extent the caller never reads: workspaces).
  fill: `in` / `inout` values - a tensor of the extent's shape, a float (standard deviation of seeded normal values) or
  None (normal values of deviation 1 for `in`, the constant 0.5 for `inout`).
  band: bytes of one tile-row block of the operand; the guard bands are max(64 KiB, band).
  runs: instead of shape / strides / offset, a list of (offset, length) runs of a flat buffer of `alloc` elements (the
  leaves an optimizer table addresses inside one parameter buffer): the extent is their union, the operand's value
  their concatenation; a tensor `fill` covers the whole buffer and the runs are cut from it."""

  def __init__(self, name, dtype, shape=None, role="in", strides=None, offset=0, alloc=None, fill=None, band=0, runs=None):
    assert role in ROLES, role
    self.name, self.dtype, self.role, self.fill = name, dtype, role, fill
    self.runs = None if runs is None else [(int(a), int(n)) for a, n in runs]
    if runs is not None:
      assert alloc is not None and all(a + n <= alloc for a, n in self.runs)
      shape, strides, offset = (sum(n for _, n in self.runs),), None, 0
      if torch.is_tensor(fill):
        self.fill = torch.cat([fill.reshape(-1)[a:a + n] for a, n in self.runs])
    self.shape = tuple(int(s) for s in shape)
    if strides is None:
      strides, acc = [], 1
      for s in reversed(self.shape):
        strides.insert(0, acc)
        acc *= s
    self.strides = tuple(int(s) for s in strides)
    self.offset = int(offset)
    last = self.offset + sum((n - 1) * s for n, s in zip(self.shape, self.strides)) + 1 if runs is None else 1
    self.alloc = int(alloc) if alloc is not None else last
    assert self.alloc >= last and all(n > 0 for n in self.shape), (name, self.alloc, last)
    self.itemsize = torch.empty((), dtype=dtype).element_size()
    self.guard = _up(max(GUARD, int(band)))
    self.nbytes = self.alloc * self.itemsize
    self.start = None   # byte offset of the allocation in the arena (set by Arena)

  def extents(self):
    """[(shape, strides, offset)] of the pieces of the extent."""
    if self.runs is None:
      return [(self.shape, self.strides, self.offset)]
    return [((n,), (1,), a) for a, n in self.runs]

  def element_offset(self, idx):
    """Element offset in the allocation of the extent element with (multi-)index idx."""
    if self.runs is None:
      return self.offset + sum(i * s for i, s in zip(idx, self.strides))
    i = idx[0]
    for a, n in self.runs:
      if i < n:
        return a + i
      i -= n
    raise IndexError(idx)


def mat(name, dtype, rows, cols, ld=None, role="in", fill=None, tile_rows=256):
  """A row-major matrix of pitch ld (elements); guard = one block of tile_rows rows."""
  ld = cols if ld is None else ld
  isz = torch.empty((), dtype=dtype).element_size()
  return Op(name, dtype, (rows, cols), role, strides=(ld, 1), fill=fill, band=tile_rows * ld * isz)


class Arena:
  def __init__(self, ops, device="cpu", seed=0, zero=None):
    """zero: optional bool mask over the arena's bytes (CPU) of 0xFF bytes to replace by 0 (read-dependence search)."""
    self.ops = {o.name: o for o in ops}
    assert len(self.ops) == len(ops), "operand names must be unique"
    cur = 0
    for o in ops:
      o.start = cur + o.guard
      cur = _up(o.start + o.nbytes) + o.guard
    self.nbytes = cur
    buf = torch.full((cur,), 0xFF, dtype=torch.uint8)
    self.inputs = {}
    gen = torch.Generator(device="cpu").manual_seed(seed)
    for o in ops:
      if o.role in ("out", "scratch"):
        continue
      f = o.fill
      if torch.is_tensor(f):
        val = f.detach().cpu().to(o.dtype).reshape(o.shape)
      elif o.role == "inout" and f is None:
        val = torch.full(o.shape, 0.5).to(o.dtype)
      else:
        val = (torch.randn(o.shape, generator=gen, dtype=torch.float32) * (1.0 if f is None else float(f))).to(o.dtype)
      at = 0
      for v in self._pieces(buf, o):
        v.copy_(val.reshape(-1)[at:at + v.numel()].reshape(v.shape))
        at += v.numel()
      self.inputs[o.name] = val.clone()
    if zero is not None:
      assert not bool((zero & (buf != 0xFF)).any()), "only 0xFF filler bytes may be zeroed"
      buf[zero] = 0
    self.device = torch.device(device)
    self.buf = buf.to(self.device)
    self.base = self.buf.data_ptr()

  # ---- views
  @staticmethod
  def _pieces(buf, o):
    flat = buf[o.start:o.start + o.nbytes].view(o.dtype)
    return [torch.as_strided(flat, sh, st, flat.storage_offset() + off) for sh, st, off in o.extents()]

  @staticmethod
  def _bytes(buf, o):
    """The extent's bytes, [..., itemsize] per piece."""
    isz = o.itemsize
    return [torch.as_strided(buf, tuple(sh) + (isz,), tuple(s * isz for s in st) + (1,), buf.storage_offset() + o.start + off * isz)
            for sh, st, off in o.extents()]

  def view(self, name):
    """The operand's extent as a strided tensor view into the arena (an operand made of runs: their concatenation, a
    copy)."""
    v = self._pieces(self.buf, self.ops[name])
    return v[0] if len(v) == 1 else torch.cat(v)

  def around(self, name):
    """(flat typed view of the allocation with both guard bands, index of the allocation's first element in it): how a
    kernel that leaves its extents is written in the CPU proof."""
    o = self.ops[name]
    lo, hi = o.start - o.guard, _up(o.start + o.nbytes) + o.guard
    return self.buf[lo:hi].view(o.dtype), o.guard // o.itemsize

  def ptr(self, name):
    """Device address of the allocation's first element (None for an absent optional operand)."""
    return None if name is None else self.base + self.ops[name].start

  def get(self, name):
    return self.view(name).detach().cpu().clone()

  # ---- masks over the arena's bytes (CPU bool tensors)
  def _extent_mask(self, roles):
    m = torch.zeros(self.nbytes, dtype=torch.bool)
    for o in self.ops.values():
      if o.role in roles:
        for v in self._bytes(m, o):
          v.fill_(True)
    return m

  def write_mask(self):
    return self._extent_mask(("out", "inout", "scratch"))

  def filler_mask(self):
    """The 0xFF bytes no output may depend on: everything outside the `in` / `inout` / `out` extents (an `out` extent
    keeps its fill in the search, so that an element never written stays recognisable)."""
    return ~self._extent_mask(("in", "inout", "out"))

  def locate(self, byte):
    """(operand, offset relative to its allocation, where) of an arena byte."""
    for o in self.ops.values():
      lo, hi = o.start - o.guard, _up(o.start + o.nbytes) + o.guard
      if lo <= byte < hi:
        rel = byte - o.start
        if rel < 0:
          where = "guard band before"
        elif rel >= o.nbytes:
          where = "guard band after"
        else:
          inside = False
          for sh, st, off in o.extents():
            e = rel // o.itemsize - off
            ok = e >= 0
            for n, s_ in sorted(zip(sh, st), key=lambda t: -t[1]):
              q, e = (divmod(e, s_) if s_ else (0, e))
              ok = ok and q < n
            inside = inside or (ok and e == 0)
          where = "extent" if inside else "pitch gap / unselected row"
        return o, rel, where
    raise AssertionError(byte)


class Result:
  def __init__(self, arena):
    self.inp = arena.inputs
    self.out = {n: arena.get(n) for n, o in arena.ops.items() if o.role in ("out", "inout")}
    self.arena = arena

  def __getitem__(self, name):
    return self.out[name] if name in self.out else self.inp[name]


def _sync(device):
  if torch.device(device).type == "cuda":
    torch.cuda.synchronize()


def _nonfinite(arena):
  """{operand: bool tensor of the extent's shape} of the non-finite elements of floating out / inout operands."""
  bad = {}
  for o in arena.ops.values():
    if o.role in ("out", "inout") and o.dtype.is_floating_point:
      b = ~torch.isfinite(arena.view(o.name).float()).cpu()
      if bool(b.any()):
        bad[o.name] = b
  return bad


def _unwritten(arena, o):
  """Elements of operand o whose bytes are all still 0xFF."""
  by = [(b == 0xFF).all(-1) for b in arena._bytes(arena.buf, o)]
  return (by[0] if len(by) == 1 else torch.cat(by)).cpu()


def _first(o, mask):
  """(byte offset relative to the allocation of the first set element, number of set elements)."""
  idx = mask.nonzero()[0].tolist()
  return o.element_offset(idx) * o.itemsize, int(mask.sum())


def run(entry, case, make_ops, call, device="cpu", seed=0, prepare=None):
  """One guarded call.  make_ops() -> list of Op (fresh objects on every invocation: the read-dependence search builds
  more arenas); call(arena) enqueues the kernel(s) on operands of that arena; prepare(arena), optional, runs before the
  snapshot and fills `in` operands whose values are addresses inside the arena (device tables of pointers).  Raises AssertionError with one line per
  finding, `<entry>[<case>]: <kind>: operand '<name>' (<where>), byte offset <relative to the operand>, <count>`;
  returns a Result (CPU tensors of the operands after the call) for the value check."""
  tag = f"{entry}[{case}]"
  arena = Arena(make_ops(), device, seed)
  if prepare is not None:
    prepare(arena)
    for n in arena.inputs:
      arena.inputs[n] = arena.get(n)
  snap = arena.buf.clone()
  call(arena)
  _sync(device)
  msgs = []
  # 1. writes
  changed = ((arena.buf != snap).cpu()) & ~arena.write_mask()
  if bool(changed.any()):
    groups = {}
    for b in changed.nonzero().flatten().tolist():
      o, rel, where = arena.locate(b)
      g = groups.setdefault((o.name, where), [rel, 0])
      g[1] += 1
      if len(groups) > 16:
        break
    for (name, where), (rel, cnt) in groups.items():
      kind = "input modified" if arena.ops[name].role == "in" and where == "extent" else "write outside the extent"
      msgs.append(f"{tag}: {kind}: operand '{name}' ({where}), byte offset {rel}, {cnt} byte(s)")
  # 3. coverage of the outputs that cannot show a NaN
  for o in arena.ops.values():
    if o.role == "out" and not o.dtype.is_floating_point:
      u = _unwritten(arena, o)
      if bool(u.any()):
        off, cnt = _first(o, u)
        msgs.append(f"{tag}: not written: operand '{o.name}' (extent), byte offset {off}, {cnt} element(s)")
  # 2. + 3. non-finite outputs: never written, or fed from outside an input extent
  bad = _nonfinite(arena)
  if bad:
    msgs += _explain(tag, arena, bad, make_ops, call, device, seed, prepare)
  assert not msgs, "\n".join(msgs)
  return Result(arena)


def _explain(tag, arena, bad, make_ops, call, device, seed, prepare=None):
  filler = arena.filler_mask()

  def still_bad(zero):
    a = Arena(make_ops(), device, seed, zero=zero)
    if prepare is not None:
      prepare(a)
    call(a)
    _sync(device)
    return _nonfinite(a), a

  msgs = []
  bad0, _ = still_bad(filler.clone())         # every byte around the operands finite: what is still non-finite was
                                              # never written (or was computed from the output's own stale contents)
  for name, b in bad.items():
    o = arena.ops[name]
    unwritten = bad0[name] & b if name in bad0 else torch.zeros_like(b)
    if bool(unwritten.any()):
      off, cnt = _first(o, unwritten)
      msgs.append(f"{tag}: not written: operand '{name}' (extent), byte offset {off}, {cnt} element(s)"
                  + ("" if o.role == "out" else " [non-finite whatever the bytes around the operands hold]"))
    dep = b & ~unwritten
    if bool(dep.any()):
      off, cnt = _first(o, dep)
      msgs.append(f"{tag}: output depends on bytes outside the input extents: operand '{name}' (extent), byte offset "
                  f"{off}, {cnt} element(s)")
  if not any("depends on" in m for m in msgs):
    return msgs
  # which bytes: keep only words [lo, hi) of the filler at 0xFF, zero the rest, and halve while the outputs stay bad
  words = (filler.view(-1, WORD).any(-1)).nonzero().flatten()
  lo, hi = 0, words.numel()
  for _ in range(64):
    if hi - lo <= 1:
      break
    mid = (lo + hi) // 2
    for l, h in ((lo, mid), (mid, hi)):
      zero = filler.clone()
      keep = words[l:h]
      zero.view(-1, WORD)[keep] = False
      if still_bad(zero)[0]:
        lo, hi = l, h
        break
    else:
      break    # the dependence needs bytes of both halves: report the range reached
  b0, b1 = int(words[lo]) * WORD, int(words[hi - 1]) * WORD + WORD
  o, rel, where = arena.locate(b0)
  msgs.append(f"{tag}: read outside the extent: operand '{o.name}' ({where}), byte offset {rel}, within {b1 - b0} byte(s)")
  return msgs
