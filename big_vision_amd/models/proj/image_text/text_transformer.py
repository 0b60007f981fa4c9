"""Text tower on gfx950 kernels behind `models.proj.image_text.text_transformer`.

Mirrors big_vision/models/proj/image_text/text_transformer.py: `Model(num_classes,
*, variant=None, **kw)` (:102-104), Flax-named params (`Embed_0/embedding`,
`pos_embedding`, `Encoder_0/...`, `head/...`), forward per `_Model.__call__`
(:55-99): embed -> +posemb -> bidirectional vit.Encoder -> pooling -> head.
`vocab_logits` (:80) is dead code for the loss and is only produced on request.
"""
from __future__ import annotations

import math

import torch

from big_vision_amd import engine as E
from big_vision_amd import ops
from big_vision_amd import utils
from big_vision_amd.models import common
from big_vision_amd.models import vit
from big_vision_amd.params import Entry, ParamStore

BF16, F32 = torch.bfloat16, torch.float32


class TextExec:
  def __init__(self, m: "_Model", store: ParamStore, prefix: str, seq_len: int):
    self.m, self.store, self.seq_len = m, store, seq_len
    D, H, M = m.width, m.num_heads, m.mlp_dim
    self.table = E._W(store, f"{prefix}Embed_0/embedding")
    self.pos = E._W(store, f"{prefix}pos_embedding", (seq_len, D))
    self.enc = E.Encoder(store, f"{prefix}Encoder_0", m.depth, D, H, M, scan=getattr(m, "scan", False))
    pool = {"last": "row", "first": "row", "mean": "gap", "gmp": "max"}.get(m.pool_type, m.pool_type)   # text_transformer.py:82-96
    # (the selected token's encoder_norm also writes the head's bf16 operand)
    self.tail = E.PooledTail(store, prefix, self.enc, pool, H, M, num_classes=m.num_classes,
                             row=-1 if m.pool_type == "last" else 0, row_bf16=True)

  def fwd(self, text, save=False, collect=False, drop=None):
    """drop (engine.Dropout): train mode with dropout > 0 - the encoder blocks' sites (text_transformer.py:72-75)."""
    m = self.m
    D = m.width
    out = {}
    ids = text.to(torch.int32).contiguous()
    n, L = ids.shape
    assert L == self.seq_len, f"text length {L} != initialised length {self.seq_len}"
    x = ops.embed_fwd(ids, self.table.f32, self.pos.f32, n, L)
    enc_out = {} if collect else None
    xL, saved = self.enc.fwd(x, n, L, save, enc_out, drop=drop)
    if collect:
      out.update(enc_out)
      T = n * L
      _, yf, _, _ = self.enc.norm.fwd(xL, T, D, want_bf16=False, want_f32=True)
      out["transformed"] = yf.view(n, L, D)
      # text_transformer.py:64 / :80: the token embedding before the position embedding, and the
      # weight-tied vocabulary logits embedding.attend(x) = x . table^T (fp32, diagnostics only)
      out["embedded"] = ops.embed_fwd(ids, self.table.f32, torch.zeros_like(self.pos.f32), n, L).view(n, L, D)
      V = self.table.f32.shape[0]
      vl = torch.empty((T, V), device=yf.device, dtype=F32)
      ops.sgemm(yf, D, 1, self.table.f32, 1, D, vl, T, V, D)
      out["vocab_logits"] = vl.view(n, L, V)
    x, t_out, tctx = self.tail.fwd(xL, saved, n, L)
    out.update({k: t_out[k] for k in ("pre_logits", "logits") if k in t_out})
    ctx = dict(n=n, L=L, ids=ids, tail=tctx)
    return x, out, (ctx if save else None)

  def bwd(self, ctx, dx, on_block=None):
    n, L, D = ctx["n"], ctx["L"], self.m.width
    dx0, _ = self.tail.bwd(ctx["tail"], dx, on_block=on_block)
    if self.table.grad is not None:
      ops.embed_bwd(ctx["ids"].view(-1), dx0, self.table.grad)
    if self.pos.grad is not None:
      ops.batchsum(dx0, self.pos.grad, n, L, D)


class _Model(common.Tower):
  """Text transformer similar to CLIP (config holder + Flax-like init/apply)."""
  Exec, encoder = TextExec, "Encoder_0"

  def __init__(self, num_classes, width=512, depth=12, mlp_dim=2048, num_heads=8, dropout=0.0,
               vocab_size=32_000, pool_type="last", scan=False, remat_policy="nothing_saveable",
               name=None):
    if not 0.0 <= float(dropout) < 1.0:
      raise ValueError(f"dropout must be in [0, 1), got {dropout}")
    self.dropout = float(dropout)
    if pool_type not in ("last", "first", "mean", "gap", "max", "gmp", "map"):
      raise NotImplementedError(f"Cannot do pooling '{pool_type}'")
    common.check_head_dim(width, num_heads)
    self.num_classes, self.width, self.depth, self.mlp_dim = num_classes, width, depth, mlp_dim
    self.num_heads, self.vocab_size, self.pool_type, self.scan = num_heads, vocab_size, pool_type, scan
    self.name = name
    self._execs = {}

  def entries(self, prefix, seq_len):
    D, H, M = self.width, self.num_heads, self.mlp_dim
    # nn.Embed default init: variance_scaling(1.0, "fan_in", "normal", out_axis=0)
    ents = [Entry(f"{prefix}Embed_0/embedding", (self.vocab_size, D), E.init_normal(1 / math.sqrt(D))),
            Entry(f"{prefix}pos_embedding", (1, seq_len, D), E.init_normal(1 / math.sqrt(D)))]
    ents += E.encoder_entries(f"{prefix}Encoder_0", self.depth, D, H, M)
    if self.pool_type == "map":
      ents += E.map_entries(f"{prefix}MAPHead_0", D, H, M)
    return ents + common.head_entries(prefix, D, self.num_classes, head_zeroinit=False)

  def layout(self, text_shape):
    return text_shape[1]


def Model(num_classes, *, variant=None, **kw):  # pylint: disable=invalid-name
  """Factory function (reference text_transformer.py:102-104)."""
  return _Model(num_classes, **{**vit.decode_variant(variant), **kw})


def load(init_params, init_file, model_cfg, dont_load=()):  # pylint: disable=invalid-name
  """Load init from checkpoint (text_transformer.py:107-119)."""
  params = utils.load_params(init_file)
  params = utils.tree_map(lambda x: x, params)
  extra_posemb = params["Encoder_0"].pop("pos_embedding", 0)
  params["pos_embedding"] = params["pos_embedding"] + extra_posemb
  if init_params:
    want_scan = "encoderblock" in init_params.get("Encoder_0", {})
  else:
    want_scan = bool((model_cfg or {}).get("scan", False))
  have_scan = "encoderblock" in params["Encoder_0"]
  if have_scan and not want_scan:
    params["Encoder_0"] = vit.scan_to_pyloop({"Transformer": params["Encoder_0"]})["Transformer"]
  elif want_scan and not have_scan:
    params["Encoder_0"] = vit.pyloop_to_scan({"Transformer": params["Encoder_0"]})["Transformer"]
  return common.merge_params(params, init_params, dont_load)
