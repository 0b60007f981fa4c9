"""ctypes binding of the kernel libraries of build.LIBS: libbvhip.so (the C ABI declared in include/bvhip.h),
libbvdistill.so (include/bvdistill.h) and libbveval.so (include/bveval.h).  One Library record each, one path that
binds them (`_bind`) and one that calls into them (`call`).

The product path has NO fallback: if the shared library is missing or a call
fails, a RuntimeError is raised.  Build it with `python big_vision_amd/build.py`
(or `__graft_entry__.build()`).
"""
import ctypes
import os

# torch bundles its own libamdhip64; it must be loaded BEFORE libbvhip.so so both
# share ONE HIP runtime (otherwise libbvhip binds /opt/rocm's copy and launches
# fail with "no ROCm-capable device").
import torch  # noqa: F401  pylint: disable=unused-import

from ctypes import c_int, c_long, c_float, c_void_p

from big_vision_amd import build

P = c_void_p

# libbvhip.so (include/bvhip.h): name -> argtypes (the return type is int unless RESTYPES names another)
PROTOTYPES = {
    "bv_version": [],
    # the caller's context (options, split-K workspace, launch counters): the library keeps no global state
    "bv_ctx_create": [], "bv_ctx_destroy": [P], "bv_ctx_set": [P, c_int, c_long], "bv_ctx_get": [P, c_int],
    "bv_ctx_set_workspace": [P, P, c_long],
    "bv_gemm_bf16": [c_int, c_int, P, c_long, P, c_long, P, c_long, c_int, c_int, c_int, c_int,
                     c_int, P, P, c_long, c_int, P, c_float, c_int, P, P],
    "bv_gemm_bf16_colsum": [c_int, c_int, P, c_long, P, c_long, P, c_long, c_int, c_int, c_int, c_int,
                            c_int, P, P, c_long, c_int, P, c_float, c_int, P, P, P],
    "bv_gemm_workspace_bytes": [c_int, c_int, c_int],
    "bv_sgemm_strided": [P, c_long, c_long, P, c_long, c_long, P, c_long, c_int, c_int, c_int,
                         c_float, c_float, P, P, P],
    "bv_layernorm_fwd": [P, P, P, P, P, P, P, c_int, c_int, c_long, c_long, c_float, P],
    "bv_layernorm_fwd_bf16x": [P, P, P, P, P, P, P, c_int, c_int, c_long, c_long, c_float, P],
    "bv_layernorm_bwd": [P, c_int, P, P, P, P, P, P, P, P, P, P, c_int, c_int, c_long, c_long, P],
    "bv_layernorm_bwd_y": [P, c_int, P, P, P, P, P, P, P, P, P, P, c_int, c_int, c_long, c_long, P, P, P],
    "bv_layernorm_bwd_bf16x": [P, c_int, P, P, P, P, P, P, P, P, P, c_int, c_int, c_long, c_long, P],
    "bv_attn_fwd": [P, P, P, c_int, c_int, c_int, P, P],
    "bv_attn_bwd": [P, P, P, P, P, P, P, c_int, c_int, c_int, P, P],
    "bv_attn_fwd_masked": [P, P, P, P, c_int, c_int, c_int, P, P],
    "bv_attn_bwd_masked": [P, P, P, P, P, P, P, c_int, c_int, c_int, P, P],
    "bv_map_attn_fwd": [P, P, P, P, c_int, c_int, c_int, P],
    "bv_map_attn_bwd": [P, P, P, P, P, P, c_int, c_int, c_int, P],
    "bv_map_attn_fwd_masked": [P, P, P, P, P, c_int, c_int, c_int, P],
    "bv_attn_fwd_dh": [P, P, P, P, c_int, c_int, c_int, c_int, P],
    "bv_attn_bwd_dh": [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "bv_map_attn_fwd_dh": [P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "bv_map_attn_bwd_dh": [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "bv_pool_gap_masked_fwd": [P, P, P, c_int, c_int, c_int, P],
    "bv_pool_gap_masked_bwd": [P, P, P, c_int, c_int, c_int, P],
    "bv_naflex_posemb_weights": [P, P, P, c_int, c_int, c_int, P],
    "bv_patchify": [P, P, c_int, c_int, c_int, c_int, P],
    "bv_patchify_ld": [P, P, c_int, c_int, c_int, c_int, c_int, P],
    "bv_embed_fwd": [P, P, P, P, c_int, c_int, c_int, c_int, P],
    "bv_embed_bwd": [P, P, P, c_int, c_int, c_int, P],
    "bv_colsum": [P, c_int, c_long, P, c_int, c_int, P],
    "bv_batchsum": [P, P, c_int, c_int, c_int, P],
    "bv_cast_bf16": [P, P, c_long, P],
    "bv_cast_f32": [P, P, c_long, P],
    "bv_transpose_bf16": [P, P, c_int, c_int, c_long, c_long, P],
    "bv_transpose_bf16_batched": [P, c_int, c_int, P],
    "bv_concat_cls": [P, P, P, c_int, c_int, c_int, P],
    "bv_pool_gap_fwd": [P, P, c_int, c_int, c_int, P],
    "bv_pool_gap_bwd": [P, P, c_int, c_int, c_int, P],
    "bv_pool_max_fwd": [P, P, P, c_int, c_int, c_int, P],
    "bv_pool_max_masked_fwd": [P, P, P, P, c_int, c_int, c_int, P],
    "bv_pool_max_bwd": [P, P, P, c_int, c_int, c_int, P],
    "bv_l2norm_fwd": [P, P, P, c_int, c_int, c_float, P],
    "bv_l2norm_bwd": [P, P, P, P, c_int, c_int, c_float, P],
    "bv_siglip_loss": [P, P, P, P, c_int, c_int, c_int, c_int, P],
    "bv_logit_stats": [P, P, P, P, P, c_int, c_int, c_int, P],
    "bv_dot_f32": [P, P, c_long, P, P],
    "bv_softmax_xent": [P, P, P, P, c_int, c_int, c_int, P],
    "bv_sigmoid_xent": [P, P, P, P, c_int, c_int, c_int, P],
    "bv_tanh_fwd": [P, P, c_long, P],
    "bv_tanh_bwd": [P, P, P, c_long, P],
    "bv_mixup": [P, P, c_float, c_int, c_long, P],
    "bv_dropout_f32": [P, P, P, P, c_long, ctypes.c_ulonglong, c_float, P],
    "bv_dropout_bf16": [P, P, c_long, ctypes.c_ulonglong, c_float, P],
    "bv_dropout_mask": [P, c_long, ctypes.c_ulonglong, c_float, P],
    "bv_sqnorm": [P, c_long, P, P],
    "bv_adam_step": [P, P, P, c_int, P, P, P, P, c_long, P, c_int, P, c_float, c_float, c_float,
                     c_float, c_float, c_float, P, P],
    "bv_trace_step": [P, P, P, c_int, P, P, P, c_long, P, c_int, P, c_float, c_float, c_int, P, P],
    "bv_adafactor_leaf": [P, P, P, c_int, P, P, P, c_int, P, c_float, c_float, c_float, c_float,
                          c_float, c_float, c_float, P, P],
    "bv_adafactor_step": [P, P, P, c_int, P, P, c_int, c_long, c_long, c_long, c_long, P, P, c_float, c_float,
                          c_float, c_float, P, c_int, P, c_float, P, P],
    # collectives for non-Python hosts (csrc/comm.cpp; the Python host uses torch.distributed, dp.py)
    "bv_comm_version": [P], "bv_comm_unique_id": [P], "bv_comm_init": [P, c_int, c_int, P], "bv_comm_destroy": [P],
    "bv_comm_all_gather": [P, P, P, c_long, c_int, P], "bv_comm_reduce_scatter": [P, P, P, c_long, c_int, P],
    "bv_comm_all_reduce_bucket": [P, P, c_long, c_long, c_int, P],
}

# the entry points of libbvhip.so that do not return an int status
RESTYPES = {"bv_gemm_workspace_bytes": c_long, "bv_ctx_create": P, "bv_ctx_destroy": None, "bv_ctx_set": c_long,
            "bv_ctx_get": c_long}

# bv_ctx options / statistics (include/bvhip.h)
OPTS = {"fast_path": 0, "gemm_nt": 1, "gemm_skew_mode": 2, "gemm_skew_pct": 3, "gemm_pre_issue": 4, "gemm_roll": 5,
        "gemm_group_n": 6, "gemm_reserve_cus": 7, "attn_cfg": 8, "sgemm_mfma": 9,
        "gemm256_calls": 100, "gemm256_multi": 101, "gemm256_fused": 102}

# libbvdistill.so (include/bvdistill.h): name -> argtypes, every one returns an int status
PROTOTYPES_DISTILL = {
    "bv_distill_version": [],
    "bv_distill_dist": [c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_int, P],
    "bv_distill_entropy": [P, P, P, c_int, c_int, c_int, P],
    "bv_distill_softmax_acc": [P, P, c_float, c_int, c_int, c_int, P],
}
# BVD_KIND_* of include/bvdistill.h, by the names of evaluators/proj/distill/distance.py
DISTILL_KINDS = {"l2": 0, "euclidean": 1, "kl": 2, "hard": 3, "logsoftmax_euclidean": 4, "agree": 5}

# libbveval.so (include/bveval.h): name -> argtypes, every one returns an int status
PROTOTYPES_EVAL = {
    "bv_eval_version": [],
    "bv_eval_classify": [c_int, P, P, P, P, P, P, c_int, c_int, P],
}
# BVE_LOSS_* of include/bveval.h, by the `loss_name` of evaluators/classification.py
EVAL_LOSSES = {"softmax_xent": 0, "sigmoid_xent": 1}

EPI_NONE, EPI_RESIDUAL, EPI_POS, EPI_GELU, EPI_GELU_BWD, EPI_ATOMIC, EPI_GELU_BWD_EMIT, EPI_GELU_GD, EPI_MUL, EPI_GELU_G = range(10)


class Library:
  """One kernel library: the file and header of its build.LIBS record (`path` may be pointed at another build of the
  same ABI before the first load()), its prototype table with the restypes that are not int, its last-error and
  version entry points and the ABI version this binding expects.  `dll` is the bound CDLL, None until load()."""

  def __init__(self, path, header, prototypes, last_error, version_fn, version, restypes=None):
    self.name, self.path, self.header = os.path.basename(path), path, header
    self.prototypes, self.restypes = prototypes, restypes or {}
    self.last_error, self.version_fn, self.version = last_error, version_fn, version
    self.dll = None


_BINDINGS = {
    "hip": dict(prototypes=PROTOTYPES, restypes=RESTYPES, last_error="bv_last_error", version_fn="bv_version", version=2),
    "distill": dict(prototypes=PROTOTYPES_DISTILL, last_error="bv_distill_last_error", version_fn="bv_distill_version",
                    version=1),
    "eval": dict(prototypes=PROTOTYPES_EVAL, last_error="bv_eval_last_error", version_fn="bv_eval_version", version=1),
}
LIBRARIES = {r.key: Library(r.path, r.header, **_BINDINGS[r.key]) for r in build.LIBS}
_owner = {}   # entry point -> the bound Library that exports it


def _bind(d):
  if not os.path.exists(d.path):
    raise RuntimeError(
        f"{d.path} is missing: the HIP extension is not built. Run "
        "`python big_vision_amd/build.py`. There is no CPU/eager fallback.")
  dll = ctypes.CDLL(d.path)
  last_error = getattr(dll, d.last_error)
  last_error.restype = ctypes.c_char_p
  last_error.argtypes = []
  for name, argtypes in d.prototypes.items():
    fn = getattr(dll, name)  # AttributeError if the ABI drifted
    fn.restype = d.restypes.get(name, c_int)
    fn.argtypes = argtypes
  if getattr(dll, d.version_fn)() != d.version:
    raise RuntimeError(f"{d.name} ABI version mismatch")
  d.dll = dll
  _owner.update(dict.fromkeys(d.prototypes, d))


def load():
  """Binds every library of LIBRARIES (once) and returns libbvhip.so.  Raises if one is not built — no fallback."""
  for d in LIBRARIES.values():
    if d.dll is None:
      _bind(d)
  return LIBRARIES["hip"].dll


def handle(key):
  """The bound library of that key ("hip", "distill", "eval"), for calls that bypass `call`."""
  load()
  return LIBRARIES[key].dll


# Optional launch observer (bench.py installs one to bracket selected kernels
# with HIP events on the launch stream); None on the normal path.
observer = None


def call(name, *args):
  d = _owner.get(name)
  if d is None:
    load()
    d = _owner.get(name)
    if d is None:
      raise AttributeError(f"{name}: no library of _lib.LIBRARIES declares it")
  obs = observer
  tok = obs.begin(name, args) if obs is not None else None
  rc = getattr(d.dll, name)(*args)
  if tok is not None:
    obs.end(tok)
  if name in d.restypes:
    return rc
  if rc != 0:
    raise RuntimeError(f"{name} failed (rc={rc}): {getattr(d.dll, d.last_error)().decode()}")
