"""Host-side operator wrappers over the C ABI of libsnap_hip.so.

Every function validates dtype / device / contiguity, allocates the outputs with
torch (device memory plumbing only) and launches the HIP kernel on torch's
current stream.  There is no CPU or PyTorch fallback: tensors must live on a
ROCm device and the shared library must be built, otherwise these raise.
"""
import contextlib
import operator
import sys
import ctypes
import threading
import typing
import weakref
import os

import numpy as np
import torch

from snap_amd import _lib

# the header's constants (include/snap_hip.h, read by _lib) under the names the wrappers and their callers use
PRO_NONE, PRO_AFFINE, PRO_GN_RELU, PRO_RELU_GN, PRO_RELU = (
    _lib.SNAP_PRO_NONE, _lib.SNAP_PRO_AFFINE, _lib.SNAP_PRO_GN_RELU, _lib.SNAP_PRO_RELU_GN, _lib.SNAP_PRO_RELU)
EPI_BIAS, EPI_RELU, EPI_RESIDUAL, EPI_UPSAMPLE2X_ADD, EPI_ROWMASK, EPI_GELU = (
    _lib.SNAP_EPI_BIAS, _lib.SNAP_EPI_RELU, _lib.SNAP_EPI_RESIDUAL, _lib.SNAP_EPI_UPSAMPLE2X_ADD,
    _lib.SNAP_EPI_ROWMASK, _lib.SNAP_EPI_GELU)
POOLING = {'max': _lib.SNAP_POOL_MAX, 'sum': _lib.SNAP_POOL_SUM, 'mean': _lib.SNAP_POOL_MEAN}
SIM_CHUNK = _lib.SNAP_SIM_CHUNK



# ----------------------------------------------------------------------------------------------------
# Tuning: every tuning / test switch of the kernel wrappers in ONE object.  None of them is needed to
# run the models and none changes a result beyond summation order; tools and tests flip them to A/B
# kernels.  The object in force is per thread and scoped (``tuning_scope(...)`` /
# ``engine_scope(engine, tuning=...)``); outside any scope it is the process default, of which the
# module attributes of the same names (``ops.CONV_TILE = '64x64'``) are thin aliases -- reading
# ``ops.CONV_TILE`` anywhere gives the value in force in the calling thread.
#   OVERLAP_AERIAL     the aerial encoder on a second HIP stream next to the StreetView encoder
#   POOLED_SPLIT       the lift hands `pooled` to the fused MLP / pool kernel pre-split (LDS-DMA A operand)
#   CLASS_ROWS         ... classed by observation count (single-observation rows carry no variance slabs)
#   LIFT_IN_CONSUMER   ... and class-1 rows are never written: a 32-byte tap record, the four image taps
#                      blended inside the fused MLP / pool kernel (the lift inside the consumer)
#   MLP_GATHER_XCD_GROUP  runs of 128-row tiles of the gathered class per XCD (its L2 keeps their taps)
#   NATIVE_GLUE        image padding / voxel-centre grid as native passes instead of torch fill + copies
#   USE_PRESPLIT       bottleneck 3x3 / closing 1x1 convs read their input through gn_norm_split on the 'bf16x3'
#                      engine (off: measured at C2 -- tools/unit_bench.py, profiles/r03_unit_bench.json -- the pre-split
#                      convs are 10-25 percent faster, the extra pass costs what they gain; the engine's own user is
#                      the exhaustive voting)
#   CONV_TILE / CONV_BK / CONV_NO_HALO / CONV_NO_RS / CONV_RS_NSPLIT / CONV_RS_FORCE / CONV_NO_WS /
#   CONV_NO_PLAIN      forced tile ('128x128' | '128x64' | '64x128' | '64x64'; travels as SnapConvDesc.tile_hint),
#                      f32 K-slab depth (16 | 32), and which body a conv launch takes (tests pin every body against
#                      the others).  None / False / 0 = the engines' choice
#   SPLITK_STATS / USE_SPLITK / USE_FUSED_GN_STATS / GN_STATS_BOTH   GroupNorm statistics from the conv
#                      epilogues / split-K reduce passes vs the stand-alone kernels
#   USE_PRESPLIT_VOTING / FUSED_TEMPLATE_PACK / PS_RES_INIT / PS_TILE   pre-split GEMM engine (direct-form voting)
#   SIM_GENERAL_KERNEL  tests: pin the general similarity kernel (the full-chunk kernel is bit-identical)
#   LATTICE_WINDOW     the refinement lattice scored from one window per point (pose_score_window; same bits)
#   FUSE_STEM          inference, 'bf16x3' engine: the ResNet stem (7x7/2 root conv + 3x3/2 max-pool) as ONE launch that
#                      never writes the conv output (conv2d_root_pool; same bits as the two launches)
#   WGRAD_SIDE_STREAM  backward: a node's kernel-gradient launches run on the second HIP stream next to its
#                      data-gradient / GroupNorm-VJP chain and are joined before the node returns (same bits)
# ----------------------------------------------------------------------------------------------------
_TUNING_DEFAULTS = {
    'OVERLAP_AERIAL': True,
    'POOLED_SPLIT': True,
    'CLASS_ROWS': True,
    'LIFT_IN_CONSUMER': True,
    'MLP_GATHER_XCD_GROUP': 8,
    'NATIVE_GLUE': True,
    'USE_PRESPLIT': False,
    'CONV_TILE': None,
    'CONV_BK': None,
    'CONV_NO_HALO': False,
    'CONV_NO_RS': False,
    'CONV_RS_NSPLIT': 0,
    'CONV_RS_FORCE': False,
    'CONV_NO_WS': False,
    'SPLITK_STATS': True,
    'CONV_NO_PLAIN': False,
    'USE_PRESPLIT_VOTING': True,
    'PS_RES_INIT': True,
    'PS_TILE': 0,
    'BF16_PS': True,          # conv2d(bf16_ring=True) launches take the one-part pre-split engine (conv_ps.hip NS = 1); False: the x_half engine
    'USE_FUSED_GN_STATS': True,
    'GN_STATS_BOTH': True,
    'USE_SPLITK': True,
    'FUSED_TEMPLATE_PACK': True,
    'SIM_GENERAL_KERNEL': False,
    'LATTICE_WINDOW': True,
    'WGRAD_SIDE_STREAM': True,
    'FUSE_STEM': True,
}


class Tuning:
  """The switches listed above as one value object (``Tuning(CONV_TILE='64x64')``; unknown names raise)."""
  __slots__ = tuple(_TUNING_DEFAULTS)

  def __init__(self, **kw):
    for k, v in _TUNING_DEFAULTS.items():
      object.__setattr__(self, k, kw.pop(k, v))
    if kw:
      raise TypeError(f'Tuning: unknown switch(es) {sorted(kw)}')

  def replace(self, **kw):
    vals = {k: getattr(self, k) for k in _TUNING_DEFAULTS}
    for k in kw:
      if k not in vals:
        raise TypeError(f'Tuning: unknown switch {k!r}')
    vals.update(kw)
    return Tuning(**vals)

  def __repr__(self):
    diff = {k: getattr(self, k) for k, v in _TUNING_DEFAULTS.items() if getattr(self, k) != v}
    return 'Tuning(' + ', '.join(f'{k}={v!r}' for k, v in diff.items()) + ')'


_DEFAULT_TUNING = Tuning()
_TUNING_TLS = threading.local()


def tuning():
  """The ``Tuning`` in force in this thread: the innermost scope's, else the process default."""
  t = getattr(_TUNING_TLS, 'tuning', None)
  return _DEFAULT_TUNING if t is None else t


@contextlib.contextmanager
def tuning_scope(base=None, **overrides):
  """Run the enclosed ops under ``base`` (default: the tuning in force) with ``overrides`` applied.
  Per thread, re-entrant; autograd nodes carry it into the backward thread with the engine."""
  prev = getattr(_TUNING_TLS, 'tuning', None)
  _TUNING_TLS.tuning = (base if base is not None else tuning()).replace(**overrides)
  try:
    yield _TUNING_TLS.tuning
  finally:
    _TUNING_TLS.tuning = prev


# the raw handle of torch's current stream on the current device: one C call (torch.cuda.current_stream() builds a
# Stream object through three layers of device-index resolution: ~9 us per launch, 3-13 ms of a step's host time --
# a fifth of the C5 step's, which the host bounds)
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_raw_device = getattr(torch._C, '_cuda_getDevice', None)


def _stream():
  if _raw_stream is not None and _raw_device is not None:
    return ctypes.c_void_p(_raw_stream(_raw_device()))
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# A second HIP stream for work that does not depend on the main chain (the aerial encoder runs
# next to the StreetView encoder: its deep stages are launches of 19-73 workgroups on a 256-CU
# part).  ``Tuning.OVERLAP_AERIAL = False`` keeps everything on one stream.
_SIDE_STREAMS = {}


def side_stream(device=None):
  """The second stream of ``device`` (one per GPU of the process; default: the current device)."""
  idx = torch.cuda.current_device() if device is None else torch.device(device).index
  if idx is None:
    idx = torch.cuda.current_device()
  s = _SIDE_STREAMS.get(idx)
  if s is None:
    s = _SIDE_STREAMS[idx] = torch.cuda.Stream(device=idx)
  return s


class KernelProfiler:
  """HIP-event timing of individual kernel launches on torch's current stream.

  ``bench.py`` installs one for a single step of the timed region to obtain the
  per-kernel durations behind the ``roofline`` object (events are recorded on the
  stream the kernels are launched on).  ``flops`` / ``nbytes`` are the ALGORITHMIC
  figures of DESIGN.md, not measured traffic.
  """

  def __init__(self):
    self.records = {}

  def region(self, name, flops=0.0, nbytes=0.0, tag=None):
    return _Region(self, name, flops, nbytes, tag)

  def launches(self, name):
    """Per-launch (tag, ms, flops, bytes) of one kernel family (after a sync)."""
    torch.cuda.synchronize()
    return [
        (r[4], r[0].elapsed_time(r[1]), _num(r[2]), _num(r[3]))
        for r in self.records.get(name, [])
    ]

  def summary(self):
    torch.cuda.synchronize()
    out = {}
    for name, recs in self.records.items():
      ms = sum(r[0].elapsed_time(r[1]) for r in recs)
      out[name] = dict(
          launches=len(recs), ms=ms, flops=sum(_num(r[2]) for r in recs),
          bytes=sum(_num(r[3]) for r in recs),
      )
    return out


def _num(v):
  """flops / bytes may be callables resolved after the sync (device-side row counts)."""
  return float(v()) if callable(v) else v


class _Region:

  def __init__(self, prof, name, flops, nbytes, tag=None):
    self.prof, self.name, self.flops, self.nbytes, self.tag = prof, name, flops, nbytes, tag

  def __enter__(self):
    self.start = torch.cuda.Event(enable_timing=True)
    self.start.record()

  def __exit__(self, *exc):
    end = torch.cuda.Event(enable_timing=True)
    end.record()
    self.prof.records.setdefault(self.name, []).append(
        (self.start, end, self.flops, self.nbytes, self.tag)
    )


class _NoRegion:

  def __enter__(self):
    pass

  def __exit__(self, *exc):
    pass


_PROFILER = None
_NO_REGION = _NoRegion()


def set_profiler(prof):
  """Install (or remove with None) a KernelProfiler; returns the previous one."""
  global _PROFILER
  old, _PROFILER = _PROFILER, prof
  return old


def _region(name, flops=0.0, nbytes=0.0, tag=None):
  if _PROFILER is None:
    return _NO_REGION
  return _PROFILER.region(name, flops, nbytes, tag() if callable(tag) else tag)


def _p(t):
  if t is None:
    return None
  return ctypes.c_void_p(t.data_ptr())


def _pv(t):
  return None if t is None else t.data_ptr()


# Small host tables (per-launch item lists of the multi-tensor kernels) go to the device through a
# ring of PINNED staging buffers with a truly asynchronous copy: a pageable-source copy stalls the
# host until the runtime has staged it and leaves the GPU idle in front of the copy (~4 ms per
# training step over its 5-6 tables, rocprofv3 kernel trace).  A slot is reused only after the
# event recorded behind its last copy has completed.
_PIN_RING = []
_PIN_NEXT = 0


_PIN_LOCK = threading.Lock()


def upload_table(items, device):
  """numpy structured / plain array -> uint8 device tensor holding its bytes."""
  raw = np.ascontiguousarray(items).view(np.uint8).reshape(-1)
  device = torch.device(device)
  if device.type != 'cuda':
    return torch.from_numpy(raw.copy()).to(device)
  global _PIN_NEXT
  n = raw.size
  # one lock around slot selection, fill and the copy's issue: autograd hook / backward threads
  # (the overlapped gradient reducer) call this next to the main thread
  with _PIN_LOCK:
    if not _PIN_RING:          # the whole ring at once (a pinned allocation takes ~0.2 s: never inside a step)
      _PIN_RING.extend([torch.empty(1 << 17, dtype=torch.uint8, pin_memory=True), None] for _ in range(16))
    slot = _PIN_RING[_PIN_NEXT % 16]
    _PIN_NEXT += 1
    if slot[1] is not None:
      slot[1].synchronize()
    if slot[0].numel() < n:
      slot[0] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    slot[0][:n].numpy()[:] = raw
    out = slot[0][:n].to(device, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    slot[1] = ev
  return out


# exp(temperature) is a KERNEL ARGUMENT of the similarity / sampling kernels (a host scalar).  Reading
# it back where it is needed drains the stream in the middle of a step (everything after it is then
# dispatched into an empty queue: ~3 ms of launch-bound gaps per training step).  ``prefetch_exp``
# queues the 4-byte read at the START of the apply; ``host_exp`` then only waits for that copy.
_HOST_SCALARS = {}


def prefetch_exp(t):
  if t is None or not t.is_cuda:
    return
  # one pinned scalar per temperature tensor, reused apply after apply: a read-back still in
  # flight into it was consumed by ``host_exp`` -- or is superseded by this one -- once its event has passed
  prev = _HOST_SCALARS.get(id(t))
  if prev is not None and prev[0]() is t:
    host = prev[2]
    prev[3].synchronize()
  else:
    host = torch.empty(1, dtype=torch.float32, pin_memory=True)
  host.copy_(torch.exp(t.detach().to(torch.float32)).reshape(1), non_blocking=True)
  ev = torch.cuda.Event()
  ev.record()
  if len(_HOST_SCALARS) > 64:
    _HOST_SCALARS.clear()
  _HOST_SCALARS[id(t)] = (weakref.ref(t), t._version, host, ev)


def host_exp(t):
  """float(exp(t)) -- the prefetched value when ``prefetch_exp(t)`` ran for this version of ``t``
  (same torch kernel, same bits), else a blocking read."""
  hit = _HOST_SCALARS.get(id(t))
  if hit is not None and hit[0]() is t and hit[1] == t._version:
    hit[3].synchronize()
    return float(hit[2][0])
  return float(torch.exp(t.detach().to(torch.float32)))


def _chk(t, dtype, name):
  if not isinstance(t, torch.Tensor):
    raise TypeError(f'{name}: expected a torch.Tensor, got {type(t)}')
  if not t.is_cuda:
    raise RuntimeError(
        f'{name}: tensor is on {t.device}; snap_amd ops run only on a ROCm GPU '
        '(no CPU fallback).'
    )
  if t.dtype != dtype:
    raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
  if not t.is_contiguous():
    raise ValueError(f'{name}: tensor must be contiguous')
  return t


def _f32(t, name):
  return _chk(t, torch.float32, name)


def _mask(t, name):
  if t.dtype == torch.bool:
    return _chk(t, torch.bool, name)
  return _chk(t, torch.uint8, name)


def _arg_chk(t, name, dtypes, shape, device, want, also=True, tail=''):
  """Argument ``t`` is a tensor of one of ``dtypes`` and of ``shape`` (None: any extent) on ``device`` (None: any ROCm
  GPU), and ``also`` holds: else ValueError(f'{want}, got <what it is>{tail}').  Then the usual ``_chk``."""
  if (not isinstance(t, torch.Tensor) or t.dtype not in dtypes
      or (not t.is_cuda if device is None else t.device != device) or t.dim() != len(shape)
      or any(s is not None and s != d for s, d in zip(shape, t.shape)) or not also):
    got = f'{t.dtype} {tuple(t.shape)} on {t.device}' if isinstance(t, torch.Tensor) else type(t)
    raise ValueError(f'{want}, got {got}{tail}')
  return _chk(t, t.dtype, name)


def _workspace_words(nbytes_fn, args, numel, unsupported):
  """The workspace of one call in whole 8-byte words (the caller allocates them as int64: 8-byte aligned, and the
  allocation stays at the wrapper's own site): ``nbytes_fn(*args)`` bytes.  The C side is not asked where ``numel``
  does not fit its int32 arguments; 0 bytes is its refusal: ValueError(unsupported)."""
  nbytes = nbytes_fn(*args) if numel < 2 ** 31 else 0
  if nbytes == 0:
    raise ValueError(unsupported)
  return nbytes // 8


# ----------------------------------------------------------------------------
# encoder
# ----------------------------------------------------------------------------
class PreSplit:
  """An activation [N, H, W, C] (C % 16 == 0) already normalised and split into two bf16 parts:
  ``data`` = [N*H*W][C/16][hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15] (the bytes of the f32 tensor,
  re-arranged per 16-channel block).  ``conv2d`` multiplies it on the pre-split engine
  (conv_ps.hip: both operands by LDS-DMA, no normalise / split work in the K loop)."""

  def __init__(self, data, shape):
    self.data = data
    self.shape = tuple(shape)
    self.device = data.device

  def numel(self):
    return int(np.prod(self.shape))


def gn_norm_split(y, gamma, beta, *, groups=32, eps=1e-5, want_stats=False):
  """relu(GroupNorm(y)) of a conv output that carries its fused partial sums, written once in the
  pre-split format -> ``PreSplit`` (or None where the pre-split engine does not apply: another
  engine, no fused statistics, C % 16 != 0)."""
  fused = getattr(y, '_snap_gn_partial', None)
  N, H, W, C = y.shape
  if (precision() != 'bf16x3' or fused is None or fused[2] or groups != 32
      or C % 16 or C > 2048 or not tuning().USE_FUSED_GN_STATS):
    return None
  lib = _lib.load()
  _f32(y, 'y'); _f32(gamma, 'gamma'); _f32(beta, 'beta')
  partial, tile_rows, _ = fused
  out = torch.empty(y.numel() * 2, dtype=torch.bfloat16, device=y.device)
  mu = sc = None
  if want_stats:
    mu = torch.empty((N, C), dtype=torch.float32, device=y.device)
    sc = torch.empty((N, C), dtype=torch.float32, device=y.device)
  with _region('gn_norm_split', 0.0, 8.0 * y.numel()):
    st = lib.snap_gn_norm_split_f32(_p(y), _p(partial), N, H * W, C, groups, eps, tile_rows,
                                    _p(gamma), _p(beta), _p(out), _p(mu), _p(sc), _stream())
  _lib.check(st, 'snap_gn_norm_split_f32')
  ps = PreSplit(out, (N, H, W, C))
  if want_stats:
    ps.stats = (mu, sc)
  return ps


def presplit(x):
  """The plain two-part split of x [..., C] f32 (C % 16 == 0) -> ``PreSplit``."""
  lib = _lib.load()
  _f32(x, 'x')
  C = x.shape[-1]
  rows = x.numel() // C
  out = torch.empty(x.numel() * 2, dtype=torch.bfloat16, device=x.device)
  with _region('presplit', 0.0, 8.0 * x.numel()):
    st = lib.snap_presplit_f32(_p(x), rows, C, _p(out), _stream())
  _lib.check(st, 'snap_presplit_f32')
  shape = tuple(x.shape) if x.dim() == 4 else (1,) * (4 - x.dim()) + tuple(x.shape)
  return PreSplit(out, shape)


def _stationary_mode(T=None):
  """SnapConvDesc.tile_hint // 1 000 000: which 1x1 bodies of the split engine may run."""
  T = tuning() if T is None else T
  if T.CONV_NO_RS:
    return 1
  if T.CONV_RS_FORCE:
    return 4 if T.CONV_NO_WS else 2
  return 3 if T.CONV_NO_WS else 0


class PackedWeights:
  """A conv kernel that exists ONLY as the split engine's two-part weight image (``data``: bf16,
  the layout of snap_conv2d_pack_weights_split_bf16 for ``shape`` = (KH, KW, Cin, Cout)) -- e.g. the
  shift-stacked template bank of the exhaustive voting, written directly in that form by
  ``pack_stacked_templates_split``.  ``conv2d`` takes it with a ``PreSplit`` input."""

  def __init__(self, data, shape):
    self.data = data
    self.shape = tuple(int(v) for v in shape)

  def numel(self):
    return int(np.prod(self.shape))


def pack_stacked_templates_split(templates, S):
  """templates [R, H, W, D] -> ``PackedWeights`` of the shift-stacked bank [H+S-1, W+S-1, D, R S^2]
  (``stack_templates`` + ``pack_weights_split_bf16(., 2)`` in one pass; the f32 bank is never built)."""
  lib = _lib.load()
  _f32(templates, 'templates')
  R, H, W, D = templates.shape
  KH, KW, RS = H + S - 1, W + S - 1, R * S * S
  nbytes = lib.snap_conv2d_packed_weights_split_bytes(KH * KW, D, RS, 2)
  if nbytes == 0:
    return None
  out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=templates.device)
  with _region('pack_stacked_templates', 0.0, 4.0 * templates.numel() + float(nbytes)):
    st = lib.snap_pack_stacked_templates_split_bf16(_p(templates), H, W, D, R, S, _p(out), nbytes, _stream())
  _lib.check(st, 'snap_pack_stacked_templates_split_bf16')
  return PackedWeights(out, (KH, KW, D, RS))


# the training-precision engines: operands rounded to bf16 / IEEE half, f32 accumulate
HALF_MATH = ('bf16', 'fp16')
# the split-bf16 engines: bf16 parts per operand
SPLIT_PARTS = {'bf16x3': 2, 'bf16x6': 3}


def kernel_image(w_shape, math):
  """Which engine a [KH,KW,Cin,Cout] kernel's launches take under ``math`` and whether they read a
  packed weight image -> ``(math, parts, packed)``: a split image beyond the engine's 32-bit offsets
  (template banks) drops the kernel to 'f32'; 'f32' and Cin < 4 read the f32 kernel itself (the
  f32 engine).  ``parts`` is the split engines' number of bf16 parts (0: a bf16 / fp16 image).  The
  ONE statement of this rule: ``plan_conv`` and the functions that prepare the images ahead of the
  launches (``pack_weights_*_multi``, ``conv2d_presplit_supported``) all ask here."""
  KH, KW, Cin, Cout = w_shape
  parts = SPLIT_PARTS.get(math, 0)
  if parts and _lib.load().snap_conv2d_packed_weights_split_bytes(KH * KW, Cin, Cout, parts) == 0:
    math, parts = 'f32', 0
  return math, parts, math != 'f32' and Cin >= 4


def conv2d_presplit_supported(x_shape, w_shape, stride=1, padding=((0, 0), (0, 0))):
  """True when ``conv2d(presplit(x), w, ...)`` has an engine for the shape: the pre-split engine's
  own limits (``snap_conv2d_presplit_supported``) and a two-part weight image within the split
  engine's 32-bit offsets.  Callers with a plain-input alternative ask before they pre-split."""
  lib = _lib.load()
  N, H, W, Cs = x_shape
  KH, KW, Cin, Cout = w_shape
  (pt, pb), (pl, pr) = padding
  if Cs != Cin or Cin % 16:
    return False
  Ho = (H + pt + pb - KH) // stride + 1
  Wo = (W + pl + pr - KW) // stride + 1
  if Ho <= 0 or Wo <= 0:
    return False
  if kernel_image(w_shape, 'bf16x3')[1] != 2:
    return False
  d = _lib.SnapConvDesc(N, H, W, Cin, Cs, KH, KW, stride, pt, pl, Ho, Wo, Cout, Cout, PRO_NONE, 0, 1.0, 0.0)
  return bool(lib.snap_conv2d_presplit_supported(ctypes.byref(d)))


class ConvPlan(typing.NamedTuple):
  """Everything one ``conv2d`` launch decides before it touches a tensor (``plan_conv``)."""
  desc: _lib.SnapConvDesc   # the launch descriptor, tile_hint included (read-only: it is passed by reference)
  out_shape: tuple          # (N, Ho, Wo, Cout)
  out_dtype: torch.dtype    # float32; bfloat16 / float16 with out_half
  engine: str               # the arithmetic the launch runs on ('f32' where no weight image applies: ``kernel_image``)
  family: str               # profiler family: conv_igemm | conv_split_<math> | conv_bf16 | conv_fp16
  tag: str                  # profiler tag prefix: '' | 'PS_' | 'PS1_' | 'RS_' | 'WS_'
  image: str                # ``_packed_weights`` key of the weight image the kernel reads; None: the f32 kernel
  parts: int                # ... and its bf16 parts (0: a bf16 / fp16 image)
  extras: bool              # the launch passes a SnapConvExtras at all (else NULL)
  workspace_bytes: int      # split-K workspace (0: K is not split)
  stats_bytes: int          # ONE buffer of GroupNorm partial sums (0: none emitted)
  stats_count: int          # 0 | 1 | 2 (2: those of y and, as a request, of relu(y))
  stats_relu: bool          # the first buffer holds the sums of relu(y)
  gn_partial_rows: int      # 32: the split-K reduce pass emits them per 32-row slab; 0: the engine's own layout
  tile_rows: int            # rows per slab as the statistics' consumers read them (``_snap_gn_partial[1]``)
  gnb: bool                 # the buffer holds the statistics of the GroupNorm VJP (``gn_bwd_stats`` accepted)
  w_split_parts: int        # the scalar SnapConvExtras fields of the same names
  w_split_root: int
  w_half: int
  x_half: int
  x_presplit: int
  ps_tile: int
  ps_res_init: int
  bk_hint: int
  tune_flags: int


def plan_conv(
    x, w, stride=1, padding=((0, 0), (0, 0)), cin=None, prologue=PRO_NONE,
    gn=None, in_affine=(1.0, 0.0), bias=None, relu=False, residual=None,
    up_prev=None, row_mask=None, rows_in=None, rows_out=None, row_count=None, out=None,
    emit_gn_stats=None, math=None, gelu=False, res_init=None, ps_tile=None, out_half=False, out_stride=None,
    gn_bwd_stats=None, bf16_ring=False,
):
  """The ``ConvPlan`` of ``conv2d(x, w, ...)`` (same arguments) under the engine and ``Tuning`` in
  force.  Pure: of every tensor argument only ``shape`` / ``dtype`` / ``numel()`` are read (meta
  tensors, ``PreSplit`` / ``PackedWeights`` of meta tensors do), nothing is allocated or launched and
  no device is needed -- the library is asked only its host queries.  Raises every ``ValueError`` of
  ``conv2d`` that follows from shapes, dtypes and flags."""
  lib = _lib.load()
  T = tuning()
  ps = isinstance(x, PreSplit)
  pw = isinstance(w, PackedWeights)
  xh = (not ps) and x.dtype in (torch.bfloat16, torch.float16)
  no_rows = rows_in is None and rows_out is None and row_count is None
  if xh:
    # the input already in the training-precision engine's element type (the half twin a GroupNorm
    # VJP wrote next to its f32 gradient): both operands by LDS-DMA (conv_bf16.hip)
    want = 'fp16' if x.dtype == torch.float16 else 'bf16'
    math = want if math is None else math
    if (math != want or prologue != PRO_NONE or rows_in is not None or x.shape[-1] % 8 or w.shape[2] % 8
        or emit_gn_stats is not None):
      raise ValueError('conv2d: a half-precision input takes the matching engine, prologue NONE, whole '
                       'channel octets, no input row list / statistics')
  if ps:
    if prologue != PRO_NONE or not no_rows or math not in (None, 'bf16x3'):
      raise ValueError('conv2d: a PreSplit input takes prologue NONE, no row lists, math bf16x3')
    math = 'bf16x3'
  if pw and not ps:
    raise ValueError('conv2d: PackedWeights (a two-part split image) go with a PreSplit input')
  N, H, W, Cs = x.shape
  KH, KW, Cin, Cout = w.shape
  if cin is None:
    cin = Cs
  if cin != Cin:
    raise ValueError(f'conv2d: kernel expects Cin={Cin}, input has {cin}')
  (pt, pb), (pl, pr) = padding
  Ho = (H + pt + pb - KH) // stride + 1
  Wo = (W + pl + pr - KW) // stride + 1
  M = N * Ho * Wo
  out_dtype = torch.float32
  if out_half:
    hm = precision() if math is None else math
    if (hm not in HALF_MATH or out is not None or emit_gn_stats is not None or up_prev is not None
        or prologue not in (PRO_NONE, PRO_RELU) or Cs % 4 or Cin < 4 or Cout % 4):
      raise ValueError('conv2d: out_half needs a training-precision engine launch (prologue NONE / RELU, '
                       'no statistics / up-sampling epilogue, channel quads)')
    out_dtype = torch.float16 if hm == 'fp16' else torch.bfloat16
  elif out is not None:
    if out_stride is not None:
      if (out_stride % 4 or out_stride < Cout or out.numel() != M * out_stride or emit_gn_stats is not None
          or residual is not None or up_prev is not None):
        raise ValueError('conv2d: out_stride needs out [rows, out_stride], out_stride % 4 == 0, a plain epilogue')
    elif out.numel() != M * Cout:
      raise ValueError('conv2d: out has the wrong size')
  if out_stride is not None and out is None:
    raise ValueError('conv2d: out_stride goes with out')
  epi = 0
  if prologue in (PRO_GN_RELU, PRO_RELU_GN):
    mu, sc, beta = gn
    if mu.numel() != N * Cin or sc.numel() != N * Cin or beta.numel() != Cin:
      raise ValueError('conv2d: GroupNorm statistics have the wrong size')
  if bias is not None:
    epi |= EPI_BIAS
    if bias.numel() != Cout:
      raise ValueError('conv2d: bias size')
  if relu:
    epi |= EPI_RELU
  if gelu:                                   # tanh-approximated GELU (ViT MLP)
    epi |= EPI_GELU
  if residual is not None:
    epi |= EPI_RESIDUAL
    y_shape = (N, Ho, Wo, Cout) if out is None else tuple(out.shape)
    if tuple(residual.shape) != y_shape:
      raise ValueError(f'conv2d: residual {tuple(residual.shape)} vs {y_shape}')
  if up_prev is not None:
    epi |= EPI_UPSAMPLE2X_ADD
    if tuple(up_prev.shape) != (N, Ho // 2, Wo // 2, Cout):
      raise ValueError('conv2d: up_prev shape')
  if row_mask is not None:
    epi |= EPI_ROWMASK
    if row_mask.numel() != M:
      raise ValueError('conv2d: row_mask size')
  tile_hint = 1000000 * _stationary_mode(T)
  if T.CONV_TILE:
    bm, bn = (int(v) for v in T.CONV_TILE.split('x'))
    tile_hint += bm * 1000 + bn
  d = _lib.SnapConvDesc(
      N, H, W, Cin, Cs, KH, KW, stride, pt, pl, Ho, Wo, Cout, Cout if out_stride is None else int(out_stride), prologue,
      epi, float(in_affine[0]), float(in_affine[1]), tile_hint,
  )
  dref = ctypes.byref(d)
  # the engine the launch will take (the statistics layout depends on it)
  math = precision() if math is None else math
  if math not in ENGINES:
    raise ValueError(f'conv2d: math={math!r}')
  math, parts, packed = kernel_image((KH, KW, Cin, Cout), math)
  packed = packed and Cs % 4 == 0
  qparts = parts if packed and not ps else 0   # (SnapConvExtras.w_split_parts of a plain-input launch)
  # a bf16 input whose launch needs nothing but the GEMM + a plain epilogue runs on the ONE-PART pre-split engine
  # (conv_ps.hip, NS = 1: both operands by LDS-DMA through the three-stage ring, 256 x 128 tiles) -- the same
  # arithmetic as the training-precision engine (operands rounded to bf16, f32 accumulate)
  ps1 = bool(bf16_ring and xh and x.dtype == torch.bfloat16 and math == 'bf16' and T.BF16_PS and Cs == Cin and Cin % 16 == 0
             and rows_out is None and row_count is None and up_prev is None and gn_bwd_stats is None
             and out is None and Cout % 4 == 0 and lib.snap_conv2d_presplit_supported(dref))
  if xh and out_half and not ps1:
    raise ValueError('conv2d: a half-precision input AND output need the one-part pre-split engine (bf16, Cin % 16 == 0, '
                     'no row lists)')
  # a stationary-operand 1 x 1 / 3 x 3 kernel of the two-part engine (1: RS, 2 / 3: WS) takes the launch
  kind = lib.snap_conv2d_stationary_kind(dref, qparts) if (qparts == 2 and no_rows) else 0
  pst = (T.PS_TILE if ps_tile is None else int(ps_tile)) if (ps or ps1) else 0
  wbytes = sbytes = scount = rows32 = tile_rows = 0
  gnb = False
  if no_rows:
    if ps:
      wbytes = lib.snap_conv2d_presplit_workspace_bytes(dref, pst) if T.USE_SPLITK else 0
    elif not (ps1 or kind or out_half):          # (the stationary kernels and the one-part engine never split K)
      wbytes = lib.snap_conv2d_workspace_bytes(dref) if T.USE_SPLITK else 0
    if wbytes:   # small-M / deep-K layer: split K
      half_engine = math in HALF_MATH and packed and Cin % 4 == 0 and not ps
      if emit_gn_stats is not None and (qparts >= 2 or half_engine) and T.SPLITK_STATS:
        # the reduce pass of the split / bf16 / fp16 engine emits the partial sums (per 32-row slab)
        sbytes = lib.snap_conv2d_splitk_gn_partial_bytes(dref)
        if sbytes:
          scount, rows32, tile_rows = 1, 32, 32
    elif (gn_bwd_stats is not None and xh and emit_gn_stats is None and out is None and up_prev is None
          and not relu and not gelu and row_mask is None):
      gx, gmu, grs, gga, gbe, gmode = gn_bwd_stats
      pbytes = lib.snap_conv2d_gn_partial_bytes_ex(dref, 0)
      if (pbytes and tuple(gx.shape) == (N, Ho, Wo, Cout) and gmu.numel() == N * Cout and grs.numel() == N * Cout
          and gga.numel() == Cout and gbe.numel() == Cout and gmode in (PRO_GN_RELU, PRO_RELU_GN)):
        sbytes, scount, gnb = pbytes, 1, True
        tile_rows = lib.snap_conv2d_tile_rows_ex(dref, 0)
    elif emit_gn_stats is not None:
      sbytes = (lib.snap_conv2d_presplit_gn_partial_bytes(dref, pst) if ps
                else lib.snap_conv2d_gn_partial_bytes_ex(dref, qparts))
      if sbytes:
        # 'both' on a split engine: the statistics of y AND of relu(y), a request (SnapConvExtras.gn_partial2_done)
        scount = 2 if (emit_gn_stats == 'both' and math in SPLIT_PARTS) else 1
        tile_rows = lib.snap_conv2d_presplit_tile_rows(dref, pst) if ps else lib.snap_conv2d_tile_rows_ex(dref, qparts)
  if ps and (parts != 2 or Cin % 16):
    raise ValueError('conv2d: the pre-split engine needs Cin % 16 == 0 and a two-part weight image')
  family, image, iparts = 'conv_igemm', None, 0
  root = xpre = res0 = 0
  if (parts and (KH, KW, stride, Cin, Cs) == (7, 7, 2, 3, 4) and (pt, pl) == (3, 3)
      and prologue in (PRO_NONE, PRO_AFFINE) and no_rows and not sbytes and not ps):
    # the RGB root convolution (7 x 7 / stride 2 / pad 3) of an image stored with 4 floats per pixel
    # runs on the split engine with its own weight image (a K slab = 4 pixels of a kernel row)
    family, image, iparts, root = f'conv_split_{math}', math + '/root', parts, 1
  elif ps1:
    family, image, iparts, xpre = 'conv_bf16', 'bf16/ps1', 1, 1
  elif packed:
    family = f'conv_split_{math}' if parts else ('conv_fp16' if math == 'fp16' else 'conv_bf16')
    image, iparts = math, parts
    if ps:
      xpre, res0 = 1, int(T.PS_RES_INIT if res_init is None else bool(res_init))
  bk_hint = tune_flags = 0
  tuned = bool(T.CONV_BK or T.CONV_NO_HALO or T.CONV_RS_NSPLIT or T.CONV_NO_PLAIN)
  if tuned:
    bk_hint = int(T.CONV_BK or 0)
    tune_flags = (_lib.SNAP_TUNE_NO_HALO * int(bool(T.CONV_NO_HALO)) | _lib.SNAP_TUNE_NO_PLAIN * int(bool(T.CONV_NO_PLAIN))
                  | ((int(T.CONV_RS_NSPLIT) & 15) << _lib.SNAP_TUNE_RS_NSPLIT_SHIFT))
  return ConvPlan(
      desc=d, out_shape=(N, Ho, Wo, Cout), out_dtype=out_dtype, engine=math if image else 'f32', family=family,
      tag='PS_' if ps else 'PS1_' if ps1 else ('', 'RS_', 'WS_', 'WS_')[kind], image=image, parts=iparts,
      extras=bool(not no_rows or wbytes or sbytes or image or tuned), workspace_bytes=wbytes,
      stats_bytes=sbytes, stats_count=scount, stats_relu=bool(sbytes) and emit_gn_stats == 'relu',
      gn_partial_rows=rows32, tile_rows=tile_rows, gnb=gnb,
      w_split_parts=iparts, w_split_root=root, w_half=int(image == 'fp16'), x_half=int(xh and not ps1),
      x_presplit=xpre, ps_tile=pst if xpre else 0, ps_res_init=res0, bk_hint=bk_hint, tune_flags=tune_flags)


def conv2d(
    x, w, *, stride=1, padding=((0, 0), (0, 0)), cin=None, prologue=PRO_NONE,
    gn=None, in_affine=(1.0, 0.0), bias=None, relu=False, residual=None,
    up_prev=None, row_mask=None, rows_in=None, rows_out=None, row_count=None, out=None,
    emit_gn_stats=None, math=None, gelu=False, res_init=None, ps_tile=None, out_half=False, out_stride=None,
    gn_bwd_stats=None, bf16_ring=False,
):
  """NHWC implicit-GEMM conv on the matrix cores.  x [N,H,W,Cs]; w [KH,KW,Cin,Cout] (HWIO).

  x may be a ``PreSplit`` (``gn_norm_split`` / ``presplit``): the launch then runs on the
  pre-split engine -- 'bf16x3' arithmetic, prologue NONE, no row lists; ``res_init`` (default
  ``PS_RES_INIT``) loads ``residual`` into the accumulators before the K loop, ``ps_tile``
  (default ``PS_TILE``) forces a row tile.

  math = 'f32' (exact f32 MFMA) | 'bf16x6' / 'bf16x3' (f32-grade split-bf16 engine: every
  operand split into 3 / 2 bf16 parts after the f32 prologue, 6 / 3 part products accumulated in
  f32 -- ~2^-24 / ~2^-17 relative error per product) | 'bf16' (operands rounded to bf16, f32
  accumulate: the training-precision engine); None = ``MATMUL_PRECISION``.

  gn = (mu [N,Cin], sc [N,Cin], beta [Cin]) for PRO_GN_RELU / PRO_RELU_GN.
  rows_in / rows_out (int32 [M]) + row_count (int32 [1], device): row-indexed launch
  over a compacted row list (see ``compact_rows``); ``out`` supplies the destination.
  emit_gn_stats = 'raw' | 'relu' | 'both': the epilogue also emits the partial sums from which
  ``group_norm_stats(y, ...)`` (same ``relu_first``) builds its result without re-reading
  y; they travel as ``y._snap_gn_partial`` ('both' = 'raw' plus, where the engine has the kernel
  variant -- split-bf16, GroupNorm -> ReLU prologue, 128 x 128 tiles --, those of relu(y) as
  ``y._snap_gn_partial_relu``).  Ignored where the shape does not allow it.
  out_half (training-precision engines 'bf16' / 'fp16' only): the result is written ONLY rounded to the
  engine's element type and returned as a bf16 / f16 tensor (the hidden activations and inter-layer
  gradients of the masked MLP: every consumer rounds them to that type anyway).
  gn_bwd_stats = (x_gn, mu, rstd, gamma, beta, mode) (a half-precision input -- the data-gradient launch that
  reads a GroupNorm VJP's twin): the epilogue also emits the statistics of the GroupNorm VJP that consumes THIS
  result as its incoming gradient (x_gn [N,Ho,Wo,Cout] is that GroupNorm's input, mode its prologue);
  ``ops_bwd.group_norm_bwd`` finds them on the result (``y._snap_gnb_partial``) and skips its first pass.
  Silently not done where the launch splits K or the shape has no statistics layout.
  bf16_ring (a bf16 input, math 'bf16', Cin % 16 == 0, no row lists / statistics / split-K): the launch runs on the
  ONE-PART pre-split engine (conv_ps.hip, NS = 1: both operands by LDS-DMA through the three-stage ring, 256 x 128
  tiles) -- the arithmetic of the training-precision engine (1 x 1: the same bits), 500-730 instead of 350-560
  TFLOP/s on large dense layers; it never splits K, so small-M / deep-K launches (the training step's) stay where
  they are: opt-in per call (the ViT encoder's inference path).  ``Tuning.BF16_PS = False`` turns it off.
  out_stride (with ``out``, a multiple of 4 >= Cout): out's rows hold out_stride floats and the result goes
  to their first Cout (the other columns are not touched); no statistics, residual or up-sampling epilogue.
  Returns y [N,Ho,Wo,Cout] (``out`` itself, [.., out_stride], with out_stride).
  """
  lib = _lib.load()
  ps = isinstance(x, PreSplit)
  pw = isinstance(w, PackedWeights)
  # the tensors: device, dtype, contiguity (what the plan cannot see); the plan checks shapes and flags
  if ps:
    xd = _chk(x.data, torch.bfloat16, 'x')
  else:
    xd = _chk(x, x.dtype if x.dtype in (torch.bfloat16, torch.float16) else torch.float32, 'x')
  wd = w.data if pw else _f32(w, 'w')   # (the pre-split engine reads only the image; this passes a non-NULL pointer)
  if out is not None:
    _f32(out, 'out')
  for t, nm in ((rows_in, 'rows_in'), (rows_out, 'rows_out'), (row_count, 'row_count')):
    if t is not None:
      _chk(t, torch.int32, nm)
  mu = sc = beta = None
  if prologue in (PRO_GN_RELU, PRO_RELU_GN):
    mu, sc, beta = gn
    _f32(mu, 'gn_mu'); _f32(sc, 'gn_sc'); _f32(beta, 'gn_beta')
  if bias is not None:
    _f32(bias, 'bias')
  if residual is not None:
    _f32(residual, 'residual')
  if up_prev is not None:
    _f32(up_prev, 'up_prev')
  if row_mask is not None:
    _mask(row_mask, 'row_mask')
  # (positional, in the order of the two signatures: this call is on every launch's host path)
  p = plan_conv(x, w, stride, padding, cin, prologue, gn, in_affine, bias, relu, residual, up_prev, row_mask, rows_in,
                rows_out, row_count, out, emit_gn_stats, math, gelu, res_init, ps_tile, out_half, out_stride,
                gn_bwd_stats, bf16_ring)
  # what the plan says: the result, split-K workspace, statistics buffers, weight image
  dev = xd.device
  y = out if out is not None else torch.empty(p.out_shape, dtype=p.out_dtype, device=dev)
  kws = torch.empty(p.workspace_bytes // 4, dtype=torch.float32, device=dev) if p.workspace_bytes else None
  partial = torch.empty(p.stats_bytes // 4, dtype=torch.float32, device=dev) if p.stats_count else None
  partial2 = torch.empty(p.stats_bytes // 4, dtype=torch.float32, device=dev) if p.stats_count == 2 else None
  wpk = None
  if p.image is not None:
    wpk = wd if pw else _packed_weights(w, p.image, p.parts)
  ex = None
  if p.extras:
    ex = _lib.SnapConvExtras()
    if rows_in is not None or rows_out is not None or row_count is not None:
      ex.rows_in, ex.rows_out, ex.row_count = _pv(rows_in), _pv(rows_out), _pv(row_count)
    if kws is not None:
      ex.workspace, ex.workspace_bytes = kws.data_ptr(), p.workspace_bytes
    if partial is not None:
      ex.gn_partial, ex.gn_partial_bytes = partial.data_ptr(), p.stats_bytes
      ex.gn_partial_relu, ex.gn_partial_rows = int(p.stats_relu), p.gn_partial_rows
    if partial2 is not None:
      ex.gn_partial2, ex.gn_partial2_bytes = partial2.data_ptr(), p.stats_bytes
    if p.gnb:
      for t, nm in zip(gn_bwd_stats[:5], ('gn_bwd x', 'gn_bwd mu', 'gn_bwd rstd', 'gn_bwd gamma', 'gn_bwd beta')):
        _f32(t, nm)
      ex.gnb_x, ex.gnb_mu, ex.gnb_rstd, ex.gnb_gamma, ex.gnb_beta = (t.data_ptr() for t in gn_bwd_stats[:5])
      ex.gnb_mode = int(gn_bwd_stats[5])
    if wpk is not None:
      ex.w_bf16, ex.w_bf16_bytes = wpk.data_ptr(), wpk.numel() * 2
      ex.w_split_parts, ex.w_split_root, ex.w_half, ex.x_half = p.w_split_parts, p.w_split_root, p.w_half, p.x_half
      ex.x_presplit, ex.ps_tile, ex.ps_res_init = p.x_presplit, p.ps_tile, p.ps_res_init
      if out_half:
        ex.y_half = y.data_ptr()
    ex.bk_hint, ex.tune_flags = p.bk_hint, p.tune_flags
  N, Ho, Wo, Cout = p.out_shape
  KH, KW, Cin = w.shape[:3]
  M = N * Ho * Wo
  kflops = 2.0 * KH * KW * Cin * Cout
  if row_count is None:
    flops = kflops * M
    nbytes = 4.0 * ((x.numel() if ps else x.numel() * (0.5 if p.x_half or p.image == 'bf16/ps1' else 1.0)) + w.numel() + y.numel()
                    + (residual.numel() if residual is not None else 0))
  else:  # resolved after the sync: only the listed rows are multiplied / moved
    flops = lambda: kflops * int(row_count.item())
    nbytes = lambda: 4.0 * (int(row_count.item()) * (Cin + Cout) + wd.numel())
  with _region(
      p.family, flops, nbytes,
      lambda: f'{p.tag}M{M}{"r" if row_count is not None else ""}_K{KH}x{KW}x{Cin}_N{Cout}_s{stride}_p{prologue}_e{p.desc.epilogue}',
  ):
    st = lib.snap_conv2d_nhwc_ex_f32(
        ctypes.byref(p.desc), _p(xd), _p(wd), None if out_half else _p(y), _p(mu), _p(sc), _p(beta), _p(bias),
        _p(residual), _p(up_prev), _p(row_mask), None if ex is None else ctypes.byref(ex),
        _stream(),
    )
  _lib.check(st, 'snap_conv2d_nhwc_ex_f32')
  if p.gnb:
    # (the GroupNorm VJP checks that it is handed the same x before it trusts these sums)
    y._snap_gnb_partial = (partial, p.tile_rows, gn_bwd_stats[0].data_ptr(), gn_bwd_stats[0]._version, int(gn_bwd_stats[5]))
  elif partial is not None:
    y._snap_gn_partial = (partial, p.tile_rows, p.stats_relu)
    if partial2 is not None and ex.gn_partial2_done:
      y._snap_gn_partial_relu = (partial2, p.tile_rows, True)
  return y


def _root_pool_plan(x, w, cin, prologue, in_affine, relu, math):
  """The ``ConvPlan`` of the root convolution where the stem runs as one launch, else None."""
  if not tuning().FUSE_STEM or isinstance(x, PreSplit) or isinstance(w, PackedWeights):
    return None
  p = plan_conv(x, w, 2, ((3, 3), (3, 3)), cin, prologue, None, in_affine, None, relu, math=math)
  ok = p.w_split_root and _lib.load().snap_conv2d_root_pool_supported(ctypes.byref(p.desc), p.parts)
  return p if ok else None


def conv2d_root_pool_supported(x, w, *, cin=None, prologue=PRO_NONE, in_affine=(1.0, 0.0), relu=False, math=None):
  """Whether ``conv2d_root_pool`` (same arguments) runs as one launch; else it is ``conv2d`` -> ``max_pool_3x3s2``.
  Pure, like ``plan_conv``."""
  return _root_pool_plan(x, w, cin, prologue, in_affine, relu, math) is not None


def conv2d_root_pool(x, w, *, cin=None, prologue=PRO_NONE, in_affine=(1.0, 0.0), relu=False, math=None, band_rows=0):
  """The ResNet stem: ``max_pool_3x3s2(conv2d(x, w, stride=2, padding=((3, 3), (3, 3)), ...))`` for a 7 x 7 root
  kernel over an image stored with 4 floats per pixel -- in ONE launch that never writes the conv output, where the
  library supports the shape (two-part split engine, 64 output channels, ``Tuning.FUSE_STEM``); as those two
  launches everywhere else.  Bit-identical either way.  ``band_rows``: tests (pooled rows per wave; 0 = automatic).
  """
  p = _root_pool_plan(x, w, cin, prologue, in_affine, relu, math)
  if p is None:
    return max_pool_3x3s2(conv2d(x, w, stride=2, padding=((3, 3), (3, 3)), cin=cin, prologue=prologue,
                                 in_affine=in_affine, relu=relu, math=math))
  lib = _lib.load()
  xd = _f32(x, 'x')
  _f32(w, 'w')
  wpk = _packed_weights(w, p.image, p.parts)
  N, Ho, Wo, Cout = p.out_shape
  y = torch.empty((N, (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1, Cout), dtype=torch.float32, device=xd.device)
  with _region(p.family, 2.0 * 147 * Cout * N * Ho * Wo, 4.0 * (x.numel() + w.numel() + y.numel()),
               lambda: f'POOL_M{N * Ho * Wo}_K7x7x3_N{Cout}_s2_p{prologue}_e{p.desc.epilogue}'):
    st = lib.snap_conv2d_root_pool_f32(ctypes.byref(p.desc), _p(xd), _p(wpk), wpk.numel() * 2, p.parts, int(band_rows),
                                       _p(y), _stream())
  _lib.check(st, 'snap_conv2d_root_pool_f32')
  return y


def pack_weights_bf16(w, half=False):
  """w [KH,KW,Cin,Cout] f32 -> the training-precision engine's weight image
  [Cout][KH*KW][roundup(Cin,8)] in bf16, or (half) IEEE float16 -- math 'fp16'."""
  lib = _lib.load()
  _f32(w, 'w')
  KH, KW, Cin, Cout = w.shape
  nbytes = lib.snap_conv2d_packed_weights_bytes(KH * KW, Cin, Cout)
  out = torch.empty(nbytes // 2, dtype=torch.float16 if half else torch.bfloat16, device=w.device)
  fn = lib.snap_conv2d_pack_weights_f16 if half else lib.snap_conv2d_pack_weights_bf16
  st = fn(_p(w), KH * KW, Cin, Cout, _p(out), nbytes, _stream())
  _lib.check(st, 'snap_conv2d_pack_weights_f16' if half else 'snap_conv2d_pack_weights_bf16')
  return out


# Bumped by every ``ForwardContext`` (= every ``apply``): the bf16 weight images are prepared
# once per apply and tensor (the map and query passes of one apply share them), never carried
# from one apply / timed step to the next -- like the StdConv standardisation.
PACK_EPOCH = 0


def _image_get(w, key, explicit=False):
  """The image remembered on ``w`` under ``key`` (``w._snap_packed``: key -> image) if it still
  holds -- packed in the current ``PACK_EPOCH``, tensor not modified in place since --, else None.
  ``explicit``: a bare image stored under the key by hand (tools) is returned as it is."""
  slot = getattr(w, '_snap_packed', None)
  hit = None if slot is None else slot.get(key)
  if isinstance(hit, tuple):
    return hit[2] if hit[0] == PACK_EPOCH and hit[1] == w._version else None
  return hit if explicit else None


def _image_put(w, key, image):
  slot = getattr(w, '_snap_packed', None)
  if slot is None:
    slot = w._snap_packed = {}
  slot[key] = (PACK_EPOCH, w._version, image)


def _packed_weights(w, math, parts):
  """The engine's weight image of ``w`` for this apply: an explicit ``w._snap_packed[math]``
  (tools) wins; otherwise packed at first use and remembered on the tensor (``_image_get``)."""
  wpk = _image_get(w, math, explicit=True)
  if wpk is None:
    if math.endswith('/root'):
      wpk = pack_weights_split_root_bf16(w, parts)
    else:
      wpk = pack_weights_split_bf16(w, parts) if parts else pack_weights_bf16(w, half=(math == 'fp16'))
    try:
      _image_put(w, math, wpk)
    except AttributeError:
      pass
  return wpk


def pack_weights_split_bf16(w, parts):
  """w [KH,KW,Cin,Cout] f32 -> the split engine's image [parts][Cout][KH*KW][roundup(Cin,8)]
  (part 0 = bf16(w), part p = bf16 of the exact f32 residual of parts < p)."""
  lib = _lib.load()
  _f32(w, 'w')
  KH, KW, Cin, Cout = w.shape
  nbytes = lib.snap_conv2d_packed_weights_split_bytes(KH * KW, Cin, Cout, parts)
  out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w.device)
  st = lib.snap_conv2d_pack_weights_split_bf16(_p(w), KH * KW, Cin, Cout, parts, _p(out), nbytes,
                                               _stream())
  _lib.check(st, 'snap_conv2d_pack_weights_split_bf16')
  return out


def pack_weights_split_root_bf16(w, parts):
  """w [7,7,3,Cout] f32 -> the split engine's ROOT image ([Cout/128][14 slabs = (kh, group of 4
  kw)][parts][128][16 k = 4 kw x (RGB + 0)])."""
  lib = _lib.load()
  _f32(w, 'w')
  if tuple(w.shape[:3]) != (7, 7, 3):
    raise ValueError('pack_weights_split_root_bf16: w must be [7, 7, 3, Cout]')
  Cout = w.shape[3]
  nbytes = lib.snap_conv2d_packed_weights_split_root_bytes(Cout, parts)
  out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w.device)
  st = lib.snap_conv2d_pack_weights_split_root_bf16(_p(w), Cout, parts, _p(out), nbytes, _stream())
  _lib.check(st, 'snap_conv2d_pack_weights_split_root_bf16')
  return out


_PACK_ITEM = np.dtype(_lib.SnapPackItem)


def pack_weights_split_multi(ws, math):
  """Prepare the split engine's weight image of every kernel in ``ws`` (HWIO tensors) with ONE
  launch and remember it on the tensors for the current apply (see ``_packed_weights``)."""
  parts = SPLIT_PARTS[math]
  lib = _lib.load()
  # (kernels that run on the f32 engine get no image: ``kernel_image``)
  todo = [w for w in ws if _image_get(w, math) is None and kernel_image(w.shape, math)[2]]
  if not todo:
    return
  items = np.zeros(len(todo), dtype=_PACK_ITEM)
  outs = []
  blk = 0
  for i, w in enumerate(todo):
    _f32(w, 'w')
    KH, KW, Cin, Cout = w.shape
    nbytes = lib.snap_conv2d_packed_weights_split_bytes(KH * KW, Cin, Cout, parts)
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w.device)
    outs.append(out)
    items[i] = (w.data_ptr(), out.data_ptr(), KH * KW, Cin, Cout, blk)
    blk += lib.snap_conv2d_pack_weights_split_blocks(KH * KW, Cin, Cout)
  table = upload_table(items, todo[0].device)
  st = lib.snap_conv2d_pack_weights_split_multi_bf16(_p(table), len(todo), blk, parts, _stream())
  _lib.check(st, 'snap_conv2d_pack_weights_split_multi_bf16')
  for w, out in zip(todo, outs):
    _image_put(w, math, out)


def pack_weights_bf16_multi(ws, with_rotated=True, math='bf16'):
  """Training precision (math 'bf16' | 'fp16'): the engine's image of every kernel in ``ws`` (HWIO
  tensors) -- and, for the data-gradient convolutions, of its rotated transpose -- with ONE launch;
  remembered on the tensors for the current apply (``_packed_weights`` / ``packed_rot_image``)."""
  lib = _lib.load()
  if math not in HALF_MATH:
    raise ValueError(f'pack_weights_bf16_multi: math={math!r}')
  half = math == 'fp16'
  todo = [w for w in ws if _image_get(w, math) is None and kernel_image(w.shape, math)[2]]
  if not todo:
    return
  n = len(todo) * (2 if with_rotated else 1)
  items = np.zeros(n, dtype=_PACK_ITEM)
  outs = []
  blk = 0
  i = 0
  for w in todo:
    _f32(w, 'w')
    KH, KW, Cin, Cout = w.shape
    taps = KH * KW
    for rot in ((False, True) if with_rotated else (False,)):
      nbytes = (lib.snap_conv2d_packed_weights_bytes(taps, Cout, (Cin + 3) // 4 * 4) if rot
                else lib.snap_conv2d_packed_weights_bytes(taps, Cin, Cout))
      out = torch.empty(nbytes // 2, dtype=torch.float16 if half else torch.bfloat16, device=w.device)
      outs.append(out)
      items[i] = (w.data_ptr(), out.data_ptr(), -taps if rot else taps, Cin, Cout, blk)
      blk += lib.snap_conv2d_pack_weights_blocks(-taps if rot else taps, Cin, Cout)
      i += 1
  table = upload_table(items, todo[0].device)
  fn = lib.snap_conv2d_pack_weights_multi_f16 if half else lib.snap_conv2d_pack_weights_multi_bf16
  st = fn(_p(table), n, blk, _stream())
  _lib.check(st, 'snap_conv2d_pack_weights_multi_f16' if half else 'snap_conv2d_pack_weights_multi_bf16')
  k = 0
  for w in todo:
    _image_put(w, math, outs[k]); k += 1
    if with_rotated:
      _image_put(w, math + '/rot', outs[k]); k += 1


def packed_rot_image(w, math='bf16'):
  """The rotated image ``pack_weights_bf16_multi`` prepared for ``w`` in this apply, or None."""
  return _image_get(w, math + '/rot')


def dense(x, kernel, bias=None, *, cin=None, prologue=PRO_NONE, relu=False,
          row_mask=None, rows_in=None, rows_out=None, row_count=None, out=None, math=None,
          gelu=False, residual=None, out_half=False, out_stride=None, bf16_ring=False):
  """x [..., Cs] @ kernel [Cin, Cout] (+bias) through the conv engine (1x1).  out_stride: ``conv2d``."""
  lead = x.shape[:-1]
  M = int(np.prod(lead)) if len(lead) else 1
  strided = out_stride is not None     # (``out`` [rows, out_stride] goes through as it is and is the result)
  y = conv2d(
      x.reshape(1, 1, M, x.shape[-1]), kernel.reshape(1, 1, *kernel.shape),
      cin=cin if cin is not None else kernel.shape[0], prologue=prologue,
      bias=bias, relu=relu, row_mask=row_mask, rows_in=rows_in, rows_out=rows_out,
      row_count=row_count, out=out if (strided or out is None) else out.reshape(1, 1, M, kernel.shape[1]),
      math=math, gelu=gelu, out_stride=out_stride,
      residual=None if residual is None else residual.reshape(1, 1, M, kernel.shape[1]),
      out_half=out_half, bf16_ring=bf16_ring,
  )
  return out if strided else y.reshape(*lead, kernel.shape[1])


def semantic_embed(rasters, idx_road, idx_other, table_road, table_other):
  """rasters [..., N] bool -> [..., (1 + len(idx_other)) * E] (semantic_raster_encoder.py:63-79)."""
  lib = _lib.load()
  _mask(rasters, 'rasters'); _f32(table_road, 'table_road'); _f32(table_other, 'table_other')
  N = rasters.shape[-1]
  M = rasters.numel() // N
  E = table_road.shape[1]
  nr, no = len(idx_road), len(idx_other)
  if tuple(table_road.shape) != (nr, E) or tuple(table_other.shape) != (2 * no, E):
    raise ValueError('semantic_embed: table shapes')
  ir = (ctypes.c_int32 * max(nr, 1))(*idx_road)
  io = (ctypes.c_int32 * max(no, 1))(*idx_other)
  out = torch.empty((*rasters.shape[:-1], (1 + no) * E), dtype=torch.float32, device=rasters.device)
  st = lib.snap_semantic_embed_f32(_p(rasters), M, N, ctypes.cast(ir, ctypes.c_void_p), nr,
                                   ctypes.cast(io, ctypes.c_void_p), no, _p(table_road),
                                   _p(table_other), E, _p(out), _stream())
  _lib.check(st, 'snap_semantic_embed_f32')
  return out


def semantic_onehot(rasters, idx_road, idx_other):
  """[M, KP] one-hot matrix of the embedding rows each pixel reads (KP = roundup(nr + 2 no, 4))."""
  lib = _lib.load()
  _mask(rasters, 'rasters')
  N = rasters.shape[-1]
  M = rasters.numel() // N
  nr, no = len(idx_road), len(idx_other)
  KP = (nr + 2 * no + 3) // 4 * 4
  ir = (ctypes.c_int32 * max(nr, 1))(*idx_road)
  io = (ctypes.c_int32 * max(no, 1))(*idx_other)
  onehot = torch.empty((M, KP), dtype=torch.float32, device=rasters.device)
  st = lib.snap_semantic_onehot_f32(_p(rasters), M, N, ctypes.cast(ir, ctypes.c_void_p), nr,
                                    ctypes.cast(io, ctypes.c_void_p), no, _p(onehot), KP, _stream())
  _lib.check(st, 'snap_semantic_onehot_f32')
  return onehot


def stack_templates(tw, S, layout='hwdr'):
  """tw [H, W, D, R] (layout 'hwdr') or templates [R, H, W, D] ('rhwd') -> shift-stacked filter
  bank [H+S-1, W+S-1, D, R*S*S] (see snap_hip.h)."""
  lib = _lib.load()
  _f32(tw, 'tw')
  if layout == 'hwdr':
    H, W, D, R = tw.shape
    fn, name = lib.snap_stack_templates_f32, 'snap_stack_templates_f32'
  else:
    R, H, W, D = tw.shape
    fn, name = lib.snap_stack_templates_rhwd_f32, 'snap_stack_templates_rhwd_f32'
  tws = torch.empty((H + S - 1, W + S - 1, D, R * S * S), dtype=torch.float32, device=tw.device)
  st = fn(_p(tw), _p(tws), H, W, D, R, S, _stream())
  _lib.check(st, name)
  return tws


def layer_norm(x, gamma, beta, eps=1e-6, out_half=False):
  """LayerNorm over the last axis (flax.linen.LayerNorm: biased variance, eps inside the sqrt).
  out_half: the result ONLY rounded to bf16 (the operand of a 'bf16' dense layer, which rounds it anyway)."""
  lib = _lib.load()
  _f32(x, 'x'); _f32(gamma, 'gamma'); _f32(beta, 'beta')
  C = x.shape[-1]
  M = x.numel() // C
  if out_half:
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    with _region('layer_norm', 0.0, 6.0 * x.numel()):
      st = lib.snap_layer_norm_bf16out_f32(_p(x), _p(gamma), _p(beta), _p(y), M, C, float(eps), _stream())
    _lib.check(st, 'snap_layer_norm_bf16out_f32')
    return y
  y = torch.empty_like(x)
  with _region('layer_norm', 0.0, 8.0 * x.numel()):
    st = lib.snap_layer_norm_f32(_p(x), _p(gamma), _p(beta), _p(y), M, C, float(eps), _stream())
  _lib.check(st, 'snap_layer_norm_f32')
  return y


def attention(qkv, scale=None, want_lse=False, out_half=False):
  """Multi-head self-attention on the bf16 matrix cores.  qkv [B, N, 3, H, 64] (fused QKV
  projection output, f32) -> [B, N, H*64] f32 = softmax(scale * Q K^T) V per head.
  want_lse: also return the base-2 log-sum-exp of the scaled scores [B, H, N] (for the VJP).
  out_half (inference): the result ONLY rounded to bf16 (the operand of the 'bf16' output projection)."""
  lib = _lib.load()
  B, N, three, H, D = qkv.shape
  if three != 3:
    raise ValueError('attention: qkv must be [B, N, 3, H, D]')
  scale = D ** -0.5 if scale is None else float(scale)
  if qkv.dtype == torch.bfloat16:
    # the QKV projection's bf16-only output: K / V move at half the bytes (inference; the result in bf16 too)
    if want_lse or not out_half:
      raise ValueError('attention: a bf16 qkv is the inference form (out_half=True, no lse)')
    _chk(qkv, torch.bfloat16, 'qkv')
    out = torch.empty((B, N, H * D), dtype=torch.bfloat16, device=qkv.device)
    with _region('attention', 4.0 * B * H * N * N * D, 2.0 * (qkv.numel() + out.numel())):
      st = lib.snap_attention_bf16io(_p(qkv), _p(out), B, N, H, D, scale, _stream())
    _lib.check(st, 'snap_attention_bf16io')
    return out
  _f32(qkv, 'qkv')
  if out_half:
    if want_lse:
      raise ValueError('attention: out_half is the inference form (no lse)')
    out = torch.empty((B, N, H * D), dtype=torch.bfloat16, device=qkv.device)
    with _region('attention', 4.0 * B * H * N * N * D, 4.0 * qkv.numel() + 2.0 * out.numel()):
      st = lib.snap_attention_bf16out_f32(_p(qkv), _p(out), B, N, H, D, scale, _stream())
    _lib.check(st, 'snap_attention_bf16out_f32')
    return out
  out = torch.empty((B, N, H * D), dtype=torch.float32, device=qkv.device)
  lse = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device) if want_lse else None
  with _region('attention', 4.0 * B * H * N * N * D, 4.0 * (qkv.numel() + out.numel())):
    st = lib.snap_attention_lse_bf16_f32(_p(qkv), _p(out), _p(lse), B, N, H, D, scale, _stream())
  _lib.check(st, 'snap_attention_lse_bf16_f32')
  return (out, lse) if want_lse else out


def gelu(x):
  """tanh-form GELU as a stand-alone kernel (training path: the pre-activation is kept)."""
  lib = _lib.load()
  _f32(x, 'x')
  y = torch.empty_like(x)
  with _region('gelu', 0.0, 8.0 * x.numel()):
    st = lib.snap_gelu_f32(_p(x), _p(y), x.numel(), _stream())
  _lib.check(st, 'snap_gelu_f32')
  return y


def compact_rows(mask, lo=1, hi=255):
  """mask [...] (bool/uint8) -> (index int32 [M] -- first `count` entries valid, ascending --
  and count int32 [1]) of the rows with lo <= mask <= hi (default: mask != 0); everything stays
  on the device."""
  lib = _lib.load()
  _mask(mask, 'mask')
  M = mask.numel()
  wsb = lib.snap_compact_rows_workspace_bytes(M)
  ws = torch.empty(wsb // 4, dtype=torch.int32, device=mask.device)
  index = torch.empty(M, dtype=torch.int32, device=mask.device)
  count = torch.empty(1, dtype=torch.int32, device=mask.device)
  st = lib.snap_compact_rows_range_u8(_p(mask), M, int(lo), int(hi), _p(index), _p(count), _p(ws),
                                      ws.numel() * 4, _stream())
  _lib.check(st, 'snap_compact_rows_range_u8')
  return index, count


def mlp2_pool_supported(cin, hidden, out_dim):
  """Shapes the fused fusion-MLP + vertical-max-pool kernel takes (mlp_pool.hip)."""
  return hidden % 32 == 0 and hidden <= 256 and out_dim % 4 == 0 and out_dim <= 128 and cin >= 4


def mlp2_pool_max(x, row_mask, w0, b0, w1, b1, *, cin, Z, relu_in=False, x_split=False,
                  zero_slabs=None, gather=None):
  """Fusion MLP (Dense -> relu -> Dense) over the rows with row_mask != 0 + max over the Z
  levels of every column, in one kernel on the bf16x3 engine (streetview_encoder.py:279-286 +
  bev_mapper.py:78-88).  x [M, Cs] (M = columns * Z, level fastest), row_mask [M];
  w0 [cin, H], w1 [H, D] -> plane [M / Z, D] f32, pvalid [M / Z] bool.  The hidden activations
  and the [M, D] volume are never written.  ``x_split``: x holds the rows pre-split
  (``lift_pool(out_split=True)``: [16-channel slab][hi | lo][16] bf16 in an f32 container); same
  bits, the kernel's A operand then travels by LDS-DMA.  ``zero_slabs`` = (first, count):
  row_mask is a CLASS per row (uint8, ``lift_pool(class_rows=True)``): rows of class 1 are exactly
  zero over those 16-channel slabs (and did not write them), rows of class >= 2 are complete --
  two row lists into one plane, the zero slabs of the first neither read nor multiplied; the same
  plane bit for bit.  ``gather`` = (f_images [B,V,h,w,C], records [B,N,8]) from
  ``lift_pool(tap_records=True)``: the class-1 rows do not exist in x -- the kernel blends their four
  image taps per GEMM0 slab from the records (the lift inside the consumer); the same plane bit for bit."""
  lib = _lib.load()
  _f32(x, 'x'); _mask(row_mask, 'row_mask')
  for t, n in ((w0, 'w0'), (b0, 'b0'), (w1, 'w1'), (b1, 'b1')):
    _f32(t, n)
  M, Cs = x.shape
  H, D = w1.shape
  if M % Z != 0 or row_mask.numel() != M or tuple(w0.shape) != (cin, H):
    raise ValueError('mlp2_pool_max: shapes')
  if not mlp2_pool_supported(cin, H, D):
    raise ValueError(f'mlp2_pool_max: unsupported widths {cin} -> {H} -> {D}')
  if zero_slabs is None:
    index, count = compact_rows(row_mask)
    index_z = count_z = None
    zlo = zn = 0
  else:
    if row_mask.dtype != torch.uint8:
      raise ValueError('mlp2_pool_max: zero_slabs needs the uint8 row classes')
    zlo, zn = int(zero_slabs[0]), int(zero_slabs[1])
    index, count = compact_rows(row_mask, 2, 255)
    index_z, count_z = compact_rows(row_mask, 1, 1)
  w0p = pack_weights_split_bf16(w0.reshape(1, 1, cin, H), 2)
  w1p = pack_weights_split_bf16(w1.reshape(1, 1, H, D), 2)
  ncols = M // Z
  plane = torch.empty(ncols, D, dtype=torch.float32, device=x.device)
  pvalid = torch.empty(ncols, dtype=torch.bool, device=x.device)
  kflops = 2.0 * (cin * H + H * D)
  kflops_z = 2.0 * ((cin - 16 * zn) * H + H * D)

  def rows_():
    return int(count.item()), (int(count_z.item()) if count_z is not None else 0)

  if gather is not None:
    f_img, recs = gather
    _f32(f_img, 'f_images')
    fd = (cin - 1) // 2
    if (zero_slabs is None or not x_split or relu_in or recs.dtype != torch.int32 or recs.numel() != M * 8
        or (zlo, zn) != (fd // 16, fd // 16) or fd % 16 or cin != 2 * fd + 1):
      raise ValueError('mlp2_pool_max: gather needs classed pre-split rows of mean | var | score and [M, 8] records')
    with _region('mlp2_pool_bf16x3', lambda: kflops * rows_()[0] + kflops_z * rows_()[1],
                 lambda: 4.0 * (rows_()[0] * cin + rows_()[1] * 8 + plane.numel()),
                 lambda: f'M{M}r_K{cin}_H{H}_N{D}_Z{Z}_gather'):
      st = lib.snap_mlp2_pool_max_gather_f32(
          _p(x), M, cin, Cs, _p(index), _p(count), _p(index_z), _p(count_z), _p(f_img), f_img.numel() * 4,
          f_img.shape[-2], f_img.shape[-1], fd, _p(recs), int(tuning().MLP_GATHER_XCD_GROUP), _p(w0p), w0p.numel() * 2,
          _p(b0), H, _p(w1p), w1p.numel() * 2, _p(b1), D, Z, ncols, _p(plane), _p(pvalid), _stream())
    _lib.check(st, 'snap_mlp2_pool_max_gather_f32')
    return plane, pvalid
  with _region('mlp2_pool_bf16x3', lambda: kflops * rows_()[0] + kflops_z * rows_()[1],
               lambda: 4.0 * (rows_()[0] * cin + rows_()[1] * (cin - 16 * zn) + plane.numel()),
               lambda: f'M{M}r_K{cin}_H{H}_N{D}_Z{Z}'):
    st = lib.snap_mlp2_pool_max_classes_f32(
        _p(x), M, cin, Cs, _p(index), _p(count), _p(index_z) if index_z is not None else None,
        _p(count_z) if count_z is not None else None, zlo, zn, _p(w0p), w0p.numel() * 2, _p(b0), H,
        _p(w1p), w1p.numel() * 2, _p(b1), D, int(relu_in), 1 if x_split else 0, Z, ncols, _p(plane),
        _p(pvalid), _stream())
  _lib.check(st, 'snap_mlp2_pool_max_classes_f32')
  return plane, pvalid


def fill_masked_rows_(y, mask, value=0.0):
  """In place: y[m, :] = value where mask[m] == 0.  y [..., C]."""
  lib = _lib.load()
  _f32(y, 'y'); _mask(mask, 'mask')
  C = y.shape[-1]
  M = y.numel() // C
  if mask.numel() != M:
    raise ValueError('fill_masked_rows_: mask size')
  st = lib.snap_fill_masked_rows_f32(_p(y), _p(mask), M, C, float(value), _stream())
  _lib.check(st, 'snap_fill_masked_rows_f32')
  return y


def weight_standardize(w, eps=1e-10):
  """StdConv kernel standardisation.  w [KH,KW,Cin,Cout] -> same shape."""
  lib = _lib.load()
  _f32(w, 'w')
  out = torch.empty_like(w)
  K = w.shape[0] * w.shape[1] * w.shape[2]
  with _region('weight_standardize', 0.0, 16.0 * w.numel()):
    st = lib.snap_weight_standardize_f32(_p(w), _p(out), K, w.shape[3], eps, _stream())
  _lib.check(st, 'snap_weight_standardize_f32')
  return out


_WSTD_ITEM = np.dtype(_lib.SnapWstdItem)


def _wstd_table(ws, dwss, outs, cols=32):
  """cols: output columns per workgroup of the kernel the table is for."""
  items = np.zeros(len(ws), dtype=_WSTD_ITEM)
  blk = 0
  for i, w in enumerate(ws):
    _f32(w, 'w'); _f32(outs[i], 'out')
    K = w.shape[0] * w.shape[1] * w.shape[2]
    items[i] = (w.data_ptr(), 0 if dwss is None else _f32(dwss[i], 'dws').data_ptr(),
                outs[i].data_ptr(), K, w.shape[3], blk, 0)
    blk += (w.shape[3] + cols - 1) // cols
  table = upload_table(items, ws[0].device)
  return table, blk


def weight_standardize_multi(ws, eps=1e-10):
  """``weight_standardize`` of a list of HWIO kernels in ONE launch."""
  lib = _lib.load()
  outs = [torch.empty_like(w) for w in ws]
  table, blocks = _wstd_table(ws, None, outs, cols=32)
  with _region('weight_standardize', 0.0, 16.0 * sum(w.numel() for w in ws)):
    st = lib.snap_weight_standardize_multi_f32(_p(table), len(ws), blocks, eps, _stream())
  _lib.check(st, 'snap_weight_standardize_multi_f32')
  return outs


def weight_standardize_bwd_multi(ws, dwss, eps=1e-10):
  """d w for a list of kernels given d standardise(w), ONE launch."""
  lib = _lib.load()
  outs = [torch.empty_like(w) for w in ws]
  table, blocks = _wstd_table(ws, dwss, outs)
  st = lib.snap_weight_standardize_bwd_multi_f32(_p(table), len(ws), blocks, eps, _stream())
  _lib.check(st, 'snap_weight_standardize_bwd_multi_f32')
  return outs


# the last unit of a ResNet stage emits the statistics of relu(y) too (its FPN level reads them)
# The arithmetic of every conv / dense ("engine"):
#   'f32'    the exact f32 matrix-core path (inference, parity);
#   'bf16x3' / 'bf16x6'  f32-grade: 2 / 3 bf16 parts per operand, f32 accumulate (conv_split.hip);
#   'bf16' / 'fp16'      operands rounded to the half type, f32 accumulate -- the reference's
#                        dtype='float16' train config (train_localization.py:93, trainer.py:387-397).
# The engine is a property of the MODEL (``BaseModel(config, meta, dtype, engine=...)``: dtype selects
# it exactly as the reference's ``model_cls(config.model, meta, dtype)`` does): every apply and the
# train step enter ``engine_scope(model.engine)``, a per-thread scope that the autograd nodes carry
# into the backward thread (autograd._engine_scoped).  MATMUL_PRECISION is only the PROCESS DEFAULT
# for calls outside any scope (direct ``ops.conv2d`` calls of tools and kernel tests).
MATMUL_PRECISION = 'f32'
ENGINES = ('f32', 'bf16', 'fp16', 'bf16x3', 'bf16x6')
_ENGINE_TLS = threading.local()


def precision():
  """The engine in force: the innermost ``engine_scope`` of this thread, else the process default."""
  e = getattr(_ENGINE_TLS, 'engine', None)
  return MATMUL_PRECISION if e is None else e


@contextlib.contextmanager
def engine_scope(engine, tuning=None):
  """Run the enclosed ops on ``engine`` (None: no change) and, if given, under the ``Tuning`` object
  ``tuning``.  Per thread, re-entrant; two models of different precision interleave freely in one process."""
  if tuning is not None:
    with tuning_scope(tuning):
      with engine_scope(engine):
        yield
    return
  if engine is None:
    yield
    return
  if engine not in ENGINES:
    raise ValueError(f'engine {engine!r}: expected one of {ENGINES}')
  prev = getattr(_ENGINE_TLS, 'engine', None)
  _ENGINE_TLS.engine = engine
  try:
    yield
  finally:
    _ENGINE_TLS.engine = prev


def engine_of_dtype(dtype):
  """reference ``dtype`` -> engine: float32 -> the process default's f32-class engine ('f32' unless
  the default is itself 'bf16x3' / 'bf16x6'), float16 -> 'fp16', bfloat16 -> 'bf16'."""
  if dtype in (torch.float16, 'float16', 'fp16'):
    return 'fp16'
  if dtype in (torch.bfloat16, 'bfloat16', 'bf16'):
    return 'bf16'
  if dtype in (torch.float32, 'float32', 'f32', None):
    return None                      # f32 class: the process default (exact f32 unless configured)
  raise ValueError(f'dtype {dtype!r}: expected float32 | float16 | bfloat16')


def group_norm_stats(x, gamma, *, groups=32, eps=1e-5, relu_first=False, want_rstd=False):
  """x [N,H,W,C] -> (mu [N,C], sc [N,C]) with sc = rstd * gamma (+ rstd [N,C])."""
  lib = _lib.load()
  _f32(x, 'x'); _f32(gamma, 'gamma')
  N, H, W, C = x.shape
  HW = H * W
  wsb = lib.snap_group_norm_stats_workspace_bytes(N, HW, C, groups)
  ws = torch.empty(wsb // 4, dtype=torch.float32, device=x.device)
  mu = torch.empty((N, C), dtype=torch.float32, device=x.device)
  sc = torch.empty((N, C), dtype=torch.float32, device=x.device)
  rstd = torch.empty((N, C), dtype=torch.float32, device=x.device) if want_rstd else None
  fused = getattr(x, '_snap_gn_partial', None)
  if fused is not None and fused[2] != bool(relu_first):
    fused = getattr(x, '_snap_gn_partial_relu', None) if relu_first else None
  if fused is not None and fused[2] == bool(relu_first) and groups == 32 and tuning().USE_FUSED_GN_STATS:
    partial, tile_rows, relu = fused     # emitted by the conv that produced x (which the kernel re-reads only
    with _region('group_norm_stats', 0.0, 4.0 * partial.numel()):   # for groups with mean^2 > 4 var)
      st = lib.snap_group_norm_stats_from_partial_f32(
          _p(partial), _p(x), N, HW, C, groups, eps, tile_rows, int(relu), _p(gamma), _p(mu), _p(sc), _p(rstd),
          _stream(),
      )
    _lib.check(st, 'snap_group_norm_stats_from_partial_f32')
    return (mu, sc, rstd) if want_rstd else (mu, sc)
  with _region('group_norm_stats', 0.0, 8.0 * x.numel()):
    st = lib.snap_group_norm_stats_f32(
        _p(x), N, HW, C, C, groups, eps, int(relu_first), _p(gamma), _p(mu),
        _p(sc), _p(rstd), _p(ws), ws.numel() * 4, _stream(),
    )
  _lib.check(st, 'snap_group_norm_stats_f32')
  if want_rstd:
    return mu, sc, rstd
  return mu, sc


def group_norm_apply(x, mu, sc, beta, mode):
  lib = _lib.load()
  _f32(x, 'x'); _f32(mu, 'mu'); _f32(sc, 'sc'); _f32(beta, 'beta')
  N, H, W, C = x.shape
  y = torch.empty_like(x)
  st = lib.snap_group_norm_apply_f32(
      _p(x), _p(y), N, H * W, C, _p(mu), _p(sc), _p(beta), mode, _stream()
  )
  _lib.check(st, 'snap_group_norm_apply_f32')
  return y


def pad_image(x, pad_h, pad_w, pad_c=0, out=None):
  """x [..., H, W, C] -> [..., H + pad_h, W + pad_w, C + pad_c], zeros at the bottom / right / in
  the extra channels, one pass (pad_to_multiple, image_encoder.py:32-39).  ``out``: a contiguous tensor
  of that shape to write into (a slice of a joint batch: several image sets padded side by side without
  concatenating them first)."""
  lib = _lib.load()
  _f32(x, 'x')
  *lead, H, W, C = x.shape
  N = int(np.prod(lead)) if lead else 1
  shape = (*lead, H + pad_h, W + pad_w, C + pad_c)
  if out is None:
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
  else:
    y = _f32(out, 'out')
    if tuple(y.shape) != tuple(shape):
      raise ValueError(f'pad_image: out {tuple(y.shape)} != {tuple(shape)}')
  st = lib.snap_pad_image_f32(_p(x), N, H, W, C, int(pad_h), int(pad_w), int(pad_c), _p(y), _stream())
  _lib.check(st, 'snap_pad_image_f32')
  return y


def voxel_points(xy, z):
  """xy [X, Y, 2] or [B, X, Y, 2] (BEV cell centres), z [B, Z] (level heights per scene) ->
  [B, X, Y, Z, 3] voxel centres (bev_mapper.py:162-196), one pass."""
  lib = _lib.load()
  _f32(xy, 'xy'); _f32(z, 'z')
  B, Z = z.shape
  X, Y = xy.shape[-3:-1]
  batched = xy.dim() == 4
  if xy.shape[-1] != 2 or (batched and xy.shape[0] != B):
    raise ValueError('voxel_points: shapes')
  out = torch.empty((B, X, Y, Z, 3), dtype=torch.float32, device=z.device)
  st = lib.snap_voxel_points_f32(_p(xy), int(batched), _p(z), B, X * Y, Z, _p(out), _stream())
  _lib.check(st, 'snap_voxel_points_f32')
  return out


def max_pool_3x3s2(x):
  lib = _lib.load()
  _f32(x, 'x')
  N, H, W, C = x.shape
  Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
  y = torch.empty((N, Ho, Wo, C), dtype=torch.float32, device=x.device)
  st = lib.snap_max_pool_3x3s2_f32(_p(x), _p(y), N, H, W, C, _stream())
  _lib.check(st, 'snap_max_pool_3x3s2_f32')
  return y


# ----------------------------------------------------------------------------
# lift
# ----------------------------------------------------------------------------
def pooled_channels(feature_dim, weighted=True, use_variance=True, add_minmax=False):
  """Channels of the pooled statistics: mean | var? | max, min? | score_max?
  (pool_multiview_features, streetview_encoder.py:141-178)."""
  return feature_dim * (1 + int(use_variance) + 2 * int(add_minmax)) + int(weighted)


def pooled_stride(feature_dim, weighted=True, use_variance=True, add_minmax=False):
  return (pooled_channels(feature_dim, weighted, use_variance, add_minmax) + 3) // 4 * 4


def lift_pool(f_images, cam, Rt, points, *, K, fisheye, feature_dim, num_bins,
              depth_min_max, max_view_distance=None, weighted=True, use_variance=True,
              add_minmax=False, grid_yz=None, valid_rows_only=False, out_split=False,
              class_rows=False, tap_records=False):
  """Fused k1-k5.  f_images [B,V,h,w,C]; cam [B,V,11]; Rt [B,V,12]; points [B,N,3].

  K = 0 selects all views.  Returns pooled [B,N,stride] (mean|var|score_max|pad by default;
  see ``pooled_channels`` for the other fusion options), valid [B,N] bool.
  ``grid_yz`` = (Y, Z): the points are the voxel centres of an [X, Y, Z] grid, level fastest --
  a traversal hint (8 x 8 column blocks per XCD), the results do not depend on it.
  ``valid_rows_only``: rows of voxels no view sees are left unwritten (uninitialised memory) --
  only for consumers that read the rows of valid voxels.  ``out_split``: rows are written
  pre-split for the split-bf16 engines ([16-channel slab][hi | lo][16] bf16, returned in an f32
  container of 16 * slabs floats per row) -- ``mlp2_pool_max(x_split=True)`` takes them.
  ``class_rows`` (with out_split): a third result, classes [B,N] uint8 = 0 invalid / 1 one visible
  observation / 2 several, and rows of class 1 do not write their (all-zero) variance slabs --
  ``mlp2_pool_max(zero_slabs=(fd / 16, fd / 16))`` takes the classes as its row mask.
  ``tap_records`` (with class_rows, out_split, valid_rows_only): a fourth result, records [B,N,8] int32;
  a class-1 voxel writes NO row but its four-tap record (byte offset | flags | wi1 | wj1 | depth score) --
  ``mlp2_pool_max(gather=(f_images, records))`` blends the taps inside the MLP kernel (the lift inside
  the consumer): those rows never exist in memory.
  """
  lib = _lib.load()
  _f32(f_images, 'f_images'); _f32(cam, 'cam'); _f32(Rt, 'Rt'); _f32(points, 'points')
  B, V, h, w, C = f_images.shape
  N = points.shape[1]
  stride = pooled_stride(feature_dim, weighted, use_variance, add_minmax)
  if out_split:
    stride = (pooled_channels(feature_dim, weighted, use_variance, add_minmax) + 15) // 16 * 16
  pooled = torch.empty((B, N, stride), dtype=torch.float32, device=f_images.device)
  valid = torch.empty((B, N), dtype=torch.uint8 if class_rows else torch.bool, device=f_images.device)
  d = _lib.SnapLiftDesc(
      B, V, h, w, C, feature_dim, num_bins if weighted else 0, N, K, int(fisheye), stride,
      float(depth_min_max[0]), float(depth_min_max[1]),
      -1.0 if max_view_distance is None else float(max_view_distance),
      int(weighted), int(use_variance), int(add_minmax),
  )
  if grid_yz is not None and N % (int(grid_yz[0]) * int(grid_yz[1])) == 0:
    d.grid_y, d.grid_z = int(grid_yz[0]), int(grid_yz[1])
  d.valid_rows_only = int(bool(valid_rows_only))
  d.out_split = int(bool(out_split))
  d.class_rows = int(bool(class_rows))
  recs = None
  if tap_records:
    if not (class_rows and out_split and valid_rows_only):
      raise ValueError('lift_pool: tap_records needs class_rows, out_split and valid_rows_only')
    recs = torch.empty((B, N, 8), dtype=torch.int32, device=f_images.device)
  with _region(
      'lift_pool', 0.0, 4.0 * (f_images.numel() + points.numel() + pooled.numel())
  ):
    if recs is not None:
      st = lib.snap_lift_pool_records_f32(
          ctypes.byref(d), _p(f_images), _p(cam), _p(Rt), _p(points), _p(pooled),
          _p(valid), _p(recs), _stream(),
      )
    else:
      st = lib.snap_lift_pool_f32(
          ctypes.byref(d), _p(f_images), _p(cam), _p(Rt), _p(points), _p(pooled),
          _p(valid), _stream(),
      )
  _lib.check(st, 'snap_lift_pool_records_f32' if recs is not None else 'snap_lift_pool_f32')
  if recs is not None:
    return pooled, valid != 0, valid, recs
  if class_rows:
    return pooled, valid != 0, valid
  return pooled, valid


def _obs_desc(f_shape, N, K, fisheye, feature_dim, max_view_distance, use_variance, add_minmax, stride):
  B, V, h, w, C = f_shape
  return _lib.SnapLiftDesc(
      B, V, h, w, C, feature_dim, 0, N, K, int(fisheye), stride, 1.0, 2.0,
      -1.0 if max_view_distance is None else float(max_view_distance),
      0, int(use_variance), int(add_minmax))


def lift_observations(f_images, cam, Rt, points, *, K, fisheye, feature_dim, max_view_distance=None):
  """First pass of the depth_mlp fusion (streetview_encoder.py:263-267): per-observation features,
  un-pooled.  f_images [B,V,h,w,fd] -> obs [B,N,S,fd+4] (features | log10 depth | unit ray),
  obs_feat [B,N,S,fd], valid [B,N]; S = K (top-K order) or V."""
  lib = _lib.load()
  _f32(f_images, 'f_images'); _f32(cam, 'cam'); _f32(Rt, 'Rt'); _f32(points, 'points')
  B, V, h, w, C = f_images.shape
  if C != feature_dim:
    raise ValueError('lift_observations: f_images must carry feature_dim channels')
  N = points.shape[1]
  S = K if K else V
  obs = torch.empty((B, N, S, feature_dim + 4), dtype=torch.float32, device=f_images.device)
  feat = torch.empty((B, N, S, feature_dim), dtype=torch.float32, device=f_images.device)
  valid = torch.empty((B, N), dtype=torch.bool, device=f_images.device)
  d = _obs_desc(f_images.shape, N, K, fisheye, feature_dim, max_view_distance, True, False, 0)
  with _region('lift_pool', 0.0, 4.0 * (f_images.numel() + obs.numel() + feat.numel())):
    st = lib.snap_lift_observations_f32(ctypes.byref(d), _p(f_images), _p(cam), _p(Rt), _p(points),
                                        _p(obs), _p(feat), _p(valid), _stream())
  _lib.check(st, 'snap_lift_observations_f32')
  return obs, feat, valid


def lift_pool_observations(obs_feat, f_shape, cam, Rt, points, *, K, fisheye, feature_dim,
                           max_view_distance=None, use_variance=True, add_minmax=False):
  """Second pass: pool_multiview_features(obs_feat, visible, None, add_minmax, use_variance)
  (streetview_encoder.py:141-178) -> pooled [B,N,stride], valid [B,N]."""
  lib = _lib.load()
  _f32(obs_feat, 'obs_feat'); _f32(cam, 'cam'); _f32(Rt, 'Rt'); _f32(points, 'points')
  B, N = points.shape[:2]
  stride = pooled_stride(feature_dim, False, use_variance, add_minmax)
  pooled = torch.empty((B, N, stride), dtype=torch.float32, device=obs_feat.device)
  valid = torch.empty((B, N), dtype=torch.bool, device=obs_feat.device)
  d = _obs_desc(f_shape, N, K, fisheye, feature_dim, max_view_distance, use_variance, add_minmax, stride)
  with _region('lift_pool', 0.0, 4.0 * (obs_feat.numel() + pooled.numel())):
    st = lib.snap_lift_pool_observations_f32(ctypes.byref(d), _p(cam), _p(Rt), _p(points),
                                             _p(obs_feat), _p(pooled), _p(valid), _stream())
  _lib.check(st, 'snap_lift_pool_observations_f32')
  return pooled, valid


def project_points(cam, Rt, points, fisheye):
  lib = _lib.load()
  _f32(cam, 'cam'); _f32(Rt, 'Rt'); _f32(points, 'points')
  B, V = cam.shape[:2]
  N = points.shape[1]
  dev = cam.device
  p2d = torch.empty((B, N, V, 2), dtype=torch.float32, device=dev)
  vis = torch.empty((B, N, V), dtype=torch.bool, device=dev)
  depth = torch.empty((B, N, V), dtype=torch.float32, device=dev)
  st = lib.snap_project_points_f32(
      B, V, N, int(fisheye), _p(cam), _p(Rt), _p(points), _p(p2d), _p(vis),
      _p(depth), _stream(),
  )
  _lib.check(st, 'snap_project_points_f32')
  return p2d, vis, depth


# ----------------------------------------------------------------------------
# BEV
# ----------------------------------------------------------------------------
def vertical_pool(vol, valid, pooling='max', want_arg=False):
  """vol [..., Z, D], valid [..., Z] -> plane [..., D], pvalid [...].  want_arg (max pooling, Z <= 64, D <= 128):
  also (argz, ties) [..., D] uint8 -- the level of every maximum and how many levels hold it, which
  ``ops_bwd.vertical_pool_bwd(arg=...)`` reads instead of the volume; None where not available."""
  lib = _lib.load()
  _f32(vol, 'vol'); _mask(valid, 'valid')
  lead = vol.shape[:-2]
  Z, D = vol.shape[-2:]
  M = int(np.prod(lead))
  plane = torch.empty((*lead, D), dtype=torch.float32, device=vol.device)
  pvalid = torch.empty(lead, dtype=torch.bool, device=vol.device)
  if want_arg:
    if pooling != 'max' or Z > 64 or D > 128:
      return (*vertical_pool(vol, valid, pooling), None)
    argz = torch.empty((*lead, D), dtype=torch.uint8, device=vol.device)
    ties = torch.empty((*lead, D), dtype=torch.uint8, device=vol.device)
    with _region('vertical_pool', 0.0, 4.0 * (vol.numel() + plane.numel()) + valid.numel()):
      st = lib.snap_vertical_pool_max_arg_f32(_p(vol), _p(valid), _p(plane), _p(pvalid), _p(argz), _p(ties),
                                              M, Z, D, _stream())
    _lib.check(st, 'snap_vertical_pool_max_arg_f32')
    return plane, pvalid, (argz, ties)
  with _region('vertical_pool', 0.0, 4.0 * (vol.numel() + plane.numel()) + valid.numel()):
    st = lib.snap_vertical_pool_f32(
        _p(vol), _p(valid), _p(plane), _p(pvalid), M, Z, D, POOLING[pooling], _stream()
    )
  _lib.check(st, 'snap_vertical_pool_f32')
  return plane, pvalid


def vertical_pool_conf(vol, valid, w, bias, log_sigmoid_scores):
  """'softmax' / 'weighted' VerticalPooling.  vol [..., Z, D]; valid [..., Z]; w [D] (or
  [D,1]); bias [1] -> plane [..., D], valid_any [...], scores [..., Z], weights [..., Z]."""
  lib = _lib.load()
  _f32(vol, 'vol'); _mask(valid, 'valid'); _f32(w, 'w'); _f32(bias, 'bias')
  Z, D = vol.shape[-2:]
  lead = vol.shape[:-2]
  M = vol.numel() // (Z * D)
  plane = torch.empty((*lead, D), dtype=torch.float32, device=vol.device)
  pvalid = torch.empty(lead, dtype=torch.bool, device=vol.device)
  scores = torch.empty((*lead, Z), dtype=torch.float32, device=vol.device)
  weights = torch.empty((*lead, Z), dtype=torch.float32, device=vol.device)
  with _region('vertical_pool', 0.0, 4.0 * (vol.numel() + plane.numel())):
    st = lib.snap_vertical_pool_conf_f32(
        _p(vol), _p(valid), _p(w), _p(bias), M, Z, D, int(log_sigmoid_scores), _p(plane),
        _p(pvalid), _p(scores), _p(weights), _stream(),
    )
  _lib.check(st, 'snap_vertical_pool_conf_f32')
  return plane, pvalid, scores, weights


def plane_fuse_match(planes, valids, pooling='max', Wm=None, bm=None,
                     normalize=True, eps=1e-5, want_fused=True):
  """Fuse modality planes and apply the matching head.

  planes: list of [..., D]; valids: list of [...] bool or None (all valid).
  Returns fused [..., D], fvalid [...], matching [..., Dm] (None if Wm is None).
  """
  lib = _lib.load()
  n = len(planes)
  lead = planes[0].shape[:-1]
  D = planes[0].shape[-1]
  M = int(np.prod(lead))
  dev = planes[0].device
  for i, p in enumerate(planes):
    _f32(p, f'planes[{i}]')
    if p.shape != planes[0].shape:
      raise ValueError('plane_fuse_match: plane shapes differ')
  pp = (ctypes.c_void_p * n)(*[p.data_ptr() for p in planes])
  vv = (ctypes.c_void_p * n)(
      *[None if v is None else _mask(v, 'valid').data_ptr() for v in valids]
  )
  fused = torch.empty((*lead, D), dtype=torch.float32, device=dev) if want_fused else None
  fvalid = torch.empty(lead, dtype=torch.bool, device=dev)
  matching = None
  Dm = 0
  if Wm is not None:
    _f32(Wm, 'Wm'); _f32(bm, 'bm')
    Dm = Wm.shape[1]
    matching = torch.empty((*lead, Dm), dtype=torch.float32, device=dev)
  st = lib.snap_plane_fuse_match_f32(
      ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(vv, ctypes.c_void_p), n, M,
      D, POOLING[pooling], _p(fused), _p(fvalid), _p(Wm), _p(bm), Dm,
      int(normalize), eps, _p(matching), _stream(),
  )
  _lib.check(st, 'snap_plane_fuse_match_f32')
  return fused, fvalid, matching


# ----------------------------------------------------------------------------
# pose
# ----------------------------------------------------------------------------


def sim_softmax(fq, fm, scale, clip_negative, num_valid, want_prob=False,
                want_rowstats=False, row_weight=None, math=None):
  """fq [B,Nq,Dm], fm [B,X,Y,Dm], num_valid [B] float ->
  sim [B,Nq,X,Y], chunk_stats [B,Nq,NC,2], (prob), (rowstats).  row_weight [B,Nq]: per-point
  confidence weights that replace the 1 / num_valid normalisation (add_confidence_query).
  math: 'f32' -- the contraction as the exact k-ordered fmaf chain (f32 MFMA); 'bf16x6' / 'bf16x3'
  -- on the bf16 matrix cores with 3 / 2-part split operands (f32 grade / ~2^-17 per product).
  None: 'f32' while ``MATMUL_PRECISION`` is 'f32', else 'bf16x6'."""
  lib = _lib.load()
  _f32(fq, 'fq'); _f32(fm, 'fm'); _f32(num_valid, 'num_valid')
  if row_weight is not None:
    _f32(row_weight, 'row_weight')
    if tuple(row_weight.shape) != tuple(fq.shape[:2]):
      raise ValueError('sim_softmax: row_weight must be [B, Nq]')
  B, Nq, Dm = fq.shape
  X, Y = fm.shape[1:3]
  XY = X * Y
  NC = (XY + SIM_CHUNK - 1) // SIM_CHUNK
  dev = fq.device
  sim = torch.empty((B, Nq, X, Y), dtype=torch.float32, device=dev)
  stats = torch.empty((B, Nq, NC, 2), dtype=torch.float32, device=dev)
  prob = torch.empty_like(sim) if want_prob else None
  rowstats = (
      torch.empty(lib.snap_sim_rowstats_bytes(B, Nq) // 4, dtype=torch.float32, device=dev).view(B, Nq, 2)
      if (want_prob or want_rowstats) else None
  )
  if math is None:
    math = 'f32' if precision() == 'f32' else 'bf16x6'
  parts = SPLIT_PARTS.get(math, 0)
  if parts and not (want_prob or want_rowstats) and Dm in (16, 32, 64):
    wsb = lib.snap_sim_split_workspace_bytes(B, Nq, XY, Dm, parts)
    ws = torch.empty(wsb // 2, dtype=torch.bfloat16, device=dev)
    with _region('sim_softmax', 2.0 * B * Nq * XY * Dm,
                 4.0 * (fq.numel() + fm.numel() + sim.numel() + stats.numel())):
      st = lib.snap_sim_softmax_split_f32(
          _p(fq), _p(fm), B, Nq, XY, Dm, float(scale), int(bool(clip_negative)) | (2 if tuning().SIM_GENERAL_KERNEL else 0),
          _p(num_valid), _p(row_weight), parts, _p(sim), _p(stats), _p(ws), wsb, _stream())
    _lib.check(st, 'snap_sim_softmax_split_f32')
    return sim, stats, None, None
  with _region(
      'sim_softmax', 2.0 * B * Nq * XY * Dm,
      4.0 * (fq.numel() + fm.numel() + sim.numel() + stats.numel()),
  ):
    st = lib.snap_sim_softmax_weighted_f32(
        _p(fq), _p(fm), B, Nq, XY, Dm, float(scale), int(clip_negative),
        _p(num_valid), _p(row_weight), _p(sim), _p(stats), _p(prob), _p(rowstats), _stream(),
    )
  _lib.check(st, 'snap_sim_softmax_weighted_f32')
  return sim, stats, prob, rowstats


def masked_softmax_rows(x, mask):
  """layers.masked_softmax over the last axis of x [B, N] (layers.py:38-43) -> (weights, inclusive
  CDF), both [B, N].  The CDF is non-decreasing, repeats its predecessor bit for bit on an entry of weight 0
  (``ransac_sample`` never draws such a row) and ends at exactly 1."""
  lib = _lib.load()
  _f32(x, 'x'); _mask(mask, 'mask')
  B, N = x.shape
  w = torch.empty_like(x)
  cdf = torch.empty_like(x)
  st = lib.snap_masked_softmax_rows_f32(_p(x), _p(mask), B, N, _p(w), _p(cdf), _stream())
  _lib.check(st, 'snap_masked_softmax_rows_f32')
  return w, cdf


def confidence_head(features, valid, kernel, bias):
  """where(valid, log_sigmoid(features @ kernel + bias), 0): features [..., D], kernel [D] ->
  [...] (bev_mapper.py:292-295)."""
  lib = _lib.load()
  _f32(features, 'features'); _f32(kernel, 'kernel')
  if not torch.is_tensor(bias):
    bias = torch.tensor([float(bias)], dtype=torch.float32, device=features.device)
  bias = _f32(bias.reshape(-1)[:1].contiguous(), 'bias')      # a device scalar: no host sync
  if valid is not None:
    _mask(valid, 'valid')
  D = features.shape[-1]
  M = features.numel() // D
  out = torch.empty(features.shape[:-1], dtype=torch.float32, device=features.device)
  st = lib.snap_confidence_head_f32(_p(features), _p(valid), _p(kernel), _p(bias), M, D, _p(out),
                                    _stream())
  _lib.check(st, 'snap_confidence_head_f32')
  return out


def ransac_sample(fq, fm, chunk_stats, scale, clip_negative, S, seed=0,
                  uniforms=None, row_table=True, row_cdf=None, sim=None, row_unscale=None):
  """Draw S correspondences per scene ~ prob_points.  Returns int32 [B,S,3].
  row_table=False takes the table-free path (same samples; tests compare the two)."""
  lib = _lib.load()
  _f32(fq, 'fq'); _f32(fm, 'fm'); _f32(chunk_stats, 'chunk_stats')
  B, Nq, Dm = fq.shape
  X, Y = fm.shape[1:3]
  if uniforms is not None:
    _f32(uniforms, 'uniforms')
    if tuple(uniforms.shape) != (B, S, 2):
      raise ValueError('ransac_sample: uniforms must be [B,S,2]')
  corr = torch.empty((B, S, 3), dtype=torch.int32, device=fq.device)
  ws = None
  if row_table:
    ws = torch.empty(lib.snap_ransac_sample_workspace_bytes(B, Nq) // 4, dtype=torch.float32,
                     device=fq.device)
  with _region('ransac_sample', 0.0, 12.0 * B * S):
    if sim is not None:
      _f32(sim, 'sim'); _f32(row_unscale, 'row_unscale')
      if sim.numel() != B * Nq * X * Y or tuple(row_unscale.shape) != (B, Nq):
        raise ValueError('ransac_sample: sim must be [B,Nq,X,Y], row_unscale [B,Nq]')
    st = lib.snap_ransac_sample_sim_f32(
        _p(fq), _p(fm), _p(chunk_stats), _p(row_cdf), _p(sim), _p(row_unscale), B, Nq, X, Y, Dm,
        float(scale), int(clip_negative), S, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(uniforms),
        _p(corr), _p(ws), 0 if ws is None else ws.numel() * 4, _stream(),
    )
  _lib.check(st, 'snap_ransac_sample_sim_f32')
  return corr


def poses_from_corr(corr, q_xy, P, retries, cell_size):
  """corr int32 [B,P*retries*2,3], q_xy [B,Nq,2] -> poses [B,P,3] (angle,tx,ty)."""
  lib = _lib.load()
  _chk(corr, torch.int32, 'corr'); _f32(q_xy, 'q_xy')
  B, Nq = q_xy.shape[:2]
  if corr.shape[1] != P * retries * 2:
    raise ValueError('poses_from_corr: corr size')
  poses = torch.empty((B, P, 3), dtype=torch.float32, device=corr.device)
  st = lib.snap_poses_from_corr_f32(
      _p(corr), _p(q_xy), B, Nq, P, retries, float(cell_size), _p(poses), _stream()
  )
  _lib.check(st, 'snap_poses_from_corr_f32')
  return poses


def pose_score(sim, poses, q_xy, valid_q, map_valid, cell_size, mask_oob=False):
  """sim [B,Nq,X,Y]; poses [B,P,3]; q_xy [B,Nq,2]; valid_q [B,Nq] -> scores [B,P]."""
  lib = _lib.load()
  _f32(sim, 'sim'); _f32(poses, 'poses'); _f32(q_xy, 'q_xy'); _mask(valid_q, 'valid_q')
  if map_valid is not None:
    _mask(map_valid, 'map_valid')
  B, Nq, X, Y = sim.shape
  P = poses.shape[1]
  wsb = lib.snap_pose_score_workspace_bytes(B, Nq, P, X, Y)
  ws = torch.empty(wsb // 4, dtype=torch.float32, device=sim.device)
  scores = torch.empty((B, P), dtype=torch.float32, device=sim.device)
  # algorithmic bytes: every VALID query point's score plane read once + poses + scores.
  with _region(
      'pose_score', 0.0, 4.0 * (sim.numel() + poses.numel() + scores.numel())
  ):
    st = lib.snap_pose_score_f32(
        _p(sim), _p(poses), _p(q_xy), _p(valid_q), _p(map_valid), B, Nq, X, Y, P,
        float(cell_size), int(mask_oob), _p(scores), _p(ws), ws.numel() * 4,
        _stream(),
    )
  _lib.check(st, 'snap_pose_score_f32')
  return scores


def pose_score_window_supported(X, Y, radius_cells):
  """True where ``pose_score_window`` takes a window of that radius on an [X, Y] score plane."""
  return bool(_lib.load().snap_pose_score_window_supported(int(X), int(Y), int(radius_cells)))


def pose_score_window(sim, poses, centers, radius_cells, q_xy, valid_q, cell_size):
  """``pose_score`` (mask_oob=False) for poses clustered around ``centers`` [B,3]: every pose of scene b maps
  every query point to within ``radius_cells`` cells of where centers[b] maps it (the refinement lattice of
  grid_refinement).  Same bits as ``pose_score``; a point's score plane is read as one small window."""
  lib = _lib.load()
  _f32(sim, 'sim'); _f32(poses, 'poses'); _f32(centers, 'centers'); _f32(q_xy, 'q_xy'); _mask(valid_q, 'valid_q')
  B, Nq, X, Y = sim.shape
  P = poses.shape[1]
  if tuple(centers.shape) != (B, 3):
    raise ValueError('pose_score_window: centers [B, 3]')
  wsb = lib.snap_pose_score_window_workspace_bytes(B, Nq, P, X, Y)
  ws = torch.empty(wsb // 4, dtype=torch.float32, device=sim.device)
  scores = torch.empty((B, P), dtype=torch.float32, device=sim.device)
  WR, WC = min(2 * radius_cells + 3, X), min((2 * radius_cells + 9) & ~3, Y)
  with _region('pose_score', 0.0, 4.0 * (B * Nq * WR * WC + poses.numel() + scores.numel())):
    st = lib.snap_pose_score_window_f32(
        _p(sim), _p(poses), _p(centers), int(radius_cells), _p(q_xy), _p(valid_q), B, Nq, X, Y, P,
        float(cell_size), _p(scores), _p(ws), ws.numel() * 4, _stream())
  _lib.check(st, 'snap_pose_score_window_f32')
  return scores


def refine_lattice(init, offs_r, offs_p):
  """init [B,3]; offs_r [nr] (rad); offs_p [np] (m) -> [B, nr*np*np, 3]."""
  lib = _lib.load()
  _f32(init, 'init'); _f32(offs_r, 'offs_r'); _f32(offs_p, 'offs_p')
  B = init.shape[0]
  nr, np_ = offs_r.numel(), offs_p.numel()
  out = torch.empty((B, nr * np_ * np_, 3), dtype=torch.float32, device=init.device)
  st = lib.snap_refine_lattice_f32(
      _p(init), _p(offs_r), _p(offs_p), B, nr, np_, _p(out), _stream()
  )
  _lib.check(st, 'snap_refine_lattice_f32')
  return out


def argmax_rows(scores, start=0):
  """argmax of scores[:, start:] -> int32 [B] (relative to start), with the order of np.argmax / jnp.argmax:
  NaN is the maximum and the FIRST NaN wins; among numbers the first maximum wins (+inf included; an all -inf row
  gives 0)."""
  lib = _lib.load()
  _f32(scores, 'scores')
  B, P = scores.shape
  idx = torch.empty((B,), dtype=torch.int32, device=scores.device)
  st = lib.snap_argmax_rows_f32(_p(scores), B, P, start, _p(idx), _stream())
  _lib.check(st, 'snap_argmax_rows_f32')
  return idx


# ----------------------------------------------------------------------------
# generic grid operators (snap/utils/grids.py:116-153)
# ----------------------------------------------------------------------------
def interpolate_nd(array, points, valid_array=None):
  """array [s_0..s_{n-1}, D], points [K, n] (corner-origin coordinates) -> values [K, D],
  valid [K] (grids.py:116-137: linear, 'nearest' extension, zero-weight-invalid-tap rule)."""
  lib = _lib.load()
  _f32(array, 'array'); _f32(points, 'points')
  K, n = points.shape
  if array.dim() != n + 1 or not 1 <= n <= 3:
    raise ValueError(f'interpolate_nd: array {tuple(array.shape)} vs points [K, {n}]')
  D = array.shape[-1]
  size = (ctypes.c_int32 * n)(*array.shape[:n])
  if valid_array is not None:
    _mask(valid_array, 'valid_array')
    if tuple(valid_array.shape) != tuple(array.shape[:n]):
      raise ValueError('interpolate_nd: valid_array shape')
  values = torch.empty((K, D), dtype=torch.float32, device=array.device)
  valid = torch.empty((K,), dtype=torch.bool, device=array.device)
  st = lib.snap_interpolate_nd_f32(_p(array), size, n, D, _p(valid_array), _p(points), K,
                                   _p(values), _p(valid), _stream())
  _lib.check(st, 'snap_interpolate_nd_f32')
  return values, valid


def _occupancy_source(volume, volume_valid, rays, points, num_samples, margin):
  """Shared checks of the two occupancy entry points -> (C arguments of the source + volume, B, P)."""
  _f32(volume, 'volume')
  if volume.dim() != 5:
    raise ValueError(f'occupancy: volume must be [B, X, Y, Z, D], got {tuple(volume.shape)}')
  B, X, Y, Z, D = (int(v) for v in volume.shape)
  if volume_valid is not None:
    _mask(volume_valid, 'volume_valid')
    if tuple(volume_valid.shape) != (B, X, Y, Z):
      raise ValueError(f'occupancy: volume_valid {tuple(volume_valid.shape)} vs volume {tuple(volume.shape)}')
  src, P = _occupancy_points(B, rays, points, num_samples, margin)
  return src + [B, _p(volume), _p(volume_valid), X, Y, Z, D], B, P, D


def _occupancy_points(B, rays, points, num_samples, margin):
  """The point-source checks of the occupancy entry points -> (C arguments of the source, P)."""
  if (rays is None) == (points is None):
    raise ValueError('occupancy: give exactly one of rays=(hits, origins, mask) and points')
  if rays is not None:
    hits, origins, mask = rays
    _f32(hits, 'hits'); _f32(origins, 'origins'); _mask(mask, 'ray mask')
    if hits.dim() != 3 or hits.shape[0] != B or hits.shape[2] != 3 or origins.shape != hits.shape:
      raise ValueError(f'occupancy: hits / origins must be [B={B}, N, 3], got {tuple(hits.shape)} / '
                       f'{tuple(origins.shape)}')
    N = int(hits.shape[1])
    if tuple(mask.shape) != (B, N):
      raise ValueError(f'occupancy: ray mask must be [B, N] = {(B, N)}, got {tuple(mask.shape)}')
    S = int(num_samples)
    if S < 1 or N < 1:
      raise ValueError('occupancy: num_samples and the ray count must be positive')
    src = [_p(hits), _p(origins), _p(mask), N, S, float(margin), None, 0]
    P = S * N
  else:
    _f32(points, 'points')
    if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 3 or points.shape[1] < 1:
      raise ValueError(f'occupancy: points must be [B={B}, Q, 3], got {tuple(points.shape)}')
    P = int(points.shape[1])
    src = [None, None, None, 0, 1, 0.0, _p(points), P]
  return src, P


def occupancy_ray_features(volume, volume_valid, cell_size, *, rays=None, points=None, num_samples=1,
                           margin=0.0, want_samples=True):
  """occupancy_net.py:34-60,107-111 up to the MLP: the query points of each scene -- rays=(hits
  [B, N, 3], origins [B, N, 3], mask [B, N]) sampled into P = num_samples * N points (k * N + n order),
  or explicit points [B, P, 3] -- interpolated in volume [B, X, Y, Z, D] at point / cell_size.
  Returns (features [B * P, D], valid [B, P], samples) with samples = (points [B, P, 3], labels
  [B, P], ray_valid [B, P]) for rays and want_samples, else None."""
  lib = _lib.load()
  args, B, P, D = _occupancy_source(volume, volume_valid, rays, points, num_samples, margin)
  dev = volume.device
  features = torch.empty((B * P, D), dtype=torch.float32, device=dev)
  valid = torch.empty((B, P), dtype=torch.bool, device=dev)
  samples = None
  if rays is not None and want_samples:
    samples = (torch.empty((B, P, 3), dtype=torch.float32, device=dev),
               torch.empty((B, P), dtype=torch.bool, device=dev), torch.empty((B, P), dtype=torch.bool, device=dev))
  sp = (None, None, None) if samples is None else tuple(_p(t) for t in samples)
  with _region('occupancy_features', 0.0, 4.0 * B * P * D * 9):
    st = lib.snap_occupancy_ray_features_f32(*args, float(cell_size), *sp, _p(features), _p(valid), _stream())
  _lib.check(st, 'snap_occupancy_ray_features_f32')
  return features, valid, samples


def occupancy_head_supported(D, hidden):
  """True when ``occupancy_head`` takes D -> hidden... -> 1 (one or two hidden widths)."""
  hidden = tuple(int(h) for h in hidden)
  if len(hidden) not in (1, 2):
    return False
  return bool(_lib.load().snap_occupancy_head_supported(int(D), hidden[0], hidden[1] if len(hidden) == 2 else 0))


def occupancy_head(volume, volume_valid, cell_size, mlp_params, *, rays=None, points=None, num_samples=1,
                   margin=0.0, want_samples=True):
  """The fused query chain of occupancy_net.py:84-116 (samples -> trilinear gather -> MLP) in one launch.
  mlp_params: [(kernel [in, out], bias [out]), ...] of MLP(occupancy_mlp), one or two hidden layers and a
  width-1 last layer (``occupancy_head_supported``).  Returns (logits [B, P], valid [B, P], samples) as
  ``occupancy_ray_features``.  Exact f32 arithmetic (the f32 Dense engine's class; within 2e-6 of its
  chain, not bitwise)."""
  lib = _lib.load()
  args, B, P, D = _occupancy_source(volume, volume_valid, rays, points, num_samples, margin)
  layers_ = list(mlp_params)
  if len(layers_) not in (2, 3):
    raise ValueError('occupancy_head: one or two hidden layers and a width-1 output layer')
  widths = []
  d_in = D
  for i, (k, b) in enumerate(layers_):
    _f32(k, f'kernel {i}'); _f32(b, f'bias {i}')
    if k.dim() != 2 or k.shape[0] != d_in or b.shape != (k.shape[1],):
      raise ValueError(f'occupancy_head: layer {i} kernel {tuple(k.shape)} / bias {tuple(b.shape)} after width {d_in}')
    d_in = int(k.shape[1])
    widths.append(d_in)
  if widths[-1] != 1:
    raise ValueError('occupancy_head: the last layer must have width 1')
  if not occupancy_head_supported(D, widths[:-1]):
    raise ValueError(f'occupancy_head: shape D={D}, hidden={tuple(widths[:-1])} not supported '
                     '(see occupancy_head_supported)')
  h1 = widths[0]
  h2 = widths[1] if len(widths) == 3 else 0
  (w0, b0), (w1, b1) = layers_[0], (layers_[1] if h2 else (None, None))
  wo, bo = layers_[-1]
  dev = volume.device
  logits = torch.empty((B, P), dtype=torch.float32, device=dev)
  valid = torch.empty((B, P), dtype=torch.bool, device=dev)
  samples = None
  if rays is not None and want_samples:
    samples = (torch.empty((B, P, 3), dtype=torch.float32, device=dev),
               torch.empty((B, P), dtype=torch.bool, device=dev), torch.empty((B, P), dtype=torch.bool, device=dev))
  sp = (None, None, None) if samples is None else tuple(_p(t) for t in samples)
  flops = 2.0 * B * P * (D * h1 + (h1 * h2 + h2 if h2 else h1))
  with _region('occupancy_head', flops, 4.0 * B * P * 2):
    st = lib.snap_occupancy_head_f32(*args, float(cell_size), _p(w0), _p(b0), h1, _p(w1), _p(b1), h2, _p(wo),
                                     _p(bo), *sp, _p(logits), _p(valid), _stream())
  _lib.check(st, 'snap_occupancy_head_f32')
  return logits, valid, samples


def expectation_nd(pdf, extent):
  """pdf [..., *extent] -> expected (fractional) index [..., n] (grids.py:148-153)."""
  lib = _lib.load()
  _f32(pdf, 'pdf')
  n = len(extent)
  if tuple(pdf.shape[-n:]) != tuple(extent) or not 1 <= n <= 3:
    raise ValueError(f'expectation_nd: pdf {tuple(pdf.shape)} vs extent {tuple(extent)}')
  lead = pdf.shape[:-n]
  rows = int(np.prod(lead)) if len(lead) else 1
  size = (ctypes.c_int32 * n)(*extent)
  out = torch.empty((rows, n), dtype=torch.float32, device=pdf.device)
  st = lib.snap_expectation_nd_f32(_p(pdf), rows, size, n, _p(out), _stream())
  _lib.check(st, 'snap_expectation_nd_f32')
  return out.reshape(*lead, n)


# ----------------------------------------------------------------------------
# exhaustive voting
# ----------------------------------------------------------------------------
def rotate_templates(feat, valid, tfm, num_rotations, cell_size, want_tw=True):
  """feat [H,W,D], valid [H,W], tfm [R/4,4] -> templates [R,H,W,D], tvalid [R,H,W],
  tw [H,W,D,R] (None unless want_tw), cw [H,W,1,R], tcount [R]."""
  lib = _lib.load()
  _f32(feat, 'feat'); _mask(valid, 'valid'); _f32(tfm, 'tfm')
  H, W, D = feat.shape
  R = num_rotations
  dev = feat.device
  templates = torch.empty((R, H, W, D), dtype=torch.float32, device=dev)
  tvalid = torch.empty((R, H, W), dtype=torch.bool, device=dev)
  tw = torch.empty((H, W, D, R), dtype=torch.float32, device=dev) if want_tw else None
  cw = torch.empty((H, W, 1, R), dtype=torch.float32, device=dev)
  tcount = torch.empty((R,), dtype=torch.float32, device=dev)
  st = lib.snap_rotate_templates_f32(
      _p(feat), _p(valid), _p(tfm), H, W, D, R, float(cell_size), _p(templates),
      _p(tvalid), _p(tw), _p(cw), _p(tcount), _stream(),
  )
  _lib.check(st, 'snap_rotate_templates_f32')
  return templates, tvalid, tw, cw, tcount


def pad_map(m, mvalid):
  lib = _lib.load()
  _f32(m, 'map'); _mask(mvalid, 'mvalid')
  H, W, D = m.shape
  dev = m.device
  mp = torch.empty((3 * H - 2, 3 * W - 2, D), dtype=torch.float32, device=dev)
  mvp = torch.empty((3 * H - 2, 3 * W - 2), dtype=torch.float32, device=dev)
  st = lib.snap_pad_map_f32(_p(m), _p(mvalid), H, W, D, _p(mp), _p(mvp), _stream())
  _lib.check(st, 'snap_pad_map_f32')
  return mp, mvp


def voting_fft_supported(R, H, W, D, Hm, Wm):
  """True where ``voting_fft`` takes the geometry (<= 1024 transform points per axis)."""
  return _lib.load().snap_voting_fft_workspace_bytes(R, H, W, D, Hm, Wm) > 0


def voting_fft_workspace_bytes(R, H, W, D, Hm, Wm):
  """Bytes of device workspace one ``voting_fft`` call allocates (0: unsupported geometry)."""
  return int(_lib.load().snap_voting_fft_workspace_bytes(R, H, W, D, Hm, Wm))


def voting_fft(templates, tvalid, m, mvalid, tcount, threshold, use_overlap=True):
  """Frequency-domain template matching: templates [R,H,W,D], tvalid [R,H,W], m [Hm,Wm,D],
  mvalid [Hm,Wm], tcount [R] -> finalised scores [R, 3Hm-1-H, 3Wm-1-W]."""
  lib = _lib.load()
  _f32(templates, 'templates'); _f32(m, 'map'); _f32(tcount, 'tcount')
  if use_overlap:
    _mask(tvalid, 'tvalid'); _mask(mvalid, 'mvalid')
  R, H, W, D = templates.shape
  Hm, Wm = m.shape[:2]
  if m.shape[2] != D:
    raise ValueError(f'voting_fft: map has {m.shape[2]} channels, templates {D}')
  nbytes = lib.snap_voting_fft_workspace_bytes(R, H, W, D, Hm, Wm)
  if nbytes == 0:
    raise ValueError(f'voting_fft: unsupported geometry R={R} H={H} W={W} D={D} map {Hm}x{Wm}')
  ws = torch.empty((nbytes,), dtype=torch.uint8, device=templates.device)
  scores = torch.empty((R, 3 * Hm - 1 - H, 3 * Wm - 1 - W), dtype=torch.float32, device=templates.device)
  with _region('voting_fft', flops=0.0, nbytes=4.0 * (templates.numel() + m.numel() + scores.numel())):
    st = lib.snap_voting_fft_f32(
        _p(templates), _p(tvalid) if use_overlap else None, _p(m), _p(mvalid) if use_overlap else None,
        _p(tcount), R, H, W, D, Hm, Wm, float(threshold), int(bool(use_overlap)), _p(ws), nbytes, _p(scores),
        _stream(),
    )
  _lib.check(st, 'snap_voting_fft_f32')
  return scores


def voting_fft_rotated(feat, valid, tfm, cell_size, m, mvalid, num_rotations, min_overlap=0.05):
  """exhaustive_pose_voting in the frequency domain with the templates sampled on the fly: feat [H,H,D],
  valid [H,H], tfm [R/4,4] (first-quadrant template transforms), m [Hm,Wm,D], mvalid [Hm,Wm] ->
  scores [R, 3Hm-1-H, 3Wm-1-H]."""
  lib = _lib.load()
  _f32(feat, 'feat'); _mask(valid, 'valid'); _f32(tfm, 'tfm'); _f32(m, 'map'); _mask(mvalid, 'mvalid')
  H, W, D = feat.shape
  R = int(num_rotations)
  Hm, Wm = m.shape[:2]
  if H != W or R % 4 or tuple(tfm.shape) != (R // 4, 4) or m.shape[2] != D:
    raise ValueError('voting_fft_rotated: square query plane, R % 4 == 0, tfm [R/4, 4], equal channel counts')
  nbytes = lib.snap_voting_fft_workspace_bytes(R, H, H, D, Hm, Wm)
  if nbytes == 0:
    raise ValueError(f'voting_fft_rotated: unsupported geometry R={R} H={H} D={D} map {Hm}x{Wm}')
  ws = torch.empty((nbytes,), dtype=torch.uint8, device=feat.device)
  scores = torch.empty((R, 3 * Hm - 1 - H, 3 * Wm - 1 - H), dtype=torch.float32, device=feat.device)
  with _region('voting_fft', flops=0.0, nbytes=4.0 * (R * feat.numel() + m.numel() + scores.numel())):
    st = lib.snap_voting_fft_rotated_f32(
        _p(feat), _p(valid), _p(tfm), float(cell_size), _p(m), _p(mvalid), R, H, D, Hm, Wm, float(min_overlap * H * H),
        _p(ws), nbytes, _p(scores), _stream())
  _lib.check(st, 'snap_voting_fft_rotated_f32')
  return scores


def template_finalize(raw, cnt, tcount, R, threshold, use_overlap=True):
  """raw, cnt [Ho,Wo,Rp] -> scores [R,Ho,Wo]."""
  lib = _lib.load()
  _f32(raw, 'raw'); _f32(tcount, 'tcount')
  if cnt is not None:
    _f32(cnt, 'cnt')
  Ho, Wo, Rp = raw.shape
  scores = torch.empty((R, Ho, Wo), dtype=torch.float32, device=raw.device)
  st = lib.snap_template_finalize_f32(
      _p(raw), _p(cnt), _p(tcount), Ho, Wo, R, Rp, float(threshold),
      int(use_overlap), _p(scores), _stream(),
  )
  _lib.check(st, 'snap_template_finalize_f32')
  return scores


# The argument checks of the vote-volume operators, each stated once (with ``_vote_taps`` and ``_vote_draws`` below).
# Every message starts with the operator's name.
def _vote_volume(op, t, name):
  """``t`` is an f32 [R, Ho, Wo] volume on a ROCm GPU, by ``_chk``'s rules (TypeError for no tensor or another dtype,
  RuntimeError for a CPU tensor) -> (R, Ho, Wo)."""
  _f32(t, f'{op}: {name}')
  if t.dim() != 3:
    raise ValueError(f'{op}: {name} [R, Ho, Wo], got {tuple(t.shape)}')
  return tuple(t.shape)


def _vote_volume_arg(op, t, name, like=None):
  """``t`` is an f32 [R, Ho, Wo] volume on a ROCm GPU -- with ``like``: of that volume's shape, on its device -- by
  ``_arg_chk``'s rules (ValueError throughout) -> (R, Ho, Wo)."""
  if like is None:
    _arg_chk(t, f'{op}: {name}', (torch.float32,), (None, None, None), None,
             f'{op}: {name} f32 [R, Ho, Wo] on a ROCm GPU')
  else:
    _arg_chk(t, f'{op}: {name}', (torch.float32,), tuple(like.shape), like.device,
             f'{op}: {name} {torch.float32} {list(like.shape)} on {like.device}')
  return tuple(t.shape)


def _vote_scale(op, scale):
  """float(scale) where it is > 0 and finite as the f32 the C side receives (below 2^128), else ValueError."""
  scale = float(scale)
  if not (scale > 0.0 and np.isfinite(ctypes.c_float(scale).value)):
    raise ValueError(f'{op}: scale must be a finite number > 0, got {scale}')
  return scale


def _vote_uniform_mix(op, uniform_mix):
  uniform_mix = float(uniform_mix)
  if not 0.0 <= uniform_mix <= 1.0:
    raise ValueError(f'{op}: uniform_mix must lie in [0, 1], got {uniform_mix}')
  return uniform_mix


def _vote_gt_index(op, gt_index, device):
  """``gt_index`` is None or an f32 [3] tensor on ``device``."""
  if gt_index is not None:
    _f32(gt_index, f'{op}: gt_index')
    if tuple(gt_index.shape) != (3,) or gt_index.device != device:
      raise ValueError(f'{op}: gt_index f32 [3] on {device}, got {tuple(gt_index.shape)} on {gt_index.device}')


def _vote_unsupported(op, R, Ho, Wo, taps=None):
  """The refusal text of a workspace query: the plain-volume limits, with ``taps`` = (Tk, Ta, Tb) the tap operators'."""
  if taps is None:
    return f'{op}: unsupported R={R} Ho={Ho} Wo={Wo} (1 <= R <= 64, Ho, Wo >= 1, R Ho Wo < 2^31)'
  return (f'{op}: unsupported R={R} Ho={Ho} Wo={Wo} Tk={taps[0]} Ta={taps[1]} Tb={taps[2]} (1 <= R <= 64, '
          'Ho, Wo >= 1, R Ho Wo < 2^31, 1 <= Tk <= 16, 1 <= Ta, Tb <= 32)')


def vote_peaks(votes, k, radius_r=1, radius_xy=1):
  """The ``k`` best peaks of a vote volume: votes [R, Ho, Wo] f32 -> (index int32 [k, 3] = (r, a, b), score f32 [k],
  count int32 [2] = (peaks found, clipped to k; NaN votes seen)).  A peak beats every other cell within
  ``radius_r`` rotations (circular) and ``radius_xy`` cells (clipped) in the order "greater value, then smaller
  flat index"; the list is ordered by value descending, then flat index ascending; rows past the found count
  hold -1 / -inf (the full contract: snap_vote_peaks_f32 in include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume('vote_peaks', votes, 'votes')
  k, radius_r, radius_xy = int(k), int(radius_r), int(radius_xy)
  words = _workspace_words(
      lib.snap_vote_peaks_workspace_bytes, (R, Ho, Wo, k, radius_r, radius_xy), votes.numel(),
      f'vote_peaks: unsupported R={R} Ho={Ho} Wo={Wo} k={k} radius_r={radius_r} radius_xy={radius_xy} '
      '(1 <= k <= 64, 0 <= radius_r <= 2 with 2 radius_r + 1 <= R, 1 <= radius_xy <= 4, R Ho Wo < 2^31)')
  ws = torch.empty((words,), dtype=torch.int64, device=votes.device)
  index = torch.empty((k, 3), dtype=torch.int32, device=votes.device)
  score = torch.empty((k,), dtype=torch.float32, device=votes.device)
  count = torch.empty((2,), dtype=torch.int32, device=votes.device)
  # algorithmic bytes: one read of the volume (the outputs are K rows)
  with _region('vote_peaks', 0.0, 4.0 * votes.numel()):
    st = lib.snap_vote_peaks_f32(_p(votes), R, Ho, Wo, k, radius_r, radius_xy, _p(index), _p(score), _p(count),
                                 _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_peaks_f32')
  return index, score, count


def vote_posterior(votes, scale=1.0, gt_index=None):
  """The pose distribution of a vote volume: votes [R, Ho, Wo] f32 (unnormalised log-scores; -inf = masked) ->
  (log_prob_xy f32 [Ho, Wo], log_prob_r f32 [R], stats f32 [16], count int32 [3]) of p = softmax(scale * votes) over
  the finite cells.  stats = (log_z, max x, E[a], E[b], Var a, Cov ab, Var b, C, S, mean rotation index, resultant
  length, entropy, log_prob_gt, 0, 0, 0); count = (contributing cells, NaN or +inf cells, ground-truth sample valid).
  ``gt_index``: None or a device f32 [3] = (k, i, j) (``exhaustive_tfm_to_index``), read on the device (the full
  contract: snap_vote_posterior_f32 in include/snap_hip.h).  ``scale * v`` must stay below the f32 maximum for every
  finite vote (not checked: that would read the volume); beyond it the outputs are NaN.  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume('vote_posterior', votes, 'votes')
  scale = _vote_scale('vote_posterior', scale)
  _vote_gt_index('vote_posterior', gt_index, votes.device)
  words = _workspace_words(lib.snap_vote_posterior_workspace_bytes, (R, Ho, Wo), votes.numel(),
                           _vote_unsupported('vote_posterior', R, Ho, Wo))
  ws = torch.empty((words,), dtype=torch.int64, device=votes.device)
  log_prob_xy = torch.empty((Ho, Wo), dtype=torch.float32, device=votes.device)
  log_prob_r = torch.empty((R,), dtype=torch.float32, device=votes.device)
  stats = torch.empty((16,), dtype=torch.float32, device=votes.device)
  count = torch.empty((3,), dtype=torch.int32, device=votes.device)
  # algorithmic bytes: one read of the volume (the outputs are a plane and a few rows)
  with _region('vote_posterior', 0.0, 4.0 * votes.numel()):
    st = lib.snap_vote_posterior_f32(_p(votes), R, Ho, Wo, scale, _p(gt_index), _p(log_prob_xy), _p(log_prob_r),
                                     _p(stats), _p(count), _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_posterior_f32')
  return log_prob_xy, log_prob_r, stats, count


def vote_credible(votes, levels, scale=1.0, gt_index=None, cell_levels=False):
  """Highest-density credible regions of a vote volume: votes [R, Ho, Wo] f32 (unnormalised log-scores; -inf = masked),
  ``levels`` a host sequence 0 < q_0 < ... < q_{L-1} < 1 (1 <= L <= 8) -> (threshold f32 [L], mass f32 [L], table
  int32 [L, 8] = (cells, pixels, rotations, a_min, a_max, b_min, b_max, 0), level_xy uint8 [Ho, Wo], level_r uint8
  [R], level_cell uint8 [R, Ho, Wo] or None (``cell_levels``), gt_stats f32 [4] = (v_gt, mass above it = the
  credibility of the ground truth, mass at or above it, 0), count int32 [4] = (contributing cells, NaN or +inf cells,
  ground truth valid, ground truth's level or -1)) of p = softmax(scale * votes) over the finite cells.  Region l holds
  the cells with v >= threshold[l], the smallest set of whole tie classes with mass >= q_l; a level map holds, per
  pixel / rotation / cell, the smallest l whose region it touches (L = none).  ``gt_index``: None or a device f32 [3]
  = (k, i, j) (``exhaustive_tfm_to_index``), rounded to the nearest cell on the device (the full contract:
  snap_vote_credible_f32 in include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume('vote_credible', votes, 'votes')
  scale = _vote_scale('vote_credible', scale)
  q = np.asarray(levels, dtype=np.float32).reshape(-1)
  L = int(q.size)
  if not (1 <= L <= 8 and bool(np.all(q > 0)) and bool(np.all(q < 1)) and bool(np.all(np.diff(q) > 0))):
    raise ValueError(f'vote_credible: levels must be 1 to 8 strictly increasing numbers inside (0, 1), got {levels}')
  _vote_gt_index('vote_credible', gt_index, votes.device)
  words = _workspace_words(lib.snap_vote_credible_workspace_bytes, (R, Ho, Wo, L), votes.numel(),
                           _vote_unsupported('vote_credible', R, Ho, Wo))
  dev = votes.device
  ws = torch.empty((words,), dtype=torch.int64, device=dev)
  threshold = torch.empty((L,), dtype=torch.float32, device=dev)
  mass = torch.empty((L,), dtype=torch.float32, device=dev)
  table = torch.empty((L, 8), dtype=torch.int32, device=dev)
  level_xy = torch.empty((Ho, Wo), dtype=torch.uint8, device=dev)
  level_r = torch.empty((R,), dtype=torch.uint8, device=dev)
  level_cell = torch.empty((R, Ho, Wo), dtype=torch.uint8, device=dev) if cell_levels else None
  gt_stats = torch.empty((4,), dtype=torch.float32, device=dev)
  count = torch.empty((4,), dtype=torch.int32, device=dev)
  host_levels = (ctypes.c_float * L)(*q.tolist())
  # algorithmic bytes: six reads of the volume for every L (snap_vote_credible_f32 in the header: the maximum, four
  # digit passes, the level pass)
  with _region('vote_credible', 0.0, 4.0 * votes.numel() * 6):
    st = lib.snap_vote_credible_f32(_p(votes), R, Ho, Wo, scale, host_levels, L, _p(gt_index), _p(threshold), _p(mass),
                                    _p(table), _p(level_xy), _p(level_r), _p(level_cell), _p(gt_stats), _p(count),
                                    _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_credible_f32')
  return threshold, mass, table, level_xy, level_r, level_cell, gt_stats, count


def vote_modes(votes, peaks, win_r=1, win_xy=4, scale=1.0, gt_index=None):
  """The modes of a vote volume: votes [R, Ho, Wo] f32 (unnormalised log-scores; -inf = masked), ``peaks`` int32
  [K, 3] = (r, a, b) rows on the same device (``vote_peaks``' index; a row with a component out of range, such as its
  -1 rows, is empty) -> (stats f32 [K, 16], count int32 [K, 2]).  A cell within ``win_r`` rotations (circular) and
  ``win_xy`` cells (clipped) of at least one peak belongs to the peak nearest in window-normalised distance, ties to
  the lowest row; over the finite cells a peak owns, with x = scale * v: stats[k] = (log_mass = log sum exp(x), max x,
  mean rotation index in [0, R), mean a, mean b, Var r, Cov ra, Cov rb, Var a, Cov ab, Var b in index units, nees_gt,
  0, 0, 0, 0); count[k] = (owned finite cells, owned NaN or +inf cells).  nees_gt = e^T (Sigma + I/12)^-1 e for
  e = gt_index - mean (NaN without one).  ``gt_index``: None or a device f32 [3] = (k, i, j)
  (``exhaustive_tfm_to_index``), read on the device.  An empty row or a mode without finite cells: -inf masses and NaN
  moments (the full contract: snap_vote_modes_f32 in include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume('vote_modes', votes, 'votes')
  _arg_chk(peaks, 'vote_modes: peaks', (torch.int32,), (None, 3), votes.device,
           f'vote_modes: peaks int32 [K, 3] on {votes.device}')
  K, win_r, win_xy = int(peaks.shape[0]), int(win_r), int(win_xy)
  scale = _vote_scale('vote_modes', scale)
  _vote_gt_index('vote_modes', gt_index, votes.device)
  words = _workspace_words(
      lib.snap_vote_modes_workspace_bytes, (R, Ho, Wo, K, win_r, win_xy), votes.numel(),
      f'vote_modes: unsupported R={R} Ho={Ho} Wo={Wo} K={K} win_r={win_r} win_xy={win_xy} '
      '(1 <= K <= 64, 0 <= win_r <= 4 with 2 win_r + 1 <= R, 1 <= win_xy <= 32, R Ho Wo < 2^31)')
  ws = torch.empty((words,), dtype=torch.int64, device=votes.device)
  stats = torch.empty((K, 16), dtype=torch.float32, device=votes.device)
  count = torch.empty((K, 2), dtype=torch.int32, device=votes.device)
  # algorithmic bytes: one read of the K windows (the second walk hits in cache), the peak table, the outputs
  window = (2 * win_r + 1) * (2 * win_xy + 1) ** 2
  with _region('vote_modes', 0.0, 4.0 * K * window + 12.0 * K + 72.0 * K):
    st = lib.snap_vote_modes_f32(_p(votes), R, Ho, Wo, scale, _p(peaks), K, win_r, win_xy, _p(gt_index), _p(stats),
                                 _p(count), _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_modes_f32')
  return stats, count


def vote_recall(votes, rho2, half_r, centres=None, scale=1.0, gt_index=None, maps=False):
  """The expected recall of a vote volume: votes [R, Ho, Wo] f32 (unnormalised log-scores; -inf = masked); ``rho2``,
  ``half_r``: host sequences of L integers (1 <= L <= 8), the squared xy radius in cells (0..1024) and the rotation
  half-width in bins (0..4, 2 half_r + 1 <= R) of L threshold pairs; ``centres``: None or an int32 [K, 3] table of
  (r, a, b) rows on the same device, K <= 64 (``vote_peaks``' index; a row with a component out of range, such as its
  -1 rows, is empty) -> (best_index int32 [L, 3], best_log_mass f32 [L], centre_log_mass f32 [K, L], gt_log_mass f32
  [L], stats f32 [4] = (log_z, max x, 0, 0), count int32 [4] = (contributing cells, NaN or +inf cells, ground truth
  valid, 0), maps f32 [L, R, Ho, Wo] or None).  Over the finite cells, with e = exp(scale * v - max) and S = sum e in
  float64, the log mass of level l at a cell is fl32(min(0, log(sum of e over the ball) - log S)), the ball being the
  cells within ``half_r[l]`` rotations (circular) and squared distance ``rho2[l]`` (clipped to the volume); -inf for a
  ball without a finite cell.  best_index / best_log_mass: the cell of the largest log mass per level (compared as
  f32, then the lower flat index; -1 rows and -inf without a finite cell): the pose of maximum expected recall.
  centre_log_mass: the log mass at each centre, -inf for an empty row.  ``gt_index``: None or a device f32 [3] =
  (k, i, j) (``exhaustive_tfm_to_index``), rounded to the nearest cell on the device as ``vote_credible`` does;
  gt_log_mass is NaN without a valid one.  ``maps``: also return the log mass of every cell; the other outputs hold
  the same bytes either way.  Every ball mass is a sum of non-negative terms (the full contract: snap_vote_recall_f32
  in include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume('vote_recall', votes, 'votes')
  dev = votes.device
  scale = _vote_scale('vote_recall', scale)
  try:
    rho2_h = [operator.index(v) for v in rho2]
    half_h = [operator.index(v) for v in half_r]
  except TypeError:
    raise ValueError(f'vote_recall: rho2 and half_r must be sequences of integers, got {rho2} and {half_r}') from None
  L = len(rho2_h)
  if not (1 <= L <= 8 and len(half_h) == L and all(0 <= v <= 1024 for v in rho2_h)
          and all(0 <= v <= 4 and 2 * v + 1 <= R for v in half_h)):
    raise ValueError(f'vote_recall: 1 to 8 pairs with 0 <= rho2 <= 1024, 0 <= half_r <= 4 and 2 half_r + 1 <= R={R}, '
                     f'got rho2={rho2_h} half_r={half_h}')
  K = 0
  if centres is not None:
    _arg_chk(centres, 'vote_recall: centres', (torch.int32,), (None, 3), dev,
             f'vote_recall: centres int32 [K, 3] on {dev}')
    K = int(centres.shape[0])
    if K > 64:
      raise ValueError(f'vote_recall: at most 64 centres, got {K}')
  _vote_gt_index('vote_recall', gt_index, dev)
  words = _workspace_words(lib.snap_vote_recall_workspace_bytes, (R, Ho, Wo, K, L), votes.numel(),
                           _vote_unsupported('vote_recall', R, Ho, Wo))
  ws = torch.empty((words,), dtype=torch.int64, device=dev)
  best_index = torch.empty((L, 3), dtype=torch.int32, device=dev)
  best_log_mass = torch.empty((L,), dtype=torch.float32, device=dev)
  centre_log_mass = torch.empty((K, L), dtype=torch.float32, device=dev)
  gt_log_mass = torch.empty((L,), dtype=torch.float32, device=dev)
  stats = torch.empty((4,), dtype=torch.float32, device=dev)
  count = torch.empty((4,), dtype=torch.int32, device=dev)
  out_maps = torch.empty((L, R, Ho, Wo), dtype=torch.float32, device=dev) if maps else None
  host_rho2 = (ctypes.c_int32 * L)(*rho2_h)
  host_half = (ctypes.c_int32 * L)(*half_h)
  # algorithmic bytes: two reads of the volume (maximum, weights), one write of the float64 weights, then per level
  # 2 half_r + 1 reads of them (the rows' halo re-reads hit in cache) and, with maps, one f32 write
  n = votes.numel()
  nbytes = 4.0 * n * 2 + 8.0 * n + sum(8.0 * n * (2 * h + 1) for h in half_h) + (4.0 * n * L if maps else 0.0)
  with _region('vote_recall', 0.0, nbytes):
    st = lib.snap_vote_recall_f32(_p(votes), R, Ho, Wo, scale, host_rho2, host_half, L, _p(centres) if K else None, K,
                                  _p(gt_index), _p(best_index), _p(best_log_mass), _p(centre_log_mass) if K else None,
                                  _p(gt_log_mass), _p(stats), _p(count), _p(out_maps), _p(ws), ws.numel() * 8,
                                  _stream())
  _lib.check(st, 'snap_vote_recall_f32')
  return best_index, best_log_mass, centre_log_mass, gt_log_mass, stats, count, out_maps


def vote_odometry(prev, cur, Kr, S, shifts=None, scale_prev=1.0, scale_cur=1.0):
  """The motion between two frames from their votes: ``prev`` [R, Ho, Wo] f32 the previous frame's log-space pose
  distribution (a filter belief, or a vote volume with its temperature as ``scale_prev``), ``cur`` [R, Ho, Wo] f32 the
  current frame's votes, ``Kr`` / ``S`` the half-widths of the window in rotation bins (2 Kr + 1 <= R) and cells
  (<= 32), ``shifts``: None or an int32 [U, R, 3] table of (k, i, j) rows on the same device
  (``pose_exhaustive_voting.increment_lattice``) -> (log_table f32 [2 Kr + 1, R, 2 S + 1, 2 S + 1], log_evidence f32
  [U], best int32 [1], stats f32 [4], count int32 [6]).  With the masses p, q of the two volumes (the filter's predict
  rule: exp(scale * (v - max)) rounded to f32, 0 below e^-40 and for a cell that is not finite) and their sums zp, zq:
  T[k][r][i][j] = sum_(a, b) q[r, a, b] p[(r + k) mod R, a + i, b + j] in float64, log_table = log(T / (zp zq));
  log_evidence[u] = log(sum_r T[shifts[u, r]] / (zp zq)), a row outside the window adding 0; best = the first arg-max
  (-1 when none is finite); stats = (log-sum-exp of scale_prev * prev, of scale_cur * cur, log sum_u
  exp(log_evidence), log_evidence[best]); count = (cells of prev with mass, NaN / +inf cells of prev, the same two of
  cur, shift rows outside the window, finite candidates) (the full contract: snap_vote_odometry_f32 in
  include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  _f32(prev, 'vote_odometry: prev')
  _f32(cur, 'vote_odometry: cur')
  if prev.dim() != 3 or prev.shape != cur.shape or prev.device != cur.device:
    raise ValueError(f'vote_odometry: prev and cur [R, Ho, Wo] on one device, got {tuple(prev.shape)} on {prev.device} '
                     f'and {tuple(cur.shape)} on {cur.device}')
  R, Ho, Wo = prev.shape
  dev = prev.device
  try:
    Kr, S = operator.index(Kr), operator.index(S)
  except TypeError:
    raise ValueError(f'vote_odometry: Kr and S must be integers, got {Kr} and {S}') from None
  if not (0 <= Kr and 2 * Kr + 1 <= R and 0 <= S <= 32):
    raise ValueError(f'vote_odometry: 0 <= Kr with 2 Kr + 1 <= R={R} and 0 <= S <= 32, got Kr={Kr} S={S}')
  try:
    scale_prev, scale_cur = _vote_scale('vote_odometry', scale_prev), _vote_scale('vote_odometry', scale_cur)
  except ValueError:
    raise ValueError(f'vote_odometry: scales must be finite numbers > 0, got {float(scale_prev)} and '
                     f'{float(scale_cur)}') from None
  U = 0
  if shifts is not None:
    _arg_chk(shifts, 'vote_odometry: shifts', (torch.int32,), (None, R, 3), dev,
             f'vote_odometry: shifts int32 [U, {R}, 3] on {dev}')
    U = int(shifts.shape[0])
    if U * R * 3 >= 2 ** 31:
      raise ValueError(f'vote_odometry: {U} candidates of {R} rows do not fit an int32 index')
  words = _workspace_words(lib.snap_vote_odometry_workspace_bytes, (R, Ho, Wo, Kr, S, U), prev.numel(),
                           _vote_unsupported('vote_odometry', R, Ho, Wo))
  ws = torch.empty((words,), dtype=torch.int64, device=dev)
  W = 2 * S + 1
  log_table = torch.empty((2 * Kr + 1, R, W, W), dtype=torch.float32, device=dev)
  log_evidence = torch.empty((U,), dtype=torch.float32, device=dev)
  best = torch.empty((1,), dtype=torch.int32, device=dev)
  stats = torch.empty((4,), dtype=torch.float32, device=dev)
  count = torch.empty((6,), dtype=torch.int32, device=dev)
  # float64 fmas: every cell of cur against its window of prev; algorithmic bytes: two reads of both volumes, one
  # write and (2 Kr + 1) reads of the masses (the halo re-reads hit in cache)
  n = prev.numel()
  with _region('vote_odometry', 2.0 * n * (2 * Kr + 1) * W * W, 4.0 * n * (4 + 2 + 2 * (2 * Kr + 1))):
    st = lib.snap_vote_odometry_f32(_p(prev), _p(cur), scale_prev, scale_cur, _p(shifts) if U else None, R, Ho, Wo,
                                    Kr, S, U, _p(log_table), _p(log_evidence) if U else None, _p(best), _p(stats),
                                    _p(count), _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_odometry_f32')
  return log_table, log_evidence, best, stats, count


def rebase_volume(volume, table, scale=1.0):
  """The wrapper of vote_rebase.hip (its messages carry the operator's name, ``vote_rebase:``; like
  ``plane_align_score`` of vote_refine.hip it is not named ``vote_*``: it takes a host table, not device operands, and
  its refusals are tabled in tests/test_gpu_vote_rebase.py).  A vote volume or belief carried into another MAP frame: volume f32 [R, Ho, Wo] (log-space, -inf = impossible
  pose), table = (dk, A, o) host numbers (``pose_exhaustive_voting.rebase_table``: dk in [0, R), A 2 x 2, o 2) ->
  (dst f32 [R, Ho, Wo], stats float64 [4], count int32 [4]).  The destination cell (r, a, b) reads the masses
  exp(scale * (volume - max)) at the rotation r - dk (circular) and the plane position A (a, b) + o with the trilinear
  split, taps of weight 0 or outside the volume skipped; dst = the normalised log-probabilities, -inf where no mass
  arrives.  stats = (log-sum-exp of scale * volume, share of the mass that arrived, largest finite volume value,
  largest dst); count = (finite cells of dst, NaN cells of dst, NaN / +inf cells of volume, cells of dst the old frame
  does not cover) (the full contract: snap_vote_rebase_f32 in include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume_arg('vote_rebase', volume, 'volume')
  scale = _vote_scale('vote_rebase', scale)
  try:
    dk, A, o = table
    dk = float(dk)
    A = np.asarray(A, dtype=np.float64).reshape(2, 2)
    o = np.asarray(o, dtype=np.float64).reshape(2)
  except (TypeError, ValueError):
    raise ValueError(f'vote_rebase: table = (dk, A [2, 2], o [2]) of host numbers, got {table!r}') from None
  if not (np.isfinite(A).all() and np.isfinite(o).all()):
    raise ValueError(f'vote_rebase: the table must be finite, got A={A.tolist()} o={o.tolist()}')
  if not 0.0 <= dk < R:
    raise ValueError(f'vote_rebase: dk must lie in [0, R={R}), got {dk}')
  words = _workspace_words(lib.snap_vote_rebase_workspace_bytes, (R, Ho, Wo), volume.numel(),
                           _vote_unsupported('vote_rebase', R, Ho, Wo))
  dev = volume.device
  ws = torch.empty((words,), dtype=torch.int64, device=dev)
  dst = torch.empty((R, Ho, Wo), dtype=torch.float32, device=dev)
  stats = torch.empty((4,), dtype=torch.float64, device=dev)
  count = torch.empty((4,), dtype=torch.int32, device=dev)
  # bytes the launches move (the kernel file's header): about 5 passes over the volume
  with _region('vote_rebase', 0.0, 4.0 * volume.numel() * 5):
    st = lib.snap_vote_rebase_f32(_p(volume), R, Ho, Wo, scale, dk, float(A[0, 0]), float(A[0, 1]), float(A[1, 0]),
                                  float(A[1, 1]), float(o[0]), float(o[1]), _p(dst), _p(stats), _p(count), _p(ws),
                                  ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_rebase_f32')
  return dst, stats, count


def temper_volume(votes, scales, gt_index=None):
  """The wrapper of vote_temper.hip (its messages carry the operator's name, ``vote_temper:``; like ``rebase_volume``
  it is not named ``vote_*``: it takes a host ladder, and its refusals are tabled in tests/test_gpu_vote_temper.py).
  A vote volume's statistics over a temperature ladder: votes [R, Ho, Wo] f32 (unnormalised log-scores; -inf =
  masked), ``scales`` a host sequence of 1 to 16 finite numbers > 0 whose f32 roundings increase strictly ->
  (table float64 [S, 8], stats float64 [4], count int32 [4]) of p_s = softmax(s * votes) over the finite cells.
  table[l] = (log_z, E[v], Var[v], entropy, log p_max, log_prob_gt, dnll = E[v] - v_gt, 0) at s = scales[l]; stats =
  (largest finite vote, v_gt, 0, 0); count = (contributing cells, NaN or +inf cells, ground-truth sample valid, 0).
  ``gt_index``: None or a device f32 [3] = (k, i, j) (``exhaustive_tfm_to_index``), sampled on the device by
  ``vote_posterior``'s rule.  ``scale * v`` is never formed in f32: there is no overflow condition on the votes (the
  full contract: snap_vote_temper_f32 in include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume('vote_temper', votes, 'votes')
  try:
    ladder = np.asarray(scales, dtype=np.float64).reshape(-1)
  except (TypeError, ValueError):
    raise ValueError(f'vote_temper: scales must be a host sequence of numbers, got {scales!r}') from None
  with np.errstate(over='ignore'):
    s32 = ladder.astype(np.float32)
  S = int(s32.size)
  if not (1 <= S <= 16 and bool(np.all(np.isfinite(s32))) and bool(np.all(s32 > 0)) and bool(np.all(np.diff(s32) > 0))):
    raise ValueError('vote_temper: scales must be 1 to 16 finite numbers > 0, strictly increasing as f32, got '
                     f'{ladder.tolist()}')
  _vote_gt_index('vote_temper', gt_index, votes.device)
  words = _workspace_words(lib.snap_vote_temper_workspace_bytes, (R, Ho, Wo, S), votes.numel(),
                           _vote_unsupported('vote_temper', R, Ho, Wo))
  dev = votes.device
  ws = torch.empty((words,), dtype=torch.int64, device=dev)
  table = torch.empty((S, 8), dtype=torch.float64, device=dev)
  stats = torch.empty((4,), dtype=torch.float64, device=dev)
  count = torch.empty((4,), dtype=torch.int32, device=dev)
  host_scales = (ctypes.c_float * S)(*s32.tolist())
  # algorithmic bytes: one read of the volume (the second launch's read of it is meant to hit in cache; the outputs are
  # S rows)
  with _region('vote_temper', 0.0, 4.0 * votes.numel()):
    st = lib.snap_vote_temper_f32(_p(votes), R, Ho, Wo, host_scales, S, _p(gt_index), _p(table), _p(stats), _p(count),
                                  _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_temper_f32')
  return table, stats, count


def prior_volume(votes, table, scale=1.0, device=None):
  """The wrapper of vote_prior.hip (its messages carry the operator's name, ``vote_prior:``; like ``rebase_volume`` and
  ``temper_volume`` it is not named ``vote_*``: it takes a host table, and its refusals are tabled in
  tests/test_gpu_vote_prior.py).  A position / heading prior fused into a vote volume or belief: votes [R, Ho, Wo] f32 (log-scores; -inf = masked) or
  None (the prior itself as a belief, on ``device``), ``table`` a host table with the attributes ``shape`` = (R, Ho,
  Wo), ``centres`` int32 [M, R, 2], ``planes`` f32 [M, R, 3] and ``comps`` f32 [M, 4], 1 <= M <= 8, as numpy arrays
  (``pose_exhaustive_voting.pose_prior``) -> (out f32 [R, Ho, Wo], resp float64 [M], stats float64 [8], count int32
  [4]).  With u the table's unnormalised log-prior of a cell and t = scale * votes + u over the finite cells: out = t -
  log_z (-inf elsewhere); stats = (log_z, the log-sum-exp of scale * votes, that of u over the whole lattice, that of u
  over the finite cells, E_post[u], 0, 0, 0); resp = the components' posterior responsibilities; count = (contributing
  cells, NaN or +inf cells, contributing cells whose mass underflowed, 0) (the full contract: snap_vote_prior_f32 in
  include/snap_hip.h).  The table is uploaded once per device and kept with the ``table`` object: a repeated prior
  uploads nothing.  No host synchronisation."""
  lib = _lib.load()
  try:
    shape = tuple(int(v) for v in table.shape)
    centres, planes, comps = table.centres, table.planes, table.comps
    M = int(comps.shape[0])
    ok = (len(shape) == 3 and centres.dtype == np.int32 and planes.dtype == np.float32 and comps.dtype == np.float32
          and centres.shape == (M, shape[0], 2) and planes.shape == (M, shape[0], 3) and comps.shape == (M, 4))
  except (AttributeError, TypeError, ValueError, IndexError):
    ok = False
  if not ok:
    raise ValueError('vote_prior: table with shape = (R, Ho, Wo), centres int32 [M, R, 2], planes f32 [M, R, 3] and '
                     f'comps f32 [M, 4] as numpy arrays, got {table!r}')
  if votes is None:
    if device is None or torch.device(device).type != 'cuda':
      raise ValueError(f'vote_prior: without votes a ROCm device must be named, got {device}')
    dev = torch.device(device)
    if dev.index is None:
      dev = torch.device('cuda', torch.cuda.current_device())
    scale = 1.0
  else:
    if _vote_volume_arg('vote_prior', votes, 'votes') != shape:
      raise ValueError(f'vote_prior: the table was built for {shape}, votes are {tuple(votes.shape)}')
    dev = votes.device
    scale = _vote_scale('vote_prior', scale)
  R, Ho, Wo = shape
  n = R * Ho * Wo
  words = _workspace_words(lib.snap_vote_prior_workspace_bytes, (R, Ho, Wo, M), n,
                           _vote_unsupported('vote_prior', R, Ho, Wo)[:-1] + f', 1 <= M <= 8; M={M})')
  from snap_amd.models import base   # (the per-device constant cache lives there; base imports this module)

  def make():   # one blob: the int32 centres, then the two f32 tables
    raw = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in (centres, planes, comps)])
    return torch.from_numpy(raw)
  blob = base.device_const('vote_prior_table', dev, make, owner=table)
  nc, npl = centres.nbytes, planes.nbytes
  ws = torch.empty((words,), dtype=torch.int64, device=dev)
  out = torch.empty((R, Ho, Wo), dtype=torch.float32, device=dev)
  resp = torch.empty((M,), dtype=torch.float64, device=dev)
  stats = torch.empty((8,), dtype=torch.float64, device=dev)
  count = torch.empty((4,), dtype=torch.int32, device=dev)
  # algorithmic bytes: one read and one write of the volume
  with _region('vote_prior', 0.0, 4.0 * n * (1 if votes is None else 2)):
    st = lib.snap_vote_prior_f32(_p(votes), R, Ho, Wo, scale, M, _p(blob), _p(blob[nc:]), _p(blob[nc + npl:]), _p(out),
                                 _p(resp), _p(stats), _p(count), _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_prior_f32')
  return out, resp, stats, count


def raster_volume(votes, raster, scale=1.0, write=0, gt_index=None, device=None):
  """The wrapper of vote_raster.hip (its messages carry the operator's name, ``vote_raster:``; like ``prior_volume`` it
  takes a host table and is not named ``vote_*``).  A road / lane raster prior fused into a vote volume or belief, over
  a ladder of S strengths: votes [R, Ho, Wo] f32 (log-scores; -inf = masked) or None (the raster prior itself as a
  belief, on ``device``), ``raster`` a host table with the attributes ``shape`` = (R, Ho, Wo), ``raster`` f32 [X, Y, 4] =
  (A, C, S, valid), ``offsets`` int32 [R, 2], ``planes`` f32 [R, 4] = (f_a, f_b, cos, sin), ``outside`` (a float, finite
  or -inf) and ``strengths`` [S] (> 0, 1 <= S <= 8) as numpy arrays (``pose_exhaustive_voting.raster_prior``);
  ``write``: the ladder index whose posterior is returned; ``gt_index``: a flat cell index, None or -1 -> (out f32 [R,
  Ho, Wo], table float64 [S, 4], stats float64 [4], count int32 [4]).  With g the raster's interpolated log-prior of a
  cell and t_s = scale * votes + strengths[s] * g over the cells F with a finite vote and g > -inf: out = t_write - log_z
  (-inf elsewhere); table[s] = (log_z_s, the log-sum-exp of strengths[s] * g over the lattice, E_s[g], Var_s[g]); stats
  = (the log-sum-exp of scale * votes, scale * votes and g at gt_index, 0); count = (cells with a finite vote, NaN or
  +inf cells, finite-vote cells the raster excludes, cells of F whose mass underflowed) (the full contract:
  snap_vote_raster_f32 in include/snap_hip.h).  The table is uploaded once per device and kept with the ``raster``
  object.  No host synchronisation."""
  lib = _lib.load()
  try:
    shape = tuple(int(v) for v in raster.shape)
    planes4, offsets, planes = raster.raster, raster.offsets, raster.planes
    strengths = np.asarray(raster.strengths, dtype=np.float64).reshape(-1)
    outside = float(raster.outside)
    X, Y = int(planes4.shape[0]), int(planes4.shape[1])
    ok = (len(shape) == 3 and planes4.dtype == np.float32 and offsets.dtype == np.int32 and planes.dtype == np.float32
          and planes4.shape == (X, Y, 4) and X >= 1 and Y >= 1 and offsets.shape == (shape[0], 2)
          and planes.shape == (shape[0], 4) and outside < np.inf)   # (NaN fails the comparison)
  except (AttributeError, TypeError, ValueError, IndexError):
    ok = False
  if not ok:
    raise ValueError('vote_raster: table with shape = (R, Ho, Wo), raster f32 [X, Y, 4], offsets int32 [R, 2], planes '
                     f'f32 [R, 4], an outside that is finite or -inf and strengths [S] as numpy arrays, got {raster!r}')
  S = int(strengths.size)
  with np.errstate(over='ignore'):
    lam = strengths.astype(np.float32)
  if not (1 <= S <= 8 and bool(np.all(np.isfinite(lam))) and bool(np.all(lam > 0))):
    raise ValueError(f'vote_raster: strengths must be 1 to 8 finite numbers > 0 as f32, got {strengths.tolist()}')
  write = int(write)
  if not 0 <= write < S:
    raise ValueError(f'vote_raster: write must index the {S} strengths, got {write}')
  if votes is None:
    if device is None or torch.device(device).type != 'cuda':
      raise ValueError(f'vote_raster: without votes a ROCm device must be named, got {device}')
    dev = torch.device(device)
    if dev.index is None:
      dev = torch.device('cuda', torch.cuda.current_device())
    scale = 1.0
  else:
    if _vote_volume_arg('vote_raster', votes, 'votes') != shape:
      raise ValueError(f'vote_raster: the table was built for {shape}, votes are {tuple(votes.shape)}')
    dev = votes.device
    scale = _vote_scale('vote_raster', scale)
  R, Ho, Wo = shape
  n = R * Ho * Wo
  gt = -1 if gt_index is None else int(gt_index)
  if not -1 <= gt < n:
    raise ValueError(f'vote_raster: gt_index must be None, -1 or a flat index below {n}, got {gt_index}')
  words = _workspace_words(lib.snap_vote_raster_workspace_bytes, (R, Ho, Wo, X, Y, S), n,
                           _vote_unsupported('vote_raster', R, Ho, Wo)[:-1] + f', X Y < 2^29; X={X} Y={Y})')
  from snap_amd.models import base   # (the per-device constant cache lives there; base imports this module)

  def make():   # one blob: the f32 raster (16-byte aligned at the front), the f32 planes, then the int32 offsets
    raw = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in (planes4, planes, offsets)])
    return torch.from_numpy(raw)
  blob = base.device_const('vote_raster_table', dev, make, owner=raster)
  nr, npl = planes4.nbytes, planes.nbytes
  lam_c = (ctypes.c_float * S)(*lam.tolist())
  ws = torch.empty((words,), dtype=torch.int64, device=dev)
  out = torch.empty((R, Ho, Wo), dtype=torch.float32, device=dev)
  table = torch.empty((S, 4), dtype=torch.float64, device=dev)
  stats = torch.empty((4,), dtype=torch.float64, device=dev)
  count = torch.empty((4,), dtype=torch.int32, device=dev)
  # algorithmic bytes: one read and one write of the volume, one read of the raster
  with _region('vote_raster', 0.0, 4.0 * n * (1 if votes is None else 2) + nr):
    st = lib.snap_vote_raster_f32(_p(votes), R, Ho, Wo, scale, _p(blob), X, Y, _p(blob[nr + npl:]), _p(blob[nr:]),
                                  outside, lam_c, S, write, gt, _p(out), _p(table), _p(stats), _p(count), _p(ws),
                                  ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_raster_f32')
  return out, table, stats, count


def vote_fuse(volumes, shifts, weights=None):
  """Multi-frame fusion of aligned vote volumes: volumes [N, R, Ho, Wo] f32 (unnormalised log-scores; -inf = masked),
  shifts f32 [N, R, 3] = (dk, da, db) on the same device (``pose_exhaustive_voting.sequence_shift_table``), weights
  None (all 1) or f32 [N] on the same device -> (fused f32 [R, Ho, Wo], count int32 [2]).  fused[r, a, b] =
  sum_n w_n * (the trilinear blend, circular in k, of volume n at (r + dk, a + da, b + db)); -inf where any frame does
  not see the pose (out of range, a non-finite shift row or a -inf tap), NaN where a tap is NaN / +inf; count =
  (finite cells, NaN cells) of ``fused`` (the full contract: snap_vote_fuse_f32 in include/snap_hip.h).  No host
  synchronisation."""
  lib = _lib.load()
  _f32(volumes, 'vote_fuse: volumes')
  if volumes.dim() != 4:
    raise ValueError(f'vote_fuse: volumes [N, R, Ho, Wo], got {tuple(volumes.shape)}')
  N, R, Ho, Wo = volumes.shape
  for t, name, shape in ((shifts, 'shifts', (N, R, 3)), (weights, 'weights', (N,))):
    if t is None and name == 'weights':
      continue
    _arg_chk(t, f'vote_fuse: {name}', (torch.float32,), shape, volumes.device,
             f'vote_fuse: {name} f32 {list(shape)} on {volumes.device}')
  words = _workspace_words(
      lib.snap_vote_fuse_workspace_bytes, (N, R, Ho, Wo), volumes.numel(),
      f'vote_fuse: unsupported N={N} R={R} Ho={Ho} Wo={Wo} (1 <= N <= 16, 1 <= R <= 64, Ho, Wo >= 1, '
      'N R Ho Wo < 2^31)')
  ws = torch.empty((words,), dtype=torch.int64, device=volumes.device)
  fused = torch.empty((R, Ho, Wo), dtype=torch.float32, device=volumes.device)
  count = torch.empty((2,), dtype=torch.int32, device=volumes.device)
  # algorithmic bytes: the output once and, per frame, the two source planes of every rotation (one where the table
  # has an integer dk, which the host does not know without reading it: the upper figure is reported)
  with _region('vote_fuse', 0.0, 4.0 * R * Ho * Wo * (1 + 2 * N)):
    st = lib.snap_vote_fuse_f32(_p(volumes), _p(shifts), _p(weights), N, R, Ho, Wo, _p(fused), _p(count), _p(ws),
                                ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_fuse_f32')
  return fused, count


def _vote_taps(op, taps, R, device):
  """The tap tuple of ``vote_filter`` / ``vote_smooth`` checked -> (taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb)."""
  if not isinstance(taps, (tuple, list)) or len(taps) != 5:
    raise ValueError(f'{op}: taps = (taps_k, lk, taps_a, taps_b, offsets)')
  taps_k, lk, taps_a, taps_b, offsets = taps
  if isinstance(lk, bool) or not isinstance(lk, (int, np.integer)) or not -2 ** 31 <= int(lk) < 2 ** 31:
    raise ValueError(f'{op}: lk must be an int32 number, got {lk!r}')
  Tk = taps_k.shape[0] if isinstance(taps_k, torch.Tensor) and taps_k.dim() == 1 else -1
  Ta = taps_a.shape[1] if isinstance(taps_a, torch.Tensor) and taps_a.dim() == 2 else -1
  Tb = taps_b.shape[1] if isinstance(taps_b, torch.Tensor) and taps_b.dim() == 2 else -1
  for t, name, dtype, shape in ((taps_k, 'taps_k', torch.float32, (Tk,)), (taps_a, 'taps_a', torch.float32, (R, Ta)),
                                (taps_b, 'taps_b', torch.float32, (R, Tb)), (offsets, 'offsets', torch.int32, (R, 2))):
    _arg_chk(t, f'{op}: {name}', (dtype,), shape, device, f'{op}: {name} {dtype} {list(shape)} on {device}')
  return taps_k, int(lk), taps_a, taps_b, offsets, Tk, Ta, Tb


def vote_filter(belief, votes, taps, scale=1.0, uniform_mix=0.0):
  """One step of the recursive pose filter on the vote lattice: belief f32 [R, Ho, Wo] (the log-space belief after the
  previous frame, -inf = impossible pose) or None (a uniform prior: a track starts), votes f32 [R, Ho, Wo] (the new
  frame), taps = (taps_k f32 [Tk], lk int, taps_a f32 [R, Ta], taps_b f32 [R, Tb], offsets int32 [R, 2]) on the same
  device (``pose_exhaustive_voting.motion_taps``) -> (belief_out f32 [R, Ho, Wo], stats f32 [4], count int32 [4]).
  The belief's masses exp(belief - max) are transported and diffused by the three tap passes (rotation, circular; rows
  and columns per output rotation), mixed with ``uniform_mix`` of a uniform distribution, multiplied by
  exp(scale * votes) and normalised over the finite cells.  stats = (log evidence of the frame, share of the mass that
  stayed in the volume, largest finite belief, largest belief_out); count = (finite cells of belief_out, NaN / +inf
  cells of belief, NaN cells of belief_out, cells of belief with mass).  Taps must be finite, >= 0 and either 0 or
  >= 2^-20 (not checked: ``motion_taps`` guarantees it; the full contract: snap_vote_filter_f32 in
  include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume_arg('vote_filter', votes, 'votes')
  if belief is not None:
    _vote_volume_arg('vote_filter', belief, 'belief', votes)
  taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb = _vote_taps('vote_filter', taps, R, votes.device)
  scale = _vote_scale('vote_filter', scale)
  uniform_mix = _vote_uniform_mix('vote_filter', uniform_mix)
  words = _workspace_words(lib.snap_vote_filter_workspace_bytes, (R, Ho, Wo, Tk, Ta, Tb), votes.numel(),
                           _vote_unsupported('vote_filter', R, Ho, Wo, (Tk, Ta, Tb)))
  ws = torch.empty((words,), dtype=torch.int64, device=votes.device)
  belief_out = torch.empty((R, Ho, Wo), dtype=torch.float32, device=votes.device)
  stats = torch.empty((4,), dtype=torch.float32, device=votes.device)
  count = torch.empty((4,), dtype=torch.int32, device=votes.device)
  # bytes the launches move (the kernel file's header): 12 passes over the volume with a belief, 3 without
  with _region('vote_filter', 0.0, 4.0 * votes.numel() * (3 if belief is None else 12)):
    st = lib.snap_vote_filter_f32(_p(belief), _p(votes), _p(taps_k), int(lk), _p(taps_a), _p(taps_b), _p(offsets),
                                  R, Ho, Wo, Tk, Ta, Tb, scale, uniform_mix, _p(belief_out), _p(stats), _p(count),
                                  _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_filter_f32')
  return belief_out, stats, count


def vote_smooth(belief, smoothed_next, taps, uniform_mix=0.0):
  """One backward step of the smoother that goes with ``vote_filter``: belief f32 [R, Ho, Wo] (the filter's belief
  after frame t), smoothed_next f32 [R, Ho, Wo] (the smoothed belief of frame t + 1; for the last frame of a track its
  filtered belief), taps = the tuple ``vote_filter`` was given for the step from t to t + 1 and ``uniform_mix`` that
  step's -> (smoothed f32 [R, Ho, Wo], stats f32 [4], count int32 [4]).  The filter's predict step is repeated on
  ``belief`` (the same device code: the same bits), the ratio smoothed_next / prior is carried back through the
  adjoint of the three tap passes (columns, rows, then the circular rotation pass) and multiplied into the belief;
  normalised over the finite cells.  stats = (log_norm: 0 up to rounding for beliefs and taps that belong together,
  share of the belief's mass that stayed in the volume, largest log ratio, largest smoothed); count = (finite cells of
  smoothed, NaN / +inf cells of belief, NaN / +inf cells of smoothed_next, cells of smoothed_next with ratio mass)
  (the full contract: snap_vote_smooth_f32 in include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume_arg('vote_smooth', belief, 'belief')
  _vote_volume_arg('vote_smooth', smoothed_next, 'smoothed_next', belief)
  taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb = _vote_taps('vote_smooth', taps, R, belief.device)
  uniform_mix = _vote_uniform_mix('vote_smooth', uniform_mix)
  words = _workspace_words(lib.snap_vote_smooth_workspace_bytes, (R, Ho, Wo, Tk, Ta, Tb), belief.numel(),
                           _vote_unsupported('vote_smooth', R, Ho, Wo, (Tk, Ta, Tb)))
  ws = torch.empty((words,), dtype=torch.int64, device=belief.device)
  smoothed = torch.empty((R, Ho, Wo), dtype=torch.float32, device=belief.device)
  stats = torch.empty((4,), dtype=torch.float32, device=belief.device)
  count = torch.empty((4,), dtype=torch.int32, device=belief.device)
  # bytes the launches move (snap_vote_smooth_f32 in the header): 22 passes over the volume
  with _region('vote_smooth', 0.0, 4.0 * belief.numel() * 22):
    st = lib.snap_vote_smooth_f32(_p(belief), _p(smoothed_next), _p(taps_k), lk, _p(taps_a), _p(taps_b), _p(offsets),
                                  R, Ho, Wo, Tk, Ta, Tb, uniform_mix, _p(smoothed), _p(stats), _p(count), _p(ws),
                                  ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_smooth_f32')
  return smoothed, stats, count


def vote_pairs(belief, smoothed_next, taps, uniform_mix=0.0):
  """The tap posteriors of one filter step given all frames: arguments as ``vote_smooth``'s (belief f32 [R, Ho, Wo] =
  the filter's belief after frame t, required: a step without a previous frame has no pair; smoothed_next = the
  smoothed belief of frame t + 1; taps and ``uniform_mix`` = that step's) -> (hist_k float64 [Tk], hist_a float64
  [R, Ta], hist_b float64 [R, Tb], stats float64 [4], count int32 [4]) on the device.  The posterior over how the pose
  moved from t to t + 1 splits into the jump branch (the uniform share of the prior) and the stay branch by tap; the
  histograms are the stay branch's marginals per axis (hist_a / hist_b per destination rotation), each summing to
  ``stay``.  stats = (stay, jump: they sum to 1; log_norm: the log of their total before normalisation, 0 up to
  rounding for arguments that belong together; mass_kept: the filter's, its bits once converted to f32); count = (cells
  of belief with mass, NaN / +inf cells of belief, NaN / +inf cells of smoothed_next, cells of smoothed_next with ratio
  mass).  Without ratio mass everything but mass_kept is 0 and log_norm -inf (the full contract: snap_vote_pairs_f32 in
  include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume_arg('vote_pairs', belief, 'belief')
  _vote_volume_arg('vote_pairs', smoothed_next, 'smoothed_next', belief)
  taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb = _vote_taps('vote_pairs', taps, R, belief.device)
  uniform_mix = _vote_uniform_mix('vote_pairs', uniform_mix)
  words = _workspace_words(lib.snap_vote_pairs_workspace_bytes, (R, Ho, Wo, Tk, Ta, Tb), belief.numel(),
                           _vote_unsupported('vote_pairs', R, Ho, Wo, (Tk, Ta, Tb)))
  ws = torch.empty((words,), dtype=torch.int64, device=belief.device)
  hist_k = torch.empty((Tk,), dtype=torch.float64, device=belief.device)
  hist_a = torch.empty((R, Ta), dtype=torch.float64, device=belief.device)
  hist_b = torch.empty((R, Tb), dtype=torch.float64, device=belief.device)
  stats = torch.empty((4,), dtype=torch.float64, device=belief.device)
  count = torch.empty((4,), dtype=torch.int32, device=belief.device)
  # bytes the launches move (snap_vote_pairs_f32 in the header): 22 passes over the volume
  with _region('vote_pairs', 0.0, 4.0 * belief.numel() * 22):
    st = lib.snap_vote_pairs_f32(_p(belief), _p(smoothed_next), _p(taps_k), lk, _p(taps_a), _p(taps_b), _p(offsets),
                                 R, Ho, Wo, Tk, Ta, Tb, uniform_mix, _p(hist_k), _p(hist_a), _p(hist_b), _p(stats),
                                 _p(count), _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_pairs_f32')
  return hist_k, hist_a, hist_b, stats, count


def vote_viterbi(score_prev, votes, log_taps, scale=1.0, log_stay=0.0, log_jump=float('-inf')):
  """One forward step of the max-product (Viterbi) recursion that goes with ``vote_filter``: score_prev f32
  [R, Ho, Wo] (the log score of the best path into every pose of the previous frame, -inf = no path) or None (a track
  starts), votes f32 [R, Ho, Wo] (the new frame), log_taps = ``vote_filter``'s tap tuple with every tap replaced by
  its logarithm, -inf for a zero tap (``pose_exhaustive_voting.motion_log_taps``) -> (score f32 [R, Ho, Wo], back int32
  [R, Ho, Wo], stats f32 [2], count int32 [6]).  score_prev minus its maximum M is carried through three max-plus tap
  passes (rotation, circular; rows and columns per output rotation; the lowest tap index among equals);
  best = max(log_stay + that, log_jump), the transported predecessor winning a tie and the jump coming from the previous
  frame's best cell J; score = fl32(scale * votes) + best, back = the predecessor's linear index ((r * Ho + a) * Wo +
  b), -1 where score is -inf.  stats = (M, largest score); count = (finite cells of score, NaN / +inf cells of
  score_prev, NaN / +inf cells of votes, cells entered by the jump, J, the lowest index of the largest score or -1).
  Only f32 additions, products and comparisons: bit for bit reproducible (the full contract: snap_vote_viterbi_f32 in
  include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume_arg('vote_viterbi', votes, 'votes')
  if score_prev is not None:
    _vote_volume_arg('vote_viterbi', score_prev, 'score_prev', votes)
  taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb = _vote_taps('vote_viterbi', log_taps, R, votes.device)
  scale, log_stay, log_jump = _vote_scale('vote_viterbi', scale), float(log_stay), float(log_jump)
  if not (log_stay <= 0.0 and log_jump <= 0.0):
    raise ValueError(f'vote_viterbi: log_stay and log_jump must be <= 0 (-inf allowed), got {log_stay}, {log_jump}')
  words = _workspace_words(lib.snap_vote_viterbi_workspace_bytes, (R, Ho, Wo, Tk, Ta, Tb), votes.numel(),
                           _vote_unsupported('vote_viterbi', R, Ho, Wo, (Tk, Ta, Tb)))
  ws = torch.empty((words,), dtype=torch.int64, device=votes.device)
  score = torch.empty((R, Ho, Wo), dtype=torch.float32, device=votes.device)
  back = torch.empty((R, Ho, Wo), dtype=torch.int32, device=votes.device)
  stats = torch.empty((2,), dtype=torch.float32, device=votes.device)
  count = torch.empty((6,), dtype=torch.int32, device=votes.device)
  # bytes the launches move (the kernel file's header): 10 passes over the volume with a score_prev, 3 without
  with _region('vote_viterbi', 0.0, 4.0 * votes.numel() * (3 if score_prev is None else 10)):
    st = lib.snap_vote_viterbi_f32(_p(score_prev), _p(votes), _p(taps_k), lk, _p(taps_a), _p(taps_b), _p(offsets),
                                   R, Ho, Wo, Tk, Ta, Tb, scale, log_stay, log_jump, _p(score), _p(back), _p(stats),
                                   _p(count), _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_viterbi_f32')
  return score, back, stats, count


def vote_backstep(back, cur):
  """One step back along ``vote_viterbi``'s back-pointers for B chains at once: back int32 [R, Ho, Wo] (a step's
  ``back``), cur int32 [B] linear indices on the same device -> prev int32 [B] = back.flatten()[cur], -1 where cur is
  outside [0, R Ho Wo) (a chain that has ended stays ended).  One small launch, no host synchronisation."""
  lib = _lib.load()
  _arg_chk(back, 'vote_backstep: back', (torch.int32,), (None, None, None), None,
           'vote_backstep: back int32 [R, Ho, Wo] on a ROCm GPU')
  _arg_chk(cur, 'vote_backstep: cur', (torch.int32,), (None,), back.device,
           f'vote_backstep: cur int32 [B] on {back.device}')
  n, B = back.numel(), cur.shape[0]
  if not (1 <= n < 2 ** 31 and 1 <= B < 2 ** 31):
    raise ValueError(f'vote_backstep: 1 <= R Ho Wo < 2^31 and 1 <= B < 2^31, got {n} cells and {B} chains')
  prev = torch.empty((B,), dtype=torch.int32, device=back.device)
  with _region('vote_backstep', 0.0, 12.0 * B):
    st = lib.snap_vote_backstep_i32(_p(back), n, _p(cur), _p(prev), B, _stream())
  _lib.check(st, 'snap_vote_backstep_i32')
  return prev


def _vote_draws(op, num, seed, stream, uniforms, device):
  """The draw arguments of ``vote_sample`` / ``vote_sample_back`` checked -> (B, seed, stream)."""
  for v, name, lo, hi in ((num, 'the number of draws', 1, 2 ** 20 + 1), (seed, 'seed', 0, 2 ** 64),
                          (stream, 'stream', -2 ** 31, 2 ** 31)):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) < hi:
      raise ValueError(f'{op}: {name} must be an integer in [{lo}, {hi}), got {v!r}')
  if uniforms is not None:
    _arg_chk(uniforms, f'{op}: uniforms', (torch.float64,), (int(num), 2), device,
             f'{op}: uniforms {torch.float64} {[int(num), 2]} on {device}')
  return int(num), int(seed), int(stream)


def vote_sample(votes, num, seed, stream=0, scale=1.0, uniforms=None):
  """``num`` independent draws from the pose distribution of a vote volume: votes f32 [R, Ho, Wo] (log-space; -inf =
  impossible) -> (index int32 [num], log_prob f32 [num], stats f32 [2], count int32 [2]) of p = softmax(scale * votes)
  with the filter's masses (cells more than 40 below the peak carry none).  index = the linear index
  (r * Ho + a) * Wo + b of the drawn cell, by the inverse CDF in lattice order (-1 for every draw when no cell has
  mass); log_prob = its normalised log-probability; stats = (log normaliser of scale * votes, largest scale * vote);
  count = (cells with mass, NaN / +inf cells).  Draw i uses the keyed Philox4x32-10 at counter (i, stream, 0, 0) with
  the 64-bit ``seed`` as key; ``uniforms`` float64 [num, 2] on the device replaces it (column 0 is used).  The same
  arguments give the same bytes (the full contract: snap_vote_sample_f32 in include/snap_hip.h).  No host
  synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume_arg('vote_sample', votes, 'votes')
  B, seed, stream = _vote_draws('vote_sample', num, seed, stream, uniforms, votes.device)
  scale = _vote_scale('vote_sample', scale)
  words = _workspace_words(lib.snap_vote_sample_workspace_bytes, (R, Ho, Wo), votes.numel(),
                           _vote_unsupported('vote_sample', R, Ho, Wo))
  ws = torch.empty((words,), dtype=torch.int64, device=votes.device)
  index = torch.empty((B,), dtype=torch.int32, device=votes.device)
  log_prob = torch.empty((B,), dtype=torch.float32, device=votes.device)
  stats = torch.empty((2,), dtype=torch.float32, device=votes.device)
  count = torch.empty((2,), dtype=torch.int32, device=votes.device)
  # bytes the launches move: two reads of the volume, the row sums written and folded, per draw a row of cells and
  # the sums above it
  with _region('vote_sample', 0.0, 8.0 * votes.numel() + 24.0 * R * Ho + B * (4.0 * Wo + 8.0 * (R + Ho) + 8.0)):
    st = lib.snap_vote_sample_f32(_p(votes), R, Ho, Wo, scale, B, seed, stream, _p(uniforms), _p(index), _p(log_prob),
                                  _p(stats), _p(count), _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_sample_f32')
  return index, log_prob, stats, count


def vote_sample_back(belief, nxt, taps, uniform_mix, seed, stream=0, uniforms=None):
  """One backward step of forward-filter / backward-sample for B chains: belief f32 [R, Ho, Wo] (``vote_filter``'s
  belief after frame t), nxt int32 [B] (the chains' linear indices at frame t + 1), taps and ``uniform_mix`` = what
  ``vote_filter`` was given for the step from t to t + 1 -> (prev int32 [B], jumped int32 [B], stats f32 [2], count
  int32 [3]).  prev is drawn from the exact conditional of the filter's transition given the chain's cell at t + 1: a
  cell of the tap window weighted by taps times the belief's mass, or -- the uniform-mix share -- a draw from the
  belief itself (jumped = 1).  prev = jumped = -1 where nxt is outside [0, R Ho Wo) (an ended chain stays ended) or
  nothing can precede the cell.  stats = (share of the belief's mass that stayed in the volume, largest finite
  belief); count = (chains with a predecessor, chains that jumped, NaN / +inf cells of belief).  Chain i uses Philox at
  counter (i, stream, 1, 0); ``uniforms`` float64 [B, 2] on the device replaces it (the full contract:
  snap_vote_sample_back_f32 in include/snap_hip.h).  No host synchronisation."""
  lib = _lib.load()
  R, Ho, Wo = _vote_volume_arg('vote_sample_back', belief, 'belief')
  _arg_chk(nxt, 'vote_sample_back: nxt', (torch.int32,), (None,), belief.device,
           f'vote_sample_back: nxt int32 [B] on {belief.device}')
  taps_k, lk, taps_a, taps_b, offsets, Tk, Ta, Tb = _vote_taps('vote_sample_back', taps, R, belief.device)
  B, seed, stream = _vote_draws('vote_sample_back', nxt.shape[0], seed, stream, uniforms, belief.device)
  uniform_mix = _vote_uniform_mix('vote_sample_back', uniform_mix)
  words = _workspace_words(lib.snap_vote_sample_back_workspace_bytes, (R, Ho, Wo, Tk, Ta, Tb), belief.numel(),
                           _vote_unsupported('vote_sample_back', R, Ho, Wo, (Tk, Ta, Tb)))
  ws = torch.empty((words,), dtype=torch.int64, device=belief.device)
  prev = torch.empty((B,), dtype=torch.int32, device=belief.device)
  jumped = torch.empty((B,), dtype=torch.int32, device=belief.device)
  stats = torch.empty((2,), dtype=torch.float32, device=belief.device)
  count = torch.empty((3,), dtype=torch.int32, device=belief.device)
  # bytes the launches move: the predict step's 8 passes over the volume (the filter's 12 less its update), one more
  # read for the row sums, and per chain its window of the belief
  with _region('vote_sample_back', 0.0, 4.0 * belief.numel() * 9 + 4.0 * B * Tk * Ta * Tb):
    st = lib.snap_vote_sample_back_f32(_p(belief), _p(taps_k), lk, _p(taps_a), _p(taps_b), _p(offsets), R, Ho, Wo, Tk,
                                       Ta, Tb, uniform_mix, _p(nxt), B, seed, stream, _p(uniforms), _p(prev),
                                       _p(jumped), _p(stats), _p(count), _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_vote_sample_back_f32')
  return prev, jumped, stats, count


def plane_align_score(fq, vq, fm, vm, poses, threshold):
  """The alignment score of two BEV planes at continuous poses: fq f32 [Hq, Wq, D] / vq bool or uint8 [Hq, Wq] (the
  query plane), fm f32 [Hm, Wm, D] / vm [Hm, Wm] (the map plane), poses f32 [P, 4] = (cos, sin, tx, ty) on the same
  device, the map <- query transform in corner frames with tx, ty in cells -> (score f32 [P], overlap int32 [P]).
  score = (sum over the valid query cells whose bilinear map sample is inside and has four valid taps of fq . the
  sampled fm) / (number of valid query cells) where more than ``threshold`` cells count, -inf elsewhere and for a
  non-finite pose row: ``template_finalize``'s normaliser and rule, so a score compares with a vote (the full contract:
  snap_plane_align_score_f32 in include/snap_hip.h).  No atomics, the same bits on every call and for every grouping
  of the poses.  No host synchronisation."""
  lib = _lib.load()
  _f32(fq, 'plane_align_score: fq'); _f32(fm, 'plane_align_score: fm')
  if fq.dim() != 3 or fm.dim() != 3 or fq.shape[-1] != fm.shape[-1]:
    raise ValueError(f'plane_align_score: fq [Hq, Wq, D] and fm [Hm, Wm, D], got {tuple(fq.shape)} / {tuple(fm.shape)}')
  Hq, Wq, D = fq.shape
  Hm, Wm = fm.shape[:2]
  for t, name, shape in ((vq, 'vq', (Hq, Wq)), (vm, 'vm', (Hm, Wm))):
    _arg_chk(t, f'plane_align_score: {name}', (torch.bool, torch.uint8), shape, fq.device,
             f'plane_align_score: {name} bool / uint8 {list(shape)} on {fq.device}')
  _arg_chk(poses, 'plane_align_score: poses', (torch.float32,), (None, 4), fq.device,
           f'plane_align_score: poses f32 [P, 4] and fm on {fq.device}', also=fm.device == fq.device,
           tail=f' / {fm.device}')
  P = poses.shape[0]
  threshold = float(threshold)
  if threshold != threshold:
    raise ValueError('plane_align_score: threshold is NaN')
  unsupported = (f'plane_align_score: unsupported query {Hq}x{Wq} map {Hm}x{Wm} D={D} P={P} (extents 1 .. 1024, '
                 'D % 4 == 0 with 4 <= D <= 128, 1 <= P < 2^20, 16-byte aligned planes)')
  if fq.data_ptr() % 16 or fm.data_ptr() % 16:
    raise ValueError(unsupported)
  words = _workspace_words(lib.snap_plane_align_score_workspace_bytes, (Hq, Wq, Hm, Wm, D, P), P, unsupported)
  ws = torch.empty((words,), dtype=torch.int64, device=fq.device)
  score = torch.empty((P,), dtype=torch.float32, device=fq.device)
  overlap = torch.empty((P,), dtype=torch.int32, device=fq.device)
  # algorithmic work: per pose and query cell, four taps of D channels, one multiply-add each (2 * 4 * D flop);
  # algorithmic bytes: both planes once, the poses, the outputs
  with _region('plane_align_score', 2.0 * 4 * P * Hq * Wq * D,
               4.0 * (fq.numel() + fm.numel()) + vq.numel() + vm.numel() + 24.0 * P):
    st = lib.snap_plane_align_score_f32(_p(fq), _p(vq), _p(fm), _p(vm), _p(poses), Hq, Wq, Hm, Wm, D, P, threshold,
                                        _p(score), _p(overlap), _p(ws), ws.numel() * 8, _stream())
  _lib.check(st, 'snap_plane_align_score_f32')
  return score, overlap


# Module attributes of the switches: aliases of the tuning in force (read) / the process default (write).
class _OpsModule(type(sys)):
  pass


for _name in _TUNING_DEFAULTS:
  setattr(_OpsModule, _name, property(
      lambda self, _n=_name: getattr(tuning(), _n),
      lambda self, v, _n=_name: object.__setattr__(_DEFAULT_TUNING, _n, v)))
sys.modules[__name__].__class__ = _OpsModule
