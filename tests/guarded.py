"""A guarded, poisoned allocator for the kernel wrappers (test helper, not a conftest).

``with guarded.scope() as sc:`` replaces the name ``torch`` inside ``snap_amd.ops``, ``snap_amd.ops_bwd``
and ``snap_amd.autograd`` by a proxy whose ``empty`` / ``empty_like`` -- the only allocation forms the
wrappers use -- hand out the middle of a larger ``uint8`` buffer:

    [ PAD bytes 0xFF | the tensor, nbytes rounded up to 16, filled with 0xFF | PAD bytes 0xFF ]

so that

* a store before / after an output, workspace or statistics buffer lands in memory the test owns and
  is reported by ``sc.check()`` (also run on exit) with the allocating wrapper line and the damaged byte
  offsets relative to the tensor;
* an element a kernel never writes still holds the poison and is found by ``guarded.unwritten``: it
  cannot inherit the right answer from the block a previous call freed;
* ``guarded.place(t, kind)`` puts an INPUT between such guards: NaN bytes (``'value'``) around anything
  that is only multiplied, added or compared -- a load past its end then poisons the result --, zero
  bytes (``'address'``) around anything a kernel turns into an address or a branch, so that an
  over-read can never become a wild address (which costs the detection for those operands).

The poison is the byte 0xFF: NaN in f32 / bf16 / f16, -1 in the signed integer types, 255 in uint8 /
bool storage (compare bool results through a uint8 view).  The global ``torch`` module is not patched.
PAD = 4096 keeps the data pointer's 256-byte alignment, so no kernel changes its aligned / unaligned
variant.  CPU and pinned allocations pass through (``scope(device='cpu')`` guards CPU allocations: the
harness's own CPU tests).
"""
import importlib
import os
import sys
import threading

import numpy as np
import torch

PAD = 4096
POISON = 0xFF
GUARD_BYTE = {'value': 0xFF, 'address': 0x00}
DEFAULT_MODULES = ('snap_amd.ops', 'snap_amd.ops_bwd', 'snap_amd.autograd')

_THIS = os.path.abspath(__file__).rstrip('c')
_ACTIVE = []            # innermost scope last
_LOCK = threading.Lock()   # (the VJP wrappers allocate from autograd's backward threads)


class GuardError(AssertionError):
  """A guard region was written.  ``damage``: one dict per damaged region -- ``site`` ('file.py:line'),
  ``func``, ``shape``, ``dtype``, ``side`` ('before' | 'after'), ``first`` / ``last`` (byte offsets relative
  to the tensor's first byte: negative in front of it, >= nbytes behind it)."""

  def __init__(self, damage):
    self.damage = damage
    lines = [
        f"{d['what']} allocated at {d['site']} ({d['func']}), shape {d['shape']}, {d['dtype']}, {d['nbytes']} bytes: "
        f"guard {d['side']} the tensor damaged, bytes {d['first']} .. {d['last']} relative to the tensor"
        for d in damage]
    super().__init__('guard regions were written:\n  ' + '\n  '.join(lines))


class Record:
  """One guarded buffer: ``view`` is what the caller got, ``buf`` the whole uint8 buffer."""
  __slots__ = ('buf', 'view', 'nbytes', 'guard', 'file', 'line', 'func', 'what')

  @property
  def site(self):
    return f'{os.path.basename(self.file)}:{self.line}'

  def matches(self, site):
    if site is None:
      return True
    base = os.path.basename(self.file)
    return site in (self.func, self.site, f'{base}:{self.func}', base)


def _round_up(n, m):
  return (n + m - 1) // m * m


def _call_site():
  f = sys._getframe(1)
  while f is not None and os.path.abspath(f.f_code.co_filename).rstrip('c') == _THIS:
    f = f.f_back
  if f is None:
    return '?', 0, '?'
  return f.f_code.co_filename, f.f_lineno, f.f_code.co_name


def _new_record(shape, dtype, device, guard, what):
  shape = tuple(int(s) for s in shape)
  itemsize = torch.empty((), dtype=dtype).element_size()
  nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize if len(shape) else itemsize
  body = _round_up(nbytes, 16)
  buf = torch.empty(PAD + body + PAD, dtype=torch.uint8, device=device)   # the real torch.empty
  buf.fill_(guard)
  buf[PAD:PAD + body] = POISON if what != 'input' else guard
  r = Record()
  r.buf, r.nbytes, r.guard, r.what = buf, nbytes, guard, what
  r.view = buf[PAD:PAD + nbytes].view(dtype).view(shape)
  r.file, r.line, r.func = _call_site()
  return r


def _sizes(size):
  if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
    return tuple(size[0])
  return tuple(size)


class _TorchProxy:
  """Delegates every attribute to the real ``torch`` except ``empty`` and ``empty_like``."""

  def __init__(self, scope):
    object.__setattr__(self, '_scope', scope)

  def __getattr__(self, name):
    return getattr(torch, name)

  def __setattr__(self, name, value):
    raise AttributeError('the torch proxy is read-only')

  def empty(self, *size, dtype=None, device=None, pin_memory=False, requires_grad=False, **kw):
    sc = self._scope
    dev = torch.device(device) if device is not None else torch.empty(0).device
    if pin_memory or kw or not sc._guards(dev):
      return torch.empty(*size, dtype=dtype, device=device, pin_memory=pin_memory, requires_grad=requires_grad, **kw)
    r = _new_record(_sizes(size), dtype or torch.get_default_dtype(), dev, POISON, 'buffer')
    sc._add(r)
    return r.view.requires_grad_() if requires_grad else r.view

  def empty_like(self, t, *, dtype=None, device=None, pin_memory=False, requires_grad=False, **kw):
    sc = self._scope
    dev = torch.device(device) if device is not None else t.device
    if pin_memory or kw or not sc._guards(dev):
      return torch.empty_like(t, dtype=dtype, device=device, pin_memory=pin_memory, requires_grad=requires_grad, **kw)
    r = _new_record(t.shape, dtype or t.dtype, dev, POISON, 'buffer')
    if not t.is_contiguous():     # (torch.empty_like keeps the strides of a dense permuted tensor)
      like = torch.empty_like(t, device='meta')
      r.view = r.view.reshape(-1).as_strided(like.shape, like.stride())
    sc._add(r)
    return r.view.requires_grad_() if requires_grad else r.view


class scope:
  """Context manager: see the module docstring.  ``modules``: module objects or dotted names (default:
  ``DEFAULT_MODULES``); ``device='cpu'`` sends allocations on that device type through the guard as well
  (device allocations always are)."""

  def __init__(self, *modules, device=None):
    self._names = modules or DEFAULT_MODULES
    self._extra = None if device is None else torch.device(device).type
    self.records = []
    self.proxy = _TorchProxy(self)
    self._saved = None

  def _guards(self, dev):
    return dev.type == 'cuda' or dev.type == self._extra

  def _add(self, r):
    with _LOCK:
      self.records.append(r)

  def __enter__(self):
    mods = [importlib.import_module(m) if isinstance(m, str) else m for m in self._names]
    self._saved = []
    for m in mods:
      self._saved.append((m, m.__dict__.get('torch', torch)))
      setattr(m, 'torch', self.proxy)
    _ACTIVE.append(self)
    return self

  def __exit__(self, exc_type, exc, tb):
    _ACTIVE.remove(self)
    for m, prev in reversed(self._saved):
      setattr(m, 'torch', prev)
    self._saved = None
    if exc_type is None:
      self.check()
    return False

  def allocations(self, site=None):
    """The views allocated (through the proxy) at ``site``: a wrapper's name ('compact_rows'), a line
    ('ops.py:1145'), 'ops.py:compact_rows' or a file name; None: all of them, in allocation order."""
    return [r.view for r in self.records if r.what == 'buffer' and r.matches(site)]

  def check(self):
    """Synchronise, then assert that both guard regions of every buffer still hold their guard byte."""
    recs = list(self.records)
    if not recs:
      return
    if any(r.buf.is_cuda for r in recs):
      torch.cuda.synchronize()
    flags = []
    for r in recs:
      end = PAD + r.nbytes
      flags.append(torch.stack([(r.buf[:PAD] != r.guard).any(), (r.buf[end:] != r.guard).any()]))
    by_dev = {}
    for i, f in enumerate(flags):
      by_dev.setdefault(f.device, []).append(i)
    bad = {}
    for dev, idx in by_dev.items():
      host = torch.stack([flags[i] for i in idx]).cpu().numpy()
      for i, row in zip(idx, host):
        if row.any():
          bad[i] = row
    if not bad:
      return
    damage = []
    for i in sorted(bad):
      r = recs[i]
      end = PAD + r.nbytes
      for side, lo, hi, flag in (('before', 0, PAD, bad[i][0]), ('after', end, r.buf.numel(), bad[i][1])):
        if not flag:
          continue
        hit = (r.buf[lo:hi] != r.guard).nonzero().reshape(-1)
        first, last = int(hit[0]) + lo - PAD, int(hit[-1]) + lo - PAD
        damage.append(dict(what=r.what, site=r.site, func=r.func, shape=tuple(r.view.shape), dtype=r.view.dtype,
                           nbytes=r.nbytes, side=side, first=first, last=last))
    raise GuardError(damage)


def place(t, kind, scope=None):
  """A bit-for-bit, contiguous copy of ``t`` in the middle of a guarded buffer.  ``kind``: 'value' (NaN
  guards: anything only multiplied, added or compared) | 'address' (zero guards: anything a kernel turns
  into an address or a branch).  The buffer joins ``scope`` (default: the innermost active one, if any),
  whose ``check()`` then also covers it: an in-place operand's guards must hold."""
  guard = GUARD_BYTE[kind]
  src = t.detach().contiguous()
  r = _new_record(src.shape, src.dtype, src.device, guard, 'input')
  if r.nbytes:
    r.view.reshape(-1).view(torch.uint8).copy_(src.reshape(-1).view(torch.uint8))
  sc = scope if scope is not None else (_ACTIVE[-1] if _ACTIVE else None)
  if sc is not None:
    sc._add(r)
  else:
    r.view._guarded_record = r
  return r.view


def unwritten(t):
  """Boolean mask (``t``'s shape) of the elements whose bytes are all still the poison 0xFF."""
  if t.element_size() == 1:
    return t.view(torch.uint8) == POISON
  raw = t.contiguous().reshape(-1).view(torch.uint8).reshape(*t.shape, t.element_size())
  return (raw == POISON).all(dim=-1)


def same_bits(a, b):
  """True when ``a`` and ``b`` (same shape and dtype) hold the same bytes, NaN payloads included."""
  if a.shape != b.shape or a.dtype != b.dtype:
    return False
  if a.element_size() == 1:
    return bool((a.view(torch.uint8) == b.view(torch.uint8)).all())
  return bool((a.contiguous().reshape(-1).view(torch.uint8) == b.contiguous().reshape(-1).view(torch.uint8)).all())
