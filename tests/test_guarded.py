"""The guarded allocator (`tests/guarded.py`) can fail: every planted defect is reported, with its offset.

CPU tensors throughout; ``guarded.scope(..., device='cpu')`` sends CPU allocations through the guard.  The
module under the scope is a stand-in with a ``torch`` global, as ``snap_amd.ops`` has one."""
import types

import pytest
import torch

import guarded


def _module(name='fake_ops'):
  m = types.ModuleType(name)
  m.torch = torch
  exec(
      'def alloc(shape, dtype=torch.float32, device="cpu", **kw):\n'
      '  return torch.empty(shape, dtype=dtype, device=device, **kw)\n'
      'def alloc_like(t):\n'
      '  return torch.empty_like(t)\n'
      'def varargs(a, b):\n'
      '  return torch.empty(a, b, dtype=torch.int32, device="cpu")\n',
      m.__dict__)
  return m


def _raw(sc, i=0):
  return sc.records[i].buf


def test_clean_fill_passes_and_poison_reads_as_documented():
  m = _module()
  with guarded.scope(m, device='cpu') as sc:
    f = m.alloc((3, 5))
    h = m.alloc((7,), torch.bfloat16)
    i = m.varargs(2, 3)
    b = m.alloc((4,), torch.bool)
    assert torch.isnan(f).all() and torch.isnan(h.float()).all() and (i == -1).all()
    assert (b.view(torch.uint8) == 255).all()
    for t in (f, h, i, b):
      assert t.is_contiguous() and t.data_ptr() % 16 == 0
      assert guarded.unwritten(t).all()
    f.fill_(1.0); h.fill_(2.0); i.fill_(3); b.fill_(True)
    for t in (f, h, i, b):
      assert not guarded.unwritten(t).any()
    sc.check()
    assert len(sc.allocations()) == 4
    assert [tuple(v.shape) for v in sc.allocations(site='alloc')] == [(3, 5), (7,), (4,)]
    assert [tuple(v.shape) for v in sc.allocations(site='varargs')] == [(2, 3)]
    assert sc.allocations(site='alloc')[0].data_ptr() == f.data_ptr()


@pytest.mark.parametrize('dtype,numel', [(torch.float32, 5), (torch.bfloat16, 3), (torch.uint8, 9), (torch.int32, 4)])
def test_planted_writes_are_reported_with_their_offsets(dtype, numel):
  m = _module()
  item = torch.empty((), dtype=dtype).element_size()
  nbytes = numel * item
  # one element before the tensor
  with pytest.raises(guarded.GuardError) as e:
    with guarded.scope(m, device='cpu') as sc:
      t = m.alloc((numel,), dtype)
      t.fill_(0)
      _raw(sc)[guarded.PAD - item:guarded.PAD] = 0
  (d,) = e.value.damage
  assert (d['side'], d['first'], d['last']) == ('before', -item, -1)
  assert d['func'] == 'alloc' and d['shape'] == (numel,) and d['dtype'] == dtype
  assert f"{d['site']} (alloc)" in str(e.value) and f'bytes {-item} .. -1' in str(e.value)
  # one element after the rounded body, and one in the rounding gap between nbytes and round_up(nbytes, 16)
  body = (nbytes + 15) // 16 * 16
  for off in ([body] + ([nbytes] if body > nbytes else [])):
    sc = guarded.scope(m, device='cpu')
    with sc:
      t = m.alloc((numel,), dtype)
      t.fill_(0)
      _raw(sc)[guarded.PAD + off:guarded.PAD + off + item] = 0
      with pytest.raises(guarded.GuardError) as e:
        sc.check()
      (d,) = e.value.damage
      assert (d['side'], d['first'], d['last']) == ('after', off, off + item - 1)
      _raw(sc)[guarded.PAD + off:guarded.PAD + off + item] = guarded.POISON     # (repaired: the exit check passes)
  # both sides at once: two entries
  sc = guarded.scope(m, device='cpu')
  with pytest.raises(guarded.GuardError) as e:
    with sc:
      m.alloc((numel,), dtype)
      _raw(sc)[0] = 1
      _raw(sc)[-1] = 1
  assert [(d['side'], d['first'], d['last']) for d in e.value.damage] == [
      ('before', -guarded.PAD, -guarded.PAD), ('after', body + guarded.PAD - 1, body + guarded.PAD - 1)]


def test_a_skipped_element_is_found():
  m = _module()
  with guarded.scope(m, device='cpu'):
    t = m.alloc((4, 6))
    t.fill_(0.5)
    t[2, 5] = t.new_empty(()).fill_(0)          # written ...
    t.view(torch.uint8).reshape(4, 6, 4)[3, 1] = guarded.POISON      # ... and one left as it was allocated
    u = guarded.unwritten(t)
    assert u.sum() == 1 and u[3, 1]
    like = m.alloc_like(t.t())                 # a dense permuted tensor keeps its strides
    assert like.shape == (6, 4) and like.stride() == t.t().stride() and guarded.unwritten(like).all()
    # a genuine NaN a kernel computed is NOT the poison pattern
    t[0, 0] = float('nan')
    assert not guarded.unwritten(t)[0, 0]


@pytest.mark.parametrize('kind,byte', [('value', 0xFF), ('address', 0x00)])
def test_place_reproduces_the_bits(kind, byte):
  g = torch.Generator().manual_seed(0)
  for t in (torch.randn(5, 7, generator=g), torch.randn(3, 2, generator=g).to(torch.bfloat16),
            torch.randint(-5, 5, (11,), generator=g, dtype=torch.int32), torch.rand(13, generator=g) < 0.5,
            torch.randn(4, 6, generator=g).t(), torch.tensor([float('nan'), float('inf'), -0.0])):
    sc = guarded.scope(_module(), device='cpu')
    with sc:
      p = guarded.place(t, kind)
      assert p.shape == t.shape and p.dtype == t.dtype and p.is_contiguous() and p.data_ptr() % 16 == 0
      assert guarded.same_bits(p, t.contiguous())
      (r,) = sc.records
      assert (r.buf[:guarded.PAD] == byte).all() and (r.buf[guarded.PAD + r.nbytes:] == byte).all()
      # an in-place operand's guards are checked with the scope's buffers
      r.buf[guarded.PAD + r.nbytes] = 0x5A
      with pytest.raises(guarded.GuardError) as e:
        sc.check()
      assert e.value.damage[0]['what'] == 'input' and e.value.damage[0]['first'] == r.nbytes
      r.buf[guarded.PAD + r.nbytes] = byte
  # 'value' guards read as NaN right behind a float operand: an over-read poisons what it feeds
  p = guarded.place(torch.ones(3), 'value')
  assert torch.isnan(torch.as_strided(p, (4,), (1,))[3])
  p = guarded.place(torch.ones(3, dtype=torch.int32), 'address')
  assert torch.as_strided(p, (4,), (1,))[3] == 0


def test_proxy_delegates_and_leaves_the_global_module_alone():
  m = _module()
  real_empty = torch.empty
  with guarded.scope(m, device='cpu') as sc:
    assert m.torch is sc.proxy and m.torch is not torch
    assert sc.proxy.float32 is torch.float32 and sc.proxy.Tensor is torch.Tensor and sc.proxy.zeros is torch.zeros
    assert sc.proxy.cuda is torch.cuda
    assert torch.empty is real_empty
    assert not torch.isnan(torch.zeros(3)).any()
    with pytest.raises(AttributeError):
      sc.proxy.no_such_attribute
  assert m.torch is torch


def test_scope_restores_the_modules_after_an_exception():
  m, m2 = _module('a'), _module('b')
  with pytest.raises(KeyError):
    with guarded.scope(m, m2, device='cpu'):
      assert m.torch is not torch and m2.torch is not torch
      raise KeyError('boom')
  assert m.torch is torch and m2.torch is torch


def test_nested_scopes():
  m = _module()
  with guarded.scope(m, device='cpu') as outer:
    a = m.alloc((2,))
    with guarded.scope(m, device='cpu') as inner:
      b = m.alloc((3,))
      assert m.torch is inner.proxy
    assert m.torch is outer.proxy
    c = m.alloc((4,))
    assert [v.numel() for v in outer.allocations()] == [2, 4] and [v.numel() for v in inner.allocations()] == [3]
    assert guarded.unwritten(a).all() and guarded.unwritten(b).all() and guarded.unwritten(c).all()
  assert m.torch is torch


def test_default_modules_are_the_wrappers_and_cpu_allocations_pass_through():
  from snap_amd import autograd, ops, ops_bwd
  with guarded.scope() as sc:
    assert ops.torch is sc.proxy and ops_bwd.torch is sc.proxy and autograd.torch is sc.proxy
    assert type(ops).__name__ == '_OpsModule'
    t = ops.torch.empty(5, dtype=torch.float32)          # CPU, no device override: the real allocator
    assert not sc.records and t.shape == (5,)
  assert ops.torch is torch and ops_bwd.torch is torch and autograd.torch is torch


def test_a_pinned_allocation_passes_through():
  m = _module()
  with guarded.scope(m, device='cpu') as sc:
    try:
      t = m.alloc((8,), pin_memory=True)
    except RuntimeError:          # no accelerator runtime to pin with: the request still went to the real torch.empty
      t = None
    assert not sc.records
    assert t is None or t.is_pinned()
