"""`-m gpu`: every kernel writes all of its output and nothing else, and reads nothing it was not given.

Every case has one form (``contained``): the wrapper runs once normally, then again on the same values inside
``guarded.scope()`` with every tensor input copied between guards (``guarded.place``).  Inside the scope every
``torch.empty`` / ``torch.empty_like`` of the wrappers -- outputs, workspaces, statistics buffers, weight images --
is the middle of a buffer of 0xFF bytes.  Asserted: both guard regions of every buffer are intact; the guarded run
equals the normal run BIT FOR BIT on every returned tensor and every in-place operand; no returned element still
holds the poison; elements the op promises to leave alone still do.  The values are checked against the oracle
elsewhere; the one tolerance in this file is `test_pose_score_bwd`'s own (2e-4, 1e-4), for the float-atomic
`mask_oob` form of the pose-score VJP, which has no repeatable order.

What the guards around INPUTS detect: ``'value'`` operands (activations, weights, statistics, cotangents ...) sit
between NaN bytes, so a load past either end that is multiplied by zero or masked late still poisons the result
and breaks the bit comparison.  ``'address'`` operands (row lists, counts, masks, validity bytes, points, poses,
cameras) sit between ZERO bytes so that an over-read can never turn into a wild address or a taken branch; an
over-read of those is therefore only caught where a zero changes the result.  Integer results equal to -1 and
uint8 results equal to 255 cannot be told from the poison; such elements are accepted because the normal run has
the same bits there.
"""
import ctypes

import numpy as np
import pytest
import torch

import guarded
import helpers
import oracle_ops
from snap_amd import _lib, ops, ops_bwd
from test_gpu_kernels import CONV_CASES, HALO_CASES, MLP_POOL_CASES, _lift_scene, rnd
from test_gpu_presplit import PS_CASES
from test_gpu_occupancy import CELL as OCC_CELL, _mlp_params, _rays, _volume as _occ_volume

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
ENGINES = ['f32', 'bf16x3', 'bf16x6', 'bf16', 'fp16']
TILES = ['128x128', '128x64', '64x128', '64x64']
V, A = 'value', 'address'


def dev(t):
  return t.to(DEV).contiguous()


def _flatten(res, prefix='out'):
  """(name, tensor) of everything a wrapper handed back: nested tuples / lists, PreSplit / PackedWeights, the
  statistics a conv result carries as attributes."""
  out = []
  if res is None:
    return out
  if isinstance(res, torch.Tensor):
    out.append((prefix, res))
    for attr in ('_snap_gn_partial', '_snap_gn_partial_relu', '_snap_gnb_partial'):
      held = getattr(res, attr, None)
      if held is not None:
        out.append((prefix + '.' + attr, held[0]))
    twin = getattr(res, '_snap_half_twin', None)
    if twin is not None:
      out.append((prefix + '._snap_half_twin', twin[0]))
    return out
  if isinstance(res, (ops.PreSplit, ops.PackedWeights)):
    out.append((prefix + '.data', res.data))
    if getattr(res, 'stats', None) is not None:
      out += _flatten(res.stats, prefix + '.stats')
    return out
  if isinstance(res, (tuple, list)):
    for i, r in enumerate(res):
      out += _flatten(r, f'{prefix}[{i}]')
    return out
  return out          # (host scalars)


def assert_same(ref, got, leave=None, ignore=None, tol=None):
  """Bit equality and no poison on every returned tensor.  ``leave``: {name: bool mask} of elements the op
  promises NOT to write -- those must still be poison in the guarded run, everything else written and equal.
  ``ignore``: {name: mask} of elements the op makes no promise about (not looked at).  The partial-sum buffers a
  conv result carries are sized for the largest tile plan and written as far as the launch's own plan goes: what
  is written must be bit-equal, and ``_statistics_consumers`` shows that nothing else is ever read AT THIS SHAPE: a
  launch that wrote too few partial sums is caught only where the finalising pass reads the missing slot.
  Integer / uint8 results are held to bit equality alone (-1 / 255 cannot be told from poison).
  ``tol`` = (atol, rtol): a float-atomic form without a repeatable order -- the tolerance of its existing test."""
  fr, fg = _flatten(ref), _flatten(got)
  assert [n for n, _ in fr] == [n for n, _ in fg], ([n for n, _ in fr], [n for n, _ in fg])
  leave, ignore = leave or {}, ignore or {}
  for (name, a), (_, b) in zip(fr, fg):
    assert a.shape == b.shape and a.dtype == b.dtype, name
    un = guarded.unwritten(b)
    if name in leave:
      keep = leave[name].expand(b.shape) if leave[name].shape != b.shape else leave[name]
      assert bool(un[keep].all()), f'{name}: {int((~un[keep]).sum())} element(s) the op promises to leave alone were written'
      a, b, un = a[~keep], b[~keep], un[~keep]
    if name in ignore:
      sel = ~(ignore[name].expand(b.shape) if ignore[name].shape != b.shape else ignore[name])
      a, b, un = a[sel], b[sel], un[sel]
    if '_snap_gn' in name:
      assert not bool(un.all()), f'{name}: nothing written'
      a, b, un = a[~un], b[~un], un[~un]
    if b.dtype.is_floating_point:
      n = int(un.sum())
      assert n == 0, f'{name}: {n} of {un.numel()} element(s) never written, first at flat index {int(un.reshape(-1).nonzero()[0])}'
    if tol is not None:
      helpers.report(name, b, a.cpu(), atol=tol[0], rtol=tol[1])
      continue
    if not guarded.same_bits(a, b):
      diff = (a.contiguous().reshape(-1).view(torch.uint8).reshape(a.numel(), -1) != b.contiguous().reshape(-1).view(torch.uint8).reshape(b.numel(), -1)).any(-1)
      idx = diff.nonzero().reshape(-1)
      raise AssertionError(f'{name}: the guarded run differs from the normal run in {idx.numel()} of {a.numel()} element(s), '
                           f'first flat index {int(idx[0])}, last {int(idx[-1])}; poisoned there: {int(un.reshape(-1)[idx].sum())}')


def _statistics_consumers(ref, got):
  """Every conv result that carries fused GroupNorm partial sums goes through the pass that reads them, inside the
  scope: the finalised statistics are bit-equal to the normal run's and hold no NaN -- the unwritten part of the
  partial-sum buffer (poison here) is never read."""
  for (name, a), (_, b) in zip(_flatten(ref), _flatten(got)):
    held = getattr(a, '_snap_gn_partial', None)
    if held is None or a.dim() != 4 or not a.dtype.is_floating_point:
      continue
    gamma = torch.ones(a.shape[-1], device=a.device)
    kinds = {bool(held[2])} | ({True} if getattr(a, '_snap_gn_partial_relu', None) is not None else set())
    for relu_first in kinds:
      want = ops.group_norm_stats(a, gamma, relu_first=relu_first, want_rstd=True)
      have = ops.group_norm_stats(b, gamma, relu_first=relu_first, want_rstd=True)
      assert_same(want, have)
      assert not any(bool(torch.isnan(t).any()) for t in have), name


def contained(fn, args, kinds, inplace=(), leave=None, ignore=None, tol=None):
  """fn(*tensors) on device tensors ``args`` (``kinds`` parallel: 'value' | 'address'; None entries pass through).
  ``inplace``: indices of operands the op modifies -- compared like results.  Returns (ref, got, scope)."""
  assert len(args) == len(kinds)
  first = [t.clone() if i in inplace else t for i, t in enumerate(args)]
  ref = fn(*first)
  torch.cuda.synchronize()
  with guarded.scope() as sc:
    placed = [None if t is None else guarded.place(t, k) for t, k in zip(args, kinds)]
    got = fn(*placed)
    sc.check()
    assert_same(ref, got, leave, ignore, tol)
    _statistics_consumers(ref, got)
    sc.check()
    for i, (t, p) in enumerate(zip(args, placed)):
      if t is None:
        continue
      want = first[i] if i in inplace else t
      assert guarded.same_bits(want, p), f'operand {i}: ' + ('in-place result differs' if i in inplace else 'an input was modified')
  return ref, got, sc


# ----------------------------------------------------------------------------------------------------
# the harness on device memory (no kernel involved)
# ----------------------------------------------------------------------------------------------------
def test_planted_writes_on_a_device_buffer():
  for off, side in ((-4, 'before'), (40, 'after'), (48, 'after')):      # 10 floats: 40 bytes, rounded to 48
    sc = guarded.scope()
    with sc:
      t = ops.torch.empty(10, dtype=torch.float32, device=DEV)
      assert t.is_cuda and t.data_ptr() % 256 == 0 and bool(torch.isnan(t).all())
      t.fill_(1.0)
      sc.check()
      raw = sc.records[0].buf
      raw[guarded.PAD + off:guarded.PAD + off + 4] = 0
      with pytest.raises(guarded.GuardError) as e:
        sc.check()
      (d,) = e.value.damage
      assert (d['side'], d['first'], d['last']) == (side, off, off + 3) and 'test_gpu_containment.py' in d['site']
      raw[guarded.PAD + off:guarded.PAD + off + 4] = guarded.POISON
    assert ops.torch is torch
  with guarded.scope():
    t = ops.torch.empty((4, 5), dtype=torch.float32, device=DEV)
    t[:, :4] = 0.0
    assert guarded.unwritten(t).sum() == 4 and bool(guarded.unwritten(t)[:, 4].all())
    p = guarded.place(torch.arange(7, dtype=torch.int32, device=DEV), A)
    assert int(torch.as_strided(p, (8,), (1,))[7]) == 0


def test_pinned_and_host_allocations_pass_through():
  with guarded.scope() as sc:
    t = ops.torch.empty(8, dtype=torch.float32, pin_memory=True)
    h = ops.torch.empty(8, dtype=torch.float32)
    assert t.is_pinned() and not t.is_cuda and not h.is_cuda and not sc.records


def test_empty_operands_are_still_refused():
  """The entries test the operand's own (null) pointer before the workspace: an empty tensor was refused while the
  workspaces carried four spare elements and still is -- the spare elements never made such a call work."""
  with pytest.raises(RuntimeError):
    ops_bwd.colsum(torch.empty((0, 12), device=DEV))
  with pytest.raises(RuntimeError):
    ops_bwd.layer_norm_bwd(torch.empty((0, 8), device=DEV), torch.empty((0, 8), device=DEV), torch.ones(8, device=DEV))


# ----------------------------------------------------------------------------------------------------
# conv / dense engine
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('math', ENGINES)
@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_cases(case, math):
  _, N, H, W, Cin, KH, KW, Cout, stride, pad = case
  x = dev(rnd((N, H, W, Cin), 1))
  w = dev(rnd((KH, KW, Cin, Cout), 2, 1.0 / np.sqrt(KH * KW * Cin)))
  contained(lambda x, w: ops.conv2d(x, w, stride=stride, padding=((pad, pad), (pad, pad)), math=math), [x, w], [V, V])


@pytest.mark.parametrize('math,bk', [('f32', 16), ('f32', 32), ('bf16x3', None), ('bf16x6', None), ('bf16', None), ('fp16', None)])
@pytest.mark.parametrize('tile', TILES)
def test_conv_every_tile_variant(tile, math, bk):
  """2 x 15 x 13, 96 -> 200, 3 x 3, GroupNorm prologue, residual + bias + ReLU: M, N and K tails under every tile."""
  N, H, W, Cin, Cout = 2, 15, 13, 96, 200
  x = rnd((N, H, W, Cin), 31) + 0.2
  w = rnd((3, 3, Cin, Cout), 32, 1 / np.sqrt(9 * Cin))
  gamma, beta = rnd((Cin,), 33) + 1, rnd((Cin,), 34) * 0.1
  mu, sc = oracle_ops.group_norm_stats(x, gamma)
  res, bias = rnd((N, H, W, Cout), 35), rnd((Cout,), 36)
  with ops.tuning_scope(CONV_TILE=tile, CONV_BK=bk):
    contained(lambda x, w, mu, sc, beta, res, bias: ops.conv2d(
        x, w, padding=((1, 1), (1, 1)), prologue=ops.PRO_GN_RELU, gn=(mu, sc, beta), residual=res, bias=bias, relu=True,
        math=math), [dev(t) for t in (x, w, mu, sc, beta, res, bias)], [V] * 7)


@pytest.mark.parametrize('math', ENGINES)
def test_dense_k257_pad_columns_do_not_reach_the_result(math):
  """cin = 257 on rows of stride 260: NaN planted in the three pad columns of every row."""
  x = rnd((700, 260), 37)
  w = dev(rnd((257, 256), 38, 1 / 16.0))
  clean = ops.dense(dev(x), w, cin=257, math=math)
  x[:, 257:] = float('nan')
  ref, got, _ = contained(lambda x, w: ops.dense(x, w, cin=257, math=math), [dev(x), w], [V, V])
  assert guarded.same_bits(clean, got) and not bool(torch.isnan(got).any())


@pytest.mark.parametrize('math', ENGINES)
def test_dense_out_stride_leaves_the_gap_columns(math):
  M, Cin, Cout, stride = 117, 20, 36, 44
  x, w, b = dev(rnd((M, Cin), 3)), dev(rnd((Cin, Cout), 4, 0.2)), dev(rnd((Cout,), 5))
  ref = ops.dense(x, w, b, math=math, out=torch.zeros(M, stride, device=DEV), out_stride=stride)
  with guarded.scope() as sc:
    out = ops.torch.empty((M, stride), dtype=torch.float32, device=DEV)
    got = ops.dense(guarded.place(x, V), guarded.place(w, V), guarded.place(b, V), math=math, out=out, out_stride=stride)
    sc.check()
    assert got is out
    un = guarded.unwritten(out)
    assert not bool(un[:, :Cout].any()) and bool(un[:, Cout:].all())
    assert guarded.same_bits(ref[:, :Cout].contiguous(), out[:, :Cout].contiguous())


@pytest.mark.parametrize('math', ENGINES)
def test_dense_row_lists_with_a_shorter_device_count(math):
  """rows_in / rows_out with row_count < len(list): unlisted output rows and rows beyond the count stay poison.
  (The lists are 'address' operands: zero guards.)"""
  M, Cin, Cout = 198, 20, 36
  g = torch.Generator().manual_seed(7)
  x, w, b = dev(rnd((M, Cin), 8)), dev(rnd((Cin, Cout), 9, 0.2)), dev(rnd((Cout,), 10))
  perm = torch.randperm(M, generator=g)[:150].to(torch.int32)
  n = 77
  rows, count = dev(perm), torch.tensor([n], dtype=torch.int32, device=DEV)
  ref = ops.dense(x, w, b, relu=True, rows_in=rows, rows_out=rows, row_count=count, out=torch.zeros(M, Cout, device=DEV), math=math)
  listed = torch.zeros(M, dtype=torch.bool, device=DEV)
  listed[rows[:n].long()] = True
  with guarded.scope() as sc:
    out = ops.torch.empty((M, Cout), dtype=torch.float32, device=DEV)
    ops.dense(guarded.place(x, V), guarded.place(w, V), guarded.place(b, V), relu=True, rows_in=guarded.place(rows, A),
              rows_out=guarded.place(rows, A), row_count=guarded.place(count, A), out=out, math=math)
    sc.check()
    un = guarded.unwritten(out)
    assert not bool(un[listed].any()) and bool(un[~listed].all())
    assert guarded.same_bits(ref[listed], out[listed])


@pytest.mark.parametrize('math', ['bf16', 'fp16'])
def test_dense_out_half(math):
  x, w, b = dev(rnd((117, 20), 11)), dev(rnd((20, 36), 12, 0.2)), dev(rnd((36,), 13))
  ref, got, _ = contained(lambda x, w, b: ops.dense(x, w, b, relu=True, math=math, out_half=True), [x, w, b], [V] * 3)
  assert got.dtype == (torch.bfloat16 if math == 'bf16' else torch.float16)


@pytest.mark.parametrize('math', ENGINES)
def test_conv_row_mask(math):
  x, w = dev(rnd((1, 1, 198, 64), 14)), dev(rnd((1, 1, 64, 160), 15, 0.1))
  mask = dev(torch.rand(198, generator=torch.Generator().manual_seed(16)) > 0.4)
  contained(lambda x, w, m: ops.conv2d(x, w, row_mask=m, math=math), [x, w, mask], [V, V, A])


@pytest.mark.parametrize('stats', [None, 'raw', 'relu'])
@pytest.mark.parametrize('math', ENGINES)
@pytest.mark.parametrize('shape', [(3, 17, 19, 512, 512, 3), (5, 9, 7, 1024, 256, 1)])
def test_split_k_workspace_and_statistics(shape, math, stats):
  """Deep reductions over few rows: the split-K workspace and (with statistics) the partial-sum buffers are
  guarded allocations of the wrapper; the statistics a result carries are compared like results."""
  N, H, W, Cin, Cout, k = shape
  x = dev(rnd((N, H, W, Cin), 1200 + Cin))
  w = dev(rnd((k, k, Cin, Cout), 1201 + Cout, 1 / np.sqrt(k * k * Cin)))
  res, b_in = dev(rnd((N, H, W, Cout), 1202)), dev(rnd((Cin,), 1204) * 0.3)
  mu, sc = ops.group_norm_stats(x, dev(rnd((Cin,), 1203) * 0.3 + 1))
  pad = ((k // 2, k // 2), (k // 2, k // 2))
  contained(lambda x, w, mu, sc, b, res: ops.conv2d(x, w, padding=pad, prologue=ops.PRO_GN_RELU, gn=(mu, sc, b), residual=res,
                                                    math=math, emit_gn_stats=stats), [x, w, mu, sc, b_in, res], [V] * 6)


@pytest.mark.parametrize('math', ['f32', 'bf16x3', 'bf16x6'])
def test_conv_emits_both_groupnorm_statistics(math):
  N, H, W, Cin, Cout = 3, 97, 120, 64, 256
  x, w, res = dev(rnd((N, H, W, Cin), 950)), dev(rnd((1, 1, Cin, Cout), 951, 1 / 8.0)), dev(rnd((N, H, W, Cout), 952))
  mu, sc = ops.group_norm_stats(x, dev(rnd((Cin,), 954) + 1))
  b_in = dev(rnd((Cin,), 955))
  ref, got, _ = contained(lambda x, w, mu, sc, b, res: ops.conv2d(x, w, prologue=ops.PRO_GN_RELU, gn=(mu, sc, b), residual=res, math=math,
                                                                  emit_gn_stats='both'), [x, w, mu, sc, b_in, res], [V] * 6)
  assert hasattr(got, '_snap_gn_partial') and hasattr(got, '_snap_gn_partial_relu') == (math != 'f32')
  # the statistics pass that reads them
  gamma = dev(rnd((Cout,), 953) + 1)
  for relu_first in (False, True):
    want = ops.group_norm_stats(ref, gamma, relu_first=relu_first, want_rstd=True)
    with guarded.scope() as sc:
      have = ops.group_norm_stats(got, guarded.place(gamma, V), relu_first=relu_first, want_rstd=True)
      sc.check()
      assert_same(want, have)


@pytest.mark.parametrize('math', ['bf16x6', 'bf16x3'])
@pytest.mark.parametrize('N,H,W,Cin,Cout,gn,extras', HALO_CASES)
def test_conv_split_halo_3x3(N, H, W, Cin, Cout, gn, extras, math):
  x = rnd((N, H, W, Cin), 500 + W) + 0.1
  w = rnd((3, 3, Cin, Cout), 501, 1 / np.sqrt(9 * Cin))
  args, kw = [dev(x), dev(w)], dict(padding=((1, 1), (1, 1)), math=math)
  if gn:
    gamma, beta = rnd((Cin,), 502) + 1, rnd((Cin,), 503) * 0.1
    mu, sc = oracle_ops.group_norm_stats(x, gamma, groups=min(32, Cin // 2))
    args += [dev(mu), dev(sc), dev(beta)]
  if extras:
    args += [dev(rnd((N, H, W, Cout), 504)), dev(rnd((Cout,), 505))]
  if not extras and Cout % 32 == 0:
    kw['emit_gn_stats'] = 'raw'

  def run(x, w, *rest):
    rest = list(rest)
    k = dict(kw)
    if gn:
      k.update(prologue=ops.PRO_GN_RELU, gn=tuple(rest[:3]))
      rest = rest[3:]
    if extras:
      k.update(residual=rest[0], bias=rest[1], relu=True)
    return ops.conv2d(x, w, **k)

  with ops.tuning_scope(USE_SPLITK=False):
    contained(run, args, [V] * len(args))


@pytest.mark.parametrize('math', ENGINES)
def test_conv_rgb_root_and_scalar_root(math):
  x = torch.rand((1, 96, 80, 4), generator=torch.Generator().manual_seed(980))
  x[..., 3] = 0.37
  w = dev(rnd((7, 7, 3, 32), 901, 1 / np.sqrt(147)))
  contained(lambda x, w: ops.conv2d(x, w, stride=2, padding=((3, 3), (3, 3)), cin=3, math=math, prologue=ops.PRO_AFFINE,
                                    in_affine=(2.0, -1.0)), [dev(x), w], [V, V])
  x3 = dev(torch.rand((1, 20, 18, 3), generator=torch.Generator().manual_seed(39)))
  w3 = dev(rnd((7, 7, 3, 64), 40, 0.1))
  contained(lambda x, w: ops.conv2d(x, w, stride=2, padding=((3, 3), (3, 3)), math=math), [x3, w3], [V, V])


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('Cin', [64, 128, 256])
def test_stationary_1x1_kernels_on_99_pixel_images(Cin, relu):
  """conv_rs.hip at images of 99 pixels (most 32-row tiles straddle two images), with the statistics they emit."""
  N, H, W, Cout = 5, 9, 11, 256
  x, w = dev(rnd((N, H, W, Cin), 70 + Cin)), dev(rnd((1, 1, Cin, Cout), 71, 1 / np.sqrt(Cin)))
  mu, sc = ops.group_norm_stats(x, dev(rnd((Cin,), 72) + 1))
  beta = dev(rnd((Cin,), 73) * 0.1)
  for force in (False, True):
    with ops.tuning_scope(CONV_RS_FORCE=force):
      contained(lambda x, w, mu, sc, b: ops.conv2d(x, w, prologue=ops.PRO_GN_RELU, gn=(mu, sc, b), math='bf16x3',
                                                   emit_gn_stats='relu' if relu else 'raw'), [x, w, mu, sc, beta], [V] * 5)


@pytest.mark.parametrize('M,K,N', [(20, 16, 4), (300, 192, 256)])
def test_one_part_ring_engine(M, K, N):
  x = dev(rnd((M, K), 80)).to(torch.bfloat16)
  w, b = dev(rnd((K, N), 81, 1 / np.sqrt(K))), dev(rnd((N,), 82))
  contained(lambda x, w, b: ops.dense(x, w, b, math='bf16', bf16_ring=True), [x, w, b], [V] * 3)
  contained(lambda x, w, b: ops.dense(x, w, b, math='bf16', bf16_ring=True, out_half=True, gelu=True), [x, w, b], [V] * 3)


@pytest.mark.parametrize('ps_tile', [1, 2])
@pytest.mark.parametrize('N,H,W,Cin,k,Cout,stride,res', PS_CASES)
def test_presplit_engine_and_its_producer(N, H, W, Cin, k, Cout, stride, res, ps_tile):
  x, w = dev(rnd((N, H, W, Cin), 90)), dev(rnd((k, k, Cin, Cout), 91, 1 / np.sqrt(k * k * Cin)))
  pad = ((k // 2, k // 2), (k // 2, k // 2))
  Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
  r = dev(rnd((N, Ho, Wo, Cout), 92)) if res else None

  def run(x, w, r):
    ps = ops.presplit(x)
    return ps, ops.conv2d(ps, w, stride=stride, padding=pad, residual=r, relu=True, emit_gn_stats='raw', ps_tile=ps_tile)

  with ops.engine_scope('bf16x3'):
    assert ops.conv2d_presplit_supported(x.shape, w.shape, stride, pad)
    contained(run, [x, w, r], [V] * 3)


@pytest.mark.parametrize('N,H,W,C', [(2, 40, 36, 64), (3, 17, 17, 512), (5, 12, 12, 128)])
def test_gn_norm_split_with_stats(N, H, W, C):
  x, w = dev(rnd((N, H, W, 32), 93)), dev(rnd((1, 1, 32, C), 94, 1 / np.sqrt(32.0)))
  gamma, beta = dev(rnd((C,), 95) * 0.3 + 1), dev(rnd((C,), 96) * 0.2)
  with ops.engine_scope('bf16x3'), ops.tuning_scope(USE_SPLITK=False):
    y = ops.conv2d(x, w, emit_gn_stats='raw')
    ref = ops.gn_norm_split(y, gamma, beta, want_stats=True)
    assert ref is not None
    with guarded.scope() as sc:
      yg = ops.conv2d(guarded.place(x, V), guarded.place(w, V), emit_gn_stats='raw')
      got = ops.gn_norm_split(yg, guarded.place(gamma, V), guarded.place(beta, V), want_stats=True)
      sc.check()
      assert_same((y, ref), (yg, got))


PROBE = 1.0 + 2.0 ** -9 + 2.0 ** -18       # bf16 parts 1, 2^-9, 2^-18: no part of a live element is zero


def _zero_padded(image, live):
  """A weight image is 'zero padded' by contract: every element is written and the padding is zero."""
  assert not bool(guarded.unwritten(image).any())
  assert bool((image.view(torch.int16)[~live] == 0).all())


@pytest.mark.parametrize('KH,Cin,Cout', [(1, 20, 36), (3, 3, 12), (3, 96, 200), (7, 3, 32)])
def test_weight_packers_write_their_zero_padding(KH, Cin, Cout):
  w = dev(rnd((KH, KH, Cin, Cout), 100 + Cin))
  for fn in (lambda w: ops.pack_weights_bf16(w), lambda w: ops.pack_weights_bf16(w, half=True),
             lambda w: ops.pack_weights_split_bf16(w, 2), lambda w: ops.pack_weights_split_bf16(w, 3)):
    ref, got, _ = contained(fn, [w], [V])
    # a second image from a kernel whose every element has three non-zero bf16 parts: what stays zero is the padding
    _zero_padded(got, fn(torch.full_like(w, PROBE)).view(torch.int16) != 0)
  if (KH, Cin) == (7, 3):
    for parts in (2, 3):
      ref, got, _ = contained(lambda w: ops.pack_weights_split_root_bf16(w, parts), [w], [V])
      _zero_padded(got, ops.pack_weights_split_root_bf16(torch.full_like(w, PROBE), parts).view(torch.int16) != 0)


@pytest.mark.parametrize('math', ['bf16x3', 'bf16x6', 'bf16', 'fp16'])
def test_multi_weight_packers(math):
  shapes = [(1, 1, 20, 36), (3, 3, 96, 200), (1, 1, 257, 64), (3, 3, 8, 12)]
  ws = [dev(rnd(s, 110 + i)) for i, s in enumerate(shapes)]
  split = math in ops.SPLIT_PARTS
  keys = [math] if split else [math, math + '/rot']

  def run(*ws):
    ops.PACK_EPOCH += 1
    if split:
      ops.pack_weights_split_multi(list(ws), math)
    else:
      ops.pack_weights_bf16_multi(list(ws), with_rotated=True, math=math)
    return [ops._image_get(w, k) for w in ws for k in keys]

  ref, got, _ = contained(run, ws, [V] * len(ws))
  assert all(t is not None for t in got)
  for single, w in zip(got[::len(keys)], ws):
    one = ops.pack_weights_split_bf16(w, ops.SPLIT_PARTS[math]) if split else ops.pack_weights_bf16(w, half=(math == 'fp16'))
    assert guarded.same_bits(one, single)


@pytest.mark.parametrize('H,W,R,D,S', [(10, 13, 12, 16, 3), (9, 9, 8, 20, 2)])
def test_pack_stacked_templates_split(H, W, R, D, S):
  t = dev(rnd((R, H, W, D), 120))
  ref, got, _ = contained(lambda t: ops.pack_stacked_templates_split(t, S), [t], [V])
  assert got is not None
  contained(lambda t: ops.stack_templates(t, S, layout='rhwd'), [t], [V])


# ----------------------------------------------------------------------------------------------------
# encoder ops
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu_first', [False, True])
@pytest.mark.parametrize('C', [64, 256])
def test_group_norm_stats_and_apply(C, relu_first):
  x, gamma, beta = dev(rnd((2, 7, 9, C), 130)), dev(rnd((C,), 131) + 1), dev(rnd((C,), 132))
  contained(lambda x, g: ops.group_norm_stats(x, g, relu_first=relu_first), [x, gamma], [V, V])
  ref, _, _ = contained(lambda x, g: ops.group_norm_stats(x, g, relu_first=relu_first, want_rstd=True), [x, gamma], [V, V])
  for mode in (ops.PRO_GN_RELU, ops.PRO_RELU_GN):
    contained(lambda x, mu, sc, b: ops.group_norm_apply(x, mu, sc, b, mode), [x, ref[0], ref[1], beta], [V] * 4)


def test_weight_standardize_and_multi():
  shapes = [(3, 3, 20, 36), (1, 1, 64, 200), (7, 7, 3, 32), (1, 1, 5, 3)]
  ws = [dev(rnd(s, 140 + i)) for i, s in enumerate(shapes)]
  for w in ws:
    contained(lambda w: ops.weight_standardize(w), [w], [V])
  ref, _, _ = contained(lambda *ws: ops.weight_standardize_multi(list(ws)), ws, [V] * len(ws))
  dws = [dev(rnd(s, 150 + i)) for i, s in enumerate(shapes)]
  for w, d in zip(ws, dws):
    contained(lambda w, d: ops_bwd.weight_standardize_bwd(w, d), [w, d], [V, V])
  contained(lambda *a: ops.weight_standardize_bwd_multi(list(a[:4]), list(a[4:])), ws + dws, [V] * 8)


def test_max_pool_pad_image_voxel_points():
  x = dev(rnd((2, 7, 9, 20), 160))
  ref, _, _ = contained(lambda x: ops.max_pool_3x3s2(x), [x], [V])
  contained(lambda x, dy: ops_bwd.max_pool_3x3s2_bwd(x, dy), [x, dev(rnd(tuple(ref.shape), 161))], [V, V])
  contained(lambda dy: ops_bwd.upsample2x_bwd(dy), [dev(rnd((2, 6, 10, 20), 162))], [V])
  for shape, ph, pw, pc in (((5, 37, 29, 3), 27, 3, 1), ((2, 3, 16, 16, 3), 16, 16, 1), ((1, 7, 9, 20), 0, 0, 0)):
    contained(lambda x: ops.pad_image(x, ph, pw, pc), [dev(rnd(shape, 163))], [V])
  xy, z = dev(rnd((11, 13, 2), 164)), dev(rnd((2, 7), 165))
  contained(lambda xy, z: ops.voxel_points(xy, z), [xy, z], [V, V])
  contained(lambda xy, z: ops.voxel_points(xy, z), [dev(rnd((2, 11, 13, 2), 166)), z], [V, V])


@pytest.mark.parametrize('M,C', [(5, 192), (1, 4)])
def test_layer_norm_gelu_and_their_vjps(M, C):
  x, gamma, beta, dy = dev(rnd((M, C), 170)), dev(rnd((C,), 171) + 1), dev(rnd((C,), 172)), dev(rnd((M, C), 173))
  contained(lambda x, g, b: ops.layer_norm(x, g, b), [x, gamma, beta], [V] * 3)
  contained(lambda x, g, b: ops.layer_norm(x, g, b, out_half=True), [x, gamma, beta], [V] * 3)
  contained(lambda x: ops.gelu(x), [x], [V])
  contained(lambda x, dy: ops_bwd.gelu_bwd(x, dy), [x, dy], [V, V])
  contained(lambda x, dy, g: ops_bwd.layer_norm_bwd(x, dy, g), [x, dy, gamma], [V] * 3)


def test_semantic_embed_and_onehot():
  g = torch.Generator().manual_seed(180)
  rasters = dev(torch.rand((2, 7, 9, 6), generator=g) > 0.5)
  idx_road, idx_other = [0, 2, 3], [1, 4, 5]
  tr, to = dev(rnd((3, 8), 181)), dev(rnd((6, 8), 182))
  contained(lambda r, tr, to: ops.semantic_embed(r, idx_road, idx_other, tr, to), [rasters, tr, to], [A, V, V])
  contained(lambda r: ops.semantic_onehot(r, idx_road, idx_other), [rasters], [A])


@pytest.mark.parametrize('shape,D', [((9,), 3), ((7, 5), 1), ((6, 8), 5), ((4, 5, 3), 2)])
def test_interpolate_nd_and_expectation_nd(shape, D):
  n = len(shape)
  g = torch.Generator().manual_seed(190 + n)
  arr = dev(rnd((*shape, D), 191))
  pts = dev((torch.rand((37, n), generator=g) * 1.4 - 0.2) * torch.tensor(shape, dtype=torch.float32))
  valid = dev(torch.rand(shape, generator=g) > 0.2)
  contained(lambda a, p: ops.interpolate_nd(a, p), [arr, pts], [V, A])
  contained(lambda a, p, v: ops.interpolate_nd(a, p, v), [arr, pts, valid], [V, A, A])
  pdf = dev(torch.rand((3, *shape), generator=g))
  contained(lambda p: ops.expectation_nd(p, shape), [pdf], [V])


# ----------------------------------------------------------------------------------------------------
# lift and BEV
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,Vw', [(0, 1), (2, 3), (4, 6)])
def test_lift_pool_on_an_odd_grid(K, Vw):
  """11 x 13 x 7 points (cameras, poses and points are 'address' operands: zero guards).  The plain form writes
  every row.  The training form (``valid_rows_only``) documents the rows of unobserved voxels as unwritten: they
  must still be poison.  ``class_rows``: rows of class 1 do not write their variance slabs.  ``tap_records``:
  class-1 voxels write no row at all but their record (records of other classes carry no promise)."""
  fd, nb = 32, 8
  f, cam, Rt, pts = _lift_scene(2, Vw, 12, 16, fd, nb, 11 * 13 * 7, seed=30 + Vw)
  kw = dict(K=K, fisheye=True, feature_dim=fd, num_bins=nb, depth_min_max=(1.0, 16.0))
  args = [dev(f), dev(cam), dev(Rt), dev(pts)]
  kinds = [V, A, A, A]
  (_, valid), _, _ = contained(lambda f, c, r, p: ops.lift_pool(f, c, r, p, **kw), args, kinds)
  assert 0 < int(valid.sum()) < valid.numel()
  contained(lambda f, c, r, p: ops.lift_pool(f, c, r, p, grid_yz=(13, 7), **kw), args, kinds)
  contained(lambda f, c, r, p: ops.lift_pool(f, c, r, p, valid_rows_only=True, **kw), args, kinds,
            leave={'out[0]': ~valid[..., None]})
  contained(lambda f, c, r, p: ops.lift_pool(f, c, r, p, out_split=True, **kw), args, kinds)
  cls = ops.lift_pool(*args, out_split=True, class_rows=True, **kw)[2]
  stride = (ops.pooled_channels(fd) + 15) // 16 * 16
  var_slabs = torch.zeros(stride, dtype=torch.bool, device=DEV)
  var_slabs[fd:2 * fd] = True                      # 16-float slabs fd / 16 .. 2 fd / 16 - 1
  one = (cls == 1)[..., None]
  contained(lambda f, c, r, p: ops.lift_pool(f, c, r, p, out_split=True, class_rows=True, **kw), args, kinds,
            leave={'out[0]': one & var_slabs})
  contained(lambda f, c, r, p: ops.lift_pool(f, c, r, p, out_split=True, class_rows=True, valid_rows_only=True, tap_records=True, **kw),
            args, kinds, leave={'out[0]': (cls <= 1)[..., None].expand(-1, -1, stride)}, ignore={'out[3]': ~one})
  contained(lambda c, r, p: ops.project_points(c, r, p, True), args[1:], [A, A, A])
  # the VJP in its deterministic form
  dp = rnd((2, 11 * 13 * 7, ops.pooled_stride(fd)), 33)
  dp[..., ops.pooled_channels(fd):] = 0
  contained(lambda f, c, r, p, d: ops_bwd.lift_pool_bwd(f, c, r, p, d, **kw), args + [dev(dp)], kinds + [V])


@pytest.mark.parametrize('K,Vw', [(0, 3), (2, 4)])
def test_lift_observations_and_their_vjps(K, Vw):
  fd = 32
  f, cam, Rt, pts = _lift_scene(2, Vw, 12, 16, fd, 0, 11 * 13 * 7, seed=40 + Vw)
  args = [dev(f), dev(cam), dev(Rt), dev(pts)]
  kw = dict(K=K, fisheye=True, feature_dim=fd)
  (obs, feat, valid), _, _ = contained(lambda f, c, r, p: ops.lift_observations(f, c, r, p, **kw), args, [V, A, A, A])
  fs = tuple(f.shape)
  (pooled, _), _, _ = contained(lambda o, c, r, p: ops.lift_pool_observations(o, fs, c, r, p, **kw), [feat] + args[1:], [V, A, A, A])
  dp = dev(rnd(tuple(pooled.shape), 41))
  contained(lambda o, c, r, p, d: ops_bwd.lift_pool_observations_bwd(o, fs, c, r, p, d, **kw), [feat] + args[1:] + [dp], [V, A, A, A, V])
  contained(lambda d, c, r, p: ops_bwd.lift_observations_bwd(d, fs, c, r, p, **kw), [dev(rnd(tuple(feat.shape), 42))] + args[1:], [V, A, A, A])


@pytest.mark.parametrize('cin,stride,H,D,Z,ncols,relu_in', MLP_POOL_CASES)
def test_mlp2_pool_max(cin, stride, H, D, Z, ncols, relu_in):
  g = torch.Generator().manual_seed(200 + cin)
  M = ncols * Z
  x = rnd((M, stride), 201)
  x[:, cin:] = 0          # (the rows' padding is zero by the lift's contract)
  mask = torch.rand(M, generator=g) > 0.4
  mask.view(ncols, Z)[0] = False               # an unobserved column
  w0, b0, w1, b1 = rnd((cin, H), 202, 1 / np.sqrt(cin)), rnd((H,), 203), rnd((H, D), 204, 1 / np.sqrt(H)), rnd((D,), 205)
  contained(lambda x, m, w0, b0, w1, b1: ops.mlp2_pool_max(x, m, w0, b0, w1, b1, cin=cin, Z=Z, relu_in=relu_in),
            [dev(t) for t in (x, mask, w0, b0, w1, b1)], [V, A, V, V, V, V])


@pytest.mark.parametrize('D', [32, 128, 256])
@pytest.mark.parametrize('Z', [1, 12, 70])
def test_vertical_pool_and_its_vjps(Z, D):
  g = torch.Generator().manual_seed(210 + Z)
  vol, valid = dev(rnd((3, 5, Z, D), 211)), dev(torch.rand((3, 5, Z), generator=g) > 0.5)
  dplane = dev(rnd((3, 5, D), 212))
  for pooling in ('max', 'sum', 'mean'):
    contained(lambda v, m: ops.vertical_pool(v, m, pooling), [vol, valid], [V, A])
    contained(lambda v, m, d: ops_bwd.vertical_pool_bwd(v, m, d, pooling), [vol, valid, dplane], [V, A, V])
  ref, _, _ = contained(lambda v, m: ops.vertical_pool(v, m, 'max', want_arg=True), [vol, valid], [V, A])
  if ref[2] is not None:
    contained(lambda v, m, d, az, ti: ops_bwd.vertical_pool_bwd(v, m, d, 'max', arg=(az, ti)),
              [vol, valid, dplane, ref[2][0], ref[2][1]], [V, A, V, A, A])


@pytest.mark.parametrize('D', [32, 128])
@pytest.mark.parametrize('Z', [1, 12, 60])
def test_vertical_pool_conf_and_its_vjp(Z, D):
  """(snap_vertical_pool_conf_f32 refuses Z > 64 and D > 128 as a bad shape: 60 stands in for 70, no 256.)"""
  g = torch.Generator().manual_seed(215 + Z)
  vol, valid = dev(rnd((3, 5, Z, D), 216)), dev(torch.rand((3, 5, Z), generator=g) > 0.5)
  dplane = dev(rnd((3, 5, D), 217))
  w, bias = dev(rnd((D,), 213, 0.2)), dev(rnd((1,), 214))
  for ls in (False, True):
    r, _, _ = contained(lambda v, m, w, b: ops.vertical_pool_conf(v, m, w, b, ls), [vol, valid, w, bias], [V, A, V, V])
    contained(lambda v, m, w, b, wt, d: ops_bwd.vertical_pool_conf_bwd(v, m, w, b, wt, d, ls),
              [vol, valid, w, bias, r[3], dplane], [V, A, V, V, V, V])


@pytest.mark.parametrize('D,Dm,pooling', [(32, 8, 'max'), (128, 32, 'max'), (128, 16, 'mean'), (20, 8, 'sum')])
def test_plane_fuse_match(D, Dm, pooling):
  """D = 128 takes the persistent kernel, the others the per-cell kernel."""
  g = torch.Generator().manual_seed(220 + D)
  planes = [dev(rnd((11, 13, D), 221 + i)) for i in range(2)]
  valids = [dev(torch.rand((11, 13), generator=g) > 0.3) for _ in range(2)]
  Wm, bm = dev(rnd((D, Dm), 223, 1 / np.sqrt(D))), dev(rnd((Dm,), 224))
  contained(lambda p0, p1, v0, v1, Wm, bm: ops.plane_fuse_match([p0, p1], [v0, v1], pooling, Wm, bm),
            planes + valids + [Wm, bm], [V, V, A, A, V, V])
  dm, df = dev(rnd((11, 13, Dm), 225)), dev(rnd((11, 13, D), 226))
  contained(lambda p0, p1, v0, v1, Wm, bm, dm, df: ops_bwd.plane_fuse_match_bwd([p0, p1], [v0, v1], pooling, Wm, bm, True, 1e-5, dm, df),
            planes + valids + [Wm, bm, dm, df], [V, V, A, A, V, V, V, V])


def test_fill_masked_rows_in_place():
  y = dev(rnd((117, 20), 230))
  mask = dev(torch.rand(117, generator=torch.Generator().manual_seed(231)) > 0.5)

  def run(y, m):
    ops.fill_masked_rows_(y, m, 0.0)

  contained(run, [y, mask], [V, A], inplace=(0,))


@pytest.mark.parametrize('M', [1, 17, 4097])
def test_compact_rows(M):
  """index: the first `count` entries are promised, the rest is not; the count is."""
  mask = dev(torch.rand(M, generator=torch.Generator().manual_seed(M)) > 0.5)
  mask[0] = True
  index, count = ops.compact_rows(mask)
  n = int(count)
  with guarded.scope() as sc:
    gi, gc = ops.compact_rows(guarded.place(mask, A))
    sc.check()
    assert guarded.same_bits(count, gc) and guarded.same_bits(index[:n], gi[:n])
    assert not bool(guarded.unwritten(gc).any()) and not bool(guarded.unwritten(gi[:n]).any())
    assert torch.equal(gi[:n].long(), mask.nonzero().reshape(-1))


# ----------------------------------------------------------------------------------------------------
# pose and voting
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('math', ['f32', 'bf16x3', 'bf16x6'])
@pytest.mark.parametrize('X,Y,Dm', [(13, 21, 8), (40, 24, 16)])
def test_sim_softmax(X, Y, Dm, math):
  B, Nq = 2, 37
  fq, fm = dev(rnd((B, Nq, Dm), 240)), dev(rnd((B, X, Y, Dm), 241))
  nv = dev(torch.tensor([30.0, 37.0]))
  contained(lambda q, m, n: ops.sim_softmax(q, m, 3.0, True, n, math=math), [fq, fm, nv], [V, V, V])
  contained(lambda q, m, n: ops.sim_softmax(q, m, 3.0, False, n, want_prob=True, math=math), [fq, fm, nv], [V, V, V])
  contained(lambda q, m, n: ops.sim_softmax(q, m, 3.0, True, n, want_rowstats=True, math=math), [fq, fm, nv], [V, V, V])


def test_masked_softmax_rows_confidence_head_and_vjps():
  g = torch.Generator().manual_seed(250)
  x, mask = dev(rnd((3, 45), 251)), dev(torch.rand((3, 45), generator=g) > 0.3)
  ref, _, _ = contained(lambda x, m: ops.masked_softmax_rows(x, m), [x, mask], [V, A])
  contained(lambda w, d: ops_bwd.masked_softmax_rows_bwd(w, d), [ref[0], dev(rnd((3, 45), 252))], [V, V])
  f, valid = dev(rnd((11, 13, 20), 253)), dev(torch.rand((11, 13), generator=g) > 0.3)
  k, b = dev(rnd((20,), 254, 0.3)), dev(rnd((1,), 255))
  contained(lambda f, v, k, b: ops.confidence_head(f, v, k, b), [f, valid, k, b], [V, A, V, V])
  contained(lambda f, v, k, b, d: ops_bwd.confidence_head_bwd(f, v, k, b, d), [f, valid, k, b, dev(rnd((11, 13), 256))], [V, A, V, V, V])


def _pose_inputs(X, Y, B=2, Nq=45, P=700):
  rng = np.random.default_rng(110)
  sim = torch.tensor(rng.random((B, Nq, X, Y), dtype=np.float32))
  cell = 0.2
  poses = np.stack([rng.uniform(-np.pi, np.pi, (B, P)), rng.uniform(-0.2 * X * cell, 1.2 * X * cell, (B, P)),
                    rng.uniform(-0.2 * Y * cell, 1.2 * Y * cell, (B, P))], -1).astype(np.float32)
  q_xy = torch.tensor(rng.uniform(-2, 2, (B, Nq, 2)).astype(np.float32))
  valid_q = torch.tensor(rng.random((B, Nq)) > 0.2)
  map_valid = torch.tensor(rng.random((B, X, Y)) > 0.1)
  return [dev(t) for t in (sim, torch.tensor(poses), q_xy, valid_q, map_valid)], cell


@pytest.mark.parametrize('mask_oob', [False, True])
@pytest.mark.parametrize('X,Y', [(25, 37), (131, 260)])
def test_pose_score_and_its_vjp(X, Y, mask_oob):
  """(131, 260): the band path.  Poses, points and validity are 'address' operands; the score planes are values."""
  args, cell = _pose_inputs(X, Y)
  ref, _, _ = contained(lambda s, p, q, v, m: ops.pose_score(s, p, q, v, m, cell, mask_oob=mask_oob), args, [V, A, A, A, A])
  if X * Y * 4 > 96 * 1024:
    return           # (the VJP takes planes up to 96 KiB: the band tiling is forward only)
  ds = dev(rnd(tuple(ref.shape), 260))
  # mask_oob: only the float-atomic form exists (no repeatable order): test_pose_score_bwd's tolerance
  contained(lambda d, p, q, v, m: ops_bwd.pose_score_bwd(d, p, q, v, m, tuple(args[0].shape), cell, mask_oob=mask_oob),
            [ds] + args[1:], [V, A, A, A, A], tol=(2e-4, 1e-4) if mask_oob else None)


def test_pose_score_window_lattice_and_argmax():
  X, Y, Nq, B, rad, cell = 33, 36, 50, 1, 4, 0.2
  g = torch.Generator().manual_seed(X + Nq)
  sim = dev(torch.randn((B, Nq, X, Y), generator=g))
  q_xy = dev((torch.rand((B, Nq, 2), generator=g) - 0.5) * 6.0)
  qn = float(q_xy.norm(dim=-1).max())
  centers = torch.stack([torch.rand(B, generator=g) * 6.28, torch.rand(B, generator=g) * X * cell, torch.rand(B, generator=g) * Y * cell], -1)
  P, budget = 3000, (rad - 1) * cell
  da = (torch.rand(B, P, generator=g) - 0.5) * 2 * min(0.3 * budget / max(qn, 1e-3), 0.5)
  room = budget - qn * da.abs().max()
  ang, rr = torch.rand(B, P, generator=g) * 6.28, torch.rand(B, P, generator=g) * float(room)
  poses = dev(torch.stack([centers[:, None, 0] + da, centers[:, None, 1] + rr * torch.cos(ang), centers[:, None, 2] + rr * torch.sin(ang)], -1))
  vq = dev(torch.rand(B, Nq, generator=g) > 0.2)
  assert ops.pose_score_window_supported(X, Y, rad)
  ref, _, _ = contained(lambda s, p, c, q, v: ops.pose_score_window(s, p, c, rad, q, v, cell), [sim, poses, dev(centers), q_xy, vq], [V, A, A, A, A])
  contained(lambda s: ops.argmax_rows(s, 1), [ref], [V])
  contained(lambda s: ops.argmax_rows(s), [dev(rnd((3, 4097), 270))], [V])
  contained(lambda i, r, p: ops.refine_lattice(i, r, p), [dev(rnd((2, 3), 271)), dev(rnd((5,), 272, 0.1)), dev(rnd((7,), 273))], [A, A, A])


def test_ransac_sample_and_poses_from_corr():
  B, Nq, X, Y, Dm, S = 2, 40, 24, 20, 16, 600
  unit = lambda t: t / t.norm(dim=-1, keepdim=True)
  fq, fm = dev(unit(rnd((B, Nq, Dm), 95))), dev(unit(rnd((B, X, Y, Dm), 96)))
  scale = float(np.exp(2.5))
  u = dev(torch.rand((B, S, 2), generator=torch.Generator().manual_seed(97)))
  _, stats, _, _ = ops.sim_softmax(fq, fm, scale, True, dev(torch.tensor([40.0, 40.0])))
  for row_table in (True, False):          # (with and without the row-prefix workspace)
    contained(lambda q, m, st, u: ops.ransac_sample(q, m, st, scale, True, S, uniforms=u, row_table=row_table), [fq, fm, stats, u], [V, V, V, V])
    contained(lambda q, m, st: ops.ransac_sample(q, m, st, scale, True, S, seed=1234, row_table=row_table), [fq, fm, stats], [V, V, V])
  P, retries = 75, 4
  corr, _, _ = contained(lambda q, m, st: ops.ransac_sample(q, m, st, scale, True, P * retries * 2, seed=7), [fq, fm, stats], [V, V, V])
  q_xy = dev(rnd((B, Nq, 2), 98) * 2.0)
  contained(lambda c, q: ops.poses_from_corr(c, q, P, retries, 0.2), [corr, q_xy], [A, A])


def test_templates_and_pad_map():
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import grids
  H, R, D = 16, 8, 8
  g = torch.Generator().manual_seed(280)
  valid = dev(torch.rand((H, H), generator=g) > 0.2)
  feat = (dev(rnd((H, H, D), 281)) * valid[..., None]).contiguous()
  tfm = pev._template_transforms(R, grids.Grid2D((H, H), 0.25), feat.device)[: R // 4].contiguous()
  for want_tw in (True, False):
    contained(lambda f, v, t: ops.rotate_templates(f, v, t, R, 0.25, want_tw=want_tw), [feat, valid, tfm], [V, A, A])
  m, mvalid = dev(rnd((20, 18, D), 282)), dev(torch.rand((20, 18), generator=g) > 0.2)
  contained(lambda m, v: ops.pad_map(m, v), [m, mvalid], [V, A])
  contained(lambda t: ops.stack_templates(t, 3), [dev(rnd((10, 13, 8, 12), 283))], [V])
  Ho, Wo, Rp = 13, 11, 12
  raw, cnt, tcount = dev(rnd((Ho, Wo, Rp), 284)), dev(torch.rand((Ho, Wo, Rp), generator=g) * 50), dev(torch.rand(R, generator=g) * 100 + 1)
  contained(lambda r, c, t: ops.template_finalize(r, c, t, R, 0.05), [raw, cnt, tcount], [V, V, V])
  contained(lambda r, t: ops.template_finalize(r, None, t, R, 0.0, use_overlap=False), [raw, tcount], [V, V])


@pytest.mark.parametrize('H,W,Hm,Wm,R,D', [(6, 7, 8, 8, 8, 6), (9, 9, 11, 10, 8, 6), (8, 8, 8, 8, 7, 34)])
def test_voting_fft(H, W, Hm, Wm, R, D):
  """3 * 8 - 2 = 22 -> a 24-point transform (the fused first stage); 3 * 11 - 2 = 31 -> 32 points (without it);
  D % 4 != 0; a map of another size than the template; an odd R with two channel groups."""
  g = torch.Generator().manual_seed(290 + H)
  tv = dev(torch.rand((R, H, W), generator=g) > 0.2)
  t = (dev(rnd((R, H, W, D), 291)) * tv[..., None]).contiguous()
  m, mv = dev(rnd((Hm, Wm, D), 292)), dev(torch.rand((Hm, Wm), generator=g) > 0.1)
  tcount = tv.reshape(R, -1).sum(-1).float()
  assert ops.voting_fft_supported(R, H, W, D, Hm, Wm)
  contained(lambda t, tv, m, mv, tc: ops.voting_fft(t, tv, m, mv, tc, 0.05), [t, tv, m, mv, tcount], [V, A, V, A, V])
  contained(lambda t, m, tc: ops.voting_fft(t, None, m, None, tc, 0.0, use_overlap=False), [t, m, tcount], [V, V, V])


@pytest.mark.parametrize('H,Hm,Wm,R,D', [(8, 8, 8, 8, 6), (10, 11, 11, 8, 6)])
def test_voting_fft_rotated(H, Hm, Wm, R, D):
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.utils import grids
  g = torch.Generator().manual_seed(295 + H)
  valid = dev(torch.rand((H, H), generator=g) > 0.15)
  feat = (dev(rnd((H, H, D), 296)) * valid[..., None]).contiguous()
  m, mv = dev(rnd((Hm, Wm, D), 297)), dev(torch.rand((Hm, Wm), generator=g) > 0.1)
  tfm = pev._template_transforms(R, grids.Grid2D((H, H), 0.25), feat.device)[: R // 4].contiguous()
  contained(lambda f, v, t, m, mv: ops.voting_fft_rotated(f, v, t, 0.25, m, mv, R), [feat, valid, tfm, m, mv], [V, A, A, V, A])


# ----------------------------------------------------------------------------------------------------
# occupancy
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,S', [(1, 1), (300, 3)])
def test_occupancy_query_kernels(N, S):
  """P = 1 and a partial workgroup (900 points); rays and explicit points; the gather VJP (rays, hits and masks are
  'address' operands)."""
  B, X, Y, Z, D = 2, 13, 11, 7, 64
  vol, vvalid = _occ_volume(B, X, Y, Z, D, seed=3)
  hits, origins, mask = _rays(B, N, (X, Y, Z), seed=4)
  kw = dict(num_samples=S, margin=0.2)
  (feats, _, samples), _, _ = contained(lambda v, vv, h, o, m: ops.occupancy_ray_features(v, vv, OCC_CELL, rays=(h, o, m), **kw),
                                        [vol, vvalid, hits, origins, mask], [V, A, A, A, A])
  pts = samples[0]
  contained(lambda v, vv, p: ops.occupancy_ray_features(v, vv, OCC_CELL, points=p), [vol, vvalid, pts], [V, A, A])
  for layers in ((64, 1), (64, 64, 1)):
    assert ops.occupancy_head_supported(D, layers[:-1])
    flat = [t for kb in _mlp_params(D, layers, seed=5) for t in kb]
    pair = lambda ts: [(ts[i], ts[i + 1]) for i in range(0, len(ts), 2)]
    contained(lambda v, vv, h, o, m, *ws: ops.occupancy_head(v, vv, OCC_CELL, pair(ws), rays=(h, o, m), **kw),
              [vol, vvalid, hits, origins, mask] + flat, [V, A, A, A, A] + [V] * len(flat))
    contained(lambda v, p, *ws: ops.occupancy_head(v, None, OCC_CELL, pair(ws), points=p), [vol, pts] + flat, [V, A] + [V] * len(flat))
  df = dev(rnd(tuple(feats.shape), 6))
  contained(lambda d, h, o, m: ops_bwd.occupancy_ray_features_vjp(d, tuple(vol.shape), OCC_CELL, rays=(h, o, m), **kw),
            [df, hits, origins, mask], [V, A, A, A])
  contained(lambda d, p: ops_bwd.occupancy_ray_features_vjp(d, tuple(vol.shape), OCC_CELL, points=p), [df, pts], [V, A])


# ----------------------------------------------------------------------------------------------------
# VJPs
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('math', ['f32', 'bf16', 'fp16'])
@pytest.mark.parametrize('N,H,W,Cin,Cout,k,stride', [(2, 9, 11, 64, 256, 1, 1), (1, 13, 9, 32, 64, 3, 1), (2, 15, 13, 96, 200, 3, 1),
                                                     (1, 6, 7, 20, 36, 1, 1), (8, 34, 34, 64, 64, 3, 1), (2, 14, 10, 64, 128, 3, 2)])
def test_conv2d_wgrad(N, H, W, Cin, Cout, k, stride, math):
  """Ragged fused-tap 3 x 3 cases (15 x 13, 96 -> 200), a split-M case (8 x 34 x 34) and the strided form."""
  pad = ((k // 2, k // 2), (k // 2, k // 2))
  Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
  x, dy = dev(rnd((N, H, W, Cin), 300)), dev(rnd((N, Ho, Wo, Cout), 301))
  contained(lambda x, dy: ops_bwd.conv2d_wgrad(x, dy, (k, k, Cin, Cout), stride=stride, padding=pad, math=math), [x, dy], [V, V])


@pytest.mark.parametrize('math', ['f32', 'bf16', 'fp16'])
def test_data_gradient_conv(math):
  """The data gradient is a conv2d of dy with the rotated kernel (full padding)."""
  dy, wr = dev(rnd((2, 15, 13, 200), 310)), dev(rnd((3, 3, 200, 96), 311, 0.05))
  contained(lambda dy, w: ops.conv2d(dy, w, padding=((1, 1), (1, 1)), math=math), [dy, wr], [V, V])


@pytest.mark.parametrize('half', [None, 'bf16', 'fp16'])
@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('mode', [ops.PRO_GN_RELU, ops.PRO_RELU_GN])
def test_group_norm_bwd(mode, with_add, half):
  N, H, W, C = 2, 7, 9, 64
  x, dz, gamma, beta = dev(rnd((N, H, W, C), 320)), dev(rnd((N, H, W, C), 321)), dev(rnd((C,), 322) + 1), dev(rnd((C,), 323))
  mu, sc, rstd = ops.group_norm_stats(x, gamma, relu_first=(mode == ops.PRO_RELU_GN), want_rstd=True)
  add = dev(rnd((N, H, W, C), 324)) if with_add else None
  _, got, _ = contained(lambda x, dz, mu, rstd, g, b, add: ops_bwd.group_norm_bwd(x, dz, mu, rstd, g, b, mode, add=add, half=half),
                        [x, dz, mu, rstd, gamma, beta, add], [V] * 7)
  if half is not None:       # the twin the data-gradient convs read: written completely, the rounded dx
    twin = ops_bwd.half_twin(got[0], half)
    assert twin is not None and not bool(guarded.unwritten(twin).any()) and guarded.same_bits(twin, got[0].to(twin.dtype))


@pytest.mark.parametrize('M,C', [(117, 36), (198, 160), (30, 256), (2049, 12)])
def test_epilogue_bwd_and_column_sums(M, C):
  g = torch.Generator().manual_seed(330)
  dy, y = dev(rnd((M, C), 331)), dev(rnd((M, C), 332))
  mask = dev(torch.rand(M, generator=g) > 0.4)
  n = max(1, M // 2)
  count = torch.tensor([n], dtype=torch.int32, device=DEV)
  rows = dev(torch.randperm(M, generator=g).to(torch.int32))
  contained(lambda dy, y, m: ops_bwd.epilogue_bwd(dy, y, m, relu=True), [dy, y, mask], [V, V, A])
  contained(lambda dy, y, m: ops_bwd.epilogue_bwd_colsum(dy, y, m, relu=True), [dy, y, mask], [V, V, A])
  beyond = (torch.arange(M, device=DEV) >= n)[:, None]       # (rows beyond the count: no promise either way)
  contained(lambda dy, y, c: ops_bwd.epilogue_bwd_colsum(dy, y, None, relu=True, row_count=c), [dy, y, count], [V, V, A],
            ignore={'out[0]': beyond})
  contained(lambda a: ops_bwd.colsum(a), [dy], [V])
  contained(lambda a, r, c: ops_bwd.colsum(a, rows=r, row_count=c), [dy, rows, count], [V, A, A])
  if C % 4 == 0 and 256 % (C // 4 if C < 1024 else 256) == 0:      # (the half kernel's widths)
    for dt in (torch.bfloat16, torch.float16):
      contained(lambda dy, y, c: ops_bwd.epilogue_bwd_colsum(dy, y, None, relu=True, row_count=c), [dy.to(dt), y.to(dt), count], [V, V, A],
                ignore={'out[0]': beyond})


@pytest.mark.parametrize('math', ['f32', 'bf16', 'fp16'])
@pytest.mark.parametrize('cin,Cs,H', [(257, 260, 256), (65, 68, 64), (20, 20, 36)])
def test_dense_wgrad_rows(cin, Cs, H, math):
  """The masked MLP's first-layer kernel gradient over a row list with a device count shorter than the list;
  257 of 260 channels takes the main + tail-quad launches (the pad columns are zero: the rows' contract)."""
  M = 198
  g = torch.Generator().manual_seed(500 + cin)
  x2 = rnd((M, Cs), 501)
  x2[:, cin:] = 0
  grad = dev(rnd((M, H), 502))
  rows = dev(torch.randperm(M, generator=g)[:150].to(torch.int32))
  count = torch.tensor([77], dtype=torch.int32, device=DEV)
  with ops.engine_scope(math):
    contained(lambda x, g_, r, c: ops_bwd.dense_wgrad_rows(x, g_, cin, H, prologue=ops.PRO_RELU, rows_z=r, rows_dy=r, row_count=c),
              [dev(x2), grad, rows, count], [V, V, A, A])


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
def test_epilogue_bwd_colsum_with_the_extra_channel(dt):
  """``wsum`` / ``dtail``: the 257th channel's kernel-gradient row and its data gradient from the gate pass.  dx is
  an in-place operand: only the last quad of the listed rows is written."""
  M, C, R, Cs = 117, 256, 150, 260
  g = torch.Generator().manual_seed(510)
  dy, y = dev(rnd((M, C), 511)).to(dt), dev(rnd((M, C), 512)).to(dt)
  x2, w_row = dev(rnd((R, Cs), 513)), dev(rnd((C,), 514, 0.1))
  rows = dev(torch.randperm(R, generator=g)[:M].to(torch.int32))
  dx = dev(rnd((R, Cs), 515))
  contained(lambda dy, y, x2, r: ops_bwd.epilogue_bwd_colsum(dy, y, None, relu=True, wsum=(x2, 256, r, False)), [dy, y, x2, rows], [V, V, V, A])
  ref, _, sc = contained(lambda dy, y, x2, r, w, dx: ops_bwd.epilogue_bwd_colsum(dy, y, None, relu=True, wsum=(x2, 256, r, True), dtail=(w, dx)),
                         [dy, y, x2, rows, w_row, dx], [V, V, V, A, V, V], inplace=(5,))


@pytest.mark.parametrize('X,Y', [(13, 21), (40, 24)])
def test_sim_bwd_prepare_in_place(X, Y):
  B, Nq = 2, 37
  dsim, sim = dev(rnd((B, Nq, X, Y), 340)), dev(rnd((B, Nq, X, Y), 341))
  coef, rcoef = dev(rnd((B,), 342)), dev(rnd((B, Nq), 343))
  contained(lambda d, s, c: ops_bwd.sim_bwd_prepare_(d, s, True, c), [dsim, sim, coef], [V, V, V], inplace=(0,))
  contained(lambda d, s, c: ops_bwd.sim_bwd_prepare_rows_(d, s, True, c), [dsim, sim, rcoef], [V, V, V], inplace=(0,))


def test_adam_update_in_place():
  sizes = [1, 1000, 4097]
  ts = [dev(rnd((n,), 350 + i)) for i, n in enumerate(sizes)]               # params
  ts += [dev(rnd((n,), 360 + i)) for i, n in enumerate(sizes)]              # grads
  ts += [dev(rnd((n,), 370 + i) * 0.1) for i, n in enumerate(sizes)]        # m
  ts += [dev(rnd((n,), 380 + i).abs() * 0.01) for i, n in enumerate(sizes)]  # v
  contained(lambda *a: ops_bwd.adam_update_(list(a[0:3]), list(a[3:6]), list(a[6:9]), list(a[9:12]), 3, 1e-3),
            ts, [V] * 12, inplace=(0, 1, 2, 6, 7, 8, 9, 10, 11))


# ----------------------------------------------------------------------------------------------------
# the workspaces no caller receives
# ----------------------------------------------------------------------------------------------------
def _ws_cases():
  lib = _lib.load()
  g = torch.Generator().manual_seed(400)
  cases = []
  for N, HW, C in ((2, 63, 64), (2, 63, 256), (1, 4097, 64)):
    x, gamma = dev(rnd((N, HW, 1, C), 401)), dev(rnd((C,), 402) + 1)
    cases.append(('group_norm_stats', lambda x=x, gamma=gamma: ops.group_norm_stats(x, gamma, want_rstd=True),
                  lib.snap_group_norm_stats_workspace_bytes(N, HW, C, 32), torch.float32))
    mu, sc, rstd = ops.group_norm_stats(x, gamma, want_rstd=True)
    dz, beta = dev(rnd((N, HW, 1, C), 403)), dev(rnd((C,), 404))
    cases.append(('group_norm_bwd', lambda x=x, dz=dz, mu=mu, rstd=rstd, gamma=gamma, beta=beta:
                  ops_bwd.group_norm_bwd(x, dz, mu, rstd, gamma, beta, ops.PRO_GN_RELU),
                  lib.snap_group_norm_bwd_workspace_bytes(N, HW, C, 32), torch.float32))
  for M in (1, 17, 4097, 100003):
    mask = dev(torch.rand(M, generator=g) > 0.5)
    cases.append(('compact_rows', lambda mask=mask: ops.compact_rows(mask), lib.snap_compact_rows_workspace_bytes(M), torch.int32))
  for X, Y in ((25, 37), (131, 260)):
    (sim, poses, q_xy, vq, mv), cell = _pose_inputs(X, Y)
    B, Nq, P = sim.shape[0], sim.shape[1], poses.shape[1]
    cases.append(('pose_score', lambda a=(sim, poses, q_xy, vq, mv), cell=cell: ops.pose_score(*a, cell),
                  lib.snap_pose_score_workspace_bytes(B, Nq, P, X, Y), torch.float32))
    if X * Y * 4 > 96 * 1024:
      continue          # (the VJP takes planes up to 96 KiB)
    ds = dev(rnd((B, P), 405))
    cases.append(('pose_score_bwd', lambda ds=ds, a=(poses, q_xy, vq, mv), s=tuple(sim.shape), cell=cell: ops_bwd.pose_score_bwd(ds, *a, s, cell),
                  lib.snap_pose_score_bwd_workspace_bytes(B, P), torch.float32))
  for M, C in ((117, 36), (30, 256), (4097, 64), (5, 1024)):
    dy, y = dev(rnd((M, C), 406)), dev(rnd((M, C), 407))
    wsb = lib.snap_colsum_workspace_bytes(M, C)
    cases.append(('colsum', lambda dy=dy: ops_bwd.colsum(dy), wsb, torch.float32))
    if 256 % (C // 4 if C < 1024 else 256) == 0:        # (other widths go through epilogue_bwd + colsum)
      cases.append(('epilogue_bwd_colsum', lambda dy=dy, y=y: ops_bwd.epilogue_bwd_colsum(dy, y, None, relu=True), wsb, torch.float32))
      cases.append(('epilogue_bwd_colsum', lambda dy=dy, y=y: ops_bwd.epilogue_bwd_colsum(dy.to(torch.bfloat16), y.to(torch.bfloat16), None, relu=True),
                    wsb, torch.float32))
    x, gamma = dev(rnd((M, C), 408)), dev(rnd((C,), 409))
    cases.append(('layer_norm_bwd', lambda x=x, dy=dy, gamma=gamma: ops_bwd.layer_norm_bwd(x, dy, gamma),
                  lib.snap_layer_norm_bwd_workspace_bytes(M, C), torch.float32))
  for (N, H, W, Cin, Cout, k), math in (((2, 9, 11, 64, 256, 1), 'f32'), ((8, 34, 34, 64, 64, 3), 'bf16'), ((2, 15, 13, 96, 200, 3), 'fp16'),
                                        ((2, 15, 13, 96, 200, 3), 'f32')):
    x, dy = dev(rnd((N, H, W, Cin), 410)), dev(rnd((N, H, W, Cout), 411))
    pad = ((k // 2, k // 2), (k // 2, k // 2))
    d, _ = ops_bwd._conv_desc(x.shape, (k, k, Cin, Cout), 1, pad, ops.PRO_NONE, (1.0, 0.0))
    d.tile_hint = 0
    cases.append(('conv2d_wgrad', lambda x=x, dy=dy, s=(k, k, Cin, Cout), pad=pad, math=math: ops_bwd.conv2d_wgrad(x, dy, s, padding=pad, math=math),
                  lib.snap_conv2d_wgrad_workspace_bytes(ctypes.byref(d)), torch.float32))
  return cases


def test_workspaces_are_exactly_what_the_queries_return():
  """Eleven wrappers used to allocate `wsb // 4 + 4` elements.  Inside the scope the workspace is fetched by its
  allocating wrapper: it holds exactly what the `*_workspace_bytes` query returns (no spare tail), and the guards
  behind it -- where the four spare elements used to be -- are intact after the call (``scope`` exit)."""
  X, Y, rad, cell = 33, 36, 4, 0.2
  seen = set()
  for name, call, wsb, dtype in _ws_cases():
    want = call()
    with guarded.scope() as sc:
      got = call()
      sc.check()
      if name == 'compact_rows':          # (index: the first `count` entries are promised)
        k = int(want[1])
        assert guarded.same_bits(want[1], got[1]) and guarded.same_bits(want[0][:k], got[0][:k])
      else:
        assert_same(want, got)
      ws = [v for v in sc.allocations(site=name) if v.dim() == 1 and v.dtype == dtype and v.numel() * 4 >= wsb and v.numel() * 4 <= wsb + 16]
      assert ws, f'{name}: no workspace of {wsb} bytes among {[tuple(v.shape) for v in sc.allocations(site=name)]}'
      assert ws[0].numel() * 4 == wsb, f'{name}: workspace of {ws[0].numel() * 4} bytes, the query returns {wsb}'
    seen.add(name)
  assert seen == {'group_norm_stats', 'group_norm_bwd', 'compact_rows', 'pose_score', 'pose_score_bwd', 'colsum', 'epilogue_bwd_colsum',
                  'layer_norm_bwd', 'conv2d_wgrad'}
  # pose_score_window: its own query
  lib = _lib.load()
  g = torch.Generator().manual_seed(83)
  sim, q_xy = dev(torch.randn((1, 50, X, Y), generator=g)), dev((torch.rand((1, 50, 2), generator=g) - 0.5) * 2.0)
  centers = dev(torch.tensor([[0.3, 3.0, 3.5]]))
  poses = (centers[:, None, :] + dev((torch.rand((1, 500, 3), generator=g) - 0.5) * torch.tensor([0.05, 0.2, 0.2]))).contiguous()
  vq = dev(torch.rand(1, 50, generator=g) > 0.2)
  want = ops.pose_score_window(sim, poses, centers, rad, q_xy, vq, cell)
  with guarded.scope() as sc:
    got = ops.pose_score_window(sim, poses, centers, rad, q_xy, vq, cell)
    sc.check()
    assert_same(want, got)
    wsb = lib.snap_pose_score_window_workspace_bytes(1, 50, 500, X, Y)
    assert any(v.numel() * 4 == wsb for v in sc.allocations(site='pose_score_window') if v.dim() == 1)


# ----------------------------------------------------------------------------------------------------
# whole model
# ----------------------------------------------------------------------------------------------------
def _tensors(tree, prefix=''):
  if isinstance(tree, torch.Tensor):
    return [(prefix, tree)]
  out = []
  if isinstance(tree, dict):
    for k in sorted(tree, key=str):
      out += _tensors(tree[k], f'{prefix}/{k}')
  elif isinstance(tree, (list, tuple)):
    for i, v in enumerate(tree):
      out += _tensors(v, f'{prefix}/{i}')
  elif hasattr(tree, '__dict__'):
    out += _tensors({k: v for k, v in vars(tree).items() if not k.startswith('_')}, prefix)
  return out


def test_whole_model_forward_inside_the_scope():
  """One tiny BEVLocalizer forward on the default engine, outside and inside the scope: every output tensor
  bit-equal, every guard of every wrapper allocation intact.  A kernel that reads memory it was never given a
  value for (an uninitialised workspace, a row nobody wrote) cannot pass: inside the scope that memory is NaN."""
  from snap_amd.data import synthetic
  from snap_amd.models import bev_localizer
  cfg = helpers.tiny_localizer_config()
  meta = synthetic.meta_data(0.2, (6.4, 6.4, 12))
  loc = bev_localizer.BEVLocalizer(cfg, meta['build_config'].scene_config, meta['grid'].bev())
  params = helpers.params_to_device(loc.init(0, device='cpu')['params'], torch.device(DEV))
  batch = helpers.batch_to_device(synthetic.make_batch(2, meta['grid'], 3, (64, 64), seed=1), torch.device(DEV))

  def run():
    pred = loc.apply({'params': params}, batch, train=False, rngs={'sampling': 3})
    torch.cuda.synchronize()
    return pred

  want = _tensors(run())
  with guarded.scope() as sc:
    got = _tensors(run())
    sc.check()
    assert len(sc.records) > 50
  assert [n for n, _ in want] == [n for n, _ in got] and len(want) > 5
  for (name, a), (_, b) in zip(want, got):
    assert guarded.same_bits(a, b), f'{name}: differs inside the scope ({int(guarded.unwritten(b).sum())} poisoned element(s))'


def test_whole_train_step_inside_the_scope():
  """One tiny train step (forward, loss, every VJP, clipping, fused Adam), outside and inside the scope, from the
  same state: the loss, the gradient norm and every updated parameter -- hence every gradient -- bit-equal."""
  import copy
  from snap_amd import models, trainer
  from snap_amd.data import synthetic
  cfg = helpers.tiny_localizer_config(num_pose_samples=48, retries=2)
  meta = synthetic.meta_data(0.2, (6.4, 6.4, 12))
  model = models.get_model('bev_localizer')(cfg, meta)
  params0 = helpers.params_to_device(model.flax_model.init(2, device='cpu')['params'], torch.device(DEV))
  batch = helpers.batch_to_device(synthetic.make_batch(2, meta['grid'], 3, (64, 64), seed=3), torch.device(DEV))
  lr_fn = trainer.make_lr_fn(2e-3, 100)

  def run():
    state = trainer.TrainState.create(copy.deepcopy(params0), rng=0)
    state, _, logs = trainer.train_step(state, batch, model=model, lr_fn=lr_fn, max_grad_norm=10.0)
    torch.cuda.synchronize()
    return [t for _, t in trainer.flatten_params(state.params)], logs

  want, wl = run()
  with guarded.scope() as sc:
    got, gl = run()
    sc.check()
    assert len(sc.records) > 100
  assert wl['is_finite'] and gl['is_finite']
  assert wl['loss'] == gl['loss'] and wl['l2_grads'] == gl['l2_grads'], (wl['loss'], gl['loss'], wl['l2_grads'], gl['l2_grads'])
  changed = 0
  for (name, p0), a, b in zip(trainer.flatten_params(params0), want, got):
    assert guarded.same_bits(a, b), f'{name}: the updated parameter differs inside the scope'
    changed += int(not torch.equal(a, p0))
  assert changed == len(want)
