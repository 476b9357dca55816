"""`-m gpu`: every producer of GroupNorm statistics against the float64 two-pass definition on data
whose group means are large against their spread (`tests/groupnorm_reference.py`: offsets of 0 ... 256
standard deviations, exactly constant groups, a group that differs only in its last three mantissa
bits, all-negative / straddling groups under relu_first).

The statistics are those of the `y` the kernel wrote (``stats64(y.cpu())``), so the conv's own rounding
is not in the comparison; the offset enters through ``residual``, and the weight columns of the
planted exact groups are zero, so `y` equals the residual there on every engine.  Which producer ran
is asserted from ``ops.plan_conv`` / ``_snap_gn_partial`` / ``snap_conv2d_stationary_kind``.

Without the hazard re-reduction (gn_finalize_tiled_kernel taking the plain sums as they are)
every fused producer fails the variance rule on the groups at 64 and 256 standard deviations and on the
constant 3.1 / 100.3 and last-bits groups (74 of the 86 cases); the stand-alone pass passes.  Figures: tests/README.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import groupnorm_reference as R
import helpers
from snap_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
WORST = {}      # producer -> [mean share, variance share, scale share] (printed per test: -s)


def _t(a):
  return torch.from_numpy(np.ascontiguousarray(a))


def _check(y, relu_first, producer, want_fused=True):
  """ops.group_norm_stats(y) by the rule; returns (mu, sc) on the device."""
  C = y.shape[-1]
  gamma = _t(np.random.default_rng(C).standard_normal(C).astype(np.float32) * 0.3 + 1)
  if want_fused:
    assert ops.tuning().USE_FUSED_GN_STATS and R.GROUPS == 32, 'group_norm_stats would not read the sums on y'
    carried = getattr(y, '_snap_gn_partial_relu' if relu_first and not y._snap_gn_partial[2] else '_snap_gn_partial')
    assert carried[2] == relu_first, 'the sums on y are not those of this statistic'
  else:
    assert not hasattr(y, '_snap_gn_partial') or not ops.tuning().USE_FUSED_GN_STATS
  mu, sc, rstd = ops.group_norm_stats(y, gamma.to(DEV), relu_first=relu_first, want_rstd=True)
  ref = R.stats64(y.cpu().numpy(), relu_first=relu_first)
  m, v = R.shares(R.per_group(mu.cpu().numpy()), R.per_group(rstd.cpu().numpy()), ref)
  s = R.scale_share(sc.cpu().numpy(), rstd.cpu().numpy(), gamma.numpy())
  w = WORST.setdefault(producer, [0.0, 0.0, 0.0])
  w[:] = [max(w[0], float(m.max())), max(w[1], float(v.max())), max(w[2], float(s.max()))]
  bad = np.argwhere((m > 1) | (v > 1))
  print(f'GNSTAT {producer} relu_first={int(relu_first)} {tuple(y.shape)}: mean {m.max():.3g} variance {v.max():.3g} '
        f'scale {s.max():.3g} of the tolerance; {len(bad)} groups over: '
        + ', '.join(f'(n{n} g{g} r{R.ratio_of(n, g)} {m[n, g]:.2g}/{v[n, g]:.2g})' for n, g in bad[:12]))
  assert m.max() <= 1 and v.max() <= 1, f'{producer}: {len(bad)} (image, group) outside the rule'
  assert s.max() <= 1, f'{producer}: sc is not rstd * gamma to one rounding'
  return mu, sc


def _layer(N, H, W, Cin, Cout, k, seed, relu_first, gn_prologue):
  """x, w, the offset field as the residual, conv kwargs.  The conv adds about CONV_STD of noise."""
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(N, H, W, Cin, generator=g)
  field, pl = R.offset_field(N, H * W, Cout, seed, R.GROUP_STD, relu_first)
  w = torch.randn(k, k, Cin, Cout, generator=g) * (R.CONV_STD / np.sqrt(k * k * Cin))
  cpg = Cout // R.GROUPS
  for grp in pl.exact_groups:
    w[..., grp * cpg:(grp + 1) * cpg] = 0
  kw = dict(padding=((k // 2, k // 2), (k // 2, k // 2)), residual=_t(field).reshape(N, H, W, Cout).to(DEV))
  xd = x.to(DEV)
  if gn_prologue:
    g_in = (torch.randn(Cin, generator=g) * 0.3 + 1).to(DEV)
    b_in = (torch.randn(Cin, generator=g) * 0.3).to(DEV)
    mu, sc = ops.group_norm_stats(xd, g_in)
    kw.update(prologue=ops.PRO_GN_RELU, gn=(mu, sc, b_in))
  return xd, w.to(DEV), kw, pl, field


def _exact_groups_hold(y, field, pl):
  cpg = y.shape[-1] // R.GROUPS
  yv = y.cpu().numpy().reshape(field.shape)
  for name, (n, grp) in pl.where.items():
    if name.startswith(('const', 'last')):
      sl = slice(grp * cpg, (grp + 1) * cpg)
      assert np.array_equal(yv[n, :, sl], field[n, :, sl]), name


def _conv(shape, math, emit, seed, gn_prologue, expect):
  """One emitting launch; `expect`: ConvPlan fields the launch must have."""
  N, H, W, Cin, Cout, k = shape
  xd, w, kw, pl, field = _layer(N, H, W, Cin, Cout, k, seed, emit != 'raw', gn_prologue)
  p = ops.plan_conv(xd, w, emit_gn_stats=emit, math=math, **kw)
  for name, val in expect.items():
    got = getattr(p, name)
    assert (val(got) if callable(val) else got == val), (name, got)
  y = ops.conv2d(xd, w, emit_gn_stats=emit, math=math, **kw)
  assert y._snap_gn_partial[1] == p.tile_rows and y._snap_gn_partial[2] == (emit == 'relu')
  _exact_groups_hold(y, field, pl)
  return y, pl


def _standalone(y, relu_first, producer):
  with ops.tuning_scope(USE_FUSED_GN_STATS=False):
    _check(y, relu_first, producer, want_fused=False)


# ---- the tiled epilogues (conv_igemm.hip, conv_split.hip incl. its halo body at 3 x 3, conv_bf16.hip)
TILED = [
    ((2, 34, 34, 64, 64, 3), None),           # 64-wide tiles
    ((5, 16, 16, 128, 256, 1), None),         # HW = 2 tiles exactly
    ((40, 12, 12, 64, 256, 1), None),         # tiles straddle images
    ((7, 9, 11, 64, 256, 1), '64x64'),        # images of 99 pixels
]


@pytest.mark.parametrize('emit', ['raw', 'relu'])
@pytest.mark.parametrize('math', ['f32', 'bf16x3', 'bf16x6', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape,tile', TILED, ids=['34x34-3x3', '16x16', '40x12x12', '99px'])
def test_tiled_epilogue(shape, tile, math, emit):
  with ops.tuning_scope(USE_SPLITK=False, CONV_TILE=tile):
    y, _ = _conv(shape, math, emit, 11, False,
                 dict(tag='', stats_count=1, gn_partial_rows=0, workspace_bytes=0, tile_rows=lambda t: 0 < t <= shape[1] * shape[2],
                      stats_relu=emit == 'relu'))
    _check(y, emit == 'relu', f'tiled epilogue {math}')
    if math == 'f32':
      _standalone(y, emit == 'relu', 'stand-alone pass')


@pytest.mark.parametrize('math', ['bf16x3', 'bf16x6'])
def test_both_statistics_from_one_epilogue(math):
  with ops.tuning_scope(USE_SPLITK=False, CONV_TILE='128x128'):
    y, _ = _conv((3, 33, 40, 64, 256, 1), math, 'both', 12, True, dict(tag='', stats_count=2, tile_rows=128))
    assert hasattr(y, '_snap_gn_partial_relu')
    for relu_first in (False, True):
      _check(y, relu_first, f"'both' epilogue {math}")


@pytest.mark.parametrize('emit', ['raw', 'relu'])
@pytest.mark.parametrize('math', ['bf16x3', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape', [(3, 17, 19, 512, 512, 3), (5, 9, 7, 1024, 256, 1)], ids=['3x3-K4608', '1x1-K1024'])
def test_split_k_reduce(shape, math, emit):
  y, _ = _conv(shape, math, emit, 13, True,
               dict(stats_count=1, gn_partial_rows=32, tile_rows=32, workspace_bytes=lambda b: b > 0))
  _check(y, emit == 'relu', f'split-K reduce {math}')


# ---- the pre-split engine (conv_ps.hip): 128- and 256-row tiles
@pytest.mark.parametrize('emit', ['raw', 'relu', 'both'])
@pytest.mark.parametrize('ps_tile,rows', [(1, 128), (2, 256)])
def test_presplit_engine_epilogue(ps_tile, rows, emit):
  N, H, W, Cin, Cout = 3, 31, 29, 64, 256                 # HW = 899: tiles straddle images
  xd, w, kw, pl, field = _layer(N, H, W, Cin, Cout, 1, 21, emit != 'raw', False)
  ps = ops.presplit(xd)
  kw = dict(residual=kw['residual'], emit_gn_stats=emit, ps_tile=ps_tile)
  p = ops.plan_conv(ps, w, **kw)
  assert (p.tag, p.tile_rows, p.stats_count, p.workspace_bytes) == ('PS_', rows, 2 if emit == 'both' else 1, 0)
  y = ops.conv2d(ps, w, **kw)
  assert y._snap_gn_partial[1] == rows and y._snap_gn_partial[2] == (emit == 'relu')
  _exact_groups_hold(y, field, pl)
  if emit != 'relu':
    _check(y, False, f'pre-split engine {rows} rows')
  if emit != 'raw':
    assert emit == 'relu' or hasattr(y, '_snap_gn_partial_relu')
    _check(y, True, f'pre-split engine {rows} rows')


# ---- conv_rs.hip
def _kind(N, H, W, Cin, Cout, k, tile_hint, epilogue=ops.EPI_RESIDUAL):
  d = _lib.SnapConvDesc(N=N, H=H, W=W, Cin=Cin, Cin_stride=Cin, KH=k, KW=k, stride=1, pad_t=k // 2, pad_l=k // 2,
                        Ho=H, Wo=W, Cout=Cout, Cout_stride=Cout, prologue=ops.PRO_GN_RELU, epilogue=epilogue,
                        in_scale=1.0, in_shift=0.0, tile_hint=tile_hint + 1000000 * ops._stationary_mode())
  return int(_lib.load().snap_conv2d_stationary_kind(ctypes.byref(d), 2))


@pytest.mark.parametrize('emit', ['raw', 'both'])
@pytest.mark.parametrize('shape,kind', [((3, 20, 23, 64, 256, 1), 2), ((7, 9, 11, 64, 256, 1), 2), ((5, 16, 17, 128, 512, 1), 2),
                                        ((3, 23, 17, 256, 1024, 1), 1)],
                         ids=['ws-64', 'ws-64-99px', 'ws-128', 'rs-256'])
def test_stationary_1x1(shape, kind, emit):
  with ops.tuning_scope(USE_SPLITK=False, CONV_TILE='128x128', CONV_RS_FORCE=True):
    assert _kind(*shape, 128128) == kind
    y, _ = _conv(shape, 'bf16x3', emit, 14, True,
                 dict(tag='WS_' if kind == 2 else 'RS_', stats_count=1 if emit == 'raw' else 2,
                      tile_rows=32 if kind == 2 else 128))
    name = 'weights-stationary 1x1' if kind == 2 else 'row-stationary 1x1'
    _check(y, False, name)
    if emit == 'both':
      assert hasattr(y, '_snap_gn_partial_relu')
      _check(y, True, name)


@pytest.mark.parametrize('emit', ['raw', 'relu'])
@pytest.mark.parametrize('N,H,W', [(2, 9, 91), (3, 11, 85)])
def test_weights_stationary_3x3(N, H, W, emit):
  """The kernel takes no residual (only a ReLU epilogue), so the offset comes out of the conv itself:
  input channels 0-31 are made the constant 1 by the prologue (sc = 0, beta = 1) and reach output channel
  c through the centre tap only (never padded) with weight offset_c / 32 -- a power-of-two scaling, the
  same sum at every pixel; channels 32-63 carry the noise.  The constant groups have no noise columns
  and must come out exactly constant.  (No last-bits group: this conv cannot write one.)"""
  with ops.tuning_scope(CONV_RS_FORCE=True):       # (the kernel below its row-count threshold)
    assert _kind(N, H, W, 64, 64, 3, 0, 0) == 3
    g = torch.Generator().manual_seed(15)
    xd = torch.randn(N, H, W, 64, generator=g).to(DEV)
    mu, sc = ops.group_norm_stats(xd, torch.ones(64, device=DEV))
    sc[:, :32] = 0
    beta = torch.zeros(64)
    beta[:32] = 1
    w = torch.zeros(3, 3, 64, 64)
    w[:, :, 32:, :] = torch.randn(3, 3, 32, 64, generator=g) / np.sqrt(9 * 32 * 0.34)     # (var relu(N(0, 1)) = 0.34)
    const = {5 + 8 * i: c for i, c in enumerate(R.CONSTANTS)}
    for grp in range(32):
      off = const.get(grp, float(R.ratio_of(0, grp)))
      w[1, 1, :32, 2 * grp:2 * grp + 2] = off / 32
      if grp in const:
        w[:, :, 32:, 2 * grp:2 * grp + 2] = 0
    kw = dict(padding=((1, 1), (1, 1)), prologue=ops.PRO_GN_RELU, gn=(mu, sc, beta.to(DEV)), emit_gn_stats=emit, math='bf16x3')
    p = ops.plan_conv(xd, w.to(DEV), **kw)
    assert (p.tag, p.stats_count, p.tile_rows) == ('WS_', 1, -H * ((W + 29) // 30))
    y = ops.conv2d(xd, w.to(DEV), **kw)
    assert y._snap_gn_partial[1] == p.tile_rows
    yv = y.cpu().numpy().reshape(N, H * W, 32, 2)
    for grp, c in const.items():
      assert (yv[:, :, grp, :] == yv[0, 0, grp, 0]).all() and abs(yv[0, 0, grp, 0] - c) < 1e-3 * c
    _check(y, emit == 'relu', 'weights-stationary 3x3')


def test_halo_body_3x3():
  """Several images per row tile on the halo body of the split engine (the shape of
  test_conv_split_halo_3x3's last case, which that test runs on the same body)."""
  with ops.tuning_scope(USE_SPLITK=False):
    assert _kind(4, 13, 13, 32, 128, 3, 0) == 0
    y, _ = _conv((4, 13, 13, 32, 128, 3), 'bf16x3', 'raw', 16, True, dict(tag='', stats_count=1, gn_partial_rows=0))
    _check(y, False, 'halo body 3x3')


# ---- the stand-alone pass
@pytest.mark.parametrize('relu_first', [False, True])
@pytest.mark.parametrize('N,HW,C', [(2, 40 * 37, 32), (2, 40 * 37, 64), (3, 72, 1024), (2, 72, 2048)])
def test_stand_alone_pass(N, HW, C, relu_first):
  assert R.gn_plan(N, HW, C)[0] > 1
  v, _ = R.values(N, HW, C, 17, relu_first)
  _check(_t(v).reshape(N, 1, HW, C).to(DEV), relu_first, 'stand-alone pass', want_fused=False)


# ---- where the statistic lands
def test_fused_statistics_through_the_consuming_conv():
  """A GroupNorm -> ReLU 1 x 1 conv (exact f32 engine) reading (mu, sc) of the fused route on the offset
  input, against the float64 conv of the float64-normalised y at test_gn_stats_and_fused_conv's bounds.
  The consumer's weight rows of the last-bits group are zero: that group's mean (100 + 3.5 ulp) is not an
  f32 number, and rstd = 316 turns the half ulp any f32 `mu` is off by into 1e-3 of the normalised value."""
  shape = (5, 16, 16, 128, 256, 1)
  with ops.tuning_scope(USE_SPLITK=False):
    y, pl = _conv(shape, 'f32', 'raw', 18, False, dict(tag='', stats_count=1))
    mu, sc = _check(y, False, 'tiled epilogue f32')
  g = torch.Generator().manual_seed(19)
  C, Co = 256, 64
  beta = torch.randn(C, generator=g) * 0.2
  w = torch.randn(1, 1, C, Co, generator=g) / np.sqrt(C)
  grp = pl.where['last bits'][1]
  w[:, :, grp * 8:(grp + 1) * 8] = 0
  got = ops.conv2d(y, w.to(DEV), prologue=ops.PRO_GN_RELU, gn=(mu, sc, beta.to(DEV)), math='f32')
  gamma = np.random.default_rng(C).standard_normal(C).astype(np.float32) * 0.3 + 1      # (_check's gamma)
  ref = R.stats64(y.cpu().numpy())
  y64 = y.cpu().numpy().astype(np.float64).reshape(5, 256, 32, 8)
  xh = (y64 - ref['mean'][:, None, :, None]) * ref['rstd'][:, None, :, None]
  xh = np.maximum(xh.reshape(5, 256, C) * gamma.astype(np.float64) + beta.numpy().astype(np.float64), 0)
  want = xh @ w.numpy().astype(np.float64).reshape(C, Co)
  err = np.abs(got.cpu().numpy().reshape(5, 256, Co) - want)
  share = float((err / (3e-5 + 1e-5 * np.abs(want))).max())
  print(f'GNSTAT consumer conv: max err {err.max():.3g}, {share:.3g} of the tolerance')
  assert share <= 1


# ---- containment
@pytest.mark.parametrize('bad', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('producer', ['tiled', 'ws'])
def test_non_finite_value_stays_in_its_group(producer, bad):
  """One NaN / inf in the first pixel of image 1 (a row tile / slab it shares with the tail of image 0):
  exactly that (image, group)'s mu and sc are non-finite, every other entry keeps the clean run's bits."""
  shape, scope, math = {
      'tiled': ((3, 17, 19, 64, 128, 1), dict(USE_SPLITK=False), 'f32'),                 # HW = 323: 64-row tiles straddle
      'ws': ((7, 9, 11, 64, 256, 1), dict(USE_SPLITK=False, CONV_TILE='128x128', CONV_RS_FORCE=True), 'bf16x3'),
  }[producer]
  N, H, W, Cin, Cout, k = shape
  cpg = Cout // R.GROUPS
  n, grp = 1, 7                    # (ratio 0; its tile neighbour (0, 7), at -256 std, is one the finalize re-reduces)
  with ops.tuning_scope(**scope):
    xd, w, kw, _, _ = _layer(N, H, W, Cin, Cout, k, 20, False, producer == 'ws')
    gamma = torch.ones(Cout, device=DEV)
    out = []
    for plant in (False, True):
      if plant:
        kw['residual'] = kw['residual'].clone()
        kw['residual'][n, 0, 0, grp * cpg + 1] = bad
      y = ops.conv2d(xd, w, emit_gn_stats='raw', math=math, **kw)
      assert y._snap_gn_partial[1] == (32 if producer == 'ws' else 64)
      assert plant == (not bool(torch.isfinite(y).all()))
      out.append([t.cpu() for t in ops.group_norm_stats(y, gamma)])
  hit = torch.zeros(N, Cout, dtype=torch.bool)
  hit[n, grp * cpg:(grp + 1) * cpg] = True
  for clean, dirty in zip(*out):
    assert torch.isfinite(clean).all()
    assert not torch.isfinite(dirty[hit]).any()
    assert torch.equal(clean[~hit], dirty[~hit])
