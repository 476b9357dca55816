"""`-m gpu`: the reduction and element-wise VJP kernels of ``encoder_bwd.hip`` (and the forward multi-launch of weight
standardisation) against float64 at their dispatch edges.

**A** GroupNorm VJP (reduce paths, the 64 KiB LDS switch, slab plans, offset data, a planted exact case, the statistics
from the dgrad epilogue), **B** weight standardisation (single and multi launches, offset columns), **C** the gate +
column-sum kernels (f32, bf16, fp16, weighted sums, the tail quad), **D** ``upsample2x_bwd``, **E** the max-pool VJP.
Inputs, float64 formulas, bounds and the restated launchers live in ``encoder_vjp_reference.py``;
``test_encoder_vjp_reference.py`` shows on the CPU that the formulas are the VJPs, that every case takes its path and
that the bounds reject the named mutants.  A result passes at ``max err / bound <= 1``.
"""
import numpy as np
import pytest
import torch

import encoder_vjp_reference as R
import groupnorm_reference as gr
import helpers
from snap_amd import ops, ops_bwd

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
MODE = {R.GN_RELU: ops.PRO_GN_RELU, R.RELU_GN: ops.PRO_RELU_GN}
HALF = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def dev(a, dtype=None):
  if a is None:
    return None
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
  return t if dtype is None else t.to(dtype)


def host(t):
  return t.float().cpu().numpy() if t.dtype in HALF.values() else t.cpu().numpy()


def canon(a):
  """-0.0 -> +0.0: the sign of an exact zero is not part of a sum's value."""
  return np.asarray(a, np.float32) + np.float32(0)


def report(label, got, ref, bound, op):
  r = R.ratio(got, ref, bound, op)
  print(f'[encoder vjp] {label}: max err / bound = {r:.4f}')
  return r


# ----------------------------------------------------------------------------------------------------
# A. GroupNorm VJP
# ----------------------------------------------------------------------------------------------------
def run_gn(c, half=None, tensors=None):
  N, H, W, C = c['shape']
  img = lambda a: dev(None if a is None else a.reshape(N, H, W, C))
  x, dz = tensors if tensors is not None else (img(c['x']), img(c['dz']))
  dx, dgamma, dbeta = ops_bwd.group_norm_bwd(x, dz, dev(c['mu']), dev(c['rstd']), dev(c['gamma']), dev(c['beta']),
                                             MODE[c['mode']], groups=c['groups'], add=img(c['add']), half=half)
  out = dict(dx=host(dx).reshape(N, H * W, C), dgamma=host(dgamma), dbeta=host(dbeta))
  if half is not None:
    out['twin'] = ops_bwd.half_twin(dx, half)
  return out, dx


def check_gn(label, got, c, chain=None):
  ref = R.gn_vjp_ref(*R.gn_args(c), chain=chain)
  return max(report(f'{label} {k}', got[k], *ref[k], 'gn_' + k) for k in ('dx', 'dgamma', 'dbeta'))


@pytest.mark.parametrize('mode', R.GN_MODES)
@pytest.mark.parametrize('name', R.GN_CASE_IDS)
def test_groupnorm_vjp_reduce_paths_lds_switch_and_slab_plans(name, mode):
  c = R.gn_case(name, mode)
  N, H, W, C = c['shape']
  assert R.gn_reduce_path(N, C, c['groups']) == c['path'] and R.gn_plan_b(N, H * W, C) == c['plan']
  assert int(R.gn_gate_offenders(c['x'], c['gamma'], c['beta'], mode, c['groups'], c['mu'], c['rstd']).sum()) == 0
  got, _ = run_gn(c)
  worst = check_gn(f'gn {name} {mode} {c["path"]} S={c["plan"][0]} lds={R.gn_lds_bytes(N, C, c["groups"])}', got, c)
  assert worst <= 1.0
  if C % 8 == 0:                                   # the rounded twin does not change the f32 result
    again, dx = run_gn(c, half='bf16')
    assert again['twin'] is not None and R.bits_equal(again['dx'], got['dx'])
    assert torch.equal(again['twin'], dx.to(torch.bfloat16))


def gpu_stats(shape, gamma, relu_first):
  N, H, W, C = shape

  def stats(v):
    mu, _, rstd = ops.group_norm_stats(dev(v.reshape(N, H, W, C)), dev(gamma), relu_first=relu_first, want_rstd=True)
    return host(mu), host(rstd)
  return stats


@pytest.mark.parametrize('mode', R.GN_MODES)
def test_groupnorm_vjp_on_offset_data_with_the_kernels_own_statistics(mode):
  c = R.gn_offset_inputs(mode, gr.offset_field)
  N, H, W, C = c['shape']
  stats = gpu_stats(c['shape'], c['gamma'], mode == R.RELU_GN)
  x, mu, rstd, moved = R.gn_settle_gate(c['x'], c['gamma'], c['beta'], mode, 32, stats)
  c.update(x=x, mu=mu, rstd=rstd)
  assert int(R.gn_gate_offenders(x, c['gamma'], c['beta'], mode, 32, mu, rstd).sum()) == 0
  got, _ = run_gn(c)
  assert check_gn(f'gn offset-data {mode} (nudged {moved})', got, c) <= 1.0
  n, g = c['planted'].where['const 3.1']
  cpg = C // 32
  assert abs(float(rstd[n, g * cpg]) * np.sqrt(1e-5) - 1) < 1e-5          # a constant group: rstd = 1 / sqrt(eps)
  if mode == R.RELU_GN:                                                     # a group below zero: dx is the add alone
    n, g = c['planted'].where['all negative']
    sl = slice(g * cpg, (g + 1) * cpg)
    assert R.bits_equal(got['dx'][n, :, sl], c['add'][n, :, sl])


@pytest.mark.parametrize('mode', R.GN_MODES)
@pytest.mark.parametrize('C,groups', R.GN_EXACT)
def test_groupnorm_vjp_planted_exact_case(C, groups, mode):
  c = R.gn_exact_case(mode, C, groups)
  assert R.gn_reduce_path(c['shape'][0], C, groups) == c['path']
  ref = R.gn_vjp_ref(*R.gn_args(c))
  got, _ = run_gn(c)
  for k in ('dx', 'dgamma', 'dbeta'):
    want = ref[k][0].astype(np.float32)
    bad = np.argwhere(canon(got[k]).view(np.uint32) != canon(want).view(np.uint32))
    assert len(bad) == 0, f'{k}: {len(bad)} differ, first at {bad[0].tolist()}'
    print(f'[encoder vjp] gn exact {mode} C={C} {c["path"]} {k}: max err / bound = 0.0000 (bit for bit)')
  x = c['x']
  if mode == R.RELU_GN:
    assert (got['dx'][x <= 0] == 0).all()
  else:
    # a closed gate (z = 0 through x = +-0 or gamma = 0) contributes nothing: its dx holds the group terms alone
    closed = np.broadcast_to((x == 0) | (c['gamma'] == 0)[None, None, :], x.shape)
    open_ = R.gn_vjp_f32(*R.gn_args(c), mutant='gate_ge')['dx']
    assert closed.any() and not R.same_values(open_, got['dx'])


@pytest.mark.parametrize('N,H,W,C,Cnext,k,mode,acc', R.GN_FUSED_SHAPES)
def test_groupnorm_vjp_fused_statistics_within_the_float64_bound(N, H, W, C, Cnext, k, mode, acc, monkeypatch):
  """The statistics pass taken in the epilogue of the data-gradient launch (``ops.conv2d(gn_bwd_stats=)``), held to the
  bound of the stand-alone pass with the chain its tiles can form: the rows of a tile plus the slots of an image."""
  monkeypatch.setattr(ops, 'USE_SPLITK', False)
  rng = np.random.default_rng(470 + C)
  gam = (rng.standard_normal(C) * 0.3 + 1).astype(np.float32)
  beta = (rng.standard_normal(C) * 0.2).astype(np.float32)
  x0 = (rng.standard_normal((N, H * W, C)) * 1.5 + 0.4).astype(np.float32)
  x, mu, rstd, _ = R.gn_settle_gate(x0, gam, beta, mode, 32, gpu_stats((N, H, W, C), gam, mode == R.RELU_GN))
  xd, mud, rsd, gd, bd = dev(x.reshape(N, H, W, C)), dev(mu), dev(rstd), dev(gam), dev(beta)
  dyh = dev(rng.standard_normal((N, H, W, Cnext)).astype(np.float32)).to(torch.bfloat16)
  w_rot = dev((rng.standard_normal((k, k, Cnext, C)) / np.sqrt(k * k * Cnext)).astype(np.float32))
  res = dev(rng.standard_normal((N, H, W, C)).astype(np.float32)) if acc else None
  pad = (k - 1) // 2
  dz = ops.conv2d(dyh, w_rot, padding=((pad, pad), (pad, pad)), residual=res, math='bf16',
                  gn_bwd_stats=(xd, mud, rsd, gd, bd, MODE[mode]))
  held = getattr(dz, '_snap_gnb_partial', None)
  assert held is not None
  tile_rows = int(held[1])
  c = dict(shape=(N, H, W, C), mode=mode, groups=32, x=x, dz=host(dz).reshape(N, H * W, C), add=None, gamma=gam,
           beta=beta, mu=mu, rstd=rstd)
  fused, _ = run_gn(c, tensors=(xd, dz))
  monkeypatch.setattr(ops_bwd, 'USE_GNB_STATS', False)
  plain, _ = run_gn(c, tensors=(xd, dz))
  chain = tile_rows + H * W // tile_rows + 2
  assert check_gn(f'gn fused-statistics {N}x{H}x{W}x{C} tile_rows={tile_rows}', fused, c, chain=max(chain, R.gn_chain(N, H * W, C))) <= 1.0
  assert check_gn(f'gn stand-alone {N}x{H}x{W}x{C}', plain, c) <= 1.0
  assert not R.bits_equal(fused['dgamma'], plain['dgamma']) or C * H * W < 4096      # (really another pass)


# ----------------------------------------------------------------------------------------------------
# B. weight standardisation
# ----------------------------------------------------------------------------------------------------
def hwio(a, shape):
  return dev(a.reshape(shape))


def run_ws(c):
  w, g = hwio(c['w'], c['shape']), hwio(c['dws'], c['shape'])
  return host(ops.weight_standardize(w)).reshape(c['w'].shape), host(ops_bwd.weight_standardize_bwd(w, g)).reshape(c['w'].shape)


@pytest.mark.parametrize('shape', R.WS_SHAPES, ids=[str(s) for s in R.WS_SHAPES])
def test_weight_standardisation_shapes(shape):
  c = R.ws_case(shape)
  ref = R.ws_ref(c['w'], c['dws'])
  fwd, bwd = run_ws(c)
  if shape[0] * shape[1] * shape[2] == 1:                 # K = 1: sigma = sqrt(eps), everything is exactly zero
    assert (fwd == 0).all() and (bwd == 0).all()
  assert report(f'ws fwd {shape}', fwd, *ref['fwd'], 'ws_fwd') <= 1.0
  assert report(f'ws bwd {shape}', bwd, *ref['bwd'], 'ws_bwd') <= 1.0


@pytest.mark.parametrize('offset', R.WS_OFFSETS)
def test_weight_standardisation_offset_columns(offset):
  c = R.ws_case(R.WS_OFFSET_SHAPE, offset)
  ref = R.ws_ref(c['w'], c['dws'])
  fwd, bwd = run_ws(c)
  share = float((ref['bwd'][1] / np.maximum(np.abs(ref['bwd'][0]), 1e-30)).mean())
  print(f'[encoder vjp] ws offset m/s={offset:g}: mean rounding {float(ref["mean_round"].max()):.3e} of a unit of ws, '
        f'mean bound / abs(dw) {share:.3e}, max abs err dw {float(np.abs(bwd - ref["bwd"][0]).max()):.3e}')
  assert report(f'ws fwd offset m/s={offset:g}', fwd, *ref['fwd'], 'ws_fwd') <= 1.0
  assert report(f'ws bwd offset m/s={offset:g}', bwd, *ref['bwd'], 'ws_bwd') <= 1.0


@pytest.mark.parametrize('name', sorted(R.WS_MULTI))
def test_weight_standardisation_multi_launches(name):
  idx = R.WS_MULTI[name]
  cs = R.ws_multi_cases(name)
  ws = [hwio(c['w'], c['shape']) for c in cs]
  gs = [hwio(c['dws'], c['shape']) for c in cs]
  fwd, bwd = ops.weight_standardize_multi(ws), ops.weight_standardize_bwd_multi(ws, gs)
  worst = 0.0
  for j, c in enumerate(cs):
    ref = R.ws_ref(c['w'], c['dws'])
    assert torch.equal(fwd[j], ops.weight_standardize(ws[j])), f'forward item {j} {c["shape"]}'
    assert torch.equal(bwd[j], ops_bwd.weight_standardize_bwd(ws[j], gs[j])), f'backward item {j} {c["shape"]}'
    worst = max(worst, R.ratio(host(fwd[j]).reshape(c['w'].shape), *ref['fwd'], 'ws_fwd'),
                R.ratio(host(bwd[j]).reshape(c['w'].shape), *ref['bwd'], 'ws_bwd'))
  print(f'[encoder vjp] ws multi {name} ({len(idx)} items, {R.wstd_table([c["shape"] for c in cs])[1]} workgroups): '
        f'max err / bound = {worst:.4f}; bit-identical to the single launches')
  assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------
# C. gate + column sums
# ----------------------------------------------------------------------------------------------------
def rc_tensor(rc):
  return None if rc is None else torch.tensor([rc], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize('C', R.COLSUM_C_FUSED + R.COLSUM_C_FALLBACK)
def test_gate_and_column_sums_f32(C):
  path = R.epilogue_colsum_path(C)
  assert path == ('fallback' if C in R.COLSUM_C_FALLBACK else 'fused')
  kern = R.colsum_kernel_of(C)
  worst = {}
  held = {}
  for M, c, use_mask, rc, relu in R.gate_variants_f32(C):
    if M not in held:
      held = {M: (dev(c['dy']), dev(c['y']), dev(c['mask']))}
    dy, y, mask = held[M]
    ref = R.gate_ref(c['dy'], c['y'], c['mask'] if use_mask else None, relu, rc, kern)
    out, sums = ops_bwd.epilogue_bwd_colsum(dy, y if relu else None, mask if use_mask else None, relu=relu,
                                            row_count=rc_tensor(rc))
    n = ref['Msum']
    assert R.same_values(host(out)[:n], ref['out'][:n].astype(np.float32)), (M, use_mask, rc, relu)
    r = R.ratio(host(sums), *ref['sums'], 'colsum')
    assert r <= 1.0, (M, use_mask, rc, relu, r)
    worst[M] = max(worst.get(M, 0.0), r)
  for M, r in worst.items():
    print(f'[encoder vjp] gate+colsum f32 M={M} C={C} {path}/{kern} slabs={R.colsum_slabs(M)}: max err / bound = {r:.4f}')
  M, c = R.COLSUM_M[-1], R.colsum_case(R.COLSUM_M[-1], C, exact=True)
  ref = R.gate_ref(c['dy'], c['y'], c['mask'], True, None, kern)
  out, sums = ops_bwd.epilogue_bwd_colsum(dev(c['dy']), dev(c['y']), dev(c['mask']), relu=True)
  assert R.same_values(host(out), ref['out'].astype(np.float32))
  assert R.bits_equal(canon(host(sums)), canon(ref['sums'][0]))          # small integers: exact sums, bit for bit


@pytest.mark.parametrize('C', R.HALF_C)
@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
def test_gate_and_column_sums_half(kind, C):
  worst = {}
  held = {}
  for M, exact, h, rc, relu in R.gate_variants_half(C, kind):
    if (M, exact) not in held:
      held = {(M, exact): (dev(h['dy'], HALF[kind]), dev(h['y'], HALF[kind]), dev(h['x2']), dev(h['rows']))}
      dy, y, x2, rows = held[(M, exact)]
      assert np.array_equal(host(dy), h['dy']) and np.array_equal(host(y), h['y'], equal_nan=True)
    w_ = worst.setdefault(M, {'colsum': 0.0, 'wsum': 0.0, 'dtail': 0.0})
    ref = R.gate_ref(h['dy'], h['y'], None, relu, rc)
    n = ref['Msum']
    out, sums = ops_bwd.epilogue_bwd_colsum(dy, y if relu else None, relu=relu, row_count=rc_tensor(rc))
    assert out.dtype == HALF[kind] and R.same_values(host(out)[:n], ref['out'][:n].astype(np.float32))
    r = R.ratio(host(sums), *ref['sums'], 'colsum')
    assert r <= 1.0, (M, rc, relu, r)
    w_['colsum'] = max(w_['colsum'], r)
    if exact:
      assert R.bits_equal(canon(host(sums)), canon(ref['sums'][0]))
    for wrelu in (False, True):
      wgt = R.half_weight(h, kind, wrelu)
      ref = R.gate_ref(h['dy'], h['y'], None, relu, rc, weight=wgt)
      dtail = None
      if C == 256:
        dx0 = np.random.default_rng(M).standard_normal((M + 3, 260)).astype(np.float32)
        dxt = dev(dx0)
        dtail = (dev(h['wtail']), dxt)
      out, sums, wsum = ops_bwd.epilogue_bwd_colsum(dy, y if relu else None, relu=relu, row_count=rc_tensor(rc),
                                                    wsum=(x2, 256, rows, wrelu), dtail=dtail)
      assert R.same_values(host(out)[:n], ref['out'][:n].astype(np.float32))
      r1, r2 = R.ratio(host(sums), *ref['sums'], 'colsum'), R.ratio(host(wsum), *ref['wsum'], 'wsum')
      assert r1 <= 1.0 and r2 <= 1.0, (M, rc, relu, wrelu, r1, r2)
      w_['wsum'] = max(w_['wsum'], r2)
      if exact:
        assert R.bits_equal(canon(host(wsum)), canon(ref['wsum'][0]))
      if dtail is not None:
        got = host(dxt)
        live = h['rows'][:n]
        wt = R.round_half(h['wtail'], kind)
        dot, bound = R.dtail_ref(ref['out'][:n], wt)
        r3 = R.ratio(got[live, 256], dot, bound, 'dtail')
        assert r3 <= 1.0, (M, rc, relu, r3)
        w_['dtail'] = max(w_['dtail'], r3)
        if exact:
          assert R.bits_equal(canon(got[live, 256]), canon(dot))
        assert (got[live, 257:] == 0).all() and not np.signbit(got[live, 257:]).any()
        keep = np.ones_like(dx0, bool)
        keep[live, 256:] = False
        assert R.bits_equal(got[keep], dx0[keep]), 'an element outside the written quads changed'
  for M, w_ in worst.items():
    print(f'[encoder vjp] gate+colsum {kind} M={M} C={C}: max err / bound = {w_["colsum"]:.4f}, '
          f'wsum {w_["wsum"]:.4f}, dtail {w_["dtail"]:.4f}')


# ----------------------------------------------------------------------------------------------------
# D. bilinear x2 up-sample VJP
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.UP_SHAPES, ids=[str(s) for s in R.UP_SHAPES])
def test_upsample2x_vjp(shape):
  dy = R.up_case(shape)
  ref, bound = R.up_ref(dy)
  assert np.abs(ref - R.up_autograd(dy)).max() <= 1e-12 * max(1.0, np.abs(ref).max())
  assert report(f'upsample2x bwd {shape}', host(ops_bwd.upsample2x_bwd(dev(dy))), ref, bound, 'upsample') <= 1.0
  ex = R.up_case(shape, exact=True)                            # weights are multiples of 1 / 16: exact on integers
  assert R.bits_equal(canon(host(ops_bwd.upsample2x_bwd(dev(ex)))), canon(R.up_autograd(ex)))
  ones = host(ops_bwd.upsample2x_bwd(dev(np.ones_like(dy))))
  assert (ones == 4).all()                                      # every coarse pixel's weights sum to 2 per axis


# ----------------------------------------------------------------------------------------------------
# E. 3 x 3 / 2 max-pool VJP
# ----------------------------------------------------------------------------------------------------
def pool(x, dy):
  return host(ops_bwd.max_pool_3x3s2_bwd(dev(x), dev(dy)))


def per_pixel_twin(x, dy):
  """The same channels through the other kernel family: (tiled result, per-pixel result) on the shared channels."""
  C = x.shape[3]
  if C % 4 == 0:
    c1 = C - 1
    return pool(x, dy)[..., :c1], pool(np.ascontiguousarray(x[..., :c1]), np.ascontiguousarray(dy[..., :c1]))
  padc = lambda a: np.ascontiguousarray(np.concatenate([a, a[..., :4 - C % 4]], axis=3))
  return pool(padc(x), padc(dy))[..., :C], pool(x, dy)


@pytest.mark.parametrize('shape,path', R.POOL_SHAPES, ids=[str(s) for s, _ in R.POOL_SHAPES])
def test_max_pool_vjp(shape, path):
  assert R.maxpool_path(shape[0], shape[3]) == path
  x, dy = R.pool_case(shape, ties=True)
  want = R.pool_autograd(x, dy)
  got = pool(x, dy)
  assert R.bits_equal(canon(got), canon(want)), 'ties must go to the first maximum in scan order'
  xr, dyr = R.pool_case(shape, ties=False)
  assert report(f'maxpool bwd {shape} {path}', pool(xr, dyr), R.pool_ref(xr, dyr), R.pool_bound(xr, dyr), 'maxpool') <= 1.0
  # NaNs: the tiled and the per-pixel kernel select the same set
  rng = np.random.default_rng(9)
  xn = (x + rng.standard_normal(shape).astype(np.float32) * 0.1).astype(np.float32)
  xn[rng.random(shape) < 0.05] = np.nan
  xn[0, :3, :3] = np.nan
  a, b = per_pixel_twin(xn, dyr)
  assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
  # whole windows of -inf and a constant plane: same bits on both kernels, and no gradient is lost
  xs, dys = R.pool_special_planes(shape)
  a, b = per_pixel_twin(xs, dys)
  assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
  gs = pool(xs, dys)
  assert R.bits_equal(canon(gs), canon(R.pool_ref(xs, dys)))
  assert float(gs.astype(np.float64).sum()) == float(dys.astype(np.float64).sum())
  print(f'[encoder vjp] maxpool bwd {shape} {path}: ties, NaN, -inf and constant planes bit for bit')
