"""The camera-ray lift on planted geometric edges (tests/lift_reference.py), through every entry
point that reaches csrc/lift_common.h: exact where the planted f32 geometry is exact, float64 with
first-order f32 tolerances elsewhere, decisions differing only where the border rule explains it.

The comparison functions (``assert_*``) take numpy arrays only: tests/test_lift_reference.py runs
mutants of the restatement through them.  See tests/README.md, "Lift: planted edges".
"""
import numpy as np
import pytest
import torch

import lift_reference as L

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FD = L.FD
OPTIONS = [(wt, var, mm) for wt in (True, False) for var in (True, False) for mm in (False, True)]
SHARES = {}          # observed worst share of the tolerance per output family (printed; README records them)


def _share(name, err, tol):
  m = tol > 0
  if m.any():
    s = float((err[m] / tol[m]).max())
    SHARES[name] = max(SHARES.get(name, 0.0), s)
    print(f'[lift-edges] {name}: worst share of the tolerance {s:.3f}')


# ------------------------------- comparison functions (numpy) ---------------------------------
def assert_projection(sc, ref64, ref32, p2d, vis, depth):
  """ops.project_points.  Planted: visibility bytes equal, coordinates and depth the mirror's bits.  Float:
  visibility flips only where the border rule allows; coordinates of agreed-visible pairs within tolerance.
  Returns the number of explained flips."""
  name = sc['name']
  vis = np.asarray(vis, bool)
  if sc['exact']:
    bad = np.argwhere(vis != ref64['vis'])
    assert len(bad) == 0, f'{name}: visibility differs at (b, n, v) = {bad[:6].tolist()}'
    want = np.stack([ref32['pi'], ref32['pj']], -1)
    assert np.array_equal(p2d, want), f'{name}: projected coordinates differ from the exact f32 values'
    assert np.array_equal(depth, ref32['depth']), f'{name}: depth differs from the exact f32 values'
    return 0
  rule = L.border_rule(ref64, sc['K'], sc['max_view_distance'])
  flip = vis != ref64['vis']
  bad = np.argwhere(flip & ~rule['vis'])
  assert len(bad) == 0, f'{name}: {len(bad)} visibility flips the border rule does not explain, first {bad[:4].tolist()}'
  both = vis & ref64['vis']
  want = np.stack([ref64['pi'], ref64['pj']], -1)
  tol = L.MARGIN * (32 if sc['fisheye'] else 16) * L.U * np.maximum(np.abs(want), 1.0)
  err = np.abs(p2d - want)
  _share('project_points', err[both], tol[both])
  assert (err[both] <= tol[both]).all(), f'{name}: coordinates beyond tolerance, worst {float((err[both] / tol[both]).max()):.2f}'
  return int(flip.sum())


def assert_rows(sc, ref64, ref32, rows, valid, family='lift_pool'):
  """Pooled rows and validity of one lift_pool-like call against the restatement run with the same options.
  Planted scenes: validity equal; statistics free of exp / log the mirror's bits; everything within the
  float64 tolerance; rows of unseen voxels zero.  Float scenes: a voxel may differ only where the border
  rule explains it.  Returns the number of explained flips."""
  name = f'{sc["name"]} {family}'
  valid = np.asarray(valid, bool)
  want, tol = ref64['rows'], ref64['tol_rows']
  with np.errstate(invalid='ignore'):
    err = np.abs(rows.astype(np.float64) - want)
    bad_el = ~(err <= tol)
  if sc['exact']:
    bad = np.argwhere(valid != ref64['valid'])
    assert len(bad) == 0, f'{name}: validity differs at (b, n) = {bad[:6].tolist()}'
    smc = ref64['smax_channel']
    ex = ref64['stats_exact']
    nst = rows.shape[-1] if smc is None else smc
    if not np.array_equal(rows[ex][:, :nst], ref32['rows'][ex][:, :nst]):
      d = np.argwhere(rows[..., :nst] != ref32['rows'][..., :nst])
      d = [tuple(int(q) for q in i) for i in d if ex[i[0], i[1]]]
      b, n, c = d[0]
      raise AssertionError(f'{name}: {len(d)} statistics differ from the exact f32 values, first at voxel ({b}, {n}) '
                           f'channel {c}: got {rows[b, n, c]!r} want {ref32["rows"][b, n, c]!r}')
    if smc is not None:
      sx = ref64['smax_exact']
      assert np.array_equal(rows[sx][:, smc], ref32['rows'][sx][:, smc]), f'{name}: score_max differs from the exact f32 values'
    assert not bad_el.any(), (f'{name}: {int(bad_el.sum())} elements beyond the float64 tolerance, first '
                              f'{np.argwhere(bad_el)[0].tolist()}: got {rows[tuple(np.argwhere(bad_el)[0])]!r} '
                              f'want {want[tuple(np.argwhere(bad_el)[0])]!r}')
    _share(family, err, tol)
    return 0
  rule = L.border_rule(ref64, sc['K'], sc['max_view_distance'])
  vflip = valid != ref64['valid']
  bad = np.argwhere(vflip & ~rule['valid'])
  assert len(bad) == 0, f'{name}: {len(bad)} validity flips the border rule does not explain, first {bad[:4].tolist()}'
  rflip = bad_el.any(-1)
  bad = np.argwhere(rflip & ~rule['order'])
  assert len(bad) == 0, (f'{name}: {len(bad)} rows beyond tolerance that the border rule does not explain, first voxel '
                         f'{bad[:1].tolist()}, worst share {float(np.nanmax(err[rflip & ~rule["order"]] / np.maximum(tol[rflip & ~rule["order"]], 1e-300))):.2f}')
  keep = ~rflip
  _share(family + ' (float)', err[keep], tol[keep])
  return int((vflip | rflip).sum())


def assert_flips_under_cap(sc, flips):
  pairs = sc['pts'].shape[0] * sc['pts'].shape[1] * sc['cam'].shape[1]
  assert flips <= L.CAP_SHARE * pairs, f'{sc["name"]}: {flips} explained flips exceed {L.CAP_SHARE:.0%} of {pairs} pairs'


def assert_observations(sc, ref64, ref32, obs, feat, valid):
  """ops.lift_observations: slot r of a voxel holds its r-th selected view's blend (zero where that view does
  not see it) | log10 depth | unit ray.  Planted: the feature part is the mirror's bits -- with the pixel
  one-hot input that IS the selected view, its tap pixels and weights."""
  name = sc['name'] + ' lift_observations'
  assert np.array_equal(obs[..., :FD], feat), f'{name}: obs and obs_feat carry different features'
  err = np.abs(obs.astype(np.float64) - ref64['obs'])
  if sc['exact']:
    assert np.array_equal(np.asarray(valid, bool), ref64['valid']), f'{name}: validity differs'
    if not np.array_equal(feat, ref32['feat']):
      b, n, r, c = (int(q) for q in np.argwhere(feat != ref32['feat'])[0])
      raise AssertionError(f'{name}: slot {r} of voxel ({b}, {n}) channel {c}: got {feat[b, n, r, c]!r} want '
                           f'{ref32["feat"][b, n, r, c]!r} (selected view {int(ref64["sel"][b, n, r])})')
    assert (err <= ref64['tol_obs']).all(), f'{name}: depth / ray beyond tolerance'
    _share('lift_observations', err, ref64['tol_obs'])
    return 0
  rule = L.border_rule(ref64, sc['K'], sc['max_view_distance'])
  vflip = np.asarray(valid, bool) != ref64['valid']
  unexplained = np.argwhere(vflip & ~rule['valid'])
  assert len(unexplained) == 0, f'{name}: validity flips the border rule does not explain at voxels {unexplained[:4].tolist()}'
  bad = (~(err <= ref64['tol_obs'])).any((-1, -2))
  unexplained = np.argwhere(bad & ~(rule['order'] | rule['order_inner']))
  assert len(unexplained) == 0, f'{name}: observations beyond tolerance at voxels {unexplained[:4].tolist()}'
  return int((bad | vflip).sum())


def assert_records(sc, ref64, ref32, recs, classes):
  """Tap records of the class-1 voxels (one visible observation): byte offset of tap (i0, j0) | view, clamp
  flags, bins | wi1 | wj1 | score."""
  name = sc['name'] + ' tap records'
  want_cls = np.where(ref64['valid'], np.where(ref64['nok'] > 1, 2, 1), 0)
  assert np.array_equal(classes, want_cls), f'{name}: row classes differ'
  one = ref64['nok'] == 1
  slot = ref64['ok'].argmax(-1)
  pick = lambda a: np.take_along_axis(a, slot[..., None], -1)[..., 0][one]
  tp, bn = ref32['taps'], ref32['bins']
  B, V = sc['cam'].shape[:2]
  C = FD + sc['nb']
  b = np.broadcast_to(np.arange(B)[:, None], one.shape)[one]
  v = pick(ref64['sel'])
  r = recs[one]
  off = (((b * V + v) * L.H + pick(tp['i0'])) * L.W + pick(tp['j0'])) * C * 4
  assert np.array_equal(r[:, 0].astype(np.int64), off), f'{name}: tap offsets differ'
  pk = r[:, 1].astype(np.int64)
  assert np.array_equal(pk & 0xff, v), f'{name}: views differ'
  assert np.array_equal((pk >> 8) & 1, (pick(tp['i1']) != pick(tp['i0'])).astype(np.int64)), f'{name}: row clamp flags differ'
  assert np.array_equal((pk >> 9) & 1, (pick(tp['j1']) != pick(tp['j0'])).astype(np.int64)), f'{name}: column clamp flags differ'
  assert np.array_equal(r[:, 2].view(np.float32), pick(tp['wi1'])) and np.array_equal(r[:, 3].view(np.float32), pick(tp['wj1'])), \
      f'{name}: tap weights differ'
  sx = pick(ref64['score_exact'])
  bx = pick(ref64['bins_exact'])
  assert np.array_equal(((pk >> 10) & 0xff)[bx], pick(bn['b0'])[bx]) and np.array_equal(((pk >> 18) & 0xff)[bx], pick(bn['b1'])[bx]), \
      f'{name}: depth bins differ'
  sc_got = np.ascontiguousarray(r[:, 4]).view(np.float32)
  assert np.array_equal(sc_got[sx], pick(ref32['score'])[sx]), f'{name}: exact scores differ'
  tol = ref64['tol_rows'][..., ref64['smax_channel']][one]
  assert (np.abs(sc_got - pick(ref64['score'])) <= tol).all(), f'{name}: scores beyond tolerance'


# ------------------------------- running the library ------------------------------------------
def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _kw(sc, weighted=True, **more):
  return dict(K=sc['K'], fisheye=sc['fisheye'], feature_dim=FD, num_bins=sc['nb'], depth_min_max=sc['depth_min_max'],
              max_view_distance=sc['max_view_distance'], weighted=weighted, **more)


def _args(sc, f):
  return [_dev(f), _dev(sc['cam']), _dev(sc['Rt']), _dev(sc['pts'])]


def _lift_pool(sc, f, weighted=True, use_variance=True, add_minmax=False):
  from snap_amd import ops
  p, v = ops.lift_pool(*_args(sc, f), **_kw(sc, weighted, use_variance=use_variance, add_minmax=add_minmax))
  return p.cpu().numpy(), v.cpu().numpy()


def _kernel_of(sc, weighted, use_variance, add_minmax):
  """Which forward kernel lift_pool_launch picks (csrc/lift.hip): knowable from the options alone."""
  nsel = sc['K'] or sc['cam'].shape[1]
  if weighted and use_variance and not add_minmax:
    return 'batched' if nsel <= 4 else 'half_wave'
  return 'half_wave_generic'


_SCENES = {s['name']: s for s in L.planted_scenes()}
_FLOAT = {}
for _s in ('depth', 'pixels', 'taps_point_clip', 'bins_nb4_min1', 'select_K2', 'tie_displaced', 'maxdist_K1_eq', 'batch_N33'):
  for _k in (0.0, 0.08):
    _f = L.fisheye_version(_SCENES[_s], _k)
    _FLOAT[_f['name']] = _f
_RANDOM = {s['name']: s for s in L.random_scenes()}
_REFS = {}


def _ref(sc, kind, opts=(True, True, False), dtype=np.float64):
  """One restatement run per (scene, readout, options, dtype), shared by the tests and never modified."""
  key = (sc['name'], kind, opts, np.dtype(dtype).name)
  if key not in _REFS:
    f = L.features(sc, kind, weighted=opts[0])
    _REFS[key] = (f, L.reference(sc, f, dtype, weighted=opts[0], use_variance=opts[1], add_minmax=opts[2]))
  return _REFS[key]


def test_kernel_choice_covers_every_forward_kernel():
  seen = {_kernel_of(sc, *o) for sc in _SCENES.values() for o in OPTIONS}
  assert seen == {'batched', 'half_wave', 'half_wave_generic'}
  assert _kernel_of(_SCENES['select_max'], True, True, False) == 'half_wave'


@pytest.mark.parametrize('name', list(_SCENES) + list(_FLOAT) + list(_RANDOM))
def test_project_points(name):
  from snap_amd import ops
  sc = {**_SCENES, **_FLOAT, **_RANDOM}[name]
  _, r64 = _ref(sc, 'pixel')
  _, r32 = _ref(sc, 'pixel', dtype=np.float32)
  a = _args(sc, np.zeros(1, np.float32))
  p2d, vis, depth = (t.cpu().numpy() for t in ops.project_points(a[1], a[2], a[3], sc['fisheye']))
  flips = assert_projection(sc, r64, r32, p2d, vis, depth)
  if name in _RANDOM:
    assert_flips_under_cap(sc, flips)


@pytest.mark.parametrize('name', list(_SCENES))
def test_lift_pool_is_exact_on_planted_scenes(name):
  """Every option combination (batched, half-wave and generic pooling) on the readouts whose statistics are
  free of exp and log; the half-wave and batched kernels give the same bits."""
  sc = _SCENES[name]
  for kind in ('pixel', 'bins', 'equal'):
    got = {}
    for opts in OPTIONS:
      f, r64 = _ref(sc, kind, opts)
      _, r32 = _ref(sc, kind, opts, np.float32)
      rows, valid = _lift_pool(sc, f, *opts)
      assert rows.shape[-1] == r64['rows'].shape[-1]
      assert_rows(sc, r64, r32, rows, valid, f'lift_pool[{_kernel_of(sc, *opts)}] {kind}')
      got[opts] = rows
    assert np.array_equal(got[(True, True, False)][..., :2 * FD], got[(True, True, True)][..., :2 * FD])


@pytest.mark.parametrize('name', list(_SCENES) + list(_FLOAT) + list(_RANDOM))
def test_lift_pool_against_float64(name):
  """Offset features (two-pass variance) and wide scores (the softmax shift) everywhere, and the pixel readout
  on the scenes that are not exact, at the first-order f32 bound times 8."""
  sc = {**_SCENES, **_FLOAT, **_RANDOM}[name]
  flips = 0
  for kind in ('wide', 'offset') + (() if sc['exact'] else ('pixel',)):
    for opts in ((True, True, False), (True, True, True), (False, True, True), (True, False, False)):
      f, r64 = _ref(sc, kind, opts)
      _, r32 = _ref(sc, kind, opts, np.float32)
      rows, valid = _lift_pool(sc, f, *opts)
      flips = max(flips, assert_rows(sc, r64, r32, rows, valid, f'lift_pool[{_kernel_of(sc, *opts)}] {kind}'))
  if name in _RANDOM:
    assert_flips_under_cap(sc, flips)


@pytest.mark.parametrize('name', list(_SCENES) + list(_FLOAT) + list(_RANDOM))
def test_observations_and_their_pooling(name):
  from snap_amd import ops
  sc = {**_SCENES, **_FLOAT, **_RANDOM}[name]
  for kind in ('pixel', 'offset'):
    opts = (False, True, True)
    f, r64 = _ref(sc, kind, opts)
    _, r32 = _ref(sc, kind, opts, np.float32)
    a = _args(sc, f)
    kw = dict(K=sc['K'], fisheye=sc['fisheye'], feature_dim=FD, max_view_distance=sc['max_view_distance'])
    obs, feat, valid = ops.lift_observations(*a, **kw)
    oflips = assert_observations(sc, r64, r32, obs.cpu().numpy(), feat.cpu().numpy(), valid.cpu().numpy())
    if name in _RANDOM:
      assert_flips_under_cap(sc, oflips)
    rows, valid2 = ops.lift_pool_observations(feat, f.shape, a[1], a[2], a[3], use_variance=True, add_minmax=True, **kw)
    assert torch.equal(valid, valid2)
    flips = assert_rows(sc, r64, r32, rows.cpu().numpy(), valid2.cpu().numpy(), f'lift_pool_observations {kind}')
    if name in _RANDOM:
      assert_flips_under_cap(sc, flips)


def _split_to_f32(p, ks):
  parts = p.view(torch.int32).view(torch.int16).view(torch.bfloat16).reshape(*p.shape[:2], ks, 2, 16)
  return parts


@pytest.mark.parametrize('name', [n for n, s in _SCENES.items() if (s['K'] or s['cam'].shape[1]) <= 4])
def test_record_path_equals_rows_path(name):
  """class_rows / tap records + the gather inside mlp2_pool_max: the records are the planted taps, rows of
  several-view voxels are the same bits on both paths, and the plane is the same bit for bit."""
  from snap_amd import ops
  sc = _SCENES[name]
  N = sc['pts'].shape[1]
  for kind in ('pixel', 'bins', 'offset'):
    f, r64 = _ref(sc, kind)
    _, r32 = _ref(sc, kind, dtype=np.float32)
    a = _args(sc, f)
    kw = _kw(sc, valid_rows_only=True, out_split=True, class_rows=True)
    p4, v4, c4 = ops.lift_pool(*a, **kw)
    p5, v5, c5, r5 = ops.lift_pool(*a, tap_records=True, **kw)
    assert torch.equal(c5, c4) and torch.equal(v5, v4)
    many = c4 == 2
    assert torch.equal(p5[many], p4[many])
    assert np.array_equal(v4.cpu().numpy(), r64['valid'])
    assert_records(sc, r64, r32, r5.cpu().numpy(), c5.cpu().numpy())
    # the split rows are hi + lo of the plain rows
    ks = (2 * FD + 1 + 15) // 16
    pf, vf = ops.lift_pool(*a, **_kw(sc))
    want = torch.zeros(*pf.shape[:2], ks * 16, device=pf.device)
    want[..., :2 * FD + 1] = pf[..., :2 * FD + 1]
    hi = want.bfloat16()
    lo = (want - hi.float()).bfloat16()
    parts = _split_to_f32(p4, ks)
    seen = (c4 == 2)[..., None].expand_as(want)
    assert torch.equal(parts[..., 0, :].reshape(want.shape)[seen], hi[seen]) and torch.equal(parts[..., 1, :].reshape(want.shape)[seen], lo[seen])
    Z = next((z for z in (7, 3) if N % z == 0), None)
    if Z is None:
      continue
    g = torch.Generator().manual_seed(7)
    cin, Hd = 2 * FD + 1, 64
    w0 = (torch.randn((cin, Hd), generator=g) / cin ** 0.5).to(DEV)
    b0 = (torch.randn(Hd, generator=g) * 0.1).to(DEV)
    w1 = (torch.randn((Hd, FD), generator=g) / Hd ** 0.5).to(DEV)
    b1 = (torch.randn(FD, generator=g) * 0.1).to(DEV)
    nv = FD // 16
    flat = lambda t: t.reshape(-1, t.shape[-1])
    want, vwant = ops.mlp2_pool_max(flat(p4), c4.reshape(-1), w0, b0, w1, b1, cin=cin, Z=Z, x_split=True, zero_slabs=(nv, nv))
    got, vgot = ops.mlp2_pool_max(flat(p5), c5.reshape(-1), w0, b0, w1, b1, cin=cin, Z=Z, x_split=True, zero_slabs=(nv, nv),
                                  gather=(a[0], r5))
    assert torch.equal(vgot, vwant) and torch.equal(got, want), float((got - want).abs().max())


@pytest.mark.parametrize('name', list(_SCENES))
def test_nonfinite_pixels_no_tap_touches_are_contained(name):
  from snap_amd import ops
  sc = _SCENES[name]
  for opts in ((True, True, False), (True, True, True), (False, False, True)):
    f, r64 = _ref(sc, 'offset', opts)
    g, planted = L.plant_nonfinite(f, r64)
    assert planted > 0 or name.startswith('taps')
    r0, v0 = _lift_pool(sc, f, *opts)
    r1, v1 = _lift_pool(sc, g, *opts)
    assert np.array_equal(v0, v1) and np.array_equal(r0.view(np.int32), r1.view(np.int32)), \
        f'{name} {opts}: {planted} non-finite pixels outside every tap reached the output'
  if (sc['K'] or sc['cam'].shape[1]) <= L.library_limits()[1]:
    f, r64 = _ref(sc, 'offset', (False, True, True))
    g, _ = L.plant_nonfinite(f, r64)
    kw = dict(K=sc['K'], fisheye=False, feature_dim=FD, max_view_distance=sc['max_view_distance'])
    o0 = ops.lift_observations(*_args(sc, f), **kw)
    o1 = ops.lift_observations(*_args(sc, g), **kw)
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(o0, o1))


def _bwd_forms(sc, f, dp, weighted=True):
  from snap_amd import ops_bwd
  a = _args(sc, f)
  kw = _kw(sc, weighted)
  out = {'deterministic': ops_bwd.lift_pool_bwd(*a, _dev(dp), **kw).cpu().numpy()}
  if weighted:
    prev, ops_bwd.DETERMINISTIC_LIFT_BWD = ops_bwd.DETERMINISTIC_LIFT_BWD, False
    try:
      out['atomic'] = ops_bwd.lift_pool_bwd(*a, _dev(dp), **kw).cpu().numpy()
    finally:
      ops_bwd.DETERMINISTIC_LIFT_BWD = prev
  return out


@pytest.mark.parametrize('name', list(_SCENES))
def test_backward_agrees_with_forward(name):
  """<dpooled, lift(f)> == <lift_bwd(dpooled), f> with dpooled on the mean channels (the map f -> mean is linear
  at fixed scores): both sides sum the same products, compared at 8 x the first-order bound of that sum.  And a
  one-hot dpooled on one-view voxels returns exactly the forward's tap pixels and weights."""
  from snap_amd import ops_bwd
  sc = _SCENES[name]
  f, r64 = _ref(sc, 'equal')
  rows, _ = _lift_pool(sc, f)
  rng = np.random.default_rng(3)
  dp = np.zeros(rows.shape, np.float32)
  dp[..., :FD] = (np.round(rng.uniform(-1, 1, dp[..., :FD].shape) * 64) / 64).astype(np.float32)
  fabs = f.copy()
  fabs[..., :FD] = np.abs(f[..., :FD])
  bound = float((np.abs(dp[..., :FD]).astype(np.float64) * L.reference(sc, fabs)['rows'][..., :FD]).sum())
  tol = L.MARGIN * 32 * L.U * bound
  lhs = float((dp.astype(np.float64) * rows.astype(np.float64)).sum())
  for form, df in _bwd_forms(sc, f, dp).items():
    rhs = float((df[..., :FD].astype(np.float64) * f[..., :FD].astype(np.float64)).sum())
    assert abs(lhs - rhs) <= tol, f'{name} {form}: <dp, lift f> = {lhs!r}, <lift_bwd dp, f> = {rhs!r}, tolerance {tol:.3e}'
    if bound:
      _share('adjoint identity ' + form, np.array([abs(lhs - rhs)]), np.array([tol]))
  # observations: obs_feat is linear in f
  fo = np.ascontiguousarray(f[..., :FD])
  a = _args(sc, fo)
  kw = dict(K=sc['K'], fisheye=False, feature_dim=FD, max_view_distance=sc['max_view_distance'])
  from snap_amd import ops
  feat = ops.lift_observations(*a, **kw)[1].cpu().numpy()
  do = (np.round(rng.uniform(-1, 1, feat.shape) * 64) / 64).astype(np.float32)
  dfo = ops_bwd.lift_observations_bwd(_dev(do), fo.shape, a[1], a[2], a[3], **kw).cpu().numpy()
  r_abs = L.reference(sc, np.abs(fo), weighted=False)
  bound = float((np.abs(do).astype(np.float64) * r_abs['feat']).sum())
  lhs = float((do.astype(np.float64) * feat.astype(np.float64)).sum())
  rhs = float((dfo.astype(np.float64) * fo.astype(np.float64)).sum())
  assert abs(lhs - rhs) <= L.MARGIN * 32 * L.U * bound, f'{name} observations: {lhs!r} vs {rhs!r}'
  # one-hot dpooled: up to 32 one-view voxels, one mean channel each
  _, r32 = _ref(sc, 'equal', dtype=np.float32)
  one = np.argwhere(r64['nok'] == 1)[:FD]
  if len(one) == 0:
    return
  # The softmax weight of a one-view voxel is exactly 1 and dpooled is 1: the gradient at a tap pixel is the f32
  # mirror's w00 .. w11, bit for bit.  Taps that the clamp puts on ONE pixel add up there: two of them in either
  # order give the same f32 sum (exact comparison); three or four (a clamped corner) add in an order the atomic
  # form does not fix -- that named class alone is held to one relative ulp, the taps added in tap order.
  dp = np.zeros(rows.shape, np.float32)
  want = np.zeros(f.shape[:4] + (FD,), np.float32)
  count = np.zeros(want.shape, np.int64)
  tp = r32['taps']
  for c, (b, n) in enumerate(one):
    dp[b, n, c] = 1.0
    s = int(r64['ok'][b, n].argmax())
    v = int(r64['sel'][b, n, s])
    for i, j, wk in (('i0', 'j0', 'w00'), ('i0', 'j1', 'w01'), ('i1', 'j0', 'w10'), ('i1', 'j1', 'w11')):
      at = (b, v, tp[i][b, n, s], tp[j][b, n, s], c)
      want[at] = np.float32(want[at] + tp[wk][b, n, s])
      count[at] += 1
  corner = count >= 3
  for form, df in _bwd_forms(sc, f, dp).items():
    got = df[..., :FD]
    assert np.array_equal(got != 0, want != 0), f'{name} {form}: the gradient touches other pixels than the forward taps'
    bad = np.argwhere((got != want) & ~corner)
    assert len(bad) == 0, (f'{name} {form}: {len(bad)} gradient values are not the bits of the forward tap weights, first at '
                           f'{bad[0].tolist()}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}')
    assert (np.abs(got.astype(np.float64) - want)[corner] <= L.ulp32(want[corner])).all(), \
        f'{name} {form}: a clamped-corner gradient is more than one ulp from the sum of its taps'


@pytest.mark.parametrize('name', ['batch_N257', 'select_max', 'taps_point_clip'])
def test_two_runs_give_identical_bytes(name):
  from snap_amd import ops
  sc = _SCENES[name]
  f, _ = _ref(sc, 'offset')
  a = _args(sc, f)

  def run():
    out = list(ops.project_points(a[1], a[2], a[3], False))
    for opts in OPTIONS:
      fo = a[0] if opts[0] else a[0][..., :FD].contiguous()
      out += list(ops.lift_pool(fo, *a[1:], **_kw(sc, opts[0], use_variance=opts[1], add_minmax=opts[2])))
    if (sc['K'] or sc['cam'].shape[1]) <= 4:      # (rows and records of the other classes are not written)
      _, v, c, r = ops.lift_pool(*a, tap_records=True, **_kw(sc, valid_rows_only=True, out_split=True, class_rows=True))
      out += [v, c, r[c == 1][:, :5]]
    if (sc['K'] or sc['cam'].shape[1]) <= L.library_limits()[1]:
      kw = dict(K=sc['K'], fisheye=False, feature_dim=FD, max_view_distance=sc['max_view_distance'])
      fo = a[0][..., :FD].contiguous()
      o = ops.lift_observations(fo, *a[1:], **kw)
      out += list(o) + list(ops.lift_pool_observations(o[1], fo.shape, *a[1:], **kw))
    return [t.cpu() for t in out]

  for x, y in zip(run(), run()):
    same = torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)
    assert same, f'{name}: two runs differ'
