"""The float64 restatement of the lift (tests/lift_reference.py) alone: it agrees with the numpy oracle,
its planted scenes are what their names say and are exact in f32, the escape caps hold, and the
comparison functions of tests/test_gpu_lift_edges.py reject mutants of it.  No GPU."""
import numpy as np
import pytest

import lift_reference as L
import oracle_ops
import test_gpu_lift_edges as G

SCENES = {s['name']: s for s in L.planted_scenes()}
f32 = np.float32


@pytest.mark.parametrize('K,V', [(0, 1), (0, 3), (2, 3), (4, 6), (4, 20), (8, 9)])
def test_restatement_agrees_with_the_oracle(K, V):
  """The random scenes of test_lift_pool, every option combination: validity equal except for flips the border
  rule explains, values at the oracle's f32 level."""
  import torch
  from test_gpu_kernels import _lift_scene
  fd, nb = 32, 8
  f, cam, Rt, pts = _lift_scene(2, V, 12, 16, fd, nb, 4000, seed=30 + V)
  pts = pts[:, :600].contiguous()
  for weighted, use_var, minmax in G.OPTIONS:
    fo = f if weighted else f[..., :fd].contiguous()
    kw = dict(K=K, fisheye=True, feature_dim=fd, num_bins=nb, depth_min_max=(1.0, 16.0), weighted=weighted,
              use_variance=use_var, add_minmax=minmax, max_view_distance=5.0 if K else None)
    pw, vw = oracle_ops.lift_pool(fo, cam, Rt, pts, **kw)
    ref = L.lift(fo.numpy(), cam.numpy(), Rt.numpy(), pts.numpy(), K=K, fisheye=True, fd=fd, nb=nb, depth_min_max=(1.0, 16.0),
                 max_view_distance=kw['max_view_distance'], weighted=weighted, use_variance=use_var, add_minmax=minmax)
    rule = L.border_rule(ref, K, kw['max_view_distance'])
    flip = ref['valid'] != vw.numpy()
    assert not (flip & ~rule['valid']).any(), 'a validity flip the border rule does not explain'
    assert flip.mean() < 0.01 and ref['valid'].mean() > 0.05
    keep = ~(flip | rule['order'])
    err = np.abs(ref['rows'] - pw.numpy().astype(np.float64))
    assert (err[keep] <= 2e-4 + 1e-4 * np.abs(ref['rows'][keep])).all(), float(err[keep].max())
  pr = oracle_ops.project_points(cam, Rt, pts, True)
  ref = L.project(cam.numpy(), Rt.numpy(), pts.numpy(), True)
  rule_vis = L.border_rule(L.lift(f.numpy(), cam.numpy(), Rt.numpy(), pts.numpy(), K=K, fisheye=True, fd=fd, nb=nb), K)['vis']
  assert not ((ref['vis'] != pr[1].numpy()) & ~rule_vis).any()
  both = ref['vis'] & pr[1].numpy()
  assert np.abs(np.stack([ref['pi'], ref['pj']], -1) - pr[0].numpy())[both].max() < 1e-4
  assert np.abs(ref['depth'] - pr[2].numpy()).max() < 1e-5
  # the selection and the observation layout (features | log10 depth | unit ray) against oracle/lift.py itself
  from oracle import lift as o_lift
  T, cams, p = oracle_ops.unpack_transforms(Rt), oracle_ops.unpack_cameras(cam, True), pts.numpy()
  p2d, vis, depth, rays = o_lift.project_points_to_views(T, cams, p)
  fo = f[..., :fd].numpy()
  ref = L.lift(fo, cam.numpy(), Rt.numpy(), p, K=K, fisheye=True, fd=fd, nb=0, weighted=False)
  rule = L.border_rule(ref, K)
  sure = ~(rule['order'] | rule['order_inner']) & (vis == ref['vis']).all(-1)
  assert sure.mean() > 0.95
  if K:
    idx, md = o_lift.view_selection(p, T, vis, K)
    assert np.array_equal(idx[sure], ref['sel'][sure])
    fin = sure & np.isfinite(md)
    assert np.array_equal(np.isfinite(md)[sure], np.isfinite(ref['min_dist'])[sure]) and np.abs(md - ref['min_dist'])[fin].max() < 1e-5
    p2d, vis, depth, rays = (o_lift.gather_batched_observations(a, idx) for a in (p2d, vis, depth, rays))
    feats = o_lift.interpolate_views_selective(fo, p2d, idx)
  else:
    feats = o_lift.interpolate_views_all(fo, p2d)
  want = np.concatenate([np.where(vis[..., None], feats, 0), np.log10(np.clip(depth, 0.1, 100))[..., None],
                         np.where(vis[..., None], rays, 0)], -1)
  assert (np.abs(ref['obs'] - want)[sure] <= 2e-4 + 1e-4 * np.abs(ref['obs'][sure])).all()     # (the oracle's f32 level, as above)


@pytest.mark.parametrize('name', list(SCENES))
def test_planted_geometry_is_exact_in_f32(name):
  """The restatement in np.float32 (the header's expression order) decides everything as float64 does: the
  planted geometry is exact.  Bin pairs may move only at the bin centres (log is not exact), as the rule says."""
  sc = SCENES[name]
  for kind in ('pixel', 'bins', 'equal'):
    for opts in G.OPTIONS:
      f = L.features(sc, kind, weighted=opts[0])
      r64 = L.reference(sc, f, weighted=opts[0], use_variance=opts[1], add_minmax=opts[2])
      r32 = L.reference(sc, f, f32, weighted=opts[0], use_variance=opts[1], add_minmax=opts[2])
      for k in ('vis', 'sel', 'ok', 'valid'):
        assert np.array_equal(r64[k], r32[k]), (name, k)
      assert np.array_equal(r64['depth'].astype(f32), r32['depth']), name
      fin = np.isfinite(r64['min_dist'])          # (a square root: rounded once in either precision)
      assert np.array_equal(fin, np.isfinite(r32['min_dist'])) and (np.abs(r64['min_dist'] - r32['min_dist'])[fin] <= L.ulp32(r64['min_dist'][fin])).all()
      for k in ('pi', 'pj'):      # (behind the near plane the division is by eps: rounded, and never looked at)
        assert np.array_equal(r64[k][r64['vis']].astype(f32), r32[k][r64['vis']]), (name, k)
      ok = r64['ok']
      for k in ('i0', 'i1', 'j0', 'j1'):
        assert np.array_equal(r64['taps'][k][ok], r32['taps'][k][ok]), (name, k)
      for k, c in (('wi1', 'ci'), ('wj1', 'cj')):     # (nextafter(w, 0) - 0.5 is not an f32: that weight is rounded once)
        w64, w32 = r64['taps'][k][ok], r32['taps'][k][ok]
        rounded = r64['taps'][c][ok].astype(f32) != r64['taps'][c][ok]
        assert np.array_equal(w64[~rounded].astype(f32), w32[~rounded]) and rounded.mean() < 0.2, (name, k)
        assert (np.abs(w64 - w32) <= 0.5 * L.ulp32(r64['taps'][c][ok])).all(), (name, k)
      rule = L.border_rule(r64, sc['K'], sc['max_view_distance'])
      moved = ok & ((r64['bins']['b0'] != r32['bins']['b0']) | (r64['bins']['b1'] != r32['bins']['b1']))
      assert not opts[0] or not (moved & (~rule['bin'] | r64['bins_exact'])).any(), name
      # the comparison the GPU file makes accepts the mirror: exact where flagged, within tolerance elsewhere
      G.assert_rows(sc, r64, r32, r32['rows'], r32['valid'])
      G.assert_projection(sc, r64, r32, np.stack([r32['pi'], r32['pj']], -1), r32['vis'], r32['depth'])
      G.assert_observations(sc, r64, r32, r32['obs'], r32['feat'], r32['valid'])
  for kind in ('wide', 'offset'):
    f = L.features(sc, kind)
    G.assert_rows(sc, L.reference(sc, f), L.reference(sc, f, f32), L.reference(sc, f, f32)['rows'], L.reference(sc, f, f32)['valid'])


def _ref(name, **kw):
  sc = SCENES[name]
  return sc, L.reference(sc, L.features(sc, 'bins'), **kw), L.reference(sc, L.features(sc, 'bins'), f32, **kw)


def test_planted_edges_are_what_their_names_say():
  e32 = float(L.EPS32)
  sc, r, r32 = _ref('depth')
  for n, e in sc['edges'].items():
    b, i = e['voxel']
    assert r['depth'][b, i, 0] == e['depth'] and bool(r['vis'][b, i, 0]) == e['visible'], n
  d = sc['edges']
  assert d['depth_eq_eps']['depth'] == e32 and f32(d['depth_below_eps']['depth']) == np.nextafter(L.EPS32, f32(0))
  sc, r, r32 = _ref('pixels')
  for n, e in sc['edges'].items():
    b, i = e['voxel']
    v = e['view']
    assert r['pj'][b, i, v] == e['x'] and r['pi'][b, i, v] == e['y'] and bool(r['vis'][b, i, v]) == e['visible'], n
  assert f32(sc['edges']['x_below_w']['x']) == np.nextafter(f32(L.W), f32(0)) and sc['edges']['x_below_0']['x'] == -2.0 ** -20
  assert f32(sc['edges']['y_below_h']['y']) == np.nextafter(f32(L.H), f32(0))
  for name in ('taps_index_clip', 'taps_point_clip'):
    sc, r, r32 = _ref(name)
    tp = r['taps']
    assert r['vis'][..., 0].all() and (r['nok'] == 1).all()
    pi = np.array([e['pi'] for e in sc['edges'].values()])
    pj = np.array([e['pj'] for e in sc['edges'].values()])
    assert np.array_equal(r['pi'][0, :, 0], pi) and np.array_equal(r['pj'][0, :, 0], pj)
    centre = (pi % 1 == 0.5) & (pi > 0.5)
    assert centre.sum() >= L.H - 1 and (tp['wi1'][0, centre, 0] == 0).all()
    first, last = pi < 0.5, pi > L.H - 0.5
    assert first.any() and last.any()
    if name == 'taps_index_clip':       # both taps clamp onto the border row
      assert (tp['i0'][0, first | last, 0] == tp['i1'][0, first | last, 0]).all()
    else:                               # the point is clipped: the pair stays (0, 1) / ends on the last row with weight 0
      assert (tp['i1'][0, first, 0] == tp['i0'][0, first, 0] + 1).all() and (tp['wi1'][0, first | last, 0] == 0).all()
    assert (tp['i0'][0, first, 0] == 0).all() and (tp['i1'][0, first, 0] == (0 if name == 'taps_index_clip' else 1)).all()
    assert (tp['i1'][0, last, 0] == L.H - 1).all()
    # the two clip rules give other weights on the first half pixel: index clip keeps wi1 = pi + 0.5, point clip gives 0
    assert (tp['wi1'][0, first, 0] == (pi[first] + 0.5 if name == 'taps_index_clip' else 0)).all()
    for k in range(1, L.H):       # both sides of every tap seam
      assert ((pi > k + 0.5 - 0.01) & (pi < k + 0.5)).any() and ((pi > k + 0.5) & (pi < k + 0.5 + 0.01)).any()
  for name, nb in (('bins_nb4_min1', 4), ('bins_nb8_min1', 8), ('bins_nb4_min2', 4)):
    sc, r, r32 = _ref(name)
    for res in (r, r32):
      bn = res['bins']
      for n in ('depth_eq_max', 'depth_above_max'):
        i = sc['edges'][n]['voxel'][1]
        assert bn['b0'][0, i, 0] == bn['b1'][0, i, 0] == nb - 1 and bn['wb1'][0, i, 0] == 0, (name, n)
      for n in ('depth_eq_min', 'depth_below_min'):
        i = sc['edges'][n]['voxel'][1]
        assert bn['b0'][0, i, 0] == 0 and bn['b1'][0, i, 0] == 1 and bn['wb1'][0, i, 0] == 0, (name, n)
    for k in range(1, nb - 1):
      i = sc['edges'][f'bin_centre_{k}']['voxel'][1]
      assert abs(r['bins']['c'][0, i, 0] - k) < 1e-12 and abs(r['rows'][0, i, r['smax_channel']] - (k - 2)) < 1e-12
  for K in (1, 2, 4):
    sc, r, r32 = _ref(f'select_K{K}')
    e = sc['edges']
    b, i = e['tie_at_origin']['voxel']
    d32 = r32['dist'][b, i]
    assert all(d32[v].tobytes() == f32(5).tobytes() and r['vis'][b, i, v] for v in e['tie_at_origin']['equal_views'])
    assert list(r['sel'][b, i]) == [2, 3, 4, 1][:K]
    assert not r['vis'][b, i, 0] and r['dist'][b, i, 0] == r['dist'][b, i].min()
    assert r['nok'][e['none_visible']['voxel']] == 0 and r['vis'][e['exactly_K']['voxel']].sum() == K
    assert r['vis'][e['more_than_K']['voxel']].sum() > K
    if K > 1:
      assert 0 < r['vis'][e['fewer_than_K']['voxel']].sum() < K
  sc, r, r32 = _ref('tie_displaced')
  e = sc['edges']['tie_behind_a_nearer_later_view']
  assert r32['dist'][0, 0, 0].tobytes() == r32['dist'][0, 0, 1].tobytes() and r['dist'][0, 0, 2] < r['dist'][0, 0, 0]
  assert tuple(r['sel'][0, 0]) == e['selected'] and r['vis'][0, 0, :3].all()
  sc, r, r32 = _ref('select_max')
  V, Kmax = L.library_limits()
  assert (V, Kmax) == (32, 8) and sc['cam'].shape[1] == V and sc['K'] == Kmax
  e = sc['edges']['tie_at_Kth_place']
  d32 = r32['dist'][0, 0]
  assert len({d32[v].tobytes() for v in e['equal_views']}) == 1 and d32[e['equal_views'][0]] == 20
  assert r['sel'][0, 0, Kmax - 1] == e['winner'] and not set(e['equal_views'][1:]) & set(r['sel'][0, 0].tolist())
  assert (np.sort(r['dist'][0, 0][r['sel'][0, 0]]) == [5, 5, 5, 10, 10, 10, 10, 20]).all()
  for name, valid in (('maxdist_K1_eq', True), ('maxdist_K1_ulp', False), ('maxdist_K2_ulp', False), ('maxdist_K0_ulp', True)):
    sc, r, r32 = _ref(name)
    assert r32['min_dist'][0, 0].tobytes() == f32(5).tobytes() and bool(r['valid'][0, 0]) == valid == sc['edges']['min_dist_5']['valid']
    if 'ulp' in name:
      assert f32(sc['max_view_distance']) == np.nextafter(f32(5), f32(0))
  for N in (1, 31, 32, 33, 257):
    sc = SCENES[f'batch_N{N}']
    assert sc['pts'].shape == (2, N, 3) and not np.array_equal(sc['cam'][0], sc['cam'][1]) and not np.array_equal(sc['Rt'][0], sc['Rt'][1])


def test_escape_caps_hold_for_the_reference_alone():
  """On each random scene of the GPU file: the decisions inside the border-flip distance number at most a
  quarter of the cap (1 % of the (voxel, view) pairs)."""
  for sc in L.random_scenes():
    r = L.reference(sc, L.features(sc, 'wide'))
    rule = L.border_rule(r, sc['K'], sc['max_view_distance'])
    pairs = r['vis'].size
    n = L.near_count(rule)
    print(f'[lift-edges] {sc["name"]}: {n} of {pairs} decisions inside the border-flip distance (cap {L.CAP_SHARE * pairs:.1f})')
    assert n <= 0.25 * L.CAP_SHARE * pairs
    assert 0.1 < r['vis'].mean() < 0.9 and (r['nok'] > 1).mean() > 0.05


# which planted scenes, readouts and options each mutant is shown
_MUTANT_RUNS = [(n, k, o) for n in SCENES for k in ('pixel', 'bins', 'wide', 'offset')
                for o in ((True, True, False), (True, True, True), (False, True, True))]


def _rejected(mut):
  hits = []
  for name, kind, opts in _MUTANT_RUNS:
    sc = SCENES[name]
    f = L.features(sc, kind, weighted=opts[0])
    kw = dict(weighted=opts[0], use_variance=opts[1], add_minmax=opts[2])
    r64, r32 = L.reference(sc, f, **kw), L.reference(sc, f, f32, **kw)
    m = L.reference(sc, f, f32, mut=(mut,), **kw)
    for check in (lambda: G.assert_rows(sc, r64, r32, m['rows'], m['valid']),
                  lambda: G.assert_projection(sc, r64, r32, np.stack([m['pi'], m['pj']], -1), m['vis'], m['depth']),
                  lambda: G.assert_observations(sc, r64, r32, m['obs'], m['feat'], m['valid'])):
      try:
        check()
      except AssertionError:
        hits.append((name, kind, opts))
        break
  return hits


@pytest.mark.parametrize('mut', [m for m in L.MUTANTS if m != 'softmax_no_floor'])
def test_mutants_are_rejected_by_the_gpu_comparisons(mut):
  hits = _rejected(mut)
  print(f'[lift-edges] mutant {mut}: rejected on {len(hits)} runs, e.g. {hits[:3]}')
  assert hits, f'mutant {mut} passes every planted scene'


@pytest.mark.parametrize('mut,scenes', [('swap_clip', ('taps_index_clip', 'taps_point_clip')),
                                        ('bin_clamp_after_log', ('bins_nb4_min1', 'bins_nb8_min1', 'bins_nb4_min2'))])
def test_clip_and_bin_mutants_are_pinned_by_the_tap_records(mut, scenes):
  """Both mutants give the same BLEND as the header on the planted points (the extra tap / bin has weight 0, or
  the pair collapses onto one bin), so values reject them through rounding at best.  The tap records carry the
  decision itself -- clamp flags and wi1 / wj1, the bin pair: G.assert_records rejects the mutant's records on
  every scene planted for it and accepts the restatement's own."""
  for name in scenes:
    sc = SCENES[name]
    f = L.features(sc, 'bins')
    r64, r32 = L.reference(sc, f), L.reference(sc, f, f32)
    G.assert_records(sc, r64, r32, *L.tap_records(sc, r32))
    with pytest.raises(AssertionError, match='tap weights differ|clamp flags differ|depth bins differ'):
      G.assert_records(sc, r64, r32, *L.tap_records(sc, L.reference(sc, f, f32, mut=(mut,))))


def test_all_negative_score_rows_are_planted():
  """Softmax is shift invariant: max(0, max score) against max score changes rounding only until exp(score)
  underflows (score < -87), so with scores in [-80, 80] no comparison of values can tell the softmax-shift
  mutant from the header.  What the floor must not do is lose all-negative rows: they are planted here and
  compared with float64 like every other row."""
  sc = SCENES['select_K4']
  r = L.reference(sc, L.features(sc, 'wide'))
  allneg = (np.where(r['ok'], r['score'], -1) < 0).all(-1) & (r['nok'] > 1)
  assert allneg.sum() >= 5 and np.where(r['ok'], r['score'], 0).min() < -60
