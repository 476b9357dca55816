"""CPU: ``vote_credible_reference`` against the definition's own words on tiny lattices, the structure of its regions,
the gap condition that lets the GPU test demand equal thresholds, and the calibration statistic on sampled ground
truths (``pose_exhaustive_voting.coverage_table``)."""
import numpy as np
import pytest

import vote_credible_reference as ref
from snap_amd.models import pose_exhaustive_voting as pev


def _by_definition(v, levels, scale):
  """For every distinct value t of F: mass{v >= t}; tau = the largest t with mass >= q Z.  Plain loops, no sort."""
  F = np.isfinite(v)
  vals = (v[F] + np.float32(0)).astype(np.float64)
  w = np.exp(np.float64(np.float32(scale)) * (vals - vals.max()))
  Z = sum(w)
  out = []
  for q in np.asarray(levels, np.float32).astype(np.float64):
    best = None
    for t in set(vals.tolist()):
      m = sum(w[vals >= t])
      if m >= q * Z and (best is None or t > best[0]):
        best = (t, m / Z)
    out.append(best)
  return out


@pytest.mark.parametrize('kind', ['smooth', 'dirty', 'ties', 'equal'])
@pytest.mark.parametrize('shape', [(3, 1, 1), (1, 5, 5), (4, 7, 7), (3, 4, 5)], ids=lambda s: '%dx%dx%d' % s)
def test_reference_equals_the_definition_on_tiny_lattices(kind, shape):
  if kind == 'dirty' and np.prod(shape) < 20:
    shape = (2, 3, 4)                                        # (the planted cells need room)
  v = dict(smooth=ref.smooth_votes, dirty=ref.dirty_votes, ties=ref.tie_votes, equal=ref.equal_votes)[kind](shape)
  for scale in (1.0, 4.0):
    for levels in (ref.LEVELS1, ref.LEVELS3, ref.LEVELS8):
      thr, mass, table, lxy, lr, lc, _, count = ref.vote_credible(v, levels, scale)
      want = _by_definition(v, levels, scale)
      assert [float(t) for t in thr] == [t for t, _ in want]
      assert np.allclose(mass, [m for _, m in want], rtol=1e-13, atol=0)
      F = np.isfinite(v)
      assert count.tolist() == [int(F.sum()), int((np.isnan(v) | (v == np.inf)).sum()), 0, -1]
      for l, t in enumerate(thr):
        with np.errstate(invalid='ignore'):
          region = F & (v >= t)
        assert ((lc <= l) == region).all()
        assert table[l].tolist() == [int(region.sum()), int(region.any(0).sum()), int(region.any((1, 2)).sum()),
                                     np.nonzero(region.any((0, 2)))[0].min(), np.nonzero(region.any((0, 2)))[0].max(),
                                     np.nonzero(region.any((0, 1)))[0].min(), np.nonzero(region.any((0, 1)))[0].max(), 0]
        assert ((lxy <= l) == region.any(0)).all() and ((lr <= l) == region.any((1, 2))).all()


def test_regions_are_nested_and_tie_classes_are_never_split():
  for name, v, scale, levels, _ in ref.all_inputs():
    if v.size > 40000 or not np.isfinite(v).any():
      continue
    thr, mass, table, _, _, lc, _, _ = ref.vote_credible(v, levels, scale)
    assert (np.diff(thr) <= 0).all() and (np.diff(mass) >= 0).all() and (np.diff(table[:, 0]) >= 0).all(), name
    q = np.asarray(levels, np.float32).astype(np.float64)
    assert (mass >= q * (1 - 1e-15)).all(), name
    F = np.isfinite(v)
    for value in np.unique(v[F]):
      assert len(np.unique(lc[F & (v == value)])) == 1, (name, value)      # (-0 == +0: one class)
  v = ref.tie_votes((36, 31, 33))
  thr, mass, table, *_ = ref.vote_credible(v, ref.tie_levels(v, 1.0, 3), 1.0)
  assert thr[0] == thr[1] and mass[0] == mass[1] and table[0].tolist() == table[1].tolist()   # two levels, one class
  assert len({float(t) for t in thr}) == 2


def test_minus_zero_and_plus_zero_are_one_class():
  v = np.array([[[0.0, -0.0, -1.0, 0.5]]], np.float32)
  thr, mass, table, _, _, lc, _, _ = ref.vote_credible(v, (0.3, 0.5, 0.9), 1.0)
  w = np.exp([0.0, -0.5, -0.5, -1.5])                       # 0.5, the two zeros, -1
  assert thr.tolist() == [0.5, 0.0, 0.0] and table[:, 0].tolist() == [1, 3, 3]
  assert np.allclose(mass, [w[0] / w.sum(), w[:3].sum() / w.sum(), w[:3].sum() / w.sum()], rtol=1e-14)
  assert lc.reshape(-1).tolist() == [1, 1, 3, 0]


def test_gap_condition_holds_for_every_listed_case():
  """gap >= max(4 bound, 1e-9): the threshold is decided beyond the kernel's fixed-point arithmetic, so the GPU test
  demands equality.  (A case that does not meet it is replaced, not loosened.)"""
  worst = None
  for name, v, scale, levels, _ in ref.all_inputs():
    g, b = ref.gap(v, scale, levels), ref.bound(v, scale)
    assert g >= max(4 * b, 1e-9), f'{name}: gap {g:.3e} against bound {b:.3e}'
    if np.isfinite(g) and (worst is None or g / max(4 * b, 1e-9) < worst[1]):
      worst = (name, g / max(4 * b, 1e-9), g, b)
  print('tightest case: %s, gap / need = %.3g (gap %.3e, bound %.3e)' % worst)


def test_bound_is_the_documented_quantum():
  v = ref.smooth_votes((36, 31, 33))
  F = np.isfinite(v)
  Z = np.exp(4.0 * (v[F].astype(np.float64) - v[F].max())).sum()
  assert v.size == 36828 and abs(ref.bound(v, 4.0) - (36828 * 2.0 ** -(62 - 16) / Z + 2.0 ** -40)) < 1e-20
  assert ref.bound(np.full((3, 1, 1), -np.inf, np.float32)) == 0


def test_ground_truth_cases():
  v, levels, scale, cases = ref.gt_cases()
  cred = ref.credibility_of_cells(v, scale)
  thr = ref.vote_credible(v, levels, scale)[0]
  names = {n for n, _, _ in cases}
  assert {'centre', 'between', 'outside', 'half_even_down', 'half_even_up', 'wrap_neg', 'wrap_top', 'masked', 'nan'} <= names
  for name, idx, cell in cases:
    st, cnt = ref.vote_credible(v, levels, scale, idx)[6:]
    valid = cell is not None and bool(np.isfinite(v[cell]))
    assert cnt[2] == int(valid), name
    if not valid:
      assert np.isnan(st[:3]).all() and st[3] == 0 and cnt[3] == -1, name
      continue
    assert st[0] == v[cell] and abs(st[1] - cred[cell]) < 1e-13 and st[2] > st[1], name
    assert cnt[3] == int((v[cell] < thr).sum()), name
    # the ground truth lies in region l exactly when its credibility is below q_l
    assert [bool(cnt[3] <= l) for l in range(3)] == [bool(st[1] < np.float64(np.float32(q))) for q in levels], name
  by = {n: c for n, _, c in cases}
  lev = ref.vote_credible(v, levels, scale)[5]
  assert lev[by['centre']] == 0 and lev[by['between']] in (1, 2) and lev[by['outside']] == 3


def _two_modes(shape=(8, 21, 21)):
  rng = np.random.default_rng(5)
  r = np.arange(shape[0])[:, None, None]
  a, b = np.arange(shape[1])[None, :, None], np.arange(shape[2])[None, None, :]
  dr = lambda c: np.minimum(np.abs(r - c), shape[0] - np.abs(r - c))
  x = np.maximum(-((a - 6) ** 2 + (b - 7) ** 2) / 18 - dr(1) ** 2 / 2,
                 -0.4 - ((a - 14) ** 2 + (b - 13) ** 2) / 18 - dr(5) ** 2 / 2)
  return (x + 0.01 * rng.standard_normal(shape)).astype(np.float32)


def test_calibration_of_sampled_ground_truths():
  """Ground truths drawn from softmax(v): their credibilities under v cover every level within 4 binomial standard
  deviations; under the over-confident 3 v the coverage at 0.9 falls out of that band."""
  v = _two_modes()
  n = 4000
  p = np.exp(v.astype(np.float64) - v.max())
  p /= p.sum()
  cells = np.random.default_rng(11).choice(v.size, size=n, p=p.reshape(-1))
  levels = np.array(ref.LEVELS3)
  band = 4 * np.sqrt(levels * (1 - levels) / n)
  good = pev.coverage_table(ref.credibility_of_cells(v, 1.0).reshape(-1)[cells], levels)
  print('calibrated:', good)
  assert good['count'] == n and (np.abs(good['coverage'] - levels) <= band).all()
  assert abs(good['mean_abs_error'] - np.abs(good['coverage'] - levels).mean()) < 1e-15
  over = pev.coverage_table(ref.credibility_of_cells(v, 3.0).reshape(-1)[cells], levels)
  print('over-confident:', over)
  assert over['coverage'][1] < levels[1] - band[1]
  # the valid mask and NaN credibilities drop frames
  c = ref.credibility_of_cells(v, 1.0).reshape(-1)[cells].copy()
  c[:10] = np.nan
  keep = np.ones(n, bool)
  keep[10:30] = False
  part = pev.coverage_table(c, levels, valid=keep)
  assert part['count'] == n - 30
  assert part['coverage'][0] == float((c[30:] < 0.5).mean())
  assert np.isnan(pev.coverage_table([np.nan], levels)['coverage']).all()
