"""``vote_smooth_reference`` (the float64 restatement the GPU tests compare ``ops.vote_smooth`` with) against an
independent formulation and its own invariants.  No GPU.

The independent formulation is the textbook alpha-beta recursion on a tiny lattice with DENSE n x n transition kernels
built by pushing unit masses through ``vote_filter_reference.predict``: nothing of the smoother's ratio / adjoint /
combine structure is in it.  The two agree to the f32 roundings of the stored quantities (the beliefs, d, p and q are
f32 by contract: a few 2^-24 relative each per frame), not to float64 noise: the tolerance is 64 * 2^-24 *
(1 + max |log gamma|), three orders below the effect of a wrong offset, factor or pass order."""
import numpy as np
import pytest

import vote_filter_reference as flt
import vote_smooth_reference as ref


def _tiny_track(eps):
  votes, taps, scale = ref.tiny_track()
  beliefs, prev = [], None
  for t in range(len(votes)):
    prev = flt.vote_filter(prev, votes[t], taps[t] or ref.still_taps(3), scale, eps)[0].astype(np.float32)
    beliefs.append(prev)
  return votes, taps, beliefs, scale


@pytest.mark.parametrize('eps', [0.0, 1e-3])
def test_definition_against_dense_alpha_beta(eps):
  votes, taps, beliefs, scale = _tiny_track(eps)
  N, n = len(votes), votes[0].size
  gamma = ref.dense_smoothing(votes, taps, scale, eps, beliefs)
  got = ref.smooth_track(beliefs, taps, eps, rounded=False)
  for t in range(N):
    g = gamma[t]
    fin = g > 0                                             # (eps = 0: the shifts leave some cells without mass)
    have = np.asarray(got[t], np.float64).reshape(n)
    assert ((have == -np.inf) == ~fin).all() and fin.sum() > n // 2
    want = np.log(g[fin] / g.sum())
    err = np.abs(have[fin] - want).max()
    tol = 64 * 2.0 ** -24 * (1 + np.abs(want).max())
    print(f'eps {eps} frame {t}: max err {err:.3e} (tol {tol:.3e})')
    assert err <= tol
  # and a wrong pass order or offset is far outside: the forward taps used as they are, not as the adjoint
  wrong = ref.vote_smooth(beliefs[1], beliefs[2], taps[1], eps)[0]
  g = gamma[1]
  both = (g > 0) & np.isfinite(wrong.reshape(n))
  assert np.abs(wrong.reshape(n)[both] - np.log(g[both] / g.sum())).max() > 1e-3


def test_normalised_and_log_norm_zero_for_filter_consistent_inputs():
  votes, taps, beliefs, _ = _tiny_track(1e-3)
  for t in (0, 1):
    out, stats, count = ref.vote_smooth(beliefs[t], beliefs[t + 1], taps[t + 1], 1e-3)
    assert abs(np.exp(out).sum() - 1) < 1e-12 and count[0] == out.size
    assert abs(stats[0]) < 64 * 2.0 ** -24 * (1 + np.abs(beliefs[t]).max())
  for c in ref.all_inputs():
    out = ref.vote_smooth(c['belief'], c['next'], c['taps'], c['uniform_mix'])[0]
    fin = np.isfinite(out)
    if fin.any():
      assert abs(np.exp(out[fin]).sum() - 1) < 1e-9, c['name']


def test_identity_taps_without_mix_return_next_where_the_belief_has_mass():
  rng = np.random.default_rng(3)
  shape = (3, 4, 5)
  belief = flt.vote_filter(None, rng.standard_normal(shape).astype(np.float32), None, 3.0, 0.0)[0].astype(np.float32)
  belief[rng.random(shape) < 0.2] = -np.inf
  still = (np.ones(1, np.float32), 0, np.ones((3, 1), np.float32), np.ones((3, 1), np.float32), np.zeros((3, 2), np.int32))
  nxt = flt.vote_filter(belief, rng.standard_normal(shape).astype(np.float32), still, 1.0, 0.0)[0].astype(np.float32)
  out, stats, count = ref.vote_smooth(belief, nxt, still, 0.0)
  has = np.isfinite(belief)
  assert (np.isfinite(out) == has).all() and count[3] == has.sum()
  assert np.abs(out[has] - nxt[has]).max() < 16 * 2.0 ** -24 * (1 + np.abs(nxt[has]).max())


def test_full_mix_returns_the_normalised_belief():
  c = {c['name']: c for c in ref.all_inputs()}['mix1']
  out, stats, _ = ref.vote_smooth(c['belief'], c['next'], c['taps'], 1.0)
  b = c['belief'].astype(np.float64)
  fin = np.isfinite(b)
  want = b[fin] - (b[fin].max() + np.log(np.exp(b[fin] - b[fin].max()).sum()))
  assert (np.isfinite(out) == fin).all() and np.abs(out[fin] - want).max() < 1e-9


@pytest.mark.parametrize('name', ['wrap', 'wrap_neg', 'ragged', 'tk16', 'wide', 'tall'])
def test_adjoint_identity(name):
  c = {c['name']: c for c in ref.all_inputs()}[name]
  w = ref._walk(c['belief'], c['next'], c['taps'], c['uniform_mix'])[3]
  lhs, rhs = (w['t2'] * w['q']).sum(), (w['p'] * w['u']).sum()
  assert lhs > 0 and abs(lhs - rhs) <= 1e-12 * lhs


def test_bad_cells_and_empty_mass():
  by = {c['name']: c for c in ref.all_inputs()}
  c = by['bad']
  out, stats, count = ref.vote_smooth(c['belief'], c['next'], c['taps'], c['uniform_mix'])
  assert np.isnan(out[3, 10, 11]) and np.isnan(out[30, 20, 5]) and int(np.isnan(out).sum()) == 2
  assert count[1] == 2 and count[2] == 2 and np.isfinite(out[7, 15, 16]) == np.isfinite(c['belief'][7, 15, 16])
  clean = ref.vote_smooth(by['ragged']['belief'], by['ragged']['next'], c['taps'], c['uniform_mix'])[2]
  assert count[3] == clean[3] - 2
  for name in ('no_mass', 'empty_belief'):
    c = by[name]
    out, stats, count = ref.vote_smooth(c['belief'], c['next'], c['taps'], c['uniform_mix'])
    assert (out == -np.inf).all() and stats[0] == -np.inf and stats[3] == -np.inf and count[0] == 0
  assert ref.vote_smooth(by['no_mass']['belief'], by['no_mass']['next'], by['no_mass']['taps'], 1e-3)[1][2] == -np.inf
  assert by['empty_belief']['uniform_mix'] > 0 and ref.vote_smooth(
      by['empty_belief']['belief'], by['empty_belief']['next'], by['empty_belief']['taps'], 0.5)[1][1] == 0


def test_exact_case_has_unit_masses():
  c = ref.exact_case()
  w = ref._walk(c['belief'], c['next'], c['taps'], 0.0)[3]
  assert set(np.unique(w['p'])) == {0.0, 1.0} and set(np.unique(w['q'])) == {0.0, 1.0} and w['Q'] >= 4
  assert (w['u'] * 2.0 ** 10 == np.round(w['u'] * 2.0 ** 10)).all() and w['fin'].sum() > 10


def test_cut_case_straddles_the_cut():
  c = {c['name']: c for c in ref.all_inputs()}['cut']
  w = ref._walk(c['belief'], c['next'], c['taps'], c['uniform_mix'])[3]
  below = w['has'] & (w['q'] == 0)
  assert below.sum() > 100 and (w['has'] & (w['q'] > 0) & (w['d'] < -30)).sum() > 100


def test_inputs_are_reproducible_and_bounds_finite():
  a, b = ref.all_inputs(), ref.all_inputs()
  assert [c['name'] for c in a] == ['tiny', 'wrap', 'wrap_far', 'wrap_neg', 'ragged', 'mix0', 'mix1', 'bad', 'wide',
                                    'tall', 'tk16', 'tiles', 'empty_belief', 'no_mass', 'cut', 'exact']
  for x, y in zip(a, b):
    assert x['belief'].tobytes() == y['belief'].tobytes() and x['next'].tobytes() == y['next'].tobytes()
    for s, t in zip(x['taps'], y['taps']):
      assert np.asarray(s).tobytes() == np.asarray(t).tobytes()
  for c in a:
    if c['name'] == 'tiles':
      continue
    tol = ref.bound(c['belief'], c['next'], c['taps'], c['uniform_mix'])
    assert np.isfinite(tol).all() and tol.max(initial=0.0) < 1e-4, c['name']
    assert np.isfinite(ref.stats_bound(c['belief'], c['next'], c['taps'], c['uniform_mix'])).all()
