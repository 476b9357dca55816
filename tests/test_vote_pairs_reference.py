"""``vote_pairs_reference`` (the float64 restatement the GPU tests compare ``ops.vote_pairs`` with) against its own
brute-force enumeration, the dense alpha-beta recursion of ``vote_smooth_reference`` and its invariants; then the EM
fit's host half (``pose_exhaustive_voting.noise_m_step`` / ``motion_noise_objective``) on the reference filter and
smoother.  No GPU."""
import functools
import math

import numpy as np
import pytest
import torch

import vote_filter_reference as flt
import vote_pairs_reference as ref
import vote_smooth_reference as smo
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import geometry, grids


def _tiny_track(eps):
  votes, taps, scale = smo.tiny_track()
  beliefs, prev = [], None
  for t in range(len(votes)):
    prev = flt.vote_filter(prev, votes[t], taps[t] or smo.still_taps(3), scale, eps)[0].astype(np.float32)
    beliefs.append(prev)
  return votes, taps, beliefs, scale


@pytest.mark.parametrize('eps', [0.0, 1e-3])
def test_marginals_of_the_enumerated_joint_are_the_separable_histograms(eps):
  """The joint N[r', tk, ta, tb] enumerated cell by cell, summed over the other two tap axes (and, for k, over the
  rotations), against (a): at float64 noise (1e-12 of a total of 1) without the f32 roundings, within the derived
  bound (once, not twice) with them.  Measured: 2.2e-16 without the roundings; with them at most 0.006 of the bound."""
  votes, taps, beliefs, _ = _tiny_track(eps)
  smoothed = smo.smooth_track(beliefs, taps, eps)
  for t in (0, 1):
    nxt = np.asarray(smoothed[t + 1], np.float32)
    N, J, xi = ref.dense_pairs(beliefs[t], np.exp(nxt.astype(np.float64)), taps[t + 1], eps)
    total = N.sum() + J
    assert abs(xi.sum() - total) < 1e-12
    want = (N.sum((0, 2, 3)) / total, N.sum((1, 3)) / total, N.sum((1, 2)) / total, N.sum() / total, J / total)
    hk, ha, hb, stats, _ = ref.vote_pairs(beliefs[t], nxt, taps[t + 1], eps, rounded=False)
    err = max(np.abs(hk - want[0]).max(), np.abs(ha - want[1]).max(), np.abs(hb - want[2]).max(),
              abs(stats[0] - want[3]), abs(stats[1] - want[4]))
    print(f'eps {eps} step {t}: unrounded max err {err:.3e}, log_norm {stats[2]:.3e} / {math.log(total):.3e}')
    assert err < 1e-12 and abs(stats[2] - math.log(total)) < 1e-12
    got = ref.vote_pairs(beliefs[t], nxt, taps[t + 1], eps)
    bk, ba, bb, bs = ref.bounds(beliefs[t], nxt, taps[t + 1], eps)
    over = lambda err, b: float(np.max(np.abs(err) / np.maximum(b, 1e-300)))
    frac = max(over(got[0] - want[0], bk), over(got[1] - want[1], ba), over(got[2] - want[2], bb),
               over(got[3][0] - want[3], bs[0]), over(got[3][1] - want[4], bs[1]))
    print(f'eps {eps} step {t}: rounded max err / bound {frac:.3f}')
    assert frac <= 1.0


# The largest |sum_x' xi - gamma_t| and |sum_x xi - gamma_{t+1}| measured on ``tiny_track`` (linear space, gammas sum
# to 1), and the tolerance: 10 x the larger.
XI_MEASURED = (2.4e-8, 8.4e-17)
XI_TOL = 2.4e-7


@pytest.mark.parametrize('eps', [0.0, 1e-3])
def test_pair_posterior_marginals_are_the_dense_smoothers_gammas(eps):
  """xi[x, x'] enumerated from the f32 belief of frame t and the dense alpha-beta gamma_{t+1} (float64, linear):
  its column sums are gamma_{t+1} (by construction, at float64 noise: measured 8.4e-17) and its row sums the dense
  gamma_t, which comes from the raw votes without any belief: measured 2.4e-8 at worst (eps = 0, step 0; the f32
  rounding of the stored belief, 2^-24 |log alpha| relative per cell, is what separates the two; the smoother's own
  identity held at 3e-10 in log space on its largest cells).  Tolerance 2.4e-7 = 10 x the measured figure; a wrong
  offset or pass order is at 1e-2."""
  votes, taps, beliefs, scale = _tiny_track(eps)
  gamma = smo.dense_smoothing(votes, taps, scale, eps, beliefs)
  shape = votes[0].shape
  for t in (0, 1):
    N, J, xi = ref.dense_pairs(beliefs[t], gamma[t + 1].reshape(shape), taps[t + 1], eps)
    e_next = np.abs(xi.sum(0) - gamma[t + 1]).max()
    e_cur = np.abs(xi.sum(1) - gamma[t]).max()
    print(f'eps {eps} step {t}: |sum_x xi - gamma_t+1| {e_next:.3e}, |sum_x\' xi - gamma_t| {e_cur:.3e}')
    assert e_next <= XI_TOL and e_cur <= XI_TOL
    assert abs(N.sum() + J - 1) <= XI_TOL
    if eps == 0:
      assert J == 0
  wrong = ref.dense_pairs(beliefs[0], gamma[2].reshape(shape), taps[2], eps)[2]
  assert np.abs(wrong.sum(1) - gamma[0]).max() > 1e-3


@functools.lru_cache(maxsize=None)
def _cases():
  return {c['name']: c for c in ref.all_inputs() if c['name'] != 'tiles'}


@pytest.mark.parametrize('name', ['tiny', 'wrap', 'wrap_far', 'wrap_neg', 'ragged', 'mix0', 'mix1', 'bad', 'wide', 'tall',
                                  'tk16', 'empty_belief', 'no_mass', 'cut', 'exact', 'still', 'big'])
def test_invariants(name):
  c = _cases()[name]
  hk, ha, hb, stats, count = ref.vote_pairs(c['belief'], c['next'], c['taps'], c['uniform_mix'])
  bk, ba, bb, bs = ref.bounds(c['belief'], c['next'], c['taps'], c['uniform_mix'], exact=name == 'exact')
  stay, jump = stats[0], stats[1]
  if name == 'no_mass':
    assert stay == 0 and jump == 0 and stats[2] == -np.inf and not hk.any() and not ha.any() and not hb.any()
    return
  assert abs(stay + jump - 1) < 1e-12
  # each table sums to stay: the f32 roundings between the passes separate them, within the bounds
  for h, b in ((hk, bk), (ha, ba), (hb, bb)):
    assert abs(h.sum() - stay) <= b.sum() + bs[0], name
  assert np.isfinite(bk).all() and np.isfinite(ba).all() and np.isfinite(bb).all()
  if c['uniform_mix'] == 0:
    assert jump == 0 and stay == 1
  if name in ('mix1', 'empty_belief'):                      # eps = 1 / no belief mass: only the jump branch
    assert jump == 1 and not hk.any()
  if name in ('tiny', 'still'):
    assert hk.tolist() == [1.0] and ha.shape[1] == 1 and hb.shape[1] == 1   # Tk = Ta = Tb = 1
    assert abs(ha.sum() - 1) < 1e-6 and abs(hb.sum() - 1) < 1e-6
  if name == 'exact':
    assert not bk.any() and not ba.any() and not bb.any() and hk.sum() == 1 and ha.sum() == 1 and hb.sum() == 1
  # the reference filter's mass_kept of the same step, rounded as the kernel rounds it
  p = flt.masses(c['belief'])[0]
  if p.sum() > 0:
    assert abs(stats[3] - flt.predict(p, c['taps']).sum() / p.sum()) <= bs[3]
  assert count.tolist()[1:] == smo.vote_smooth(c['belief'], c['next'], c['taps'], c['uniform_mix'])[2].tolist()[1:]


def test_still_taps_put_every_histogram_on_one_tap():
  c = _cases()['still']
  hk, ha, hb, stats, _ = ref.vote_pairs(c['belief'], c['next'], c['taps'], 0.0)
  assert hk.tolist() == [1.0] and stats[0] == 1 and stats[1] == 0
  # per rotation the single tap holds that rotation's share of gamma_{t+1}
  share = np.exp(c['next'].astype(np.float64)).sum((1, 2))
  assert np.abs(ha[:, 0] - share).max() < 1e-6 and np.abs(hb[:, 0] - share).max() < 1e-6
  assert abs(stats[2]) < 64 * 2.0 ** -24 * (1 + np.abs(c['belief']).max())


# ---------------------------------------------------------------------------------------------------------------
# EM on the reference filter and smoother
# ---------------------------------------------------------------------------------------------------------------
R_EM, GRID_EM = 8, grids.Grid2D((8, 9), 0.25)               # the lattice [8, 15, 17]
PLANTED = dict(sigma_xy=0.15, sigma_yaw=0.12)
START = dict(sigma_xy=0.45, sigma_yaw=0.36, uniform_mix=1e-3)


def np_taps(inc, grid, R, sigma_xy, sigma_yaw, truncate=3.0):
  """``motion_taps`` on the host: the same float64 tables rounded to f32 once -> the numpy tap tuple."""
  (wk, lk), (wa, la), (wb, lb) = pev._motion_axes(inc, grid, R, sigma_xy, sigma_yaw, truncate)
  return (wk[0].astype(np.float32), int(lk[0]), wa.astype(np.float32), wb.astype(np.float32),
          np.stack([la, lb], -1).astype(np.int32))


@functools.lru_cache(maxsize=None)
def em_track():
  """12 frames on [8, 15, 17]: known odometry increments (back and forth, so the track stays inside), the true
  motion = odometry + planted Gaussian noise, votes sharply peaked (0.6 cells / 0.4 bins) at the true continuous
  index -> (votes [12] f32, increments [12] (entry 0 None), scale)."""
  rng = np.random.default_rng(11)
  R, grid = R_EM, GRID_EM
  f64 = lambda *v: torch.tensor(v if len(v) > 1 else v[0], dtype=torch.float64)
  pose = pev.exhaustive_index_to_tfm(torch.tensor([3.0, 7.0, 8.0], dtype=torch.float64), grid, R)
  pose = geometry.Transform2D(pose.angle.double(), pose.t.double())
  votes, increments = [], []
  k, a, b = np.meshgrid(np.arange(R), np.arange(15), np.arange(17), indexing='ij')
  for n in range(12):
    if n == 0:
      increments.append(None)
    else:
      sign = 1.0 if (n // 2) % 2 == 0 else -1.0
      odo = geometry.Transform2D(f64(0.35 * sign), f64(0.3 * sign, -0.22 * sign))
      true = geometry.Transform2D(odo.angle + rng.normal(0, PLANTED['sigma_yaw']),
                                  odo.t + f64(*rng.normal(0, PLANTED['sigma_xy'], 2)))
      pose = pose @ true.inv
      increments.append(odo)
    idx = pev.exhaustive_tfm_to_index(pose, grid, R).numpy()
    dk = (k - idx[0] + R / 2) % R - R / 2
    v = -(dk ** 2 / (2 * 0.4 ** 2) + ((a - idx[1]) ** 2 + (b - idx[2]) ** 2) / (2 * 0.6 ** 2))
    votes.append(v.astype(np.float32))
  return votes, increments, 1.0


def reference_e_step(votes, increments, scale, grid, R, sigma_xy, sigma_yaw, uniform_mix):
  """Reference filter, smoother and tap posteriors of a track -> (stats dicts as ``track_statistics`` gives them, with
  numpy arrays; the total log-evidence)."""
  taps = [None] + [np_taps(inc, grid, R, sigma_xy, sigma_yaw) for inc in increments[1:]]
  beliefs, prev, evidence = [], None, 0.0
  for t in range(len(votes)):
    out, st, _ = flt.vote_filter(prev, votes[t], taps[t] or smo.still_taps(R), scale, uniform_mix)
    prev = out.astype(np.float32)
    beliefs.append(prev)
    evidence += float(np.float32(st[0]))
  smoothed = smo.smooth_track(beliefs, taps, uniform_mix)
  stats = []
  for t in range(len(votes) - 1):
    hk, ha, hb, s, _ = ref.vote_pairs(beliefs[t], np.asarray(smoothed[t + 1], np.float32), taps[t + 1], uniform_mix)
    stats.append(dict(hist_k=hk, hist_a=ha, hist_b=hb, stay=s[0], jump=s[1], log_norm=s[2], mass_kept=s[3],
                      taps=taps[t + 1]))
  return stats, evidence


def reference_fit(votes, increments, scale, grid, R, start, iterations):
  cur, records = dict(start), []
  for _ in range(iterations):
    stats, evidence = reference_e_step(votes, increments, scale, grid, R, **cur)
    m = pev.noise_m_step(stats, increments, grid, R, cur['sigma_xy'], cur['sigma_yaw'])
    records.append(dict(cur, log_evidence=evidence, jump=m['jump'], m_step=m))
    cur = dict(sigma_xy=m['sigma_xy'], sigma_yaw=m['sigma_yaw'], uniform_mix=m['uniform_mix'])
  return cur, records


def test_em_on_the_reference_raises_the_objective_and_the_evidence():
  """Planted sigma_xy = 0.15 m, sigma_yaw = 0.12 rad; start 3 x too large (0.45 m, 0.36 rad, uniform_mix 1e-3), five
  iterations on the default candidate grid.  Asserted: every M-step's chosen candidate has an objective >= that of the
  current value (exact by construction: the current value is a candidate), and the log-evidence of the fitted values
  exceeds the initial one.  Not asserted, recorded: the fit ends at sigma_xy = 0.1593 m (planted 0.15), sigma_yaw =
  0.36 rad (unchanged: 0.46 of a 0.785 rad bin, where every narrower candidate puts less than 2^-20 on an outer tap
  that carries posterior mass and is at -inf, and every wider one scores lower), uniform_mix = 1e-6 (its floor: no
  step needs the jump); the log-evidence goes -43.66 -> -41.50 -> -39.64 -> -36.71 -> -35.38, and is -35.38 at the
  fitted values."""
  votes, increments, scale = em_track()
  fitted, records = reference_fit(votes, increments, scale, GRID_EM, R_EM, START, 5)
  for i, r in enumerate(records):
    m = r['m_step']
    print(f"iteration {i}: sigma_xy {r['sigma_xy']:.4f} sigma_yaw {r['sigma_yaw']:.4f} uniform_mix "
          f"{r['uniform_mix']:.3e} log_evidence {r['log_evidence']:.4f} jump {r['jump']:.3e}")
    for name in ('sigma_xy', 'sigma_yaw'):
      print(f"  {name}: " + ' '.join(f'{c:.4f}:{o:.4f}' for c, o in zip(m['candidates'][name], m['objective'][name])))
      chosen = m['objective'][name][m['candidates'][name].index(m[name])]
      assert chosen >= m['current'][name] and math.isfinite(m['current'][name])
      assert r[name] in m['candidates'][name]
  final = reference_e_step(votes, increments, scale, GRID_EM, R_EM, **fitted)[1]
  print(f'fitted {fitted}, log_evidence {final:.4f}')
  assert final > records[0]['log_evidence']
  assert pev.NOISE_UNIFORM_MIX_RANGE[0] <= fitted['uniform_mix'] <= pev.NOISE_UNIFORM_MIX_RANGE[1]


def test_objective_edge_cases():
  votes, increments, scale = em_track()
  stats, _ = reference_e_step(votes[:3], increments[:3], scale, GRID_EM, R_EM, **START)
  at = lambda sxy, syaw, **kw: pev.motion_noise_objective(stats, increments[:3], GRID_EM, R_EM, sxy, syaw, **kw)
  here = at(START['sigma_xy'], START['sigma_yaw'])
  assert math.isfinite(here) and here < 0
  assert abs(at(START['sigma_xy'], START['sigma_yaw'], support='tables') - here) < 1e-9 * abs(here)
  # a narrower candidate has no tap where the histograms have mass: on its own support as soon as it loses a tap ...
  assert at(0.85 * START['sigma_xy'], START['sigma_yaw']) == -math.inf
  assert at(START['sigma_xy'], 0.5 * START['sigma_yaw']) == -math.inf
  # ... on the tables' support only once its outermost taps fall below the smallest tap
  assert math.isfinite(at(0.85 * START['sigma_xy'], START['sigma_yaw'], support='tables'))
  assert at(0.01, START['sigma_yaw'], support='tables') == -math.inf
  # 0 log 0 = 0: a wider candidate has taps the histograms never reach, and stays finite
  assert math.isfinite(at(0.9, 0.7))
  with pytest.raises(ValueError):
    at(0.3, 0.3, support='other')
  with pytest.raises(ValueError):
    pev.motion_noise_objective(stats, increments[:2], GRID_EM, R_EM, 0.3, 0.3)
  # the candidate grid holds the current value and never leaves what motion_taps accepts
  m = pev.noise_m_step(stats, increments[:3], GRID_EM, R_EM, 1.2, 1.3, candidates=(0.01, 1.0, 50.0))
  for name, cur in (('sigma_xy', 1.2), ('sigma_yaw', 1.3)):
    assert cur in m['candidates'][name] and len(m['candidates'][name]) == 3
  for sxy in m['candidates']['sigma_xy']:
    for syaw in m['candidates']['sigma_yaw']:
      pev._motion_axes(increments[1], GRID_EM, R_EM, sxy, syaw, 3.0)
