"""CPU pins of the temperature-ladder contract (snap_vote_temper_f32, include/snap_hip.h): the float64 numpy
restatement ``vote_temper_reference`` against ``scipy.special.logsumexp`` and softmax moments, against
``vote_posterior_reference`` at every scale, its derivative identities and closed forms, the documented error bound
against a float32 restatement of the kernel's per-pixel sums on every input of the GPU tests, the C entry points'
argument validation (no launch), and the host half of the temperature fit (``solve_temperature``, ``TemperatureFit``
through ``add_table`` on CPU tensors, ``temperature_ladder``)."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.special import logsumexp, softmax

import vote_posterior_reference as pref
import vote_temper_reference as ref
from snap_amd import _lib
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import grids

# (without 'huge': scale * v leaves what a float64 sum of exponentials can hold, and vote_posterior's contract)
SMALL = [n for n in ref.all_inputs() if n[1].size <= 40000 and n[0] != 'huge']


def _kernel_f32(v, scales, gt=None):
  """The kernel's arithmetic restated in numpy: d, x, e and the two products in f32, a pixel's sums over r in f32 in
  order, float64 above.  Not bit-equal to the device (numpy's exp rounds differently); the same rounding points."""
  f32, f64 = np.float32, np.float64
  want = ref.vote_temper(v, scales, gt)
  F = np.isfinite(v)
  if not F.any():
    return want[0]
  R = v.shape[0]
  m = f32(v[F].max())
  table = want[0].copy()
  v_gt = want[1][1]
  with np.errstate(invalid='ignore', under='ignore', over='ignore'):
    d = np.where(F, v - m, f32(0)).astype(f32).reshape(R, -1)
    Ff = F.reshape(R, -1)
    for l, s in enumerate(ref.ladder(scales)):
      x = np.maximum((f32(s) * d).astype(f32), f32(-128))
      e = np.where(Ff, np.exp(x).astype(f32), f32(0))
      ex = (e * x).astype(f32)
      exx = (ex * x).astype(f32)
      s0, s1, s2 = (np.zeros(d.shape[1], f32) for _ in range(3))
      for r in range(R):
        s0, s1, s2 = (s0 + e[r]).astype(f32), (s1 + ex[r]).astype(f32), (s2 + exx[r]).astype(f32)
      S0, S1, S2 = s0.astype(f64).sum(), s1.astype(f64).sum(), s2.astype(f64).sum()
      A, smu = np.log(S0), S1 / S0
      mu, q = smu / s, S2 / S0 / (s * s)
      log_z = s * f64(m) + A
      table[l, :7] = (log_z, m + mu, max(q - mu * mu, 0.0), A - smu, -A, s * v_gt - log_z, (m + mu) - v_gt)
  return table


@pytest.mark.parametrize('case', SMALL, ids=[c[0] for c in SMALL])
def test_reference_against_scipy(case):
  name, v, scales, gt = case
  table, stats, count = ref.vote_temper(v, scales, gt)
  F = np.isfinite(v)
  assert count[0] == F.sum() and count[1] == (np.isnan(v) | (v == np.inf)).sum()
  vf = v[F].astype(np.float64)
  assert stats[0] == vf.max()
  for l, s in enumerate(ref.ladder(scales)):
    x = s * vf
    log_z = logsumexp(x)
    p = softmax(x)
    mean = (p * vf).sum()
    var = (p * (vf - mean) ** 2).sum()
    ent = -(p[p > 0] * np.log(p[p > 0])).sum()
    assert abs(table[l, 0] - log_z) <= 1e-12 * max(1, abs(log_z))
    assert abs(table[l, 1] - mean) <= 1e-12 and abs(table[l, 2] - var) <= 1e-11
    assert abs(table[l, 3] - ent) <= 1e-10 and abs(table[l, 4] - np.log(p.max())) <= 1e-12
    assert table[l, 7] == 0


@pytest.mark.parametrize('case', SMALL, ids=[c[0] for c in SMALL])
def test_log_prob_gt_against_the_posterior_reference(case):
  name, v, scales, gt = case
  table, stats, count = ref.vote_temper(v, scales, gt)
  for l, s in enumerate(ref.ladder(scales)):
    ps, pc = pref.vote_posterior(v, np.float32(s), gt)[2:]
    assert pc.tolist() == count[:3].tolist()
    assert abs(ps[0] - table[l, 0]) <= 1e-11 * max(1, abs(ps[0])) and abs(ps[11] - table[l, 3]) <= 1e-10
    if count[2]:
      assert abs(ps[12] - table[l, 5]) <= 1e-11 * max(1, abs(ps[12]))
    else:
      assert np.isnan(ps[12]) and np.isnan(table[l, 5]) and np.isnan(table[l, 6]) and np.isnan(stats[1])


def test_the_ground_truth_cases_are_what_they_are_called():
  v, cases = ref.gt_cases()
  for name, idx, valid in cases:
    table, stats, count = ref.vote_temper(v, ref.LADDERS[5], idx)
    assert count[2] == valid, name
  # circular in k: R + 2.5 samples what 2.5 samples; an integer index is the cell itself
  a = ref.vote_temper(v, (1.0,), (v.shape[0] + 2.5, 6.5, 6.5))[1][1]
  b = ref.vote_temper(v, (1.0,), (2.5, 6.5, 6.5))[1][1]
  assert a == b and ref.vote_temper(v, (1.0,), (2.0, 4.0, 9.0))[1][1] == np.float64(v[2, 4, 9])


def test_finite_differences():
  """d log_z / d s = E[v] and d E[v] / d s = Var[v] (central differences at a relative step of 2^-10, on scales that are
  f32 numbers: the ladder is rounded to f32)."""
  v = ref.random_votes((4, 7, 7))
  for s in (0.5, 2.0, 8.0):
    h = s * 2.0 ** -10
    t = ref.vote_temper(v, (s - h, s, s + h))[0]
    assert abs((t[2, 0] - t[0, 0]) / (2 * h) - t[1, 1]) <= 1e-5 * (1 + abs(t[1, 1]))
    assert abs((t[2, 1] - t[0, 1]) / (2 * h) - t[1, 2]) <= 1e-5 * (1 + t[1, 2])


def test_two_valued_votes_closed_form():
  """n0 cells at 0 and n1 at -c: log_z = log(n0 + n1 exp(-s c)), E[v] = -c w, Var[v] = c^2 w (1 - w) with
  w = n1 exp(-s c) / (n0 + n1 exp(-s c))."""
  n0, n1, c = 5, 17, 1.5
  v = np.full((2, 4, 4), -np.inf, np.float32)
  v.reshape(-1)[:n0] = 0
  v.reshape(-1)[n0:n0 + n1] = -c
  scales = ref.LADDERS[5]
  t = ref.vote_temper(v, scales)[0]
  for l, s in enumerate(ref.ladder(scales)):
    z = n0 + n1 * np.exp(-s * c)
    w = n1 * np.exp(-s * c) / z
    assert abs(t[l, 0] - np.log(z)) <= 1e-13 and abs(t[l, 1] + c * w) <= 1e-13
    assert abs(t[l, 2] - c * c * w * (1 - w)) <= 1e-13 and abs(t[l, 4] + np.log(z)) <= 1e-13


def test_zero_or_masked_votes():
  v = ref.exact_votes((36, 31, 33))
  n = int(np.isfinite(v).sum())
  t = ref.vote_temper(v, ref.LADDERS[16])[0]
  assert (t[:, 0] == np.log(n)).all() and (t[:, 1] == 0).all() and (t[:, 2] == 0).all()
  assert (t[:, 3] == np.log(n)).all() and (t[:, 4] == -np.log(n)).all()


def test_empty_single_and_huge():
  t, s, c = ref.vote_temper(np.full((3, 2, 2), -np.inf, np.float32), (1.0, 2.0), (0.0, 0.0, 0.0))
  assert (t[:, 0] == -np.inf).all() and np.isnan(t[:, 1:7]).all() and (t[:, 7] == 0).all()
  assert s[0] == -np.inf and np.isnan(s[1]) and c.tolist() == [0, 0, 0, 0]
  v, cell = ref.single_cell_votes()
  t = ref.vote_temper(v, ref.LADDERS[5])[0]
  assert (t[:, 1] == np.float64(v[cell])).all() and (t[:, 2:5] == 0).all()
  # votes around 1e30 at a scale of 1e10: everything finite, the two tied maxima share the mass
  t, s, c = ref.vote_temper(ref.huge_votes(), ref.HUGE_SCALES, ref.HUGE_GT)
  assert np.isfinite(t).all() and c[2] == 1 and abs(t[-1, 3] - np.log(2)) < 1e-15 and t[-1, 1] == s[0]
  assert np.isfinite(ref.bound(ref.huge_votes(), ref.HUGE_SCALES, ref.HUGE_GT)).all()
  with np.errstate(over='ignore', invalid='ignore'):
    assert np.isnan(pref.two_level_f32(ref.huge_votes(), 1e10)[2][0])           # what the ladder's contract avoids


@pytest.mark.parametrize('case', ref.all_inputs(), ids=[c[0] for c in ref.all_inputs()])
def test_the_bound_holds_for_the_kernels_rounding_points(case):
  name, v, scales, gt = case
  want = ref.vote_temper(v, scales, gt)[0]
  tol = ref.bound(v, scales, gt)
  got = _kernel_f32(v, scales, gt)
  with np.errstate(invalid='ignore'):
    err = np.where((got == want) | (np.isnan(got) & np.isnan(want)), 0.0, np.abs(got - want))
  assert np.isfinite(tol).all() and (tol[:, 7] == 0).all()
  share = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0.0))
  print(name, 'largest share of the bound per column', share.max(0).round(3).tolist())
  assert (err <= tol).all(), (name, np.argwhere(~(err <= tol))[0].tolist())
  # and the bound is not vacuous: log_z within 1e-4 for every input with votes of order 1
  if name != 'huge':
    assert tol[:, 0].max() < 1e-4


def test_c_entry_points_refuse_before_any_launch():
  lib = _lib.load()
  q = lib.snap_vote_temper_workspace_bytes
  assert q(4, 7, 7, 16) > 0 and q(64, 1, 1, 1) > 0 and q(4, 7, 7, 16) % 8 == 0
  assert q(65, 7, 7, 4) == 0 and q(0, 7, 7, 4) == 0 and q(4, 0, 7, 4) == 0 and q(4, 7, 7, 0) == 0 and q(4, 7, 7, 17) == 0
  assert q(64, 6000, 6000, 4) == 0                                              # 2^31 cells and beyond
  assert q(2, 520, 520, 16) == 1024 * 48 * 8 + 1024 * 4 + 1024 * 8              # the plan is capped at 1024 workgroups
  host = (ctypes.c_double * 64)()                                               # stands for every device pointer: never read
  p = ctypes.cast(host, ctypes.c_void_p)
  need = q(4, 7, 7, 3)
  def call(R=4, scales=(1.0, 2.0, 3.0), S=None, nbytes=need, votes=p, ws=p):
    arr = (ctypes.c_float * max(len(scales), 1))(*scales)
    return lib.snap_vote_temper_f32(votes, R, 7, 7, arr, len(scales) if S is None else S, None, p, p, p, ws, nbytes, None)
  assert call(votes=None) == -3 and call(ws=None) == -3
  assert call(R=65) == -1 and call(S=0) == -1 and call(scales=(1.0,) * 17) == -1
  for bad in ((1.0, 1.0, 2.0), (2.0, 1.0, 3.0), (0.0, 1.0, 2.0), (-1.0, 1.0, 2.0), (1.0, 2.0, float('inf')),
              (1.0, float('nan'), 3.0)):
    assert call(scales=bad) == -2, bad
  assert call(nbytes=need - 1) == -5
  assert call(ws=ctypes.c_void_p(p.value + 4)) == -5


def test_temperature_ladder():
  t = pev.temperature_ladder(0.25, 16.0, 16)
  assert t.dtype == np.float64 and t.shape == (16,) and t[0] == 0.25 and t[-1] == 16.0
  assert np.allclose(t[1:] / t[:-1], 64 ** (1 / 15)) and (np.diff(t.astype(np.float32)) > 0).all()
  assert pev.temperature_ladder(2.0, 2.0, 1).tolist() == [2.0]
  for bad in ((1.0, 1.0 + 2.0 ** -23, 16), (2.0, 1.0, 4), (0.0, 1.0, 4), (1.0, float('inf'), 4), (1.0, 2.0, 17),
              (1.0, 2.0, 0), (1.0, 1.0, 2), (float('nan'), 2.0, 3)):
    with pytest.raises(ValueError):
      pev.temperature_ladder(*bad)


def _quadratic_rows(t, s_star, curvature=3.0, frames=7):
  """nll, slope, var of the convex NLL curvature / 2 (s - s_star)^2 on the ladder t."""
  t = np.asarray(t, np.float64)
  return 0.5 * curvature * (t - s_star) ** 2, curvature * (t - s_star), np.full(t.size, curvature), frames


def test_solve_temperature_brackets_and_interpolates():
  t = pev.temperature_ladder(0.5, 8.0, 9)
  out = pev.solve_temperature(t, *_quadratic_rows(t, 2.3))
  assert out['bracketed'] and out['bracket'] == (t[4], t[5]) and t[4] < 2.3 < t[5] and out['frames'] == 7
  assert abs(out['temperature'] - 2.3) < 1e-12                 # a linear slope: the Hermite interpolant is exact
  assert out['nll'].shape == (9,)
  # a cubic slope with matching derivatives: still exact; a convex non-polynomial: inside the bracket and close
  g = lambda s: (s - 1.7) ** 3 + (s - 1.7)
  dg = lambda s: 3 * (s - 1.7) ** 2 + 1
  out = pev.solve_temperature(t, np.zeros(9), g(t), dg(t), 3)
  assert out['bracketed'] and out['bracket'][0] < 1.7 < out['bracket'][1] and abs(out['temperature'] - 1.7) < 1e-12
  out = pev.solve_temperature(t, np.zeros(9), np.log(t / 3.1), 1 / t, 3)
  assert out['bracket'][0] < 3.1 < out['bracket'][1] and abs(out['temperature'] - 3.1) < 2e-3
  # derivatives that contradict the values: the root of the interpolant still lies in the bracket
  out = pev.solve_temperature(t, np.zeros(9), t - 2.3, np.full(9, 1e6), 3)
  assert out['bracket'][0] <= out['temperature'] <= out['bracket'][1]
  out = pev.solve_temperature(t, np.zeros(9), t - 2.3, np.full(9, np.inf), 3)
  assert out['temperature'] == 0.5 * (out['bracket'][0] + out['bracket'][1])   # not finite: the bracket's midpoint
  # a ladder point that is the minimiser
  out = pev.solve_temperature(t, *_quadratic_rows(t, t[3]))
  assert out['bracketed'] and out['bracket'][0] <= t[3] <= out['bracket'][1] and abs(out['temperature'] - t[3]) < 1e-12
  out = pev.solve_temperature(t, *_quadratic_rows(t, t[0]))
  assert out['bracketed'] and out['temperature'] == t[0]


def test_solve_temperature_without_a_sign_change():
  t = pev.temperature_ladder(0.5, 8.0, 9)
  low = pev.solve_temperature(t, *_quadratic_rows(t, 0.1))
  assert not low['bracketed'] and low['temperature'] == 0.5 and low['bracket'] == (0.5, 0.5)
  high = pev.solve_temperature(t, *_quadratic_rows(t, 20.0))
  assert not high['bracketed'] and high['temperature'] == 8.0 and high['bracket'] == (8.0, 8.0)
  none = pev.solve_temperature(t, np.zeros(9), np.zeros(9), np.zeros(9), 0)
  assert not none['bracketed'] and np.isnan(none['temperature']) and none['frames'] == 0


def test_temperature_fit_on_reference_tables():
  """``TemperatureFit.add_table`` on CPU tensors built from the reference: the reference alone brackets the exact
  minimiser strictly inside the first ladder (what the GPU test relies on), the frames with an invalid ground truth
  change nothing, and the Hermite estimate lies in the bracket."""
  volumes, gts = ref.fit_frames()
  lo, hi, num = ref.FIT_LADDER
  ladder = pev.temperature_ladder(lo, hi, num)
  s_star, frames = ref.nll_minimiser(volumes, gts, lo, hi)
  assert frames == ref.FIT_FRAMES - 2 and ladder[1] < s_star < ladder[-2]
  grid = grids.Grid2D((5, 5), 0.25)
  fit, fit_valid = pev.TemperatureFit(grid, 4, ladder), pev.TemperatureFit(grid, 4, ladder)
  assert fit.solve()['frames'] == 0 and np.isnan(fit.solve()['temperature'])
  for v, gt in zip(volumes, gts):
    table, _, count = ref.vote_temper(v, ladder, gt)
    fit.add_table(torch.from_numpy(table), torch.from_numpy(count))
    if count[2]:
      fit_valid.add_table(torch.from_numpy(table), torch.from_numpy(count))
  out, out_valid = fit.solve(), fit_valid.solve()
  assert out['frames'] == frames and out['bracketed']
  assert out['temperature'] == out_valid['temperature'] and (out['nll'] == out_valid['nll']).all()
  assert out['bracket'][0] < s_star < out['bracket'][1] and out['bracket'][0] <= out['temperature'] <= out['bracket'][1]
  print(f'exact minimiser {s_star:.9f}, Hermite estimate {out["temperature"]:.9f} in {out["bracket"]}')
  assert abs(out['temperature'] - s_star) < 0.05 * (out['bracket'][1] - out['bracket'][0])
  used = out['temperatures'].tolist()                          # (the ladder as f32: what the kernel multiplies by)
  assert int(np.argmin(out['nll'])) in (used.index(out['bracket'][0]), used.index(out['bracket'][1]))
  with pytest.raises(ValueError):
    fit.add_table(torch.zeros((3, 8), dtype=torch.float64), torch.zeros(4, dtype=torch.int32))
