"""CPU pins of ``vote_filter_reference`` (the float64 restatement the GPU tests compare ``ops.vote_filter`` with) and of
the host builder ``pose_exhaustive_voting.motion_taps`` to things that are neither: a non-separable 3-D brute-force
sum with ``scipy.special.logsumexp``, the moments of the tap rows, the direction of motion through the host index <->
transform helpers, the mass cut at M - 40, hand-written masking cases."""
import math

import numpy as np
import pytest
import scipy.special
import torch

import vote_filter_reference as ref
import vote_fuse_reference as fuse_ref
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import geometry, grids


def _np_taps(taps):
  taps_k, lk, taps_a, taps_b, offsets = taps
  return tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (taps_k, lk, taps_a, taps_b, offsets))


def test_against_a_non_separable_brute_force_sum():
  rng = np.random.default_rng(0)
  R, Ho, Wo = 4, 5, 6
  belief = (rng.standard_normal((R, Ho, Wo)) * 3).astype(np.float32)
  belief[1, 2, 3] = -np.inf
  belief[2, 0, 0] = belief.max() - np.float32(50)           # below the cut: no mass
  votes = rng.standard_normal((R, Ho, Wo)).astype(np.float32)
  votes[0, 4, 5] = -np.inf
  taps = (ref.rand_taps(rng, 1, 3)[0], -1, ref.rand_taps(rng, R, 3), ref.rand_taps(rng, R, 2),
          rng.integers(-2, 1, (R, 2)).astype(np.int32))
  scale, eps = 1.5, 0.01
  tk, lk, ta, tb, off = taps
  d = belief - belief.max()                                 # f32 - f32: the contract's one f32 subtraction
  assert d.dtype == np.float32
  p = np.where(np.isfinite(belief) & (d >= -40), np.exp(d.astype(np.float64)), 0).astype(np.float32).astype(np.float64)
  t2 = np.zeros((R, Ho, Wo))
  for r in range(R):
    for a in range(Ho):
      for b in range(Wo):
        for ik in range(3):
          for ia in range(3):
            for ib in range(2):
              sa, sb = a + off[r, 0] + ia, b + off[r, 1] + ib
              if 0 <= sa < Ho and 0 <= sb < Wo:
                t2[r, a, b] += float(tk[ik]) * float(ta[r, ia]) * float(tb[r, ib]) * p[(r + lk + ik) % R, sa, sb]
  prior = (1 - float(np.float32(eps))) * t2 / t2.sum() + float(np.float32(eps)) / t2.size
  with np.errstate(divide='ignore'):
    u = float(np.float32(scale)) * votes.astype(np.float64) + np.log(prior)
  want = u - scipy.special.logsumexp(u[np.isfinite(u)])
  out, stats, count = ref.vote_filter(belief, votes, taps, scale, eps)
  assert (np.isfinite(out) == np.isfinite(want)).all() and out[0, 4, 5] == -np.inf
  fin = np.isfinite(want)
  assert np.abs(out[fin] - want[fin]).max() < 1e-12
  assert abs(stats[0] - scipy.special.logsumexp(u[np.isfinite(u)])) < 1e-12
  assert abs(stats[1] - t2.sum() / p.sum()) < 1e-14 and stats[1] < 1          # mass left through the borders
  assert stats[2] == belief.max() and abs(stats[3] - want[fin].max()) < 1e-12
  assert count.tolist() == [fin.sum(), 0, 0, R * Ho * Wo - 2]
  assert abs(np.exp(out[fin]).sum() - 1) < 1e-12
  b = ref.bound(belief, votes, taps, scale, eps)
  assert (b[fin] > 0).all() and (b[~fin] == 0).all() and b.max() < 2e-5


def test_start_uniform_mix_and_masking():
  rng = np.random.default_rng(1)
  R, Ho, Wo = 3, 4, 5
  votes = rng.standard_normal((R, Ho, Wo)).astype(np.float32)
  votes[1, 1, 1] = -np.inf
  belief = rng.standard_normal((R, Ho, Wo)).astype(np.float32)
  taps = (ref.rand_taps(rng, 1, 2)[0], 0, ref.rand_taps(rng, R, 2), ref.rand_taps(rng, R, 2), np.zeros((R, 2), np.int32))
  # belief = None and eps = 1 are the same update: softmax(scale * votes) over the finite cells, evidence against 1 / n
  fin = np.isfinite(votes)
  lz = scipy.special.logsumexp(2.0 * votes[fin].astype(np.float64))
  for out, stats, count in (ref.vote_filter(None, votes, taps, 2.0, 0.3), ref.vote_filter(belief, votes, taps, 2.0, 1.0)):
    assert np.abs(out[fin] - (2.0 * votes[fin] - lz)).max() < 1e-12 and out[1, 1, 1] == -np.inf
    assert abs(stats[0] - (lz - math.log(votes.size))) < 1e-12
    assert count[0] == votes.size - 1 and count[2] == 0
  _, stats, count = ref.vote_filter(None, votes, taps, 2.0, 0.3)
  assert stats[1] == 1 and stats[2] == -np.inf and count[1] == 0 and count[3] == 0
  # bad cells: a NaN / +inf belief cell has no mass and is counted; a NaN / +inf vote gives NaN and is left out
  b2, v2 = belief.copy(), votes.copy()
  b2[0, 0, 0], b2[2, 3, 4] = np.nan, np.inf
  v2[0, 2, 2], v2[2, 2, 2] = np.nan, np.inf
  out, stats, count = ref.vote_filter(b2, v2, taps, 1.0, 0.0)
  assert np.isnan(out[0, 2, 2]) and np.isnan(out[2, 2, 2]) and count.tolist()[1:3] == [2, 2]
  assert stats[2] == belief[np.isfinite(b2)].max() and count[3] == votes.size - 2
  assert abs(np.exp(out[np.isfinite(out)]).sum() - 1) < 1e-12
  # eps = 0 and a belief without mass where the taps look: -inf; nothing finite at all: everything -inf, log_z = -inf
  b3 = np.full((R, Ho, Wo), -np.inf, np.float32)
  b3[0, 0, 0] = 0
  far = (np.ones(1, np.float32), 0, np.ones((R, 1), np.float32), np.ones((R, 1), np.float32),
         np.tile(np.array([[Ho, 0]], np.int32), (R, 1)))
  out, stats, count = ref.vote_filter(b3, votes, far, 1.0, 0.0)
  assert (out == -np.inf).all() and stats[0] == -np.inf and stats[1] == 0 and count.tolist() == [0, 0, 0, 1]
  out, stats, count = ref.vote_filter(b3, votes, far, 1.0, 0.5)          # the uniform share alone
  assert count[0] == votes.size - 1 and stats[1] == 0


def test_the_cut_keeps_m_minus_40_and_drops_the_next_number_below():
  for M in (np.float32(0), np.float32(3.5), np.float32(-17.25)):
    edge = np.float32(M - np.float32(40))
    assert float(edge) == float(M) - 40                                  # exact in f32 for these M
    below = np.nextafter(edge, np.float32(-np.inf), dtype=np.float32)
    belief = np.array([[[M, edge, below, -np.inf]]], np.float32)
    p, m, bad, mass = ref.masses(belief)
    assert m == M and bad == 0 and mass == 2
    assert p[0, 0, 0] == 1 and p[0, 0, 1] == float(np.float32(math.exp(-40))) and p[0, 0, 2] == 0 and p[0, 0, 3] == 0
    one = (np.ones(1, np.float32), 0, np.ones((1, 1), np.float32), np.ones((1, 1), np.float32), np.zeros((1, 2), np.int32))
    out, stats, count = ref.vote_filter(belief, np.zeros((1, 1, 4), np.float32), one, 1.0, 0.0)
    assert np.isfinite(out[0, 0, :2]).all() and (out[0, 0, 2:] == -np.inf).all() and count.tolist() == [2, 0, 0, 2]
    assert abs(out[0, 0, 1] - out[0, 0, 0] - math.log(float(np.float32(math.exp(-40))))) < 1e-12


TAP_GEOMETRIES = [
    # extent, cell, R, (angle, tx, ty), sigma_xy, sigma_yaw, truncate
    ((16, 16), 0.25, 8, (0.3, 0.6, -0.4), 0.3, 0.9, 4.0),
    ((16, 16), 0.25, 8, (-0.3, -0.45, 0.7), 0.5, 0.8, 3.0),
    ((12, 20), 0.5, 36, (0.21, 1.3, 0.35), 1.1, 0.2, 4.0),
    ((12, 20), 0.5, 36, (-2.9, -0.8, 2.2), 2.4, 0.3, 3.0),
]


@pytest.mark.parametrize('extent,cell,R,rel,sxy,syaw,truncate', TAP_GEOMETRIES)
def test_motion_taps_moments(extent, cell, R, rel, sxy, syaw, truncate):
  grid = grids.Grid2D(extent, cell)
  tfm = geometry.Transform2D(torch.tensor(rel[0], dtype=torch.float64), torch.tensor(rel[1:], dtype=torch.float64))
  tk, lk, ta, tb, off = _np_taps(pev.motion_taps(tfm, grid, R, sxy, syaw, truncate))
  shifts = fuse_ref.shift_table([rel[0]], [rel[1:]], extent, cell, R)[0]          # float64 [R, 3]
  assert tk.dtype == np.float32 and ta.dtype == np.float32 and off.dtype == np.int32 and isinstance(lk, int)
  assert ta.shape[0] == R and tb.shape[0] == R and off.shape == (R, 2)
  for rows, first, centre, sigma, limit in ((tk[None], np.array([lk]), shifts[:1, 0], syaw * R / (2 * math.pi), 16),
                                            (ta, off[:, 0], shifts[:, 1], sxy / cell, 32),
                                            (tb, off[:, 1], shifts[:, 2], sxy / cell, 32)):
    rho = math.ceil(truncate * sigma)
    assert rows.shape[1] == 2 * rho + 2 <= limit
    assert ((rows == 0) | (rows >= ref.MIN_TAP)).all() and np.isfinite(rows).all()
    w = rows.astype(np.float64)
    j = first[:, None] + np.arange(rows.shape[1])[None]
    assert np.abs(w.sum(1) - 1).max() <= rows.shape[1] * 2.0 ** -24
    mean = (w * j).sum(1) / w.sum(1)
    assert np.abs(mean - centre).max() < 1e-6
    f = centre - np.floor(centre)
    assert (first == np.floor(centre) - rho).all()
    var = (w * (j - mean[:, None]) ** 2).sum(1) / w.sum(1)
    # the Gaussian sampled at the integers has the variance sigma^2 (sigma >= 1 index unit here: the sampling error
    # exp(-2 pi^2 sigma^2) is nothing) less its truncated tails: at most 2 int_{t sigma}^inf x^2 phi = sigma^2 (2 t
    # phi(t) + 2 (1 - Phi(t))), 2.93e-2 sigma^2 at t = 3 and 1.13e-3 sigma^2 at t = 4.  (Beyond t = 4 the outermost
    # taps fall below 2^-20 and are dropped, one side before the other: the mean then holds to ~1e-5 only.)
    assert sigma >= 1
    tail = {3.0: 2.94e-2, 4.0: 1.14e-3}[truncate] * sigma ** 2
    want = sigma ** 2 + f * (1 - f)
    assert (var <= want + 1e-6).all() and (var >= want - tail - 1e-6).all()


def test_motion_taps_without_noise_are_vote_fuses_split():
  grid = grids.Grid2D((12, 20), 0.5)
  R = 36
  for rel in ((0.21, 1.3, 0.35), (-1.234, -0.8, 2.2), (0.0, 0.0, 0.0), (2 * math.pi / 36, 0.5, -1.0)):
    tfm = geometry.Transform2D(torch.tensor(rel[0], dtype=torch.float64), torch.tensor(rel[1:], dtype=torch.float64))
    tk, lk, ta, tb, off = _np_taps(pev.motion_taps(tfm, grid, R, 0.0, 0.0))
    tab = pev.sequence_shift_table(tfm, grid, R).numpy()[0]                        # f32 [R, 3]
    assert tk.shape == (2,) and ta.shape == (R, 2) and tb.shape == (R, 2)
    for rows, first, d in ((tk[None], [lk], tab[:1, 0]), (ta, off[:, 0], tab[:, 1]), (tb, off[:, 1], tab[:, 2])):
      for row, l0, dd in zip(rows, first, d):
        l, f = fuse_ref._split(dd)
        if f < ref.MIN_TAP or 1 - f < ref.MIN_TAP:
          continue                                            # (a fraction below the smallest tap is dropped)
        assert l0 == l and abs(float(row[1]) - f) <= 2.0 ** -23 * max(1.0, abs(float(dd))) + 2.0 ** -24
        assert abs(float(row[0]) - (1 - f)) <= 2.0 ** -23 * max(1.0, abs(float(dd))) + 2.0 ** -24
  # the identity: one tap of weight exactly 1 at offset 0 on every axis
  tfm = geometry.Transform2D(torch.zeros((), dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
  tk, lk, ta, tb, off = _np_taps(pev.motion_taps(tfm, grid, R, 0.0, 0.0))
  assert tk.tolist() == [1, 0] and lk == 0 and (ta == [1, 0]).all() and (tb == [1, 0]).all() and not off.any()


def test_motion_taps_limits():
  grid = grids.Grid2D((16, 16), 0.25)
  tfm = geometry.Transform2D(torch.zeros((), dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
  pev.motion_taps(tfm, grid, 8, 15 * 0.25 / 3, 7 * (2 * math.pi / 8) / 3)       # rho = 15 and 7: the largest tables
  with pytest.raises(ValueError):
    pev.motion_taps(tfm, grid, 8, 15.1 * 0.25 / 3, 0.0)                          # rho = 16: 34 taps
  with pytest.raises(ValueError):
    pev.motion_taps(tfm, grid, 8, 0.0, 7.1 * (2 * math.pi / 8) / 3)              # rho = 8: 18 taps
  with pytest.raises(ValueError):
    pev.motion_taps(tfm, grid, 8, -1.0, 0.0)
  with pytest.raises(ValueError):
    pev.motion_taps(geometry.Transform2D(torch.zeros(2), torch.zeros(2, 2)), grid, 8, 0.1, 0.1)


@pytest.mark.parametrize('yaw,t', [(0.3, (1.0, -0.2)), (-0.3, (-0.2, 1.0))])
@pytest.mark.parametrize('i0', [(3, 14, 17), (0, 20, 9), (7, 12, 12)])
def test_the_belief_moves_the_way_the_vehicle_does(yaw, t, i0):
  """A delta belief at the pose index i0, uniform votes, a small increment: the expected index of the predicted
  belief is the index of m_t_cur = m_t_prev @ cur_t_prev^-1, within 0.51 of a bin / cell per axis (the xy tables are
  those of the output rotation, and the mass is spread over two rotations)."""
  R, H, cell = 8, 16, 0.25
  grid = grids.Grid2D((H, H), cell)
  Ho = 2 * H - 1
  cur_t_prev = geometry.Transform2D(torch.tensor(yaw, dtype=torch.float64), torch.tensor(t, dtype=torch.float64))
  taps = _np_taps(pev.motion_taps(cur_t_prev, grid, R, 0.15, 0.2))
  belief = np.full((R, Ho, Ho), -np.inf, np.float32)
  belief[i0] = 0
  out, stats, count = ref.vote_filter(belief, np.zeros((R, Ho, Ho), np.float32), taps, 1.0, 0.0)
  assert abs(stats[1] - 1) < 1e-6 and count[3] == 1
  p = np.where(np.isfinite(out), np.exp(out), 0.0)
  assert abs(p.sum() - 1) < 1e-12
  k, a, b = np.meshgrid(np.arange(R), np.arange(Ho), np.arange(Ho), indexing='ij')
  dk = (k - i0[0] + R / 2) % R - R / 2                                   # unwrapped around i0
  got = np.array([i0[0] + (p * dk).sum(), (p * a).sum(), (p * b).sum()])
  m_t_prev = fuse_ref.index_to_tfm_f64(np.array(i0, np.float64), grid, R)
  want = pev.exhaustive_tfm_to_index(m_t_prev @ cur_t_prev.inv, grid, R).numpy()
  d = got - want
  d[0] = (d[0] + R / 2) % R - R / 2
  print(f'yaw {yaw} i0 {i0}: expected index {got.round(3).tolist()}, composed {want.round(3).tolist()}')
  assert np.abs(d).max() <= 0.51
  assert np.abs((want - np.array(i0))[1:]).max() > 1.0 and abs(want[0] - i0[0]) > 0.3                         # the increment is not lost in the tolerance
  # the helper's own f32 transform agrees with the float64 one used above
  helper = pev.exhaustive_index_to_tfm(torch.tensor(i0, dtype=torch.float64), grid, R)
  assert abs(float(helper.angle) - float(m_t_prev.angle)) < 1e-6 and float((helper.t - m_t_prev.t).abs().max()) < 1e-5


def test_the_named_cases():
  cases = {c['name']: c for c in ref.all_inputs()}
  args = lambda c: (c['belief'], c['votes'], c['taps'], c['scale'], c['uniform_mix'])
  for c in cases.values():
    tk, lk, ta, tb, off = c['taps']
    for t in (tk, ta, tb):
      assert t.dtype == np.float32 and ((t == 0) | (t >= ref.MIN_TAP)).all()
    assert off.dtype == np.int32 and c['votes'].dtype == np.float32
  for name in ('wrap', 'ragged', 'bad', 'tk16', 'exact'):
    out, stats, count = ref.vote_filter(*args(cases[name]))
    fin = np.isfinite(out)
    assert abs(np.exp(out[fin]).sum() - 1) < 1e-9 and count[0] == fin.sum() and stats[3] == out[fin].max()
    b = ref.bound(*args(cases[name]))
    assert (b[fin] > 0).all() and b.max() < 1e-4, name
  # lk and lk + R (and lk - 3 R) are the same rotation pass
  a, b_, c_ = (ref.vote_filter(*args(cases[n]))[0] for n in ('wrap', 'wrap_far', 'wrap_neg'))
  same = lambda x, y: np.array_equal(x, y, equal_nan=True)
  assert cases['wrap_far']['taps'][1] == cases['wrap']['taps'][1] + 4 + 3 and not same(a, b_)
  assert cases['wrap_neg']['taps'][1] % 4 == cases['wrap_far']['taps'][1] % 4 and same(b_, c_)
  # ragged: the two rotations whose taps all fall outside receive no mass; with eps = 0 they are -inf
  out0 = ref.vote_filter(*args(cases['mix0']))[0]
  assert (out0[[5, 17]] == -np.inf).all() and np.isfinite(out0).any()
  out, stats, count = ref.vote_filter(*args(cases['ragged']))
  assert np.isfinite(out[5]).any() and stats[1] < 0.99 and 0.25 < np.mean(cases['ragged']['belief'] == -np.inf) < 0.35
  assert count[3] < np.isfinite(cases['ragged']['belief']).sum()         # some finite cells lie below the cut
  out, stats, count = ref.vote_filter(*args(cases['bad']))
  assert count[1] == 2 and count[2] == 2
  out, stats, count = ref.vote_filter(*args(cases['empty_belief']))
  assert stats[1] == 0 and stats[2] == -np.inf and count[3] == 0 and count[0] == out.size
  # the exact case: t2 and S are sums of dyadic numbers, far from any rounding
  c = cases['exact']
  p, M, _, _ = ref.masses(c['belief'])
  t2 = ref.predict(p, c['taps'])
  assert M == 0 and (t2 * 2 ** 10 == np.round(t2 * 2 ** 10)).all() and t2.sum() > 0
