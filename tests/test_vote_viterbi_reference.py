"""The numpy f32 restatement of ``snap_vote_viterbi_f32`` (``vote_viterbi_reference``) against checks that share none
of its structure, and the host pieces of the feature that need no GPU: the log-tap tables, the binding's signatures
and the argument validation of ``viterbi_track`` / ``VoteViterbi``."""
import itertools

import numpy as np
import pytest
import torch

import vote_filter_reference as flt
import vote_smooth_reference as smo
import vote_viterbi_reference as ref
from snap_amd import _lib
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import geometry, grids

SMALL = [c for c in ref.all_inputs() if c['votes'].size <= 40000]


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize('c', SMALL, ids=lambda c: c['name'])
def test_passes_equal_the_joint_maximum_and_back_attains_it(c):
  w = ref.walk(c['score_prev'], c['votes'], c['ltaps'], c['scale'], c['log_stay'], c['log_jump'])
  score, back = w['score'], w['back']
  if c['score_prev'] is None:
    assert (back == -1).all() and w['count'][4] == -1 and w['stats'][0] == -np.inf
    assert ((score == -np.inf) == ~np.isfinite(c['votes'])).all()
    return
  assert ((back == -1) == (score == -np.inf)).all()
  assert (_bits(ref.brute_force(w['d'], c['ltaps'])) == _bits(w['m2'])).all()
  # every finite cell: the score is the contract's expression of the predecessor `back` names
  ls, lj = np.float32(c['log_stay']), np.float32(c['log_jump'])
  flat, jumped, sv = score.reshape(-1), w['jumped'].reshape(-1), w['sv'].reshape(-1)
  cells = np.flatnonzero(back.reshape(-1) >= 0)
  rng = np.random.default_rng(3)
  for x in (cells if len(cells) <= 600 else rng.choice(cells, 600, replace=False)):
    y = int(back.reshape(-1)[x])
    if jumped[x]:
      assert y == w['J'] and _bits(flat[x]) == _bits(np.float32(sv[x] + lj))
    else:
      value = ref.path_value(w['d'], c['ltaps'], x, y)
      assert value > -np.inf and _bits(value) == _bits(w['m2'].reshape(-1)[x])
      assert _bits(flat[x]) == _bits(np.float32(sv[x] + np.float32(ls + value)))
      assert np.float32(ls + value) >= (lj if w['J'] >= 0 else -np.inf)


def test_named_cases_hit_what_they_are_named_for():
  cases = {c['name']: c for c in ref.all_inputs()}
  run = lambda c: ref.walk(c['score_prev'], c['votes'], c['ltaps'], c['scale'], c['log_stay'], c['log_jump'])
  w = run(cases['ties'])
  n = w['score'].size
  assert (w['back'].reshape(-1) == np.arange(n)).all() and w['count'].tolist() == [n, 0, 0, 0, 0, 0]
  w = run(cases['jump_only'])
  assert (w['back'] == w['J']).all() and w['count'][3] == n_cells(w)
  w = run(cases['no_jump_outside'])
  assert (w['score'] == -np.inf).all() and (w['back'] == -1).all() and w['count'][5] == -1 and w['count'][4] >= 0
  w = run(cases['stay_off'])
  assert w['count'][3] == w['count'][0] > 0
  w = run(cases['bad'])
  assert w['count'][1] == 2 and w['count'][2] == 2
  w = run(cases['empty'])
  assert w['count'].tolist() == [0, 0, 0, 0, -1, -1]
  assert any(np.isneginf(t).any() for t in cases['ragged']['ltaps'][2:4])


def n_cells(w):
  return int(np.isfinite(w['score']).sum())


@pytest.mark.parametrize('eps', [0.0, 0.05])
def test_the_traced_path_is_the_best_of_all_paths(eps):
  """R = 2, Ho = 2, Wo = 3, three frames: 12^3 paths, each scored with the contract's own f32 expressions."""
  votes, ltaps = ref.tiny_track()
  scale = 1.5
  steps = ref.track(votes, ltaps, scale, eps)
  linear, jumps, total = ref.trace(steps)
  n = votes[0].size
  scores = {p: ref.path_score(p, votes, ltaps, steps, scale, eps) for p in itertools.product(range(n), repeat=3)}
  best = max(scores.values())
  assert np.isfinite(best)
  assert _bits(scores[tuple(int(i) for i in linear)]) == _bits(best) == _bits(steps[-1]['stats'][1])
  # ... and per end cell: the recursion's score is the best path into that cell
  for x in range(n):
    into = max(s for p, s in scores.items() if p[-1] == x)
    assert _bits(into) == _bits(steps[-1]['score'].reshape(-1)[x])
  assert total == float(best) + sum(float(s['M']) for s in steps[1:])
  if eps == 0.0:
    assert not jumps.any()


def test_marginal_argmaxes_can_be_an_impossible_track_and_the_viterbi_path_is_not():
  """Why the feature exists.  One row of six cells, two frames, eps = 0; a pose stays or moves one cell down (column
  taps 1/2, 1/2 at offsets 0, +1).  Frame 0 likes cell 5 (0.4) over cells 1 (0.32) and 2 (0.28); frame 1 likes cell 1
  (1.0) over cells 4 and 5 (0.45).  The smoothed marginals peak at cell 5 in frame 0 (0.18 against 0.16 and 0.14 of
  the joint mass) and at cell 1 in frame 1 (0.30 against 0.09): a step from 5 to 1, which has probability zero."""
  with np.errstate(divide='ignore'):
    v0 = np.log(np.array([0, 0.32, 0.28, 0, 0, 0.4])).astype(np.float32).reshape(1, 1, 6)
    v1 = np.log(np.array([0, 1.0, 0, 0, 0.45, 0.45])).astype(np.float32).reshape(1, 1, 6)
  one = np.ones((1, 1), np.float32)
  taps = (np.ones(1, np.float32), 0, one, np.array([[0.5, 0.5]], np.float32), np.zeros((1, 2), np.int32))
  b0 = flt.vote_filter(None, v0, smo.still_taps(1), 1.0, 0.0)[0].astype(np.float32)
  b1 = flt.vote_filter(b0, v1, taps, 1.0, 0.0)[0].astype(np.float32)
  smoothed = smo.smooth_track([b0, b1], [None, taps], 0.0)
  x0, x1 = (int(np.argmax(np.asarray(s).reshape(-1))) for s in smoothed)
  assert (x0, x1) == (5, 1)
  possible = lambda prev, cur: prev in (cur, cur + 1)       # the source of cell b is b or b + 1
  assert not possible(x0, x1)
  steps = ref.track([v0, v1], [None, ref.log_taps(taps)], 1.0, 0.0)
  linear, jumps, _ = ref.trace(steps)
  assert linear.tolist() == [1, 1] and possible(*linear.tolist()) and not jumps.any()


def test_motion_log_taps_are_the_logs_of_motion_taps():
  grid = grids.Grid2D((16, 16), 0.25)
  inc = geometry.Transform2D(torch.tensor(0.12, dtype=torch.float64), torch.tensor([0.3, -0.2], dtype=torch.float64))
  zeros = 0
  # (no motion with sigma = 0: the taps are (1, 0) on every axis, so -inf log-taps occur)
  for inc, sigma_xy, sigma_yaw in ((inc, 0.2, 0.15), (inc, 0.0, 0.0), (inc, 0.6, 0.4), (pev._no_motion(), 0.0, 0.0)):
    taps = pev.motion_taps(inc, grid, 8, sigma_xy, sigma_yaw, device='cpu')
    logs = pev.motion_log_taps(inc, grid, 8, sigma_xy, sigma_yaw, device='cpu')
    assert logs[1] == taps[1] and torch.equal(logs[4], taps[4]) and logs[4].dtype == torch.int32
    for w, lw in zip((taps[0], taps[2], taps[3]), (logs[0], logs[2], logs[3])):
      w, lw = w.numpy(), lw.numpy()
      assert lw.dtype == np.float32 and lw.shape == w.shape
      with np.errstate(divide='ignore'):
        want = np.log(w.astype(np.float64)).astype(np.float32)
      assert (_bits(lw) == _bits(want)).all() and ((lw == -np.inf) == (w == 0)).all() and (lw <= 0).all()
      zeros += int((w == 0).sum())
  assert zeros > 0
  still = pev._still_log_taps(8, 'cpu')
  assert [tuple(t.shape) for t in (still[0], still[2], still[3], still[4])] == [(1,), (8, 1), (8, 1), (8, 2)]
  assert still[1] == 0 and all(float(t.abs().max()) == 0 for t in (still[0], still[2], still[3], still[4]))


def test_the_binding_declares_the_new_symbols():
  sig = _lib.SIGNATURES
  assert len(sig['snap_vote_viterbi_workspace_bytes'][1]) == 6
  assert len(sig['snap_vote_viterbi_f32'][1]) == 23 and len(sig['snap_vote_backstep_i32'][1]) == 6


def test_track_arguments_are_validated():
  grid = grids.Grid2D((4, 4), 0.25)
  v = torch.zeros((4, 7, 7))
  kw = dict(sigma_xy=0.2, sigma_yaw=0.1)
  with pytest.raises(ValueError):
    pev.viterbi_track([v, v], [None], grid, 4, **kw)
  with pytest.raises(ValueError):
    pev.viterbi_track([], [], grid, 4, **kw)
  with pytest.raises(ValueError):
    pev.viterbi_track([v, torch.zeros((4, 7, 6))], [None, None], grid, 4, **kw)
  with pytest.raises(ValueError):
    pev.viterbi_track([v[0]], [None], grid, 4, **kw)
  with pytest.raises(ValueError):
    pev.viterbi_track([v], [None], grid, 5, **kw)
  with pytest.raises(ValueError):
    pev.VoteViterbi(grid, 4, uniform_mix=1.5, **kw)
  track = pev.VoteViterbi(grid, 4, **kw)
  assert track.score is None and track.history == []
  with pytest.raises(ValueError):
    track.path()
  with pytest.raises(ValueError):
    track.step(v[0])
  with pytest.raises(ValueError):
    track.step(torch.zeros((5, 7, 7)))
