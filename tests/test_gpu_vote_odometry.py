"""`-m gpu`: ``ops.vote_odometry`` (vote_odometry.hip, through the C ABI) and the host entry points built on it, against
the float64 restatement ``vote_odometry_reference``.

Both sides form the same f32 masses (up to one ulp of two correct exp implementations), multiply them exactly in float64
and round a float64 logarithm to f32 once: counts and the -inf patterns are EQUAL, and every finite log value is within
``ref.tolerance`` = 2 f32 ulps of the rounded reference + 2^-22 (derived there; the order of the float64 sums adds
< n 2^-53, far below).  Every call runs under ``guarded.scope()``: guard regions intact (outputs and workspace), no
output element left unwritten, one workspace allocation of exactly ``workspace_bytes``."""
import ctypes
import math

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_odometry_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import geometry, grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
NAMES = [c['name'] for c in ref.cases()]


def _run(c):
  """One guarded call -> (log_table, log_evidence, best, stats, count) as numpy arrays."""
  prev = torch.from_numpy(c['prev']).to(DEV)
  cur = torch.from_numpy(c['cur']).to(DEV)
  sh = None if c['shifts'] is None else torch.from_numpy(np.ascontiguousarray(c['shifts'], dtype=np.int32)).to(DEV)
  R, Ho, Wo = c['prev'].shape
  Kr, S, U = c['Kr'], c['S'], 0 if sh is None else sh.shape[0]
  with guarded.scope() as sc:
    shp = None if sh is None else guarded.place(sh, 'address')
    out = ops.vote_odometry(guarded.place(prev, 'value'), guarded.place(cur, 'value'), Kr, S, shp, c['scale_prev'],
                            c['scale_cur'])
    shapes = [(2 * Kr + 1, R, 2 * S + 1, 2 * S + 1), (U,), (1,), (4,), (6,)]
    # (the poison is all-ones: a NaN no kernel writes, and -1, which no count is; -1 IS best's value without a finite
    # candidate, so best is checked against the kernel's own log_evidence instead, exactly)
    for t, shape in zip(out, shapes):
      assert tuple(t.shape) == shape and (t is out[2] or not bool(guarded.unwritten(t).any()))
    ws = [a for a in sc.allocations('vote_odometry') if a.dtype == torch.int64]
    assert len(ws) == 1 and ws[0].numel() * 8 == _lib.load().snap_vote_odometry_workspace_bytes(R, Ho, Wo, Kr, S, U)
    res = [t.cpu().numpy() for t in out]
  return res


def _assert_logs(got, want64, what):
  want = ref.round_log(want64)
  assert got.dtype == np.float32 and got.shape == want.shape, what
  assert not np.isnan(got).any() and not np.isposinf(got).any(), what
  assert (np.isneginf(got) == np.isneginf(want)).all(), f'{what}: -inf patterns'
  live = np.isfinite(want)
  if not live.any():
    return
  err = np.abs(got[live].astype(np.float64) - want[live].astype(np.float64))
  tol = ref.tolerance(want[live])
  print(f'{what}: worst error / tolerance {float(np.max(err / tol)):.4f}, worst error {float(err.max()):.3e}')
  assert (err <= tol).all(), f'{what}: {got[live][err > tol][:8]} vs {want[live][err > tol][:8]}'


def _assert_case(got, c, want, what):
  log_table, log_evidence, best, stats, count = got
  assert (count == want['count']).all(), f'{what}: count {count} != {want["count"]}'
  _assert_logs(log_table, want['log_table'], f'{what} log_table')
  _assert_logs(log_evidence, want['log_evidence'], f'{what} log_evidence')
  _assert_logs(stats, want['stats'], f'{what} stats')
  # best: exactly the first arg-max of the kernel's OWN log_evidence ...
  fin = np.isfinite(log_evidence)
  own = int(np.argmax(np.where(fin, log_evidence, -np.inf))) if fin.any() else -1
  assert int(best[0]) == own, f'{what}: best {best} vs own {own}'
  if own >= 0:
    assert stats[3].view(np.int32) == log_evidence[own].view(np.int32)
  # ... and the reference's where the reference decides it by more than four tolerances
  if want['best'] >= 0:
    tol = float(ref.tolerance(ref.round_log(want['log_evidence'])[want['best']]))
    if c['planted'] is not None:
      assert want['best'] == c['planted'] and ref.runner_up_margin(want) > 4 * tol, what   # decided on the reference
    if ref.runner_up_margin(want) > 4 * tol:
      assert own == want['best'], f'{what}: best {own} vs the reference {want["best"]}'
  else:
    assert own == -1


@pytest.mark.parametrize('name', NAMES)
def test_against_the_float64_reference(name):
  c, want = ref.shared()[name]
  got = _run(c)
  _assert_case(got, c, want, name)
  if name == 'all_masked':
    assert np.isneginf(got[0]).all() and np.isneginf(got[1]).all() and got[2][0] == -1 and np.isneginf(got[3]).all()
    assert got[4].tolist() == [0, 0, 0, 0, 0, 0]
  if name == 'no_candidates':
    assert got[1].shape == (0,) and got[2][0] == -1 and np.isneginf(got[3][2:]).all() and got[4][4:].tolist() == [0, 0]
  if name == 'ragged':
    assert got[4][1] == 3 and got[4][3] == 2 and got[4][4] == 4
  if name == 'minimal':
    assert got[0].tolist() == [[[[0.0]]]] and got[1].tolist() == [0.0] and got[3].tolist() == [0.25, -3.0, 0.0, 0.0]
  # a second call gives identical bytes
  again = _run(c)
  for a, b in zip(got, again):
    assert a.tobytes() == b.tobytes(), name


def test_raw_abi_refusals_launch_nothing():
  lib = _lib.load()
  R, Ho, Wo, Kr, S, U = 4, 6, 7, 1, 2, 3
  need = lib.snap_vote_odometry_workspace_bytes(R, Ho, Wo, Kr, S, U)
  assert need > 0 and need % 8 == 0
  for bad in ((0, Ho, Wo, 0, S, U), (65, Ho, Wo, Kr, S, U), (R, 0, Wo, Kr, S, U), (R, Ho, Wo, 2, S, U),
              (R, Ho, Wo, -1, S, U), (R, Ho, Wo, Kr, 33, U), (R, Ho, Wo, Kr, -1, U), (R, Ho, Wo, Kr, S, -1),
              (64, 8192, 8192, Kr, S, U)):
    assert lib.snap_vote_odometry_workspace_bytes(*bad) == 0, bad
  assert lib.snap_vote_odometry_workspace_bytes(1, 1, 1, 0, 0, 0) > 0
  vol = torch.zeros((R, Ho, Wo), device=DEV)
  sh = torch.zeros((U, R, 3), dtype=torch.int32, device=DEV)
  W = 2 * S + 1
  outs = [torch.full((2 * Kr + 1, R, W, W), 7.0, device=DEV), torch.full((U,), 7.0, device=DEV),
          torch.full((1,), 7, dtype=torch.int32, device=DEV), torch.full((4,), 7.0, device=DEV),
          torch.full((6,), 7, dtype=torch.int32, device=DEV)]
  ws = torch.zeros((need // 8,), dtype=torch.int64, device=DEV)
  p = lambda t: ctypes.c_void_p(t.data_ptr())

  def call(prev=vol, shifts=sh, kr=Kr, s=S, scale=1.0, nbytes=need, wsp=None):
    return lib.snap_vote_odometry_f32(None if prev is None else p(prev), p(vol), scale, 1.0,
                                      None if shifts is None else p(shifts), R, Ho, Wo, kr, s, U, p(outs[0]),
                                      p(outs[1]), p(outs[2]), p(outs[3]), p(outs[4]),
                                      ctypes.c_void_p(ws.data_ptr() + (4 if wsp else 0)), nbytes, None)

  assert call(prev=None) == -3 and call(shifts=None) == -3
  assert call(kr=2) == -1 and call(s=33) == -1
  assert call(scale=0.0) == -2 and call(scale=float('inf')) == -2 and call(scale=float('nan')) == -2
  assert call(nbytes=need - 1) == -5 and call(wsp=True) == -5
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in outs) and not bool(ws.any())
  assert call() == 0
  torch.cuda.synchronize()
  assert not any(bool((t == 7).all()) for t in outs)


# ------------------------------- the host entry points --------------------------------------------
H, R = 12, 8                                                 # volumes [8, 23, 23], cells of 0.5 m, bins of 45 degrees
LATTICE = dict(range_xy=1.0, range_yaw=2 * math.pi / R)      # 3 x 5 x 5 candidates


def _grid():
  return grids.Grid2D((H, H), 0.5)


def _two_peak_volume(seed, peaks=((0, 9, 12, 12.0), (2, 14, 8, 9.0))):
  """N(0, 1) noise plus two Gaussian bumps, at rotations 0 and 90 degrees: there every lattice candidate's shift is a
  whole number of cells before rounding, so two candidates a cell apart never share a row at both peaks."""
  rng = np.random.default_rng(seed)
  n = 2 * H - 1
  v = rng.normal(0.0, 1.0, (R, n, n))
  a, b = np.mgrid[0:n, 0:n]
  for r0, a0, b0, height in peaks:
    v[r0] += height * np.exp(-((a - a0) ** 2 + (b - b0) ** 2) / (2 * 1.5 ** 2))
  return torch.from_numpy(v.astype(np.float32)).to(DEV)


def _transport(prev, shifts_row):
  """``ops.vote_fuse``'s own integer shift: cur[r, a, b] = prev[r + dk, a + da(r), b + db(r)] (-inf outside)."""
  sh = shifts_row.to(torch.float32).clone()
  sh[:, 0] = torch.remainder(sh[:, 0], R)
  return ops.vote_fuse(prev[None].contiguous(), sh[None].contiguous().to(DEV))[0]


def test_increment_from_votes_recovers_a_planted_motion():
  grid = _grid()
  cand, shifts, Kr, S = pev.increment_lattice(grid, R, **LATTICE)
  assert tuple(shifts.shape) == (75, R, 3) and Kr == 1
  prev = _two_peak_volume(11)
  for true in (2 * 25 + 3 * 5 + 0, 0 * 25 + 1 * 5 + 4, 37):   # (+1 bin, +0.5 m, -1 m), (-1 bin, -0.5 m, +1 m), none
    cur = _transport(prev, shifts[true])
    with guarded.scope():
      out = pev.increment_from_votes(prev, cur, grid, R, **LATTICE)
    assert set(out) == {'log_evidence', 'log_posterior', 'index', 'cur_t_prev', 'mean', 'cov', 'candidates', 'shifts',
                        'log_table', 'count', 'stats'}
    want = ref.vote_odometry(prev.cpu().numpy(), cur.cpu().numpy(), Kr, S, shifts.numpy())
    tol = float(ref.tolerance(ref.round_log(want['log_evidence'])[want['best']]))
    assert want['best'] == true and ref.runner_up_margin(want) > 4 * tol         # decided on the reference
    _assert_logs(out['log_evidence'].cpu().numpy(), want['log_evidence'], f'planted {true}')
    assert out['index'] == true
    assert float(out['cur_t_prev'].angle) == float(cand.angle[true]) and (out['cur_t_prev'].t == cand.t[true]).all()
    lp = out['log_posterior'].cpu()
    assert lp.dtype == torch.float64 and abs(float(torch.logsumexp(lp, 0))) < 1e-12 and int(lp.argmax()) == true
    mean, cov = out['mean'], out['cov']
    assert abs(float(mean[0] - cand.angle[true])) <= 2 * math.pi / R and (mean[1:] - cand.t[true]).abs().max() <= 0.5
    assert tuple(cov.shape) == (3, 3) and torch.allclose(cov, cov.T) and bool((torch.linalg.eigvalsh(cov) > -1e-12).all())
    # explicit candidates give the same bytes; a prior far from the truth moves the MAP, one on it does not
    same = pev.increment_from_votes(prev, cur, grid, R, candidates=cand)
    assert guarded.same_bits(same['log_evidence'], out['log_evidence']) and same['index'] == true
    kept = pev.increment_from_votes(prev, cur, grid, R, prior=(cand[true], 0.5, 0.5), **LATTICE)
    assert kept['index'] == true and guarded.same_bits(kept['log_evidence'], out['log_evidence'])
    other = (true + 30) % 75
    moved = pev.increment_from_votes(prev, cur, grid, R, prior=(cand[other], 1e-3, 1e-3), **LATTICE)
    assert moved['index'] == other


def test_step_estimated_reproduces_the_filter_given_the_true_increments():
  grid = _grid()
  cand, shifts, _, _ = pev.increment_lattice(grid, R, **LATTICE)
  true = [None, 2 * 25 + 3 * 5 + 1, 1 * 25 + 0 * 5 + 3]
  frames = [_two_peak_volume(12)]
  for t in true[1:]:
    frames.append(_transport(frames[-1], shifts[t]))
  kw = dict(sigma_xy=0.3, sigma_yaw=0.2, temperature=1.5)
  given, estimated = pev.VoteFilter(grid, R, **kw), pev.VoteFilter(grid, R, **kw)
  with pytest.raises(ValueError):
    estimated.estimate_increment(frames[0], **LATTICE)
  for n, (votes, t) in enumerate(zip(frames, true)):
    a = given.step(votes, None if t is None else cand[t])
    with guarded.scope():
      b = estimated.step_estimated(votes, **LATTICE)
    assert set(b) == set(a) | {'increment'}
    assert (b['increment'] is None) == (n == 0)
    if n:
      assert b['increment']['index'] == t, f'frame {n}: {b["increment"]["index"]} vs {t}'
    for k in a:
      assert guarded.same_bits(a[k], b[k]), f'frame {n}: {k}'
  assert guarded.same_bits(given.belief, estimated.belief)


def test_estimate_increments_feeds_fuse_votes():
  grid = _grid()
  cand, shifts, _, _ = pev.increment_lattice(grid, R, **LATTICE)
  true = [None, 1 * 25 + 4 * 5 + 1, 1 * 25 + 1 * 5 + 4]      # translations: (+1 m, -0.5 m), (-0.5 m, +1 m)
  frames = [_two_peak_volume(13)]
  for t in true[1:]:
    frames.append(_transport(frames[-1], shifts[t]))
  with guarded.scope():
    increments, q0_t_q, steps = pev.estimate_increments(frames, grid, R, details=True, **LATTICE)
  assert increments[0] is None and steps[0] is None and len(increments) == 3 and tuple(q0_t_q.shape) == (3,)
  for n in (1, 2):
    assert steps[n]['index'] == true[n]
    assert float(increments[n].angle) == float(cand.angle[true[n]]) and (increments[n].t == cand.t[true[n]]).all()
  assert float(q0_t_q.angle[0]) == 0 and (q0_t_q.t[0] == 0).all()
  want_t = -(cand.t[true[1]] + cand.t[true[2]])
  assert torch.allclose(q0_t_q.t[2], want_t, atol=1e-12) and float(q0_t_q.angle[2]) == 0
  fused, count = pev.fuse_votes(frames, q0_t_q, grid, R)
  flat = int(torch.where(torch.isfinite(fused), fused, torch.full_like(fused, -math.inf)).argmax())
  n = 2 * H - 1
  assert (flat // (n * n), flat // n % n, flat % n) == (0, 9, 12), 'the fused arg-max is the planted pose'
  # the list is what the track operators take
  track = pev.viterbi_track(frames, increments, grid, R, 0.3, 0.2)
  assert track is not None


def test_validation_errors_launch_nothing():
  grid = _grid()
  prev = _two_peak_volume(14)
  with guarded.scope() as sc:
    with pytest.raises(ValueError):
      ops.vote_odometry(prev, prev, 0, 33)
    with pytest.raises(ValueError):
      ops.vote_odometry(prev, prev, 4, 1)                    # 2 Kr + 1 > R = 8
    with pytest.raises(ValueError):
      ops.vote_odometry(prev, prev[:, :-1].contiguous(), 1, 1)
    with pytest.raises(ValueError):
      ops.vote_odometry(prev, prev, 1, 1, torch.zeros((3, R + 1, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
      ops.vote_odometry(prev, prev, 1, 1, scale_cur=0.0)
    with pytest.raises(ValueError):
      pev.increment_from_votes(prev, prev[:4].contiguous(), grid, R, **LATTICE)
    with pytest.raises(ValueError):
      pev.increment_from_votes(prev, prev, grid, R, range_xy=17.0, range_yaw=0.0)     # S = 34 cells
    with pytest.raises(ValueError):
      pev.increment_from_votes(prev, prev, grid, R, range_xy=0.0, range_yaw=math.pi)   # 2 Kr + 1 > R
    with pytest.raises(ValueError):
      pev.VoteFilter(grid, R, 0.3, 0.2).estimate_increment(prev, **LATTICE)
    assert not sc.allocations('vote_odometry')
  with pytest.raises(RuntimeError):
    ops.vote_odometry(prev.cpu(), prev.cpu(), 1, 1)
