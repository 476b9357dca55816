"""`-m gpu`: ``ops.vote_filter`` (vote_filter.hip, through the C ABI) and the host entry points built on it, against the
float64 numpy restatement ``vote_filter_reference`` within twice its derived rounding bound; ``count`` exactly, the NaN
and -inf cells identical, ``stats`` within twice its own derived bound.

Every launch tiles each rotation's pixels p = a * Wo + b into runs of 256, one workgroup per tile up to 2048
workgroups, which then stride over the tiles.  ``tiny`` [1, 1, 1]: one tap per axis; ``wrap`` / ``wrap_far`` /
``wrap_neg`` [4, 7, 7]: Tk = 3 with lk = -1, R + 2 and -3 R - 2 (one partial tile per rotation); ``ragged``
[36, 31, 33]: four tiles per rotation, the last ragged, Tk = 4, Ta = 8, Tb = 6 with zero taps, offsets of both signs,
two rotations whose taps all fall outside, 30 % -inf in the belief, the border mask in the votes; ``mix0`` / ``mix1``:
eps = 0 and 1 on the same data (``ragged`` is eps = 1e-3); ``start``: belief = None; ``bad``: a NaN and a +inf belief
cell, a NaN and a +inf vote; ``wide`` [2, 20, 300] Ta = 1, Tb = 32 and ``tall`` [2, 300, 20] Ta = 32, Tb = 1: the
widest tables, rows that span workgroups; ``tk16`` [5, 6, 9]: Tk = 16 > R; ``empty_belief``: no finite belief cell.
The boundary of this tiling: ``tiles`` [2, 520, 520]: 2114 tiles on 2048 workgroups (every launch strides, and every
fold of the per-workgroup partials has more entries than one pass of its 256 threads).  Every call runs under
``guarded.scope()``: guard regions intact (outputs and workspace), no output element left unwritten, the workspace the
size ``snap_vote_filter_workspace_bytes`` states.

Observed on an MI355X (each case prints its figures), largest err / bound: ``tiny`` 0.00, ``wrap`` 0.27, ``wrap_far`` /
``wrap_neg`` 0.27, ``ragged`` 0.29, ``mix0`` 0.30 (2.0e-6 against 7.7e-6), ``bad`` 0.29, ``wide`` 0.18, ``tall`` 0.18,
``tk16`` 0.15, ``tiles`` 0.26, ``exact`` 0.09; the localize frames with a predict step 0.11.  Where the prior is
uniform the bound is the final f32 rounding alone (2^-24 |belief_out|, the most a rounding to nearest can be off) and
the ratio is close to 1 by construction: ``mix1`` / ``start`` 0.91, ``empty_belief`` 0.98, the first localize frame
0.98.  ``stats``: ``log_z`` at most 0.59 of its bound (the first localize frame, where the bound is float64 noise
and the f32 rounding alone; below 0.01 with a predict step), ``mass_kept`` 0.07, the largest belief_out 0.17.
Cross-checks: ``vote_fuse`` 0.09, ``vote_posterior`` 0.18 of the summed bounds.  2 x the bound is allowed."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_filter_reference as ref
import vote_fuse_reference as fuse_ref
import vote_posterior_reference as post_ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import geometry, grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE

@functools.lru_cache(maxsize=None)
def _inputs():
  return {c['name']: c for c in ref.all_inputs()}


def _args(c):
  return c['belief'], c['votes'], c['taps'], c['scale'], c['uniform_mix']


@functools.lru_cache(maxsize=None)
def _want(name):
  c = _inputs()[name]
  return ref.vote_filter(*_args(c)), ref.bound(*_args(c)), ref.stats_bound(*_args(c))


def _dev(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_taps(taps, place=False):
  tk, lk, ta, tb, off = taps
  put = (lambda t, kind: guarded.place(t, kind)) if place else (lambda t, kind: t)
  return (put(_dev(tk), 'value'), int(lk), put(_dev(ta), 'value'), put(_dev(tb), 'value'), put(_dev(off), 'address'))


def _run(belief, votes, taps, scale=1.0, uniform_mix=0.0):
  """One guarded call -> numpy (belief_out, stats, count)."""
  R, Ho, Wo = votes.shape
  with guarded.scope() as sc:
    b = None if belief is None else guarded.place(_dev(belief), 'value')
    out = ops.vote_filter(b, guarded.place(_dev(votes), 'value'), _dev_taps(taps, place=True), scale, uniform_mix)
    assert [tuple(o.shape) for o in out] == [(R, Ho, Wo), (4,), (4,)]
    assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.int32]
    ws = [a for a in sc.allocations('vote_filter') if a.dtype == torch.int64]
    need = _lib.load().snap_vote_filter_workspace_bytes(R, Ho, Wo, len(taps[0]), taps[2].shape[1], taps[3].shape[1])
    assert len(ws) == 1 and ws[0].numel() * 8 == need
    for o, what in zip(out, ('belief_out', 'stats', 'count')):   # (the kernel's NaN is 0x7fc00000, not the poison)
      assert not bool(guarded.unwritten(o).any()), f'{what}: elements never written'
    res = tuple(o.cpu().numpy() for o in out)
  return res


def _assert_within(got, want, tol, stol, what, factor=2.0):
  (g, gs, gc), (w, ws, wc) = got, want
  assert gc.tolist() == wc.tolist(), f'{what}: count {gc.tolist()} != {wc.tolist()}'
  assert (np.isnan(g) == np.isnan(w)).all(), f'{what}: NaN cells differ'
  assert ((g == -np.inf) == (w == -np.inf)).all(), f'{what}: -inf cells differ'
  fin = np.isfinite(w)
  err = np.abs(g[fin].astype(np.float64) - w[fin])
  if fin.any():
    print(f'{what}: max err {err.max():.3e}, max bound {tol[fin].max():.3e}, '
          f'max err / bound {np.max(err / np.maximum(tol[fin], 1e-300)):.3f}')
  bad = ~(err <= factor * tol[fin])
  assert not bad.any(), f'{what}: {int(bad.sum())} cells outside {factor} x bound'
  for i, name in enumerate(('log_z', 'mass_kept', 'peak', 'top')):
    if np.isfinite(ws[i]):
      e = abs(float(gs[i]) - ws[i])
      print(f'{what}: stats {name} err {e:.3e}, bound {stol[i]:.3e}')
      assert e <= factor * stol[i], f'{what}: stats[{i}] {gs[i]} against {ws[i]}'
    else:
      assert float(gs[i]) == ws[i], f'{what}: stats[{i}] {gs[i]} against {ws[i]}'
  # normalisation: float64 sum of exp over the finite cells is 1 within max |belief_out| 2^-23
  if fin.any():
    gf = g[np.isfinite(g)].astype(np.float64)
    total = np.exp(gf).sum()
    print(f'{what}: sum exp(belief_out) - 1 = {total - 1:.3e}')
    assert abs(total - 1) <= np.abs(gf).max() * 2.0 ** -23


CASES = ['tiny', 'wrap', 'wrap_far', 'wrap_neg', 'ragged', 'mix0', 'mix1', 'start', 'bad', 'wide', 'tall', 'tk16',
         'tiles', 'empty_belief', 'exact']


@pytest.mark.parametrize('name', CASES)
def test_against_the_reference(name):
  c = _inputs()[name]
  want, tol, stol = _want(name)
  _assert_within(_run(*_args(c)), want, tol, stol, name)


def test_nothing_finite_gives_minus_infinity_everywhere():
  c = _inputs()['wrap']
  votes = np.full(c['votes'].shape, -np.inf, np.float32)
  g, gs, gc = _run(c['belief'], votes, c['taps'], 1.0, 1e-3)
  assert (g == -np.inf).all() and gs[0] == -np.inf and gs[3] == -np.inf and gc.tolist()[:3] == [0, 0, 0]
  assert gc[3] == ref.masses(c['belief'])[3] and abs(gs[1] - ref.vote_filter(*_args(c))[1][1]) < 1e-5


def test_integer_shifts_agree_with_vote_fuse():
  """sigma = 0 taps with integer shifts, eps = 0, scale = 1: belief_out + log_z is vote_fuse([votes, belief]) with the
  belief read at the shifted cell, up to the constants of the normalisation: log(prior) = (belief - M) - log(S) where
  the mass is kept.  The -inf mask is identical; values agree within the sum of both bounds."""
  rng = np.random.default_rng(11)
  R, Ho, Wo = 6, 17, 19
  belief = (rng.standard_normal((R, Ho, Wo)) * 2 - 9).astype(np.float32)     # every cell within the cut of the peak
  belief[rng.random((R, Ho, Wo)) < 0.2] = -np.inf
  votes = rng.standard_normal((R, Ho, Wo)).astype(np.float32)
  votes[rng.random((R, Ho, Wo)) < 0.1] = -np.inf
  shifts = np.zeros((2, R, 3), np.float32)
  shifts[1, :, 0] = 2
  shifts[1, :, 1:] = rng.integers(-3, 4, (R, 2))
  taps = (np.array([1, 0], np.float32), 2, np.tile(np.array([1, 0], np.float32), (R, 1)),
          np.tile(np.array([1, 0], np.float32), (R, 1)), shifts[1, :, 1:].astype(np.int32))
  g, gs, gc = _run(belief, votes, taps, 1.0, 0.0)
  vol = np.stack([votes, belief])
  with guarded.scope():
    fused, _ = ops.vote_fuse(_dev(vol), _dev(shifts))
  fused = fused.cpu().numpy()
  assert ((g == -np.inf) == (fused == -np.inf)).all() and np.isfinite(g).any() and (fused == -np.inf).any()
  fin = np.isfinite(fused)
  # belief_out + log_z = votes + (belief' - M) - log S, S = sum of the transported masses (float64, from the masses)
  p, M, _, _ = ref.masses(belief)
  S = ref.predict(p, taps).sum()
  lhs = g[fin].astype(np.float64) + float(gs[0])
  rhs = fused[fin].astype(np.float64) - float(M) - math.log(S)
  tol = (ref.bound(belief, votes, taps, 1.0, 0.0)[fin] + ref.stats_bound(belief, votes, taps, 1.0, 0.0)[0]
         + fuse_ref.bound(vol, shifts)[fin]
         # log p = belief' - M up to the rounding of the f32 subtraction and of exp to f32
         + 2.0 ** -24 * (np.abs(belief[np.isfinite(belief)]).max() + abs(float(M))) + 2.0 ** -23)
  err = np.abs(lhs - rhs)
  print(f'vote_fuse cross-check: max err {err.max():.3e}, max err / bound {np.max(err / tol):.3f}')
  assert (err <= tol).all()


def test_uniform_mix_one_agrees_with_vote_posterior():
  """eps = 1: belief_out = scale * votes - log_z_V and stats[0] = log_z_V - log(n), log_z_V from ops.vote_posterior."""
  c = _inputs()['ragged']
  votes, scale = c['votes'], c['scale']
  g, gs, gc = _run(c['belief'], votes, c['taps'], scale, 1.0)
  with guarded.scope():
    post = ops.vote_posterior(_dev(votes), scale)
  lz = float(post[2][0])
  fin = np.isfinite(votes)
  assert (np.isfinite(g) == fin).all() and gc[0] == int(post[3][0])
  lz_tol = post_ref.bound(votes, scale)[2][0]                              # vote_posterior's own bound of its log_z
  x = float(np.float32(scale)) * votes[fin].astype(np.float64)
  tol = ref.bound(c['belief'], votes, c['taps'], scale, 1.0)[fin] + lz_tol
  err = np.abs(g[fin].astype(np.float64) - (x - lz))
  print(f'vote_posterior cross-check: max err {err.max():.3e}, max err / bound {np.max(err / tol):.3f}')
  assert (err <= tol).all()
  e0 = abs(float(gs[0]) - (lz - math.log(votes.size)))
  assert e0 <= ref.stats_bound(c['belief'], votes, c['taps'], scale, 1.0)[0] + lz_tol + 2.0 ** -23 * abs(float(gs[0]))


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for name in ('ragged', 'bad', 'tiles', 'start'):
    c = _inputs()[name]
    belief, votes, taps = _dev(c['belief']), _dev(c['votes']), _dev_taps(c['taps'])
    first = ops.vote_filter(belief, votes, taps, c['scale'], c['uniform_mix'])
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_filter(belief, votes, taps, c['scale'], c['uniform_mix'])
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    R, Ho, Wo = votes.shape
    Tk, Ta, Tb = taps[0].shape[0], taps[2].shape[1], taps[3].shape[1]
    nbytes = lib.snap_vote_filter_workspace_bytes(R, Ho, Wo, Tk, Ta, Tb)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    outs = []
    for fill in (-1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = (torch.empty((R, Ho, Wo), device=DEV), torch.empty((4,), device=DEV),
           torch.empty((4,), dtype=torch.int32, device=DEV))
      st = lib.snap_vote_filter_f32(p(belief), p(votes), p(taps[0]), taps[1], p(taps[2]), p(taps[3]), p(taps[4]), R, Ho,
                                    Wo, Tk, Ta, Tb, c['scale'], c['uniform_mix'], p(o[0]), p(o[1]), p(o[2]), p(ws), nbytes,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name


def test_bad_arguments_raise_without_launching():
  R, Ho, Wo = 4, 5, 6
  votes = torch.zeros((R, Ho, Wo), device=DEV)
  belief = torch.zeros((R, Ho, Wo), device=DEV)
  tk, ta, tb = torch.ones(2, device=DEV) / 2, torch.ones((R, 3), device=DEV) / 3, torch.ones((R, 2), device=DEV) / 2
  off = torch.zeros((R, 2), dtype=torch.int32, device=DEV)
  good = (tk, 0, ta, tb, off)
  ops.vote_filter(belief, votes, good)
  bad_taps = [(tk.double(), 0, ta, tb, off), (tk.cpu(), 0, ta, tb, off), (tk, 0.5, ta, tb, off), (tk, 2 ** 31, ta, tb, off),
              (tk, 0, ta[:3], tb, off), (tk, 0, ta, tb, off.long()), (tk, 0, ta, tb, off[:, :1]),
              (torch.ones(17, device=DEV), 0, ta, tb, off), (tk, 0, torch.ones((R, 33), device=DEV), tb, off),
              (tk, 0, ta, torch.ones((R, 0), device=DEV), off), (tk, 0, ta, tb), (tk[None], 0, ta, tb, off)]
  for taps in bad_taps:
    with pytest.raises(ValueError):
      ops.vote_filter(belief, votes, taps)
  for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=float('inf')), dict(scale=float('nan')),
             dict(uniform_mix=-0.1), dict(uniform_mix=1.5), dict(uniform_mix=float('nan'))):
    with pytest.raises(ValueError):
      ops.vote_filter(belief, votes, good, **kw)
  for b, v in ((belief[:3], votes), (belief.double(), votes), (belief.cpu(), votes), (belief, votes[0]),
               (belief, votes.double()), (None, votes.cpu())):
    with pytest.raises(ValueError):
      ops.vote_filter(b, v, good)
  big = torch.zeros((65, 2, 2), device=DEV)
  with pytest.raises(ValueError):
    ops.vote_filter(None, big, (tk, 0, torch.ones((65, 1), device=DEV), torch.ones((65, 1), device=DEV),
                                torch.zeros((65, 2), dtype=torch.int32, device=DEV)))
  lib = _lib.load()
  wsb = lib.snap_vote_filter_workspace_bytes
  assert wsb(0, 5, 6, 2, 3, 2) == 0 and wsb(65, 5, 6, 2, 3, 2) == 0 and wsb(4, 0, 6, 2, 3, 2) == 0
  assert wsb(4, 5, 6, 0, 3, 2) == 0 and wsb(4, 5, 6, 17, 3, 2) == 0 and wsb(4, 5, 6, 2, 33, 2) == 0
  assert wsb(4, 5, 6, 2, 3, 0) == 0 and wsb(64, 4096, 8192, 2, 3, 2) == 0          # R Ho Wo = 2^31
  need = wsb(R, Ho, Wo, 2, 3, 2)
  assert need == R * Ho * Wo * 4 + 4 * (4 * 8 + 4 * 4 + 2 * 4)                      # t1 and 4 workgroups' partials
  ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
  out = torch.full((R, Ho, Wo), 7.0, device=DEV)
  stats = torch.full((4,), 7.0, device=DEV)
  count = torch.full((4,), 7, dtype=torch.int32, device=DEV)
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

  def call(R_=R, Tk=2, Ta=3, Tb=2, scale=1.0, eps=0.0, nbytes=need, votes_=votes, wsp=None, count_=count):
    return lib.snap_vote_filter_f32(p(belief), p(votes_), p(tk), 0, p(ta), p(tb), p(off), R_, Ho, Wo, Tk, Ta, Tb, scale,
                                    eps, p(out), p(stats), p(count_), wsp if wsp is not None else p(ws), nbytes, None)

  assert call(R_=0) == -1 and call(R_=65, nbytes=1 << 30) == -1 and call(Tk=17) == -1 and call(Ta=0) == -1
  assert call(Tb=33) == -1
  assert call(votes_=None) == -3 and call(count_=None) == -3 and call(R_=65, votes_=None) == -3
  assert call(scale=0.0) == -2 and call(scale=float('inf')) == -2 and call(eps=1.5) == -2 and call(eps=float('nan')) == -2
  assert call(nbytes=need - 1) == -5 and call(wsp=ctypes.c_void_p(ws.data_ptr() + 4)) == -5
  torch.cuda.synchronize()
  assert bool((out == 7).all()) and bool((stats == 7).all()) and bool((count == 7).all())   # nothing ran


def test_vote_filter_localize_on_a_tiny_scene():
  """16^2 planes, D = 8, R = 8 (``method=None`` takes the direct form), three frames with a small motion.  The belief
  is the reference filter of the returned per-frame votes, step by step from the kernel's previous belief, within the
  bound; the peaks are ``poses_from_votes`` of the belief, bit for bit; ``reset()`` restarts the track."""
  H, D, R, N = 16, 8, 8, 3
  rng = np.random.default_rng(4321)
  grid = grids.Grid2D((H, H), 0.25)
  valid = torch.ones((H, H), dtype=torch.bool, device=DEV)
  pm = types.FeaturePlane(features=torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV), valid=valid)
  planes = [types.FeaturePlane(features=torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV),
                               valid=valid) for _ in range(N)]
  steps = [None, geometry.Transform2D(torch.tensor(0.12, dtype=torch.float64), torch.tensor([0.3, -0.2], dtype=torch.float64)),
           geometry.Transform2D(torch.tensor(-0.2, dtype=torch.float64), torch.tensor([-0.4, 0.15], dtype=torch.float64))]
  kw = dict(sigma_xy=0.2, sigma_yaw=0.15, temperature=4.0, uniform_mix=1e-3)
  track = pev.VoteFilter(grid, R, **kw)
  assert track.belief is None
  prev, first = None, None
  for n in range(N):
    with guarded.scope():
      out = track.localize(planes[n], pm, steps[n], num_peaks=4)
    assert set(out) == {'map_t_query', 'index', 'score', 'count', 'votes', 'votes_frame', 'log_evidence', 'mass_kept'}
    assert out['votes'] is track.belief and tuple(out['votes'].shape) == (R, 2 * H - 1, 2 * H - 1)
    assert guarded.same_bits(out['votes_frame'], pev.exhaustive_pose_voting(planes[n], pm, R, grid))
    frame = out['votes_frame'].cpu().numpy()
    if n == 0:
      taps, first = pev._still_taps(R, DEV), out
    else:
      taps = pev.motion_taps(steps[n], grid, R, kw['sigma_xy'], kw['sigma_yaw'])
    taps = tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in taps)
    args = (prev, frame, taps, kw['temperature'], kw['uniform_mix'])
    want = ref.vote_filter(*args)
    got = (out['votes'].cpu().numpy(), np.array([float(out['log_evidence']), float(out['mass_kept']), want[1][2],
                                                 float(out['score'][0])]), want[2])
    assert got[0].dtype == np.float32
    _assert_within(got, want, ref.bound(*args), ref.stats_bound(*args), f'frame {n}')
    peaks = pev.poses_from_votes(out['votes'], grid, R, num_peaks=4)
    for k in ('index', 'score', 'count'):
      assert guarded.same_bits(peaks[k], out[k]), k
    assert int(out['count'][0]) >= 1
    prev = got[0]
  assert float(first['mass_kept']) == 1.0
  post = track.localize(planes[0], pm, None, num_peaks=4, posterior=True)       # no motion: the belief is diffused
  alone = pev.posterior_from_votes(post['votes'], grid, R)
  for k in ('log_prob_xy', 'log_prob_r', 'stats', 'count'):
    assert guarded.same_bits(post['posterior'][k], alone[k]), k
  track.reset()
  assert track.belief is None
  again = track.localize(planes[0], pm, steps[1], num_peaks=4)                  # the increment of a first step is ignored
  assert guarded.same_bits(again['votes'], first['votes']) and guarded.same_bits(again['index'], first['index'])
  step = pev.filter_votes(None, first['votes_frame'], None, grid, R, **kw)
  assert guarded.same_bits(step['belief'], first['votes']) and tuple(step['count'].shape) == (4,)
