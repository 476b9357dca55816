"""`-m gpu`: ``ops.vote_smooth`` (vote_smooth.hip, through the C ABI) and the host entry points built on it, against the
float64 numpy restatement ``vote_smooth_reference`` within twice its derived rounding bound; ``count`` exactly, the NaN
and -inf cells identical, ``stats`` within twice its own derived bound.

The tiling is the filter's (a tile = one rotation and 256 consecutive pixels, up to 2048 workgroups striding over the
tiles), and so are the shapes: ``tiny`` [1, 1, 1]; ``wrap`` / ``wrap_far`` / ``wrap_neg`` [4, 7, 7]: Tk = 3 with lk = -1,
R + 2 and -3 R - 2, where the adjoint wraps the other way; ``ragged`` [36, 31, 33]: four tiles per rotation, the last
ragged, zero taps, offsets of both signs, two rotations whose taps all fall outside, 30 % -inf; ``mix0`` / ``mix1``:
eps = 0 and 1 on the same data; ``bad``: a NaN and a +inf cell in ``belief`` and in ``next``; ``wide`` [2, 20, 300]
Tb = 32 and ``tall`` [2, 300, 20] Ta = 32; ``tk16`` [5, 6, 9]: Tk = 16 > R; ``tiles`` [2, 520, 520]: 2114 tiles on 2048
workgroups; ``empty_belief`` / ``no_mass``: no belief mass / ``next`` all -inf; ``cut``: a ``next`` that is not the
filter's, ratios on both sides of the e^-40 cut; ``exact``: masses in {0, 1}, power-of-two taps, integer shifts: u and Q
are the reference's bit for bit, and the bound is float64 noise and the final f32 rounding alone.  ``next`` is the
reference filter's result one step further.  Every call runs under ``guarded.scope()``: guard regions intact (outputs
and workspace), no output element left unwritten, the workspace the size ``snap_vote_smooth_workspace_bytes`` states.

Observed on an MI355X (each case prints its figures), largest err / bound: ``tiny`` 0.00, ``wrap`` 0.18, ``wrap_far`` /
``wrap_neg`` 0.19, ``ragged`` 0.18 (4.1e-6 against 2.3e-5), ``mix0`` 0.17, ``bad`` 0.18, ``wide`` 0.11, ``tall`` 0.10,
``tk16`` 0.12, ``tiles`` 0.17, ``cut`` 0.18; ``mix1`` 0.77 (eps = 1: the prior is uniform and the bound is little more than
the final f32 rounding); ``exact`` 0.68 of a bound that is float64 noise and the final rounding alone (1.2e-7 against
3.5e-7); the tiny scene's frames 0.03.  ``stats``, outside ``exact``: ``log_norm`` at most 0.17 of its bound (``mix1``;
0.01 with eps < 1), ``mass_kept`` 0.07, ``G`` 0.39 (``empty_belief``: the f32 rounding of G alone; 0.04 otherwise), the
largest smoothed 0.01; on ``exact`` 0.32 / 0.16 / 0.48 / 0.34.  With the filter's own beliefs abs(log_norm) is
2.5e-8 ... 6.8e-8 against summed bounds of 3.4e-5 ... 3.8e-5; the dense alpha-beta check 7.3e-7 ... 1.1e-6 against
8.3e-5 ... 1.1e-4.  2 x the bound is allowed."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_filter_reference as flt
import vote_smooth_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import geometry, grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _inputs():
  return {c['name']: c for c in ref.all_inputs()}


def _args(c):
  return c['belief'], c['next'], c['taps'], c['uniform_mix']


@functools.lru_cache(maxsize=None)
def _want(name):
  c = _inputs()[name]
  exact = name == 'exact'
  return (ref.vote_smooth(*_args(c)),) + ref.bounds(*_args(c), exact=exact)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_taps(taps, place=False):
  tk, lk, ta, tb, off = taps
  put = (lambda t, kind: guarded.place(t, kind)) if place else (lambda t, kind: t)
  return (put(_dev(tk), 'value'), int(lk), put(_dev(ta), 'value'), put(_dev(tb), 'value'), put(_dev(off), 'address'))


def _host_taps(taps):
  return tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in taps)


def _run(belief, nxt, taps, uniform_mix=0.0):
  """One guarded call -> numpy (smoothed, stats, count)."""
  R, Ho, Wo = belief.shape
  with guarded.scope() as sc:
    out = ops.vote_smooth(guarded.place(_dev(belief), 'value'), guarded.place(_dev(nxt), 'value'),
                          _dev_taps(taps, place=True), uniform_mix)
    assert [tuple(o.shape) for o in out] == [(R, Ho, Wo), (4,), (4,)]
    assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.int32]
    ws = [a for a in sc.allocations('vote_smooth') if a.dtype == torch.int64]
    need = _lib.load().snap_vote_smooth_workspace_bytes(R, Ho, Wo, len(taps[0]), taps[2].shape[1], taps[3].shape[1])
    assert len(ws) == 1 and ws[0].numel() * 8 == need
    for o, what in zip(out, ('smoothed', 'stats', 'count')):      # (the kernel's NaN is 0x7fc00000, not the poison)
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
  for i, name in enumerate(('log_norm', 'mass_kept', 'G', 'top')):
    if np.isfinite(ws[i]):
      e = abs(float(gs[i]) - ws[i])
      print(f'{what}: stats {name} err {e:.3e}, bound {stol[i]:.3e}')
      assert e <= factor * stol[i], f'{what}: stats[{i}] {gs[i]} against {ws[i]}'
    else:
      assert float(gs[i]) == ws[i], f'{what}: stats[{i}] {gs[i]} against {ws[i]}'
  # normalisation: float64 sum of exp over the finite cells is 1 within max |smoothed| 2^-23
  if fin.any():
    gf = g[np.isfinite(g)].astype(np.float64)
    total = np.exp(gf).sum()
    print(f'{what}: sum exp(smoothed) - 1 = {total - 1:.3e}')
    assert abs(total - 1) <= np.abs(gf).max() * 2.0 ** -23


CASES = ['tiny', 'wrap', 'wrap_far', 'wrap_neg', 'ragged', 'mix0', 'mix1', 'bad', 'wide', 'tall', 'tk16', 'tiles',
         'empty_belief', 'no_mass', 'cut', 'exact']


@pytest.mark.parametrize('name', CASES)
def test_against_the_reference(name):
  c = _inputs()[name]
  want, tol, stol = _want(name)
  got = _run(*_args(c))
  _assert_within(got, want, tol, stol, name)
  if name == 'no_mass':
    assert (got[0] == -np.inf).all() and got[1][0] == -np.inf and got[1][2] == -np.inf and got[2].tolist()[2:] == [0, 0]


def _gpu_track(eps):
  """The tiny track filtered on the GPU -> (votes, host taps, scale, beliefs [3] numpy f32, the filter's stats)."""
  votes, taps, scale = ref.tiny_track()
  beliefs, stats, prev = [], [], None
  for t in range(len(votes)):
    out = ops.vote_filter(prev, _dev(votes[t]), _dev_taps(taps[t] or ref.still_taps(3)), scale, eps)
    prev = out[0]
    beliefs.append(out[0].cpu().numpy())
    stats.append(out[1].cpu().numpy())
  return votes, taps, scale, beliefs, stats


@pytest.mark.parametrize('eps', [0.0, 1e-3])
def test_mass_kept_is_the_filters_bits_and_log_norm_is_zero(eps):
  """belief_t, votes_{t+1} and the taps through ``ops.vote_filter``, then ``vote_smooth(belief_t, belief_{t+1})``:
  stats[1] is the filter's mass_kept bit for bit (the predict code is shared), and |log_norm| lies within the summed
  bounds: the filter's cell bound of belief_{t+1} (sum gamma_{t+1} is off by at most that), the normalisation slack of
  belief_t (max |belief_t| 2^-23, what the filter's own test allows) and the smoother's bound of log_norm."""
  votes, taps, scale, beliefs, fstats = _gpu_track(eps)
  for name in ('ragged', 'tiles'):
    c = {c['name']: c for c in flt.all_inputs()}[name]
    first = ops.vote_filter(None, _dev(c['votes']), _dev_taps(c['taps']), c['scale'], eps)[0]
    second = ops.vote_filter(first, _dev(c['votes'][::-1].copy()), _dev_taps(c['taps']), c['scale'], eps)
    b0, b1 = first.cpu().numpy(), second[0].cpu().numpy()
    g, gs, gc = _run(b0, b1, c['taps'], eps)
    assert gs[1].tobytes() == second[1][1].cpu().numpy().tobytes(), f'{name}: mass_kept {gs[1]} / {second[1][1]}'
    fb = flt.bound(b0, c['votes'][::-1].copy(), c['taps'], c['scale'], eps)
    tol = 2 * fb.max() + np.abs(b0[np.isfinite(b0)]).max() * 2.0 ** -23 + 2 * ref.stats_bound(b0, b1, c['taps'], eps)[0]
    print(f'{name} eps {eps}: log_norm {float(gs[0]):.3e}, summed bounds {tol:.3e}')
    assert abs(float(gs[0])) <= tol
  for t in (0, 1):
    g, gs, gc = _run(beliefs[t], beliefs[t + 1], taps[t + 1], eps)
    assert gs[1].tobytes() == fstats[t + 1][1].tobytes()


@pytest.mark.parametrize('eps', [0.0, 1e-3])
def test_dense_alpha_beta_with_every_volume_from_the_gpu(eps):
  """The independent formulation of test_vote_smooth_reference.py with the three frames filtered and smoothed on the
  GPU.  Agreement within the f32 roundings of the stored volumes (64 * 2^-24 (1 + max |log gamma|), as there) plus
  twice the filter's bounds of the frames behind a volume and the smoother's bounds of the steps behind it."""
  votes, taps, scale, beliefs, _ = _gpu_track(eps)
  N, n = len(votes), votes[0].size
  gamma = ref.dense_smoothing(votes, taps, scale, eps, beliefs)
  tol_f = sum(flt.bound(None if t == 0 else beliefs[t - 1], votes[t], taps[t] or ref.still_taps(3), scale, eps).max()
              for t in range(N))
  smoothed, tol_s = [None] * N, 0.0
  smoothed[-1] = beliefs[-1]
  for t in range(N - 2, -1, -1):
    smoothed[t] = _run(beliefs[t], smoothed[t + 1], taps[t + 1], eps)[0]
    tol_s += ref.bound(beliefs[t], smoothed[t + 1], taps[t + 1], eps).max()
    g = gamma[t]
    fin = g > 0
    have = smoothed[t].reshape(n)
    assert ((have == -np.inf) == ~fin).all()
    want = np.log(g[fin])
    err = np.abs(have[fin].astype(np.float64) - want).max()
    tol = 64 * U * (1 + np.abs(want).max()) + 2 * (tol_f + tol_s)
    print(f'eps {eps} frame {t}: max err {err:.3e}, tolerance {tol:.3e}')
    assert err <= tol


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for name in ('ragged', 'bad', 'tiles'):
    c = _inputs()[name]
    belief, nxt, taps = _dev(c['belief']), _dev(c['next']), _dev_taps(c['taps'])
    first = ops.vote_smooth(belief, nxt, taps, c['uniform_mix'])
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_smooth(belief, nxt, taps, c['uniform_mix'])
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    R, Ho, Wo = belief.shape
    Tk, Ta, Tb = taps[0].shape[0], taps[2].shape[1], taps[3].shape[1]
    nbytes = lib.snap_vote_smooth_workspace_bytes(R, Ho, Wo, Tk, Ta, Tb)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    outs = []
    for fill in (-1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = (torch.empty((R, Ho, Wo), device=DEV), torch.empty((4,), device=DEV),
           torch.empty((4,), dtype=torch.int32, device=DEV))
      st = lib.snap_vote_smooth_f32(p(belief), p(nxt), p(taps[0]), taps[1], p(taps[2]), p(taps[3]), p(taps[4]), R, Ho, Wo,
                                    Tk, Ta, Tb, c['uniform_mix'], p(o[0]), p(o[1]), p(o[2]), p(ws), nbytes,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name


def test_bad_arguments_raise_without_launching():
  R, Ho, Wo = 4, 5, 6
  belief = torch.zeros((R, Ho, Wo), device=DEV)
  nxt = torch.zeros((R, Ho, Wo), device=DEV)
  tk, ta, tb = torch.ones(2, device=DEV) / 2, torch.ones((R, 3), device=DEV) / 3, torch.ones((R, 2), device=DEV) / 2
  off = torch.zeros((R, 2), dtype=torch.int32, device=DEV)
  good = (tk, 0, ta, tb, off)
  ops.vote_smooth(belief, nxt, good)
  bad_taps = [(tk.double(), 0, ta, tb, off), (tk.cpu(), 0, ta, tb, off), (tk, 0.5, ta, tb, off), (tk, 2 ** 31, ta, tb, off),
              (tk, 0, ta[:3], tb, off), (tk, 0, ta, tb, off.long()), (tk, 0, ta, tb, off[:, :1]),
              (torch.ones(17, device=DEV), 0, ta, tb, off), (tk, 0, torch.ones((R, 33), device=DEV), tb, off),
              (tk, 0, ta, torch.ones((R, 0), device=DEV), off), (tk, 0, ta, tb), (tk[None], 0, ta, tb, off)]
  for taps in bad_taps:
    with pytest.raises(ValueError):
      ops.vote_smooth(belief, nxt, taps)
  for kw in (dict(uniform_mix=-0.1), dict(uniform_mix=1.5), dict(uniform_mix=float('nan'))):
    with pytest.raises(ValueError):
      ops.vote_smooth(belief, nxt, good, **kw)
  for b, v in ((belief[:3], nxt), (belief.double(), nxt), (belief.cpu(), nxt), (belief, nxt[0]), (belief, nxt.double()),
               (belief, nxt.cpu()), (None, nxt), (belief, None)):
    with pytest.raises(ValueError):
      ops.vote_smooth(b, v, good)
  big = torch.zeros((65, 2, 2), device=DEV)
  with pytest.raises(ValueError):
    ops.vote_smooth(big, big.clone(), (tk, 0, torch.ones((65, 1), device=DEV), torch.ones((65, 1), device=DEV),
                                       torch.zeros((65, 2), dtype=torch.int32, device=DEV)))
  lib = _lib.load()
  wsb = lib.snap_vote_smooth_workspace_bytes
  assert wsb(0, 5, 6, 2, 3, 2) == 0 and wsb(65, 5, 6, 2, 3, 2) == 0 and wsb(4, 0, 6, 2, 3, 2) == 0
  assert wsb(4, 5, 6, 0, 3, 2) == 0 and wsb(4, 5, 6, 17, 3, 2) == 0 and wsb(4, 5, 6, 2, 33, 2) == 0
  assert wsb(4, 5, 6, 2, 3, 0) == 0 and wsb(64, 4096, 8192, 2, 3, 2) == 0          # R Ho Wo = 2^31
  need = wsb(R, Ho, Wo, 2, 3, 2)
  assert need == R * Ho * Wo * 4 + 4 * (6 * 8 + 5 * 4 + 2 * 4)                      # one volume and 4 workgroups' partials
  ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
  out = torch.full((R, Ho, Wo), 7.0, device=DEV)
  stats = torch.full((4,), 7.0, device=DEV)
  count = torch.full((4,), 7, dtype=torch.int32, device=DEV)
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

  def call(R_=R, Tk=2, Ta=3, Tb=2, eps=0.0, nbytes=need, belief_=belief, next_=nxt, wsp=None, count_=count):
    return lib.snap_vote_smooth_f32(p(belief_), p(next_), p(tk), 0, p(ta), p(tb), p(off), R_, Ho, Wo, Tk, Ta, Tb, eps,
                                    p(out), p(stats), p(count_), wsp if wsp is not None else p(ws), nbytes, None)

  assert call(R_=0) == -1 and call(R_=65, nbytes=1 << 30) == -1 and call(Tk=17) == -1 and call(Ta=0) == -1
  assert call(Tb=33) == -1
  assert call(belief_=None) == -3 and call(next_=None) == -3 and call(count_=None) == -3
  assert call(R_=65, next_=None) == -3
  assert call(eps=1.5) == -2 and call(eps=-0.5) == -2 and call(eps=float('nan')) == -2
  assert call(nbytes=need - 1) == -5 and call(wsp=ctypes.c_void_p(ws.data_ptr() + 4)) == -5
  torch.cuda.synchronize()
  assert bool((out == 7).all()) and bool((stats == 7).all()) and bool((count == 7).all())   # nothing ran


def test_vote_filter_smooth_on_a_tiny_scene():
  """16^2 planes, D = 8, R = 8, three frames with a small motion: ``VoteFilter(keep_history=True).localize`` x 3, then
  ``.smooth(num_peaks=4)``.  The last frame is the filter's belief bit for bit; the earlier frames are the reference
  recursion over the kernel's own beliefs, step by step from the kernel's smoothed next frame, within the bound; the
  peaks are ``poses_from_votes`` of the smoothed volume bit for bit; ``smooth_track`` gives the same volumes;
  ``keep_history=False`` leaves ``localize``'s dicts as they are; ``smooth()`` without a history raises."""
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
  track, plain = pev.VoteFilter(grid, R, keep_history=True, **kw), pev.VoteFilter(grid, R, **kw)
  assert track.history == [] and not hasattr(plain, 'history')
  with pytest.raises(ValueError):
    track.smooth()
  with pytest.raises(ValueError):
    plain.smooth()
  outs = []
  for n in range(N):
    with guarded.scope():
      outs.append(track.localize(planes[n], pm, steps[n], num_peaks=4))
      base = plain.localize(planes[n], pm, steps[n], num_peaks=4)
    assert set(outs[-1]) == set(base) == {'map_t_query', 'index', 'score', 'count', 'votes', 'votes_frame',
                                          'log_evidence', 'mass_kept'}
    for k in ('index', 'score', 'count', 'votes', 'votes_frame', 'log_evidence', 'mass_kept'):
      assert guarded.same_bits(outs[-1][k], base[k]), k
  assert len(track.history) == N and all(h[0] is o['votes'] for h, o in zip(track.history, outs))
  with pytest.raises(ValueError):
    plain.smooth()
  with guarded.scope():
    frames = track.smooth(num_peaks=4, posterior=True)
  assert len(frames) == N and frames[-1]['votes'] is outs[-1]['votes'] and frames[-1]['log_norm'] is None
  assert guarded.same_bits(frames[-1]['votes'], track.belief)
  nxt = frames[-1]['votes'].cpu().numpy()
  for t in range(N - 2, -1, -1):
    f = frames[t]
    assert set(f) == {'map_t_query', 'index', 'score', 'count', 'votes', 'log_norm', 'posterior'}
    taps = _host_taps(pev.motion_taps(steps[t + 1], grid, R, kw['sigma_xy'], kw['sigma_yaw']))
    belief = outs[t]['votes'].cpu().numpy()
    args = (belief, nxt, taps, kw['uniform_mix'])
    want = ref.vote_smooth(*args)
    got = (f['votes'].cpu().numpy(), np.array([float(f['log_norm']), want[1][1], want[1][2], float(f['score'][0])]),
           want[2])
    assert got[0].dtype == np.float32
    _assert_within(got, want, *ref.bounds(*args), f'frame {t}')
    assert abs(float(f['log_norm'])) <= 1e-4                 # (beliefs and increments belong together)
    peaks = pev.poses_from_votes(f['votes'], grid, R, num_peaks=4)
    for k in ('index', 'score', 'count'):
      assert guarded.same_bits(peaks[k], f[k]), k
    alone = pev.posterior_from_votes(f['votes'], grid, R)
    assert guarded.same_bits(f['posterior']['log_prob_xy'], alone['log_prob_xy'])
    nxt = got[0]
  vols = pev.smooth_track([o['votes'] for o in outs], steps, grid, R, kw['sigma_xy'], kw['sigma_yaw'], kw['uniform_mix'])
  assert vols[-1] is outs[-1]['votes'] and all(guarded.same_bits(v, f['votes']) for v, f in zip(vols, frames))
  one = pev.smooth_votes(outs[0]['votes'], frames[1]['votes'], steps[1], grid, R, kw['sigma_xy'], kw['sigma_yaw'],
                         kw['uniform_mix'])
  assert set(one) == {'smoothed', 'log_norm', 'mass_kept', 'count', 'stats'}
  assert guarded.same_bits(one['smoothed'], frames[0]['votes'])
  assert guarded.same_bits(one['mass_kept'], outs[1]['mass_kept'])       # the filter's bits of that step
  track.reset()
  assert track.history == [] and track.belief is None
