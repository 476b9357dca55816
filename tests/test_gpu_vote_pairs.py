"""`-m gpu`: ``ops.vote_pairs`` (vote_pairs.hip, through the C ABI) and the host entry points built on it, against the
float64 numpy restatement ``vote_pairs_reference`` within twice its derived rounding bound; ``count`` exactly.

The cases are ``vote_smooth_reference.all_inputs()`` (the smoother's: see test_gpu_vote_smooth.py; ``tiny`` has Tk = Ta =
Tb = 1; ``tiles`` [2, 520, 520] has 2114 tiles on 2048 workgroups and 1024 reduction workgroups per rotation striding
over 1057 tiles; ``exact`` is compared with no tolerance), then ``still`` [3, 4, 5] (one tap of weight 1 per axis:
every histogram is a single entry) and ``big`` [64, 97, 89]: R at its limit, P = 8633 no multiple of 256, 2176 tiles
> 2048 workgroups, 32 reduction workgroups per rotation on 34 tiles, Tk = 16 and Ta = Tb = 32 with zero taps.  Every
call runs under ``guarded.scope()``: guard regions intact (outputs and workspace), no output element left unwritten,
the workspace the size ``snap_vote_pairs_workspace_bytes`` states.

Observed on an MI355X (each case prints its figures), largest err / bound over the three histograms, stay and jump:
``tiny``, ``mix1``, ``empty_belief``, ``no_mass`` and ``exact`` 0 (``exact`` is compared for equality), ``tall``,
``tiles`` and ``still`` 0.001, ``big`` 0.003, ``wrap_far``, ``wrap_neg`` and ``tk16`` 0.004, ``mix0`` and ``wide``
0.006, ``wrap`` and ``ragged`` 0.007, ``bad`` 0.008, ``cut`` 0.010: the bound carries the worst case of every f32
chain behind q, the kernel's errors are far from aligned.  The three-frame track: 0.006 and 0.435 (the jump share,
3e-5 of the step, off by 2e-12 against a bound of 8e-10).  With the filter's own beliefs |log_norm| is 6e-10 ... 2e-8
against summed bounds of 4.1e-5 ... 4.6e-5.  2 x the bound is allowed."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_filter_reference as flt
import vote_pairs_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from test_vote_pairs_reference import GRID_EM, R_EM, START, em_track, np_taps, reference_e_step

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE


@functools.lru_cache(maxsize=None)
def _inputs():
  return {c['name']: c for c in ref.all_inputs()}


def _args(c):
  return c['belief'], c['next'], c['taps'], c['uniform_mix']


@functools.lru_cache(maxsize=None)
def _want(name):
  c = _inputs()[name]
  return ref.vote_pairs(*_args(c)), ref.bounds(*_args(c), exact=name == 'exact')


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_taps(taps, place=False):
  tk, lk, ta, tb, off = taps
  put = (lambda t, kind: guarded.place(t, kind)) if place else (lambda t, kind: t)
  return (put(_dev(tk), 'value'), int(lk), put(_dev(ta), 'value'), put(_dev(tb), 'value'), put(_dev(off), 'address'))


def _run(belief, nxt, taps, uniform_mix=0.0):
  """One guarded call -> numpy (hist_k, hist_a, hist_b, stats, count)."""
  R, Ho, Wo = belief.shape
  Tk, Ta, Tb = len(taps[0]), taps[2].shape[1], taps[3].shape[1]
  with guarded.scope() as sc:
    out = ops.vote_pairs(guarded.place(_dev(belief), 'value'), guarded.place(_dev(nxt), 'value'),
                         _dev_taps(taps, place=True), uniform_mix)
    assert [tuple(o.shape) for o in out] == [(Tk,), (R, Ta), (R, Tb), (4,), (4,)]
    assert [o.dtype for o in out] == [torch.float64] * 4 + [torch.int32]
    ws = [a for a in sc.allocations('vote_pairs') if a.dtype == torch.int64]
    need = _lib.load().snap_vote_pairs_workspace_bytes(R, Ho, Wo, Tk, Ta, Tb)
    assert len(ws) == 1 and ws[0].numel() * 8 == need
    for o, what in zip(out, ('hist_k', 'hist_a', 'hist_b', 'stats', 'count')):
      assert not bool(guarded.unwritten(o).any()), f'{what}: elements never written'
    res = tuple(o.cpu().numpy() for o in out)
  return res


def _assert_within(got, want, tol, what, exact=False, factor=2.0):
  assert got[4].tolist() == want[4].tolist(), f'{what}: count {got[4].tolist()} != {want[4].tolist()}'
  worst = 0.0
  for g, w, b, name in zip(got[:3], want[:3], tol[:3], ('hist_k', 'hist_a', 'hist_b')):
    assert np.isfinite(g).all() and (g >= 0).all(), f'{what}: {name}'
    err = np.abs(g - w)
    if exact:
      assert (g == w).all(), f'{what}: {name} differs by {err.max():.3e} where no tolerance is allowed'
      continue
    frac = float(np.max(err / np.maximum(b, 1e-300))) if err.max() > 0 else 0.0
    worst = max(worst, frac)
    print(f'{what}: {name} max err {err.max():.3e}, max bound {b.max():.3e}, max err / bound {frac:.3f}')
    assert (err <= factor * b).all(), f'{what}: {name} outside {factor} x bound'
  gs, ws, bs = got[3], want[3], tol[3]
  for i, name in enumerate(('stay', 'jump', 'log_norm', 'mass_kept')):
    if not np.isfinite(ws[i]) or (exact and i != 2):
      assert gs[i] == ws[i], f'{what}: {name} {gs[i]} against {ws[i]}'
      continue
    e = abs(gs[i] - ws[i])
    if i < 2 and e > 0:
      worst = max(worst, e / max(bs[i], 1e-300))
    print(f'{what}: {name} {gs[i]:.9g} err {e:.3e}, bound {bs[i]:.3e}')
    assert e <= factor * bs[i], f'{what}: {name} {gs[i]} against {ws[i]}'
  print(f'{what}: largest err / bound {worst:.3f}')
  # stay + jump = 1 and every table sums to stay
  if ws[0] + ws[1] > 0:
    assert abs(gs[0] + gs[1] - 1) <= 4 * 2.0 ** -53
    for g, b, name in zip(got[:3], tol[:3], ('hist_k', 'hist_a', 'hist_b')):
      e = abs(g.sum() - gs[0])
      print(f'{what}: sum {name} - stay = {g.sum() - gs[0]:.3e}, bound of the sum {b.sum() + bs[0]:.3e}')
      assert e <= factor * (b.sum() + bs[0]) + g.size * 2.0 ** -52, f'{what}: sum {name}'


CASES = ['tiny', 'wrap', 'wrap_far', 'wrap_neg', 'ragged', 'mix0', 'mix1', 'bad', 'wide', 'tall', 'tk16', 'tiles',
         'empty_belief', 'no_mass', 'cut', 'exact', 'still', 'big']


@pytest.mark.parametrize('name', CASES)
def test_against_the_reference(name):
  c = _inputs()[name]
  want, tol = _want(name)
  got = _run(*_args(c))
  _assert_within(got, want, tol, name, exact=name == 'exact')
  if name == 'no_mass':
    assert not got[0].any() and not got[1].any() and not got[2].any() and got[3][:3].tolist() == [0, 0, -np.inf]
  if name in ('tiny', 'still'):
    assert got[0].tolist() == [1.0] and got[3][0] == 1 and got[3][1] == 0
  if name == 'big':
    assert (len(c['taps'][0]), c['taps'][2].shape[1], c['taps'][3].shape[1]) == (16, 32, 32)


@pytest.mark.parametrize('eps', [0.0, 1e-3])
def test_mass_kept_is_the_filters_bits_and_log_norm_is_zero(eps):
  """belief_t, votes_{t+1} and the taps through ``ops.vote_filter``, then ``vote_pairs(belief_t, belief_{t+1})``:
  stats[3] converted to f32 is the filter's mass_kept bit for bit (the predict code is shared), and |log_norm| lies
  within the summed bounds: the filter's cell bound of belief_{t+1} twice, the normalisation slack of belief_{t+1}
  (max |belief| 2^-23, what the filter's own test allows) and this op's bound of log_norm twice."""
  for name in ('ragged', 'tiles'):
    c = {c['name']: c for c in flt.all_inputs()}[name]
    first = ops.vote_filter(None, _dev(c['votes']), _dev_taps(c['taps']), c['scale'], eps)[0]
    second = ops.vote_filter(first, _dev(c['votes'][::-1].copy()), _dev_taps(c['taps']), c['scale'], eps)
    b0, b1 = first.cpu().numpy(), second[0].cpu().numpy()
    got = _run(b0, b1, c['taps'], eps)
    kept = np.float32(got[3][3])
    assert float(kept) == got[3][3] and kept.tobytes() == second[1][1].cpu().numpy().tobytes(), name
    fb = flt.bound(b0, c['votes'][::-1].copy(), c['taps'], c['scale'], eps)
    tol = 2 * fb.max() + np.abs(b1[np.isfinite(b1)]).max() * 2.0 ** -23 + 2 * ref.bounds(b0, b1, c['taps'], eps)[3][2]
    print(f'{name} eps {eps}: log_norm {got[3][2]:.3e}, summed bounds {tol:.3e}')
    assert abs(got[3][2]) <= tol


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for name in ('ragged', 'bad', 'big'):
    c = _inputs()[name]
    belief, nxt, taps = _dev(c['belief']), _dev(c['next']), _dev_taps(c['taps'])
    first = ops.vote_pairs(belief, nxt, taps, c['uniform_mix'])
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_pairs(belief, nxt, taps, c['uniform_mix'])
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    R, Ho, Wo = belief.shape
    Tk, Ta, Tb = taps[0].shape[0], taps[2].shape[1], taps[3].shape[1]
    nbytes = lib.snap_vote_pairs_workspace_bytes(R, Ho, Wo, Tk, Ta, Tb)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    outs = []
    for fill in (-1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = tuple(torch.empty_like(t) for t in first)
      st = lib.snap_vote_pairs_f32(p(belief), p(nxt), p(taps[0]), taps[1], p(taps[2]), p(taps[3]), p(taps[4]), R, Ho, Wo,
                                   Tk, Ta, Tb, c['uniform_mix'], p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(ws),
                                   nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
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
  ops.vote_pairs(belief, nxt, good)
  bad_taps = [(tk.double(), 0, ta, tb, off), (tk.cpu(), 0, ta, tb, off), (tk, 0.5, ta, tb, off), (tk, 2 ** 31, ta, tb, off),
              (tk, 0, ta[:3], tb, off), (tk, 0, ta, tb, off.long()), (tk, 0, ta, tb, off[:, :1]),
              (torch.ones(17, device=DEV), 0, ta, tb, off), (tk, 0, torch.ones((R, 33), device=DEV), tb, off),
              (tk, 0, ta, torch.ones((R, 33), device=DEV), off), (tk, 0, ta, torch.ones((R, 0), device=DEV), off),
              (tk, 0, ta, tb), (tk[None], 0, ta, tb, off)]
  for taps in bad_taps:
    with pytest.raises(ValueError):
      ops.vote_pairs(belief, nxt, taps)
  for kw in (dict(uniform_mix=-0.1), dict(uniform_mix=1.5), dict(uniform_mix=float('nan'))):
    with pytest.raises(ValueError):
      ops.vote_pairs(belief, nxt, good, **kw)
  for b, v in ((belief[:3], nxt), (belief.double(), nxt), (belief.cpu(), nxt), (belief, nxt[0]), (belief, nxt.double()),
               (belief, nxt.cpu()), (None, nxt), (belief, None)):
    with pytest.raises(ValueError):
      ops.vote_pairs(b, v, good)
  big = torch.zeros((65, 2, 2), device=DEV)
  with pytest.raises(ValueError):
    ops.vote_pairs(big, big.clone(), (tk, 0, torch.ones((65, 1), device=DEV), torch.ones((65, 1), device=DEV),
                                      torch.zeros((65, 2), dtype=torch.int32, device=DEV)))
  lib = _lib.load()
  wsb = lib.snap_vote_pairs_workspace_bytes
  assert wsb(0, 5, 6, 2, 3, 2) == 0 and wsb(65, 5, 6, 2, 3, 2) == 0 and wsb(4, 0, 6, 2, 3, 2) == 0
  assert wsb(4, 5, 6, 0, 3, 2) == 0 and wsb(4, 5, 6, 17, 3, 2) == 0 and wsb(4, 5, 6, 2, 33, 2) == 0
  assert wsb(4, 5, 6, 2, 3, 0) == 0 and wsb(64, 4096, 8192, 2, 3, 2) == 0          # R Ho Wo = 2^31
  need = wsb(R, Ho, Wo, 2, 3, 2)
  # four volumes, 4 workgroups' partials (4 float64, 4 int32, 1 f32 each), 4 x 1 partial rows of 2 + 3 + 2 float64
  assert need == 4 * R * Ho * Wo * 4 + 4 * (4 * 8 + 4 * 4) + 4 * 4 + 4 * (2 + 3 + 2) * 8
  ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
  hk, ha, hb = (torch.full(s, 7.0, dtype=torch.float64, device=DEV) for s in ((2,), (R, 3), (R, 2)))
  stats = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
  count = torch.full((4,), 7, dtype=torch.int32, device=DEV)
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

  def call(R_=R, Tk=2, Ta=3, Tb=2, eps=0.0, nbytes=need, belief_=belief, next_=nxt, wsp=None, count_=count, hk_=hk):
    return lib.snap_vote_pairs_f32(p(belief_), p(next_), p(tk), 0, p(ta), p(tb), p(off), R_, Ho, Wo, Tk, Ta, Tb, eps,
                                   p(hk_), p(ha), p(hb), p(stats), p(count_), wsp if wsp is not None else p(ws), nbytes,
                                   None)

  assert call(R_=0) == -1 and call(R_=65, nbytes=1 << 30) == -1 and call(Tk=17) == -1 and call(Ta=0) == -1
  assert call(Tb=33) == -1
  assert call(belief_=None) == -3 and call(next_=None) == -3 and call(count_=None) == -3 and call(hk_=None) == -3
  assert call(R_=65, next_=None) == -3
  assert call(eps=1.5) == -2 and call(eps=-0.5) == -2 and call(eps=float('nan')) == -2
  assert call(nbytes=need - 1) == -5 and call(wsp=ctypes.c_void_p(ws.data_ptr() + 4)) == -5
  torch.cuda.synchronize()
  for t in (hk, ha, hb, stats, count):
    assert bool((t == 7).all())                                # nothing ran


def _gpu_em_track(frames):
  votes, increments, scale = em_track()
  return [_dev(v) for v in votes[:frames]], increments[:frames], scale


def test_pair_statistics_on_a_three_frame_track():
  """Three frames of the EM track filtered and smoothed on the GPU (``filter_votes``, ``smooth_track``), then
  ``track_statistics``: each step against the reference on the GPU's own volumes, within twice the bound; the tables
  are ``motion_taps``' (the host restatement's bits); |log_norm| is small (the arguments belong together)."""
  votes, increments, scale = _gpu_em_track(3)
  kw = dict(sigma_xy=START['sigma_xy'], sigma_yaw=START['sigma_yaw'], uniform_mix=START['uniform_mix'])
  beliefs, belief = [], None
  for v, inc in zip(votes, increments):
    belief = pev.filter_votes(belief, v, inc, GRID_EM, R_EM, temperature=scale, **kw)['belief']
    beliefs.append(belief)
  smoothed = pev.smooth_track(beliefs, increments, GRID_EM, R_EM, **kw)
  with guarded.scope():
    stats = pev.track_statistics(beliefs, smoothed, increments, GRID_EM, R_EM, **kw)
  assert len(stats) == 2
  for t, st in enumerate(stats):
    assert set(st) == {'hist_k', 'hist_a', 'hist_b', 'stay', 'jump', 'log_norm', 'mass_kept', 'count', 'stats', 'taps'}
    taps = np_taps(increments[t + 1], GRID_EM, R_EM, kw['sigma_xy'], kw['sigma_yaw'])
    for a, b in zip(st['taps'], taps):
      assert (a == b) if isinstance(b, int) else (a.cpu().numpy().tobytes() == b.tobytes())
    args = (beliefs[t].cpu().numpy(), smoothed[t + 1].cpu().numpy(), taps, kw['uniform_mix'])
    got = tuple(st[k].cpu().numpy() for k in ('hist_k', 'hist_a', 'hist_b', 'stats', 'count'))
    _assert_within(got, ref.vote_pairs(*args), ref.bounds(*args), f'step {t}')
    assert float(st['stay']) == got[3][0] and float(st['jump']) == got[3][1] and abs(float(st['log_norm'])) <= 1e-4
  with pytest.raises(ValueError):
    pev.track_statistics(beliefs, smoothed[:2], increments, GRID_EM, R_EM, **kw)


def test_two_em_iterations_choose_the_references_candidates():
  """``fit_motion_noise`` for two iterations on six frames of the EM track: at each iteration's own starting values the
  reference E-step (numpy filter, smoother and tap posteriors) and ``noise_m_step`` give the reference's objective per
  candidate; the candidate the GPU fit chose has a reference objective within 1e-9 relative of the reference's best
  (equal-objective ties may differ in index)."""
  votes, increments, scale = _gpu_em_track(6)
  host_votes = em_track()[0][:6]
  fitted, records = pev.fit_motion_noise(votes, increments, GRID_EM, R_EM, START['sigma_xy'], START['sigma_yaw'],
                                         START['uniform_mix'], temperature=scale, iterations=2)
  assert len(records) == 2 and set(fitted) == {'sigma_xy', 'sigma_yaw', 'uniform_mix'}
  for i, r in enumerate(records):
    cur = dict(sigma_xy=r['sigma_xy'], sigma_yaw=r['sigma_yaw'], uniform_mix=r['uniform_mix'])
    stats, evidence = reference_e_step(host_votes, increments, scale, GRID_EM, R_EM, **cur)
    m = pev.noise_m_step(stats, increments, GRID_EM, R_EM, cur['sigma_xy'], cur['sigma_yaw'])
    print(f"iteration {i}: {cur}, log_evidence {r['log_evidence']:.6f} (reference {evidence:.6f}), jump {r['jump']:.3e}")
    assert abs(r['log_evidence'] - evidence) <= 1e-3 and abs(r['jump'] - m['jump']) <= 1e-4 * m['jump'] + 1e-12
    for name in ('sigma_xy', 'sigma_yaw'):
      assert r['m_step']['candidates'][name] == m['candidates'][name]
      obj = dict(zip(m['candidates'][name], m['objective'][name]))
      best, chosen = max(obj.values()), obj[r['m_step'][name]]
      print(f"  {name}: GPU chose {r['m_step'][name]:.6f}, the reference {m[name]:.6f}; objectives {chosen:.9f} / {best:.9f}")
      assert chosen >= best - 1e-9 * abs(best)
  last = records[-1]['m_step']
  assert fitted == dict(sigma_xy=last['sigma_xy'], sigma_yaw=last['sigma_yaw'], uniform_mix=last['uniform_mix'])


def test_fit_noise_leaves_the_filter_alone_without_apply():
  votes, increments, scale = _gpu_em_track(4)
  kw = dict(sigma_xy=START['sigma_xy'], sigma_yaw=START['sigma_yaw'], uniform_mix=START['uniform_mix'])
  track = pev.VoteFilter(GRID_EM, R_EM, temperature=scale, keep_history=True, **kw)
  plain = pev.VoteFilter(GRID_EM, R_EM, temperature=scale, **kw)
  with pytest.raises(ValueError):
    track.fit_noise(votes)                                     # no history yet
  for v, inc in zip(votes, increments):
    track.step(v, inc)
  with pytest.raises(ValueError):
    plain.fit_noise(votes)
  with pytest.raises(ValueError):
    track.fit_noise()                                          # the history keeps beliefs, not the volumes
  with pytest.raises(ValueError):
    track.fit_noise(votes[:3])
  belief, history = track.belief, list(track.history)
  fitted, records = track.fit_noise(votes, iterations=1)
  assert (track.sigma_xy, track.sigma_yaw, track.uniform_mix) == (kw['sigma_xy'], kw['sigma_yaw'], kw['uniform_mix'])
  assert track.belief is belief and track.history == history and len(records) == 1
  assert fitted['sigma_xy'] < kw['sigma_xy']                   # (the start is 3 x the planted noise)
  again, _ = track.fit_noise(votes, iterations=1, apply=True)
  assert again == fitted
  assert (track.sigma_xy, track.sigma_yaw, track.uniform_mix) == (fitted['sigma_xy'], fitted['sigma_yaw'],
                                                                  fitted['uniform_mix'])
  assert track.belief is belief
