"""`-m gpu`: ``ops.vote_viterbi`` / ``ops.vote_backstep`` (vote_viterbi.hip, through the C ABI) and the host entry points
built on them, against the numpy f32 restatement ``vote_viterbi_reference`` BIT FOR BIT: ``score_out`` compared as
int32 words (the -inf cells identical), ``back``, ``stats`` and ``count`` exactly.  There is no tolerance: the contract
is f32 additions, products and comparisons only.

The cases are the filter tests' shapes (``vote_viterbi_reference.all_inputs``): ``tiny`` [1, 1, 1]; ``first``
(score_prev = NULL); ``wrap`` / ``wrap_far`` / ``wrap_neg`` [4, 7, 7], Tk = 3 with lk = -1, R + 2, -3 R - 2; ``tk16``
[5, 6, 9]; ``ragged`` [36, 31, 33] (four tiles per rotation, the last ragged, -inf log-taps, offsets of both signs, two
rotations whose taps all fall outside, 30 % -inf cells); ``wide`` [2, 20, 300] Tb = 32; ``tall`` [2, 300, 20] Ta = 32;
``tiles`` [2, 520, 520]: 2114 tiles on 2048 workgroups; ``ties``; ``jump_only``; ``no_jump_outside``; ``stay_off``;
``bad``; ``empty``.  Every call runs under ``guarded.scope()``: guard regions intact (outputs and workspace), no output
element left unwritten, the workspace the size ``snap_vote_viterbi_workspace_bytes`` states."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_viterbi_reference as ref
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
  return c['score_prev'], c['votes'], c['ltaps'], c['scale'], c['log_stay'], c['log_jump']


@functools.lru_cache(maxsize=None)
def _want(name):
  return ref.vote_viterbi(*_args(_inputs()[name]))


def _dev(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_taps(taps, place=False):
  tk, lk, ta, tb, off = taps
  put = (lambda t, kind: guarded.place(t, kind)) if place else (lambda t, kind: t)
  return (put(_dev(tk), 'value'), int(lk), put(_dev(ta), 'value'), put(_dev(tb), 'value'), put(_dev(off), 'address'))


def _run(score_prev, votes, ltaps, scale, log_stay, log_jump):
  """One guarded call -> numpy (score_out, back, stats, count)."""
  R, Ho, Wo = votes.shape
  with guarded.scope() as sc:
    prev = None if score_prev is None else guarded.place(_dev(score_prev), 'value')
    out = ops.vote_viterbi(prev, guarded.place(_dev(votes), 'value'), _dev_taps(ltaps, place=True), scale, log_stay,
                           log_jump)
    assert [tuple(o.shape) for o in out] == [(R, Ho, Wo), (R, Ho, Wo), (2,), (6,)]
    assert [o.dtype for o in out] == [torch.float32, torch.int32, torch.float32, torch.int32]
    ws = [a for a in sc.allocations('vote_viterbi') if a.dtype == torch.int64]
    need = _lib.load().snap_vote_viterbi_workspace_bytes(R, Ho, Wo, len(ltaps[0]), ltaps[2].shape[1], ltaps[3].shape[1])
    assert len(ws) == 1 and ws[0].numel() * 8 == need
    # (-1 in back and count is the poison's own pattern: those two are covered by the exact comparison below, which a
    # poisoned element fails wherever the reference is not -1, and by test_back_is_written_over_other_values)
    for o, what in zip((out[0], out[2]), ('score_out', 'stats')):
      assert not bool(guarded.unwritten(o).any()), f'{what}: elements never written'
    res = tuple(o.cpu().numpy() for o in out)
  return res


def _assert_same(got, want, what):
  (g, gb, gs, gc), (w, wb, ws, wc) = got, want
  print(f'{what}: stats {gs.tolist()} count {gc.tolist()}')
  assert gc.tolist() == wc.tolist(), f'{what}: count {gc.tolist()} != {wc.tolist()}'
  assert (gs.view(np.int32) == ws.view(np.int32)).all(), f'{what}: stats {gs.tolist()} != {ws.tolist()}'
  differ = g.view(np.int32) != w.view(np.int32)
  assert not differ.any(), f'{what}: {int(differ.sum())} cells of score_out differ in their bits'
  assert (gb == wb).all(), f'{what}: {int((gb != wb).sum())} cells of back differ'


CASES = ['tiny', 'first', 'wrap', 'wrap_far', 'wrap_neg', 'tk16', 'ragged', 'wide', 'tall', 'tiles', 'ties',
         'jump_only', 'no_jump_outside', 'stay_off', 'bad', 'empty']


@pytest.mark.parametrize('name', CASES)
def test_against_the_reference_bit_for_bit(name):
  assert set(CASES) == set(_inputs())
  got = _run(*_args(_inputs()[name]))
  _assert_same(got, _want(name), name)
  score, back, stats, count = got
  n = score.size
  if name == 'ties':
    assert (back.reshape(-1) == np.arange(n)).all() and count.tolist() == [n, 0, 0, 0, 0, 0]
  if name == 'jump_only':
    assert (back == count[4]).all() and count[3] == n
  if name == 'no_jump_outside':
    assert (score == -np.inf).all() and (back == -1).all() and count[5] == -1 and stats[1] == -np.inf
  if name == 'first':
    assert (back == -1).all() and stats[0] == -np.inf and count[4] == -1


def _raw_call(lib, c, dev, ws, nbytes, out):
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
  prev, votes, taps = dev
  R, Ho, Wo = votes.shape
  return lib.snap_vote_viterbi_f32(p(prev), p(votes), p(taps[0]), taps[1], p(taps[2]), p(taps[3]), p(taps[4]), R, Ho, Wo,
                                   taps[0].shape[0], taps[2].shape[1], taps[3].shape[1], c['scale'], c['log_stay'],
                                   c['log_jump'], p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(ws), nbytes,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_two_calls_give_identical_bytes_and_every_output_is_overwritten():
  """Also with garbage in the workspace and with outputs pre-filled by a value that is not the guard's poison (back
  and count legitimately hold -1, the poison's pattern in int32)."""
  lib = _lib.load()
  for name in ('ragged', 'bad', 'tiles', 'first', 'no_jump_outside'):
    c = _inputs()[name]
    dev = (_dev(c['score_prev']), _dev(c['votes']), _dev_taps(c['ltaps']))
    first = ops.vote_viterbi(dev[0], dev[1], dev[2], c['scale'], c['log_stay'], c['log_jump'])
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_viterbi(dev[0], dev[1], dev[2], c['scale'], c['log_stay'], c['log_jump'])
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    R, Ho, Wo = dev[1].shape
    nbytes = lib.snap_vote_viterbi_workspace_bytes(R, Ho, Wo, dev[2][0].shape[0], dev[2][2].shape[1], dev[2][3].shape[1])
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    outs = []
    for fill in (-1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = (torch.full((R, Ho, Wo), 7.0, device=DEV), torch.full((R, Ho, Wo), 7, dtype=torch.int32, device=DEV),
           torch.full((2,), 7.0, device=DEV), torch.full((6,), 7, dtype=torch.int32, device=DEV))
      assert _raw_call(lib, c, dev, ws, nbytes, o) == 0
      outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name


def test_bad_arguments_raise_without_launching():
  R, Ho, Wo = 4, 5, 6
  votes = torch.zeros((R, Ho, Wo), device=DEV)
  prev = torch.zeros((R, Ho, Wo), device=DEV)
  tk, ta, tb = -torch.ones(2, device=DEV), -torch.ones((R, 3), device=DEV), -torch.ones((R, 2), device=DEV)
  off = torch.zeros((R, 2), dtype=torch.int32, device=DEV)
  good = (tk, 0, ta, tb, off)
  ops.vote_viterbi(prev, votes, good, 1.0, -0.1, -5.0)
  for taps in ((tk.double(), 0, ta, tb, off), (tk, 0.5, ta, tb, off), (tk, 0, ta[:3], tb, off),
               (torch.zeros(17, device=DEV), 0, ta, tb, off), (tk, 0, torch.zeros((R, 33), device=DEV), tb, off),
               (tk, 0, ta, tb)):
    with pytest.raises(ValueError):
      ops.vote_viterbi(prev, votes, taps)
  for kw in (dict(scale=0.0), dict(scale=float('inf')), dict(scale=float('nan')), dict(log_jump=0.5),
             dict(log_stay=1e-3), dict(log_stay=float('nan')), dict(log_jump=float('nan'))):
    with pytest.raises(ValueError):
      ops.vote_viterbi(prev, votes, good, **kw)
  for b, v in ((prev[:3], votes), (prev.double(), votes), (prev.cpu(), votes), (prev, votes[0]), (None, votes.cpu())):
    with pytest.raises(ValueError):
      ops.vote_viterbi(b, v, good)
  for back, cur in ((torch.zeros((R, Ho, Wo), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)),
                    (torch.zeros((R, Ho, Wo), dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)),
                    (torch.zeros((R, Ho, Wo), dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)),
                    (torch.zeros((R, Ho, Wo), dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32))):
    with pytest.raises(ValueError):
      ops.vote_backstep(back, cur)
  lib = _lib.load()
  wsb = lib.snap_vote_viterbi_workspace_bytes
  assert wsb(0, 5, 6, 2, 3, 2) == 0 and wsb(65, 5, 6, 2, 3, 2) == 0 and wsb(4, 0, 6, 2, 3, 2) == 0
  assert wsb(4, 5, 6, 0, 3, 2) == 0 and wsb(4, 5, 6, 17, 3, 2) == 0 and wsb(4, 5, 6, 2, 33, 2) == 0
  assert wsb(4, 5, 6, 2, 3, 0) == 0 and wsb(64, 4096, 8192, 2, 3, 2) == 0          # R Ho Wo = 2^31
  need = wsb(R, Ho, Wo, 2, 3, 2)
  # m1, two byte volumes, and 4 workgroups' partials (2 f32 and 6 int32 each)
  assert need == R * Ho * Wo * 4 + 2 * R * Ho * Wo + 4 * (2 * 4 + 6 * 4)
  ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
  out = torch.full((R, Ho, Wo), 7.0, device=DEV)
  back = torch.full((R, Ho, Wo), 7, dtype=torch.int32, device=DEV)
  stats = torch.full((2,), 7.0, device=DEV)
  count = torch.full((6,), 7, dtype=torch.int32, device=DEV)
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

  def call(R_=R, Tk=2, Ta=3, Tb=2, scale=1.0, ls=-0.1, lj=-5.0, nbytes=need, votes_=votes, wsp=None, back_=back):
    return lib.snap_vote_viterbi_f32(p(prev), p(votes_), p(tk), 0, p(ta), p(tb), p(off), R_, Ho, Wo, Tk, Ta, Tb, scale,
                                     ls, lj, p(out), p(back_), p(stats), p(count), wsp if wsp is not None else p(ws),
                                     nbytes, None)

  assert call(R_=0) == -1 and call(R_=65, nbytes=1 << 30) == -1 and call(Tk=17) == -1 and call(Ta=0) == -1
  assert call(Tb=33) == -1
  assert call(votes_=None) == -3 and call(back_=None) == -3 and call(R_=65, votes_=None) == -3
  assert call(scale=0.0) == -2 and call(scale=float('inf')) == -2 and call(lj=0.5) == -2 and call(ls=float('nan')) == -2
  assert call(nbytes=need - 1) == -5 and call(wsp=ctypes.c_void_p(ws.data_ptr() + 4)) == -5
  cur = torch.zeros(1, dtype=torch.int32, device=DEV)
  prv = torch.full((1,), 7, dtype=torch.int32, device=DEV)
  bs = lib.snap_vote_backstep_i32
  assert bs(None, 5, p(cur), p(prv), 1, None) == -3 and bs(p(back), 5, p(cur), None, 1, None) == -3
  assert bs(p(back), 0, p(cur), p(prv), 1, None) == -1 and bs(p(back), 5, p(cur), p(prv), 0, None) == -1
  torch.cuda.synchronize()
  assert bool((out == 7).all()) and bool((back == 7).all()) and bool((stats == 7).all()) and bool((count == 7).all())
  assert bool((prv == 7).all())                                                     # nothing ran


# ---------------------------------------------------------------------------------------------------------------
# the track: four synthetic frames on a small grid
# ---------------------------------------------------------------------------------------------------------------
H, D, R, N = 16, 8, 8, 4
KW = dict(sigma_xy=0.2, sigma_yaw=0.15, temperature=4.0, uniform_mix=1e-3)


def _increments():
  t = lambda a, x, y: geometry.Transform2D(torch.tensor(a, dtype=torch.float64), torch.tensor([x, y], dtype=torch.float64))
  return [None, t(0.12, 0.3, -0.2), t(-0.2, -0.4, 0.15), None]


@functools.lru_cache(maxsize=None)
def _scene():
  """-> (grid, volumes [N] device f32 [R, 2H-1, 2H-1], increments, the reference's steps): the frames' votes come from
  ``exhaustive_pose_voting`` once and are shared; the reference runs on their bits with ``motion_log_taps``' tables."""
  rng = np.random.default_rng(4321)
  grid = grids.Grid2D((H, H), 0.25)
  valid = torch.ones((H, H), dtype=torch.bool, device=DEV)
  plane = lambda: types.FeaturePlane(features=torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV),
                                     valid=valid)
  pm = plane()
  planes = [plane() for _ in range(N)]
  volumes = [pev.exhaustive_pose_voting(pq, pm, R, grid) for pq in planes]
  incs = _increments()
  ltaps = [None]
  for inc in incs[1:]:
    taps = pev.motion_log_taps(inc if inc is not None else pev._no_motion(), grid, R, KW['sigma_xy'], KW['sigma_yaw'])
    ltaps.append(tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in taps))
  steps = ref.track([v.cpu().numpy() for v in volumes], ltaps, KW['temperature'], KW['uniform_mix'])
  return grid, volumes, incs, steps, (planes, pm)


def _assert_path(got, steps, grid, end=None):
  linear, jumps, total = ref.trace(steps, end)
  assert got['linear'].dtype == torch.int32 and got['indices'].dtype == torch.int32 and got['jumps'].dtype == torch.bool
  assert got['linear'].cpu().tolist() == linear.tolist()
  assert got['jumps'].cpu().tolist() == jumps.tolist()
  shape = steps[0]['score'].shape
  want_idx = np.stack(np.unravel_index(linear, shape), -1)
  assert got['indices'].cpu().tolist() == want_idx.tolist() and (linear >= 0).all()
  assert got['log_score'].dtype == torch.float64
  # N float64 additions of numbers below 2^7 in magnitude
  assert abs(float(got['log_score']) - total) <= N * 2.0 ** -52 * 128
  tfm = pev.exhaustive_indices_to_tfm(got['indices'], grid, R)
  assert guarded.same_bits(got['m_t_q'].angle, tfm.angle) and guarded.same_bits(got['m_t_q'].t, tfm.t)


def test_viterbi_track_and_the_class_follow_the_reference_chain():
  grid, volumes, incs, steps, (planes, pm) = _scene()
  with guarded.scope():
    out = pev.viterbi_track(volumes, incs, grid, R, **KW)
  assert set(out) == {'indices', 'linear', 'm_t_q', 'log_score', 'jumps'}
  _assert_path(out, steps, grid)
  track = pev.VoteViterbi(grid, R, **KW)
  for n in range(N):
    with guarded.scope():
      loc = track.localize(planes[n], pm, incs[n], num_peaks=4)
    assert loc['votes'] is track.score and guarded.same_bits(loc['votes_frame'], volumes[n])
    s = steps[n]
    assert (loc['votes'].cpu().numpy().view(np.int32) == s['score'].view(np.int32)).all(), n
    assert (loc['back'].cpu().numpy() == s['back']).all(), n
    assert track.history[-1]['count'].cpu().tolist() == s['count'].tolist()
    peaks = pev.poses_from_votes(track.score, grid, R, num_peaks=4)
    assert guarded.same_bits(peaks['index'], loc['index'])
  _assert_path(track.path(), steps, grid)
  # B alternatives at once: the peaks of the last score
  P = (2 * H - 1) ** 2
  idx = peaks['index'].long()
  ends = (idx[:, 0] * P + idx[:, 1] * (2 * H - 1) + idx[:, 2]).to(torch.int32)
  many = track.path(ends)
  assert tuple(many['linear'].shape) == (N, 4) and tuple(many['indices'].shape) == (N, 4, 3)
  for i, e in enumerate(ends.cpu().tolist()):
    linear, jumps, total = ref.trace(steps, e)
    assert many['linear'][:, i].cpu().tolist() == linear.tolist() and many['jumps'][:, i].cpu().tolist() == jumps.tolist()
    assert abs(float(many['log_score'][i]) - total) <= N * 2.0 ** -52 * 128
  track.reset()
  assert track.score is None and track.history == []


def test_vote_backstep_one_and_many_chains():
  grid, volumes, incs, steps, _ = _scene()
  back = [_dev(s['back']) for s in steps]
  n = steps[0]['back'].size
  for cur in ([int(steps[-1]['count'][5])], [3, -1, n, n - 1, int(steps[-1]['count'][5])]):
    chain = np.array(cur, np.int32)
    for t in range(N - 1, 0, -1):
      with guarded.scope():
        got = ops.vote_backstep(back[t], _dev(chain))
        assert got.dtype == torch.int32 and tuple(got.shape) == (len(cur),)
      want = ref.vote_backstep(steps[t]['back'], chain)
      assert got.cpu().tolist() == want.tolist()
      chain = want
    if len(cur) == 5:
      assert chain[1] == -1 and chain[2] == -1                # a cur of -1 and of n: no predecessor, and it stays so
