"""`-m gpu`: ``ops.vote_sample`` / ``ops.vote_sample_back`` (vote_sample.hip, through the C ABI) and the host entry points
built on them, against the dense float64 restatement ``vote_sample_reference``.

With the uniforms GIVEN every draw is checked for membership: the returned cell has mass and u Z lies in the cell's
interval of the reference's CDF widened by TOL Z, TOL = 2^-22 (derived in the reference's docstring: one f32 ulp on
every mass, n 2^-53 on every float64 sum).  The Philox path must give the bytes of the path with the reference's
Philox uniforms given.  The seeded statistics run end to end through ``VoteFilter.sample``; their bound is the
reference sampler's own largest |z| plus 1 (test_vote_sample_reference.py).  Every call runs under ``guarded.scope()``:
guard regions intact, no output element left unwritten, the workspace exactly the stated size."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_sample_reference as ref
from test_vote_sample_reference import STAT_SEED, STAT_TRACKS, Z_REFERENCE
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE


@functools.lru_cache(maxsize=None)
def _sample_cases():
  return {c['name']: c for c in ref.sample_inputs()}


@functools.lru_cache(maxsize=None)
def _back_cases():
  return {c['name']: c for c in ref.back_inputs()}


@functools.lru_cache(maxsize=None)
def _model(name):
  c = _sample_cases()[name]
  return ref.model(c['votes'], c['scale'])


@functools.lru_cache(maxsize=None)
def _back_model(name):
  c = _back_cases()[name]
  return ref.back_model(c['belief'], c['taps'], c['eps'])


def _dev(a):
  return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_taps(taps, place=False):
  tk, lk, ta, tb, off = taps
  put = (lambda t, kind: guarded.place(t, kind)) if place else (lambda t, kind: t)
  return (put(_dev(tk), 'value'), int(lk), put(_dev(ta), 'value'), put(_dev(tb), 'value'), put(_dev(off), 'address'))


def _written(outs, names):
  """No element still holds the poison.  (-1 in an int32 output IS the poison's pattern: those outputs are covered by
  the membership / equality checks, which a poisoned element fails wherever -1 is not the answer, and by the
  determinism test's pre-filled outputs.)"""
  for o, what in zip(outs, names):
    if o.dtype == torch.float32:
      assert not bool(guarded.unwritten(o).any()), f'{what}: elements never written'


def _sample(votes, num, seed, stream, scale, uni):
  """One guarded call -> numpy (index, log_prob, stats, count)."""
  R, Ho, Wo = votes.shape
  with guarded.scope() as sc:
    u = None if uni is None else guarded.place(_dev(np.stack([uni, uni], -1)), 'value')
    out = ops.vote_sample(guarded.place(_dev(votes), 'value'), num, seed, stream, scale, u)
    assert [tuple(o.shape) for o in out] == [(num,), (num,), (2,), (2,)]
    assert [o.dtype for o in out] == [torch.int32, torch.float32, torch.float32, torch.int32]
    ws = [a for a in sc.allocations('vote_sample') if a.dtype == torch.int64]
    assert len(ws) == 1 and ws[0].numel() * 8 == _lib.load().snap_vote_sample_workspace_bytes(R, Ho, Wo)
    _written(out[1:3], ('log_prob', 'stats'))
    res = tuple(o.cpu().numpy() for o in out)
  return res


def _sample_back(belief, nxt, taps, eps, seed, stream, uni):
  """One guarded call -> numpy (prev, jumped, stats, count)."""
  R, Ho, Wo = belief.shape
  B = len(nxt)
  with guarded.scope() as sc:
    u = None if uni is None else guarded.place(_dev(uni), 'value')
    out = ops.vote_sample_back(guarded.place(_dev(belief), 'value'), guarded.place(_dev(nxt.astype(np.int32)), 'address'),
                               _dev_taps(taps, place=True), eps, seed, stream, u)
    assert [tuple(o.shape) for o in out] == [(B,), (B,), (2,), (3,)]
    assert [o.dtype for o in out] == [torch.int32, torch.int32, torch.float32, torch.int32]
    ws = [a for a in sc.allocations('vote_sample_back') if a.dtype == torch.int64]
    need = _lib.load().snap_vote_sample_back_workspace_bytes(R, Ho, Wo, len(taps[0]), taps[2].shape[1], taps[3].shape[1])
    assert len(ws) == 1 and ws[0].numel() * 8 == need
    _written(out[2:3], ('stats',))
    res = tuple(o.cpu().numpy() for o in out)
  return res


SAMPLE_CASES = ['tiny', 'small', 'ragged', 'wide', 'tall', 'tiles', 'one_cell', 'no_mass', 'scaled']


@pytest.mark.parametrize('name', SAMPLE_CASES)
def test_every_draw_is_a_member_of_its_cdf_interval(name):
  assert set(SAMPLE_CASES) == set(_sample_cases())
  c, m = _sample_cases()[name], _model(name)
  u = ref.given_uniforms(m, np.random.default_rng(len(name)))
  idx, lp, stats, count = _sample(c['votes'], len(u), 1, 0, c['scale'], u)
  want = ref.vote_sample(c['votes'], len(u), 1, 0, c['scale'], np.stack([u, u], -1))
  print(f'{name}: {len(u)} draws, {int((idx != want[0]).sum())} differ from the dense answer; stats {stats.tolist()} '
        f'count {count.tolist()}')
  assert count.tolist() == want[3].tolist()
  assert stats[1] == np.float32(want[2][1])
  if not m['Z'] > 0:
    assert (idx == -1).all() and (lp == -np.inf).all() and stats[0] == -np.inf
    return
  ok = ref.member(m, idx, u)
  assert ok.all(), f'{name}: draws {np.nonzero(~ok)[0].tolist()} outside their interval: u {u[~ok]}, cells {idx[~ok]}'
  # log_prob of the RETURNED cell: one f32 rounding of a float64 expression whose log Z is off by at most 2^-22
  lp_want = (m['s'][idx].astype(np.float64) - float(m['M'])) - np.log(m['Z'])
  assert (np.abs(lp - lp_want) <= 2.0 ** -22 + 2.0 ** -23 * np.abs(lp_want)).all()
  assert abs(stats[0] - want[2][0]) <= 2.0 ** -22 + 2.0 ** -23 * abs(want[2][0])
  if name == 'one_cell':
    assert (idx == np.nonzero(m['p'])[0][0]).all() and (lp == 0).all()


def test_stratified_counts_are_within_one():
  """[3, 4, 5], u_i = (i + 0.5) / 3840: every cell's count is within 1 of 3840 p (the uniforms are 1 / B apart, far
  wider than the rounding slack, so this is exact)."""
  rng = np.random.default_rng(9)
  votes = (rng.standard_normal((3, 4, 5)) * 1.5).astype(np.float32)
  votes[1, 2, 3] = -np.inf
  B = 3840
  u = (np.arange(B) + 0.5) / B
  idx = _sample(votes, B, 0, 0, 1.0, u)[0]
  m = ref.model(votes, 1.0)
  counts = np.bincount(idx, minlength=60)
  assert (np.abs(counts - B * m['p'] / m['Z']) <= 1.0).all() and counts[np.ravel_multi_index((1, 2, 3), (3, 4, 5))] == 0
  assert (np.diff(idx) >= 0).all()                          # the inverse CDF is monotone in u


BACK_CASES = ['wrap', 'wrap_far', 'wrap_neg', 'tk16', 'ragged', 'wide', 'never_jumps', 'always_jumps']


def _back_uniforms(bm, nxt, rng):
  """(u0, u1) per chain: random, with the edges 0 and 1 - 2^-53 and, for some, u0 exactly on the branch boundary."""
  uni = rng.random((len(nxt), 2))
  uni[4] = (0.0, 0.0)
  uni[5] = (1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53)
  for i in range(6, min(12, len(nxt))):
    _, _, W, A, J = ref.window(bm, int(nxt[i]))
    if A + J > 0:
      uni[i, 0] = min(J / (A + J), 1.0 - 2.0 ** -53)
  return uni


@pytest.mark.parametrize('name', BACK_CASES)
def test_backward_step_branch_and_predecessor(name):
  assert set(BACK_CASES) == set(_back_cases())
  c, bm = _back_cases()[name], _back_model(name)
  rng = np.random.default_rng(len(name) + 100)
  nxt = ref.back_chains(bm, rng, 60)
  if name == 'never_jumps':                                 # rotation 5: every row source is below the volume
    nxt = np.concatenate([nxt, [np.ravel_multi_index((5, 10, 10), bm['shape'])]])
  uni = _back_uniforms(bm, nxt, rng)
  prev, jumped, stats, count = _sample_back(c['belief'], nxt, c['taps'], c['eps'], 1, 0, uni)
  want = ref.vote_sample_back(c['belief'], nxt, c['taps'], c['eps'], 1, 0, uni)
  print(f'{name}: {len(nxt)} chains, {int((prev != want[0]).sum())} differ from the dense answer, '
        f'{int((jumped == 1).sum())} jumps; stats {stats.tolist()} count {count.tolist()}')
  for i, x in enumerate(nxt):
    ok, why = ref.back_admissible(bm, int(x), uni[i, 0], uni[i, 1], int(prev[i]), int(jumped[i]))
    assert ok, f'{name}: chain {i} at {x}: prev {prev[i]} jumped {jumped[i]}: {why}'
  assert prev[2] == -1 and prev[3] == -1 and jumped[2] == -1 and jumped[3] == -1      # next = -1 and next = n
  assert count.tolist() == [(prev >= 0).sum(), (jumped == 1).sum(), bm['bad']]
  assert stats[1] == np.float32(bm['M'])
  # S / sum p: the filter's own bound for this statistic
  import vote_filter_reference as flt
  assert abs(stats[0] - bm['kept']) <= flt.stats_bound(c['belief'], c['belief'], c['taps'], 1.0, c['eps'])[1]
  if name == 'never_jumps':
    assert (jumped <= 0).all() and prev[-1] == -1 and jumped[-1] == -1
  if name == 'always_jumps':
    inside = (nxt >= 0) & (nxt < bm['n'])
    assert (jumped[inside] == 1).all()


def test_predict_statistics_are_the_filters_bits_in_all_four_operators():
  """``vote_filter``, ``vote_smooth``, ``vote_pairs`` and ``vote_sample_back`` run one predict step (vote_predict.h) on
  the same belief and taps: ``mass_kept`` has the same f32 bits from all four (pairs' float64 holds that f32) and the
  peak the same bits from the filter and the sampler.  [5, 7, 9]: a ragged last tile of 63 cells, more rotations than
  waves; offsets that push taps off the volume on every side, so some mass is lost."""
  rng = np.random.default_rng(41)
  R, Ho, Wo = 5, 7, 9
  belief = (rng.standard_normal((R, Ho, Wo)) * 3.0).astype(np.float32)
  belief[rng.random((R, Ho, Wo)) < 0.1] = -np.inf
  votes = rng.standard_normal((R, Ho, Wo)).astype(np.float32)
  norm = lambda t: (t / t.sum(-1, keepdims=True)).astype(np.float32)
  taps = (norm(rng.random(3) + 0.1), 4, norm(rng.random((R, 2)) + 0.1), norm(rng.random((R, 4)) + 0.1),
          np.array([[-3, 2], [2, -5], [0, 7], [6, -1], [-1, 0]], np.int32))
  eps = 1e-3
  b, t = _dev(belief), _dev_taps(taps)
  nxt = _dev(np.arange(0, R * Ho * Wo, 7, dtype=np.int32))
  with guarded.scope():
    filtered, f_stats, _ = ops.vote_filter(b, _dev(votes), t, 1.0, eps)
    s_stats = ops.vote_smooth(b, filtered, t, eps)[1]
    p_stats = ops.vote_pairs(b, filtered, t, eps)[3]
    b_stats = ops.vote_sample_back(b, nxt, t, eps, 3)[2]
    f_stats, s_stats, p_stats, b_stats = (x.cpu().numpy() for x in (f_stats, s_stats, p_stats, b_stats))
  bits = lambda v: int(np.float32(v).view(np.int32))
  kept = [bits(f_stats[1]), bits(s_stats[1]), bits(p_stats[3]), bits(b_stats[0])]
  print(f'mass_kept {f_stats[1]!r}: bits {[hex(k) for k in kept]}; peak {f_stats[2]!r} / {b_stats[1]!r}')
  assert p_stats.dtype == np.float64 and float(np.float32(p_stats[3])) == p_stats[3]
  assert len(set(kept)) == 1
  assert bits(f_stats[2]) == bits(b_stats[1]) and f_stats[2] == belief[np.isfinite(belief)].max()
  assert 0.0 < f_stats[1] < 1.0


def test_philox_path_is_the_uniforms_path():
  """uniforms=None against the reference's Philox uniforms for the same (seed, stream), given: identical bytes."""
  seed = 0x0123456789ABCDEF
  for name, stream in (('ragged', 7), ('small', -2), ('no_mass', 0)):
    c = _sample_cases()[name]
    B = 777
    a = _sample(c['votes'], B, seed, stream, c['scale'], None)
    with guarded.scope():
      b = ops.vote_sample(_dev(c['votes']), B, seed, stream, c['scale'], _dev(ref.uniforms(B, seed, stream, 0)))
    assert (a[0] == b[0].cpu().numpy()).all(), name
    assert (a[1].view(np.int32) == b[1].cpu().numpy().view(np.int32)).all(), name
    assert name == 'no_mass' or len(set(a[0].tolist())) >= 10       # (draws, not one cell)
  for name, stream in (('ragged', 3), ('tk16', -1)):
    c, bm = _back_cases()[name], _back_model(name)
    nxt = ref.back_chains(bm, np.random.default_rng(5), 300)
    a = _sample_back(c['belief'], nxt, c['taps'], c['eps'], seed, stream, None)
    b = _sample_back(c['belief'], nxt, c['taps'], c['eps'], seed, stream, ref.uniforms(len(nxt), seed, stream, 1))
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[3].tolist() == b[3].tolist(), name
    other = _sample_back(c['belief'], nxt, c['taps'], c['eps'], seed, stream + 1, None)
    assert (a[0] != other[0]).any(), name                           # the stream is part of the counter


def _raw_sample(lib, votes, scale, B, seed, stream, uni, out, ws, nbytes, R=None):
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
  R_, Ho, Wo = votes.shape
  return lib.snap_vote_sample_f32(p(votes), R_ if R is None else R, Ho, Wo, scale, B, seed, stream, p(uni), p(out[0]),
                                  p(out[1]), p(out[2]), p(out[3]), ws, nbytes, None)


def _raw_back(lib, belief, taps, eps, nxt, B, seed, stream, uni, out, ws, nbytes, **kw):
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
  R, Ho, Wo = belief.shape
  a = dict(belief_ptr=p(belief), R=R, Tk=taps[0].shape[0], Ta=taps[2].shape[1], Tb=taps[3].shape[1])
  a.update(kw)
  return lib.snap_vote_sample_back_f32(a['belief_ptr'], p(taps[0]), taps[1], p(taps[2]), p(taps[3]), p(taps[4]), a['R'], Ho,
                                       Wo, a['Tk'], a['Ta'], a['Tb'], eps, p(nxt), B, seed, stream, p(uni), p(out[0]),
                                       p(out[1]), p(out[2]), p(out[3]), ws, nbytes, None)


def _fresh_outputs(B, ncount):
  return (torch.full((B,), 7, dtype=torch.int32, device=DEV),
          torch.full((B,), 7.0 if ncount == 2 else 7, dtype=torch.float32 if ncount == 2 else torch.int32, device=DEV),
          torch.full((2,), 7.0, device=DEV), torch.full((ncount,), 7, dtype=torch.int32, device=DEV))


def test_two_calls_give_identical_bytes_and_every_output_is_overwritten():
  """Also with garbage in the workspace and with outputs pre-filled by a value that is not the guard's poison."""
  lib = _lib.load()
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  for name in ('ragged', 'tiles', 'no_mass'):
    c = _sample_cases()[name]
    votes, B = _dev(c['votes']), 500
    first = ops.vote_sample(votes, B, 11, 2, c['scale'])
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_sample(votes, B, 11, 2, c['scale'])
    nbytes = lib.snap_vote_sample_workspace_bytes(*votes.shape)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    outs = [second]
    for fill in (-1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = _fresh_outputs(B, 2)
      assert _raw_sample(lib, votes, c['scale'], B, 11, 2, None, o, p(ws), nbytes) == 0
      outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name
  for name in ('ragged', 'wrap_neg'):
    c, bm = _back_cases()[name], _back_model(name)
    belief, taps = _dev(c['belief']), _dev_taps(c['taps'])
    nxt = _dev(ref.back_chains(bm, np.random.default_rng(6), 200).astype(np.int32))
    B = nxt.numel()
    first = ops.vote_sample_back(belief, nxt, taps, c['eps'], 11, 2)
    second = ops.vote_sample_back(belief, nxt, taps, c['eps'], 11, 2)
    nbytes = lib.snap_vote_sample_back_workspace_bytes(*belief.shape, taps[0].shape[0], taps[2].shape[1], taps[3].shape[1])
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    outs = [second]
    for fill in (-1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = _fresh_outputs(B, 3)
      assert _raw_back(lib, belief, taps, c['eps'], nxt, B, 11, 2, None, o, p(ws), nbytes) == 0
      outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name


def test_bad_arguments_return_their_codes_without_launching():
  lib = _lib.load()
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  R, Ho, Wo, B = 4, 5, 6, 8
  votes = torch.zeros((R, Ho, Wo), device=DEV)
  wsb = lib.snap_vote_sample_workspace_bytes
  assert wsb(0, 5, 6) == 0 and wsb(65, 5, 6) == 0 and wsb(4, 0, 6) == 0 and wsb(4, 5, 0) == 0
  assert wsb(64, 4096, 8192) == 0                                                   # R Ho Wo = 2^31
  need = wsb(R, Ho, Wo)
  # 4 workgroups' partials (f32, int32), 20 row sums and counts, 64 plane sums, 4 totals
  assert need == 4 * 4 + 4 * 4 + 20 * 8 + 20 * 4 + 64 * 8 + 4 * 8
  ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
  out = _fresh_outputs(B, 2)
  call = lambda B_=B, scale=1.0, nbytes=need, wsp=None, R_=None, v=votes, o=out: _raw_sample(
      lib, v, scale, B_, 1, 0, None, o, wsp if wsp is not None else p(ws), nbytes, R_)
  assert call(R_=0) == -1 and call(R_=65, nbytes=1 << 30) == -1 and call(B_=0) == -1 and call(B_=(1 << 20) + 1) == -1
  assert call(scale=0.0) == -2 and call(scale=float('inf')) == -2 and call(scale=float('nan')) == -2
  assert call(nbytes=need - 1) == -5 and call(wsp=ctypes.c_void_p(ws.data_ptr() + 4)) == -5
  assert lib.snap_vote_sample_f32(None, R, Ho, Wo, 1.0, B, 1, 0, None, p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(ws),
                                  need, None) == -3
  assert lib.snap_vote_sample_f32(p(votes), 0, Ho, Wo, 1.0, B, 1, 0, None, None, p(out[1]), p(out[2]), p(out[3]), p(ws),
                                  need, None) == -3                                 # NULL is checked first
  tk, ta, tb = torch.ones(2, device=DEV) / 2, torch.ones((R, 3), device=DEV) / 3, torch.ones((R, 2), device=DEV) / 2
  taps = (tk, 0, ta, tb, torch.zeros((R, 2), dtype=torch.int32, device=DEV))
  nxt = torch.zeros(B, dtype=torch.int32, device=DEV)
  bwsb = lib.snap_vote_sample_back_workspace_bytes
  assert bwsb(0, 5, 6, 2, 3, 2) == 0 and bwsb(4, 5, 6, 17, 3, 2) == 0 and bwsb(4, 5, 6, 2, 33, 2) == 0
  assert bwsb(4, 5, 6, 2, 3, 0) == 0 and bwsb(64, 4096, 8192, 2, 3, 2) == 0
  bneed = bwsb(R, Ho, Wo, 2, 3, 2)
  # two volumes, 4 workgroups' partials (f32; 2 int32; 2 float64), 20 row sums, 64 plane sums, 4 totals
  assert bneed == 2 * R * Ho * Wo * 4 + 4 * 4 + 4 * 8 + 4 * 16 + 20 * 8 + 64 * 8 + 4 * 8
  bws = torch.empty(bneed // 8 + 1, dtype=torch.int64, device=DEV)
  bout = _fresh_outputs(B, 3)
  back = lambda eps=0.1, B_=B, nbytes=bneed, wsp=None, **kw: _raw_back(
      lib, votes, taps, eps, nxt, B_, 1, 0, None, bout, wsp if wsp is not None else p(bws), nbytes, **kw)
  assert back(belief_ptr=None) == -3 and back(belief_ptr=None, R=0) == -3                   # a NULL belief; NULL comes first
  assert back(R=0) == -1 and back(Tk=17) == -1 and back(Ta=0) == -1 and back(Tb=33) == -1
  assert back(B_=0) == -1 and back(B_=(1 << 20) + 1) == -1
  assert back(eps=-0.1) == -2 and back(eps=1.5) == -2 and back(eps=float('nan')) == -2
  assert back(nbytes=bneed - 1) == -5 and back(wsp=ctypes.c_void_p(bws.data_ptr() + 4)) == -5
  torch.cuda.synchronize()
  for o in out + bout:
    assert bool((o == 7).all())                                                     # nothing ran
  # the Python wrappers refuse before the C side is asked
  for kw in (dict(num=0), dict(num=(1 << 20) + 1), dict(seed=-1), dict(seed=1 << 64), dict(stream=1 << 31),
             dict(scale=0.0), dict(uniforms=torch.zeros((8, 2), device=DEV)),
             dict(uniforms=torch.zeros((7, 2), dtype=torch.float64, device=DEV))):
    a = dict(num=8, seed=1)
    a.update(kw)
    with pytest.raises(ValueError):
      ops.vote_sample(votes, **a)
  for b, n_ in ((votes[:3], nxt), (votes.double(), nxt), (votes, nxt.long()), (votes, nxt.cpu()), (votes.cpu(), nxt)):
    with pytest.raises(ValueError):
      ops.vote_sample_back(b, n_, taps, 0.1, 1)
  with pytest.raises(ValueError):
    ops.vote_sample_back(votes, nxt, taps, 1.5, 1)
  with pytest.raises(ValueError):
    ops.vote_sample_back(votes, nxt, taps[:4], 0.1, 1)


# ---------------------------------------------------------------------------------------------------------------
# end to end: VoteFilter.sample on the statistical scene
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _filtered():
  scene = ref.stat_scene()
  track = pev.VoteFilter(scene['grid'], scene['R'], keep_history=True, **scene['kw'])
  for v, inc in zip(scene['votes'], scene['incs']):
    track.step(_dev(v), inc)
  return scene, track


def test_seeded_statistics_end_to_end():
  """65536 tracks from ``VoteFilter.sample``: frame 0's frequencies against ``smooth_track``'s frame-0 marginal, the
  last frame's against the belief, over the cells with an expected count >= 20.  The bound is the reference sampler's
  own largest |z| with this seed, plus 1."""
  scene, track = _filtered()
  with guarded.scope():
    out = track.sample(STAT_TRACKS, STAT_SEED)
  beliefs, incs = zip(*track.history)
  gamma = pev.smooth_track(beliefs, incs, scene['grid'], scene['R'], scene['kw']['sigma_xy'], scene['kw']['sigma_yaw'],
                           scene['kw']['uniform_mix'])
  linear = out['linear'].cpu().numpy().astype(np.int64)
  assert (linear >= 0).all()
  z0, n0 = ref.max_abs_z(linear[0], np.exp(gamma[0].double().cpu().numpy()))
  z2, n2 = ref.max_abs_z(linear[-1], np.exp(beliefs[-1].double().cpu().numpy()))
  print(f'max |z|: frame 0 {z0:.3f} over {n0} cells, last frame {z2:.3f} over {n2} cells; bound {Z_REFERENCE + 1}')
  assert n0 >= 40 and n2 >= 40
  assert z0 <= Z_REFERENCE + 1 and z2 <= Z_REFERENCE + 1
  # the reference sampler on the kernel's own beliefs and tables, same seed: the very same tracks, but for draws whose
  # uniform lies within rounding of a CDF boundary (a handful in 3 x 65536 at 2^-22)
  taps = [None] + [tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in pev.motion_taps(
      inc, scene['grid'], scene['R'], scene['kw']['sigma_xy'], scene['kw']['sigma_yaw'], device='cpu')) for inc in incs[1:]]
  want, want_jumps = ref.sample_tracks([b.cpu().numpy() for b in beliefs], taps, scene['kw']['uniform_mix'], 4096,
                                       STAT_SEED)
  same = (linear[:, :4096] == want).all(0)
  print(f'{int((~same).sum())} of 4096 tracks differ from the reference sampler\'s')
  assert same.mean() >= 0.99
  assert (out['jumps'].cpu().numpy()[:, :4096][:, same] == want_jumps[:, same]).all()


def test_host_api_shapes_and_transforms():
  scene, track = _filtered()
  R, grid = scene['R'], scene['grid']
  with guarded.scope():
    s = pev.sample_votes(track.belief, grid, R, 33, 5, stream=2, temperature=0.5)
  assert set(s) == {'linear', 'indices', 'm_t_q', 'log_prob', 'count', 'stats'}
  assert tuple(s['linear'].shape) == (33,) and s['linear'].dtype == torch.int32
  assert tuple(s['indices'].shape) == (33, 3) and s['indices'].dtype == torch.int32
  assert tuple(s['log_prob'].shape) == (33,) and s['log_prob'].dtype == torch.float32
  want_idx = np.stack(np.unravel_index(s['linear'].cpu().numpy(), tuple(track.belief.shape)), -1)
  assert s['indices'].cpu().tolist() == want_idx.tolist()
  tfm = pev.exhaustive_indices_to_tfm(s['indices'], grid, R)
  assert guarded.same_bits(s['m_t_q'].angle, tfm.angle) and guarded.same_bits(s['m_t_q'].t, tfm.t)
  out = track.sample(17, 3)
  N = len(track.history)
  assert set(out) == {'linear', 'indices', 'm_t_q', 'jumps'}
  assert tuple(out['linear'].shape) == (N, 17) and out['linear'].dtype == torch.int32
  assert tuple(out['indices'].shape) == (N, 17, 3) and out['indices'].dtype == torch.int32
  assert tuple(out['jumps'].shape) == (N, 17) and out['jumps'].dtype == torch.bool and not bool(out['jumps'][0].any())
  tfm = pev.exhaustive_indices_to_tfm(out['indices'].reshape(-1, 3), grid, R)
  assert guarded.same_bits(out['m_t_q'].angle, tfm.angle) and guarded.same_bits(out['m_t_q'].t, tfm.t)
  assert tuple(torch.as_tensor(out['m_t_q'].angle).shape)[0] == N * 17
  again = track.sample(17, 3)
  assert guarded.same_bits(out['linear'], again['linear'])
  beliefs, incs = zip(*track.history)
  same = pev.sample_tracks(beliefs, incs, grid, R, scene['kw']['sigma_xy'], scene['kw']['sigma_yaw'], 17, 3,
                           scene['kw']['uniform_mix'])
  assert guarded.same_bits(out['linear'], same['linear'])
  with pytest.raises(ValueError):
    pev.VoteFilter(grid, R, **scene['kw']).sample(4, 1)
  with pytest.raises(ValueError):
    pev.sample_votes(track.belief[:2], grid, R, 4, 1)
