"""`-m gpu`: ``ops.rebase_volume`` (vote_rebase.hip, through the C ABI) and the host entry points built on it, against
the float64 numpy restatement ``vote_rebase_reference`` within twice its derived rounding bound; ``count`` exactly, the
NaN and -inf cells identical, ``stats`` within twice its own derived bound.

The gather tiles every plane into 16 x 16 blocks, one workgroup per tile up to 2048 workgroups, which then stride over
the tiles; the other launches tile each rotation's pixels into runs of 256 the same way.  ``tiny`` [1, 1, 1]: the
identity; ``identity`` / ``shift`` / ``ragged`` / ``scale`` [36, 31, 33]: 2 x 3 tiles per plane, the last of each
axis partial, 30 % -inf plus the border mask (``shift``: phi = 0, (2, -3) cells; ``ragged``: phi = 0.37, fractional
shift and dk; ``scale``: the same at scale 0.5); ``quarter`` [8, 15, 15]: a quarter turn about the map centre,
``quarter_lattice`` about the lattice's middle (a permutation); ``wrap_*`` [4, 7, 7]: dk within 1e-9 of R, 0, 1 and 3;
``bad_identity`` / ``bad_ragged``: a NaN and a +inf source cell; ``gone``: a translation larger than the volume;
``thin_*`` [4, 1, 300] / [4, 300, 1]: planes one cell high / wide, shifted and turned.  The boundary of the tiling:
``tiles`` [2, 520, 520]: 2 x 33 x 33 = 2178 gather tiles and 2114 runs of 256 on 2048 workgroups (every launch strides,
and every fold of the per-workgroup partials has more entries than one pass of its 256 threads).  Every call runs under
``guarded.scope()``: guard regions intact (outputs and workspace), no output element left unwritten, the workspace the
size ``snap_vote_rebase_workspace_bytes`` states.

Observed on an MI355X (each case prints its figures), largest err / bound: ``tiny`` 0.00, ``identity`` 0.66, ``shift``
0.48, ``quarter`` 0.49, ``quarter_lattice`` 0.47, ``ragged`` 0.67 (9.5e-7 against 2.8e-6), ``scale`` 0.66, the four
``wrap_*`` 0.45 - 0.46, ``bad_identity`` 0.48, ``bad_ragged`` 0.66, ``thin_row`` 0.48, ``thin_row_turned`` 0.31,
``thin_col`` 0.49, ``thin_col_turned`` 0.45, ``tiles`` 0.79 (1.9e-6 against 2.5e-6), the table that is no rotation
0.65.  The errors are the final rounding to f32 (at most 2^-24 |dst|, which is most of the bound where |dst| is large:
a ratio below but close to 1 is expected there); the masses themselves came out as numpy's: ``stats`` ``log_z`` err 0
in every case, ``mass_kept`` at most 2.2e-16 (0.000 of its bound), the largest dst at most 0.19 of its bound.
Cross-check with ``vote_posterior``: ``log_z`` 4.3e-8 against a summed bound of 3.7e-6; the identity's cells 0.63 of
theirs.  2 x the bound is allowed."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_posterior_reference as post_ref
import vote_rebase_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import geometry, grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE


@functools.lru_cache(maxsize=None)
def _inputs():
  return {c['name']: c for c in ref.all_inputs()}


def _args(c):
  return c['src'], c['table'], c['scale']


@functools.lru_cache(maxsize=None)
def _want(name):
  c = _inputs()[name]
  return ref.vote_rebase(*_args(c)), ref.bound(*_args(c)), ref.stats_bound(*_args(c))


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(src, table, scale=1.0):
  """One guarded call -> numpy (dst, stats, count)."""
  R, Ho, Wo = src.shape
  with guarded.scope() as sc:
    out = ops.rebase_volume(guarded.place(_dev(src), 'value'), table, scale)
    assert [tuple(o.shape) for o in out] == [(R, Ho, Wo), (4,), (4,)]
    assert [o.dtype for o in out] == [torch.float32, torch.float64, torch.int32]
    ws = [a for a in sc.allocations('rebase_volume') if a.dtype == torch.int64]
    need = _lib.load().snap_vote_rebase_workspace_bytes(R, Ho, Wo)
    assert len(ws) == 1 and ws[0].numel() * 8 == need
    for o, what in zip(out, ('dst', 'stats', 'count')):      # (the kernel's NaN is 0x7fc00000, not the poison)
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
    if np.isfinite(ws[i]) and stol[i] > 0:
      e = abs(float(gs[i]) - ws[i])
      print(f'{what}: stats {name} err {e:.3e}, bound {stol[i]:.3e}, err / bound {e / stol[i]:.3f}')
      assert e <= factor * stol[i], f'{what}: stats[{i}] {gs[i]} against {ws[i]}'
    else:
      assert float(gs[i]) == ws[i], f'{what}: stats[{i}] {gs[i]} against {ws[i]}'
  # normalisation: float64 sum of exp over the finite cells is 1 within the cells' own rounding
  if fin.any():
    gf = g[np.isfinite(g)].astype(np.float64)
    total = np.exp(gf).sum()
    print(f'{what}: sum exp(dst) - 1 = {total - 1:.3e}')
    assert abs(total - 1) <= np.abs(gf).max() * 2.0 ** -23 + 2.0 ** -22


CASES = ['tiny', 'identity', 'shift', 'quarter', 'quarter_lattice', 'ragged', 'scale', 'wrap_below_R', 'wrap_above_0',
         'wrap_below_1', 'wrap_above_3', 'bad_identity', 'bad_ragged', 'gone', 'thin_row', 'thin_row_turned',
         'thin_col', 'thin_col_turned', 'tiles']


def test_the_cases_are_the_reference_s():
  assert sorted(CASES) == sorted(_inputs())


@pytest.mark.parametrize('name', CASES)
def test_against_the_reference(name):
  c = _inputs()[name]
  want, tol, stol = _want(name)
  _assert_within(_run(*_args(c)), want, tol, stol, name)


def test_identity_is_the_normalised_source_and_agrees_with_vote_posterior():
  """The identity reads exactly one cell: dst = scale * src - log_z within the bound, log_z that of
  ``ops.vote_posterior`` within the summed bounds; nothing is lost and every cell is covered."""
  c = _inputs()['identity']
  src, table, scale = _args(c)
  g, gs, gc = _run(src, table, scale)
  with guarded.scope():
    post = ops.vote_posterior(_dev(src), scale)
  lz = float(post[2][0])
  lz_tol = post_ref.bound(src, scale)[2][0]
  fin = np.isfinite(src)
  assert (np.isfinite(g) == fin).all() and gc.tolist() == [int(fin.sum()), 0, 0, 0] and gs[1] == 1.0
  e0 = abs(float(gs[0]) - lz)
  print(f'vote_posterior cross-check: log_z err {e0:.3e}, bound {ref.stats_bound(src, table, scale)[0] + lz_tol:.3e}')
  assert e0 <= ref.stats_bound(src, table, scale)[0] + lz_tol
  x = float(np.float32(scale)) * src[fin].astype(np.float64)
  tol = ref.bound(src, table, scale)[fin] + ref.stats_bound(src, table, scale)[0]
  err = np.abs(g[fin].astype(np.float64) - (x - float(gs[0])))
  print(f'identity: max err {err.max():.3e}, max err / bound {np.max(err / tol):.3f}')
  assert (err <= tol).all()


def test_bad_cells_poison_only_their_readers():
  c = _inputs()['bad_identity']
  g, gs, gc = _run(*_args(c))
  nan = np.isnan(g)
  assert nan.sum() == 2 and nan[3, 10, 11] and nan[30, 20, 5] and gc.tolist()[1:3] == [2, 2]
  g, gs, gc = _run(*_args(_inputs()['bad_ragged']))
  want = _want('bad_ragged')[0][0]
  assert 2 < np.isnan(g).sum() <= 2 * 18 and (np.isnan(g) == np.isnan(want)).all() and gc[2] == 2


def test_nothing_arrives_from_a_translation_larger_than_the_volume():
  c = _inputs()['gone']
  g, gs, gc = _run(*_args(c))
  assert (g == -np.inf).all() and gs[1] == 0.0 and gs[3] == -np.inf and gc.tolist() == [0, 0, 0, g.size]
  assert np.isfinite(gs[0]) and gs[2] == c['src'][np.isfinite(c['src'])].max()
  g, gs, gc = _run(np.full((3, 5, 6), -np.inf, np.float32), ref.IDENTITY)
  assert (g == -np.inf).all() and gs.tolist() == [-np.inf, 0.0, -np.inf, -np.inf] and gc.tolist() == [0, 0, 0, 0]


def test_a_table_that_is_no_rotation_reads_the_source_directly():
  """A = 3 I: the footprint of a tile is wider than the staging area, so the taps come from the source itself; the
  same reference, the same bound."""
  c = _inputs()['ragged']
  table = (0.5, np.eye(2) * 3.0, np.array([-20.25, -30.5]))
  args = (c['src'], table, c['scale'])
  _assert_within(_run(*args), ref.vote_rebase(*args), ref.bound(*args), ref.stats_bound(*args), 'scaled')


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for name in ('ragged', 'bad_ragged', 'tiles'):
    src, table, scale = _args(_inputs()[name])
    vol = _dev(src)
    first = ops.rebase_volume(vol, table, scale)
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.rebase_volume(vol, table, scale)
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    R, Ho, Wo = src.shape
    nbytes = lib.snap_vote_rebase_workspace_bytes(R, Ho, Wo)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dk, A, o = table
    outs = []
    for fill in (-1, 0x3ff0000000000000):
      ws.fill_(fill)
      out = (torch.empty((R, Ho, Wo), device=DEV), torch.empty((4,), dtype=torch.float64, device=DEV),
             torch.empty((4,), dtype=torch.int32, device=DEV))
      st = lib.snap_vote_rebase_f32(p(vol), R, Ho, Wo, scale, dk, A[0, 0], A[0, 1], A[1, 0], A[1, 1], o[0], o[1],
                                    p(out[0]), p(out[1]), p(out[2]), p(ws), nbytes,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      outs.append(out)
    torch.cuda.synchronize()
    for out in outs:
      for a, b in zip(first, out):
        assert guarded.same_bits(a, b), name


def test_bad_arguments_raise_without_allocating():
  vol = torch.zeros((4, 5, 6), device=DEV)
  good = ref.IDENTITY
  nan_table = (0.0, np.array([[1.0, 0.0], [float('nan'), 1.0]]), np.zeros(2))
  ops.rebase_volume(vol, good)
  bad = [dict(volume=vol.cpu()), dict(volume=vol.double()), dict(volume=torch.zeros((4, 5, 12), device=DEV)[:, :, ::2]),
         dict(volume=torch.zeros((65, 2, 2), device=DEV)), dict(volume=vol[0]), dict(volume=None),
         dict(scale=0.0), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=float('inf')),
         dict(table=nan_table), dict(table=(0.0, np.eye(2), np.array([0.0, float('inf')]))),
         dict(table=(4.0, np.eye(2), np.zeros(2))), dict(table=(-1e-9, np.eye(2), np.zeros(2))),
         dict(table=(float('nan'), np.eye(2), np.zeros(2))), dict(table=(0.0, np.eye(3), np.zeros(2))),
         dict(table=None)]
  for kw in bad:
    a = dict(volume=vol, table=good, scale=1.0)
    a.update(kw)
    with guarded.scope() as sc:
      with pytest.raises(ValueError) as info:
        ops.rebase_volume(a['volume'], a['table'], a['scale'])
      print(f'{sorted(kw)}: {info.value}')
      assert str(info.value).startswith('vote_rebase:'), str(info.value)
      assert not sc.allocations(), 'a refused call allocated nothing'
  lib = _lib.load()
  wsb = lib.snap_vote_rebase_workspace_bytes
  assert wsb(0, 5, 6) == 0 and wsb(65, 5, 6) == 0 and wsb(4, 0, 6) == 0 and wsb(4, 5, 0) == 0
  assert wsb(64, 4096, 8192) == 0                                                  # R Ho Wo = 2^31
  need = wsb(4, 5, 6)
  assert need == 4 * (2 * 8 + 2 * 4 + 4 * 4)                                       # 4 workgroups' partials
  ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
  out = torch.full((4, 5, 6), 7.0, device=DEV)
  stats = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
  count = torch.full((4,), 7, dtype=torch.int32, device=DEV)
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

  def call(R=4, scale=1.0, dk=0.0, a00=1.0, ob=0.0, nbytes=need, src=vol, wsp=None, count_=count):
    return lib.snap_vote_rebase_f32(p(src), R, 5, 6, scale, dk, a00, 0.0, 0.0, 1.0, 0.0, ob, p(out), p(stats), p(count_),
                                    wsp if wsp is not None else p(ws), nbytes, None)

  assert call(R=0) == -1 and call(R=65, nbytes=1 << 30) == -1
  assert call(src=None) == -3 and call(count_=None) == -3 and call(R=65, src=None) == -3
  assert call(scale=0.0) == -2 and call(scale=float('inf')) == -2 and call(dk=4.0) == -2 and call(dk=-0.5) == -2
  assert call(dk=float('nan')) == -2 and call(a00=float('nan')) == -2 and call(ob=float('inf')) == -2
  assert call(nbytes=need - 1) == -5 and call(wsp=ctypes.c_void_p(ws.data_ptr() + 4)) == -5
  torch.cuda.synchronize()
  assert bool((out == 7).all()) and bool((stats == 7).all()) and bool((count == 7).all())   # nothing ran


def _tfm(phi, tau):
  return geometry.Transform2D(torch.tensor(float(phi), dtype=torch.float64), torch.tensor(tau, dtype=torch.float64))


def _blob(R, Ho, Wo, centre, rng):
  k, a, b = np.meshgrid(np.arange(R), np.arange(Ho), np.arange(Wo), indexing='ij')
  dk = (k - centre[0] + R / 2) % R - R / 2
  x = -(dk ** 2 / (2 * 0.7 ** 2) + ((a - centre[1]) ** 2 + (b - centre[2]) ** 2) / (2 * 1.5 ** 2))
  return _dev((np.clip(x, -30, None) + rng.standard_normal(x.shape) * 0.01).astype(np.float32))


def test_a_track_survives_a_change_of_map_frame():
  """A Gaussian blob belief through ``VoteFilter.step``, ``rebase``, ``poses_from_votes``: the best pose is
  new_t_old @ the pose before, within one cell and one rotation bin (compared as indices); the next ``step`` re-opens
  the cells the old lattice did not cover."""
  H, R, cell = 16, 8, 0.25
  rng = np.random.default_rng(99)
  grid = grids.Grid2D((H, H), cell)
  Ho = 2 * H - 1
  track = pev.VoteFilter(grid, R, sigma_xy=0.2, sigma_yaw=0.15, temperature=1.0, uniform_mix=1e-3)
  with guarded.scope():
    track.step(_blob(R, Ho, Ho, (3.0, 13.0, 17.0), rng))
    before = pev.poses_from_votes(track.belief, grid, R, num_peaks=1)
    new_t_old = _tfm(0.37, [0.9, -0.6])
    out = track.rebase(new_t_old)
    after = pev.poses_from_votes(track.belief, grid, R, num_peaks=1)
  assert set(out) == {'votes', 'log_z', 'mass_kept', 'count', 'stats'} and out['votes'] is track.belief
  assert before['index'][0].tolist() == [3, 13, 17]
  # the belief was normalised; a turned bilinear gather keeps the mass only approximately
  assert abs(float(out['log_z'])) < 1e-5 and 0.9 < float(out['mass_kept']) < 1.1
  pose = before['map_t_query'][0]
  pose = geometry.Transform2D(pose.angle.cpu().to(torch.float64), pose.t.cpu().to(torch.float64))
  want = pev.exhaustive_tfm_to_index(new_t_old @ pose, grid, R).numpy()
  got = after['index'][0].cpu().numpy().astype(np.float64)
  print(f'rebased peak {got.tolist()}, composed pose at {want.tolist()}')
  assert abs((got[0] - want[0] + R / 2) % R - R / 2) <= 1.0 and np.abs(got[1:] - want[1:]).max() <= 1.0
  uncovered = int(out['count'][3])
  assert uncovered > 0 and int((track.belief == -math.inf).sum()) >= uncovered
  with guarded.scope():
    nxt = track.step(_blob(R, Ho, Ho, tuple(want), rng))
  assert bool(torch.isfinite(nxt['belief']).all())
  got = pev.poses_from_votes(nxt['belief'], grid, R, num_peaks=1)['index'][0].cpu().numpy().astype(np.float64)
  assert abs((got[0] - want[0] + R / 2) % R - R / 2) <= 1.0 and np.abs(got[1:] - want[1:]).max() <= 1.0


def test_history_rules():
  H, R = 8, 4
  rng = np.random.default_rng(5)
  grid = grids.Grid2D((H, H), 0.25)
  Ho = 2 * H - 1
  move = _tfm(0.0, [0.25, 0.0])
  for keep in (False, True):
    track = pev.VoteFilter(grid, R, sigma_xy=0.2, sigma_yaw=0.15, keep_history=keep)
    with pytest.raises(ValueError, match='no belief'):
      track.rebase(move)
  track = pev.VoteFilter(grid, R, sigma_xy=0.2, sigma_yaw=0.15, keep_history=True)
  track.step(_blob(R, Ho, Ho, (1.0, 7.0, 7.0), rng))
  held = track.belief
  with pytest.raises(ValueError, match='old map frame'):
    track.rebase(move)
  assert track.belief is held and len(track.history) == 1                       # nothing was touched
  out = track.rebase(move, drop_history=True)
  assert track.history == [] and track.belief is out['votes'] and track.belief is not held
  track.step(_blob(R, Ho, Ho, (1.0, 8.0, 7.0), rng))
  assert len(track.history) == 1
  plain = pev.VoteFilter(grid, R, sigma_xy=0.2, sigma_yaw=0.15)
  plain.step(_blob(R, Ho, Ho, (1.0, 7.0, 7.0), rng))
  plain.rebase(move)                                                            # no history kept: nothing to drop
  assert not hasattr(plain, 'history')
