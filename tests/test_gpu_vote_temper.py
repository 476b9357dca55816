"""`-m gpu`: ``ops.temper_volume`` (vote_temper.hip, through the C ABI) and the host entry points built on it
(``temper_votes``, ``TemperatureFit``, ``fit_temperature``), against the float64 numpy restatement
``vote_temper_reference`` within twice its documented error bound (a function of the input: the reference module's
docstring).

Launch 2 tiles the pixels p = a * Wo + b into runs of 256, one workgroup each (up to 1024 workgroups, then several
tiles per workgroup), one kernel instance per ladder length S.  ``[4, 7, 7]``: one partial tile; ``[1, 5, 5]`` and
``[3, 1, 1]``: the smallest extents; ``[36, 31, 33]``: four tiles, a ragged last one, Ho != Wo; ``[64, 5, 300]``: the
largest R; ``[2, 520, 520]``: 1057 tiles on 1024 workgroups (the float64 accumulators carry over a second tile); S in
{1, 5, 16}.  Every call runs under ``guarded.scope()``: guard regions intact (outputs and workspace), the workspace as
large as the query says, no output element left unwritten, the zero columns included.

Observed on an MI355X (each test prints its figures): the bound is a worst-case sum over the rounding points, and the
largest observed share of it is 0.05 on the reference cases (0.048 on E[v] at ``[1, 5, 5]``, S = 5; 0.024 on log_z at
``[4, 7, 7]``, S = 16; 0.006 at ``[2, 520, 520]``; 0.017 at votes of 1e30) and 0.21 on Var[v] of a ``[4, 9, 9]`` fit
volume (2 allowed); the {0, -inf} case equals numpy's log bit for bit (4 float64 ulps allowed); against
``ops.vote_posterior`` the largest difference is 4.6e-7 on log_z where the two bounds sum to 6.2e-6.  The fit on 30
valid frames: exact minimiser 2.248453139, Hermite estimate 4.0e-6 off after one round of 16 points, 3.2e-9 off after
three rounds (final bracket 2.246999741 .. 2.249770403, widened by 3.9e-6 for the assertion)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_posterior_reference as pref
import vote_temper_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.utils import grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE


@functools.lru_cache(maxsize=None)
def _inputs():
  return {c[0]: c for c in ref.all_inputs()}


@functools.lru_cache(maxsize=None)
def _want(name):
  _, v, scales, gt = _inputs()[name]
  return ref.vote_temper(v, scales, gt), ref.bound(v, scales, gt)


def _run(v, scales, gt=None):
  """One guarded call -> numpy (table, stats, count)."""
  votes = torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
  gt_dev = None if gt is None else torch.tensor(gt, dtype=torch.float32, device=DEV)
  S = len(scales)
  with guarded.scope() as sc:
    gtp = None if gt_dev is None else guarded.place(gt_dev, 'address')
    out = ops.temper_volume(guarded.place(votes, 'value'), scales, gtp)
    R, Ho, Wo = v.shape
    assert [tuple(o.shape) for o in out] == [(S, 8), (4,), (4,)]
    assert [o.dtype for o in out] == [torch.float64, torch.float64, torch.int32]
    ws = [a for a in sc.allocations('temper_volume') if a.dtype == torch.int64]
    assert len(ws) == 1 and ws[0].numel() * 8 == _lib.load().snap_vote_temper_workspace_bytes(R, Ho, Wo, S)
    for o, what in zip(out, ('table', 'stats', 'count')):   # (the kernel's NaN is 0x7ff8000000000000, not the poison)
      assert not bool(guarded.unwritten(o).any()), f'{what}: elements never written'
    res = tuple(o.cpu().numpy() for o in out)
  assert (res[0][:, 7] == 0).all() and (res[1][2:] == 0).all() and res[2][3] == 0
  return res


def _assert_within(got, want, tol, factor=2.0, what=''):
  (gt_, gs, gc), (wt, ws, wc) = got, want
  assert gc.tolist() == wc.tolist(), f'{what}: count {gc.tolist()} != {wc.tolist()}'
  for g, w in zip(gs, ws):                                   # stats = (m, v_gt, 0, 0): exact (v_gt to float64 rounding)
    assert (np.isnan(g) and np.isnan(w)) or g == w or abs(g - w) <= 2.0 ** -48 * abs(w), f'{what}: stats {gs} != {ws}'
  special = ~np.isfinite(wt)
  assert ((np.isnan(gt_) == np.isnan(wt)) & ((gt_ == wt) | ~special | np.isnan(wt))).all(), f'{what}: NaN / inf pattern'
  with np.errstate(invalid='ignore'):
    err = np.where(special | (gt_ == wt), 0.0, np.abs(gt_ - wt))
    share = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0.0))
  print(f'{what}: largest share of the bound per column', dict(zip(ref.COLUMNS, share.max(0).round(4).tolist())))
  bad = ~(err <= factor * tol)
  assert not bad.any(), f'{what}: {int(bad.sum())} outside, first {np.argwhere(bad)[0].tolist()}: {gt_[bad][0]!r} vs {wt[bad][0]!r}'


@pytest.mark.parametrize('S', sorted(ref.LADDERS))
@pytest.mark.parametrize('shape', ref.RANDOM_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_random_shapes(shape, S):
  name = 'random%s_S%d' % (shape, S)
  _, v, scales, gt = _inputs()[name]
  want, tol = _want(name)
  assert want[2][2] == 1
  _assert_within(_run(v, scales, gt), want, tol, what=name)


def test_several_tiles_per_workgroup():
  """[2, 520, 520]: 1057 tiles on 1024 workgroups, so workgroups 0 .. 32 walk two tiles each (``ref.fold_votes``: masked
  tiles before and after live ones, raised tiles).  The ground-truth index lies in a second tile."""
  _, v, scales, gt = _inputs()['fold']
  assert v.shape[1] * v.shape[2] > 1024 * ref.TILE
  want, tol = _want('fold')
  assert want[2][2] == 1 and tol[:, 0].max() < 1e-4
  _assert_within(_run(v, scales, gt), want, tol, what='fold')


def _f64_ulps(got, want):
  want = np.asarray(want, np.float64)
  return np.where(np.asarray(got) == want, 0.0, np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want)))


@pytest.mark.parametrize('shape', [(36, 31, 33), (4, 7, 7), (64, 5, 300)], ids=lambda s: '%dx%dx%d' % s)
def test_exact_case(shape):
  """Votes in {0, -inf}: every exponential is exactly 1 or 0 at every scale and every sum an integer, so log_z =
  entropy = -log p_max = log n with ONE float64 log of an exact integer: within 4 float64 ulps of numpy's (the device
  library's log and numpy's are each within 1 ulp of the true value, and the true value may sit at a rounding
  boundary); E[v] and Var[v] are exactly 0."""
  v = ref.exact_votes(shape)
  n = int(np.isfinite(v).sum())
  table, stats, count = _run(v, ref.LADDERS[16])
  assert count.tolist() == [n, 0, 0, 0] and stats[0] == 0 and np.isnan(stats[1])
  for col, want in ((0, np.log(n)), (3, np.log(n)), (4, -np.log(n))):
    u = _f64_ulps(table[:, col], want)
    print(f'exact {shape} {ref.COLUMNS[col]}: {u.max():.1f} float64 ulp')
    assert u.max() <= 4
  assert (table[:, 1] == 0).all() and (table[:, 2] == 0).all() and np.isnan(table[:, 5:7]).all()


def test_single_contributing_cell():
  v, c = ref.single_cell_votes()
  table, stats, count = _run(v, ref.LADDERS[5], tuple(float(i) for i in c))
  s = ref.ladder(ref.LADDERS[5])
  assert count.tolist() == [1, 0, 1, 0] and stats[0] == v[c] and stats[1] == v[c]
  assert (table[:, 0] == s * np.float64(v[c])).all() and (table[:, 1] == v[c]).all()
  assert (table[:, 2] == 0).all() and (table[:, 3] == 0).all() and (table[:, 4] == 0).all()      # exactly
  assert (table[:, 5] == 0).all() and (table[:, 6] == 0).all()
  _assert_within(_run(v, ref.LADDERS[5]), *_want('single'), what='single')


def test_two_tied_maxima_at_a_huge_scale():
  """At scale 1e4 every other cell is 2500 below: its weight is exactly 0 and the entropy is log 2 (the exact case's
  4 float64 ulps), E[v] exactly the tied value and Var[v] exactly 0."""
  _, v, scales, gt = _inputs()['tied']
  table, stats, count = _run(v, scales, gt)
  assert _f64_ulps(table[1, 3], np.log(2)) <= 4 and table[1, 4] == -table[1, 3]   # (one float64 log of an exact 2)
  assert table[1, 1] == 0.5 and table[1, 2] == 0 and count[0] > 2
  _assert_within((table, stats, count), *_want('tied'), what='tied')


@pytest.mark.parametrize('shape', [(36, 31, 33), (3, 1, 1)], ids=lambda s: '%dx%dx%d' % s)
def test_empty_volume(shape):
  table, stats, count = _run(np.full(shape, -np.inf, np.float32), ref.LADDERS[5], (0.5, 0.0, 0.0))
  assert (table[:, 0] == -np.inf).all() and np.isnan(table[:, 1:7]).all() and (table[:, 7] == 0).all()
  assert stats[0] == -np.inf and np.isnan(stats[1]) and count.tolist() == [0, 0, 0, 0]


def test_nan_and_plus_inf_are_excluded_and_counted():
  bad, masked, n = ref.nan_inf_votes()
  got_bad, got_masked = _run(bad, ref.LADDERS[5]), _run(masked, ref.LADDERS[5])
  assert got_bad[2].tolist() == [got_masked[2][0], n, 0, 0] and got_masked[2][1] == 0
  for a, b in zip(got_bad[:2], got_masked[:2]):              # the rest is unchanged, bit for bit
    assert guarded.same_bits(torch.from_numpy(a), torch.from_numpy(b))
  _assert_within(got_bad, *_want('nan_inf'), what='nan_inf')


def test_ground_truth_sample():
  v, cases = ref.gt_cases()
  scales = ref.LADDERS[5]
  for name, idx, valid in cases:
    want, tol = _want('gt_' + name)
    assert want[2][2] == valid
    got = _run(v, scales, idx)
    assert got[2][2] == valid and bool(np.isnan(got[1][1])) == (not valid), name
    assert bool(np.isnan(got[0][:, 5:7]).all()) == (not valid) and bool(np.isnan(got[0][:, 5:7]).any()) == (not valid)
    _assert_within(got, want, tol, what='gt_' + name)
  none = _run(v, scales, None)
  assert none[2][2] == 0 and np.isnan(none[1][1]) and np.isnan(none[0][:, 5:7]).all()
  assert (none[0][:, :5].view(np.int64) == got[0][:, :5].view(np.int64)).all()   # the sample changes nothing else


def test_votes_around_1e30_with_scale_1e10():
  """scale * v = 1e40 is beyond f32: ``vote_posterior`` returns NaN here (its documented condition); the ladder never
  forms that product in f32, so every output is finite and within the bound, also at scales of 1e-30, where the
  weights are spread and the second moment is of the order of 1e58."""
  _, v, scales, gt = _inputs()['huge']
  assert 1e10 in scales and float(np.float32(1e10)) * float(v[np.isfinite(v)].max()) > 3.5e38
  got = _run(v, scales, gt)
  assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and got[2][2] == 1
  _assert_within(got, *_want('huge'), what='huge')
  post = ops.vote_posterior(torch.from_numpy(v).to(DEV), 1e10)[2]
  assert bool(torch.isnan(post[0]))


def test_agrees_with_vote_posterior_at_every_scale():
  """log_z, entropy and log_prob_gt against ``ops.vote_posterior(votes, s, gt)``'s stats[0], [11] and [12], within the
  sum of the two references' bounds."""
  for name in ('random(36, 31, 33)_S16', 'random(4, 7, 7)_S5', 'gt_interior'):
    _, v, scales, gt = _inputs()[name]
    votes = torch.from_numpy(v).to(DEV)
    gt_dev = torch.tensor(gt, dtype=torch.float32, device=DEV)
    table = ops.temper_volume(votes, scales, gt_dev)[0].cpu().numpy()
    tol = _want(name)[1]
    for l, s in enumerate(ref.ladder(scales)):
      st = ops.vote_posterior(votes, float(s), gt_dev)[2].cpu().numpy().astype(np.float64)
      ptol = pref.bound(v, np.float32(s), gt)[2]
      for col, pcol in ((0, 0), (3, 11), (5, 12)):
        err, allowed = abs(table[l, col] - st[pcol]), tol[l, col] + ptol[pcol]
        print(f'{name} s={s:.4g} {ref.COLUMNS[col]}: |difference| {err:.3e}, sum of the bounds {allowed:.3e}')
        assert err <= allowed, (name, s, ref.COLUMNS[col], table[l, col], st[pcol])


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for name in ('random(36, 31, 33)_S16', 'random(64, 5, 300)_S5', 'gt_interior', 'fold'):
    _, v, scales, gt = _inputs()[name]
    votes = torch.from_numpy(v.copy()).to(DEV)
    gt_dev = None if gt is None else torch.tensor(gt, dtype=torch.float32, device=DEV)
    first = ops.temper_volume(votes, scales, gt_dev)
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.temper_volume(votes, scales, gt_dev)
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    # the C entry point on one workspace, left full of garbage between the calls
    R, Ho, Wo = v.shape
    S = len(scales)
    host = (ctypes.c_float * S)(*np.asarray(scales, np.float32).tolist())
    nbytes = lib.snap_vote_temper_workspace_bytes(R, Ho, Wo, S)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    outs = []
    for fill in (0x7ff8000000000001, -1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = (torch.empty((S, 8), dtype=torch.float64, device=DEV), torch.empty((4,), dtype=torch.float64, device=DEV),
           torch.empty((4,), dtype=torch.int32, device=DEV))
      st = lib.snap_vote_temper_f32(
          ctypes.c_void_p(votes.data_ptr()), R, Ho, Wo, host, S, None if gt_dev is None else ctypes.c_void_p(gt_dev.data_ptr()),
          *(ctypes.c_void_p(t.data_ptr()) for t in o), ctypes.c_void_p(ws.data_ptr()), nbytes,
          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name


def _good():
  return dict(votes=torch.zeros((3, 4, 5), dtype=torch.float32, device=DEV), scales=(0.5, 1.0, 2.0), gt_index=None)


_GT = lambda: torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device=DEV)
BAD_CALLS = [
    ('scales-empty', 'scales', lambda: (), ValueError),
    ('scales-17', 'scales', lambda: tuple(1.0 + i for i in range(17)), ValueError),
    ('scales-not-increasing', 'scales', lambda: (1.0, 3.0, 2.0), ValueError),
    ('scales-equal-as-f32', 'scales', lambda: (1.0, 1.0 + 2.0 ** -30), ValueError),
    ('scales-zero', 'scales', lambda: (0.0, 1.0), ValueError),
    ('scales-negative', 'scales', lambda: (-1.0, 1.0), ValueError),
    ('scales-inf', 'scales', lambda: (1.0, float('inf')), ValueError),
    ('scales-inf-as-f32', 'scales', lambda: (1.0, 1e39), ValueError),
    ('scales-nan', 'scales', lambda: (1.0, float('nan')), ValueError),
    ('scales-no-numbers', 'scales', lambda: ('a', 'b'), ValueError),
    ('votes-f64', 'votes', lambda: torch.zeros((3, 4, 5), dtype=torch.float64, device=DEV), TypeError),
    ('votes-nontensor', 'votes', lambda: np.zeros((3, 4, 5), np.float32), TypeError),
    ('votes-cpu', 'votes', lambda: torch.zeros((3, 4, 5), dtype=torch.float32), RuntimeError),
    ('votes-2d', 'votes', lambda: torch.zeros((4, 5), dtype=torch.float32, device=DEV), ValueError),
    ('votes-noncontig', 'votes', lambda: torch.zeros((3, 4, 10), dtype=torch.float32, device=DEV)[..., ::2], ValueError),
    ('votes-R65', 'votes', lambda: torch.zeros((65, 4, 5), dtype=torch.float32, device=DEV), ValueError),
    ('gt_index-shape2', 'gt_index', lambda: _GT()[:2].contiguous(), ValueError),
    ('gt_index-cpu', 'gt_index', lambda: _GT().cpu(), RuntimeError),
    ('gt_index-f64', 'gt_index', lambda: _GT().double(), TypeError),
]


@pytest.mark.parametrize('arg,value,exc', [row[1:] for row in BAD_CALLS], ids=[row[0] for row in BAD_CALLS])
def test_bad_call_is_refused(arg, value, exc):
  """A call that is good but for ONE argument: the exception class of ``test_gpu_vote_args``' table for a wrapper that
  checks its volume through ``_chk``, the operator's name in front, and nothing allocated before the refusal."""
  a = _good()
  a[arg] = value()
  with guarded.scope() as sc:
    with pytest.raises(exc) as info:
      ops.temper_volume(a['votes'], a['scales'], a['gt_index'])
    print(f'{type(info.value).__name__}: {info.value}')
    assert type(info.value) is exc
    assert str(info.value).startswith('vote_temper:'), str(info.value)
    assert not sc.allocations(), 'a refused call allocated nothing'
  assert ops.temper_volume(**_good()) is not None               # the good call runs: each entry fails for its mistake alone


# ---- temper_votes, TemperatureFit, fit_temperature --------------------------------------------------------------------
FIT_R = ref.FIT_SHAPE[0]
FIT_GRID = grids.Grid2D((5, 5), 0.25)                          # votes [4, 9, 9] = [R, 2H-1, 2W-1]


@functools.lru_cache(maxsize=None)
def _fit_set():
  """(device volumes, ground-truth transforms, numpy volumes, the indices the device reads, the exact minimiser)."""
  volumes, gts = ref.fit_frames()
  dev = [torch.from_numpy(v).to(DEV) for v in volumes]
  tfms = [pev.exhaustive_index_to_tfm(torch.tensor(g, dtype=torch.float32), FIT_GRID, FIT_R) for g in gts]
  # what the kernel samples: the transform pushed back through exhaustive_tfm_to_index, rounded to f32
  seen = [tuple(pev.exhaustive_tfm_to_index(t, FIT_GRID, FIT_R).to(torch.float32).reshape(3).tolist()) for t in tfms]
  lo, hi, _ = ref.FIT_LADDER
  s_star, frames = ref.nll_minimiser(volumes, seen, lo, hi)
  return dev, tfms, volumes, seen, s_star, frames


def test_temper_votes():
  dev, tfms, volumes, seen, _, _ = _fit_set()
  ladder = pev.temperature_ladder(*ref.FIT_LADDER)
  for f in (0, 5, 17):
    with guarded.scope():
      out = pev.temper_votes(dev[f], FIT_GRID, FIT_R, ladder, tfms[f])
    assert set(out) == {'log_z', 'mean_vote', 'var_vote', 'entropy', 'log_p_max', 'log_prob_gt', 'nll_slope', 'valid_gt',
                        'count', 'table', 'stats'}
    want, tol = ref.vote_temper(volumes[f], ladder, seen[f]), ref.bound(volumes[f], ladder, seen[f])
    got = (out['table'].cpu().numpy(), out['stats'].cpu().numpy(), out['count'].cpu().numpy())
    _assert_within(got, want, tol, what=f'temper_votes frame {f}')
    assert bool(out['valid_gt']) == (f == 0) == bool(want[2][2])
    for key, col in (('log_z', 0), ('mean_vote', 1), ('var_vote', 2), ('entropy', 3), ('log_p_max', 4),
                     ('log_prob_gt', 5), ('nll_slope', 6)):
      assert out[key].dtype == torch.float64 and guarded.same_bits(out[key].contiguous(), out['table'][:, col].contiguous())
    # entropy falls and confidence rises with the temperature
    assert (np.diff(got[0][:, 3]) < 0).all() and (np.diff(got[0][:, 4]) > 0).all()
  none = pev.temper_votes(dev[0], FIT_GRID, FIT_R, ladder)
  assert not bool(none['valid_gt']) and bool(torch.isnan(none['log_prob_gt']).all())
  with pytest.raises(ValueError):
    pev.temper_votes(dev[0], FIT_GRID, FIT_R + 1, ladder)
  with pytest.raises(ValueError):
    pev.temper_votes(dev[0], FIT_GRID, FIT_R, (2.0, 1.0))


def _slope_bound(volumes, seen, ladder):
  """The sum over the valid frames of the reference's bound on dnll, per ladder point."""
  total = np.zeros(len(ladder))
  for v, g in zip(volumes, seen):
    if ref.vote_temper(v, ladder, g)[2][2]:
      total += ref.bound(v, ladder, g)[:, 6]
  return total


def test_temperature_fit_brackets_the_exact_minimiser():
  dev, tfms, volumes, seen, s_star, frames = _fit_set()
  ladder = pev.temperature_ladder(*ref.FIT_LADDER)
  assert frames == ref.FIT_FRAMES - 2 and ladder[1] < s_star < ladder[-2]       # strictly inside (also pinned on the CPU)
  fit = pev.TemperatureFit(FIT_GRID, FIT_R, ladder)
  with guarded.scope():
    for votes, tfm in zip(dev, tfms):
      fit.add(votes, tfm)
  out = fit.solve()
  assert out['frames'] == frames and out['bracketed'] and out['nll'].shape == (len(ladder),)
  lo, hi = out['bracket']
  assert lo <= out['temperature'] <= hi and lo < s_star < hi
  print(f'one round: exact minimiser {s_star:.9f}, Hermite estimate {out["temperature"]:.9f} '
        f'(distance {abs(out["temperature"] - s_star):.3e}) in the bracket ({lo:.6f}, {hi:.6f})')
  # the frames with an invalid ground truth (5 and 17) change nothing: the same sums without them, bit for bit
  only_valid = pev.TemperatureFit(FIT_GRID, FIT_R, ladder)
  for f, (votes, tfm) in enumerate(zip(dev, tfms)):
    if f not in (5, 17):
      only_valid.add(votes, tfm)
  other = only_valid.solve()
  assert other['temperature'] == out['temperature'] and (other['nll'] == out['nll']).all() and other['frames'] == frames
  # add_table on the stored tables gives the same sums
  stored = pev.TemperatureFit(FIT_GRID, FIT_R, ladder)
  for votes, tfm in zip(dev, tfms):
    gt = pev.exhaustive_tfm_to_index(tfm, FIT_GRID, FIT_R).to(device=DEV, dtype=torch.float32).reshape(3).contiguous()
    table, _, count = ops.temper_volume(votes, ladder, gt)
    stored.add_table(table, count)
  assert stored.solve()['temperature'] == out['temperature']
  # the total nll against the reference, within the summed bound
  want = sum(-ref.vote_temper(v, ladder, g)[0][:, 5] for v, g in zip(volumes, seen) if ref.vote_temper(v, ladder, g)[2][2])
  allowed = sum(ref.bound(v, ladder, g)[:, 5] for v, g in zip(volumes, seen) if ref.vote_temper(v, ladder, g)[2][2])
  assert (np.abs(out['nll'] - want) <= 2 * allowed).all()


def test_fit_temperature_three_rounds():
  dev, tfms, volumes, seen, s_star, frames = _fit_set()
  lo, hi, num = ref.FIT_LADDER
  out = pev.fit_temperature(dev, tfms, FIT_GRID, FIT_R, lo, hi, num=num, rounds=3)
  assert out['bracketed'] and out['frames'] == frames and len(out['brackets']) == 3
  widths = [b[1] / b[0] for b in out['brackets']]
  assert widths[0] > widths[1] > widths[2] > 1
  assert abs(np.log(widths[1]) * (num - 1) / np.log(widths[0]) - 1) < 1e-4       # shrinks by num - 1 in the exponent
  for a, b in zip(out['brackets'], out['brackets'][1:]):
    assert a[0] <= b[0] < b[1] <= a[1]
  b_lo, b_hi = out['brackets'][-1]
  # the slope's error propagated to the root: 2 * bound(slope) / the smaller total curvature at the bracket's ends
  ends = np.array([b_lo, b_hi])
  slope_tol = _slope_bound(volumes, seen, ends).max()
  curvature = min(sum(ref.vote_temper(v, ends, g)[0][i, 2] for v, g in zip(volumes, seen)
                      if ref.vote_temper(v, ends, g)[2][2]) for i in (0, 1))
  widen = 2 * slope_tol / curvature
  print(f'three rounds: exact minimiser {s_star:.9f}, Hermite estimate {out["temperature"]:.9f} (distance '
        f'{abs(out["temperature"] - s_star):.3e}), final bracket ({b_lo:.9f}, {b_hi:.9f}), widened by {widen:.3e}')
  assert b_lo - widen <= s_star <= b_hi + widen
  assert b_lo <= out['temperature'] <= b_hi


def test_a_ladder_that_does_not_bracket():
  dev, tfms, volumes, seen, s_star, frames = _fit_set()
  for lo, hi, end in ((0.25, 1.0, 1.0), (4.0, 16.0, 4.0)):       # the minimiser (2.25) lies above / below the ladder
    assert not lo < s_star < hi
    fit = pev.TemperatureFit(FIT_GRID, FIT_R, pev.temperature_ladder(lo, hi, 5))
    for votes, tfm in zip(dev, tfms):
      fit.add(votes, tfm)
    out = fit.solve()
    assert not out['bracketed'] and out['temperature'] == end and out['bracket'] == (end, end)
    more = pev.fit_temperature(dev, tfms, FIT_GRID, FIT_R, lo, hi, num=5, rounds=3)
    assert not more['bracketed'] and more['temperature'] == end and len(more['brackets']) == 1
