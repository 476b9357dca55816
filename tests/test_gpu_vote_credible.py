"""`-m gpu`: ``ops.vote_credible`` (vote_credible.hip, through the C ABI) and the host entry points built on it, against
the float64 full-sort restatement ``vote_credible_reference``.

Every listed input meets the gap condition (test_vote_credible_reference), so thresholds, tables, level maps, counts
and the ground-truth value are compared with EQUALITY; the masses within twice the reference's bound plus one f32
rounding.  Shapes as in the posterior's test: ``[3, 1, 1]`` and ``[1, 5, 5]`` the smallest extents; ``[4, 7, 7]`` one
partial tile; ``[36, 31, 33]`` ragged tiles, Ho != Wo; ``[64, 5, 300]`` the largest R; ``[8, 200, 210]`` a sharp peak
(region 0 is a handful of cells); ``[2, 520, 520]`` more tiles than workgroups in both tile walks.  Every call runs
under ``guarded.scope()``: guard regions intact (outputs and workspace), no output element left unwritten.

Observed on an MI355X (each test prints its figures): every mass within 3.0e-8 of the reference, i.e. inside the one
f32 rounding (the bounds are 1e-12 .. 3e-9); the tightest listed gap is 12 times what the condition needs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_credible_reference as ref
from snap_amd import _lib, ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
NAMES = ('threshold', 'mass', 'table', 'level_xy', 'level_r', 'level_cell', 'gt_stats', 'count')


@functools.lru_cache(maxsize=None)
def _inputs():
  return {c[0]: c for c in ref.all_inputs()}


@functools.lru_cache(maxsize=None)
def _want(name):
  _, v, scale, levels, gt = _inputs()[name]
  return ref.vote_credible(v, levels, scale, gt), ref.bound(v, scale)


def _run(v, levels, scale, gt=None, cell_levels=True):
  """One guarded call -> the outputs as numpy arrays (level_cell None without ``cell_levels``)."""
  votes = torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
  gt_dev = None if gt is None else torch.tensor(gt, dtype=torch.float32, device=DEV)
  R, Ho, Wo = v.shape
  L = len(levels)
  with guarded.scope() as sc:
    gtp = None if gt_dev is None else guarded.place(gt_dev, 'address')
    out = ops.vote_credible(guarded.place(votes, 'value'), levels, scale, gtp, cell_levels)
    shapes = [(L,), (L,), (L, 8), (Ho, Wo), (R,), (R, Ho, Wo), (4,), (4,)]
    dtypes = [torch.float32, torch.float32, torch.int32, torch.uint8, torch.uint8, torch.uint8, torch.float32,
              torch.int32]
    for o, s, d, nm in zip(out, shapes, dtypes, NAMES):
      if nm == 'level_cell' and not cell_levels:
        assert o is None
        continue
      assert tuple(o.shape) == s and o.dtype == d, nm
    ws = [a for a in sc.allocations('vote_credible') if a.dtype == torch.int64]
    assert len(ws) == 1 and ws[0].numel() * 8 == _lib.load().snap_vote_credible_workspace_bytes(R, Ho, Wo, L)
    # (the poison is the all-ones pattern: NaN in f32, -1 in int32, 255 in uint8.  The kernel's NaN is 0x7fc00000 and
    #  its levels are <= 8; its -1 entries (an empty region's box, an invalid ground truth's level) ARE the poison's
    #  bits, so the int32 outputs are checked where the contract has no -1)
    has_f = bool(np.isfinite(v).any())
    for o, nm in zip(out, NAMES):
      if o is None:
        continue
      un = guarded.unwritten(o)
      if nm == 'table' and not has_f:
        un = un[:, [0, 1, 2, 7]]
      if nm == 'count':
        un = un[:3]
      assert not bool(un.any()), f'{nm}: elements never written'
    res = tuple(None if o is None else o.cpu().numpy() for o in out)
  return res


def _assert_equal(got, want, eps, what):
  (gth, gm, gtab, gxy, gr, gc, gst, gcnt), (wth, wm, wtab, wxy, wr, wc, wst, wcnt) = got, want
  assert ((gth == wth) | (np.isnan(gth) & np.isnan(wth))).all(), f'{what}: threshold {gth} != {wth}'
  assert (gtab == wtab).all(), f'{what}: table\n{gtab}\n!=\n{wtab}'
  assert (gxy == wxy).all() and (gr == wr).all(), f'{what}: level maps'
  if gc is not None:
    assert (gc == wc).all(), f'{what}: level_cell differs in {int((gc != wc).sum())} cells'
  assert gcnt.tolist() == wcnt.tolist(), f'{what}: count {gcnt.tolist()} != {wcnt.tolist()}'
  assert gst[0] == wst[0] or (np.isnan(gst[0]) and np.isnan(wst[0])), f'{what}: v_gt {gst[0]} != {wst[0]}'
  assert gst[3] == 0
  for g, w, nm in [(gm, wm, 'mass'), (gst[1:3], wst[1:3], 'gt tail masses')]:
    assert (np.isnan(g) == np.isnan(w)).all(), f'{what}: {nm} {g} vs {w}'
    err = np.where(np.isnan(w), 0.0, np.abs(g.astype(np.float64) - w))
    tol = 2 * eps + 2.0 ** -24 * np.where(np.isnan(w), 0.0, np.abs(w))
    print(f'{what} {nm}: max err {err.max():.3e}, allowed {tol.max():.3e} (bound {eps:.3e})')
    assert (err <= tol).all(), f'{what}: {nm} {g} vs {w}'


CASES = [n for n in (c[0] for c in ref.all_inputs()) if not n.startswith('gt_')]


@pytest.mark.parametrize('name', CASES)
def test_against_the_full_sort_reference(name):
  _, v, scale, levels, gt = _inputs()[name]
  want, eps = _want(name)
  got = _run(v, levels, scale, gt)
  _assert_equal(got, want, eps, name)
  # counts as the posterior's on the same volume (an empty F included: both report 0 contributing cells)
  post = ops.vote_posterior(torch.from_numpy(v).to(DEV), scale)[3].cpu().numpy()
  assert got[7][:2].tolist() == post[:2].tolist()
  if name.startswith('ties') and len(levels) == 3:
    assert got[0][0] == got[0][1] and (got[2][0] == got[2][1]).all() and got[1][0] == got[1][1]
  if name.startswith('equal'):
    assert (got[0] == 0).all() and (got[2][:, 0] == int(np.isfinite(v).sum())).all() and (got[1] == 1).all()
  if name.startswith('masked'):
    L = len(levels)
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and np.isnan(got[6][:3]).all()
    assert (got[2] == np.array([0, 0, 0, -1, -1, -1, -1, 0])).all()
    assert (got[3] == L).all() and (got[4] == L).all() and (got[5] == L).all() and got[7].tolist() == [0, 0, 0, -1]


def test_peak_region_is_a_handful_of_cells():
  """[8, 200, 210], sigma 0.7 cells in the far corner: the kernel's region 0 is a few pixels in every rotation, its
  box hugs the corner, and a ground truth on the best cell has nothing ranked above it."""
  _, v, scale, levels, _ = _inputs()['peak_s1_L3']
  R, Ho, Wo = v.shape
  got = _run(v, levels, scale, (3.0, float(Ho - 1), float(Wo - 2)))
  cells, pixels, rotations, a0, a1, b0, b1, _ = got[2][0].tolist()
  assert cells == R * pixels and 1 <= pixels <= 8 and rotations == R
  assert a0 >= Ho - 4 and a1 == Ho - 1 and b0 >= Wo - 5 and b1 <= Wo - 1
  assert int((got[3] == 0).sum()) == pixels and (got[4] == 0).all()
  assert got[6][1] == 0 and got[7][2:].tolist() == [1, 0]


def test_without_cell_levels_the_rest_is_unchanged():
  _, v, scale, levels, _ = _inputs()['dirty(36, 31, 33)_s4_L3']
  a, b = _run(v, levels, scale, cell_levels=True), _run(v, levels, scale, cell_levels=False)
  assert b[5] is None
  for x, y, nm in zip(a, b, NAMES):
    if nm != 'level_cell':
      assert guarded.same_bits(torch.from_numpy(x), torch.from_numpy(y)), nm


def test_ground_truth_cases():
  v, levels, scale, cases = ref.gt_cases()
  base = _run(v, levels, scale, None)
  assert base[7][2:].tolist() == [0, -1] and np.isnan(base[6][:3]).all()
  for name, idx, cell in cases:
    want, eps = _want('gt_' + name)
    got = _run(v, levels, scale, idx)
    valid = cell is not None and bool(np.isfinite(v[cell]))
    assert got[7][2] == int(valid), name
    if valid:
      assert got[6][0] == v[cell] and got[7][3] == int((v[cell] < got[0]).sum()), name
    else:
      assert np.isnan(got[6][:3]).all() and got[7][3] == -1, name
    _assert_equal(got, want, eps, 'gt_' + name)
    for x, y in zip(base[:6], got[:6]):                       # the ground truth changes nothing else
      assert guarded.same_bits(torch.from_numpy(x), torch.from_numpy(y)), name


def test_two_calls_give_identical_bytes_also_with_garbage_in_the_workspace():
  lib = _lib.load()
  for name in ('smooth(36, 31, 33)_s4_L8', 'dirty(64, 5, 300)_s4_L3', 'ties(2, 520, 520)_s1_L3', 'peak_s1_L3',
               'gt_between'):
    _, v, scale, levels, gt = _inputs()[name]
    votes = torch.from_numpy(v.copy()).to(DEV)
    gt_dev = None if gt is None else torch.tensor(gt, dtype=torch.float32, device=DEV)
    first = ops.vote_credible(votes, levels, scale, gt_dev, True)
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_credible(votes, levels, scale, gt_dev, True)
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b), name
    R, Ho, Wo = v.shape
    L = len(levels)
    nbytes = lib.snap_vote_credible_workspace_bytes(R, Ho, Wo, L)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=DEV)
    host = (ctypes.c_float * L)(*levels)
    outs = []
    for fill in (0x7ff8000000000001, -1, 0x3ff0000000000000):
      ws.fill_(fill)
      o = [torch.empty_like(t) for t in first]
      st = lib.snap_vote_credible_f32(
          ctypes.c_void_p(votes.data_ptr()), R, Ho, Wo, scale, host, L,
          None if gt_dev is None else ctypes.c_void_p(gt_dev.data_ptr()), *(ctypes.c_void_p(t.data_ptr()) for t in o),
          ctypes.c_void_p(ws.data_ptr()), nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
      assert st == 0
      outs.append(o)
    torch.cuda.synchronize()
    for o in outs:
      for a, b in zip(first, o):
        assert guarded.same_bits(a, b), name


def test_bad_arguments_raise_without_launching():
  votes = torch.zeros((4, 5, 6), device=DEV)
  for levels in ((0.9, 0.5), (0.5, 0.5), (0.0, 0.5), (0.5, 1.0), (), tuple(np.linspace(0.1, 0.9, 9)), (float('nan'),)):
    with pytest.raises(ValueError):
      ops.vote_credible(votes, levels)
  with pytest.raises(ValueError):
    ops.vote_credible(torch.zeros((65, 5, 5), device=DEV), (0.5,))
  for scale in (0.0, -2.0, float('inf'), float('nan')):
    with pytest.raises(ValueError):
      ops.vote_credible(votes, (0.5,), scale)
  with pytest.raises(ValueError):
    ops.vote_credible(votes[0], (0.5,))
  with pytest.raises(ValueError):
    ops.vote_credible(votes, (0.5,), 1.0, torch.zeros(2, device=DEV))
  lib = _lib.load()
  assert lib.snap_vote_credible_workspace_bytes(4, 5, 6, 0) == 0 and lib.snap_vote_credible_workspace_bytes(4, 5, 6, 9) == 0
  assert lib.snap_vote_credible_workspace_bytes(65, 5, 6, 3) == 0
  need = lib.snap_vote_credible_workspace_bytes(4, 5, 6, 8)
  ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=DEV)
  o = ([torch.full((8,), 7.0, device=DEV) for _ in range(2)] + [torch.full((64,), 7, dtype=torch.int32, device=DEV)]
       + [torch.full((n,), 7, dtype=torch.uint8, device=DEV) for n in (30, 4, 120)]
       + [torch.full((4,), 7.0, device=DEV), torch.full((4,), 7, dtype=torch.int32, device=DEV)])
  p = lambda t: ctypes.c_void_p(t.data_ptr())

  def call(R=4, scale=1.0, levels=(0.5, 0.9), L=None, nbytes=need, wsp=None, outs=None, vp=p(votes)):
    host = (ctypes.c_float * max(len(levels), 1))(*levels)
    outs = [p(t) for t in o] if outs is None else outs
    return lib.snap_vote_credible_f32(vp, R, 5, 6, scale, host, len(levels) if L is None else L, None, *outs,
                                      p(ws) if wsp is None else wsp, nbytes, None)

  assert call(R=65) == -1
  assert call(scale=0.0) == -2 and call(scale=float('nan')) == -2
  assert call(levels=(0.9, 0.5)) == -2 and call(levels=(0.5, 0.5)) == -2                 # unsorted
  assert call(levels=(0.0, 0.5)) == -2 and call(levels=(0.5, 1.0)) == -2                 # 0 and 1
  assert call(L=0) == -2 and call(levels=tuple(np.linspace(0.1, 0.9, 9))) == -2           # L = 0 and 9
  assert call(nbytes=lib.snap_vote_credible_workspace_bytes(4, 5, 6, 2) - 1) == -5         # short
  assert call(wsp=ctypes.c_void_p(ws.data_ptr() + 4)) == -5                                # misaligned
  assert call(vp=None) == -3
  for k in (0, 1, 2, 3, 4, 6, 7):                                # every output but level_cell
    outs = [p(t) for t in o]
    outs[k] = None
    assert call(outs=outs) == -3, k
  torch.cuda.synchronize()
  assert all(bool((t == 7).all()) for t in o)                  # nothing ran


@pytest.mark.parametrize('method,D', [('fft', 6), ('direct', 8)])
def test_credible_from_votes_and_localize_exhaustive(method, D):
  """A planted pose at 16^2, R = 8 (the posterior test's scene): the dict agrees with the reference on the votes the
  localizer returns; without the argument ``localize_exhaustive`` returns the same keys and bits as before."""
  H, R = 16, 8
  rng = np.random.default_rng(77 + H)
  grid = grids.Grid2D((H, H), 0.25)
  valid = torch.ones((H, H), dtype=torch.bool, device=DEV)
  fq = torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV)
  fm = torch.roll(torch.rot90(fq, 2, (0, 1)), (2, -1), (0, 1)).contiguous()
  pq, pm = types.FeaturePlane(features=fq, valid=valid), types.FeaturePlane(features=fm, valid=valid)
  base = pev.localize_exhaustive(pq, pm, R, grid, method=method)
  assert set(base) == {'map_t_query', 'index', 'score', 'count', 'votes'}
  gt_tf = pev.exhaustive_index_to_tfm(base['index'][0].to(torch.float32), grid, R)
  levels, temperature = (0.5, 0.9), 0.05
  with guarded.scope():
    out = pev.localize_exhaustive(pq, pm, R, grid, method=method,
                                  credible=dict(levels=levels, temperature=temperature, m_t_q_gt=gt_tf, cell_levels=True))
  assert set(out) == set(base) | {'credible'}
  for k in base:
    a, b = (base[k], out[k]) if k != 'map_t_query' else (base[k].t, out[k].t)
    assert guarded.same_bits(a, b), k
  cred = out['credible']
  assert set(cred) == {'threshold', 'mass', 'table', 'level_xy', 'level_r', 'level_cell', 'gt_stats', 'count', 'area_m2',
                       'yaw_span_deg', 'volume', 'gt_credibility', 'gt_level', 'gt_valid', 'covered'}
  votes = out['votes'].cpu().numpy()
  gt_idx = pev.exhaustive_tfm_to_index(gt_tf, grid, R).to(torch.float32).cpu().numpy()
  g, eps = ref.gap(votes, temperature, levels), ref.bound(votes, temperature)
  print(f'{method}: gap {g:.3e}, bound {eps:.3e}')
  assert g >= max(4 * eps, 1e-9)
  want = ref.vote_credible(votes, levels, temperature, gt_idx)
  _assert_equal(tuple(cred[k].cpu().numpy() for k in NAMES), want, eps, method)
  table = want[2]
  assert np.allclose(cred['area_m2'].cpu().numpy(), table[:, 1] * 0.0625, rtol=1e-6)
  assert np.allclose(cred['yaw_span_deg'].cpu().numpy(), table[:, 2] * 360 / R, rtol=1e-6)
  assert np.allclose(cred['volume'].cpu().numpy(), table[:, 0] * 0.0625 * 2 * np.pi / R, rtol=1e-6)
  # the planted pose is the best cell: nothing ranks above it, so it is in every region
  assert bool(cred['gt_valid']) and float(cred['gt_credibility']) == 0 and int(cred['gt_level']) == 0
  assert cred['covered'].cpu().tolist() == [True, True]
  plain = pev.localize_exhaustive(pq, pm, R, grid, method=method, credible=True)['credible']
  assert 'gt_credibility' not in plain and plain['level_cell'] is None and plain['threshold'].shape == (3,)
  g1 = ref.gap(votes, 1.0, ref.LEVELS3)
  assert g1 >= max(4 * ref.bound(votes, 1.0), 1e-9)
  w1 = ref.vote_credible(votes, ref.LEVELS3, 1.0)
  assert (plain['threshold'].cpu().numpy() == w1[0]).all() and (plain['table'].cpu().numpy() == w1[2]).all()


def test_vote_filter_credible():
  """``VoteFilter.credible`` works on the belief (log space, scale 1) and agrees with the reference on it."""
  H, R = 16, 8
  grid = grids.Grid2D((H, H), 0.25)
  v = ref.smooth_votes((R, 2 * H - 1, 2 * H - 1), seed=4)
  f = pev.VoteFilter(grid, R, sigma_xy=0.3, sigma_yaw=0.1, temperature=2.0)
  with pytest.raises(ValueError):
    f.credible()
  f.step(torch.from_numpy(v).to(DEV))
  belief = f.belief.cpu().numpy()
  gt_tf = pev.exhaustive_index_to_tfm(torch.tensor([3.0, 12.0, 20.0]), grid, R)
  out = f.credible(levels=(0.5, 0.9), m_t_q_gt=gt_tf)
  gt_idx = pev.exhaustive_tfm_to_index(gt_tf, grid, R).to(torch.float32).cpu().numpy()
  g, eps = ref.gap(belief, 1.0, (0.5, 0.9)), ref.bound(belief, 1.0)
  assert g >= max(4 * eps, 1e-9)
  want = ref.vote_credible(belief, (0.5, 0.9), 1.0, gt_idx)
  got = tuple(None if out[k] is None else out[k].cpu().numpy() for k in NAMES)
  _assert_equal(got, want, eps, 'filter')
  assert bool(out['gt_valid']) and out['covered'].cpu().tolist() == [bool(want[7][3] <= 0), bool(want[7][3] <= 1)]
  assert abs(float(out['gt_credibility']) - want[6][1]) <= 2 * eps + 2.0 ** -24
