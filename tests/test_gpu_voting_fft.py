"""`-m gpu`: the frequency-domain voting (``voting_fft.hip`` / ``voting_fft_body.h``) at EVERY transform size it has
(N = 16 ... 1024, each once on either axis, at the largest and at the smallest map that needs it, plus 342 x 342)
against ``voting_fft_reference.py``: the -inf mask exact against the integer counts and the reference's threshold
rule, finite scores within ``MARGIN`` x the per-rotation bound of float64, the argmax wherever float64 decides it,
planted deltas at the place and value the closed form gives, counts on the threshold, degenerate rows, containment.

The comparison functions (``check_*``) take numpy arrays only: tests/test_voting_fft_reference.py runs mutants of the
reference through them.  See tests/README.md, "Frequency-domain voting".
"""
import numpy as np
import pytest
import torch

import voting_fft_reference as V

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHARES = {}          # worst observed share of the tolerance (MARGIN x bound) per transform size; README records them
AXIS = V.axis_geometries()
AXIS_IDS = [g['name'] for g in AXIS]


# ------------------------------- comparison functions (numpy) ---------------------------------
def check_mask(name, got, counts, thr):
  """-inf exactly where the integer count fails ``count > f32(thr)``; no escape class."""
  got, counts = np.asarray(got), np.asarray(counts)
  assert got.dtype == np.float32 and got.shape == counts.shape, f'{name}: {got.dtype} {got.shape} != {counts.shape}'
  want = V.finite_rule(counts, thr)
  bad = np.isneginf(got) != ~want
  if bad.any():
    i = tuple(int(v) for v in np.argwhere(bad)[0])
    raise AssertionError(f'{name}: {int(bad.sum())} cells of the -inf mask differ, first at {i}: count {counts[i]} '
                         f'against {float(np.float32(thr))!r}, got {got[i]!r}')
  return want


def check_scores(name, got, want, bound, key, where=None):
  """Within MARGIN x bound[r] of the float64 scores ``want`` on the cells ``where`` (default: all); float64
  non-finite values there (NaN of an empty template) must be met as such."""
  got, want = np.asarray(got), np.asarray(want, np.float64)
  assert got.dtype == np.float32 and got.shape == want.shape, f'{name}: {got.dtype} {got.shape} != {want.shape}'
  where = np.ones(want.shape, bool) if where is None else where
  tol = np.broadcast_to(V.MARGIN * np.asarray(bound, np.float64)[:, None, None], want.shape)
  fin = where & np.isfinite(want) & np.isfinite(tol)
  with np.errstate(invalid='ignore'):
    odd = where & ~np.isfinite(want) & ~((got == want) | (np.isnan(got) & np.isnan(want)))
  assert not odd.any(), f'{name}: non-finite float64 scores not met, first at {np.argwhere(odd)[0].tolist()}'
  assert np.isfinite(got[fin]).all(), f'{name}: non-finite scores where float64 is finite'
  err = np.abs(got.astype(np.float64) - np.where(fin, want, 0.0))[fin]
  share = err / tol[fin]
  if share.size and share.max() > 1.0:
    k = int(np.argmax(share))
    raise AssertionError(f'{name}: {int((share > 1).sum())} scores beyond {V.MARGIN:g} x bound, worst error '
                         f'{err[k]:.3e} against a tolerance of {tol[fin][k]:.3e}')
  if share.size:
    SHARES[key] = max(SHARES.get(key, 0.0), float(share.max()))


def check_argmax(name, got, want, finite, bound):
  """argmax per rotation equals float64's wherever its top-two gap exceeds 2 x MARGIN x bound[r].
  Returns the number of rotations float64 decided."""
  got = np.asarray(got)
  w = np.where(finite, np.asarray(want, np.float64), -np.inf).reshape(len(want), -1)
  decided = 0
  for r in range(len(w)):
    if not np.isfinite(bound[r]) or np.isfinite(w[r]).sum() < 2:
      continue
    top = np.partition(w[r], -2)[-2:]
    if top[1] - top[0] > 2 * V.MARGIN * bound[r]:
      decided += 1
      a = int(np.nanargmax(np.where(np.isnan(got[r].reshape(-1)), -np.inf, got[r].reshape(-1))))
      assert a == int(np.argmax(w[r])), f'{name}: rotation {r}: argmax {a}, float64 {int(np.argmax(w[r]))}'
  return decided


def check_case(name, got, c, key):
  """One axis case (voting_fft_reference.axis_case) with the default overlap test."""
  fin = check_mask(name, got, c['counts'], c['thr'])
  check_scores(name, got, c['raw'], c['bound'], key, where=fin)
  return check_argmax(name, got, c['raw'], fin, c['bound'])


def check_planted(name, got, want, bound, key):
  """Planted deltas: every nonzero of the closed form at its place with its value, everything else 0, within the
  bound."""
  assert np.count_nonzero(want) > 0
  check_scores(name, got, want, bound, key)


# ------------------------------- running the kernels ---------------------------------
def _t(a):
  return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run_matching(q, tv, m, mv, min_overlap=0.05, method='fft'):
  from snap_amd.models import pose_exhaustive_voting as pev
  return pev.template_matching(_t(q), _t(tv), _t(m), _t(mv), min_overlap=min_overlap, method=method).cpu().numpy()


def run_entry(q, tv, m, mv, tcount, thr, use_overlap=True):
  from snap_amd import ops
  return ops.voting_fft(_t(q), None if tv is None else _t(tv), _t(m), None if mv is None else _t(mv),
                        _t(np.asarray(tcount, np.float32)), thr, use_overlap=use_overlap).cpu().numpy()


def _sizes(g):
  geo = V.geometry(g['H'], g['W'], g['Hm'], g['Wm'])
  want = (g['N'], 64) if g['axis'] == 1 else (64, g['N'])
  assert (geo['N1'], geo['N2']) == want, (g['name'], geo)        # the size under test IS reached, on its axis
  return geo


def test_case_table_reaches_every_size_on_both_axes():
  from snap_amd import ops
  reached = {(V.geometry(g['H'], g['W'], g['Hm'], g['Wm'])['N1'], V.geometry(g['H'], g['W'], g['Hm'], g['Wm'])['N2'])
             for g in AXIS}
  assert reached == {(N, 64) for N in V.GPU_SIZES} | {(64, N) for N in V.GPU_SIZES}
  for g in AXIS + [V.SQUARE]:
    assert ops.voting_fft_supported(g['R'], g['H'], g['W'], g['D'], g['Hm'], g['Wm']), g['name']
  assert {g['R'] for g in AXIS} == {1, 2, 3, 17, 20} and {g['D'] for g in AXIS} == {2, 6, 16, 18, 34}


@pytest.mark.parametrize('kind', ['noise', 'offset'])
@pytest.mark.parametrize('name', AXIS_IDS)
def test_every_transform_size(name, kind):
  """A / B(i, ii) / C / D: unit noise (all-valid masks at the largest maps: the largest counts) and 10 + noise with
  partial validity, at every N on either axis."""
  c = V.axis_case(name, kind)
  g = c['g']
  _sizes(g)
  got = run_matching(c['q'], c['tv'], c['m'], c['mv'])
  assert check_case(f'{name} {kind}', got, c, g['N']) > 0


@pytest.mark.parametrize('name', AXIS_IDS)
def test_planted_deltas(name):
  """B(iii): one nonzero template cell per rotation and one nonzero map cell per channel -- corners, interior, the
  middle of each border -- read out where the closed form puts them (no overlap test, null masks)."""
  g = {c['name']: c for c in AXIS}[name]
  _sizes(g)
  q, m, want, _ = V.planted(g)
  tc = np.full(V.PLANT_R, V.PLANT_TCOUNT, np.float32)
  got = run_entry(q, None, m, None, tc, 0.0, use_overlap=False)
  check_planted(f'{name} planted', got, want, V.bound(q, m, tc), g['N'])


def _rotated(fq, vq, fm, vm, R, cell, min_overlap=0.05):
  """The rotated entry, and the explicit templates the stand-alone rotate kernel samples from the same plane."""
  from snap_amd.models import pose_exhaustive_voting as pev
  from snap_amd.models import types
  from snap_amd.utils import grids
  H = fq.shape[0]
  grid = grids.Grid2D((H, H), cell)
  t, tv = pev.sample_query_templates(_t(fq), _t(vq), R, grid)
  got = pev.exhaustive_pose_voting(types.FeaturePlane(_t(fq), _t(vq)), types.FeaturePlane(_t(fm), _t(vm)), R, grid,
                                   method='fft', min_overlap=min_overlap)
  return got.cpu().numpy(), t.cpu().numpy(), tv.cpu().numpy().astype(bool)


@pytest.mark.parametrize('name', [n for n in AXIS_IDS if '-max-' in n])
def test_rotated_entry_at_every_transform_size(name):
  """The rotated entry (templates sampled inside the first transform) on the largest map of every N: float64 on the
  templates ``sample_query_templates`` gives for the same plane."""
  g = {c['name']: c for c in AXIS}[name]
  _sizes(g)
  H, R = min(g['Hm'], g['Wm']), (20 if g['N'] <= 64 else 4)
  D = -(-g['D'] // 4) * 4                   # (the stand-alone rotate kernel, the source of the templates, takes D % 4 == 0)
  rng = np.random.default_rng(g['N'] * 8 + g['axis'])
  vq = rng.random((H, H)) > 0.15
  fq = (rng.standard_normal((H, H, D)) * vq[..., None]).astype(np.float32)
  fm = rng.standard_normal((g['Hm'], g['Wm'], D)).astype(np.float32)
  vm = rng.random((g['Hm'], g['Wm'])) > 0.1
  got, t, tv = _rotated(fq, vq, fm, vm, R, 0.25)
  tc = tv.sum((-1, -2)).astype(np.float64)
  fin = check_mask(name, got, V.counts64(tv, vm), V.threshold(0.05, H, H))
  check_scores(f'{name} rotated', got, V.raw64(t, fm) / tc[:, None, None], V.bound(t, fm, tc), g['N'], where=fin)


def test_square_map_of_342_cells():
  """N = 1024 on both axes, all-valid masks (counts up to 342^2 = 116 964), 10 + noise: the dynamic-LDS attribute
  branch and the thread cap of the launcher; outputs inside guards."""
  import guarded
  from snap_amd import ops
  c = V.axis_case('N1024-square', 'offset')
  g = c['g']
  assert (V.geometry(342, 342, 342, 342)['N1'], V.geometry(342, 342, 342, 342)['N2']) == (1024, 1024)
  assert (c['counts'][0] == V.counts_all_valid(342, 342, 342, 342)).all() and c['counts'].max() == 116964
  args = [_t(a) for a in (c['q'], c['tv'], c['m'], c['mv'])] + [_t(c['tcount'].astype(np.float32))]
  with guarded.scope() as sc:
    got_t = ops.voting_fft(*args, float(0.05 * 342 * 342))
    sc.check()
    assert int(guarded.unwritten(got_t).sum()) == 0
    got = got_t.cpu().numpy()
  assert check_case('342 x 342', got, c, 1024) > 0
  again = ops.voting_fft(*args, float(0.05 * 342 * 342)).cpu().numpy()
  assert (again.view(np.uint32) == got.view(np.uint32)).all()


def test_square_map_of_342_cells_rotated_entry():
  rng = np.random.default_rng(342)
  vq = rng.random((342, 342)) > 0.15
  fq = (rng.standard_normal((342, 342, 4)) * vq[..., None]).astype(np.float32)
  fm = rng.standard_normal((342, 342, 4)).astype(np.float32)
  vm = rng.random((342, 342)) > 0.1
  got, t, tv = _rotated(fq, vq, fm, vm, 4, 0.25)
  tc = tv.sum((-1, -2)).astype(np.float64)
  fin = check_mask('342 rotated', got, V.counts64(tv, vm), V.threshold(0.05, 342, 342))
  check_scores('342 rotated', got, V.raw64(t, fm) / tc[:, None, None], V.bound(t, fm, tc), 1024, where=fin)


# ------------------------------- D: counts on the threshold ---------------------------------
@pytest.mark.parametrize('H,W,Hm,Wm', V.THRESHOLD_GEOMETRIES)
def test_counts_on_the_threshold(H, W, Hm, Wm):
  """All-valid masks: the count is the area of the overlap rectangle.  threshold = k passed straight to the entry:
  count == k is -inf, count == k + 1 is finite, for k = 0, 1, HW - 1, HW."""
  R, D = 2, 2
  rng = np.random.default_rng(H * 1000 + Hm)
  q = (1.0 + rng.random((R, H, W, D))).astype(np.float32)
  m = (1.0 + rng.random((Hm, Wm, D))).astype(np.float32)
  tv, mv = np.ones((R, H, W), bool), np.ones((Hm, Wm), bool)
  area = V.counts_all_valid(H, W, Hm, Wm)
  counts = np.broadcast_to(area, (R,) + area.shape)
  tc = np.full(R, H * W, np.float32)
  raw = V.raw64(q, m) / (H * W)
  for k in V.threshold_values(H, W):
    got = run_entry(q, tv, m, mv, tc, float(k))
    fin = check_mask(f'k={k}', got, counts, k)
    assert (area == k).any() and np.isneginf(got[:, area == k]).all()
    if k < H * W:
      assert (area == k + 1).any() and np.isfinite(got[:, area == k + 1]).all()
    else:
      assert not fin.any()
    check_scores(f'k={k}', got, raw, V.bound(q, m, tc), max(V.geometry(H, W, Hm, Wm)['N1'], V.geometry(H, W, Hm, Wm)['N2']), where=fin)


@pytest.mark.parametrize('min_overlap,H', V.ROTATED_THRESHOLDS)
def test_rotated_entry_applies_the_reference_threshold(min_overlap, H):
  """min_overlap x H x H is an integer that an f32 chain of products misses by one ulp (8, 1, 63, 12; 20 for the
  default, which it does not miss): a pose whose count EQUALS it is -inf on every path -- the rotated entry, the
  explicit entry and the direct form on the templates sampled from the same plane."""
  fq, vq, fm, vm = V.rotated_inputs(min_overlap, H)
  got, t, tv = _rotated(fq, vq, fm, vm, V.ROTATED_R, V.ROTATED_CELL, min_overlap)
  counts, thr = V.counts64(tv, vm), V.threshold(min_overlap, H, H)
  assert float(thr) == round(min_overlap * H * H)
  on = int((counts == int(thr)).sum())
  print(f'min_overlap={min_overlap} H={H}: threshold {float(thr)}, {on} cells with count == threshold')
  assert on > 0
  check_mask('explicit entry', run_matching(t, tv, fm, vm, min_overlap, 'fft'), counts, thr)
  check_mask('direct form', run_matching(t, tv, fm, vm, min_overlap, 'direct'), counts, thr)
  check_mask('rotated entry', got, counts, thr)


# ------------------------------- E: degenerate rows ---------------------------------
def test_degenerate_rows():
  g = dict(name='degenerate', H=11, W=9, Hm=16, Wm=11, R=5, D=6)
  q, tv, m, mv = V.build(g, 'offset')
  q, tv = q.copy(), tv.copy()
  q[2] = 0; tv[2] = False                                 # a wholly invalid template: tcount[2] == 0
  tc = tv.sum((-1, -2)).astype(np.float64)
  counts, b = V.counts64(tv, mv), V.bound(q, m, tc)
  got = run_matching(q, tv, m, mv)
  fin = check_mask('empty template', got, counts, V.threshold(0.05, 11, 9))
  assert np.isneginf(got[2]).all() and fin.any()
  check_scores('empty template', got, V.scores64(q, tv, m, mv, 0.05), b, 48, where=fin)
  want = V.scores64(q, tv, m)                               # no overlap test: 0 / 0
  assert np.isnan(want[2]).all()
  got = run_matching(q, tv, m, mv, min_overlap=None)
  assert np.isnan(got[2]).all()
  check_scores('empty template, no overlap test', got, want, b, 48)
  got = run_matching(q, tv, m, np.zeros_like(mv))           # an all-invalid map
  assert np.isneginf(got).all()
  got = run_entry(q, None, m, None, np.maximum(tc, 1), 0.0, use_overlap=False)     # null masks
  check_scores('null masks', got, V.scores64(q, tv, m, tcount=np.maximum(tc, 1)), V.bound(q, m, np.maximum(tc, 1)), 48)


# ------------------------------- what the entries refuse ---------------------------------
def test_refusals_carry_their_status():
  from snap_amd import _lib, ops
  lib = _lib.load()
  p = lambda t: t.data_ptr()
  ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
  f = torch.zeros(4 * 4 * 4 * 2, device=DEV)
  b = torch.ones(4 * 4 * 4, dtype=torch.uint8, device=DEV)
  out = torch.zeros(1 << 12, device=DEV)

  def explicit(R, H, W, D, Hm, Wm, nbytes=ws.numel(), tvalid=p(b)):
    return lib.snap_voting_fft_f32(p(f), tvalid, p(f), p(b), p(f), R, H, W, D, Hm, Wm, 0.0, 1, p(ws), nbytes, p(out), None)

  def rotated(R, H, D, Hm, Wm):
    return lib.snap_voting_fft_rotated_f32(p(f), p(b), p(f), 0.25, p(f), p(b), R, H, D, Hm, Wm, 0.0, p(ws), ws.numel(),
                                           p(out), None)
  assert explicit(4, 4, 4, 2, 343, 4) == _lib.SNAP_ERR_UNSUPPORTED          # 3 * 343 - 2 > 1024 points
  assert explicit(4, 4, 4, 2, 4, 343) == _lib.SNAP_ERR_UNSUPPORTED
  assert explicit(4, 11, 4, 2, 4, 4) == _lib.SNAP_ERR_UNSUPPORTED           # a template beyond the padded map: Ho = 0
  assert explicit(0, 4, 4, 2, 4, 4) == _lib.SNAP_ERR_BAD_SHAPE
  assert explicit(4, 4, 4, 2, 4, 4, nbytes=256) == _lib.SNAP_ERR_WORKSPACE
  assert explicit(4, 4, 4, 2, 4, 4, tvalid=None) == _lib.SNAP_ERR_NULL
  assert rotated(6, 4, 2, 4, 4) == _lib.SNAP_ERR_BAD_SHAPE                  # R % 4 != 0
  assert rotated(4, 4, 2, 343, 4) == _lib.SNAP_ERR_UNSUPPORTED
  assert rotated(4, 11, 2, 4, 4) == _lib.SNAP_ERR_UNSUPPORTED
  assert ops.voting_fft_workspace_bytes(4, 10, 4, 2, 4, 4) > 0 and not ops.voting_fft_supported(4, 11, 4, 2, 4, 4)
  torch.cuda.synchronize()
  assert float(out.abs().sum()) == 0.0                                      # a refused call writes nothing


# ------------------------------- F: containment and repeatability ---------------------------------
@pytest.mark.parametrize('name', ['N192-max-axis1', 'N512-max-axis2', 'N1024-max-axis1', 'N1024-min-axis2'])
def test_containment_and_repeatability(name):
  """NaN / +-inf planted in ONE template leave every other rotation bit-equal to the clean run; two runs are
  bit-equal; outputs inside a guarded scope with the guards intact and every score written."""
  import guarded
  g = dict({c['name']: c for c in AXIS}[name], R=5, D=6)
  _sizes(g)
  q, tv, m, mv = V.build(g, 'offset')
  clean = run_matching(q, tv, m, mv)
  assert (run_matching(q, tv, m, mv).view(np.uint32) == clean.view(np.uint32)).all()
  bad = q.copy()
  i, j = np.argwhere(tv[3])[0]
  bad[3, i, j, 0], bad[3, i, j, 1], bad[3, -1, -1, 2] = np.nan, np.inf, -np.inf
  got = run_matching(bad, tv, m, mv)
  others = [0, 1, 2, 4]
  assert (got[others].view(np.uint32) == clean[others].view(np.uint32)).all()
  assert not np.isfinite(got[3][np.isfinite(clean[3])]).any()
  from snap_amd import ops
  args = [_t(a) for a in (q, tv, m, mv)] + [_t(tv.sum((-1, -2)).astype(np.float32))]
  with guarded.scope() as sc:
    out = ops.voting_fft(*args, float(0.05 * g['H'] * g['W']))
    sc.check()
    assert int(guarded.unwritten(out).sum()) == 0
    assert (out.cpu().numpy().view(np.uint32) == clean.view(np.uint32)).all()


def test_zz_report_shares():
  """Prints the worst observed share of MARGIN x bound per transform size (tests/README.md records them)."""
  print('SHARES ' + ' '.join(f'{k}:{v:.3f}' for k, v in sorted(SHARES.items())))
  assert all(v <= 1.0 for v in SHARES.values())
