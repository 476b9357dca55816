"""`-m gpu`: ``ops.vote_peaks`` (vote_peaks.hip) and the host entry points built on it, against the numpy
restatement ``vote_peaks_reference``.  Every comparison is exact: indices are integers, scores are copies of the
input's bits (compared through an int32 view).

The kernel tiles a volume into (rotation, 16-row band, 64-column block) tiles and runs at most 1024 workgroups, each
striding over its tiles and folding their peaks into one running best K.  The three small shapes have one column
block and one tile per workgroup: partial tiles, row bands, the rotation wrap and the merge of the per-workgroup
lists.  ``[36, 113, 520]`` has 8 bands x 9 column blocks x 36 = 2592 tiles, two or three per workgroup: column
halos that hold real data, plateaus and ties across block borders, the stride loop, the fold of new peaks into a
best K that already exists and its K-th-key pruning -- on both kernel bodies (radius (1, 1) and the generic one).
The data kinds put plateaus and cross-tile ties, fewer peaks than K, NaN / +-inf and the corners there.  Every kernel
call runs under ``guarded.scope()``: guard regions intact, and no output element left unwritten.  An index row of -1
has the bits of the 0xFF poison, so ``test_empty_rows_are_written`` repeats the short lists under another poison
byte.
"""
import functools

import numpy as np
import pytest
import torch

import guarded
import helpers
import vote_peaks_reference as ref
from snap_amd import ops
from snap_amd.models import pose_exhaustive_voting as pev
from snap_amd.models import types
from snap_amd.utils import grids

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
SHAPES = [(4, 5, 7), (8, 31, 33), (36, 63, 63), (36, 113, 520)]
SETTINGS = [(1, 1, 1), (16, 1, 1), (64, 2, 4), (5, 0, 2)]      # (K, radius_r, radius_xy)
KINDS = ['normal', 'quantised', 'mostly_minus_inf', 'corners', 'nan_beside_maxima', 'all_minus_inf']


@functools.lru_cache(maxsize=None)
def _votes(shape, kind):
  R, Ho, Wo = shape
  rng = np.random.default_rng(1000 * KINDS.index(kind) + sum(shape))
  v = rng.standard_normal(shape).astype(np.float32)
  corners = [(r, a, b) for r in (0, R - 1) for a in (0, Ho - 1) for b in (0, Wo - 1)]
  if kind in ('quantised', 'mostly_minus_inf'):
    v = np.clip(np.round(v), -2, 2).astype(np.float32)        # (np.round leaves -0.0 behind: -0 == +0 ties)
  if kind == 'mostly_minus_inf':
    keep = v[[R - 1, 0], Ho - 2:, :3].copy()                  # two rotations across the wrap, 2 x 3 cells each
    v[:] = -np.inf
    v[[R - 1, 0], Ho - 2:, :3] = keep
  if kind == 'corners':
    for c in corners:
      v[c] = 10.0                                             # equal values: the wrap neighbours tie
    if Ho > 16 and Wo > 64:                                   # ... and across a band and a column-block border
      for r in (0, 1, R - 1):
        v[r, 15, 63] = v[r, 16, 64] = 10.0
      v[2, 15, 64], v[2, 16, 63] = 9.0, 9.5
  if kind == 'nan_beside_maxima':
    for i, (r, a, b) in enumerate(corners):
      v[r, a, b] = np.inf if i == 3 else 20.0 + i
      v[r, a, min(b + 1, Wo - 1) if b == 0 else b - 1] = np.nan
    v[R // 2, Ho // 2, Wo // 2] = 30.0
    v[R // 2, Ho // 2 - 1, Wo // 2] = np.nan
    v[(R // 2 + 1) % R, Ho // 2, Wo // 2] = np.nan
    if Ho > 16 and Wo > 64:                                   # a maximum whose NaN neighbours lie in other tiles
      v[1, 15, 63] = 40.0
      v[1, 16, 64] = v[1, 15, 64] = v[2, 15, 63] = np.nan
  if kind == 'all_minus_inf':
    v[:] = -np.inf
  v.setflags(write=False)
  return v


@functools.lru_cache(maxsize=None)
def _want(shape, kind, setting):
  return ref.vote_peaks(_votes(shape, kind), *setting)


def _run(votes_dev, setting, accept_minus_one=None):
  """One guarded call -> numpy (index, score, count).  Asserts intact guards and fully written outputs;
  ``accept_minus_one``: boolean [K] of the index rows that are -1 by contract (the poison's own bits)."""
  k = setting[0]
  with guarded.scope() as sc:
    index, score, count = ops.vote_peaks(guarded.place(votes_dev, 'value'), *setting)
    assert tuple(index.shape) == (k, 3) and index.dtype == torch.int32
    assert tuple(score.shape) == (k,) and score.dtype == torch.float32
    assert tuple(count.shape) == (2,) and count.dtype == torch.int32
    un_i = guarded.unwritten(index).cpu().numpy()
    if accept_minus_one is not None:
      un_i = un_i & ~accept_minus_one[:, None]
    assert not un_i.any(), f'index: rows never written: {np.flatnonzero(un_i.any(-1)).tolist()}'
    assert not bool(guarded.unwritten(score).any()), 'score: elements never written'
    assert not bool(guarded.unwritten(count).any()), 'count: elements never written'
    out = index.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
  return out


def _assert_equal(got, want, what):
  gi, gs, gc = got
  wi, ws, wc = want
  assert gc.tolist() == wc.tolist(), f'{what}: count {gc.tolist()} != {wc.tolist()}'
  bad = np.flatnonzero((gi != wi).any(-1) | (gs.view(np.int32) != ws.view(np.int32)))
  assert bad.size == 0, (f'{what}: {bad.size} row(s) differ, first {bad[0]}: got {gi[bad[0]].tolist()} {gs[bad[0]]!r}, '
                         f'want {wi[bad[0]].tolist()} {ws[bad[0]]!r}')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('setting', SETTINGS, ids=lambda s: 'K%d_r%d_xy%d' % s)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_vote_peaks_equals_the_restatement(shape, setting, kind):
  votes = torch.from_numpy(_votes(shape, kind).copy()).to(DEV)
  if not ref.supported(shape, *setting):                       # (4 rotations cannot hold a window of 5)
    with pytest.raises(ValueError):
      ops.vote_peaks(votes, *setting)
    return
  want = _want(shape, kind, setting)
  if kind == 'mostly_minus_inf' and setting[0] > 1:
    assert 0 < want[2][0] < setting[0]                          # fewer peaks than K
  if kind == 'all_minus_inf':
    assert want[2][0] == 0
  if kind == 'nan_beside_maxima':
    assert want[2][1] == int(np.isnan(_votes(shape, kind)).sum()) > 0
  got = _run(votes, setting, accept_minus_one=(want[0] == -1).all(-1))
  _assert_equal(got, want, f'{shape} {setting} {kind}')


@pytest.mark.parametrize('kind', ['mostly_minus_inf', 'all_minus_inf'])
def test_empty_rows_are_written(kind, monkeypatch):
  """Rows past the found count hold index -1 = the bits of the guarded allocator's 0xFF poison: under the poison
  byte 0xEE a row the kernel skipped would show."""
  monkeypatch.setattr(guarded, 'POISON', 0xEE)
  shape, setting = (8, 31, 33), (16, 1, 1)
  want = _want(shape, kind, setting)
  assert want[2][0] < setting[0]
  got = _run(torch.from_numpy(_votes(shape, kind).copy()).to(DEV), setting)
  _assert_equal(got, want, kind)


@pytest.mark.parametrize('kind', ['normal', 'quantised', 'corners'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_k1_equals_argmax_rows(shape, kind):
  """On NaN-free data the single best peak is the volume's first maximum: the existing argmax kernel's answer."""
  v = _votes(shape, kind)
  votes = torch.from_numpy(v.copy()).to(DEV)
  flat = int(ops.argmax_rows(votes.reshape(1, -1))[0])
  for rr, rx in ((1, 1), (0, 2)):
    index, score, count = _run(votes, (1, rr, rx))
    r, a, b = index[0].tolist()
    assert (r * shape[1] + a) * shape[2] + b == flat == int(np.argmax(v))
    assert score.view(np.int32)[0] == v.reshape(-1)[flat].view(np.int32) and count.tolist() == [1, 0]


def test_two_calls_give_identical_bytes():
  for shape, setting, kind in (((36, 63, 63), (64, 2, 4), 'quantised'), ((8, 31, 33), (16, 1, 1), 'nan_beside_maxima'),
                               ((36, 113, 520), (64, 2, 4), 'quantised'), ((36, 113, 520), (16, 1, 1), 'normal')):
    votes = torch.from_numpy(_votes(shape, kind).copy()).to(DEV)
    first = ops.vote_peaks(votes, *setting)
    torch.empty(1 << 20, device=DEV).fill_(float('nan'))       # (stir the allocator's free blocks)
    second = ops.vote_peaks(votes, *setting)
    for a, b in zip(first, second):
      assert guarded.same_bits(a, b)


@pytest.mark.parametrize('method,D', [('fft', 6), ('direct', 8)])
def test_localize_exhaustive_query_equal_to_map(method, D):
  """The smallest geometry of the frequency-domain voting's containment test (H = 8, R = 8, D = 6), query = map:
  the list is the restatement's on the returned votes, the best pose is the identity placement (0, H-1, W-1), and
  its transform is ``exhaustive_index_to_tfm`` of that index.  Once more on the direct form, whose template kernel
  takes whole groups of four channels: the same H and R with D = 8."""
  H, R = 8, 8
  rng = np.random.default_rng(295 + H)
  valid = torch.tensor(rng.random((H, H)) > 0.15).to(DEV)
  feat = (torch.tensor(rng.standard_normal((H, H, D)).astype(np.float32)).to(DEV) * valid[..., None]).contiguous()
  plane = types.FeaturePlane(features=feat, valid=valid)
  grid = grids.Grid2D((H, H), 0.25)
  with guarded.scope():
    out = pev.localize_exhaustive(plane, plane, R, grid, method=method)
  assert set(out) == {'map_t_query', 'index', 'score', 'count', 'votes'}
  votes = out['votes'].cpu().numpy()
  assert votes.shape == (R, 2 * H - 1, 2 * H - 1)
  want = ref.vote_peaks(votes, 16, 1, 1)
  _assert_equal((out['index'].cpu().numpy(), out['score'].cpu().numpy(), out['count'].cpu().numpy()), want, method)
  assert out['index'][0].tolist() == [0, H - 1, H - 1]
  tfs = out['map_t_query']
  assert tuple(tfs.shape) == (16,)
  one = pev.exhaustive_index_to_tfm(out['index'][0], grid, R)
  assert torch.equal(tfs.angle[0], one.angle) and torch.equal(tfs.t[0], one.t)
  assert float(tfs.angle[0]) == 0.0 and tfs.t[0].abs().max().item() < 0.25       # half a cell: the +0.5 offset
  # the batched helper gives the same bits on the device as on the host, and NaN for rows without a peak
  host = pev.exhaustive_indices_to_tfm(out['index'].cpu(), grid, R)
  assert guarded.same_bits(tfs.angle.cpu(), host.angle) and guarded.same_bits(tfs.t.cpu(), host.t)
  found = int(out['count'][0])
  assert not bool(torch.isnan(tfs.t[:found]).any()) and bool(torch.isnan(tfs.t[found:]).all())
  # other settings reach the kernel through **peaks
  few = pev.localize_exhaustive(plane, plane, R, grid, method=method, num_peaks=3, radius_r=0, radius_xy=2)
  _assert_equal(tuple(few[n].cpu().numpy() for n in ('index', 'score', 'count')),
                ref.vote_peaks(few['votes'].cpu().numpy(), 3, 0, 2), method + ' K=3')
