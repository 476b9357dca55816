"""`-m gpu`: the refusals of the vote-volume wrappers of ``snap_amd.ops``, as one table of bad calls.

Every entry is a call that is good but for ONE argument, on a volume of [3, 4, 5] with taps of Tk = Ta = Tb = 1 and
K = L = 1.  The table gives the exception class per wrapper and kind of mistake: the wrappers that check their volume
through ``_chk`` raise TypeError for a non-tensor or another dtype and RuntimeError for a CPU tensor, the ones that
check it through ``_arg_chk`` raise ValueError throughout, and every refused scale, ``uniform_mix``, ``gt_index`` shape
or unsupported ``R`` is a ValueError.  Every message starts with the wrapper's name, and a refused call has allocated
nothing (the checks run in front of the first ``torch.empty``)."""
import numpy as np
import pytest
import torch

import guarded
import helpers
from snap_amd import ops

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
R, HO, WO = 3, 4, 5


def _vol(kind='good', dtype=torch.float32, lead=()):
  """The volume argument, good or with one mistake (``lead``: vote_fuse's frame axis)."""
  if kind == '2d':
    return torch.zeros((HO, WO), dtype=dtype, device=DEV)
  if kind == 'noncontig':
    return torch.zeros(lead + (R, HO, 2 * WO), dtype=dtype, device=DEV)[..., ::2]
  v = torch.zeros(lead + (65 if kind == 'R65' else R, HO, WO), dtype=dtype, device=DEV)
  return dict(good=v, R65=v, cpu=v.cpu(), f64=v.double(), nontensor=v.cpu().numpy())[kind]


def _planes(v):
  return v.shape[-3] if isinstance(v, torch.Tensor) and v.dim() >= 3 else R


def _taps(v):
  n = _planes(v)
  one = torch.ones((n, 1), dtype=torch.float32, device=DEV)
  return torch.ones((1,), dtype=torch.float32, device=DEV), 0, one, one.clone(), torch.zeros((n, 2), dtype=torch.int32,
                                                                                            device=DEV)


def _i32(*shape):
  return torch.zeros(shape, dtype=torch.int32, device=DEV)


def _gt(kind):
  g = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device=DEV)
  return dict(shape2=g[:2].contiguous(), cpu=g.cpu(), f64=g.double())[kind]


def _plane_align(fq):
  fm = torch.zeros((R, HO, WO), dtype=torch.float32, device=DEV)
  valid = torch.ones((R, HO), dtype=torch.bool, device=DEV)
  return ops.plane_align_score(fq, valid, fm, valid.clone(), torch.zeros((1, 4), dtype=torch.float32, device=DEV), 0.0)


# wrapper -> (how it checks its volume, the volume arguments by name, the call): ``a`` holds the volumes by name and
# 'scale*' / 'uniform_mix' / 'gt_index', each good unless the entry replaces it.
CHK, ARG = 'chk', 'arg'
WRAPPERS = {
    'vote_peaks': (CHK, ('votes',), lambda a: ops.vote_peaks(a['votes'], 1)),
    'vote_posterior': (CHK, ('votes',), lambda a: ops.vote_posterior(a['votes'], a['scale'], a['gt_index'])),
    'vote_credible': (CHK, ('votes',), lambda a: ops.vote_credible(a['votes'], (0.5,), a['scale'], a['gt_index'])),
    'vote_modes': (CHK, ('votes',), lambda a: ops.vote_modes(a['votes'], _i32(1, 3), 1, 1, a['scale'], a['gt_index'])),
    'vote_recall': (CHK, ('votes',), lambda a: ops.vote_recall(a['votes'], [1], [0], _i32(1, 3), a['scale'],
                                                               a['gt_index'])),
    'vote_odometry': (CHK, ('prev', 'cur'), lambda a: ops.vote_odometry(a['prev'], a['cur'], 0, 1, None, a['scale'],
                                                                        a['scale_cur'])),
    'vote_fuse': (CHK, ('volumes',), lambda a: ops.vote_fuse(
        a['volumes'], torch.zeros((1, _planes(a['volumes']), 3), dtype=torch.float32, device=DEV))),
    'vote_filter': (ARG, ('votes', 'belief'), lambda a: ops.vote_filter(a['belief'], a['votes'], _taps(a['votes']),
                                                                        a['scale'], a['uniform_mix'])),
    'vote_smooth': (ARG, ('belief', 'smoothed_next'), lambda a: ops.vote_smooth(
        a['belief'], a['smoothed_next'], _taps(a['belief']), a['uniform_mix'])),
    'vote_pairs': (ARG, ('belief', 'smoothed_next'), lambda a: ops.vote_pairs(
        a['belief'], a['smoothed_next'], _taps(a['belief']), a['uniform_mix'])),
    'vote_viterbi': (ARG, ('votes', 'score_prev'), lambda a: ops.vote_viterbi(a['score_prev'], a['votes'],
                                                                              _taps(a['votes']), a['scale'])),
    'vote_backstep': (ARG, ('back',), lambda a: ops.vote_backstep(a['back'], _i32(1))),
    'vote_sample': (ARG, ('votes',), lambda a: ops.vote_sample(a['votes'], 1, 0, 0, a['scale'])),
    'vote_sample_back': (ARG, ('belief',), lambda a: ops.vote_sample_back(a['belief'], _i32(1), _taps(a['belief']),
                                                                          a['uniform_mix'], 0)),
    'plane_align_score': (CHK, ('fq',), lambda a: _plane_align(a['fq'])),
}
TAKES = {
    'scale': ('vote_posterior', 'vote_credible', 'vote_modes', 'vote_recall', 'vote_odometry', 'vote_filter',
              'vote_viterbi', 'vote_sample'),
    'scale_cur': ('vote_odometry',),
    'uniform_mix': ('vote_filter', 'vote_smooth', 'vote_pairs', 'vote_sample_back'),
    'gt_index': ('vote_posterior', 'vote_credible', 'vote_modes', 'vote_recall'),
    # the wrappers whose C side limits R to 64 (vote_peaks, vote_modes and vote_backstep take any R that fits an int32
    # cell count; plane_align_score has no R)
    'R65': tuple(op for op in WRAPPERS if op not in ('vote_peaks', 'vote_modes', 'vote_backstep', 'plane_align_score')),
}
VOLUME_ERRORS = {CHK: dict(cpu=RuntimeError, f64=TypeError, nontensor=TypeError, noncontig=ValueError),
                 ARG: dict(cpu=ValueError, f64=ValueError, nontensor=ValueError, noncontig=ValueError)}
VOLUME_ERRORS[CHK]['2d'] = VOLUME_ERRORS[ARG]['2d'] = ValueError
GT_ERRORS = dict(shape2=ValueError, cpu=RuntimeError, f64=TypeError)


def _table():
  """(id, wrapper, the argument replaced, what replaces it, the exception class)."""
  rows = []
  for op, (style, volumes, _) in WRAPPERS.items():
    for name in volumes:
      for kind, exc in VOLUME_ERRORS[style].items():
        rows.append((f'{op}-{name}-{kind}', op, name, kind, exc))
    if op in TAKES['R65']:
      rows.append((f'{op}-R65', op, None, 'R65', ValueError))
    for arg in ('scale', 'scale_cur'):
      if op in TAKES[arg]:
        rows += [(f'{op}-{arg}-{v}', op, arg, v, ValueError) for v in (0, -1, float('inf'), float('nan'), 1e39)]
    if op in TAKES['uniform_mix']:
      rows += [(f'{op}-uniform_mix-{v}', op, 'uniform_mix', v, ValueError) for v in (-0.1, 1.5, float('nan'))]
    if op in TAKES['gt_index']:
      rows += [(f'{op}-gt_index-{kind}', op, 'gt_index', kind, exc) for kind, exc in GT_ERRORS.items()]
  return rows


TABLE = _table()


def test_the_table_covers_every_wrapper():
  names = [n for n in dir(ops) if n.startswith('vote_') and callable(getattr(ops, n))] + ['plane_align_score']
  assert sorted(names) == sorted(WRAPPERS)
  assert {row[1] for row in TABLE} == set(WRAPPERS)


@pytest.mark.parametrize('op,arg,value,exc', [row[1:] for row in TABLE], ids=[row[0] for row in TABLE])
def test_bad_call_is_refused(op, arg, value, exc):
  style, volumes, call = WRAPPERS[op]
  dtype = torch.int32 if op == 'vote_backstep' else torch.float32
  lead = (1,) if op == 'vote_fuse' else ()
  # every volume of the call has R planes: 65 of them in the R65 entries
  a = {name: _vol('R65' if value == 'R65' else 'good', dtype, lead) for name in volumes}
  a.update(scale=1.0, scale_cur=1.0, uniform_mix=0.0, gt_index=None)
  if arg in volumes:
    a[arg] = _vol(value, dtype, lead)
  elif arg == 'gt_index':
    a[arg] = _gt(value)
  elif arg is not None:
    a[arg] = value
  with guarded.scope() as sc:
    with pytest.raises(exc) as info:
      call(a)
    print(f'{op}: {type(info.value).__name__}: {info.value}')
    assert type(info.value) is exc
    assert str(info.value).startswith(op + ':'), str(info.value)
    assert not sc.allocations(), 'a refused call allocated nothing'


def test_good_calls_are_taken():
  """The table's good call of every wrapper runs: each entry above fails for its one mistake alone."""
  for op, (style, volumes, call) in WRAPPERS.items():
    dtype = torch.int32 if op == 'vote_backstep' else torch.float32
    a = {name: _vol('good', dtype, (1,) if op == 'vote_fuse' else ()) for name in volumes}
    a.update(scale=1.0, scale_cur=1.0, uniform_mix=0.0, gt_index=None)
    if op == 'plane_align_score':                  # (D % 4 == 0: the one wrapper whose good call needs another shape)
      a['fq'] = torch.zeros((R, HO, 8), dtype=torch.float32, device=DEV)
      fm, valid = torch.zeros((R, HO, 8), dtype=torch.float32, device=DEV), torch.ones((R, HO), dtype=torch.bool,
                                                                                      device=DEV)
      out = ops.plane_align_score(a['fq'], valid, fm, valid.clone(), torch.zeros((1, 4), dtype=torch.float32,
                                                                                 device=DEV), 0.0)
    else:
      out = call(a)
    assert out is not None, op
  torch.cuda.synchronize()
