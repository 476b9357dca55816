"""The fused ResNet stem (``ops.conv2d_root_pool``: 7x7/2 root conv + 3x3/2 max-pool in one launch) against the two
launches it replaces, ``ops.conv2d`` -> ``ops.max_pool_3x3s2``, on the same inputs: bit equality, no tolerance.  The
reference is always the two existing kernels (the tiled root kernel below the weights-stationary kernel's row
threshold, that kernel itself with ``CONV_RS_FORCE``: both give the same bits)."""
import ctypes

import pytest
import torch

import helpers
from snap_amd import _lib, ops
from test_gpu_containment import contained
from test_gpu_kernels import rnd

pytestmark = pytest.mark.gpu

DEV = helpers.DEVICE
PAD = ((3, 3), (3, 3))

# (N, H, W): conv output (H / 2, W / 2) rounded up, pooled output half of that rounded up
SHAPES = {
    'one_tile': (2, 64, 64),          # conv 32: exactly one 32-pixel row tile, two column tiles of 15 pooled pixels
    'tile_plus_one': (2, 64, 66),     # conv 33
    'tile_minus_one': (2, 64, 62),    # conv 31
    'odd': (3, 38, 70),               # conv 19 x 35: the last pooled row and column have two taps
    'short': (1, 6, 128),             # conv 3 rows: shorter than one band
    'bands': (1, 160, 96),            # conv 80 rows = 40 pooled rows: several bands
}


def _image(N, H, W, seed):
  x = rnd((N, H, W, 4), seed)
  x[..., 3] = 0.0                     # pad_to_multiple(channel_pad=1)
  return x.to(DEV).contiguous()


def _kernel(seed, cout=64, k=7):
  return (rnd((k, k, 3, cout), seed) * 0.2).to(DEV).contiguous()


def _two_launches(x, w, **kw):
  return ops.max_pool_3x3s2(ops.conv2d(x, w, stride=2, padding=PAD, cin=3, **kw))


def _bits(t):
  return t.contiguous().view(torch.int32)


def _affine(on):
  return dict(prologue=ops.PRO_AFFINE, in_affine=(2.0, -1.0)) if on else {}


@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'plain'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_fused_stem_matches_the_two_launches(name, affine):
  N, H, W = SHAPES[name]
  x, w = _image(N, H, W, 11), _kernel(12)
  kw = _affine(affine)
  with ops.engine_scope('bf16x3'):
    want = _two_launches(x, w, **kw)
    assert ops.conv2d_root_pool_supported(x, w, cin=3, **kw)
    # 0: the band length the launcher chooses; 3 and 7 do not divide the 40 pooled rows of 'bands'
    for band in (0, 3, 7) if name == 'bands' else (0, 2):
      got = ops.conv2d_root_pool(x, w, cin=3, band_rows=band, **kw)
      assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (name, band)
  if name == 'one_tile':
    # ... and against the weights-stationary root kernel itself (below its row threshold only on request)
    with ops.engine_scope('bf16x3'), ops.tuning_scope(CONV_RS_FORCE=True):
      assert torch.equal(_bits(_two_launches(x, w, **kw)), _bits(want))


def test_fused_stem_relu_epilogue():
  N, H, W = SHAPES['odd']
  x, w = _image(N, H, W, 21), _kernel(22)
  with ops.engine_scope('bf16x3'):
    want = _two_launches(x, w, relu=True, **_affine(True))
    got = ops.conv2d_root_pool(x, w, cin=3, relu=True, **_affine(True))
  assert bool((want == 0).any()) and torch.equal(_bits(got), _bits(want))


def test_fused_stem_nan_and_inf():
  """A NaN and a -inf in the image reach the output only through the conv: the same elements are NaN, every other
  element has the same bits."""
  N, H, W = SHAPES['odd']
  x, w = _image(N, H, W, 31), _kernel(32)
  x[1, 17, 33, 1] = float('nan')
  x[2, 3, 69, 0] = float('-inf')
  x[0, 0, 0, 2] = float('-inf')
  with ops.engine_scope('bf16x3'):
    want = _two_launches(x, w)
    got = ops.conv2d_root_pool(x, w, cin=3)
  nan = torch.isnan(want)
  assert bool(nan.any()) and not bool(nan.all())
  assert torch.equal(torch.isnan(got), nan)
  assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def test_unsupported_shapes_take_the_two_launches():
  lib = _lib.load()

  def desc(cout=64, k=7, stride=2, pad=3):
    H = W = 64
    Ho = (H + 2 * pad - k) // stride + 1
    return _lib.SnapConvDesc(N=1, H=H, W=W, Cin=3, Cin_stride=4, KH=k, KW=k, stride=stride, pad_t=pad, pad_l=pad,
                             Ho=Ho, Wo=Ho, Cout=cout, Cout_stride=cout, prologue=ops.PRO_NONE, epilogue=0,
                             in_scale=1.0, in_shift=0.0, tile_hint=0)

  assert lib.snap_conv2d_root_pool_supported(ctypes.byref(desc()), 2) == 1
  assert lib.snap_conv2d_root_pool_supported(ctypes.byref(desc(cout=128)), 2) == 0
  assert lib.snap_conv2d_root_pool_supported(ctypes.byref(desc(k=3, stride=1, pad=1)), 2) == 0
  assert lib.snap_conv2d_root_pool_supported(ctypes.byref(desc()), 3) == 0
  one = torch.zeros(64, device=DEV)
  for d, parts in ((desc(cout=128), 2), (desc(k=3, stride=1, pad=1), 2), (desc(), 3)):
    st = lib.snap_conv2d_root_pool_f32(ctypes.byref(d), one.data_ptr(), one.data_ptr(), 1 << 20, parts, 0,
                                       one.data_ptr(), None)
    assert st == -2, st                                         # SNAP_ERR_UNSUPPORTED: nothing launched
  # the wrapper: 128 output channels and the three-part engine run as conv2d -> max_pool_3x3s2
  x = _image(2, 64, 64, 41)
  for cout, engine in ((128, 'bf16x3'), (64, 'bf16x6')):
    w = _kernel(42, cout)
    with ops.engine_scope(engine):
      assert not ops.conv2d_root_pool_supported(x, w, cin=3)
      assert torch.equal(_bits(ops.conv2d_root_pool(x, w, cin=3)), _bits(_two_launches(x, w)))
  with ops.engine_scope('bf16x3'), ops.tuning_scope(FUSE_STEM=False):
    assert not ops.conv2d_root_pool_supported(x, _kernel(42), cin=3)


def test_fused_stem_writes_all_of_its_output_and_nothing_else():
  N, H, W = SHAPES['odd']
  x, w = _image(N, H, W, 51), _kernel(52)
  with ops.engine_scope('bf16x3'):
    assert ops.conv2d_root_pool_supported(x, w, cin=3, **_affine(True))
    contained(lambda x, w: ops.conv2d_root_pool(x, w, cin=3, **_affine(True)), [x, w], ['value', 'value'])


def test_resnet_inference_is_bit_identical_with_and_without_the_fused_stem():
  """The smallest encoder whose root block has 64 channels (the tiny test config's width 0.5 gives 32, which the
  fused kernel does not take)."""
  from snap_amd.configs import defaults
  from snap_amd.models import base, resnet
  cfg = defaults.resnet()
  cfg.depth = [1, 1]
  cfg.width = 1
  cfg.limit_num_blocks = 2
  enc = resnet.ResNetV2(cfg)
  assert not cfg.skip_root_block
  params = helpers.params_to_device(enc.init_params(torch.Generator().manual_seed(0), 'cpu'), DEV)
  image = _image(2, 70, 98, 61)
  outs = {}
  for fuse in (True, False):
    base.clear_caches()
    with torch.no_grad(), ops.engine_scope('bf16x3'), ops.tuning_scope(FUSE_STEM=fuse):
      prof = ops.KernelProfiler()
      ops.set_profiler(prof)
      try:
        outs[fuse] = enc(params, image)
      finally:
        ops.set_profiler(None)
      torch.cuda.synchronize()
      tags = [str(r[4]) for recs in prof.records.values() for r in recs]
      assert any('POOL_' in t for t in tags) == fuse, tags
  a, b = outs[True], outs[False]
  assert torch.equal(_bits(a['stem']), _bits(b['stem']))
  last = sorted(a['stage2'])[-1]
  assert torch.equal(_bits(a['stage2'][last]), _bits(b['stage2'][last]))
