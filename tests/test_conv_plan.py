"""CPU tests of ``ops.plan_conv``: which engine, weight image, split-K workspace and statistics layout
a ``conv2d`` launch gets is a pure function of shapes, dtypes, flags and the ``Tuning`` in force.

The expectations are literals: the values the launches below passed to ``snap_conv2d_nhwc_ex_f32`` BEFORE
the planner existed (recorded from ``conv2d`` with the launch replaced by a recorder), at the real layer
shapes of the C2 / C3 / C4 / C5 workloads.  Tensors are meta tensors: nothing is allocated."""
import pytest
import torch

from snap_amd import ops

BF, F16 = torch.bfloat16, torch.float16
GN, NONE, AFF, RELU = ops.PRO_GN_RELU, ops.PRO_NONE, ops.PRO_AFFINE, ops.PRO_RELU


def _t(*shape, dtype=torch.float32):
  return torch.empty(shape, dtype=dtype, device='meta')


def _plan(x, w, engine=None, tune=None, ps=False, pw=False, gn=False, res=False, bias=False, rows='', out_cols=None,
          gnb=None, **kw):
  """x = (N, H, W, Cs[, dtype]); w = (KH, KW, Cin, Cout); ps / pw: as PreSplit / PackedWeights."""
  dtype = x[4] if len(x) == 5 else torch.float32
  N, H, W, Cs = x[:4]
  KH, KW, Cin, Cout = w
  xt = ops.PreSplit(_t(N * H * W * Cs * 2, dtype=BF), x[:4]) if ps else _t(N, H, W, Cs, dtype=dtype)
  wt = ops.PackedWeights(_t(8, dtype=BF), w) if pw else _t(*w)
  (pt, pb), (pl, pr) = kw.get('padding', ((0, 0), (0, 0)))
  s = kw.get('stride', 1)
  Ho, Wo = (H + pt + pb - KH) // s + 1, (W + pl + pr - KW) // s + 1
  if gn is True:
    gn = (_t(N, Cin), _t(N, Cin), _t(Cin))
  if gn:
    kw.update(prologue=GN, gn=gn)
  if res:
    kw['residual'] = _t(N, Ho, Wo, Cout)
  if bias is not False:
    kw['bias'] = _t(Cout) if bias is True else bias
  if 'i' in rows:
    kw['rows_in'] = _t(N * Ho * Wo, dtype=torch.int32)
  if 'o' in rows:
    kw['rows_out'] = _t(N * Ho * Wo, dtype=torch.int32)
  if 'c' in rows:
    kw['row_count'] = _t(1, dtype=torch.int32)
  if out_cols is not None:
    kw['out'] = _t(N * Ho * Wo, out_cols)
  if gnb is not None:
    kw['gn_bwd_stats'] = (_t(N, Ho, Wo, Cout + gnb), _t(N, Cout), _t(N, Cout), _t(Cout), _t(Cout), GN)
  with ops.engine_scope(engine), ops.tuning_scope(**(tune or {})):
    plan = ops.plan_conv(xt, wt, **kw)
    asked = 'bf16x3' if ps else kw.get('math') or {BF: 'bf16', F16: 'fp16'}.get(dtype) or ops.precision()
    return plan, ops.kernel_image(w, asked)


P1, P3 = ((1, 1), (1, 1)), ((3, 3), (3, 3))
# StreetView ResNet stages at C2 (40 images of 544 x 544), the aerial / training sizes, ViT-B/16 tokens, voting banks
S1, S3, S4s, S4t = (40, 136, 136), (40, 34, 34), (8, 17, 17), (4, 17, 17)
VIT = (1, 1, 23120)

# (label, x, w, arguments) -> (engine, family, tag, image, parts, workspace bytes,
#                              (statistics bytes, buffers, gn_partial_rows, tile_rows, of relu(y)), GroupNorm-VJP statistics)
NOSTATS = (0, 0, 0, 0, False)
TABLE = [
    ('f32 tiled', S3 + (1024,), (1, 1, 1024, 256), dict(math='f32', gn=True, emit_gn_stats='raw'),
     ('f32', 'conv_igemm', '', None, 0, 0, (901120, 1, 0, 128, False), False)),
    ('bf16x3 tiled, both statistics', S1 + (256,), (1, 1, 256, 64), dict(math='bf16x3', gn=True, emit_gn_stats='both'),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3', 2, 0, (2990080, 2, 0, 128, False), False)),
    ('bf16x6', S1 + (256,), (1, 1, 256, 64), dict(math='bf16x6', gn=True, emit_gn_stats='both'),
     ('bf16x6', 'conv_split_bf16x6', '', 'bf16x6', 3, 0, (2990080, 2, 0, 128, False), False)),
    ('bf16', S1 + (256,), (1, 1, 256, 64), dict(math='bf16', gn=True, emit_gn_stats='raw'),
     ('bf16', 'conv_bf16', '', 'bf16', 0, 0, (2990080, 1, 0, 128, False), False)),
    ('fp16 from the scope, relu statistics', S1 + (256,), (1, 1, 256, 64), dict(engine='fp16', gn=True, emit_gn_stats='relu'),
     ('fp16', 'conv_fp16', '', 'fp16', 0, 0, (2990080, 1, 0, 128, True), False)),
    ('bf16x3 from the scope, no statistics', S1 + (256,), (1, 1, 256, 64), dict(engine='bf16x3'),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3', 2, 0, NOSTATS, False)),
    ('weight-stationary 1x1', S1 + (64,), (1, 1, 64, 256), dict(engine='bf16x3', gn=True, res=True, emit_gn_stats='raw'),
     ('bf16x3', 'conv_split_bf16x3', 'WS_', 'bf16x3', 2, 0, (47513600, 1, 0, 32, False), False)),
    ('weight-stationary 3x3', S1 + (64,), (3, 3, 64, 64), dict(math='bf16x3', padding=P1, gn=True, emit_gn_stats='both'),
     ('bf16x3', 'conv_split_bf16x3', 'WS_', 'bf16x3', 2, 0, (13926400, 2, 0, -680, False), False)),
    ('row-stationary 1x1', S3 + (256,), (1, 1, 256, 1024), dict(math='bf16x3', gn=True, res=True, emit_gn_stats='raw'),
     ('bf16x3', 'conv_split_bf16x3', 'RS_', 'bf16x3', 2, 0, (3604480, 1, 0, 128, False), False)),
    ('... is a two-part kernel', S3 + (256,), (1, 1, 256, 1024), dict(math='bf16x6', gn=True, res=True, emit_gn_stats='raw'),
     ('bf16x6', 'conv_split_bf16x6', '', 'bf16x6', 3, 0, (3604480, 1, 0, 128, False), False)),
    ('no stationary kernels', S1 + (64,), (1, 1, 64, 256), dict(math='bf16x3', gn=True, res=True, tune=dict(CONV_NO_RS=True)),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3', 2, 0, NOSTATS, False)),
    ('no weight-stationary kernels', S1 + (64,), (1, 1, 64, 256), dict(math='bf16x3', gn=True, res=True, tune=dict(CONV_NO_WS=True)),
     ('bf16x3', 'conv_split_bf16x3', 'RS_', 'bf16x3', 2, 0, NOSTATS, False)),
    ('split-K + statistics', S4s + (512,), (3, 3, 512, 512), dict(math='bf16x3', padding=P1, gn=True, emit_gn_stats='both'),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3', 2, 52084736, (360448, 1, 32, 32, False), False)),
    ('split-K + statistics, bf16', S4t + (512,), (3, 3, 512, 512), dict(math='bf16', padding=P1, gn=True, emit_gn_stats='relu'),
     ('bf16', 'conv_bf16', '', 'bf16', 0, 47349760, (180224, 1, 32, 32, True), False)),
    ('split-K, f32: no statistics', S4s + (512,), (3, 3, 512, 512), dict(math='f32', padding=P1, gn=True, emit_gn_stats='raw'),
     ('f32', 'conv_igemm', '', None, 0, 52084736, NOSTATS, False)),
    ('split-K, SPLITK_STATS off', S4s + (512,), (3, 3, 512, 512),
     dict(math='bf16x3', padding=P1, gn=True, emit_gn_stats='both', tune=dict(SPLITK_STATS=False)),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3', 2, 52084736, NOSTATS, False)),
    ('USE_SPLITK off', S4s + (512,), (3, 3, 512, 512),
     dict(math='bf16x3', padding=P1, gn=True, emit_gn_stats='both', tune=dict(USE_SPLITK=False)),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3', 2, 0, (131072, 2, 0, 128, False), False)),
    ('forced tile', S3 + (1024,), (1, 1, 1024, 256), dict(math='bf16x3', gn=True, emit_gn_stats='both', tune=dict(CONV_TILE='64x64')),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3', 2, 0, (1638400, 2, 0, 64, False), False)),
    ('RGB root', (40, 544, 544, 4), (7, 7, 3, 64), dict(math='bf16x3', stride=2, padding=P3, cin=3, prologue=AFF),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3/root', 2, 0, NOSTATS, False)),
    ('RGB root with statistics: f32', (40, 544, 544, 4), (7, 7, 3, 64),
     dict(math='bf16x6', stride=2, padding=P3, cin=3, prologue=AFF, emit_gn_stats='raw'),
     ('f32', 'conv_igemm', '', None, 0, 0, (11878400, 1, 0, 128, False), False)),
    ('RGB root, bf16: f32', (40, 544, 544, 4), (7, 7, 3, 64), dict(math='bf16', stride=2, padding=P3, cin=3, prologue=AFF),
     ('f32', 'conv_igemm', '', None, 0, 0, NOSTATS, False)),
    ('Cin = 3', (8, 136, 136, 4), (3, 3, 3, 64), dict(math='bf16x3', padding=P1, cin=3, prologue=AFF, emit_gn_stats='both'),
     ('f32', 'conv_igemm', '', None, 0, 0, (598016, 2, 0, 128, False), False)),
    ('ViT patch embedding', (20, 544, 544, 3), (16, 16, 3, 768), dict(engine='bf16', stride=16, prologue=AFF, bias=True),
     ('f32', 'conv_igemm', '', None, 0, 0, NOSTATS, False)),
    ('over-large split image: f32', (1, 300, 300, 64), (256, 256, 64, 1024), dict(math='bf16x3'),
     ('f32', 'conv_igemm', '', None, 0, 49766400, NOSTATS, False)),
    ('stacked template bank', (1, 321, 321, 32), (66, 66, 32, 576), dict(math='bf16x3', stride=3),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3', 2, 0, NOSTATS, False)),
    ('... pre-split, packed by hand', (1, 321, 321, 32), (66, 66, 32, 576), dict(ps=True, pw=True, stride=3, ps_tile=3),
     ('bf16x3', 'conv_split_bf16x3', 'PS_', 'bf16x3', 2, 153363456, NOSTATS, False)),
    ('pre-split + statistics', S1 + (256,), (1, 1, 256, 64), dict(ps=True, res=True, emit_gn_stats='raw'),
     ('bf16x3', 'conv_split_bf16x3', 'PS_', 'bf16x3', 2, 0, (2990080, 1, 0, 128, False), False)),
    ('pre-split, both', S1 + (256,), (1, 1, 256, 64),
     dict(ps=True, res=True, emit_gn_stats='both', math='bf16x3', ps_tile=1, res_init=False),
     ('bf16x3', 'conv_split_bf16x3', 'PS_', 'bf16x3', 2, 0, (2990080, 2, 0, 128, False), False)),
    ('pre-split, split-K', S4s + (512,), (3, 3, 512, 512), dict(ps=True, padding=P1, emit_gn_stats='raw'),
     ('bf16x3', 'conv_split_bf16x3', 'PS_', 'bf16x3', 2, 52084736, NOSTATS, False)),
    ('one-part ring', VIT + (768, BF), (1, 1, 768, 3072), dict(math='bf16', bf16_ring=True, out_half=True),
     ('bf16', 'conv_bf16', 'PS1_', 'bf16/ps1', 1, 0, NOSTATS, False)),
    ('ring off', VIT + (768, BF), (1, 1, 768, 3072), dict(bf16_ring=True, bias=True, tune=dict(BF16_PS=False)),
     ('bf16', 'conv_bf16', '', 'bf16', 0, 0, NOSTATS, False)),
    ('bf16 input', VIT + (768, BF), (1, 1, 768, 3072), dict(math='bf16'),
     ('bf16', 'conv_bf16', '', 'bf16', 0, 0, NOSTATS, False)),
    ('fp16 input', VIT + (768, F16), (1, 1, 768, 3072), dict(res=True),
     ('fp16', 'conv_fp16', '', 'fp16', 0, 0, NOSTATS, False)),
    ('GroupNorm-VJP statistics', (20, 68, 68, 128, BF), (3, 3, 128, 128), dict(padding=P1, gnb=0),
     ('bf16', 'conv_bf16', '', 'bf16', 0, 0, (778240, 1, 0, 128, False), True)),
    ('... silently not with another shape', (20, 68, 68, 128, BF), (3, 3, 128, 128), dict(padding=P1, gnb=4),
     ('bf16', 'conv_bf16', '', 'bf16', 0, 0, NOSTATS, False)),
    ('row lists', (1, 1, 739840, 128), (1, 1, 128, 160), dict(math='bf16x3', prologue=RELU, bias=True, rows='ioc', out_cols=160),
     ('bf16x3', 'conv_split_bf16x3', '', 'bf16x3', 2, 0, NOSTATS, False)),
    ('half output, Cin = 257 in rows of 272', (1, 1, 3932160, 272), (1, 1, 257, 256),
     dict(math='bf16', cin=257, bias=True, relu=True, rows='ic', out_half=True),
     ('bf16', 'conv_bf16', '', 'bf16', 0, 0, NOSTATS, False)),
    ('out_stride', (1, 1, 262144, 160), (1, 1, 160, 128), dict(math='bf16', rows='oc', out_cols=144, out_stride=144),
     ('bf16', 'conv_bf16', '', 'bf16', 0, 0, NOSTATS, False)),
]


@pytest.mark.parametrize('label,x,w,kw,want', TABLE, ids=[r[0] for r in TABLE])
def test_plan_matches_the_recorded_launch(label, x, w, kw, want):
  p, (img_math, img_parts, img_packed) = _plan(x, w, **dict(kw))
  got = (p.engine, p.family, p.tag, p.image, p.parts, p.workspace_bytes,
         (p.stats_bytes, p.stats_count, p.gn_partial_rows, p.tile_rows, p.stats_relu), p.gnb)
  assert got == want
  # the shared rule gives the image the plan asks ``_packed_weights`` for; the two images with a layout of their
  # own (RGB root: Cin = 3, no ordinary image; one-part ring) are prepared on demand under the key's suffix
  key, _, special = (p.image or '').partition('/')
  if special == 'root':
    assert not img_packed and (img_math, img_parts) == (key, p.parts)
  elif special == 'ps1':
    assert img_packed and img_math == key == 'bf16' and p.parts == 1
  elif p.image is None:
    assert not img_packed or x[3] % 4
  else:
    assert img_packed and (img_math, img_parts) == (p.image, p.parts)
  assert p.w_split_parts == p.parts and p.extras == bool(
      p.image or p.workspace_bytes or p.stats_bytes or kw.get('rows') or p.bk_hint or p.tune_flags)
  assert p.out_shape[3] == w[3] and p.out_dtype == (
      {'bf16': BF, 'fp16': F16}[p.engine] if kw.get('out_half') else torch.float32)


def test_plan_scalar_extras_and_tile_hint():
  S3x, w = S3 + (1024,), (1, 1, 1024, 256)
  p = _plan(S3x, w, math='bf16x3')[0]
  assert (p.desc.tile_hint, p.bk_hint, p.tune_flags, p.w_split_root, p.w_half, p.x_half, p.x_presplit) == (0,) * 7
  assert _plan(S3x, w, math='bf16x3', tune=dict(CONV_RS_FORCE=True))[0].desc.tile_hint == 2000000
  assert _plan(S3x, w, math='bf16x3', tune=dict(CONV_RS_FORCE=True, CONV_NO_WS=True))[0].desc.tile_hint == 4000000
  assert _plan(S3x, w, math='bf16x3', tune=dict(CONV_TILE='128x64', CONV_NO_RS=True))[0].desc.tile_hint == 1128064
  p = _plan(S3x, w, math='f32', tune=dict(CONV_BK=32))[0]
  assert (p.bk_hint, p.tune_flags, p.extras, p.image) == (32, 0, True, None)
  flags = lambda **t: _plan(S1 + (64,), (3, 3, 64, 64), math='bf16x3', padding=P1, tune=t)[0].tune_flags
  assert (flags(CONV_NO_HALO=True), flags(CONV_NO_PLAIN=True), flags(CONV_RS_NSPLIT=2)) == (1, 8, 32)
  # an f32 launch with nothing to say passes no SnapConvExtras at all
  assert not _plan(S3x, w, math='f32')[0].extras
  p = _plan((40, 544, 544, 4), (7, 7, 3, 64), math='bf16x3', stride=2, padding=P3, cin=3)[0]
  assert (p.w_split_parts, p.w_split_root, p.x_half) == (2, 1, 0)
  p = _plan(VIT + (768, F16), (1, 1, 768, 3072))[0]
  assert (p.w_half, p.x_half, p.x_presplit) == (1, 1, 0)
  p = _plan(VIT + (768, BF), (1, 1, 768, 3072), bf16_ring=True, ps_tile=1, tune=dict(PS_TILE=2))[0]
  assert (p.w_split_parts, p.x_half, p.x_presplit, p.ps_tile, p.ps_res_init) == (1, 0, 1, 1, 0)
  p = _plan((1, 321, 321, 32), (66, 66, 32, 576), ps=True, pw=True, stride=3, ps_tile=3)[0]
  assert (p.x_presplit, p.ps_tile, p.ps_res_init) == (1, 3, 1)
  p = _plan(S1 + (256,), (1, 1, 256, 64), ps=True, res=True, res_init=False, tune=dict(PS_TILE=2))[0]
  assert (p.x_presplit, p.ps_tile, p.ps_res_init) == (1, 2, 0)


def test_kernel_image_is_what_the_pack_passes_skip():
  assert ops.kernel_image((1, 1, 256, 64), 'bf16x3') == ('bf16x3', 2, True)
  assert ops.kernel_image((1, 1, 256, 64), 'bf16x6') == ('bf16x6', 3, True)
  assert ops.kernel_image((1, 1, 256, 64), 'fp16') == ('fp16', 0, True)
  assert ops.kernel_image((1, 1, 256, 64), 'f32') == ('f32', 0, False)
  assert ops.kernel_image((7, 7, 3, 64), 'bf16x3') == ('bf16x3', 2, False)      # Cin < 4: the f32 engine (or the root image)
  assert ops.kernel_image((3, 3, 3, 64), 'bf16') == ('bf16', 0, False)
  assert ops.kernel_image((256, 256, 64, 1024), 'bf16x3') == ('f32', 0, False)  # beyond the 32-bit offsets
  assert ops.kernel_image((256, 256, 64, 512), 'bf16x3') == ('bf16x3', 2, True)
  assert ops.kernel_image((256, 256, 64, 1024), 'bf16') == ('bf16', 0, True)
  assert not ops.conv2d_presplit_supported((1, 600, 600, 64), (256, 256, 64, 1024))
  assert ops.conv2d_presplit_supported((1, 321, 321, 32), (66, 66, 32, 576), 3)
  assert not ops.conv2d_presplit_supported((1, 321, 321, 24), (66, 66, 24, 576), 3)


RAISES = [
    ('a half-precision input takes the matching engine', VIT + (768, BF), (1, 1, 768, 3072), dict(math='fp16')),
    ('a half-precision input takes the matching engine', VIT + (768, BF), (1, 1, 768, 3072), dict(gn=True)),
    ('a half-precision input takes the matching engine', VIT + (768, BF), (1, 1, 768, 3072), dict(emit_gn_stats='raw')),
    ('a half-precision input takes the matching engine', (1, 4, 4, 12, BF), (1, 1, 12, 8), {}),
    ('a half-precision input AND output need the one-part', VIT + (768, BF), (1, 1, 768, 3072), dict(math='bf16', out_half=True)),
    ('a PreSplit input takes prologue NONE', S1 + (256,), (1, 1, 256, 64), dict(ps=True, math='bf16')),
    ('a PreSplit input takes prologue NONE', S1 + (256,), (1, 1, 256, 64), dict(ps=True, gn=True)),
    ('a PreSplit input takes prologue NONE', S1 + (256,), (1, 1, 256, 64), dict(ps=True, rows='o', out_cols=64)),
    ('PackedWeights .* go with a PreSplit input', S1 + (256,), (1, 1, 256, 64), dict(pw=True, math='bf16x3')),
    ('the pre-split engine needs Cin % 16 == 0', (1, 4, 4, 8), (1, 1, 8, 8), dict(ps=True)),
    ('kernel expects Cin=1024, input has 7', S3 + (1024,), (1, 1, 1024, 256), dict(cin=7)),
    ("math='int8'", S3 + (1024,), (1, 1, 1024, 256), dict(math='int8')),
    ('out_half needs a training-precision engine launch', S3 + (1024,), (1, 1, 1024, 256), dict(math='f32', out_half=True)),
    ('out_half needs a training-precision engine launch', S3 + (1024,), (1, 1, 1024, 256), dict(math='bf16', out_half=True, gn=True)),
    ('out_half needs a training-precision engine launch', (1, 4, 4, 8), (1, 1, 8, 6), dict(math='bf16', out_half=True)),
    ('out_stride goes with out', S3 + (1024,), (1, 1, 1024, 256), dict(out_stride=260)),
    ('out_stride needs out', S3 + (1024,), (1, 1, 1024, 256), dict(out_cols=262, out_stride=262)),
    ('out_stride needs out', S3 + (1024,), (1, 1, 1024, 256), dict(out_cols=260, out_stride=260, res=True)),
    ('out has the wrong size', S3 + (1024,), (1, 1, 1024, 256), dict(out_cols=260)),
    ('GroupNorm statistics have the wrong size', S3 + (1024,), (1, 1, 1024, 256), dict(gn=(_t(3), _t(40, 1024), _t(1024)))),
    ('bias size', S3 + (1024,), (1, 1, 1024, 256), dict(bias=_t(5))),
    (r'residual \(1, 2, 3, 4\) vs \(40, 34, 34, 256\)', S3 + (1024,), (1, 1, 1024, 256), dict(residual=_t(1, 2, 3, 4))),
    ('up_prev shape', S3 + (1024,), (1, 1, 1024, 256), dict(up_prev=_t(1, 2, 3, 4))),
    ('row_mask size', S3 + (1024,), (1, 1, 1024, 256), dict(row_mask=_t(5, dtype=torch.bool))),
]


@pytest.mark.parametrize('match,x,w,kw', RAISES, ids=[f'{i}-{r[0][:24]}' for i, r in enumerate(RAISES)])
def test_plan_raises_what_conv2d_raised(match, x, w, kw):
  with pytest.raises(ValueError, match='conv2d: ' + match):
    _plan(x, w, **dict(kw))


def test_conv2d_still_checks_its_tensors_first():
  """The launcher refuses what the plan cannot see (device, dtype, contiguity) before it plans."""
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    ops.conv2d(torch.zeros(1, 4, 4, 8), torch.zeros(1, 1, 8, 8), cin=7)
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    ops.dense(torch.zeros(16, 8), torch.zeros(8, 8), out=torch.zeros(16, 12), out_stride=12)
