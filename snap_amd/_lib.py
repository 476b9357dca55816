"""ctypes binding of libsnap_hip.so, derived from the C ABI's own header.

include/snap_hip.h is the only statement of the ABI: at import this module reads it and builds
``SIGNATURES`` (name -> (restype, argtypes) of every prototype), one ``ctypes.Structure`` per
``typedef struct`` and the header's integer constants (enumerators and ``#define SNAP_*``), all
module attributes under their header names.  To add an entry point, declare it in the header and
bump ``SNAP_ABI_VERSION`` there; nothing is repeated here.  ``parse_header`` refuses (ValueError)
any declaration it does not fully understand: a symbol that slipped through would be called with
ctypes' default convention.

There is NO fallback: if the shared library is missing or a symbol is absent the
import of :mod:`snap_amd.ops` raises.  Build it with ``make -C snap_amd/csrc`` or
``python -c "import __graft_entry__ as g; g.build()"``.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# SNAP_HIP_LIB: alternative build of the same ABI (A/B experiments); default = in-tree.
LIB_PATH = os.environ.get('SNAP_HIP_LIB') or os.path.join(_HERE, 'lib', 'libsnap_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'snap_hip.h')

_SCALARS = {
    'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64,
    'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double,
}
# what a pointer may point to besides a scalar above or a struct declared earlier in the header
_POINTEES = {'void', 'char', 'uint8_t', 'uint32_t'}
# The structs the host fills and passes by reference travel as typed pointers; every other pointer,
# the device arrays of the *Item structs included, travels as a raw address.
_BY_REFERENCE = {'SnapConvDesc', 'SnapConvExtras', 'SnapLiftDesc'}

_DECLARATION = re.compile(r'''
    (?:typedef\s+)?enum\s*\w*\s*\{(?P<enumerators>[^{}]*)\}\s*\w*\s*;
  | typedef\s+struct\s+\w+\s*\{(?P<members>[^{}]*)\}\s*(?P<struct>\w+)\s*;
  | (?P<restype>[\w\s*]+?)\b(?P<function>snap_[a-z0-9_]+)\s*\((?P<params>[^()]*)\)\s*;
''', re.X)
_MEMBER = re.compile(r'([\w\s*]+?[\s*])(\w+(?:\s*,\s*\w+)*)')   # type, then one or more plain names
_PARAM = re.compile(r'([\w\s*]+?[\s*])\w+')


def _int_expr(text):
  """Value of an expression of integer literals, ``<<`` and ``|``; int() names any other text."""
  value = 0
  for term in text.split('|'):
    first, *shifts = term.split('<<')
    v = int(first, 0)
    for s in shifts:
      v <<= int(s, 0)
    value |= v
  return value


def _ctype(text, structs, returned=False):
  """The ctypes type of a C type written without its declarator name."""
  words = text.replace('*', ' ').split()
  base = ' '.join(w for w in words if w != 'const')
  stars = text.count('*')
  if not stars and base in _SCALARS:
    return _SCALARS[base]
  if stars and (base in _SCALARS or base in _POINTEES or base in structs):
    if stars == 1 and base in _BY_REFERENCE and base in structs:
      return ctypes.POINTER(structs[base])
    if stars == 1 and base == 'char' and returned:
      return ctypes.c_char_p
    return ctypes.c_void_p
  raise ValueError(f'snap_hip.h: unknown type {text.strip()!r}')


def _struct(name, members, structs):
  fields = []
  for member in filter(None, (m.strip() for m in members.split(';'))):
    m = _MEMBER.fullmatch(member)   # arrays, function pointers and bit fields do not match
    names = m and m.group(2).replace(',', ' ').split()
    if not m or ('*' in m.group(1) and len(names) > 1):
      raise ValueError(f'snap_hip.h: struct {name}: cannot read member {member!r}')
    fields += [(n, _ctype(m.group(1), structs)) for n in names]
  return type(name, (ctypes.Structure,), {'_fields_': fields})


def _argtypes(name, params, structs):
  if params.strip() == 'void':
    return []
  argtypes = []
  for param in params.split(','):
    m = _PARAM.fullmatch(param.strip())   # arrays and unnamed parameters do not match
    if not m:
      raise ValueError(f'snap_hip.h: {name}: cannot read parameter {param.strip()!r}')
    argtypes.append(_ctype(m.group(1), structs))
  return argtypes


def parse_header(text):
  """The C header's text -> (signatures, structs, constants); ValueError on anything not understood."""
  text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
  signatures, structs, constants = {}, {}, {}
  for define in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(.*)$', text, flags=re.M):
    name, *value = define.split(None, 1)
    if value:   # (the include guard has none)
      if not name.isidentifier():
        raise ValueError(f'snap_hip.h: cannot read #define {define!r}')
      constants[name] = _int_expr(value[0])
  text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
  rest = []
  end = 0
  for m in _DECLARATION.finditer(text):
    rest.append(text[end:m.start()])
    end = m.end()
    if m.group('enumerators') is not None:
      for enumerator in filter(None, (e.strip() for e in m.group('enumerators').split(','))):
        name, _, value = enumerator.partition('=')
        constants[name.strip()] = _int_expr(value)
    elif m.group('struct'):
      structs[m.group('struct')] = _struct(m.group('struct'), m.group('members'), structs)
    else:
      name = m.group('function')
      signatures[name] = (_ctype(m.group('restype'), structs, returned=True), _argtypes(name, m.group('params'), structs))
  rest.append(text[end:])
  # everything between the declarations read above is the extern "C" bracket and nothing else: a
  # prototype the pattern did not take (a function-pointer parameter, say) is left over here
  left = re.sub(r'extern\s+"C"\s*\{|\}', '', ''.join(rest)).split()
  if left:
    raise ValueError(f'snap_hip.h: cannot read {" ".join(left)[:200]!r}')
  return signatures, structs, constants


with open(HEADER_PATH) as _f:
  SIGNATURES, _structs, _constants = parse_header(_f.read())
globals().update(_structs)     # SnapConvDesc, SnapConvExtras, SnapLiftDesc, SnapPackItem, ...
globals().update(_constants)   # SNAP_OK, SNAP_PRO_NONE, SNAP_TUNE_NO_PLAIN, ...
ABI_VERSION = _constants['SNAP_ABI_VERSION']

_lib = None


def load():
  """Load libsnap_hip.so and bind every declared symbol; raises if impossible."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise RuntimeError(
        f'{LIB_PATH} not found: the HIP extension is not built. '
        'Run `make -C snap_amd/csrc` (needs hipcc); there is no CPU fallback.'
    )
  lib = ctypes.CDLL(LIB_PATH)
  for name, (restype, argtypes) in SIGNATURES.items():
    fn = getattr(lib, name)  # AttributeError if the symbol is missing
    fn.restype = restype
    fn.argtypes = argtypes
  if lib.snap_abi_version() != ABI_VERSION:
    raise RuntimeError(
        f'libsnap_hip.so ABI {lib.snap_abi_version()} != expected {ABI_VERSION}; rebuild.'
    )
  _lib = lib
  return lib


def check(status, what):
  if status != 0:
    msg = load().snap_status_string(status).decode()
    raise RuntimeError(f'{what} failed: {msg} (status {status})')
