"""ctypes binding of libxview_hip.so (the C ABI declared in include/xview_hip.h).

The library is the product's only compute path: if it is missing or a call fails this module
raises -- there is no CPU or PyTorch fallback.
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libxview_hip.so')
CSRC = os.path.join(_HERE, 'csrc')
HEADER = os.path.join(os.path.dirname(_HERE), 'include', 'xview_hip.h')


class XvError(RuntimeError):
    pass


class xv_act(ctypes.Structure):
    _fields_ = [('data', ctypes.c_void_p), ('n', ctypes.c_int32), ('h', ctypes.c_int32),
                ('w', ctypes.c_int32), ('c', ctypes.c_int32), ('dtype', ctypes.c_int32),
                ('scale_exp', ctypes.c_int32)]


class xv_pack_desc(ctypes.Structure):
    _fields_ = [('w_hwio', ctypes.c_void_p), ('packed', ctypes.c_void_p), ('packed_dgrad', ctypes.c_void_p),
                ('k', ctypes.c_int32), ('cin', ctypes.c_int32), ('cout', ctypes.c_int32), ('reserved', ctypes.c_int32)]


_SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'size_t': ctypes.c_size_t,
            'float': ctypes.c_float}


def _ctype(ctext, decl, restype=False):
    """The ctypes type of one C parameter or return type, by a closed map; anything else is an error, never a guess."""
    words = re.findall(r'\w+|\*', ctext)
    base = ' '.join(w for w in words if w not in ('const', '*'))
    stars = words.count('*')
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and re.fullmatch(r'\w+', base):
        if base == 'xv_act':
            return ctypes.POINTER(xv_act)
        return ctypes.c_char_p if restype and base == 'char' else ctypes.c_void_p
    if stars == 2 and re.fullmatch(r'\w+', base):
        return ctypes.POINTER(ctypes.c_void_p)              # a host array of device pointers
    raise XvError('include/xview_hip.h: no ctypes mapping for %r in `%s`' % (ctext.strip(), decl))


def parse_header(text):
    """(functions, constants, structs) of the C header: name -> (restype, [argtypes]) for every declaration, name -> int for
    every integer `#define XV_*`, name -> [(field, C type)] for every `typedef struct`.  Plain text processing: no
    preprocessor, no compiler."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    constants = {m.group(1): int(m.group(2))
                 for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(XV_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$', text, re.M)}
    structs = {}
    struct = re.compile(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;', re.S)
    for name, body in struct.findall(text):
        fields = structs[name] = []
        for member in filter(None, (' '.join(f.split()) for f in body.split(';'))):
            m = re.fullmatch(r'(.*?[\s*])(\w+(?:\s*,\s*\w+)*)', member)        # type, then one or more names
            if not m:
                raise XvError('include/xview_hip.h: cannot parse member `%s` of %s' % (member, name))
            fields += [(field.strip(), m.group(1).replace(' *', '*').strip()) for field in m.group(2).split(',')]
    text = struct.sub(' ', text)
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)                  # include guards, includes, defines
    text = re.sub(r'extern\s+"C"\s*\{|^\s*\}\s*$', ' ', text, flags=re.M)
    functions = {}
    for decl in filter(None, (' '.join(d.split()) for d in text.split(';'))):
        m = re.fullmatch(r'([\w\s*]+?)\s*\b(\w+)\s*\(([^()]*)\)', decl)
        if not m or m.group(2) in functions:
            raise XvError('include/xview_hip.h: not a function declaration, or declared twice: `%s`' % decl)
        params = [] if m.group(3).strip() == 'void' else m.group(3).split(',')
        args = []
        for p in params:
            pm = re.fullmatch(r'\s*(.*?[\s*])(\w+)\s*', p)               # type, then the parameter's name
            if not pm:
                raise XvError('include/xview_hip.h: cannot parse parameter `%s` of `%s`' % (p.strip(), decl))
            args.append(_ctype(pm.group(1), decl))
        functions[m.group(2)] = (_ctype(m.group(1), decl, restype=True), args)
    return functions, constants, structs


def _read_header():
    if not os.path.exists(HEADER):
        raise XvError('%s not found: the ctypes table is derived from it' % HEADER)
    with open(HEADER) as f:
        return f.read()


# name -> (restype, argtypes) of every symbol include/xview_hip.h declares; its XV_* integers; its structs' members
SIGNATURES, CONSTANTS, STRUCTS = parse_header(_read_header())

_lib = None


def source_hash():
    """sha256 (first 16 hex digits) over the library's sources, as csrc/Makefile computes SRC_HASH."""
    import hashlib
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()
    h = hashlib.sha256()
    hdrs = re.search(r'^HDRS := (.*)$', mk, re.M).group(1).split()
    for rel in srcs + hdrs + ['Makefile']:
        with open(os.path.join(CSRC, rel), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def build(force=False):
    """Compile csrc/*.hip for gfx950 into libxview_hip.so (hipcc cross-compiles without a GPU).
    force=True (or XV_FORCE_REBUILD=1) recompiles every object from scratch; otherwise `make` rebuilds what
    changed.  Either way the result must carry the hash of the sources it sits next to."""
    if force or os.environ.get('XV_FORCE_REBUILD') == '1':
        subprocess.run(['make', '-C', CSRC, 'clean'], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(['make', '-C', CSRC, '-j4'], check=True, stdout=subprocess.DEVNULL)
    if not os.path.exists(LIB_PATH):
        raise XvError('build did not produce ' + LIB_PATH)
    global _lib
    _lib = None
    got = lib().xv_source_hash().decode()
    if got != source_hash():
        raise XvError('built library is stamped %s but the sources hash to %s' % (got, source_hash()))
    return LIB_PATH


def lib():
    """Load (once) and return the ctypes handle; raises XvError if the library is absent or was built from
    other sources than the ones next to it (when those are present: they always are in this repository)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise XvError('%s not found: run `python -c "import __graft_entry__ as g; g.build()"` '
                          '(hipcc --offload-arch=gfx950); there is no fallback path' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        if os.path.exists(os.path.join(CSRC, 'Makefile')) and os.environ.get('XV_ALLOW_STALE_LIB') != '1':
            got = handle.xv_source_hash().decode()
            if got != source_hash():
                raise XvError('%s was built from other sources (stamp %s, sources %s): rebuild with '
                              '`python -c "import __graft_entry__ as g; g.build()"`' % (LIB_PATH, got, source_hash()))
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        names = {v: k for k, v in CONSTANTS.items() if k.startswith('XV_E')}
        kind = names.get(code, 'hipError_t %d' % code)
        raise XvError('%s failed: %s' % (what, kind))
