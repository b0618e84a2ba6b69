"""include/t2vae.h read as the one table of the library's C ABI: prototypes, struct layouts and integer limits.

t2v_hip.py binds libt2vae_hip.so from what this module parses, so an entry point, a struct field or a limit is declared in
the header and nowhere else.  Pure Python (re, os, ctypes): no torch, no library, no GPU.  The parser never guesses: whatever
it cannot map raises T2VHipError naming the function, field or macro.
"""
import ctypes as C
import os
import re


class T2VHipError(RuntimeError):
    pass


# ../include/t2vae.h from the package, as csrc/Makefile reaches it (../../include/t2vae.h from csrc/)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 't2vae.h')

# C scalar type -> ctypes, by value (arguments, returns, struct fields): the whole table, the parser adds only the header's structs
SCALARS = {
    'int': C.c_int, 'int32_t': C.c_int,
    'long': C.c_long,
    'long long': C.c_longlong,
    'unsigned long long': C.c_ulonglong,
    'size_t': C.c_size_t,
    'uint32_t': C.c_uint32,
    'uint64_t': C.c_uint64,
    'int64_t': C.c_int64,
    'float': C.c_float,
    'double': C.c_double,
}
# types that only ever stand behind a `*`
POINTEES = ('void', 'char', 'int16_t')
# structs the HOST fills and passes by address -> the name of their ctypes.Structure: `T*` is POINTER(<that class>)
HOST_STRUCTS = {
    't2v_dec_weights': '_DecWeights', 't2v_dec_train_bufs': '_DecTrainBufs', 't2v_dec_bwd_bufs': '_DecBwdBufs',
    't2v_dec_persist_weights': '_DecPersistWeights', 't2v_dec_persist_bufs': '_DecPersistBufs',
    't2v_dec_train_persist_weights': '_DecTrainPersistWeights', 't2v_gemm_group': '_GemmGroup', 't2v_achain_dw': '_AchainDw',
    't2v_dec_infer_bufs': '_DecInferBufs', 't2v_dec_items': '_DecItems', 't2v_dec_window': '_DecWindow',
}
# records that live in DEVICE memory: their Structure gives the layout, `T*` is a plain device pointer (c_void_p or None)
DEVICE_STRUCTS = {'t2v_step_params': '_StepRecord'}

_DEFINE_VALUE = re.compile(r'^(-?(?:0[xX][0-9a-fA-F]+|\d+))(?:\s*<<\s*(\d+))?$')       # 2048, -3, 1 << 20
_TOKEN = re.compile(r'[A-Za-z_]\w*|\*|\[\d+\]|\S')
_TYPE_WORDS = set(w for t in SCALARS for w in t.split()) | set(POINTEES) | set(HOST_STRUCTS) | set(DEVICE_STRUCTS)


def _decl(text, who):
    """`const float* B[3]` -> (base type, stars, name or None, array length or None); `who` names the culprit in errors"""
    toks = _TOKEN.findall(text)
    i = 1 if toks[:1] == ['const'] else 0
    j = i
    while j < len(toks) and toks[j] in _TYPE_WORDS:
        j += 1
    base = ' '.join(toks[i:j])
    if j < len(toks) and toks[j] == 'const':
        j += 1
    stars = 0
    while j < len(toks) and toks[j] == '*':
        stars += 1
        j += 2 if toks[j + 1:j + 2] == ['const'] else 1
    name = length = None
    if j < len(toks) and re.match(r'[A-Za-z_]\w*$', toks[j]):
        name, j = toks[j], j + 1
    if j < len(toks) and re.match(r'\[\d+\]$', toks[j]):
        length, j = int(toks[j][1:-1]), j + 1
    if not base:
        raise T2VHipError("%s: unknown type in `%s`" % (who, text.strip()))
    if j != len(toks):
        raise T2VHipError("%s: cannot split the declaration `%s`" % (who, text.strip()))
    if base not in SCALARS and base not in POINTEES and base not in HOST_STRUCTS and base not in DEVICE_STRUCTS:
        raise T2VHipError("%s: unknown type `%s` in `%s`" % (who, base, text.strip()))
    return base, stars, name, length


class Abi(object):
    """prototypes: {name: (restype, [argtypes])} in header order; layouts: {struct: [(field, ctype)]};
    classes: {struct: its ctypes.Structure, C_NAME = the struct's name}; defines: {macro: int} of the integer macros"""

    def __init__(self, text, where='include/t2vae.h'):
        text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
        text = re.sub(r'//[^\n]*', ' ', text)
        self._macros = dict((m.group(1), m.group(2).strip())
                            for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$', text, flags=re.M))
        self.defines = {}
        for name, value in self._macros.items():
            if value.startswith('(') and value.endswith(')'):
                value = value[1:-1].strip()
            m = _DEFINE_VALUE.match(value)
            if m:
                self.defines[name] = int(m.group(1), 0) << int(m.group(2) or 0)
        text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
        text, wrapped = re.subn(r'extern\s+"C"\s*\{', ' ', text)
        if wrapped:
            text, brace, tail = text.rpartition('}')
            if not brace or tail.strip():
                raise T2VHipError('%s: the extern "C" wrapper is not closed at the end' % where)
        declared = re.findall(r'\b(t2v_\w+)\s*\(', text)
        # the structs first (a prototype may name one that is defined further down), then every other `...;` is a prototype
        self.layouts, self.classes, self.prototypes = {}, {}, {}
        text = re.sub(r'typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;', self._struct, text)
        for d in text.split(';'):
            if d.strip():
                self._prototype(' '.join(d.split()))
        if declared != list(self.prototypes):
            raise T2VHipError("%s: not parsed as prototypes: %s" % (where, ', '.join(n for n in declared if n not in self.prototypes)))

    def _struct(self, m):
        name, fields = m.group(1), []
        if m.group(3) != name:
            raise T2VHipError("struct %s is typedef'd as %s" % (name, m.group(3)))
        if name not in HOST_STRUCTS and name not in DEVICE_STRUCTS:
            raise T2VHipError("struct %s is named in neither HOST_STRUCTS nor DEVICE_STRUCTS of t2v_abi.py" % name)
        for d in m.group(2).split(';'):
            if not d.strip():
                continue
            who = '%s.%s' % (name, d.split()[-1])
            base, stars, field, length = _decl(d, who)
            if field is None:
                raise T2VHipError("%s: cannot split the declaration `%s`" % (who, d.strip()))
            if not stars and base not in SCALARS:
                raise T2VHipError("%s: unknown type `%s` by value" % (who, base))
            ctype = C.c_void_p if stars else SCALARS[base]
            fields.append((field, ctype * length if length else ctype))
        self.layouts[name] = fields
        self.classes[name] = type(HOST_STRUCTS.get(name) or DEVICE_STRUCTS[name], (C.Structure,), {'C_NAME': name, '_fields_': list(fields)})
        return ' '

    def _prototype(self, d):
        m = re.match(r'^([\w\s\*]+?)\s*\b(\w+)\s*\(([^()]*)\)$', d)
        if not m:
            raise T2VHipError("cannot split the declaration `%s`" % d[:120])
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if name in self.prototypes:
            raise T2VHipError("%s is declared twice" % name)
        base, stars, extra, length = _decl(ret, name)
        if extra is not None or length is not None:
            raise T2VHipError("%s: cannot split the declaration `%s`" % (name, d[:120]))
        if (base, stars) == ('void', 0):
            restype = None
        elif (base, stars) == ('char', 1):
            restype = C.c_char_p
        elif not stars and base in SCALARS:
            restype = SCALARS[base]
        else:
            raise T2VHipError("%s: unknown return type `%s`" % (name, ret))
        self.prototypes[name] = (restype, [] if params in ('', 'void') else [self._argtype(p, name) for p in params.split(',')])

    def _argtype(self, text, fn):
        who = '%s(%s)' % (fn, text.strip())
        base, stars, name, length = _decl(text, who)
        if length is not None:
            raise T2VHipError("%s: an array parameter" % who)
        if not stars:
            if base not in SCALARS:
                raise T2VHipError("%s: unknown type `%s` by value" % (who, base))
            return SCALARS[base]
        if stars == 1 and base in HOST_STRUCTS:
            if base not in self.classes:
                raise T2VHipError("%s: struct %s is not defined in the header" % (who, base))
            return C.POINTER(self.classes[base])
        if stars == 2 and base == 'void':           # const void* const*, void* const*: a host array of device addresses
            return C.POINTER(C.c_void_p)
        if stars > 2 or (stars == 2 and base not in SCALARS):
            raise T2VHipError("%s: unknown pointer type" % who)
        return C.c_void_p       # device memory, t2v_step_params included; a host array such as `const float* const*` or `const int*` too

    def define(self, name):
        """the integer value of `#define name ...`"""
        if name not in self.defines:
            raise T2VHipError("%s: %s" % (name, "`%s` is not an integer expression" % self._macros[name]
                                          if name in self._macros else "not #defined in the header"))
        return self.defines[name]


_ABI = {}


def load(path=HEADER):
    """the parsed header (once per process and path)"""
    if path not in _ABI:
        try:
            with open(path) as f:
                text = f.read()
        except OSError as e:
            raise T2VHipError("C header %s not readable (%s): the binding is derived from it" % (path, e.strerror))
        try:
            _ABI[path] = Abi(text, path)
        except T2VHipError as e:
            raise T2VHipError("%s: %s" % (path, e))
    return _ABI[path]
