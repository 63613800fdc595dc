"""ctypes binding of ``libbrever_hip.so``, derived from its C header.

``include/brever_hip.h`` is the single declaration of the C ABI. At import ``SIGNATURES`` is parsed from its prototypes
(``parse_header``), ``CtnConfig`` / ``LaunchOpts`` / ``DccrnStreamConfig`` are generated from its structs
(``parse_structs``) and ``OPT_*`` / ``DCCRN_STREAM_MAX_LEVELS`` read from its ``#define``s (``parse_constants``), so an
entry point, a field or a limit is added or changed there and nowhere else. ``call`` / ``query`` invoke an entry point
by name and raise with the library's own message; pointer arguments take tensors directly. ``Library`` is that binding
for any library of ``csrc/``: this module and every module with a library of its own use it once.

The HIP library is the product; there is no CPU or PyTorch fallback. Every
helper here raises ``RuntimeError`` when the shared library is missing or when
it is handed a tensor that is not on a ROCm device.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))


class _c_ptr(ctypes.c_void_p):
    """Pointer argument: a tensor passes its ``data_ptr()``; None, ints, ``bytes``, ctypes buffers and ``byref``
    go through as for ``c_void_p``. No device check here -- the header does not say which pointers are host
    pointers (``require_device``)."""

    @staticmethod           # (called once per pointer argument of every call: the lookups are bound here)
    def from_param(obj, _tensor=torch.Tensor, _void_p=ctypes.c_void_p, _other=ctypes.c_void_p.from_param):
        if isinstance(obj, _tensor):
            return _void_p(obj.data_ptr())
        return _other(obj)


_SCALARS = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'int': ctypes.c_int,
            'uint32_t': ctypes.c_uint32, 'float': ctypes.c_float}


def _ctype(decl, proto, ret=False):
    """ctypes type of one declaration of the header (``const float* x``, ``int64_t n``, a result type). The map
    is closed: anything else raises, naming the prototype."""
    m = re.fullmatch(r'\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w*)\s*', decl)
    base, star, name = m.groups() if m else ('', '', '')
    if star:
        t = ctypes.c_char_p if base == 'char' else ctypes.c_void_p if ret else _c_ptr
        known = not ret or base in ('char', 'void')
    else:
        t = None if base == 'void' else _c_ptr if base == 'brv_stream_t' else _SCALARS.get(base)
        known = base in _SCALARS or base == ('void' if ret else 'brv_stream_t')
    if not known or (ret and name):
        raise RuntimeError(f'{proto}: no ctypes type for {decl.strip()!r}')
    return t


def parse_header(text):
    """``{name: (restype, argtypes)}`` of every ``ret brv_name(args);`` of a C header."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^[ \t]*#(?:.*\\\n)*.*$', ' ', text, flags=re.M)
    table = {}
    for ret, name, args in re.findall(r'([^;{}()]*)\b(brv_\w+)\s*\(([^;{}]*);', text):
        args = args.rstrip()
        if not args.endswith(')') or '(' in args or ')' in args[:-1]:
            raise RuntimeError(f'{name}: cannot split the argument list ({args!r}')
        args = args[:-1].strip()
        argtypes = [] if args in ('', 'void') else [_ctype(a, name) for a in args.split(',')]
        table[name] = (_ctype(ret, name, ret=True), argtypes)
    for name in re.findall(r'\b(brv_\w+)\s*\(', text):
        if name not in table:
            raise RuntimeError(f'{name}: not a prototype the parser can read')
    return table


def parse_constants(text):
    """``{name: int}`` of every ``#define BRV_NAME <integer literal>`` of a C header: decimal or hex, an optional
    ``u`` / ``l`` suffix, optionally in parentheses and negative. A macro with parameters or without a value (an
    include guard) is no constant; any other value of a ``BRV_`` macro raises, naming the macro."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S).replace('\\\n', ' ')
    table = {}
    for name, params, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(BRV_\w+)(\(?)(.*)$', text, flags=re.M):
        value = value.strip()
        if params or not value:
            continue
        inner = value[1:-1].strip() if value[0] == '(' and value[-1] == ')' else value
        m = re.fullmatch(r'(-?)\s*(0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)[uUlL]*', inner)
        if not m:
            raise RuntimeError(f'{name}: {value!r} is not an integer literal the parser can read')
        table[name] = int(m.group(1) + m.group(2), 0)
    return table


def _extent(text, constants):
    """Value of one array extent of a struct field: an integer, ``NAME``, ``k*NAME`` or ``NAME + k`` with ``NAME`` in
    ``constants``; None for anything else."""
    m = re.fullmatch(r'\s*(?:(\d+)|(\d+)\s*\*\s*([A-Za-z_]\w*)|([A-Za-z_]\w*)(?:\s*\+\s*(\d+))?)\s*', text)
    n, k, scaled, plain, more = m.groups() if m else (None,)*5
    if n:
        return int(n)
    if scaled in constants:
        return int(k)*constants[scaled]
    return constants[plain] + int(more or 0) if plain in constants else None


def parse_structs(text, constants):
    """``{name: ctypes.Structure subclass}`` of every ``typedef struct brv_x { ... } brv_x;`` of a C header. A field is
    an ``int32_t``, ``uint32_t``, ``int64_t``, ``float`` or a pointer (``c_void_p``), alone or an array of one to three
    extents (``_extent``). The grammar is closed: anything else raises, naming the struct and the field."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#(?:.*\\\n)*.*$', ' ', text, flags=re.M)
    table = {}
    for tag, body, name in re.findall(r'\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w*)\s*;', text, flags=re.S):
        *decls, rest = body.split(';')
        if name != tag or not tag.startswith('brv_') or '{' in body or rest.strip() or not decls:
            raise RuntimeError(f'struct {tag}: not a `typedef struct brv_x {{ fields; }} brv_x;`')
        fields = []
        for decl in decls:
            m = re.fullmatch(r'\s*(?:const\s+)?(\w+)\b(.*)', decl, flags=re.S)
            base, declarators = m.groups() if m else ('', decl)
            for d in declarators.split(','):
                m = re.fullmatch(r'\s*(\*?)\s*([A-Za-z_]\w*)\s*((?:\[[^\[\]]*\]\s*){0,3})', d)
                star, field, dims = m.groups() if m else ('', d.strip() or decl.strip(), '')
                t = ctypes.c_void_p if star else _SCALARS.get(base) if base != 'int' else None
                if not m or t is None:
                    raise RuntimeError(f'{tag}.{field}: no ctypes type for {decl.strip()!r}')
                for dim in reversed(re.findall(r'\[([^\[\]]*)\]', dims)):
                    n = _extent(dim, constants)
                    if n is None:
                        raise RuntimeError(f'{tag}.{field}: cannot read the array extent [{dim}]')
                    t = t*n
                fields.append((field, t))
        table[tag] = type(tag, (ctypes.Structure,), {'_fields_': fields, '__doc__': f'``{tag}`` of the C header.'})
    for tag in re.findall(r'\bstruct\s+(\w*)', text):
        if tag not in table:
            raise RuntimeError(f'struct {tag}: not a struct definition the parser can read')
    return table


def _header_text(path):
    if not os.path.exists(path):
        raise RuntimeError(f'{path} is missing: the binding is derived from the C header')
    with open(path) as f:
        return f.read()


class Library:
    """The binding of one shared library of ``csrc/``: ``include/<header>`` is the single declaration of its C ABI and
    ``csrc/<soname>`` (or the build that the environment variable ``env`` names, read here) is loaded at the first
    use. ``what`` ends the message of a library that is not built: there is no fallback. A module binds its library
    once and takes ``lib``, ``call``, ``query``, ``last_error`` from it as plain functions and the header's tables."""

    def __init__(self, header, soname, env, what, last_error=None):
        self.header_path = os.path.join(os.path.dirname(_HERE), 'include', header)
        self.path = os.environ.get(env) or os.path.join(_HERE, 'csrc', soname)
        # read from the header once: name -> (restype, argtypes), BRV_NAME -> int, struct name -> Structure subclass
        text = _header_text(self.header_path)
        self.signatures, self.constants = parse_header(text), parse_constants(text)
        self.structs = parse_structs(text, self.constants)
        if last_error is None:
            last_error, = (name for name in self.signatures if name.endswith('_last_error'))
        handle = None         # (a cell of the closures below: a call on the loaded library looks nothing else up)

        def lib():
            """Load the shared library once; fail loudly if it is not built."""
            nonlocal handle
            if handle is None:
                if not os.path.exists(self.path):
                    raise RuntimeError(
                        f'{self.path} is missing: build it with '
                        '`python -c "import __graft_entry__ as g; g.build()"` or '
                        f'`make -C brever_amd/csrc` (needs hipcc, targets gfx950). {what}')
                loaded = ctypes.CDLL(self.path)
                for name, (restype, argtypes) in self.signatures.items():
                    fn = getattr(loaded, name)
                    fn.restype, fn.argtypes = restype, argtypes
                handle = loaded
            return handle

        def message():
            """The library's message of this thread's last failing call."""
            msg = getattr(lib(), last_error)()
            return msg.decode() if msg else ''

        def check(status, what):
            if status != 0:
                raise RuntimeError(f'{what} failed with status {status}: {message()}')

        def call(name, *args):
            """Call the entry point ``name``, which returns an int status; anything but 0 raises with the library's
            message."""
            status = getattr(handle or lib(), name)(*args)
            if status:
                check(status, name)

        def query(name, *args):
            """Value of the int64_t size / count query ``name``; a negative one raises like ``call``."""
            n = getattr(handle or lib(), name)(*args)
            if n < 0:
                check(int(n), name)
            return n

        self.lib, self.last_error, self.check, self.call, self.query = lib, message, check, call, query


# BRV_LIB_PATH: load another build of the same library (tools/: diagnostic builds). The header sits next to the
# package (there is no install layout); diagnostic builds share it.
_LIB = Library('brever_hip.h', 'libbrever_hip.so', 'BRV_LIB_PATH',
               'brever_amd has no CPU/PyTorch fallback for its kernels.')
LIB_PATH, HEADER_PATH, SIGNATURES = _LIB.path, _LIB.header_path, _LIB.signatures
lib, last_error, check, call, query = _LIB.lib, _LIB.last_error, _LIB.check, _LIB.call, _LIB.query
# the header's structs, and its constants: every BRV_OPT_<flag> as OPT_<flag>
CtnConfig, LaunchOpts = _LIB.structs['brv_ctn_config'], _LIB.structs['brv_launch_opts']
DccrnStreamConfig = _LIB.structs['brv_dccrn_stream_config']
DCCRN_STREAM_MAX_LEVELS = _LIB.constants['BRV_DCCRN_STREAM_MAX_LEVELS']
globals().update((name[4:], value) for name, value in _LIB.constants.items() if name.startswith('BRV_OPT_'))

# environment switch -> option flag (read by the HOST at call time; the library itself reads no
# environment). '0' selects the flag for the *_FUSE switches, any value for the BRV_NO_* ones.
_ENV_FLAGS = (('BRV_FWD_FUSE', OPT_NO_FWD_FUSE, '0'), ('BRV_BWD_FUSE', OPT_NO_BWD_FUSE, '0'),
              ('BRV_NO_WS', OPT_NO_WS, None), ('BRV_DWPW2_WS', OPT_DWPW2_WS, '1'),
              ('BRV_NO_DZ_FUSE', OPT_NO_DZ_FUSE, None), ('BRV_NO_DZ1_FUSE', OPT_NO_DZ1_FUSE, None),
              ('BRV_NO_WGRAD_FULL', OPT_NO_WGRAD_FULL, None), ('BRV_NO_WGRAD_SPLIT', OPT_NO_WGRAD_SPLIT, None),
              ('BRV_PW1_RC', OPT_NO_PW1_RC, '0'), ('BRV_PW1_RC_WGRAD', OPT_PW1_RC_WGRAD, '1'),
              ('BRV_PW1_RC_TILES', OPT_PW1_RC_TILES, '1'), ('BRV_WGRAD_128', OPT_NO_WGRAD_128, '0'))
# switches of the two kernel variants that were measured slower and removed: refused, so
# that an A/B run given a stale switch does not compare the default with itself
_RETIRED_SWITCHES = ('BRV_DWPW2_V2', 'BRV_BWD_PERSIST')
_prof = None            # profiler handle of this process's calls (prof_enable)


def launch_opts(cu_eighths=8):
    """Options for one Conv-TasNet call: A/B switches from the environment, the share of
    the chip the persistent kernels take, the active profiler. Returns the struct (keep it alive for
    the duration of the call) -- pass ``ctypes.byref`` of it."""
    for name in _RETIRED_SWITCHES:
        if os.environ.get(name) == '1':
            raise RuntimeError(f'{name}=1: this kernel variant was retired (DESIGN.md 5m / 5n); unset the switch')
    flags = 0
    for name, flag, on_value in _ENV_FLAGS:
        v = os.environ.get(name)
        if v is not None and (on_value is None or v == on_value):
            flags |= flag
    target = os.environ.get('BRV_WG_TARGET')
    return LaunchOpts(ctypes.sizeof(LaunchOpts), flags, int(cu_eighths),
                      int(target) if target else 0, _prof)


def opts_ptr(opts):
    return ctypes.byref(opts)


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                'brever_amd kernels run on a ROCm device only; got a '
                f'{t.device} tensor (there is no CPU fallback)'
            )


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def gemm_f32(a, b, d, batch, M, N, K, lda, ldb, ldd, a_bs, b_bs, d_bs, trans_a, trans_b, kbatch, a_kbs, b_kbs,
             bias, mode):
    """``brv_gemm_f32``; a product whose output has too few tiles to fill the chip (weight gradients summed over the
    batch, convolutions at the low resolutions) goes through ``brv_gemm_f32_ws`` with scratch from the caching
    allocator: ordered reduction split, split-bf16 form where the layout allows (csrc/gemm_f32_big.hip)."""
    if M >= 32 and N >= 32:
        nbytes = lib().brv_gemm_f32_workspace_bytes(batch, M, N, K, trans_a, trans_b, kbatch)
        if nbytes > 0:
            ws = torch.empty(nbytes//4, dtype=torch.float32, device=d.device)
            call('brv_gemm_f32_ws', a, b, d, batch, M, N, K, lda, ldb, ldd, a_bs, b_bs, d_bs, trans_a, trans_b,
                 kbatch, a_kbs, b_kbs, bias, mode, ws, nbytes, stream())
            return
    call('brv_gemm_f32', a, b, d, batch, M, N, K, lda, ldb, ldd, a_bs, b_bs, d_bs, trans_a, trans_b,
         kbatch, a_kbs, b_kbs, bias, mode, stream())


def prof_enable(mode):
    """0: off; 1: event-time every launch of the Conv-TasNet calls made through ``launch_opts``;
    2: the same with the depthwise backward kernels labelled per dilation."""
    global _prof
    if _prof is not None:
        lib().brv_prof_destroy(_prof)
        _prof = None
    if mode:
        _prof = ctypes.c_void_p(lib().brv_prof_create(1 if mode == 2 else 0))


def profile_collect():
    """Per-label aggregate of the event-timed launches since ``prof_enable`` / the last collect:
    ``{label: dict(calls, ms, flops, bytes)}``."""
    if _prof is None:
        return {}
    n = lib().brv_prof_collect(_prof, None, 0)
    buf = ctypes.create_string_buffer(int(n) + 16)
    lib().brv_prof_collect(_prof, buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        label, calls, ms, flops, nbytes = line.split()
        out[label] = dict(calls=int(calls), ms=float(ms), flops=float(flops),
                          bytes=float(nbytes))
    return out
