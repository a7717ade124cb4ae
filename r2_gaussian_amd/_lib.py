"""ctypes binding of libr2hip.so, derived from the C ABI's one declaration, include/r2hip.h.

The header is parsed once, at import: every ``R2_API`` prototype becomes an entry of ``_SIGNATURES`` and every integer
``#define R2_*`` a module attribute (``parse_header``).  Adding an entry point means declaring it in the header; nothing here
changes.

The product path has NO fallback: if the HIP library is missing or fails to load, importing the ops
raises.  Build it with ``python -m r2_gaussian_amd.build`` (or ``__graft_entry__.build()``).
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# R2HIP_LIB selects an experiment build (profiling ablations); the default is the product library
LIB_PATH = os.environ.get("R2HIP_LIB") or os.path.join(_HERE, "libr2hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "r2hip.h")

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)


class R2HipError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong}
_RETURNS = dict(_SCALARS, **{"void": None, "const char *": C.c_char_p})
_PARAMS = dict(_SCALARS, r2_alloc_fn=ALLOC_FN)
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(R2_\w+)[ \t]+(?:(-?\d+)|\([ \t]*(-?\d+)[ \t]*\))[ \t]*$", re.M)
_PROTOTYPE = re.compile(r"R2_API\s+([\w\s*]+?)\b(r2_\w+)\s*\(([^()]*)\)\s*;")


def parse_header(text):
    """-> ({name: (restype, [argtypes])}, {R2_NAME: int}) of a header written like include/r2hip.h.

    Comments and preprocessor lines are dropped; what remains is matched as ``R2_API <ret> r2_name(<params>);``.  The types:

        parameter with ``*`` or an array declarator                      c_void_p
            (``long long out[3]``, ``const char *``, ``const float *const *``)
        int / float / double                                              c_int / c_float / c_double
        size_t / long long / unsigned long long                           c_size_t / c_longlong / c_ulonglong
        r2_alloc_fn                                                       ALLOC_FN
        return void / const char * / one of the scalar types              None / c_char_p / as above

    Anything else raises R2HipError naming the declaration: a type that is not listed (add it to the rule with the header),
    a parameter without a name, an ``R2_API`` the pattern does not consume.  Nothing is guessed.

    Every pointer is c_void_p because the header cannot tell a host pointer from a device pointer: the out-parameters of the
    stats, profile and offset calls are host pointers and take ``byref(...)``, a ctypes array, ``pointer(...)``, None or an
    address like any other.

    Constants: ``#define R2_<NAME> <integer>``, the integer decimal, possibly negative and parenthesised; other defines
    (``R2_API`` itself, non-integers) are not constants."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {m.group(1): int(m.group(2) or m.group(3)) for m in _DEFINE.finditer(text)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    signatures = {}
    for at in re.finditer(r"\bR2_API\b", text):
        m = _PROTOTYPE.match(text, at.start())
        if m is None:
            raise R2HipError("r2hip.h: cannot parse the declaration `%s ...`" % " ".join(text[at.start():at.start() + 120].split()))
        ret, name, params = " ".join(m.group(1).replace("*", " * ").split()), m.group(2), m.group(3).split(",")
        if ret not in _RETURNS:
            raise R2HipError("r2hip.h: return type `%s` of %s is not in the binding's type rule" % (ret, name))
        args = []
        for p in [] if m.group(3).strip() == "void" else params:
            if "*" in p or p.rstrip().endswith("]"):
                args.append(C.c_void_p)
                continue
            ctype = " ".join(p.split()[:-1])   # the last word is the parameter's name
            if ctype not in _PARAMS:
                raise R2HipError("r2hip.h: parameter `%s` of %s is not in the binding's type rule" % (" ".join(p.split()), name))
            args.append(_PARAMS[ctype])
        signatures[name] = (_RETURNS[ret], args)
    return signatures, constants


with open(HEADER_PATH, "r", encoding="utf-8") as _fh:
    _SIGNATURES, _CONSTANTS = parse_header(_fh.read())
globals().update(_CONSTANTS)   # R2_ABI_VERSION, R2_ERR_INVALID, ... under the header's names

_lib = None


def bind(path):
    """CDLL(path) with the header's restype / argtypes on every symbol and the ABI version checked: this build or another one."""
    L = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)   # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if L.r2_abi_version() != R2_ABI_VERSION:
        raise R2HipError("%s ABI %d != expected %d" % (os.path.basename(path), L.r2_abi_version(), R2_ABI_VERSION))
    return L


def lib():
    """Load libr2hip.so once; raise loudly when it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise R2HipError(
                "libr2hip.so not found at %s -- the HIP extension is required (no fallback). "
                "Run `python -m r2_gaussian_amd.build`." % LIB_PATH)
        _lib = bind(LIB_PATH)
    return _lib


def exported_symbols():
    return sorted(_SIGNATURES)


def check(rc, what):
    if rc < 0:
        msg = lib().r2_last_error()
        raise R2HipError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else ""))
    return rc


def stage_names():
    L = lib()
    return [L.r2_profile_stage_name(i).decode() for i in range(L.r2_profile_stage_count())]


def profile_enable(stages=None):
    """Enable HIP-event timing for the named stages (None = all, [] = off)."""
    names = stage_names()
    if stages is None:
        mask = (1 << len(names)) - 1
    else:
        mask = 0
        for s in stages:
            mask |= 1 << names.index(s)
    lib().r2_profile_enable(mask)


def path_stats(reset=False):
    """-> {name: count} of the chain counters (csrc/dispatch.hpp): which chain every forward took and why."""
    L = lib()
    n = L.r2_path_stat_count()
    buf = (C.c_longlong * n)()
    L.r2_path_stats(buf, n, int(reset))
    return {L.r2_path_stat_name(i).decode(): int(buf[i]) for i in range(n)}


def sync_wait_stats(reset=True):
    """-> (total microseconds the host busy-waited for num_rendered, number of waits)."""
    us, n = C.c_double(0.0), C.c_longlong(0)
    lib().r2_sync_wait_stats(C.byref(us), C.byref(n), int(reset))
    return us.value, n.value


def profile_host(reset=True):
    """-> (host microseconds per forward before its synchronisation wait, after it, number of forwards)."""
    a, b, n = C.c_double(0.0), C.c_double(0.0), C.c_longlong(0)
    lib().r2_profile_host(C.byref(a), C.byref(b), C.byref(n), int(reset))
    return a.value / max(n.value, 1), b.value / max(n.value, 1), n.value


def profile_read(reset=True):
    """-> {stage: (total_ms, launches)} for stages that ran."""
    L = lib()
    n = L.r2_profile_stage_count()
    ms = (C.c_double * n)()
    cnt = (C.c_longlong * n)()
    L.r2_profile_read(ms, cnt, int(reset))
    names = stage_names()
    return {names[i]: (ms[i], cnt[i]) for i in range(n) if cnt[i] > 0}
