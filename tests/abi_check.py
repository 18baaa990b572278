"""Helper, not a test: the one place that compiles a host program against include/cfm.h.  It has the compiler say what the header declares --
every struct's size and each member's offset and size, every function's prototype -- and states the same of the ctypes binding in cfm/__init__.py,
so that tests/test_abi_cpu.py compares the two whole.  Nothing here loads the shared library."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "cfm.h")).read(), flags=re.S)


def declared_functions():
    return sorted(set(re.findall(r"\b(cfm_[a-z0-9_]+)\s*\(", _header())))


def declared_structs():
    return sorted(re.findall(r"typedef\s+struct\s*\{[^{}]*\}\s*(cfm_\w+)\s*;", _header()))


def mirrors(cfm):
    """{C name: ctypes.Structure subclass} over every one the cfm module holds; one without a `_c_name_` is an error."""
    found = [v for v in vars(cfm).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure]
    unnamed = [c.__name__ for c in found if not hasattr(c, "_c_name_")]
    assert not unnamed, "cfm: ctypes mirrors without a _c_name_: %s" % unnamed
    return {c._c_name_: c for c in found}


def _run(tmp_path, name, compiler, text):
    src = tmp_path / name
    src.write_text(text)
    exe = tmp_path / (name + ".exe")
    subprocess.run(compiler + ["-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()


def struct_mismatches(cfm, tmp_path):
    """(number of fields compared, ["cfm_x_desc.member: C size/offset a/b, ctypes c/d", ...]); a struct's own line compares sizeof.  A Python field the
    header lacks does not compile."""
    prints, want = [], {}
    for c_name, cls in sorted(mirrors(cfm).items()):
        prints.append('printf("%s %%zu 0\\n", sizeof(%s));' % (c_name, c_name))
        want[c_name] = (ctypes.sizeof(cls), 0)
        for field in (f[0] for f in cls._fields_):
            member = getattr(cls, "_c_fields_", {}).get(field, field)
            prints.append('printf("%s.%s %%zu %%zu\\n", sizeof(((%s*)0)->%s), offsetof(%s, %s));' % (c_name, field, c_name, member, c_name, member))
            want["%s.%s" % (c_name, field)] = (getattr(cls, field).size, getattr(cls, field).offset)
    out = _run(tmp_path, "structs.c", ["gcc", "-std=c99"], '#include <stdio.h>\n#include <stddef.h>\n#include "cfm.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(prints))
    got = {k: (int(size), int(off)) for k, size, off in (line.split() for line in out)}
    assert set(got) == set(want)
    return len(want) - len(mirrors(cfm)), ["%s: C size/offset %d/%d, ctypes %d/%d" % ((k,) + got[k] + want[k]) for k in want if got[k] != want[k]]


_TRAIT = """#include <cstdio>
#include <cstdint>
#include <string>
#include <type_traits>
#include "cfm.h"
template <class T> constexpr char code() {
    if (std::is_pointer_v<T>) return 'p';
    if (std::is_void_v<T>) return 'v';
    if (std::is_same_v<T, int32_t> || std::is_same_v<T, int>) return 'i';
    if (std::is_same_v<T, int64_t>) return 'q';
    if (std::is_same_v<T, uint32_t>) return 'I';
    if (std::is_same_v<T, float>) return 'f';
    if (std::is_same_v<T, double>) return 'd';
    return '?';
}
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> { static std::string str() { return std::string{code<R>(), ':'} + std::string{code<A>()...}; } };
int main() {
%s
    return 0;
}
"""
_CODES = {None: "v", ctypes.c_void_p: "p", ctypes.c_char_p: "p", ctypes.c_int32: "i", ctypes.c_int: "i", ctypes.c_int64: "q", ctypes.c_uint32: "I",
          ctypes.c_float: "f", ctypes.c_double: "d"}


def _code(t):
    if isinstance(t, type) and issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr)):
        return "p"
    return _CODES.get(t, "?")


def c_signatures(names, tmp_path):
    """{function: "r:aaa"} as the C++ compiler reads include/cfm.h: p pointer, v void, i int32, q int64, I uint32, f float, d double, ? anything else."""
    body = "\n".join('    std::printf("%s %%s\\n", sig<decltype(&%s)>::str().c_str());' % (n, n) for n in names)
    return dict(line.split() for line in _run(tmp_path, "protos.cpp", ["g++", "-std=c++17"], _TRAIT % body))


def table_signatures(cfm):
    """The same strings from cfm.PROTOTYPES."""
    return {name: "%s:%s" % (_code(restype), "".join(_code(a) for a in argtypes)) for name, restype, *argtypes in cfm.PROTOTYPES}
