"""CPU tests of the ctypes binding's types: lib.bind() takes them from the signature table inside the library (csrc/abi.hip, derived by the compiler from
include/mafyolo_hip.h).  Witnesses: what the hand-written binding of the parent commit declared, the header read by a regex, the step tape's own table."""
import ctypes
import json
import os
import re

import pytest

from maf_yolo_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_FNS = {"maf_abi_count", "maf_abi_name", "maf_abi_signature"}
NO_ARGTYPES_BEFORE = {"maf_last_error", "maf_version", "maf_op_size", "maf_tape_rec_size", "maf_augment_sample_size", "maf_augment_paste_size"}


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return lib.load()


def _type_named(name):
    """The ctypes object behind a type name of the fixture ("c_int", "None", "LP_MafOp": POINTER(lib.MafOp))."""
    if name == "None":
        return None
    if name.startswith("LP_"):
        return ctypes.POINTER(_type_named(name[3:]))
    return getattr(lib, name) if hasattr(lib, name) else getattr(ctypes, name)


def test_binding_is_the_parent_commits(built):
    """tests/golden/abi_parent.json is what lib.load() of commit 93c594a (the last one with hand-written argtypes) set on each of its 113 functions: restype,
    argtypes and the slots typed with a POINTER(...), by type name — recorded by running THAT load() against a stub in place of ctypes.CDLL whose
    functions start with restype = c_int (the ctypes default) and no argtypes (null in the file).  The table-driven binding must give every function the
    same objects; the one allowed difference is [] for the six (void) functions that had no argtypes."""
    with open(os.path.join(ROOT, "tests", "golden", "abi_parent.json")) as f:
        parent = json.load(f)
    assert len(parent) == 113 and set(parent) | TABLE_FNS == set(lib.EXPORTS)
    assert {n for n, p in parent.items() if p["argtypes"] is None} == NO_ARGTYPES_BEFORE
    for name, p in parent.items():
        fn = getattr(built, name)
        assert fn.restype is _type_named(p["restype"]), name
        want = [_type_named(t) for t in p["argtypes"] or []]
        assert len(fn.argtypes) == len(want) and all(a is b for a, b in zip(fn.argtypes, want)), (name, fn.argtypes, p["argtypes"])
        typed = {str(i): t.__name__ for i, t in enumerate(fn.argtypes) if isinstance(t, type(ctypes.POINTER(ctypes.c_int)))}
        assert typed == p["typed"], name


_SCALARS = {"void": "v", "float": "f", "double": "d", "int": "i", "int32_t": "i", "int64_t": "l", "maf_stream_t": "p"}


def _kind(ctype):
    t = " ".join(ctype.replace("*", " * ").split())
    if "*" in t:
        return "s" if t == "const char *" else "p"
    return _SCALARS[t[len("const "):] if t.startswith("const ") else t]        # KeyError: a type the ABI does not pass


def header_signatures():
    """{function: signature string} read from the header's text alone: comments and preprocessor lines stripped, every prototype matched by a regex."""
    text = open(os.path.join(ROOT, "include", "mafyolo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
    sigs = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(maf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() == "void" else [re.sub(r"\s*\b\w+$", "", p.strip()) for p in params.split(",")]
        assert name not in sigs, name
        sigs[name] = _kind(ret) + ":" + "".join(_kind(p) for p in params)
    return sigs


def test_library_table_equals_header(built):
    """A second, independent reading of the header: the strings the compiler derived must be the ones a regex over the prototypes gives, for every function."""
    want = header_signatures()
    assert len(want) == 116 and set(want) == set(lib.EXPORTS)
    assert want["maf_nms_ex"] == "i:piiiddpiiiiplpppip" and want["maf_last_error"] == "s:" and want["maf_timer_destroy"] == "v:p" and want["maf_tape_fn_id"] == "i:s"
    got = {built.maf_abi_name(i).decode(): built.maf_abi_signature(i).decode() for i in range(built.maf_abi_count())}
    assert built.maf_abi_count() == 116 and got == want
    assert built.maf_abi_name(-1) is None and built.maf_abi_signature(built.maf_abi_count()) is None


class _Fn:
    def __init__(self, call=None):
        self.call, self.restype, self.argtypes = call, ctypes.c_int, None

    def __call__(self, *a):
        return self.call(*a)


class _StubLibrary:
    """Stands in for ctypes.CDLL: serves `table` ({name: signature}) through the three table functions, or has none of them (table = None: an old build)."""

    def __init__(self, table):
        if table is not None:
            rows = list(table.items())
            self.maf_abi_count = _Fn(lambda: len(rows))
            self.maf_abi_name = _Fn(lambda i: rows[i][0].encode())
            self.maf_abi_signature = _Fn(lambda i: rows[i][1].encode())

    def __getattr__(self, name):            # reached only for what __init__ did not set
        if not name.startswith("maf_") or name in TABLE_FNS:
            raise AttributeError(name)
        setattr(self, name, _Fn())
        return getattr(self, name)


def test_bind_refuses_what_does_not_fit(monkeypatch):
    table = header_signatures()
    L = _StubLibrary(table)
    lib.bind(L)                             # the whole table as it is: accepted, and the stub's functions carry the types
    assert L.maf_nms_workspace_bytes.restype is ctypes.c_int64 and L.maf_nms_workspace_bytes.argtypes == [ctypes.c_int32] * 3
    assert L.maf_op_launch.argtypes == [ctypes.POINTER(lib.MafOp), ctypes.c_void_p] and L.maf_version.argtypes == [] and L.maf_timer_destroy.restype is None
    with pytest.raises(lib.MafError, match=r"\bmaf_pack_dw\b"):             # the library lacks a function of EXPORTS
        lib.bind(_StubLibrary({n: s for n, s in table.items() if n != "maf_pack_dw"}))
    with pytest.raises(lib.MafError, match=r"\bmaf_not_in_exports\b"):      # the library has one more
        lib.bind(_StubLibrary(dict(table, maf_not_in_exports="i:p")))
    with monkeypatch.context() as m:                                        # the same from the other side: EXPORTS lost a name the library has
        m.setattr(lib, "EXPORTS", [n for n in lib.EXPORTS if n != "maf_zero"])
        with pytest.raises(lib.MafError, match=r"\bmaf_zero\b"):
            lib.bind(_StubLibrary(table))
    for slot in (1, 17, 18):                                                # maf_nms_ex "i:piiiddpiiiiplpppip": an int32, the stream (a pointer: fine), past the end
        with monkeypatch.context() as m:
            m.setitem(lib.TYPED_POINTERS, "maf_nms_ex", {slot: ctypes.POINTER(ctypes.c_int32)})
            if slot == 17:
                lib.bind(_StubLibrary(table))
            else:
                with pytest.raises(lib.MafError, match=r"argument %d of maf_nms_ex\b" % slot):
                    lib.bind(_StubLibrary(table))
    with monkeypatch.context() as m:                                        # a refinement for a function the library does not have
        m.setitem(lib.TYPED_POINTERS, "maf_gone", {0: ctypes.c_void_p})
        with pytest.raises(lib.MafError, match=r"\bmaf_gone\b"):
            lib.bind(_StubLibrary(table))
    with pytest.raises(lib.MafError, match=r"maf_abi_count.*rebuild"):      # built before the table existed
        lib.bind(_StubLibrary(None))


def test_tape_table_agrees(built):
    """The step tape's own compiler-derived table (csrc/tape.hip) counts the same arguments for every tape-able entry point (tape.py walks fn.argtypes)."""
    tapeable = [n for n in lib.EXPORTS if built.maf_tape_fn_id(n.encode()) != -1000]
    assert len(tapeable) >= 28 and "maf_stream_fork" in tapeable and "maf_bn_sum_forward_stats" in tapeable
    for name in tapeable:
        assert len(getattr(built, name).argtypes) == built.maf_tape_fn_nargs(built.maf_tape_fn_id(name.encode())), name
