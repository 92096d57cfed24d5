"""CPU: the reusable-session entries and pfdr_reload are declared, exported and
listed; the ABI is still 4; the ctypes mirror has the header's field order."""
import os
import re

from cp_pfdr_graph_d1_amd import pfdr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "pfdr_mi355x.h")

NEW_ENTRIES = ["pfdr_session_create_reusable", "pfdr_session_reload"]


def _struct_body():
    txt = open(HEADER).read()
    m = re.search(r"typedef\s+struct\s+pfdr_reload\s*\{(.*?)\}\s*pfdr_reload;", txt, re.S)
    assert m, "pfdr_reload is not declared"
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_header_declares_the_entries_and_abi_4():
    txt = open(HEADER).read()
    assert re.search(r"\bint\s+pfdr_session_create_reusable\s*\(\s*pfdr_session\s*\*\*\s*\w+,\s*"
                     r"const\s+pfdr_problem\s*\*\s*\w+,\s*const\s+pfdr_csc\s*\*\s*\w+\)", txt)
    assert re.search(r"\bint\s+pfdr_session_reload\s*\(\s*pfdr_session\s*\*\s*\w+,\s*"
                     r"const\s+pfdr_reload\s*\*\s*\w+\)", txt)
    assert re.search(r"int\s+pfdr_abi_version\(void\);\s*/\*\s*4\b", txt)


def test_header_struct_fields():
    """int mem; five const void *; six doubles; int itMax -- in this order"""
    names = []
    for decl in _struct_body().split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = re.match(r"(const\s+void|double|int)\b", decl).group(1)
        for name in decl[len(ctype):].split(","):
            names.append((re.sub(r"\s+", " ", ctype), name.replace("*", "").strip()))
    assert names == [("int", "mem"), ("const void", "X"), ("const void", "Y"),
                     ("const void", "La_d1"), ("const void", "La_l1"), ("const void", "L"),
                     ("double", "min"), ("double", "max"), ("double", "rho"),
                     ("double", "condMin"), ("double", "difRcd"), ("double", "difTol"),
                     ("int", "itMax")]
    import ctypes as C
    kinds = {"int": C.c_int, "const void": C.c_void_p, "double": C.c_double}
    assert [(kinds[t], n) for t, n in names] == [(t, n) for n, t in pfdr.Reload._fields_]


def test_library_exports_the_entries():
    lib = pfdr.load()
    assert lib.pfdr_abi_version() == pfdr.ABI_VERSION == 4
    for name in NEW_ENTRIES:
        assert name in pfdr.EXPORTED, name
        assert hasattr(lib, name), name


def test_python_front_end_has_reload():
    import inspect
    assert "reusable" in inspect.signature(pfdr.Session.__init__).parameters
    assert list(inspect.signature(pfdr.Session.reload).parameters)[1:] == [
        "Y", "La_d1", "La_l1", "X0", "L", "lo", "hi", "rho", "condMin", "difRcd", "difTol", "itMax"]
