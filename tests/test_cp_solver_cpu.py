"""The resumable cut-pursuit solver (pfdr_cp_solver_*), the part that needs no
GPU: the header declares the handle's functions and its two structs, the built
library exports them, and the Python face has the documented signatures."""
import inspect
import os
import re
import subprocess

from cp_pfdr_graph_d1_amd import pfdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVER = ["pfdr_cp_solver_" + n for n in ("create", "destroy", "run", "get_state", "set_state",
                                          "set_partition", "set_penalties", "stats")]
NEW = SOLVER + ["pfdr_cpgraph_set_weights", "pfdr_cpgraph_set_active_by_labels"]


def header():
    return open(os.path.join(ROOT, "include", "pfdr_mi355x.h")).read()


def test_header_declares_the_handle():
    hdr = header()
    declared = set(re.findall(r"\b(pfdr_[a-z0-9_]+)\s*\(", hdr))
    for n in NEW:
        assert n in declared, n
        assert n in pfdr.EXPORTED, n
    assert re.search(r"typedef struct pfdr_cp_solver pfdr_cp_solver;", hdr)
    for struct, fields in (("pfdr_cp_problem", ("kind", "duplex", "dtype", "mem", "V, E, N, K",
                                                "*Y", "*A", "*Eu, *Ev", "*La_d1", "*La_l1",
                                                "positivity", "min, max", "al")),
                           ("pfdr_cp_params", ("CP_difTol", "CP_itMax", "rho, condMin, difRcd, "
                                               "difTol", "itMax", "verbose"))):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S)
        assert m, struct
        for f in fields:
            assert f in m.group(1), (struct, f)
    assert "int pfdr_abi_version(void);          /* 4" in hdr  # additive: the ABI stays 4
    assert pfdr.ABI_VERSION == 4


def test_library_exports_the_handle():
    out = subprocess.run(["nm", "-D", "--defined-only", pfdr.LIB_PATH], check=True,
                         capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for n in NEW:
        assert n in exported, n
    assert pfdr.load().pfdr_abi_version() == 4


def test_ctypes_mirrors_match_the_structs():
    hdr = header()
    for struct, cls in (("pfdr_cp_problem", pfdr.CPProblem), ("pfdr_cp_params", pfdr.CPParams)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [w.strip(" *") for w in re.sub(r"^(const\s+)?\w+\s+", "", decl).split(",")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def test_python_face():
    for n in ("create", "destroy", "run", "get_state", "set_state", "set_partition",
              "set_penalties", "stats"):
        assert callable(getattr(pfdr.Lib, "cp_solver_" + n)), n
    S = pfdr.CPSolver
    assert list(inspect.signature(S.__init__).parameters)[1:] == [
        "kind", "Y_or_Q", "Eu", "Ev", "La_d1", "A", "N", "La_l1", "positivity", "lo", "hi", "K",
        "al", "duplex"]
    run = list(inspect.signature(S.run).parameters)
    assert run[1:9] == ["CP_difTol", "CP_itMax", "rho", "condMin", "difRcd", "difTol", "itMax",
                        "verbose"]
    assert list(inspect.signature(S.set_partition).parameters)[1:] == ["label", "values"]
    assert list(inspect.signature(S.set_penalties).parameters)[1:] == ["La_d1", "La_l1"]
    for n in ("state", "set_state", "stats", "close"):
        assert callable(getattr(S, n)), n
