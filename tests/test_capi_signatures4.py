"""The fourth signature table of the policy kernel entries (capi.SIGNATURES4: the unsuffixed entries that take the row count first) against
include/d3il_rollout.h, in the way tests/test_capi_signatures.py, tests/test_capi_signatures2.py and tests/test_capi_signatures3.py hold the other three; and that
load() / launch() serve all four tables by name.  No GPU, no library."""
import ctypes as C
import os
import re

import pytest
import torch

from d3il_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "d3il_rollout.h")
PROTOTYPE = re.compile(r"^int (d3il_\w+)\((.*?)\);", re.S | re.M)
SUFFIXED = re.compile(r"d3il_\w+_(f32|f16x3)")
SCALARS = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "long": C.c_long, "int": C.c_int, "float": C.c_float}


def header_prototypes():
    """{entry: ((parameter name, ctype), ..)} of every unsuffixed ``int d3il_*(long n_env, .., void* stream)`` prototype of the header: a kernel entry that takes
    the row count first and the stream last."""
    with open(HEADER) as f:
        text = f.read()
    out = {}
    for name, params in PROTOTYPE.findall(text):
        parts = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        if SUFFIXED.fullmatch(name) or (parts[0][0].strip(), parts[0][1]) != ("long", "n_env") or (parts[-1][0].strip(), parts[-1][1]) != ("void*", "stream"):
            continue
        out[name] = tuple((pname, C.c_void_p if ctype.strip().endswith("*") else SCALARS[ctype.strip()]) for ctype, pname in parts)
    return out


def test_fourth_table_covers_the_row_count_first_entries_of_the_header():
    protos = header_prototypes()
    assert set(protos) == set(capi.SIGNATURES4) == {"d3il_bc_gmm"}
    assert not set(capi.SIGNATURES4) & (set(capi.SIGNATURES) | set(capi.SIGNATURES2) | set(capi.SIGNATURES3)) and all(name in capi.EXPORTS for name in capi.SIGNATURES4)
    assert not any(SUFFIXED.fullmatch(name) for name in capi.SIGNATURES4)


@pytest.mark.parametrize("name", ["d3il_bc_gmm"])
def test_names_and_types_match_the_header(name):
    proto = header_prototypes()[name]
    assert [n for n, _ in capi.SIGNATURES4[name]] == [n for n, _ in proto]
    assert [t for _, t in capi.SIGNATURES4[name]] == [t for _, t in proto]
    assert proto[0] == ("n_env", C.c_long) and proto[1] == ("t_device", C.c_void_p) and proto[-1] == ("stream", C.c_void_p) and len(proto) == 36
    d = dict(proto)
    assert d["seed"] is C.c_uint64 and d["env_offset"] is C.c_uint64 and d["comps"] is C.c_void_p and d["min_std"] is C.c_float and d["std_mode"] is C.c_int and d["G"] is C.c_int


def test_the_definition_in_the_source_has_the_prototypes_parameters():
    src = open(os.path.join(os.path.dirname(HEADER), "..", "d3il_amd", "csrc", "rollout.hip")).read()
    m = re.search(r"^int d3il_bc_gmm\((.*?)\) \{", src, re.S | re.M)
    names = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).group(2) for p in m.group(1).split(",")]
    assert names == [n for n, _ in capi.SIGNATURES4["d3il_bc_gmm"]]


class StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def test_launch_serves_the_fourth_table_by_name(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(capi, "_LIB", lib)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": 0})())
    sig = capi.SIGNATURES4["d3il_bc_gmm"][:-1]
    names = [n for n, _ in sig]
    args = {n: (None if t is C.c_void_p else 1) for n, t in sig}
    args["state"] = torch.zeros(2, 5)
    capi.launch("d3il_bc_gmm", torch.device("cpu"), **args)
    (called, vals), = lib.calls
    assert called == "d3il_bc_gmm" and len(vals) == len(names) + 1 and vals[names.index("state")] == args["state"].data_ptr() and vals[0] == 1 and vals[1] is None
    assert vals[names.index("w_std")] is None      # (NULL in low-noise mode)
    del args["w_feat"]
    with pytest.raises(TypeError, match=r"missing arguments \['w_feat'\], unknown arguments \['w_out'\]"):
        capi.launch("d3il_bc_gmm", torch.device("cpu"), w_out=None, **args)
    assert len(lib.calls) == 1
    # the other three tables are still served
    assert "d3il_beso_step" in capi._LAUNCH and "d3il_cvae_decode_f32" in capi._LAUNCH and "d3il_ddpm_mlp_chain" in capi._LAUNCH


def test_the_library_binds_the_entry():
    """load() gives the entry the table's argtypes; the tag constant keeps the name the pinned set of *_TAG names leaves free; the ABI version stays."""
    from d3il_amd import policies as P
    lib = capi.load()
    assert lib.d3il_bc_gmm.argtypes == [t for _, t in capi.SIGNATURES4["d3il_bc_gmm"]]
    assert capi.TAG_BC_GMM == P.BC_GMM_TAG == 0x474D0000 and not hasattr(capi, "BC_GMM_TAG")
    assert lib.d3il_version() == 2
