"""The second signature table of the policy kernel entries (capi.SIGNATURES2: the entries whose names carry no _f32 / _f16x3 suffix) against include/d3il_rollout.h, in
the way tests/test_capi_signatures.py holds capi.SIGNATURES; and that load() / launch() serve both tables by name.  No GPU, no library."""
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
    """{entry: ((parameter name, ctype), ..)} of every unsuffixed ``int d3il_*(const float* .., void* stream)`` prototype of the header: a kernel entry takes device
    arrays first and the stream last; the handle-based calls (d3il_step, d3il_reset, ..) take their handle first."""
    with open(HEADER) as f:
        text = f.read()
    out = {}
    for name, params in PROTOTYPE.findall(text):
        parts = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        if SUFFIXED.fullmatch(name) or parts[0][0].strip() != "const float*" or (parts[-1][0].strip(), parts[-1][1]) != ("void*", "stream"):
            continue
        out[name] = tuple((pname, C.c_void_p if ctype.strip().endswith("*") else SCALARS[ctype.strip()]) for ctype, pname in parts)
    return out


def test_second_table_covers_the_unsuffixed_policy_entries_of_the_header():
    protos = header_prototypes()
    assert set(protos) == set(capi.SIGNATURES2) == {"d3il_beso_step"}
    assert not set(capi.SIGNATURES2) & set(capi.SIGNATURES) and all(name in capi.EXPORTS for name in capi.SIGNATURES2)
    assert not any(SUFFIXED.fullmatch(name) for name in capi.SIGNATURES2)


@pytest.mark.parametrize("name", sorted(capi.SIGNATURES2))
def test_names_and_types_match_the_header(name):
    proto = header_prototypes()[name]
    assert [n for n, _ in capi.SIGNATURES2[name]] == [n for n, _ in proto]
    assert [t for _, t in capi.SIGNATURES2[name]] == [t for _, t in proto]
    assert proto[-1] == ("stream", C.c_void_p)


class StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def beso_args():
    names = [n for n, _ in capi.SIGNATURES2["d3il_beso_step"][:-1]]
    args = {n: (None if t is C.c_void_p else 1) for n, t in capi.SIGNATURES2["d3il_beso_step"][:-1]}
    args["x"] = torch.zeros(2, 5, 8)
    return names, args


def test_launch_serves_the_second_table_by_name(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(capi, "_LIB", lib)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": 0})())
    names, args = beso_args()
    capi.launch("d3il_beso_step", torch.device("cpu"), **args)
    (called, vals), = lib.calls
    assert called == "d3il_beso_step" and len(vals) == len(names) + 1 and vals[names.index("x")] == args["x"].data_ptr() and vals[names.index("hk")] is None
    del args["coef"]
    with pytest.raises(TypeError, match=r"missing arguments \['coef'\], unknown arguments \['temb'\]"):
        capi.launch("d3il_beso_step", torch.device("cpu"), temb=None, **args)
    assert len(lib.calls) == 1
