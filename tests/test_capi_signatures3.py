"""The third signature table of the policy kernel entries (capi.SIGNATURES3: the unsuffixed entries that take the device step word first) against
include/d3il_rollout.h, in the way tests/test_capi_signatures.py and tests/test_capi_signatures2.py hold the other two; and that load() / launch() serve all three
tables by name.  No GPU, no library."""
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
    """{entry: ((parameter name, ctype), ..)} of every unsuffixed ``int d3il_*(const uint32_t* t_device, .., void* stream)`` prototype of the header: a kernel entry
    that takes the device step word first and the stream last."""
    with open(HEADER) as f:
        text = f.read()
    out = {}
    for name, params in PROTOTYPE.findall(text):
        parts = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        if SUFFIXED.fullmatch(name) or (parts[0][0].strip(), parts[0][1]) != ("const uint32_t*", "t_device") or (parts[-1][0].strip(), parts[-1][1]) != ("void*", "stream"):
            continue
        out[name] = tuple((pname, C.c_void_p if ctype.strip().endswith("*") else SCALARS[ctype.strip()]) for ctype, pname in parts)
    return out


def test_third_table_covers_the_step_word_first_entries_of_the_header():
    protos = header_prototypes()
    assert set(protos) == set(capi.SIGNATURES3) == {"d3il_ddpm_mlp_chain"}
    assert not set(capi.SIGNATURES3) & (set(capi.SIGNATURES) | set(capi.SIGNATURES2)) and all(name in capi.EXPORTS for name in capi.SIGNATURES3)
    assert not any(SUFFIXED.fullmatch(name) for name in capi.SIGNATURES3)


@pytest.mark.parametrize("name", ["d3il_ddpm_mlp_chain"])
def test_names_and_types_match_the_header(name):
    proto = header_prototypes()[name]
    assert [n for n, _ in capi.SIGNATURES3[name]] == [n for n, _ in proto]
    assert [t for _, t in capi.SIGNATURES3[name]] == [t for _, t in proto]
    assert proto[0] == ("t_device", C.c_void_p) and proto[-1] == ("stream", C.c_void_p)
    assert dict(proto)["seed"] is C.c_uint64 and dict(proto)["env_offset"] is C.c_uint64 and dict(proto)["n_env"] is C.c_long and dict(proto)["bad"] is C.c_void_p


def test_the_definition_in_the_source_has_the_prototypes_parameters():
    src = open(os.path.join(os.path.dirname(HEADER), "..", "d3il_amd", "csrc", "rollout.hip")).read()
    m = re.search(r"^int d3il_ddpm_mlp_chain\((.*?)\) \{", src, re.S | re.M)
    names = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).group(2) for p in m.group(1).split(",")]
    assert names == [n for n, _ in capi.SIGNATURES3["d3il_ddpm_mlp_chain"]]


class StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def test_launch_serves_the_third_table_by_name(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(capi, "_LIB", lib)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": 0})())
    sig = capi.SIGNATURES3["d3il_ddpm_mlp_chain"][:-1]
    names = [n for n, _ in sig]
    args = {n: (None if t is C.c_void_p else 1) for n, t in sig}
    args["state"] = torch.zeros(2, 5)
    capi.launch("d3il_ddpm_mlp_chain", torch.device("cpu"), **args)
    (called, vals), = lib.calls
    assert called == "d3il_ddpm_mlp_chain" and len(vals) == len(names) + 1 and vals[names.index("state")] == args["state"].data_ptr() and vals[0] is None
    del args["tbias"]
    with pytest.raises(TypeError, match=r"missing arguments \['tbias'\], unknown arguments \['temb'\]"):
        capi.launch("d3il_ddpm_mlp_chain", torch.device("cpu"), temb=None, **args)
    assert len(lib.calls) == 1
    # the other two tables are still served
    assert "d3il_beso_step" in capi._LAUNCH and "d3il_cvae_decode_f32" in capi._LAUNCH
