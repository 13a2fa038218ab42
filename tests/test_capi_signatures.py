"""The signature table of the policy kernel entries (capi.SIGNATURES) against include/d3il_rollout.h, and the argument checks of capi.launch.  No GPU, no library."""
import ctypes as C
import os
import re

import pytest
import torch

from d3il_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "d3il_rollout.h")
POLICY_ENTRY = re.compile(r"^int (d3il_(?:\w+_f32|\w+_f16x3))\((.*?)\);", re.S | re.M)
SCALARS = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "long": C.c_long, "int": C.c_int, "float": C.c_float}


def header_prototypes():
    """{entry: ((parameter name, ctype), ..)} of every ``int d3il_*_f32 / _f16x3(...)`` prototype of the header."""
    with open(HEADER) as f:
        text = f.read()
    out = {}
    for name, params in POLICY_ENTRY.findall(text):
        sig = []
        for p in params.split(","):
            ctype, pname = re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups()
            ctype = ctype.strip()
            sig.append((pname, C.c_void_p if ctype.endswith("*") else SCALARS[ctype]))
        out[name] = tuple(sig)
    return out


def test_table_covers_the_policy_entries_of_the_header():
    protos = header_prototypes()
    assert len(protos) == 18
    assert set(protos) == set(capi.SIGNATURES)


@pytest.mark.parametrize("name", sorted(capi.SIGNATURES))
def test_names_and_types_match_the_header(name):
    proto = header_prototypes()[name]
    assert [n for n, _ in capi.SIGNATURES[name]] == [n for n, _ in proto]
    assert [t for _, t in capi.SIGNATURES[name]] == [t for _, t in proto]
    assert proto[-1] == ("stream", C.c_void_p)


class StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def stub(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(capi, "_LIB", lib)
    return lib


def layernorm_args():
    x = torch.zeros(2, 8)
    return dict(x=x, weight=torch.ones(8), bias=None, y=torch.empty_like(x), rows=2, C=8, eps=1e-5)


def test_launch_names_a_missing_argument(stub):
    args = layernorm_args()
    del args["weight"], args["eps"]
    with pytest.raises(TypeError, match=r"missing arguments \['eps', 'weight'\]"):
        capi.launch("d3il_layernorm_f32", torch.device("cpu"), **args)
    assert stub.calls == []


def test_launch_names_an_unknown_argument(stub):
    with pytest.raises(TypeError, match=r"unknown arguments \['gamma'\]"):
        capi.launch("d3il_layernorm_f32", torch.device("cpu"), gamma=None, **layernorm_args())
    args = layernorm_args()
    args["stream"] = 0          # the stream is the helper's to fill
    with pytest.raises(TypeError, match=r"unknown arguments \['stream'\]"):
        capi.launch("d3il_layernorm_f32", torch.device("cpu"), **args)
    assert stub.calls == []


def test_launch_refuses_a_tensor_on_another_device(stub):
    with pytest.raises(TypeError, match="weight is on cpu, the launch is on cuda:0"):
        capi.launch("d3il_layernorm_f32", torch.device("cuda:0"), **dict(layernorm_args(), x=None, y=None))
    assert stub.calls == []
