"""The fifth signature table of the policy kernel entries (capi.SIGNATURES5: suffixed entries whose prototype has the return type on a line of its own) against
include/d3il_rollout.h, in the way the other four test files hold theirs; and that load() / launch() serve it by name.  No GPU."""
import ctypes as C
import os
import re

import torch

from d3il_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "d3il_rollout.h")
PROTOTYPE = re.compile(r"^int\n(d3il_\w+)\((.*?)\);", re.S | re.M)
SCALARS = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "long": C.c_long, "int": C.c_int, "float": C.c_float}


def header_prototypes():
    with open(HEADER) as f:
        text = f.read()
    out = {}
    for name, params in PROTOTYPE.findall(text):
        parts = [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(",")]
        out[name] = tuple((pname, C.c_void_p if ctype.strip().endswith("*") else SCALARS[ctype.strip()]) for ctype, pname in parts)
    return out


def test_fifth_table_covers_the_two_line_prototypes_of_the_header():
    protos = header_prototypes()
    assert set(protos) == set(capi.SIGNATURES5) == {"d3il_gpt_trunk72_f16x3"}
    others = set(capi.SIGNATURES) | set(capi.SIGNATURES2) | set(capi.SIGNATURES3) | set(capi.SIGNATURES4)
    assert not set(capi.SIGNATURES5) & others and all(name in capi.EXPORTS for name in capi.SIGNATURES5)
    assert set(capi.ALL_SIGNATURES) == others | set(capi.SIGNATURES5) == set(capi._LAUNCH)


def test_names_and_types_match_the_header_and_the_definition():
    proto = header_prototypes()["d3il_gpt_trunk72_f16x3"]
    assert capi.SIGNATURES5["d3il_gpt_trunk72_f16x3"] == proto
    assert [n for n, _ in proto] == ["x", "w_packed", "vec", "ln_eps", "out", "n_seq", "T", "n_layer", "stream"]
    assert dict(proto)["ln_eps"] is C.c_float and dict(proto)["n_seq"] is C.c_long and dict(proto)["T"] is C.c_int and proto[-1] == ("stream", C.c_void_p)
    src = open(os.path.join(os.path.dirname(HEADER), "..", "d3il_amd", "csrc", "rollout.hip")).read()
    m = re.search(r"^int d3il_gpt_trunk72_f16x3\((.*?)\) \{", src, re.S | re.M)
    assert [re.fullmatch(r"\s*(.*?)(\w+)\s*", p).group(2) for p in m.group(1).split(",")] == [n for n, _ in proto]


def test_the_entry_validates_before_it_launches():
    """Shape and pointer checks answer without a device: D3IL_EUNSUPPORTED for T, n_layer and n_seq out of range, D3IL_EINVAL for null, misaligned and aliased pointers."""
    L = capi.load()
    assert L.d3il_gpt_trunk72_f16x3.argtypes == [t for _, t in capi.SIGNATURES5["d3il_gpt_trunk72_f16x3"]]
    x, w, v, o = (C.c_void_p(4096 + 1024 * k) for k in range(4))      # never dereferenced on these paths
    call = lambda x=x, w=w, v=v, o=o, n=3, T=5, nl=4: L.d3il_gpt_trunk72_f16x3(x, w, v, 1e-5, o, n, T, nl, None)
    for kw in (dict(T=0), dict(T=17), dict(nl=0), dict(nl=9), dict(n=0)):
        assert call(**kw) == -5, kw
    for kw in (dict(x=None), dict(w=None), dict(v=None), dict(o=None), dict(x=C.c_void_p(4100)), dict(v=C.c_void_p(8200)), dict(o=x)):
        assert call(**kw) == -1, kw
    assert b"d3il_gpt_trunk72_f16x3" in L.d3il_last_error()


class StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def test_launch_serves_the_fifth_table_by_name(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(capi, "_LIB", lib)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"cuda_stream": 0})())
    x = torch.zeros(2, 3, 72)
    capi.launch("d3il_gpt_trunk72_f16x3", torch.device("cpu"), x=x, w_packed=None, vec=None, ln_eps=1e-5, out=None, n_seq=2, T=3, n_layer=4)
    (called, vals), = lib.calls
    assert called == "d3il_gpt_trunk72_f16x3" and vals == (x.data_ptr(), None, None, 1e-5, None, 2, 3, 4, 0)
