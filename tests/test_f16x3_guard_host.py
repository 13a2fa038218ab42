"""Range / NaN guard of the split-f16 policy kernels (csrc/policy_f16x3.h, include/d3il_rollout.h d3il_f16x3_set_guard): the parts that answer without a GPU.
The kernels themselves are tested in tests/test_gpu_f16x3_guard.py."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")


def test_set_guard_null_answers_without_a_device():
    from d3il_amd import capi
    L = capi.load()
    assert "d3il_f16x3_set_guard" in capi.EXPORTS
    assert L.d3il_f16x3_set_guard(None) == 0           # guard off (the default): no device is touched
    assert L.d3il_f16x3_set_guard(C.c_void_p(0)) == 0
    assert L.d3il_version() == 2                         # an addition to the ABI, not a new version
    assert (capi.HXG_CLIPPED, capi.HXG_NONFINITE, capi.HXG_LAUNCHES, capi.HXG_N) == (0, 1, 2, 4)


def test_guard_counter_names_agree_with_the_header():
    import os
    import re
    from d3il_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "d3il_rollout.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    vals = {n: int(v) for n, v in re.findall(r"\b(D3IL_HXG_[A-Z]+)\s*=\s*(\d+)", text)}
    assert vals == {"D3IL_HXG_CLIPPED": capi.HXG_CLIPPED, "D3IL_HXG_NONFINITE": capi.HXG_NONFINITE, "D3IL_HXG_LAUNCHES": capi.HXG_LAUNCHES, "D3IL_HXG_N": capi.HXG_N}


def test_weight_counter_on_known_entries():
    from d3il_amd.policies import split_f16, weights_out_of_range
    w = torch.tensor([[0.5, 1e5, -7e4], [float("nan"), float("inf"), 65504.0], [-65504.0, 0.0, -float("inf")]])
    n = weights_out_of_range(w)
    assert n.dtype == torch.int64 and n.dim() == 0 and int(n) == 5          # 1e5, -7e4, nan, inf, -inf; +-65504 itself is in range
    assert int(weights_out_of_range(torch.tensor([1e5, -7e4, float("nan"), float("inf"), 65504.0]))) == 4
    assert int(weights_out_of_range(torch.randn(480, 120))) == 0
    # the split itself is what it was: saturating, bit for bit
    hi, lo = split_f16(torch.tensor([1e5, -7e4, 65504.0, 0.1]))
    assert hi.tolist()[:3] == [65504.0, -65504.0, 65504.0] and lo.tolist()[:3] == [0.0, 0.0, 0.0]
    assert float(hi[3]) == float(torch.tensor(0.1).half()) and float(lo[3]) == float(((torch.tensor(0.1) - torch.tensor(0.1).half().float()) * 2048.0).half())


def test_range_guard_without_a_device_fails_loudly():
    from d3il_amd import policies as P
    with pytest.raises(RuntimeError, match="HIP device"):
        P.RangeGuard("cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            P.RangeGuard()
        assert P.range_guard() is None
