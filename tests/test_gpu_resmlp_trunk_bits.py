"""The five kernels that run the ResidualMLPNetwork trunk of csrc/policy_resmlp.h (k_resmlp_f32, k_cvae_decode, k_bet_mlp, k_bc_gmm, k_ddpm_mlp_chain), through
their C entries, against the output BITS recorded from the library before the trunk's device code was written once (tests/golden/resmlp_trunk_bits.npz, written by
tests/golden/gen_resmlp_trunk_bits.py, which also makes the inputs here): hidden 128 with 0 and 3 blocks, hidden 256 with 2, n_env = 17 (a second workgroup with one
live row), the input width at the entry's maximum and at 4, the chain at T = 1 and T = 3, every draw from the device's Philox stream.  Every output tensor must be
equal bit for bit.  The bits of expf / logf belong to the compiler: with another hipcc than the recorded one the GPU cases skip and say which two."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_resmlp_trunk_bits", os.path.join(HERE, "golden", "gen_resmlp_trunk_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
IDS = G.case_ids()


@pytest.fixture(scope="module")
def recorded():
    return np.load(G.FIXTURE)


def test_the_fixture_holds_every_case(recorded):
    outs = {"resmlp": {"out"}, "cvae": {"actions", "z_out"}, "bet_mlp": {"actions", "bins", "u_out", "probs"}, "bc_gmm": {"actions", "comps", "u_out", "z_out", "probs"},
            "ddpm_mlp": {"actions", "bad", "noise_out"}}
    want = {"%s__%s__%s" % (e, n, k) for e, n in IDS for k in outs[e]} | {"hipcc_version"}
    assert set(recorded.files) == want
    assert len(IDS) == 15 and all(recorded[k].dtype in (np.uint32, np.int32) for k in want - {"hipcc_version"})
    for e, n in IDS:
        G.healthy(e, {k: recorded["%s__%s__%s" % (e, n, k)] for k in outs[e]})


@pytest.mark.parametrize("entry,name", IDS, ids=["%s-%s" % c for c in IDS])
def test_the_inputs_do_their_job(entry, name):
    """No GPU: both arms of dd_mish and only finite outputs on the f64 mirror, so that a later change of seed or shape cannot quietly empty a case."""
    G.check_inputs(entry, name)


@gpu
@pytest.mark.parametrize("entry,name", IDS, ids=["%s-%s" % c for c in IDS])
def test_bits(recorded, entry, name):
    have, rec = G.hipcc_version(), str(recorded["hipcc_version"])
    if have != rec:
        pytest.skip("the fixture's bits were recorded with the library of [%s]; the installed compiler is [%s]" % (rec, have))
    bits = G.launch(entry, name, torch.device("cuda:0"))
    for k, v in bits.items():
        want = recorded["%s__%s__%s" % (entry, name, k)]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        diff = np.flatnonzero(v.reshape(-1) != want.reshape(-1))
        print("%s %s %s: %d of %d words differ" % (entry, name, k, diff.size, v.size))
        assert diff.size == 0, "%s: %d words differ, the first at %d: %#x against %#x" % (k, diff.size, diff[0], v.reshape(-1)[diff[0]], want.reshape(-1)[diff[0]])
