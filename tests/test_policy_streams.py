"""The host forms of the policies' Philox streams against tests/golden/policy_streams.npz - written by tests/golden/gen_policy_streams.py with the per-policy stream
builders as they stood BEFORE they were folded into policies.philox_words / uniform24 / box_muller_f64.  Every public ``*_words`` / ``*_uniforms`` / ``*_normals``
function must give the same array, bit for bit, dtype and shape included (the f64 normals too: the same numpy operations in the same order), at three rows whose
counters cross the low-word carry, a seed with a high word, step words 0 and 2^32 - 1 and both ends of every tag layout.  The device forms are compared with these
functions by the per-policy GPU tests; this test is what catches a slip in the shared builder without a GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_policy_streams as gen  # noqa: E402

G = np.load(gen.OUT)


def test_every_public_stream_function_reproduces_its_golden_array():
    now = gen.streams()
    assert sorted(now) == sorted(G.files) and len(now) == 40
    for k in sorted(now):
        a, g = now[k], G[k]
        assert a.dtype == g.dtype and a.shape == g.shape, k
        assert np.array_equal(a, g), k
    # what the shapes are there for: the rows cross the carry into the high counter word, and the streams of different rows, steps and tags are different streams
    assert gen.OFFSET + 1 == 2 ** 32 and gen.SEED >> 32 and gen.N == 3
    w = [G["cvae_words__t%d" % t] for t in gen.STEPS]
    assert w[0].dtype == np.uint32 and w[0].shape == (3, 8, 4) and not np.array_equal(w[0], w[1]) and len({r.tobytes() for r in w[0].reshape(24, 4)}) == 24
    assert G["ddpm_gpt_normals__t0_k1_W2_A3"].dtype == np.float64 and G["bet_uniforms__t0"].dtype == np.float32
