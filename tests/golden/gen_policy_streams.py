"""Golden vectors for the host forms of the policies' Philox streams (d3il_amd/policies.py): the word builders, the 24-bit uniforms and the f64 Box-Muller normals
of BeT, DDPM-GPT, IBC, ACT, CVAE and DDPM-ACT, called through their PUBLIC names only, at the smallest shapes at which a stream builder can go wrong - three rows, a
seed with a non-zero high word, an environment offset of 2^32 - 1 (rows 1 and 2 carry into the high counter word), step words 0 and 2^32 - 1, and the two ends of every
tag layout.

    python tests/golden/gen_policy_streams.py            # writes tests/golden/policy_streams.npz (fixed archive timestamps: a second run reproduces it byte for byte)
    python tests/golden/gen_policy_streams.py --check    # compares instead of writing

The committed file was written by the code BEFORE the stream builders were folded into one; tests/test_policy_streams.py asserts np.array_equal (dtype and shape
included) on every array, so a change to the shared builder that moves any policy's stream fails on the CPU.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from d3il_amd import policies as P  # noqa: E402

OUT = os.path.join(HERE, "policy_streams.npz")
N = 3
SEED = 0x9E3779B97F4A7C15          # non-zero high word
OFFSET = 2 ** 32 - 1               # row 0 ends the low counter word, rows 1 and 2 carry
STEPS = (0, 2 ** 32 - 1)


def streams() -> dict:
    """name -> array; the name spells the call."""
    out = {}
    for t in STEPS:
        a = (SEED, OFFSET, N, t)
        out["bet_uniforms__t%d" % t] = P.bet_uniforms(*a)
        for k, W, A in ((1, 2, 3), (255, 16, 8)):
            out["ddpm_gpt_words__t%d_k%d_W%d" % (t, k, W)] = P.ddpm_gpt_words(*a, k, W)
            out["ddpm_gpt_normals__t%d_k%d_W%d_A%d" % (t, k, W, A)] = P.ddpm_gpt_normals(*a, k, W, A)
        for kind in (0, 1, 2):
            out["ibc_words__t%d_kind%d_k63_S64" % (t, kind)] = P.ibc_words(*a, kind, 63, 64)
        out["ibc_start_uniforms__t%d_A3_S64" % t] = P.ibc_start_uniforms(*a, 3, 64)
        out["ibc_normals__t%d_k63_A8_S64" % t] = P.ibc_normals(*a, 63, 8, 64)
        out["ibc_pick_uniforms__t%d" % t] = P.ibc_pick_uniforms(*a)
        out["act_latent_words__t%d" % t] = P.act_latent_words(*a)
        out["act_latent_uniforms__t%d" % t] = P.act_latent_uniforms(*a)
        out["cvae_words__t%d" % t] = P.cvae_words(*a)
        for L in (1, 32):
            out["cvae_latent_normals__t%d_L%d" % (t, L)] = P.cvae_latent_normals(*a, L)
        for k in (1, 255):
            out["ddpm_act_words__t%d_k%d_Ta4" % (t, k)] = P.ddpm_act_words(*a, k, 4)
            out["ddpm_act_normals__t%d_k%d_Ta4_A8" % (t, k)] = P.ddpm_act_normals(*a, k, 4, 8)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def archive(arrays: dict) -> bytes:
    """A compressed .npz with fixed member timestamps (np.savez stamps the current time)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.save(b, arrays[k])
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(), zipfile.ZIP_DEFLATED)
    return buf.getvalue()


if __name__ == "__main__":
    data = archive(streams())
    if "--check" in sys.argv:
        assert open(OUT, "rb").read() == data, "tests/golden/policy_streams.npz differs from what the public functions give now"
        print("ok: %s reproduces" % OUT)
    else:
        with open(OUT, "wb") as f:
            f.write(data)
        print("wrote %s: %d arrays, %d bytes" % (OUT, len(streams()), len(data)))
