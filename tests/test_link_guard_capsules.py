"""Link-near guard, data and ABI (CPU): the committed bounding capsules of the rod robot's collision hulls hold their hulls (T1), and the flag bit and
the entry point are declared where the binding looks for them (T2)."""
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = os.path.join(ROOT, "d3il_amd", "model", "blobs", "panda_link_capsules.json")
HULLS = os.path.join(ROOT, "tests", "golden", "panda_link_hulls.npz")
BODIES = ["link0", "link1", "link2", "link3", "link4", "link5", "link6", "link7", "hand", "leftfinger", "rightfinger"]


def _segment_distance(v, p0, p1):
    d = p1 - p0
    L2 = float(d @ d)
    s = np.clip((v - p0) @ d / L2, 0.0, 1.0) if L2 > 0 else np.zeros(len(v))
    return np.linalg.norm(v - (p0 + np.outer(s, d)), axis=1)


def test_every_hull_vertex_lies_inside_its_capsule():
    """T1: every hull vertex within 1e-9 m of its capsule; a capsule's radius is no larger than the radius of the bounding sphere of its hull about the
    hull vertices' centroid (the sphere the fit degenerates to: a capsule looser than that is a bug in the fit)."""
    with open(CAPS) as f:
        js = json.load(f)
    hulls = np.load(HULLS)
    caps = {c["body"]: c for c in js["capsules"]}
    assert sorted(caps) == sorted("panda_rb0_" + b for b in BODIES) and sorted(hulls.files) == sorted(BODIES)
    assert js["margin"] == 0.02
    for b in BODIES:
        c, v = caps["panda_rb0_" + b], hulls[b]
        assert v.dtype == np.float64 and v.ndim == 2 and v.shape[1] == 3 and len(v) >= 8
        p0, p1, r = np.array(c["p0"]), np.array(c["p1"]), c["r"]
        excess = float((_segment_distance(v, p0, p1) - r).max())
        sphere = float(np.linalg.norm(v - v.mean(0), axis=1).max())
        print("%-12s r %.4f length %.4f excess %.2e bounding sphere %.4f" % (b, r, np.linalg.norm(p1 - p0), excess, sphere))
        assert excess <= 1e-9, (b, excess)
        assert 0 < r <= sphere, (b, r, sphere)
        assert c["statics"] == int(b in ("link5", "link6", "link7", "hand", "leftfinger", "rightfinger"))


def test_capsule_body_ids_match_the_blobs():
    """The body id recorded per task is the body's place in that blob's body list (what d3il_set_link_guard takes)."""
    with open(CAPS) as f:
        js = json.load(f)
    for task in ("pushing", "sorting", "sorting_2", "inserting"):
        with open(os.path.join(ROOT, "d3il_amd", "model", "blobs", task + ".json")) as f:
            names = [b["name"] for b in json.load(f)["bodies"]]
        for c in js["capsules"]:
            assert names[c["body_id"][task]] == c["body"]
    from d3il_amd import capi
    arr, margin = capi.link_capsules(names)
    assert arr.shape == (11, 9) and margin == 0.02 and (arr[:, 8] > 0).all()


def test_abi_constant_and_symbol():
    """T2: D3IL_PFLAG_LINK_NEAR == 1 << 20 == capi.PFLAG_LINK_NEAR == capi.SFLAG_HAND_NEAR; d3il_set_link_guard declared and exported."""
    from d3il_amd import capi
    hdr = open(os.path.join(ROOT, "include", "d3il_rollout.h")).read()
    m = re.search(r"D3IL_PFLAG_LINK_NEAR\s*=\s*1\s*<<\s*(\d+)", hdr)
    assert m and int(m.group(1)) == 20
    assert capi.PFLAG_LINK_NEAR == 1 << 20 == capi.SFLAG_HAND_NEAR
    assert re.search(r"int\s+d3il_set_link_guard\s*\(\s*d3il_handle\s+h\s*,\s*const\s+double\s*\*\s*capsules\s*,\s*int\s+n\s*,\s*double\s+margin\s*,\s*int64_t\s*\*\s*flagged_episodes_device\s*\)\s*;", hdr)
    assert "d3il_set_link_guard" in capi.EXPORTS
    src = open(os.path.join(ROOT, "d3il_amd", "csrc", "rollout.hip")).read()
    assert re.search(r"^int d3il_set_link_guard\(", src, re.M)
    assert "static_assert(D3IL_PFLAG_LINK_NEAR == LG_FLAG && D3IL_PFLAG_LINK_NEAR == D3IL_SFLAG_HAND_NEAR" in src
