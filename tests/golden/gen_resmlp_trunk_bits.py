"""The output BITS of the five kernels that run the ResidualMLPNetwork trunk of csrc/policy_resmlp.h - k_resmlp_f32, k_cvae_decode, k_bet_mlp, k_bc_gmm,
k_ddpm_mlp_chain - through their C entries, recorded once from the library as it stood BEFORE the trunk's device code was written once:
    python tests/golden/gen_resmlp_trunk_bits.py          (needs the GPU; writes tests/golden/resmlp_trunk_bits.npz)
tests/test_gpu_resmlp_trunk_bits.py regenerates the inputs with the functions below, launches and compares every output bit for bit.

Per entry three networks - hidden 128 without blocks, hidden 128 with 3 blocks, hidden 256 with 2 blocks - at n_env = 17 (two workgroups, the second with one live
row: the tail clamp), the input width once at the entry's maximum and once at 4; the chain runs T = 1 and T = 3.  Every draw comes from the device's Philox stream
(SEED, OFFSET, step word TWORD).  Weights and states come from numpy.random.RandomState (the legacy stream, frozen across NumPy versions) and nothing else: no
torch initialiser, no library function, so the inputs are the same numbers everywhere.  The first layer has gain GAIN: the f64 mirror below must show, in every
case with blocks, a Mish argument above 20 and one below -20 (both arms of dd_mish) and only finite outputs - asserted here and again by the test's CPU half.
No weights are stored: the fixture holds the output tensors as uint32 / int32 and the compiler's version string (the bits of expf / logf belong to the compiler)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "resmlp_trunk_bits.npz")

N, SEED, OFFSET, TWORD, GAIN = 17, 0x5EED0123456789AB, (1 << 32) - 5, 0x00C0FFEE, 12.0
# entry -> [(case name, dict(hidden, blocks, obs = the state's width, ..))]; the input row is obs wide (resmlp, bet_mlp, bc_gmm), obs + L (cvae), A + t_dim + obs (chain)
CASES = {
    "resmlp": [("h128b0", dict(hidden=128, blocks=0, obs=4, out=16)), ("h128b3", dict(hidden=128, blocks=3, obs=28, out=3)), ("h256b2", dict(hidden=256, blocks=2, obs=13, out=7))],
    "cvae": [("h128b0", dict(hidden=128, blocks=0, obs=32, L=32, A=16)), ("h128b3", dict(hidden=128, blocks=3, obs=3, L=1, A=2)), ("h256b2", dict(hidden=256, blocks=2, obs=20, L=8, A=7))],
    "bet_mlp": [("h128b0", dict(hidden=128, blocks=0, obs=28, A=8)), ("h128b3", dict(hidden=128, blocks=3, obs=4, A=2)), ("h256b2", dict(hidden=256, blocks=2, obs=11, A=3))],
    "bc_gmm": [("h128b0", dict(hidden=128, blocks=0, obs=4, A=2, G=5, std_mode=0)), ("h128b3", dict(hidden=128, blocks=3, obs=28, A=8, G=64, std_mode=2)),
               ("h256b2", dict(hidden=256, blocks=2, obs=11, A=3, G=17, std_mode=1))],
    "ddpm_mlp": [("h128b0", dict(hidden=128, blocks=0, obs=1, A=2, t_dim=1, T=3)), ("h128b3", dict(hidden=128, blocks=3, obs=48, A=8, t_dim=8, T=1)),
                 ("h256b2", dict(hidden=256, blocks=2, obs=20, A=3, t_dim=4, T=3))],
}
MIN_STD = 1e-3


def case_ids():
    return [(e, name) for e, cs in CASES.items() for name, _ in cs]


def hipcc_version():
    exe = "/opt/rocm/bin/hipcc"
    for d in os.environ.get("PATH", "").split(os.pathsep):
        if os.path.exists(os.path.join(d, "hipcc")):
            exe = os.path.join(d, "hipcc")
            break
    try:
        out = subprocess.run([exe, "--version"], capture_output=True, text=True).stdout
    except OSError:
        return "no hipcc"
    return " / ".join(l.strip() for l in out.splitlines() if l.startswith(("HIP version", "AMD clang version")))      # (not the install directory)


def mish(x):
    sp = np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))
    return x * np.tanh(sp)


def inputs(entry, name):
    """Everything a launch of (entry, case) reads, as float32 numpy arrays in the reference's (unpacked) layout; RandomState seeded by the case's position."""
    c = dict(CASES[entry])[name]
    rs = np.random.RandomState(1000 * list(CASES).index(entry) + [n for n, _ in CASES[entry]].index(name) + 7)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    H, nb, obs = c["hidden"], c["blocks"], c["obs"]
    width = obs + c.get("L", 0) + (c["A"] + c["t_dim"] if entry == "ddpm_mlp" else 0)
    A = c.get("A", c.get("out"))
    d = dict(c, width=width, A=A)
    d["state"] = f(rs.standard_normal((N, obs)))
    d["W_in"], d["b_in"] = f(rs.standard_normal((H, width)) * (GAIN / np.sqrt(width))), f(rs.standard_normal(H))
    d["blk"] = [(f(rs.standard_normal((H, H)) / np.sqrt(H)), f(rs.standard_normal(H) * 0.5)) for _ in range(2 * nb)]
    lin = lambda rows, gain: (f(rs.standard_normal((rows, H)) * (gain / np.sqrt(H))), f(rs.standard_normal(rows) * 0.1))
    d["lo"], d["hi"] = f(-0.5 - rs.uniform(size=A)), f(0.5 + rs.uniform(size=A))
    d["scale"], d["shift"] = f(0.5 + rs.uniform(size=A)), f(rs.standard_normal(A))
    if entry in ("resmlp", "cvae", "ddpm_mlp"):
        d["W_out"], d["b_out"] = lin(A, 0.02)
    if entry == "bet_mlp":
        d["W_head"], d["b_head"] = lin(64 * (1 + A), 0.02)
        d["centers"] = f(rs.standard_normal((64, A)) * 0.5)
    if entry == "bc_gmm":
        d["W_feat"], d["b_feat"] = lin(H, 0.05)
        d["W_logit"], d["b_logit"] = lin(c["G"], 0.3)
        d["W_mean"], d["b_mean"] = lin(c["G"] * A, 0.1)
        d["W_std"], d["b_std"] = lin(c["G"] * A, 0.3)
    if entry == "ddpm_mlp":
        T = c["T"]
        d["temb"] = f(rs.standard_normal((T, c["t_dim"])))
        c1 = rs.uniform(0.1, 0.9, size=T)
        sig = rs.uniform(0.05, 0.3, size=T)
        sig[0] = 0.0
        d["sched"] = f(np.stack([rs.uniform(1.0, 1.5, size=T), rs.uniform(0.1, 1.0, size=T), c1, 1.0 - c1, sig], axis=1))
    return d


def mirror(entry, name):
    """The case in f64 on the CPU, the draws from the host form of the Philox stream: (the arguments of every Mish the trunk evaluates, every output value)."""
    from d3il_amd import policies as P
    d = inputs(entry, name)
    D = lambda a: np.asarray(a, dtype=np.float64)
    pre = []

    def trunk(x):
        h = x @ D(d["W_in"]).T + D(d["b_in"])
        for b in range(d["blocks"]):
            (w1, b1), (w2, b2) = d["blk"][2 * b], d["blk"][2 * b + 1]
            u = mish(h) @ D(w1).T + D(b1)
            pre.extend([h, u])
            h = h + mish(u) @ D(w2).T + D(b2)
        return h
    s = D(d["state"])
    if entry == "resmlp":
        out = [trunk(s) @ D(d["W_out"]).T + D(d["b_out"])]
    elif entry == "cvae":
        z = np.clip(P.cvae_latent_normals(SEED, OFFSET, N, TWORD, d["L"]), -0.5, 0.5)
        out = [trunk(np.concatenate([s, z], axis=1)) @ D(d["W_out"]).T + D(d["b_out"])]
    elif entry == "bet_mlp":
        out = [trunk(s) @ D(d["W_head"]).T + D(d["b_head"])]
    elif entry == "bc_gmm":
        v = trunk(s) @ D(d["W_feat"]).T + D(d["b_feat"])
        pre.append(v)
        ft = mish(v)
        out = [ft @ D(d[w]).T + D(d[b]) for w, b in (("W_logit", "b_logit"), ("W_mean", "b_mean"), ("W_std", "b_std"))]
        out.append(np.exp(out[2]))      # (std_mode 1 exponentiates the raw std)
    else:
        T, A = d["T"], d["A"]
        x = P.ddpm_mlp_normals(SEED, OFFSET, N, TWORD, 0, A)
        out = []
        for i in range(T - 1, -1, -1):
            eps = trunk(np.concatenate([x, np.tile(D(d["temb"][i]), (N, 1)), s], axis=1)) @ D(d["W_out"]).T + D(d["b_out"])
            sra, srm1, c1, c2, sig = D(d["sched"][i])
            x0 = np.clip(sra * x - srm1 * eps, D(d["lo"]), D(d["hi"]))
            zk = P.ddpm_mlp_normals(SEED, OFFSET, N, TWORD, T - i, A) if i > 0 else 0.0
            x = (c1 * x0 + c2 * x) + sig * zk
            out += [eps, x]
    return pre, out


def check_inputs(entry, name):
    """What the issue asks of the inputs, on the f64 mirror alone: both arms of dd_mish are taken in every case with blocks, and no output is non-finite."""
    pre, out = mirror(entry, name)
    assert all(np.isfinite(o).all() for o in out), (entry, name, "a non-finite output in the f64 mirror")
    blocks = dict(CASES[entry])[name]["blocks"]
    if blocks:
        p = np.concatenate([v.reshape(-1) for v in pre])
        assert (p > 20.0).any() and (p < -20.0).any(), (entry, name, "the Mish arguments do not reach beyond +-20", float(p.min()), float(p.max()))
    return len(pre)


def launch(entry, name, dev):
    """One launch of (entry, case) on ``dev`` through capi.launch: {output name: numpy array of uint32 / int32 bits}."""
    import torch
    from d3il_amd import capi
    from d3il_amd import policies as P
    d = inputs(entry, name)
    H, A, obs, nb = d["hidden"], d["A"], d["obs"], d["blocks"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    layer = lambda W, b: SimpleNamespace(weight=torch.from_numpy(W), bias=torch.from_numpy(b), in_features=W.shape[1], out_features=W.shape[0])
    lin_in = layer(d["W_in"], d["b_in"])
    blocks = [(layer(*d["blk"][2 * b]), layer(*d["blk"][2 * b + 1])) for b in range(nb)]
    todev = lambda pk: {k: (v.to(dev) if hasattr(v, "to") else v) for k, v in pk.items()}
    empty = lambda *shape, dtype=torch.float32: torch.full(shape, -1000.5 if dtype == torch.float32 else -77, dtype=dtype, device=dev)
    state, tail = t(d["state"]), dict(lo=t(d["lo"]), hi=t(d["hi"]), scale=t(d["scale"]), shift=t(d["shift"]))
    draw = dict(seed=SEED, env_offset=OFFSET, t_device=torch.tensor([TWORD], dtype=torch.int32, device=dev))
    shape = dict(hidden=H, n_blocks=nb)
    if entry == "resmlp":
        w = todev(P.pack_resmlp_weights(lin_in, blocks, layer(d["W_out"], d["b_out"])))
        o = dict(out=empty(N, A))
        capi.launch("d3il_resmlp_f32", dev, x=state, **P.resmlp_args(w), w_out=w["w_out"], b_out=w["b_out"], **o, rows=N, in_dim=obs, out_dim=A, **shape)
    elif entry == "cvae":
        w = todev(P.pack_resmlp_weights(lin_in, blocks, layer(d["W_out"], d["b_out"]), in_cols=64))
        o = dict(actions=empty(N, A), z_out=empty(N, d["L"]))
        capi.launch("d3il_cvae_decode_f32", dev, state=state, **P.resmlp_args(w), w_out=w["w_out"], b_out=w["b_out"], **tail, **draw, z_in=None, **o, n_env=N, obs_dim=obs,
                    latent=d["L"], A=A, **shape)
    elif entry == "bet_mlp":
        w = todev(P.pack_bet_mlp_weights(lin_in, blocks, layer(d["W_head"], d["b_head"])))
        o = dict(actions=empty(N, A), bins=empty(N, dtype=torch.int32), u_out=empty(N), probs=empty(N, 64))
        capi.launch("d3il_bet_mlp_f32", dev, state=state, **P.resmlp_args(w), w_logit=w["w_logit"], b_logit=w["b_logit"], w_off=w["w_off"], b_off=w["b_off"], centers=t(d["centers"]),
                    **tail, **draw, u_in=None, **o, n_env=N, obs_dim=obs, V=64, A=A, **shape)
    elif entry == "bc_gmm":
        G = d["G"]
        net = SimpleNamespace(mlp=SimpleNamespace(_parts=lambda: (lin_in, blocks, layer(d["W_feat"], d["b_feat"]))), n_gaussians=G, logits_mlp=layer(d["W_logit"], d["b_logit"]),
                              mean_mlp=layer(d["W_mean"], d["b_mean"]), std_mlp=layer(d["W_std"], d["b_std"]))
        w = todev(P.pack_bc_gmm_weights(net))
        low = d["std_mode"] == 0
        o = dict(actions=empty(N, A), comps=empty(N, dtype=torch.int32), u_out=empty(N), z_out=empty(N, A), probs=empty(N, G))
        capi.launch("d3il_bc_gmm", dev, n_env=N, t_device=draw["t_device"], state=state, **P.resmlp_args(w), w_feat=w["w_feat"], b_feat=w["b_feat"], w_logit=w["w_logit"],
                    b_logit=w["b_logit"], w_mean=w["w_mean"], b_mean=w["b_mean"], w_std=None if low else w["w_std"], b_std=None if low else w["b_std"], **tail, seed=SEED,
                    env_offset=OFFSET, u_in=None, z_in=None, **o, obs_dim=obs, G=G, A=A, std_mode=d["std_mode"], min_std=MIN_STD, **shape)
    else:
        T, td = d["T"], d["t_dim"]
        part = lambda a, b: layer(np.ascontiguousarray(d["W_in"][:, a:b]), d["b_in"])
        w = todev(P.pack_resmlp_weights(part(A + td, d["width"]), blocks, layer(d["W_out"], d["b_out"]), in_cols=64))
        w_x = P.pack_resmlp_weights(part(0, A), [], layer(d["W_out"], d["b_out"]), in_cols=8)["w_in"].to(dev)
        # the time embedding's share of the input layer, [T][H]: an INPUT here, so summed in f64 in a fixed order (no BLAS call whose order could differ by machine)
        tb = d["b_in"].astype(np.float64) + sum(d["temb"][:, k:k + 1].astype(np.float64) * d["W_in"][:, A + k].astype(np.float64)[None, :] for k in range(td))
        tbias = t(tb.astype(np.float32))
        o = dict(actions=empty(N, A), bad=empty(N, dtype=torch.int32), noise_out=empty(T + 1, N, A))
        capi.launch("d3il_ddpm_mlp_chain", dev, state=state, w_x=w_x, w_state=w["w_in"], tbias=tbias, w_blocks=w["w_blk"], b_blocks=w["b_blk"], w_out=w["w_out"], b_out=w["b_out"],
                    sched=t(d["sched"]), **tail, **draw, noise_in=None, **o, n_env=N, obs_dim=obs, A=A, t_dim=td, n_timesteps=T, **shape)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy().view(np.int32 if v.dtype == torch.int32 else np.uint32) for k, v in o.items()}


def healthy(entry, bits):
    """No row of a launch was flagged non-finite (the mirror says none is): no 0x7FC00000 action, no -1 bin / component, no bad flag; no output word left unwritten."""
    assert not (bits["out" if entry == "resmlp" else "actions"] == 0x7FC00000).any(), (entry, "a NaN action")
    for k in ("bins", "comps"):
        assert k not in bits or (bits[k] >= 0).all(), (entry, k)
    assert "bad" not in bits or (bits["bad"] == 0).all(), (entry, "bad")
    for k, v in bits.items():
        assert not (v == (np.float32(-1000.5).view(np.uint32) if v.dtype == np.uint32 else -77)).any(), (entry, k, "unwritten")


def main():
    import torch
    from d3il_amd import capi
    dev = torch.device("cuda:0")
    rec = {"hipcc_version": np.array(hipcc_version())}
    for entry, name in case_ids():
        n_pre = check_inputs(entry, name)
        bits = launch(entry, name, dev)
        healthy(entry, bits)
        for k, v in bits.items():
            rec["%s__%s__%s" % (entry, name, k)] = v
        print("%s %s: %d Mish layers in the mirror, %s" % (entry, name, n_pre, ", ".join("%s %s" % (k, v.shape) for k, v in bits.items())))
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez_compressed(out, **rec)
    print("library %s\nwrote %s (%d bytes)" % (capi.lib_path(), out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
