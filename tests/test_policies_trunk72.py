"""The host side of the 72-wide trunk kernel (policies.pack_trunk72_weights, run_blocks and their helpers), without a GPU: the packed stream against the layout
include/d3il_rollout.h states, run_blocks against the loop it replaced, the refusals, the chain's PackedWeights, and the input conditions of the two GPU test files
(tests/test_gpu_trunk72.py, tests/test_gpu_policies_trunk72.py)."""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import test_gpu_policies_trunk72 as pol72      # noqa: E402  (modules, so nothing of them is collected here)
from tests import test_gpu_trunk72 as k72      # noqa: E402


def unpack(w_layer):
    """One layer of the stream [28][768][8] back into Wqkv, Wproj, W1, W2 as f64 hi + 2^-11 lo, written from the layout of the header with plain loops over
    (stage, entry, lane); also returns the number of packed values that were read (the rest must be padding)."""
    v = (w_layer.double().reshape(28, 6, 2, 64, 8))
    val = v[:, :, 0] + v[:, :, 1] / 2048.0      # [28][6][64][8]
    mats = [torch.zeros(216, 72, dtype=torch.float64), torch.zeros(72, 72, dtype=torch.float64), torch.zeros(288, 72, dtype=torch.float64),
            torch.zeros(72, 288, dtype=torch.float64)]
    used = torch.zeros(28, 6, 64, 8, dtype=torch.bool)
    for stage in range(28):
        for ent in range(6):
            for lane in range(64):
                g, i = lane // 16, lane % 16
                for e in range(8):
                    if stage < 10 or (stage - 10) % 2 == 0:
                        u, s = ent // 3, ent % 3
                        m, tile = (0, 2 * stage + u) if stage < 7 else (1, 2 * (stage - 7) + u) if stage < 10 else (2, 2 * ((stage - 10) // 2) + u)
                        row, col = 16 * tile + i, 32 * s + 8 * g + e
                    else:
                        m, k = 3, (stage - 11) // 2
                        row, col = 16 * ent + i, 32 * k + 16 * (e >> 2) + 4 * g + (e & 3)
                    if row < mats[m].shape[0] and col < mats[m].shape[1]:
                        mats[m][row, col] = val[stage, ent, lane, e]
                        used[stage, ent, lane, e] = True
    return mats, used


def test_pack_round_trip():
    from d3il_amd import policies as P
    blocks = k72.blocks_of(13, 4)
    pk = P.pack_trunk72_weights(blocks)
    assert pk["w"].shape == (4, P.TRUNK72_STAGES, P.TRUNK72_STAGE_V, 8) and pk["w"].dtype == torch.float16 and pk["w"].is_contiguous()
    assert pk["vec"].shape == (4, P.TRUNK72_VEC) and pk["vec"].dtype == torch.float32 and int(pk["w_oor"]) == 0
    for l in (0, 3):
        mats, used = unpack(pk["w"][l])
        for got, want in zip(mats, P.trunk72_layer_matrices(blocks[l])):
            err = (got - want.double()).abs()
            assert float((err / want.double().abs().clamp_min(2.0 ** -13)).max()) <= 2.0 ** -22, "22 bits at O(1) weights"
        v = pk["w"][l].reshape(28, 6, 2, 64, 8)
        assert int(used.sum()) == 2 * (216 * 72 + 72 * 72 + 288 * 72) - 288 * 72 and not bool(v[:, :, 0][~used].any()) and not bool(v[:, :, 1][~used].any()), "padding is zero"
        blk = blocks[l]
        a = blk.attn
        want_vec = torch.cat((blk.ln1.weight, blk.ln1.bias, a.query.bias, a.key.bias, a.value.bias, a.proj.bias, blk.ln2.weight, blk.ln2.bias, blk.mlp[0].bias, blk.mlp[2].bias))
        assert torch.equal(pk["vec"][l], want_vec)
    bad = copy.deepcopy(blocks)
    with torch.no_grad():
        bad[1].mlp[0].weight[3, 4] = 7e4
        bad[2].attn.key.weight[0, 0] = float("nan")
    assert int(P.pack_trunk72_weights(bad)["w_oor"]) == 2
    assert P.trunk72_pack_index("cpu") is P.trunk72_pack_index("cpu")      # behind _cached_index


def old_loop(blocks, x, keep=None):
    for blk in blocks[:-1]:
        x = blk(x)
    return blocks[-1](x, keep=keep)


def test_run_blocks_on_the_cpu_is_the_old_loop(monkeypatch):
    from d3il_amd import policies as P
    monkeypatch.setattr(P, "trunk72", lambda *a: pytest.fail("the kernel has no business on the CPU"))
    blocks = k72.blocks_of(13, 4)
    x = k72.rows_of(3, 9, 11)
    keep = torch.arange(2, 11, 2)
    assert torch.equal(P.run_blocks(blocks, x), old_loop(blocks, x)) and torch.equal(P.run_blocks(blocks, x, keep=keep), old_loop(blocks, x, keep))
    # ... and the five places that walked the chain themselves give what they gave: DiffusionGPT (three forms), MinGPTTrunk, DiffusionGPTDenoiser
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        gpt, trunk, den = P.DiffusionGPT(4, 2, 72, 4, 4, 5), P.MinGPTTrunk(4, 72, 4, 4, 5, 64, 2), P.DiffusionGPTDenoiser(4, 2, 72, 4, 4, 5)
    xb = k72.rows_of(4, 6, 11)
    with torch.no_grad():
        assert torch.equal(gpt.hidden(xb, keep), old_loop(gpt.blocks, xb, keep)) and torch.equal(den.hidden(xb, keep), old_loop(den.blocks, xb, keep))
        o = torch.randn(6, 5, 4, generator=k72.gen(5))
        h = (trunk.tok_emb(o) + trunk.pos_emb[:, :5, :]).contiguous()
        assert torch.equal(trunk.hidden(o, keep=keep[:1]), old_loop(trunk.blocks, h, keep[:1]))
        st, ac, sg = torch.randn(6, 5, 4, generator=k72.gen(6)), torch.randn(6, 5, 2, generator=k72.gen(7)), torch.full((6,), 0.3)
        assert gpt(st, ac, sg).shape == (6, 5, 2) and den(ac, torch.arange(6), st).shape == (6, 5, 2)


def test_refusals():
    """The shape and input predicates, whatever the device: 6 heads, T = 17, mismatched eps, gradients wanted; on the CPU the kernel is never taken."""
    from d3il_amd import policies as P
    blocks = k72.blocks_of(13, 4)
    x = k72.rows_of(3, 9, 11)
    assert P.trunk72_shape_refusal(blocks) is None and P.trunk72_input_refusal(blocks, x) is None
    assert not P.trunk72_static_ok(blocks), "CPU weights"
    six = torch.nn.Sequential(*[P._Block(72, 6, 16) for _ in range(2)]).requires_grad_(False)
    assert "4 heads" in P.trunk72_shape_refusal(six)
    wide = torch.nn.Sequential(*[P._Block(120, 6, 16) for _ in range(2)]).requires_grad_(False)
    assert P.trunk72_shape_refusal(wide) is not None and P.trunk72_shape_refusal(torch.nn.Sequential(*[copy.deepcopy(blocks[0]) for _ in range(9)])) is not None
    eps = copy.deepcopy(blocks)
    eps[2].ln2.eps = 1e-6
    assert "eps" in P.trunk72_shape_refusal(eps)
    assert "T <= 16" in P.trunk72_input_refusal(blocks, k72.rows_of(3, 2, 17))
    assert P.trunk72_input_refusal(blocks, x[:, :, :64]) is not None and P.trunk72_input_refusal(blocks, x.double()) is not None
    assert "contiguous" in P.trunk72_input_refusal(blocks, x[:, ::2]) and "contiguous" in P.trunk72_input_refusal(blocks, x.reshape(-1)[1:1 + 8 * 11 * 72].view(8, 11, 72))
    with torch.enable_grad():
        assert "gradients" in P.trunk72_input_refusal(blocks, x.clone().requires_grad_(True))
        train = copy.deepcopy(blocks).requires_grad_(True)
        assert "gradients" in P.trunk72_input_refusal(train, x)
        with torch.no_grad():
            assert P.trunk72_input_refusal(train, x) is None
    assert P.trunk72_switch_on() == (P.TRUNK72_DEFAULT != "0")


def test_switches(monkeypatch):
    from d3il_amd import policies as P
    monkeypatch.delenv("D3IL_POLICY_GEMM", raising=False)
    monkeypatch.setenv("D3IL_POLICY_TRUNK72", "1")
    assert P.trunk72_switch_on()
    monkeypatch.setenv("D3IL_POLICY_TRUNK72", "0")
    assert not P.trunk72_switch_on()
    monkeypatch.setenv("D3IL_POLICY_TRUNK72", "1")
    monkeypatch.setenv("D3IL_POLICY_GEMM", "f32")
    assert not P.trunk72_switch_on()


def test_the_chain_keeps_its_own_packed_weights():
    """One PackedWeights per chain, a plain attribute: state_dict() keeps the reference's names, a deep copy gets its own, an in-place write repacks, invalidate too."""
    from d3il_amd import policies as P
    blocks = copy.deepcopy(k72.blocks_of(13, 4))
    names = set(blocks.state_dict())
    pw = P.trunk72_packed(blocks)
    assert P.trunk72_packed(blocks) is pw and set(blocks.state_dict()) == names and len(list(blocks.children())) == 4
    pack = lambda b: (P._trunk72_params(b), lambda: P.pack_trunk72_weights(b))
    pw.ensure(*pack(blocks))
    w0, ptr = pw.buf["w"].clone(), pw.buf["w"].data_ptr()
    twin = copy.deepcopy(blocks)
    tw = P.trunk72_packed(twin)
    assert tw is not pw and tw.buf["w"].data_ptr() != ptr
    with torch.no_grad():
        blocks[1].attn.proj.weight.mul_(2.0)
    pw.ensure(*pack(blocks))
    assert pw.buf["w"].data_ptr() == ptr and not torch.equal(pw.buf["w"][1], w0[1]) and torch.equal(pw.buf["w"][0], w0[0])      # in place: a captured graph reads the new weights
    tw.ensure(*pack(twin))
    assert torch.equal(tw.buf["w"], w0)
    old = blocks[0].ln1.weight.detach().clone()
    blocks[0].ln1.weight.data.add_(1.0)      # a write the version counters do not see
    pw.ensure(*pack(blocks))
    assert torch.equal(pw.buf["vec"][0, :72], old)
    P.invalidate_blocks_packed(blocks)
    pw.ensure(*pack(blocks))
    assert torch.equal(pw.buf["vec"][0, :72], blocks[0].ln1.weight)


def test_the_inputs_do_their_job():
    """Every case of the GPU files has the property its name claims."""
    # ---- the NaN sits where the case says, in one operand
    c = k72.NAN_CASE
    x, bad = k72.nan_input()
    where = torch.isnan(bad).nonzero().tolist()
    assert where == [[c["seq"], c["tok"], c["col"]]] and 0 < c["tok"] < c["T"] and torch.isfinite(x).all()
    assert c["seq"] // (16 // c["T"]) == 0 and c["n_seq"] > 16 // c["T"], "the NaN sequence shares its tile with clean ones, and there is a second tile"
    # ---- the clipped case: exactly one row has a split-site operand beyond 65504, at the GELU output, about 7e4; no operand is non-finite
    blocks, xc = k72.clip_case()
    sites = []
    k72.restate(blocks, xc, torch.float64, "cpu", sites)
    over = [(v.abs().amax(dim=-1) > 65504.0).nonzero().tolist() for v in sites[0]]
    cc = k72.CLIP_CASE
    assert over == [[], [], [], [[cc["seq"], cc["tok"]]]] and all(bool(torch.isfinite(v).all()) for v in sites[0])
    ge = sites[0][3]
    assert 6.9e4 < float(ge.abs().max()) < 7.1e4 and float(ge.abs().amax(dim=-1).flatten().sort().values[-2]) < 3.0e4, "the other rows stay far from the bound"
    # ---- the padded shapes have dead rows and dead waves
    for T in k72.T_ALL:
        spt = 16 // T
        ns = k72.seq_counts(T)
        assert 1 in ns and spt in ns and spt + 1 in ns and 4 * spt + 1 in ns and 130 in ns
        tiles = lambda n: -(-n // spt)
        assert any(tiles(n) % 4 != 0 for n in ns), "dead waves"
        assert T == 16 or 16 % T != 0 or any(n % spt != 0 for n in ns), "dead rows inside a live tile (at T = 16 a live tile is full: only whole waves are dead)"
    assert [16 - (16 // T) * T for T in k72.T_ALL] == [0, 1, 1, 5, 0]
    for n, T in k72.WIDE_CASES:
        assert -(-n // (16 // T)) == k72.WIDE_TILES + 1
    from d3il_amd import policies as P
    assert k72.WIDE_TILES == P.TRUNK72_WIDE_TILES
    assert all(-(-n // (16 // T)) < k72.WIDE_TILES for n, T in k72.ACC_CASES + k72.CHAIN_CASES + k72.DEEP_CASES)
    assert k72.CHAIN_CASES == [(6, 3), (3, 11)] and k72.DEEP_CASES == [(130, 3), (17, 11)]
    # ---- the attention scales do what ATT_SCALE says: sharp rows are nearly one-hot, flat rows nearly uniform
    for att, lo, hi in (("sharp", 0.5, 1.01), ("flat", 0.0, 0.2)):
        b = k72.blocks_of(12, 1, att)[0]
        xs = k72.rows_of(7, 9, 11).double()
        h = torch.nn.functional.layer_norm(xs, (72,), b.ln1.weight.double(), b.ln1.bias.double(), b.ln1.eps)
        q, k = (torch.nn.functional.linear(h, l.weight.double(), l.bias.double()).view(9, 11, 4, 18).transpose(1, 2) for l in (b.attn.query, b.attn.key))
        p = torch.softmax((q @ k.transpose(-2, -1))[:, :, -1, :] / 18 ** 0.5, dim=-1)      # the last query sees all 11 keys
        assert lo < float(p.max(dim=-1).values.median()) < hi, att
    # ---- the BeT margin cap holds for the f64 reference alone: at most 3 of 130 lanes per step lie within 1e-4 of a CDF edge
    b = pol72.BET
    _, ref = pol72.bet_policies(P, "cpu")
    obs = pol72.observations(b["obs_seed"], pol72.LANES, b["steps"], "cpu")
    left_out = []
    with torch.no_grad():
        for t in range(b["steps"]):
            logits, cdf, u, bins = pol72.bet_reference_step(ref, obs[:, t])
            left_out.append(int((~pol72.bet_far_lanes(cdf, u)).sum()))
            assert len(set(bins.tolist())) > 8, "the draw is neither uniform nor one-hot"
    assert max(left_out) <= b["max_left_out"], left_out
    assert ref.hist.len.tolist() == [b["window"]] * pol72.LANES
