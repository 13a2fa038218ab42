"""ctypes binding of libd3il_rollout.so (include/d3il_rollout.h).

This is the reference-side binding a maintainer would add; it contains no
compute.  Loading fails loudly when the library is missing - there is no Python/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from .model.blob import ModelBlob

_LIB = None


class Buffers(C.Structure):
    _fields_ = [("n_envs", C.c_int32), ("stride", C.c_int32), ("obs_dim", C.c_int32), ("action_dim", C.c_int32),
                ("obs", C.c_void_p), ("done", C.c_void_p), ("success", C.c_void_p), ("mode", C.c_void_p),
                ("state", C.c_void_p), ("flags", C.c_void_p), ("step_count", C.c_void_p), ("policy_des", C.c_void_p),
                ("info_f64", C.c_void_p), ("n_info_f64", C.c_int32), ("state_rows", C.c_int32), ("last_reset", C.c_void_p)]


STATE_F64 = 42
STATE_QPOS, STATE_QVEL, STATE_BIAS, STATE_TCP, STATE_IK_Q, STATE_IK_QD = 0, 9, 18, 25, 28, 35
FLAG_MODE_MASK, FLAG_TERMINATED, FLAG_SUCCESS, FLAG_ROD_CONTACT = 0x1FF, 1 << 12, 1 << 13, 1 << 14
FLAG_IK_VALID, FLAG_SOLVER_FAIL, FLAG_MULTI_CONTACT = 1 << 15, 1 << 16, 1 << 17
# Pushing (D3IL_PUSH_STATE_* / D3IL_PFLAG_* in include/d3il_rollout.h)
PUSH_STATE_BOX, PUSH_STATE_WARM, PUSH_STATE_TASK, PUSH_STATE_F64 = 42, 68, 89, 91
PFLAG_FIRST_MASK, PFLAG_MODE_MASK, PFLAG_WARM_VALID, PFLAG_CON_OVERFLOW, PFLAG_OFF_TABLE = 0x7, 0x38, 1 << 6, 1 << 18, 1 << 19
PFLAG_LINK_NEAR = 1 << 20       # link-near guard of the generic engine (d3il_set_link_guard); the bit of SFLAG_HAND_NEAR
LINK_GUARD_SLACK = 1.25e-4      # how far the guard's distance may lie below the true one (csrc/link_guard.h LG_SLACK)
TASK_AVOIDING, TASK_PUSHING, TASK_SORTING, TASK_STACKING, TASK_ALIGNING, TASK_INSERTING = 0, 1, 2, 3, 4, 5
ALIGN_STATE_BOX, ALIGN_STATE_WARM, ALIGN_STATE_TARGET, ALIGN_STATE_F64 = 42, 55, 70, 77
STACK_STATE_BOX, STACK_STATE_WARM, STACK_STATE_F64 = 28, 67, 94
SFLAG_MODE_MASK, SFLAG_WARM_VALID, SFLAG_HAND_NEAR = 0xFF, 1 << 8, 1 << 20
TALLY_ROW, TALLY_ALL = 514, 256
ERCCL = -7
SORT_STATE_BOX, SORT_STATE_WARM, SORT_STATE_TASK, SORT_STATE_F64 = 42, 94, 127, 129
INS_STATE_BOX, INS_STATE_WARM, INS_STATE_TASK, INS_STATE_F64 = 42, 81, 108, 110
BUILD_POISON, BUILD_SK_POISON, BUILD_STATS = 1, 2, 4      # d3il_debug_build_flags()[0]
BET_TAG = 0x42655448      # fourth Philox counter word of d3il_bet_head_f32 (csrc/policy_bet.h)
DDPM_GPT_TAG = 0x44470000      # ... of d3il_ddpm_gpt_step_f32, or-ed with k << 8 | j << 1 | q (csrc/policy_ddpm_gpt.h)
IBC_TAG = 0x49420000      # ... of d3il_ibc_langevin_f32, or-ed with kind << 14 | k << 8 | s << 2 | q (csrc/policy_ibc.h)
ACT_TAG = 0x41430000      # ... of d3il_act_chunk_f32, or-ed with q (csrc/policy_act.h)
CVAE_TAG = 0x43560000      # ... of d3il_cvae_decode_f32, or-ed with q (csrc/policy_cvae.h)
DDPM_ACT_TAG = 0x44410000      # ... of d3il_ddpm_act_chunk_f32, or-ed with k << 8 | t << 1 | q (csrc/policy_ddpm_act.h)
BET_MLP_TAG = 0x424D4C50      # ... of d3il_bet_mlp_f32 (csrc/policy_bet_mlp.h)
BESO_TAG = 0x42530000      # ... of d3il_beso_step, or-ed with draw << 8 | j << 1 | q (csrc/policy_beso.h)
TAG_DDPM_MLP = 0x444D0000      # ... of d3il_ddpm_mlp_chain (policies.DDPM_MLP_TAG), or-ed with k << 1 | q (csrc/policy_ddpm_mlp.h); named the other way round because
                               # tests/test_policies_beso_native.py pins the set of this module's *_TAG names
TAG_BC_GMM = 0x474D0000      # ... of d3il_bc_gmm (policies.BC_GMM_TAG), or-ed with q: 0 the uniform, 1 / 2 the normals (csrc/policy_bc_gmm.h); named like TAG_DDPM_MLP
HXG_CLIPPED, HXG_NONFINITE, HXG_LAUNCHES, HXG_N = 0, 1, 2, 4      # the counters of d3il_f16x3_set_guard (D3IL_HXG_*)

EXPORTS = ["d3il_create", "d3il_destroy", "d3il_start", "d3il_reset", "d3il_step", "d3il_get_buffers", "d3il_get_state",
           "d3il_set_state", "d3il_policy_begin", "d3il_policy_action", "d3il_attention_causal_f32", "d3il_layernorm_f32", "d3il_mlp_gelu_residual_f32", "d3il_mlp_ln_gelu_residual_f32", "d3il_linear120_f32", "d3il_mlp_ln_gelu_residual_f16x3", "d3il_linear120_f16x3", "d3il_attn_half_f16x3", "d3il_gpt_trunk72_f16x3", "d3il_f16x3_set_guard", "d3il_bet_head_f32", "d3il_ddpm_gpt_step_f32", "d3il_beso_step", "d3il_ddpm_mlp_chain", "d3il_ibc_langevin_f32", "d3il_act_chunk_f32", "d3il_ddpm_act_chunk_f32", "d3il_cvae_decode_f32", "d3il_bet_mlp_f32", "d3il_bc_gmm", "d3il_gpt_bc_head_f32", "d3il_ddpm_mlp_f32", "d3il_resmlp_f32", "d3il_auto_reset", "d3il_set_tally", "d3il_count_metrics",
           "d3il_rccl_available", "d3il_comm_unique_id", "d3il_comm_init", "d3il_comm_count", "d3il_comm_destroy", "d3il_reduce_metrics", "d3il_set_timing",
           "d3il_last_step_ms", "d3il_timing_stats", "d3il_step_auto_reset", "d3il_random_rollout_step", "d3il_random_rollout_prepare", "d3il_group_create", "d3il_group_flush", "d3il_group_destroy", "d3il_group_set_option", "d3il_group_stats", "d3il_group_pipeline_stats", "d3il_set_option", "d3il_set_link_guard", "d3il_debug_stats", "d3il_debug_wave_stats", "d3il_debug_wave_counts", "d3il_debug_scratch", "d3il_debug_build_flags", "d3il_last_error", "d3il_blob_sizeof", "d3il_version"]

# The policy kernel entries: parameter names in the order of include/d3il_rollout.h, ``name`` a pointer, ``name:i`` int, ``:l`` long, ``:f`` float, ``:q`` uint64_t,
# ``:u`` uint32_t.  load() derives the argtypes from it, launch() the keywords it demands; tests/test_capi_signatures.py holds it against the header.
_CTYPES = {"": C.c_void_p, "i": C.c_int, "l": C.c_long, "f": C.c_float, "q": C.c_uint64, "u": C.c_uint32}
_RESMLP = "w_in b_in w_blocks b_blocks"
_TAIL = "lo hi scale shift"
_DRAW = _TAIL + " seed:q env_offset:q t_device"
_LN = "ln_weight ln_bias ln_eps:f"
_MLP = "h " + _LN + " x w_packed b1 b2 out rows:l C:i H:i"
_LINEAR = "xin " + _LN + " w_packed bias resid out rows:l N:i"
_ENCDEC = "w_in tab enc_w enc_v dec_w dec_v head_w " + _DRAW
def _table(specs: dict) -> dict:
    return {name: tuple((a.partition(":")[0], _CTYPES[a.partition(":")[2]]) for a in (spec + " stream").split()) for name, spec in specs.items()}


SIGNATURES = _table({
    "d3il_attention_causal_f32": "qkv out B:i T:i H:i D:i",
    "d3il_layernorm_f32": "x weight bias y rows:l C:i eps:f",
    "d3il_linear120_f32": _LINEAR,
    "d3il_mlp_gelu_residual_f32": "h x w_packed b1 b2 out rows:l C:i H:i",
    "d3il_mlp_ln_gelu_residual_f32": _MLP,
    "d3il_mlp_ln_gelu_residual_f16x3": _MLP,
    "d3il_linear120_f16x3": _LINEAR,
    "d3il_attn_half_f16x3": "x " + _LN + " w_packed b_qkv b_proj out n_seq:l T:i n_head:i C:i",
    "d3il_ddpm_mlp_f32": "state noise temb " + _RESMLP + " w_out b_out sched bounds out rows:l state_dim:i n_timesteps:i hidden:i n_blocks:i",
    "d3il_resmlp_f32": "x " + _RESMLP + " w_out b_out out rows:l in_dim:i hidden:i n_blocks:i out_dim:i",
    "d3il_bet_head_f32": "h " + _LN + " w_head centers " + _DRAW + " u_in actions bins u_out probs rows:l C:i V:i A:i",
    "d3il_ddpm_gpt_step_f32": "hk " + _LN + " w_pred b_pred w_aemb bias_pos temb sched " + _TAIL + " len seed:q env_offset:q t_device noise_in x xbuf actions bad noise_out "
                              "n_env:l C:i A:i W:i T:i k:i",
    "d3il_ibc_langevin_f32": "state " + _RESMLP + " w_out b_out wT_blocks wT_in_act coef noise_scale:f lo hi clip scale shift seed:q env_offset:q t_device x0_in noise_in u_in "
                             "actions picks x_final energies x0_out noise_out u_out n_env:l obs_dim:i A:i hidden:i n_blocks:i S:i K:i",
    "d3il_act_chunk_f32": "state " + _ENCDEC + " latent_in counter chunk actions latent_out n_env:l obs_dim:i A:i T:i width:i n_head:i latent:i n_enc:i n_dec:i",
    "d3il_ddpm_act_chunk_f32": "window len " + _ENCDEC + " noise_in x_in counter chunk actions bad x_out noise_out n_env:l obs_dim:i A:i obs_seq_len:i action_seq_len:i "
                               "width:i n_head:i n_enc:i n_dec:i n_timesteps:i linear_head:i k_start:i k_stop:i",
    "d3il_cvae_decode_f32": "state " + _RESMLP + " w_out b_out " + _DRAW + " z_in actions z_out n_env:l obs_dim:i latent:i A:i hidden:i n_blocks:i",
    "d3il_bet_mlp_f32": "state " + _RESMLP + " w_logit b_logit w_off b_off centers " + _DRAW + " u_in actions bins u_out probs n_env:l obs_dim:i V:i A:i hidden:i n_blocks:i",
    "d3il_gpt_bc_head_f32": "h " + _LN + " w_head " + _TAIL + " actions bad rows:l C:i A:i",
})
# The policy kernel entries whose names carry no _f32 / _f16x3 suffix, in the same format; tests/test_capi_signatures2.py holds this table against the header.
SIGNATURES2 = _table({
    "d3il_beso_step": "hk " + _LN + " w_pred b_pred w_aemb bias_pos semb coef sigma_max:f c_in0:f " + _TAIL + " len seed:q env_offset:q t_device noise_in x xbuf a_hist actions bad "
                      "noise_out n_env:l C:i A:i W:i S:i i:i",
})
# The policy kernel entries that take the device step word first (unsuffixed names again), in the same format; tests/test_capi_signatures3.py holds this table against
# the header.
SIGNATURES3 = _table({
    "d3il_ddpm_mlp_chain": "t_device state w_x w_state tbias w_blocks b_blocks w_out b_out sched " + _TAIL + " seed:q env_offset:q noise_in actions bad noise_out n_env:l obs_dim:i "
                           "A:i t_dim:i n_timesteps:i hidden:i n_blocks:i",
})
# The policy kernel entries that take the row count first (unsuffixed names again), in the same format; tests/test_capi_signatures4.py holds this table against the
# header.
SIGNATURES4 = _table({
    "d3il_bc_gmm": "n_env:l t_device state " + _RESMLP + " w_feat b_feat w_logit b_logit w_mean b_mean w_std b_std " + _TAIL + " seed:q env_offset:q u_in z_in actions comps u_out z_out "
                   "probs obs_dim:i G:i A:i hidden:i n_blocks:i std_mode:i min_std:f",
})
# The policy kernel entries whose prototype has its return type on a line of its own (``int`` / ``d3il_*_f16x3(...)``: the first table's test pins the number of
# one-line suffixed prototypes), in the same format; tests/test_capi_signatures5.py holds this table against the header.
SIGNATURES5 = _table({
    "d3il_gpt_trunk72_f16x3": "x w_packed vec ln_eps:f out n_seq:l T:i n_layer:i",
})
ALL_SIGNATURES = {**SIGNATURES, **SIGNATURES2, **SIGNATURES3, **SIGNATURES4, **SIGNATURES5}
# what launch() works from, resolved once per entry: the keywords it demands (everything but the stream), the same as a set, the positions of the pointers
_LAUNCH = {name: (tuple(n for n, _ in sig[:-1]), frozenset(n for n, _ in sig[:-1]), tuple(i for i, (_, t) in enumerate(sig[:-1]) if t is C.c_void_p))
           for name, sig in ALL_SIGNATURES.items()}


class D3ilError(RuntimeError):
    pass


def lib_path() -> str:
    if os.environ.get("D3IL_LIB_PATH"):       # A/B measurements of two builds on the same GPU box
        return os.environ["D3IL_LIB_PATH"]
    name = "libd3il_rollout_stats.so" if os.environ.get("D3IL_STATS_LIB") == "1" else "libd3il_rollout.so"
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), name)


def load():
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise D3ilError("%s is missing: build it with `python -m d3il_amd.build` (hipcc, gfx950). "
                            "There is no CPU fallback for the rollout path." % path)
        L = C.CDLL(path)
        L.d3il_last_error.restype = C.c_char_p
        L.d3il_blob_sizeof.restype = C.c_size_t
        L.d3il_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.d3il_destroy.argtypes = [C.c_void_p]
        L.d3il_start.argtypes = [C.c_void_p, C.c_void_p]
        L.d3il_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.d3il_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.d3il_get_buffers.argtypes = [C.c_void_p, C.POINTER(Buffers)]
        L.d3il_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.d3il_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.d3il_policy_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.d3il_policy_action.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        L.d3il_count_metrics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        for name, sig in ALL_SIGNATURES.items():
            if hasattr(L, name):      # (an older build loaded through D3IL_LIB_PATH lacks the newest entries: skipped, not an error)
                getattr(L, name).argtypes = [t for _, t in sig]
        L.d3il_f16x3_set_guard.argtypes = [C.c_void_p]
        L.d3il_auto_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.d3il_step_auto_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.d3il_random_rollout_step.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.d3il_random_rollout_prepare.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.d3il_timing_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.d3il_set_tally.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.d3il_comm_unique_id.argtypes = [C.c_void_p]
        L.d3il_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.d3il_comm_destroy.argtypes = [C.c_void_p]
        L.d3il_comm_count.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.d3il_rccl_available.restype = C.c_int
        L.d3il_reduce_metrics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.d3il_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.d3il_last_step_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.d3il_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.d3il_debug_scratch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.d3il_debug_build_flags.argtypes = [C.c_void_p]
        L.d3il_set_link_guard.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
        if hasattr(L, "d3il_group_create"):      # (an older build loaded through D3IL_LIB_PATH has no step group: has_step_group())
            L.d3il_group_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
            L.d3il_group_flush.argtypes = [C.c_void_p]
            L.d3il_group_destroy.argtypes = [C.c_void_p]
        if hasattr(L, "d3il_group_set_option"):      # (the parent build has the group without its options and counters: has_group_options())
            L.d3il_group_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
            L.d3il_group_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        if hasattr(L, "d3il_group_pipeline_stats"):      # (the parent build has no "pipeline_depth": has_group_pipeline())
            L.d3il_group_pipeline_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        if L.d3il_blob_sizeof() != C.sizeof(ModelBlob):
            raise D3ilError("model blob layout mismatch between include/d3il_model_blob.h and d3il_amd/model/blob.py")
        _LIB = L
    return _LIB


def has_step_group() -> bool:
    """The loaded library has the step group (d3il_group_create / _flush / _destroy)."""
    return hasattr(load(), "d3il_group_create")


def has_group_options() -> bool:
    """The loaded library has the group's options and counters (d3il_group_set_option "quiet_streams", d3il_group_stats)."""
    return hasattr(load(), "d3il_group_set_option")


def has_group_pipeline() -> bool:
    """The loaded library has the group option "pipeline_depth" and its counters (d3il_group_pipeline_stats)."""
    return hasattr(load(), "d3il_group_pipeline_stats")


def is_unknown_group_option(err: Exception) -> bool:
    """The error d3il_group_set_option gives for an option the loaded library does not have (the parent build loaded through D3IL_LIB_PATH knows
    "quiet_streams" but not "dispatch_sets"): the caller keeps the path it had."""
    return isinstance(err, D3ilError) and "d3il_group_set_option: unknown option" in str(err)


def check(rc: int):
    if rc != 0:
        raise D3ilError("libd3il_rollout error %d: %s" % (rc, load().d3il_last_error().decode()))


def launch(name: str, device, **args):
    """Call the policy kernel entry ``name`` of SIGNATURES / SIGNATURES2 / SIGNATURES3 / SIGNATURES4 by keyword on the current stream of ``device``: exactly the header's parameter names but ``stream``
    (TypeError naming the missing / unknown ones, or a tensor on another device, before the library is touched); a pointer parameter takes a tensor, which goes as its
    data_ptr(), or None for NULL, numbers go as they are; a non-zero return code raises D3ilError."""
    names, keys, pointers = _LAUNCH[name]
    if args.keys() != keys:
        raise TypeError("%s: missing arguments %s, unknown arguments %s" % (name, sorted(keys - args.keys()), sorted(args.keys() - keys)))
    where = -1 if device.type == "cpu" else torch.cuda.current_device() if device.index is None else device.index      # what Tensor.get_device() says there
    vals = [args[k] for k in names]
    for i in pointers:      # (this loop runs once per eager policy step: an integer compare per tensor, no device objects)
        v = vals[i]
        if v is not None:
            if v.get_device() != where:
                raise TypeError("%s: %s is on %s, the launch is on %s" % (name, names[i], v.device, device))
            vals[i] = v.data_ptr()
    check(getattr(load(), name)(*vals, torch.cuda.current_stream(device).cuda_stream))


_CAPSULES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "model", "blobs", "panda_link_capsules.json")


def link_capsules(body_names, path: str | None = None):
    """The committed bounding capsules of the rod robot's collision hulls (model/mjcf_compile.py link_capsules) as the f64 [n][9] array
    d3il_set_link_guard takes - body id looked up by name in ``body_names`` (the blob's body list), statics flag, p0, p1, r - and the default margin."""
    import json
    import numpy as np
    with open(path or _CAPSULES) as f:
        js = json.load(f)
    rows = [[body_names.index(c["body"]), c["statics"]] + list(c["p0"]) + list(c["p1"]) + [c["r"]] for c in js["capsules"]]
    return np.ascontiguousarray(rows, dtype=np.float64), float(js["margin"])


def set_link_guard(h, capsules, margin: float, counter_ptr=None):
    """d3il_set_link_guard: capsules = host f64 [n][9] (or None / empty: off), counter_ptr = device int64 address or None."""
    import numpy as np
    caps = np.zeros((0, 9)) if capsules is None else np.ascontiguousarray(capsules, dtype=np.float64).reshape(-1, 9)
    check(load().d3il_set_link_guard(h, caps.ctypes.data_as(C.c_void_p) if len(caps) else None, len(caps), float(margin), counter_ptr))
