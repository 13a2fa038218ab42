"""The rollout loops of the Sim classes: the one the xy-commanded tasks share (pushing_sim.py:69-84, sorting_sim.py:118-133: obs := desired xy || env obs, action := policy
delta + desired xy, frozen z and quaternion; what is recorded is ``info[...]`` of the step that returned ``done``), the joint-space loop of Stacking and the xyz loop of Aligning, run over the sub-batches of a
rank (envs/sub_batch.py): every sub-batch steps on its own stream with its own agent clone; the host looks at the ``finished`` flags every 16th
step only."""
from __future__ import annotations

import logging
import os

import torch

from ..envs.sub_batch import SubBatchSet

log = logging.getLogger(__name__)


class _Lanes:
    pass


class _PolicyRangeScope:
    """The range / NaN guard of the split-f16 policy kernels (policies.RangeGuard) around one rollout.  policy_range_guard: True = on, False = off, None = follow
    D3IL_POLICY_RANGE_GUARD.  On: the process's guard (or a new one) is enabled for the rollout and what it counted DURING the rollout is reported - per rank -
    together with the out-of-range weight entries of the agents that know them (BESOPolicy.weights_out_of_range); every non-zero counter is logged as a warning."""

    def __init__(self, policy_range_guard, dev):
        from .. import policies
        self.P = policies
        on = os.environ.get("D3IL_POLICY_RANGE_GUARD", "0") == "1" if policy_range_guard is None else bool(policy_range_guard)
        self.guard = self.suspended = self.before = None
        self.mine = False
        if os.environ.get("D3IL_POLICY_RANGE_GUARD", "0") == "1":
            policies._env_range_guard(dev)      # the environment's guard comes first: it outlives the rollout, a guard of this scope does not
        cur = policies.range_guard()
        if on:
            self.guard = cur if cur is not None else policies.RangeGuard(dev)
            self.mine = cur is None
            if self.mine:
                self.guard.enable()
            self.before = self.guard.read()
        elif policy_range_guard is not None and cur is not None:      # an explicit "off" holds against a guard the environment variable has switched on
            cur.disable()
            self.suspended = cur

    def restore(self):
        """The process's guard setting as it was before the rollout (idempotent)."""
        if self.suspended is not None:
            self.suspended.enable()
            self.suspended = None
        if self.mine and self.guard is not None and self.guard.enabled:
            self.guard.disable()

    def finish(self, agents):
        if self.guard is None:
            self.restore()
            return None
        now = self.guard.read()
        rep = {k: now[k] - self.before[k] for k in now}
        self.restore()
        seen, w = set(), 0
        for a in agents:
            pol = next((c for c in (a, getattr(a, "inner", None)) if callable(getattr(c, "weights_out_of_range", None))), None)      # (CapturedPolicy keeps its policy in .inner)
            if pol is not None and id(getattr(pol, "inner", pol)) not in seen:      # sub-batch clones share their network
                seen.add(id(getattr(pol, "inner", pol)))
                w += int(pol.weights_out_of_range())
        rep["weights_out_of_range"] = w
        for k in ("clipped", "nonfinite", "weights_out_of_range"):
            if rep[k]:
                log.warning("policy range guard: %s = %d (split-f16 policy kernels, csrc/policy_f16x3.h: operands beyond +-65504 saturate, NaN / Inf rows come out NaN)", k, rep[k])
        return rep


def xy_rollout(batches: SubBatchSet, max_steps: int, record: dict, predict=None, policy_range_guard=None):
    """record: {info key: (dtype, initial value)}.  Returns {key: tensor [n]} (sub-batch order = rollout order) plus 'flags' (the environments'
    flag words after the rollout) and 'policy_range' (the range guard's report, None when it is off).  predict(agent, obs_in) -> [n, 2] f64 (the Sim class's
    ``_predict`` hook)."""
    dev = batches.device
    if predict is None:
        def predict(agent, obs_in):
            return agent.predict_batch(obs_in).to(device=dev, dtype=torch.float64).reshape(obs_in.shape[0], 2)

    def begin(b):
        st = b.state = _Lanes()
        n = b.n
        st.quat = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=dev).expand(n, 4)
        st.finished = torch.zeros(n, dtype=torch.bool, device=dev)
        st.rec = {k: torch.full((n,), init, dtype=dt, device=dev) for k, (dt, init) in record.items()}
        pred_action = b.env.robot_state().clone()
        st.fixed_z = pred_action[:, 2:3].clone()
        st.des_xy = pred_action[:, :2].clone()
        st.obs = b.env.obs

    def step(b):
        st = b.state
        obs_in = torch.cat((st.des_xy, st.obs.to(torch.float64)), dim=1)
        delta = predict(b.agent, obs_in)
        des_new = delta + obs_in[:, :2]
        st.des_xy = torch.where(st.finished.unsqueeze(1), st.des_xy, des_new)
        action = torch.cat((st.des_xy, st.fixed_z, st.quat), dim=1).contiguous()
        st.obs, _, done, info = b.env.step(action)
        newly = ~st.finished & done.bool()
        for k in st.rec:
            st.rec[k] = torch.where(newly, info[k].to(st.rec[k].dtype), st.rec[k])
        st.finished |= done.bool()

    return _run(batches, max_steps, begin, step, record, policy_range_guard)


def _run(batches: SubBatchSet, max_steps: int, begin, step, record: dict, policy_range_guard=None):
    """The driver the rollout loops share: begin / step per sub-batch on its own stream, the host looks at the ``finished`` flags every 16th step."""
    dev = batches.device
    scope = _PolicyRangeScope(policy_range_guard, dev)
    try:
        batches.each(begin)
        for t in range(max_steps):
            batches.each(step)
            if t % 16 == 15:                                   # the only host synchronisation of the loop
                batches.join()
                if bool(torch.stack([b.state.finished.all() for b in batches]).all()):
                    break
        batches.join()
        torch.cuda.synchronize(dev)      # the tables below are read on the caller's stream; the sub-batch streams have nothing left in flight
        out = {k: torch.cat([b.state.rec[k] for b in batches]) for k in record}
        out["flags"] = torch.cat([b.env.flags[:b.n].clone() for b in batches])
        out["policy_range"] = scope.finish([b.agent for b in batches])
    finally:
        scope.restore()      # also when a step raised: no guard of this scope stays enabled, none it suspended stays off
    return out


def _record(st, done, info):
    newly = ~st.finished & done.bool()
    for k in st.rec:
        st.rec[k] = torch.where(newly, info[k].to(st.rec[k].dtype), st.rec[k])
    st.finished |= done.bool()


def _begin_lanes(b, record, dev):
    st = b.state = _Lanes()
    st.finished = torch.zeros(b.n, dtype=torch.bool, device=dev)
    st.rec = {k: torch.full((b.n,), init, dtype=dt, device=dev) for k, (dt, init) in record.items()}
    return st


def joint_rollout(batches: SubBatchSet, max_steps: int, record: dict, policy_range_guard=None):
    """Stacking (stacking_sim.py:88-109): the policy input is the LAST COMMAND (7 desired joint positions + gripper command, initially env.robot_state())
    concatenated with the env observation; its output is a joint-position delta plus the gripper command."""
    dev = batches.device

    def begin(b):
        st = _begin_lanes(b, record, dev)
        st.pred_action = b.env.robot_state().to(torch.float32)              # stacking_sim.py:90-91
        st.obs = b.env.obs

    def step(b):
        st = b.state
        obs20 = torch.cat((st.pred_action, st.obs), dim=1)                  # np.concatenate((pred_action, obs)), stacking_sim.py:99
        out = b.agent.predict_batch(obs20).to(device=dev, dtype=torch.float32).reshape(b.n, 8)
        new_action = torch.cat((out[:, :7] + obs20[:, :7], out[:, 7:8]), dim=1)   # pred_action[:7] += obs[:7], stacking_sim.py:104
        st.pred_action = torch.where(st.finished.unsqueeze(1), st.pred_action, new_action)
        st.obs, _, done, info = b.env.step(st.pred_action.to(torch.float64).contiguous())
        _record(st, done, info)

    return _run(batches, max_steps, begin, step, record, policy_range_guard)


def xyz_rollout(batches: SubBatchSet, max_steps: int, record: dict, predict, policy_range_guard=None):
    """Aligning (aligning_sim.py:96-108): obs := desired xyz || env obs, action := policy delta + desired xyz (the policy commands x, y AND z), frozen
    quaternion [0, 1, 0, 0].  predict(agent, obs20) -> [n, 3] f64."""
    dev = batches.device

    def begin(b):
        st = _begin_lanes(b, record, dev)
        st.quat = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=dev).expand(b.n, 4)
        st.des = b.env.robot_state().clone()                                  # pred_action = env.robot_state(), aligning_sim.py:96
        st.obs = b.env.obs

    def step(b):
        st = b.state
        obs20 = torch.cat((st.des, st.obs.to(torch.float64)), dim=1)         # np.concatenate((pred_action[:3], obs)), aligning_sim.py:99
        des_new = predict(b.agent, obs20) + obs20[:, :3]                       # aligning_sim.py:101-102
        st.des = torch.where(st.finished.unsqueeze(1), st.des, des_new)
        st.obs, _, done, info = b.env.step(torch.cat((st.des, st.quat), dim=1).contiguous())
        _record(st, done, info)

    return _run(batches, max_steps, begin, step, record, policy_range_guard)
