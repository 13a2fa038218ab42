"""Sub-batches: a process's environments stepped as S independent environment batches on S HIP streams.

The reference spreads an evaluation over ``n_cores`` worker processes, each stepping its own slice of the contexts / rollouts
(simulation/avoiding_sim.py:87-124, pushing_sim.py:129-165, sorting_sim.py:160-189: ``mp.Process`` per core, shared result tables).
The counterpart on one GPU: the rollouts of a rank are cut into S contiguous sub-batches; each owns an environment handle
(its own state buffers, tally and kernel launches), a HIP stream and a clone of the agent's per-episode state.  A step launch lasts as
long as its slowest workgroup, and launches of different streams overlap - sub-batch B's physics runs while sub-batch A's policy does
(DESIGN section 18.10).  Rollouts are independent of each other, so for a policy that computes every row from that row alone (deterministic, or seeded
per rollout) the integer result tables are those of one batch (tests/test_subbatch_sims.py); a policy that draws from the process-wide torch generator
(DDPMPolicy and the older BESOPolicy: torch.randn per predict call) draws in another order per sub-batch - the same distribution, not the same table.
BESO on the Philox stream is policies.BESONativePolicy: its noise is keyed by the global rollout index and its tables do not depend on the cut.

Used by the Sim classes (``n_sub_batches=``) and by ``bench.py`` (``--sub-batches``).
"""
from __future__ import annotations

import copy
import os
import warnings

import torch

MIN_ENVS = 64          # one wavefront of environments: below that a sub-batch only adds launches
DEFAULT_HW_QUEUES = 4   # what the HIP runtime maps streams onto when GPU_MAX_HW_QUEUES is not set
MAX_CONCURRENT = 4     # dispatches of different streams the MI355X runs side by side (measured: 8 / 16 / 32 sub-batches of the contact tasks take 2 / 4 / 8 rounds of
                       # four - Pushing contact regime 7.6 / 18.0 / 27.5 / 46.5 ms per step at S = 4 / 8 / 16 / 32 although all 256 workgroups would fit the chip and
                       # GPU_MAX_HW_QUEUES was raised; profiles/r05/subbatch_sweep/): more sub-batches than this only add launches
CUS = 256              # MI355X: the Avoiding kernel's third ("serve") wave pays while the GPU holds at most one workgroup per CU


def plan(n: int, n_sub_batches: int, min_envs: int = MIN_ENVS):
    """[(offset, count)] of at most ``n_sub_batches`` contiguous sub-batches of ``n`` environments, every one at least ``min_envs`` wide
    (fewer sub-batches when n is small), sizes differing by at most one."""
    s = max(1, min(int(n_sub_batches), n // min_envs if n >= min_envs else 1))
    base, extra = divmod(n, s)
    out, off = [], 0
    for i in range(s):
        c = base + (1 if i < extra else 0)
        out.append((off, c))
        off += c
    return out


def ensure_hw_queues(n_streams: int):
    """Streams only overlap when the runtime gives them hardware queues of their own: ``GPU_MAX_HW_QUEUES`` (read once, when HIP initialises)
    must be >= the number of sub-batches.  Before initialisation the variable is raised; afterwards a too small value is reported."""
    cur = os.environ.get("GPU_MAX_HW_QUEUES")
    have = int(cur) if cur and cur.isdigit() else DEFAULT_HW_QUEUES
    if have >= n_streams:
        return have
    if not torch.cuda.is_initialized():
        os.environ["GPU_MAX_HW_QUEUES"] = str(n_streams)
        return n_streams
    warnings.warn("%d sub-batches but GPU_MAX_HW_QUEUES = %d was fixed when HIP initialised: their streams share hardware queues and will not fully "
                  "overlap (export GPU_MAX_HW_QUEUES=%d before the first GPU call)" % (n_streams, have, n_streams))
    return have


def fork_agent(agent):
    """A clone of a batched agent for one sub-batch: networks, scalers and everything immutable are shared, per-episode state (history deques,
    action-chunk buffers, non-parameter tensors; agents.RowwiseAgent's rule) is copied - the sub-batches call ``predict_batch`` in turn and must not
    see each other's histories.  Agents that know better provide ``fork()``."""
    if hasattr(agent, "fork"):
        return agent.fork()
    from ..agents import _is_lane_state
    c = copy.copy(agent)
    for k, v in list(vars(agent).items()):
        if k.startswith("_parameters") or k.startswith("_modules") or k.startswith("_buffers"):
            continue                      # torch.nn.Module internals stay shared
        if _is_lane_state(v):
            setattr(c, k, copy.deepcopy(v))
    return c


class SubBatch:
    """One sub-batch: offset / count inside the rank's rollout range, its environment, stream and agent clone."""
    __slots__ = ("index", "offset", "n", "env", "stream", "own_stream", "agent", "state")

    def __init__(self, index, offset, n, env, stream, own_stream):
        self.index, self.offset, self.n, self.env, self.stream, self.own_stream = index, offset, n, env, stream, own_stream
        self.agent, self.state = None, None


class SubBatchSet:
    """Owns the S environment handles and streams of a rank.

    make_env(count, offset) -> environment (constructed under the sub-batch's stream; the set then binds the stream to the handle, so every library
    call of that environment - step, reset, auto-reset, tally - is launched on it without a stream context per call).

    THE RULE when the set has formed a step group (``self.group``; Avoiding with fewer hardware queues than streams): the group runs with the library's
    ``quiet_streams`` option, so between two ``random_rollout_step`` rounds the caller queues nothing on the sub-batch streams that reads or writes what the
    step touches (the environments' buffers, ``actions``, episode counters, tally) - except on the first stream of each set, or after ``join()``.
    (A group of four or more sub-batches is cut into two dispatch sets, ``_step_group``: the first stream of a set is that of its first sub-batch, and it
    stays ordered for what the sub-batches of ITS set touch - the other set launches elsewhere, possibly steps ahead or behind.)
    ``join()`` flushes the group, which re-arms the library's join of the streams: torch work queued on any sub-batch stream before ``join()`` is ordered
    before the next round, work queued after a round sees that round.  Library calls on an environment (reset, get_state, options, timing) re-arm by
    themselves.  Without a group every stream is ordered as usual.

    A group whose rounds are PIPELINED (``_step_group``: the library's ``pipeline_depth`` option; ``group.pipeline_stats()`` says whether
    rounds were) has no exception: consecutive rounds are in flight on several sub-batch streams at once, and between two rounds of a running sequence NO
    sub-batch stream - the first included - is ordered with respect to what the step touches.  ``join()`` (the flush ends the sequence and puts every
    sub-batch stream behind its last round), any other library call on an environment, or a device synchronisation (``torch.cuda.synchronize()``)
    restores the order; read results behind one of them.
    """

    def __init__(self, n: int, n_sub_batches: int, device, make_env, min_envs: int = MIN_ENVS):
        self.device = torch.device(device)
        self.parts = plan(n, n_sub_batches, min_envs)
        self.n = n
        S = len(self.parts)
        hw_queues = ensure_hw_queues(S) if S > 1 else DEFAULT_HW_QUEUES
        self.group = None
        if S > MAX_CONCURRENT:
            warnings.warn("%d sub-batches: the GPU runs %d dispatches of different streams at a time, the others wait their turn (DESIGN section 19.6)" % (S, MAX_CONCURRENT))
        self.default_stream = torch.cuda.current_stream(self.device)
        self.batches = []
        for i, (off, cnt) in enumerate(self.parts):
            own = S > 1
            stream = torch.cuda.Stream(self.device) if own else self.default_stream
            with torch.cuda.stream(stream):
                env = make_env(cnt, off)
                if own:
                    env.bind_stream(stream)
                # Avoiding: the serve wave is taken while the whole GPU holds at most one workgroup per CU - the library sees one sub-batch, the set all
                if own and hasattr(env, "set_option") and type(env).__name__ == "ObstacleAvoidanceVecEnv":
                    env.set_option("serve_wave_max_workgroups", CUS // S)
            self.batches.append(SubBatch(i, off, cnt, env, stream, own))
        if S > 1:
            for b in self.batches:      # set-up work of the sub-batch streams is ordered before whatever the caller does next on its stream
                self.default_stream.wait_stream(b.stream)
            self.group = self._step_group(hw_queues)

    def _step_group(self, hw_queues: int):
        """Avoiding: with fewer hardware queues than the S streams and the null stream need, two sub-batches share a queue and their step launches run one after
        the other; the library then sends the ``random_rollout_step`` calls of one step as ONE dispatch (a step group).  With a queue per
        stream nothing is grouped.  ``D3IL_STEP_GROUP=0|1`` overrides the choice (A/B runs).  The group runs with ``quiet_streams`` (the
        rule is in the class docstring) where the library has the option.

        A group of four or more members, an even count, is cut into TWO dispatch sets (option ``dispatch_sets``) when the process has at
        least three hardware queues: the first half launches on the first sub-batch's stream, the second half on the stream of its own first sub-batch, and
        neither waits for the other's slowest workgroup.  With two queues (one of them the null stream's) both leaders would share one, and the halves would
        run one after the other.  ``D3IL_STEP_GROUP_SETS=1|2`` overrides the choice (A/B runs); a library without the option keeps one set.

        Where the library can pipeline the rounds (below), that comes first and the group keeps one set; the two sets are what is left for a library
        without ``pipeline_depth`` (it answers "unknown option"), for fewer than three hardware queues and for a group too large to stay resident."""
        envs = [b.env for b in self.batches]
        want = hw_queues < len(envs) + 1
        if os.environ.get("D3IL_STEP_GROUP") in ("0", "1"):
            want = os.environ["D3IL_STEP_GROUP"] == "1"
        if not want or not all(type(e).__name__ == "ObstacleAvoidanceVecEnv" for e in envs):
            return None
        from .avoiding import StepGroup
        from .. import capi
        if len(envs) > StepGroup.MAX_MEMBERS or not capi.has_step_group():      # (an older library loaded through D3IL_LIB_PATH: today's path)
            return None
        group = StepGroup(envs, quiet_streams=capi.has_group_options())
        # Pipelined rounds (option ``pipeline_depth``) where the library has them and the whole group, D rounds deep, stays resident
        # with one workgroup per CU: D = min(3, members, hardware queues - 1 (the null stream's), CUs // workgroups of the group).  The group then keeps ONE
        # dispatch set - depth and two sets together need more queues than there are.  ``D3IL_STEP_GROUP_PIPE=0|2|3`` overrides the choice (A/B runs).
        wgs = sum((b.n + MIN_ENVS - 1) // MIN_ENVS for b in self.batches)
        depth = min(3, len(envs), hw_queues - 1, CUS // max(1, wgs))
        # An explicit ``D3IL_STEP_GROUP_SETS`` without it asks for that form of dispatch sets, unpipelined.
        if os.environ.get("D3IL_STEP_GROUP_PIPE") in ("0", "2", "3"):
            depth = int(os.environ["D3IL_STEP_GROUP_PIPE"])
        elif os.environ.get("D3IL_STEP_GROUP_SETS") in ("1", "2"):
            depth = 1
        if depth >= 2 and capi.has_group_pipeline() and group.try_option("pipeline_depth", depth):
            return group
        sets = 2 if len(envs) >= 4 and len(envs) % 2 == 0 and hw_queues >= 3 else 1
        if os.environ.get("D3IL_STEP_GROUP_SETS") in ("1", "2"):
            sets = int(os.environ["D3IL_STEP_GROUP_SETS"])
        if sets != 1 and sets <= len(envs):
            group.try_option("dispatch_sets", sets)      # (False: the library has no dispatch sets - one dispatch per step, as before)
        return group

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)

    def each(self, fn):
        """fn(sub_batch) for every sub-batch with torch's current stream set to the sub-batch's (the policy's torch kernels go there); the caller's
        stream is restored afterwards.  Under a step group (class docstring): torch work that fn queues on a sub-batch stream and that touches what the
        Avoiding rollout step touches needs a ``join()`` before the next round."""
        if len(self.batches) == 1:
            fn(self.batches[0])
            return
        try:
            for b in self.batches:
                torch.cuda.set_stream(b.stream)
                fn(b)
        finally:      # also when fn raises (a library error, an assert inside a policy): the process must not stay on a sub-batch stream
            torch.cuda.set_stream(self.default_stream)

    def join(self):
        """The caller's stream waits for everything queued on the sub-batch streams (no host synchronisation).  The set's synchronisation point: under a
        step group it also re-arms the group, so the next round is ordered behind what the sub-batch streams hold by then."""
        if self.group is not None:
            self.group.flush()      # a round that not every sub-batch has joined goes out now; the next merged round joins the streams again
        if len(self.batches) > 1:
            for b in self.batches:
                self.default_stream.wait_stream(b.stream)

    def fork_agents(self, agent):
        """Per-sub-batch agent clones (one sub-batch: the agent itself).  An agent that wants to know which rollouts its rows are (per-rollout seeds,
        goals) implements ``set_rollout_range(offset, count)``: rows 0 .. count-1 of its batch are rollouts offset .. offset+count-1 of the rank."""
        from ..agents import as_batched
        for b in self.batches:
            a = agent if len(self.batches) == 1 else fork_agent(agent)
            if hasattr(a, "set_rollout_range"):
                a.set_rollout_range(b.offset, b.n)
            b.agent = as_batched(a, b.n)
            if b.agent is not a and hasattr(b.agent, "set_rollout_range"):      # an adapter built from a reference agent (policies.BeTPolicy.from_reference)
                b.agent.set_rollout_range(b.offset, b.n)
            b.agent.reset()
        if len(self.batches) > 1:      # the clones' device state (step word, histories, tables) was written on the caller's stream: the sub-batch streams go on behind it
            cur = torch.cuda.current_stream(self.device)
            for b in self.batches:
                if b.own_stream:
                    b.stream.wait_stream(cur)

    @property
    def link_near_episodes(self) -> int:
        """Episodes flagged by the link-near guard, summed over the sub-batches (0 for tasks without the guard)."""
        return sum(int(getattr(b.env, "link_near_episodes", 0)) for b in self.batches if b.env is not None)

    def close(self):
        if self.group is not None:
            self.group.close()
            self.group = None
        for b in self.batches:
            if b.env is not None:
                b.env.close()
                b.env = None
