"""Link-near guard of the generic-engine tasks (Pushing, Sorting, Inserting): the environment side of ``d3il_set_link_guard``.

The engine collides the rod with the scene and nothing else of the robot; the guard raises ``capi.PFLAG_LINK_NEAR`` in an environment's
flag word when a bounding capsule of one of the robot's other collision hulls (``model/blobs/panda_link_capsules.json``) comes within
``margin`` of a cube or a static box at the end of an env step (csrc/link_guard.h).  The bit is per episode, like the divergence flags."""
from __future__ import annotations

import ctypes as C

import torch

from .. import capi


class LinkGuardMixin:
    """``link_guard=`` constructor keyword, ``set_link_guard`` and ``link_near_episodes`` of the generic-engine environments."""

    link_guard_margin = None

    def _init_link_guard(self, enabled: bool):
        self._lg_count = torch.zeros(1, dtype=torch.int64, device=self.device)      # device counter the guard kernel adds to
        self.link_guard = False
        if enabled:
            self.set_link_guard(True)

    def set_link_guard(self, enabled: bool = True, margin: float | None = None, capsules=None):
        """Switch the guard on (the committed capsules and margin unless given: ``capsules`` f64 [n, 9] as d3il_set_link_guard takes them) or off."""
        if not enabled:
            capi.set_link_guard(self.h, None, 0.0, None)
            self.link_guard = False
            return
        caps, default_margin = capi.link_capsules([b["name"] for b in self.js["bodies"]])
        if capsules is not None:
            caps = capsules
        self.link_guard_margin = float(default_margin if margin is None else margin)
        with torch.cuda.device(self.device):
            capi.set_link_guard(self.h, caps, self.link_guard_margin, C.c_void_p(self._lg_count.data_ptr()))
        self.link_guard = True

    @property
    def link_near_episodes(self) -> int:
        """Episodes of this environment batch that carried PFLAG_LINK_NEAR so far (reads the device counter: synchronises)."""
        return int(self._lg_count.item())

    def link_near(self) -> torch.Tensor:
        """bool [n_envs]: the bit of the running episodes."""
        return (self.flags[:self.n_envs] & capi.PFLAG_LINK_NEAR) != 0
