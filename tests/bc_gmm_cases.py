"""What tests/test_policies_bc_gmm.py (CPU) and tests/test_gpu_bc_gmm.py share: the random-weight cases of the BC-GMM kernel tests with their f64 restatement
(policies.BCGMMPolicy._predict_torch on a double copy of the network), a bank of uniforms that keeps BC_GMM_EDGE from every edge of the f64 CDF, a bank of normals,
and the constants of the launch whose uniform is drawn on the device - chosen on the CPU, with the host Philox and the f64 restatement, so that the reference alone
leaves at most DRAWN_CAP of the 257 rows within EDGE of an edge."""
import copy

import torch

from d3il_amd import policies as P

N = 257      # 16 full tiles and one row
# name: (hidden, residual blocks, obs, action components, mixture components, std mode, bounds in scaled space)
CASES = {"h128b0_o1a1g1_low": (128, 0, 1, 1, 1, "low_noise", 0.004),
         "h128b3_o4a2g8_low": (128, 3, 4, 2, 8, "low_noise", 0.004),      # the avoiding script's shape
         "h256b3_o20a3g17_exp": (256, 3, 20, 3, 17, "exp", 0.5),
         "h128b3_o28a8g24_softplus": (128, 3, 28, 8, 24, "softplus", 0.5),
         "h256b0_o28a8g64_exp": (256, 0, 28, 8, 64, "exp", 0.5),
         "h128b3_o20a3g64_low": (128, 3, 20, 3, 64, "low_noise", 0.004)}
# the device-drawn launch (case h256b0_o28a8g64_exp): 64 edges x 2e-4 = 1.3 % of the rows are expected within EDGE of an edge; these constants give DRAWN_NEAR
DRAWN_CASE, DRAWN_SEED, DRAWN_T, DRAWN_OFFSET, DRAWN_CAP, DRAWN_NEAR = "h256b0_o28a8g64_exp", 0x1234567890ABCDEF, 0x80000007, (1 << 32) + 1000, 4, 3
_CACHE = {}


class Case:
    def __init__(self, name, tweak=None):
        self.name = name
        self.hidden, self.nblk, self.obs, self.A, self.G, self.std, bound = CASES[name]
        i = list(CASES).index(name)
        low = self.std == "low_noise"
        self.pol = P.BCGMMPolicy.random(self.obs, self.A, device="cpu", seed=40 + i, hidden_dim=self.hidden, n_blocks=self.nblk, n_gaussians=self.G, action_scale=0.4, bound=bound,
                                        std_activation="exp" if low else self.std, low_noise_eval=low)
        self.pol.out_shift = (torch.arange(self.A, dtype=torch.float32) * 0.001 - 0.003).contiguous()      # a shift, so that the inverse scaling is a product AND a sum
        if tweak is not None:
            self.pol.model = copy.deepcopy(self.pol.model)
            with torch.no_grad():
                tweak(self.pol.model)
        g = torch.Generator().manual_seed(50 + i)
        self.state = torch.randn(N, self.obs, generator=g) * 0.8
        self.z = torch.randn(N, self.A, generator=g)
        self.pol64 = copy.copy(self.pol)
        self.pol64.model = copy.deepcopy(self.pol.model).double()
        u = torch.rand(N, generator=g)
        cdf = torch.cumsum(self.reference(u)[2], dim=1)
        self.redrawn = 0
        for r in range(N):      # the bank: a u within EDGE of an edge of the f64 normalised CDF is drawn again
            while float((cdf[r] - float(u[r])).abs().min()) < P.BC_GMM_EDGE:
                u[r] = torch.rand(1, generator=g)[0]
                self.redrawn += 1
        self.u = u
        self.want, self.comps, self.p64 = self.reference(u)

    def reference(self, u, z=None, state=None):
        """The f64 restatement: (actions, components, probabilities)."""
        s = self.state if state is None else state
        z = self.z if z is None else z
        return self.pol64._predict_torch(s.double(), torch.as_tensor(u).double(), torch.as_tensor(z).double()[:s.shape[0]])

    def near_edge(self, u):
        """Rows whose u lies within EDGE of an edge of their f64 normalised CDF."""
        u = torch.as_tensor(u).double()
        return (torch.cumsum(self.reference(u)[2], dim=1) - u.unsqueeze(1)).abs().min(dim=1).values < P.BC_GMM_EDGE


def case(name):
    if name not in _CACHE:
        _CACHE[name] = Case(name)
    return _CACHE[name]


def drawn_reference():
    """The host's draws of the device-drawn launch, the f64 result on them and the rows left out: (case, u f32, z f64, (actions, components, probabilities), near)."""
    c = case(DRAWN_CASE)
    u = torch.as_tensor(P.bc_gmm_uniforms(DRAWN_SEED, DRAWN_OFFSET, N, DRAWN_T))
    z = torch.as_tensor(P.bc_gmm_normals(DRAWN_SEED, DRAWN_OFFSET, N, DRAWN_T, c.A))
    return c, u, z, c.reference(u, z), c.near_edge(u)
