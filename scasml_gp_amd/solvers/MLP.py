"""``MLP`` with the reference's call surface (solvers/MLP.py:5-288), running on libscasml_hip."""
from .. import tables
from ._picard import PicardSolver, deliver


class MLP(PicardSolver):
    '''Multilevel Picard Iteration for high dimensional semilinear PDE (solvers/MLP.py:5-25)'''
    _variant = "quad"

    def __init__(self, equation, seed=0, compat_crn=False, compat_f16=False, compat_rng=None, reference_mode=False):
        """reference_mode=True: what the reference's solver object computes -- its random stream under its key schedule
        (compat_rng="jax") and its solver-level float16 casts (compat_f16) -- in one switch."""
        super().__init__(equation, None, seed, compat_crn=compat_crn, compat_f16=compat_f16, compat_rng=compat_rng, reference_mode=reference_mode)

    def f(self, x_t, u, z):
        return self.equation.f(x_t, u, z)                         # :27-41

    def g(self, x_t):
        return self.equation.g(x_t)[:, 0]                         # :43-55

    def inverse_gamma(self, gamma_input):
        '''Inverse of the gamma function through Lambert W (solvers/MLP.py:57-69); scalar or array in, the same out.'''
        return tables.inverse_gamma(gamma_input)

    def lgwt(self, N, a, b):
        '''(nodes, weights) exactly as the reference's routine returns them, its scalar quirk at :99 included (solvers/MLP.py:71-109).'''
        return tables.lgwt_reference(int(N), a, b)

    def approx_parameters(self, rhomax):
        return tables.approx_parameters(int(rhomax), float(self.T))   # :111-139 (cached)

    def uz_solve(self, n, rho, x_t, return_stderr=False):
        '''(batch, 1 + d): u and z of solvers/MLP.py:141-274.  return_stderr=True: (uz, se), se the (batch, 1) float32 Monte-Carlo standard
        error of u (of the unclipped root sum; the Picard truncation bias is not in it): scasml_picard_tree_stderr in include/scasml_hip.h.
        ValueError where a term of the root call has one sample (rho <= 2).
        return_stderr="uz": (uz, se_uz), se_uz the (batch, 1 + d) float32 standard errors of (u, z_1 .. z_d) -- column 0 bit for bit the se of
        return_stderr=True -- under the same refusals (scasml_picard_tree_stderr_uz in include/scasml_hip.h).  se_z is the error of the
        UNCLIPPED root sum while the returned z is clipped: where a component sits on the clip, se_z says how little the clipped value
        means (d = 20, n = 2, rho = 3, clip 1: median se of u 0.06, of a z component 0.65; at an ordinary point, t = 0.31, 34 % of the
        returned components sit on the clip).  Where the unclipped z_i is NaN or infinite, se_z_i is not finite.  The truncation bias and
        the inner calls' clips are not in it.
        An equation with torch callbacks that sets staged_stderr = True (NotImplementedError without it) gets both estimates, under the same definition and refusals, from the last stage of the staged tree
        (scasml_picard_stage_stderr).'''
        self.Mf, self.Mg, self.Q, self.c, self.w = self.approx_parameters(rho)
        uz, _, was_numpy, se = self._solve(n, rho, x_t, return_stderr)
        return deliver(uz, was_numpy, se)

    def u_solve(self, n, rho, x_t, return_stderr=False):
        if return_stderr:
            uz, se = self.uz_solve(n, rho, x_t, return_stderr=True)
            return uz[:, 0:1], se
        return self.uz_solve(n, rho, x_t)[:, 0:1]                 # :276-288
