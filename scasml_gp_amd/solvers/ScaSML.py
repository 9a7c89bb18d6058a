"""``ScaSML`` (solvers/ScaSML.py:5-304): multilevel Picard on the defect u - u_GP, on libscasml_hip."""
from .. import tables
from ._picard import PicardSolver, deliver


class ScaSML(PicardSolver):
    '''Multilevel Picard Iteration calibrated GP for high dimensional semilinear PDE'''
    _variant = "quad"

    def __init__(self, equation, GP, seed=0, compat_crn=False, compat_f16=False, compat_rng=None, reference_mode=False):
        """reference_mode=True: the reference's random stream under its key schedule (compat_rng="jax") and its solver-level float16
        casts (compat_f16) in one switch; with the default GP (compat="reference") that is the reference's ScaSML."""
        self.GP = GP
        super().__init__(equation, GP, seed, compat_crn=compat_crn, compat_f16=compat_f16, compat_rng=compat_rng, reference_mode=reference_mode)

    def __setattr__(self, name, value):
        object.__setattr__(self, name, value)
        if name == "GP" and "_engine" in self.__dict__:            # harness reassigns solver.GP
            self._engine.gp = value

    def f(self, x_t, u_breve, z_breve):
        '''solvers/ScaSML.py:29-47 (host view; the kernels fuse this into the tree walk).'''
        eq = self.equation
        u_hat = self.GP.predict(x_t)
        grad_x = self.GP.compute_gradient(x_t, u_hat)[:, :-1]
        return eq.f(x_t, u_breve + u_hat, eq.sigma(x_t) * grad_x + z_breve) - eq.f(x_t, u_hat, eq.sigma(x_t) * grad_x)

    def g(self, x_t):
        return (self.equation.g(x_t) - self.GP.predict(x_t))[:, 0]   # :49-63

    def inverse_gamma(self, gamma_input):
        '''Inverse of the gamma function through Lambert W (solvers/ScaSML.py:65-77); scalar or array in, the same out.'''
        return tables.inverse_gamma(gamma_input)

    def lgwt(self, N, a, b):
        '''(nodes, weights) exactly as the reference's routine returns them, its scalar quirk at :99 included (solvers/ScaSML.py:79-117).'''
        return tables.lgwt_reference(int(N), a, b)

    def approx_parameters(self, rhomax):
        return tables.approx_parameters(int(rhomax), float(self.T))

    def uz_solve(self, n, rho, x_t, return_stderr=False):
        '''solvers/ScaSML.py:149-284.  return_stderr=True: (uz, se), se the (batch, 1) float32 Monte-Carlo standard error of u_breve
        (scasml_picard_tree_stderr in include/scasml_hip.h); ValueError where a term of the root call has one sample (rho <= 2).
        return_stderr="uz": (uz, se_uz), se_uz the (batch, 1 + d) float32 standard errors of the correction (u_breve, z_breve_1 ..
        z_breve_d) -- column 0 bit for bit the se of return_stderr=True -- under the same refusals (scasml_picard_tree_stderr_uz in
        include/scasml_hip.h).  se_z is the error of the UNCLIPPED root sum while the returned z is clipped (at equation.uncertainty):
        where a component sits on the clip, se_z says how little the clipped value means (for MLP at d = 20, n = 2, rho = 3, clip 1: median
        se of u 0.06, of a z component 0.65; at an ordinary point, t = 0.31, 34 % of the returned components sit on the clip).  Where the
        unclipped z_i is NaN or infinite, se_z_i is not finite.  The truncation bias, the inner calls' clips and the surrogate's own error
        are not in it: this is the se of the correction.'''
        self.Mf, self.Mg, self.Q, self.c, self.w = self.approx_parameters(rho)       # :161
        uz, _, was_numpy, se = self._solve(n, rho, x_t, return_stderr)
        return deliver(uz, was_numpy, se)

    def u_solve(self, n, rho, x_t, return_stderr=False):
        '''u_hat + u_breve, solvers/ScaSML.py:286-304.  return_stderr=True: (u, se) with se the (batch, 1) float32 standard error of the
        CORRECTION u_breve: u_hat is deterministic given the fit, so se(u_hat + u_breve) = se(u_breve).  It is the Monte-Carlo error of the
        unclipped Picard sum on the defect and nothing else: the surrogate's own error (GP.predict_variance) and the Picard truncation
        bias are not in it, and the clip of u_breve is not modelled.'''
        self.Mf, self.Mg, self.Q, self.c, self.w = self.approx_parameters(rho)
        uz, uhat, was_numpy, se = self._solve(n, rho, x_t, bool(return_stderr))
        return deliver(self._sum16(uz[:, 0:1] + uhat[:, None]), was_numpy, se)

    def _sum16(self, total):
        """compat_f16: u_breve + u_hat is a float16 sum in the reference (:300-304: u_breve float16 by :284 -- in the full-history solver by
        float16 arithmetic throughout -- and u_hat float16 by models/GP.py:671); held in float32."""
        import torch
        return total.to(torch.float16).to(torch.float32) if self._engine.compat_f16 else total
