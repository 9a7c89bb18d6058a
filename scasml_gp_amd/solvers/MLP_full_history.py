"""``MLP_full_history`` (solvers/MLP_full_history.py:6-196) on libscasml_hip."""
from .MLP import MLP
from ._picard import deliver


class MLP_full_history(MLP):
    '''Full-history multilevel Picard: one uniformly random time per sample, M^n / M^(n-l) samples.  The constructor is MLP's;
    reference_mode=True here means the reference's random stream with every draw from the one key of MLP_full_history.py:92-93, and its
    solver-level float16 casts, in one switch.'''
    _variant = "fh"

    def uz_solve(self, n, rho, x_t, M, return_stderr=False):
        '''solvers/MLP_full_history.py:64-180 (rho is ignored there as well).  return_stderr=True: (uz, se), se the (batch, 1) float32
        Monte-Carlo standard error of u (of the unclipped root sum; the Picard truncation bias is not in it): scasml_picard_tree_stderr in
        include/scasml_hip.h.  ValueError for M = 1 (one sample per term).
        return_stderr="uz": (uz, se_uz), se_uz the (batch, 1 + d) float32 standard errors of (u, z_1 .. z_d) -- column 0 bit for bit the se of
        return_stderr=True -- under the same refusals (scasml_picard_tree_stderr_uz in include/scasml_hip.h).  se_z is the error of the
        UNCLIPPED root sum while the returned z is clipped: where a component sits on the clip, se_z says how little the clipped value
        means (d = 20, n = 2, rho = 3, clip 1: median se of u 0.06, of a z component 0.65; at an ordinary point, t = 0.31, 34 % of the
        returned components sit on the clip).  Where the unclipped z_i is NaN or infinite, se_z_i is not finite.  The truncation bias and
        the inner calls' clips are not in it.  At t = T the full history's z scale is 1 / 0: the se_z of such a row is not finite.
        An equation with torch callbacks that sets staged_stderr = True (NotImplementedError without it) gets both estimates, under the same definition and refusals, from the last stage of the staged tree
        (scasml_picard_stage_stderr).'''
        uz, _, was_numpy, se = self._solve(n, M, x_t, return_stderr)
        return deliver(uz, was_numpy, se)

    def u_solve(self, n, rho, x_t, M=3, return_stderr=False):
        if return_stderr:
            uz, se = self.uz_solve(n, rho, x_t, M, return_stderr=True)
            return uz[:, 0:1], se
        return self.uz_solve(n, rho, x_t, M)[:, 0:1]              # :182-196
