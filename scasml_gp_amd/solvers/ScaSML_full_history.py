"""``ScaSML_full_history`` (solvers/ScaSML_full_history.py:5-221) on libscasml_hip."""
from .ScaSML import ScaSML
from ._picard import deliver


class ScaSML_full_history(ScaSML):
    '''Full-history multilevel Picard on the defect u - u_GP.'''
    _variant = "fh"

    def uz_solve(self, n, rho, x_t, M, return_stderr=False):
        '''solvers/ScaSML_full_history.py:75-199.  return_stderr=True: (uz, se) as ScaSML.uz_solve; ValueError for M = 1.
        return_stderr="uz": (uz, se_uz), the (batch, 1 + d) standard errors of the correction (u_breve, z_breve), as ScaSML.uz_solve states
        them: of the unclipped root sum (a component on the clip: se_z says how little the clipped value means; 34 % of the components at an
        ordinary point of MLP, d = 20, n = 2, rho = 3), not finite where the unclipped z_i is not -- every row at t = T, where the z scale
        is 1 / 0 -- and without the truncation bias, the inner calls' clips and the surrogate's own error.'''
        uz, _, was_numpy, se = self._solve(n, M, x_t, return_stderr)
        return deliver(uz, was_numpy, se)

    def u_solve(self, n, rho, x_t, M=3, return_stderr=False):
        '''return_stderr=True: (u, se), se the standard error of the correction u_breve alone, as ScaSML.u_solve states it.'''
        uz, uhat, was_numpy, se = self._solve(n, M, x_t, bool(return_stderr))         # :201-221
        return deliver(self._sum16(uz[:, 0:1] + uhat[:, None]), was_numpy, se)
