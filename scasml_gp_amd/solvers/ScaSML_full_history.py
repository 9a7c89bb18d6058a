"""``ScaSML_full_history`` (solvers/ScaSML_full_history.py:5-221) on libscasml_hip."""
from .ScaSML import ScaSML
from ._picard import deliver


class ScaSML_full_history(ScaSML):
    '''Full-history multilevel Picard on the defect u - u_GP.'''
    _variant = "fh"

    def uz_solve(self, n, rho, x_t, M, return_stderr=False):
        '''solvers/ScaSML_full_history.py:75-199.  return_stderr=True: (uz, se) as ScaSML.uz_solve; ValueError for M = 1.'''
        uz, _, was_numpy, se = self._solve(n, M, x_t, return_stderr)
        return deliver(uz, was_numpy, se)

    def u_solve(self, n, rho, x_t, M=3, return_stderr=False):
        '''return_stderr=True: (u, se), se the standard error of the correction u_breve alone, as ScaSML.u_solve states it.'''
        uz, uhat, was_numpy, se = self._solve(n, M, x_t, return_stderr)               # :201-221
        return deliver(self._sum16(uz[:, 0:1] + uhat[:, None]), was_numpy, se)
