"""Moments of the populations as stand-alone operators: rho = sum f, u = (sum c f) / rho,
Pi = sum cc f (reference xlb/operator/macroscopic/{zero_moment,first_moment,macroscopic,
second_moment}.py; kernel-backend call style macroscopic.py:57-64)."""

from ... import _lib
from ...compute_backend import ComputeBackend
from ..operator import Operator


def _macro(op, f, rho, u):
    _lib.check(
        _lib.load().xlbhip_macroscopic(
            op._ctx.handle, op.velocity_set.hip_id, op._compute_code, f.handle, rho.handle if rho is not None else None, u.handle if u is not None else None
        )
    )


class ZeroMoment(Operator):
    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f, rho):
        _macro(self, f, rho, None)
        return rho


class FirstMoment(Operator):
    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f, u):
        _macro(self, f, None, u)
        return u


class Macroscopic(Operator):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.zero_moment = ZeroMoment(self.velocity_set, self.precision_policy, self.compute_backend)
        self.first_moment = FirstMoment(self.velocity_set, self.precision_policy, self.compute_backend)

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f, rho, u):
        _macro(self, f, rho, u)
        return rho, u


class SecondMoment(Operator):
    """Pi components in the order (xx, xy, xz, yy, yz, zz) / (xx, xy, yy)."""

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f, pi):
        _lib.check(_lib.load().xlbhip_second_moment(self._ctx.handle, self.velocity_set.hip_id, self._compute_code, f.handle, pi.handle))
        return pi


class ScalarMoment(Operator):
    """phi = sum_j g_j of a scalar-transport field g (cardinality 2 d + 1: ScalarTransportStepper), cardinality 1."""

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, g, phi):
        _lib.check(_lib.load().xlbhip_scalar_moment(self._ctx.handle, self.velocity_set.hip_id, self._compute_code, g.handle, phi.handle))
        return phi


class MacroscopicAdjoint(Operator):
    """The transpose of Macroscopic at f applied to (dL/drho, dL/du): dL/df_l = rho_bar + sum_d u_bar_d (c_dl - u_d) / rho, written into
    the population-shaped field lam.  This is how a loss stated in rho and u enters an AdjointStepper sweep.  rho_bar (cardinality 1)
    or u_bar (cardinality d) may be None for zero.  No counterpart in the reference, which gets it from jax.grad."""

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f, rho_bar, u_bar, lam):
        _lib.macroscopic_adjoint(self._ctx, self.velocity_set.hip_id, self._compute_code, f, rho_bar, u_bar, lam)
        return lam
