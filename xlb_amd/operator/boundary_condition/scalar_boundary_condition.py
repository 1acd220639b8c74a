"""Boundary rules of the transported scalar (ScalarTransportStepper).

A scalar rule attaches to a FLUID boundary condition by ``on=``: there is no second mask.  It acts at the cells that carry the fluid
BC's id in ``bc_mask``, on the scalar directions (the lattice's main directions) whose bit is set in the fluid's ``missing_mask`` — so
a body from indices or from a mesh masker works unchanged.  A boundary cell whose fluid BC has no rule attached is adiabatic.  At
FullwayBounceBackBC cells the scalar is bounced fullway, like the fluid.

Not covered: flux (Neumann != 0) walls, conjugate heat transfer, the wall-velocity term of anti-bounce-back at moving walls."""

import math

from ... import _lib
from .boundary_condition import BoundaryCondition, FullwayBounceBackBC


class ScalarBoundaryCondition:
    rule = None

    def __init__(self, on, value=0.0):
        if not isinstance(on, BoundaryCondition):
            raise ValueError("a scalar boundary rule attaches to a fluid boundary condition: on=<BoundaryCondition>")
        self.on = on
        self.value = float(value)
        if not math.isfinite(self.value):
            raise ValueError("the scalar value must be finite")

    def _hip_rule(self):
        return (self.on.id, self.rule, self.value)


class ScalarDirichletBC(ScalarBoundaryCondition):
    """Anti-bounce-back at the halfway wall: the scalar takes ``value`` at the link midpoint."""

    rule = _lib.Scalar.DIRICHLET

    def __init__(self, value, on):
        super().__init__(on, value)
        if isinstance(on, FullwayBounceBackBC):
            raise ValueError("ScalarDirichletBC cannot attach to a FullwayBounceBackBC: the scalar is bounced fullway there (use a halfway wall)")


class ScalarAdiabaticBC(ScalarBoundaryCondition):
    """Bounce-back: zero flux through the wall (the default of every boundary cell)."""

    rule = _lib.Scalar.ADIABATIC

    def __init__(self, on):
        super().__init__(on)


class ScalarDoNothingBC(ScalarBoundaryCondition):
    """The BC's cells keep their own pre-streaming scalar populations, all directions (what DoNothingBC does for f)."""

    rule = _lib.Scalar.DO_NOTHING

    def __init__(self, on):
        super().__init__(on)
