"""Steppers of the HIP backend: the fused incompressible Navier-Stokes step, the same with an immersed boundary, the same
with a transported scalar, the discrete adjoint of the plain BGK step, the porous BGK step (a per-cell solidity, with its
adjoint), the Shan-Chen liquid-vapour step and the Shan-Chen step of two immiscible components."""

from .stepper import Stepper as Stepper
from .nse_stepper import IncompressibleNavierStokesStepper as IncompressibleNavierStokesStepper
from .ibm_stepper import IBMStepper as IBMStepper, IBMBody as IBMBody, RigidMotion as RigidMotion, RigidDynamics as RigidDynamics
from .scalar_stepper import ScalarTransportStepper as ScalarTransportStepper
from .porous_stepper import PorousStepper as PorousStepper
from .adjoint_stepper import AdjointStepper as AdjointStepper
from .multiphase_stepper import (
    MultiphaseStepper as MultiphaseStepper,
    ShanChenExponential as ShanChenExponential,
    ShanChenDensity as ShanChenDensity,
    CarnahanStarling as CarnahanStarling,
)
from .multicomponent_stepper import MulticomponentStepper as MulticomponentStepper, ShanChenMixture as ShanChenMixture
