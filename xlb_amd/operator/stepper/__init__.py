"""Steppers of the HIP backend: the fused incompressible Navier-Stokes step, the same with an immersed boundary, and the same
with a transported scalar."""

from .stepper import Stepper as Stepper
from .nse_stepper import IncompressibleNavierStokesStepper as IncompressibleNavierStokesStepper
from .ibm_stepper import IBMStepper as IBMStepper, IBMBody as IBMBody, RigidMotion as RigidMotion, RigidDynamics as RigidDynamics
from .scalar_stepper import ScalarTransportStepper as ScalarTransportStepper
