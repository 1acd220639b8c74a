"""Steppers of the HIP backend: the fused incompressible Navier-Stokes step, and the same with an immersed boundary."""

from .stepper import Stepper as Stepper
from .nse_stepper import IncompressibleNavierStokesStepper as IncompressibleNavierStokesStepper
from .ibm_stepper import IBMStepper as IBMStepper, IBMBody as IBMBody, RigidMotion as RigidMotion, RigidDynamics as RigidDynamics
