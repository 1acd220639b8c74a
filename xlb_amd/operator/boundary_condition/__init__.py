from .boundary_condition import (
    BoundaryCondition as BoundaryCondition,
    ImplementationStep as ImplementationStep,
    boundary_condition_registry as boundary_condition_registry,
    EquilibriumBC as EquilibriumBC,
    HalfwayBounceBackBC as HalfwayBounceBackBC,
    FullwayBounceBackBC as FullwayBounceBackBC,
    DoNothingBC as DoNothingBC,
    ZouHeBC as ZouHeBC,
    RegularizedBC as RegularizedBC,
    ExtrapolationOutflowBC as ExtrapolationOutflowBC,
    HybridBC as HybridBC,
)
from .scalar_boundary_condition import (
    ScalarBoundaryCondition as ScalarBoundaryCondition,
    ScalarDirichletBC as ScalarDirichletBC,
    ScalarAdiabaticBC as ScalarAdiabaticBC,
    ScalarDoNothingBC as ScalarDoNothingBC,
)
