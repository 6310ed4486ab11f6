"""Differentiable lattice Boltzmann time stepping (reference ``pystencils_autodiff.lbm``)."""
from ._autodiff_lbstep import AutoDiffLatticeBoltzmannStep, PdfFieldNotDetectedException, SimulationResultsTensors
from ._method import (LBStencil, create_lb_adjoint_rule, create_lb_update_rule, equilibrium_setter, macroscopic_getter,
                      macroscopic_setter, relaxation_rate_from_magic_number)
from ._wall_force import BoundaryLinks, WallForceKernels, boundary_links, force_table
from .boundaries import (UBB, AdjointBoundaryCondition, AdjointNoSlip, Boundary, FixedDensity, FreeSlip,
                         NeighbourBoundary, NoSlip, ZeroGradientOutflow, link_coefficients, link_form, link_program,
                         make_slice, neighbour_link_program)

__all__ = ['AutoDiffLatticeBoltzmannStep', 'PdfFieldNotDetectedException', 'SimulationResultsTensors', 'LBStencil',
           'create_lb_update_rule', 'create_lb_adjoint_rule', 'macroscopic_getter', 'equilibrium_setter',
           'macroscopic_setter', 'Boundary', 'NoSlip', 'UBB', 'FixedDensity', 'NeighbourBoundary', 'FreeSlip',
           'ZeroGradientOutflow', 'AdjointNoSlip', 'AdjointBoundaryCondition', 'link_coefficients', 'link_form',
           'link_program', 'neighbour_link_program', 'make_slice', 'relaxation_rate_from_magic_number',
           'BoundaryLinks', 'WallForceKernels', 'boundary_links', 'force_table']
