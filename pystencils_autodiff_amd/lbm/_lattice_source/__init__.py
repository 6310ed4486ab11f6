"""The text of the lattice Boltzmann kernels (``_lattice_kernels`` compiles and launches them).

``LatticeSource`` (``spec``) says what to print — the lattice (stencil, collision, force, walls and their links), the
target (HIP / C), the index type, the addressing mode and the adjoint mode — and ``emit`` prints it: the forward cell
(``lbm_fwd_cell``, ``collision``), the adjoint cell (``lbm_adj_cell``, ``adjoint``: prologue, moment-like sums, force
adjoint, ω-field adjoint, scatter), the adjoint's second pass (``lbm_adj_rho_cell``, ``links``) and the entry points
that call them for every cell (``entries``): HIP grid kernels, the HIP fix-up kernel over a cell list, or C loop
nests. Every kernel's argument list is one table (``args.kernel_args``), which the launcher reads too, and the
per-cell fields among the arguments are the rows of another (``fields.CELL_FIELDS``). The
``macroscopic`` variant (``macroscopic``) adds the density / velocity outputs to the forward cell and their adjoint
seeds to the adjoint cell's load of ``g``; without the flag no line of any source changes.
The ``solid_field`` variant (``solid``) blends the forward cell's stored value with the arriving population of the opposite
direction by a per-cell solid fraction σ, blends the adjoint cell's ``v_j`` likewise and accumulates ``dσ``; without the
flag no line of any source changes either.

Adjoint modes. ``programs`` gives per wall id None or the boundary's ``link_program`` (links of the cell's own pdfs the
fused form does not take, ``boundaries.link_program``; their table rows are zeros): the forward evaluates the link
from the cell's own pdfs ``c0 … c{Q-1}`` (loaded inside the link's branch), the adjoint's first pass stores ``v_j`` of
each program-linked component j to a per-cell scratch array and the second pass (``lbm_adj_rho``) adds
``Σ_j J_jk(c) v_j`` to component k of the cell — the Jacobians are evaluated there, on the cells next to a wall, not in
the first pass, whose registers they would take on every cell (``mode='inline'``, the C target).
HIP (``mode='main'`` / ``'fix'``): the forward evaluates the programs inline as above; the main adjoint carries no
program code and leaves the cells marked ``FIX_BIT`` (fluid cells next to a program wall) to ONE list-driven fix-up
kernel (``lbm_adj_fix``): the regular scatter plus ``out_k(x) += G_k``, ``G_k = Σ_j J_jk v_j`` (``adjoint.prologue``
and ``adjoint.scatter_store`` have the protocol of the two launches). The lattice's bulk runs the plain adjoint
(measured: profiles/r05_lbm_pressure.jsonl, r06_lbm_fix_merge.jsonl).
"""
from .adjoint import adjoint_cell
from .args import kernel_args, struct_format  # noqa: F401 (the launcher's)
from .collision import forward_cell
from .common import Context
from .entries import c_entries, hip_fix_entry, hip_grid_entries
from .fields import CELL_FIELDS  # noqa: F401 (the launcher's and the step's)
from .links import link_tables, rho_cell
from .smagorinsky import smagorinsky_rate
from .spec import (ARRAYS, FIX_BIT, FIX_BLOCK, SELF_BIT, LatticeSource, density_links_message,  # noqa: F401
                   link_programs, link_rows)


def emit(spec):
    """Source of the forward (``lbm_fwd``) and adjoint (``lbm_adj``) kernels of ``spec`` (a ``LatticeSource``)."""
    s, cx, L = spec, Context(spec), []
    if not s.hip:
        L.append('#include <stdint.h>\ntypedef long long i64;')
    if s.h and not s.hip:
        # the pdf arrays hold the half floats' bits: the CPU backend's conversion helpers
        from ...backends.cpu_kernel import _HALF_HELPERS
        L.append('#include <string.h>' + _HALF_HELPERS.rstrip('\n'))
    L.append(f'typedef {("_Float16" if s.hip else "uint16_t") if s.h else s.ctype} T;\ntypedef {s.idx} IDX;')
    if s.hip:
        L.append('typedef unsigned u32x2 __attribute__((ext_vector_type(2)));')
    link_tables(cx, L)
    smagorinsky_rate(cx, L)
    forward_cell(cx, L)
    adjoint_cell(cx, L)
    if s.two:
        rho_cell(cx, L)
    (c_entries if not s.hip else hip_fix_entry if s.fix else hip_grid_entries)(cx, L)
    return '\n'.join(L) + '\n'
