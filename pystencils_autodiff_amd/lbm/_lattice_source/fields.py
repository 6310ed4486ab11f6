"""The ONE table of the lattice kernels' per-cell fields, beside the one of their arguments (``args``): a row per field
(the force ``F(x)``, the relaxation rate ``ω(x)``, the solid fraction ``σ(x)``) says how the kernels see it — the
``LatticeSource`` flag that prints it, its pointer and stride arguments — and how the host speaks of it. ``kernel_args``
prints its pointer and stride blocks from the rows; the launcher (``_lattice_kernels``) checks, keys, binds and measures
the fields by them and the step (``_autodiff_lbstep``) finds them in a rule and names them in its errors.

The printed names are irregular (``omf`` / ``domega`` beside ``sigf`` / ``dsolid``) and pinned by the emitted sources'
shas: the rows record them as they are."""
from typing import NamedTuple


class CellField(NamedTuple):
    """One per-cell field of the kernels. ``kind``: its key in a launch's bundle (``{kind: (array, adjoint)}``) and its
    ``Arg.group``; ``flag``: the ``LatticeSource`` attribute that is true when the kernels take it; ``operand`` /
    ``adjoint``: the printed pointer arguments (the adjoint: of the adjoint kernels alone, accumulated into);
    ``prefix`` / ``axes``: its stride arguments ``{prefix}_{axis}``; ``vector``: the array is ``[*domain, D]`` (else
    ``[*domain]``); ``rule``: the update rule's attribute that holds its expression. The words of its error messages:
    ``what`` ('… of shape', 'take no …'), ``kernels`` ('the … lattice kernels'), ``name`` ('need the …') and ``short``
    ('the … adjoint')."""
    kind: str
    flag: str
    operand: str
    adjoint: str
    prefix: str
    axes: str
    vector: bool
    rule: str
    what: str
    kernels: str
    name: str
    short: str

    @property
    def strides(self):
        """The names of its stride arguments, in the table's order."""
        return tuple(f'{self.prefix}_{a}' for a in self.axes)


CELL_FIELDS = (
    CellField('force', 'ff', 'force', 'dforce', 'f', 'czyx', True, 'force',
              'force field', 'force-field', 'force', 'force'),
    CellField('omega', 'of', 'omf', 'domega', 'w', 'zyx', False, 'relaxation_rate',
              'relaxation-rate field', 'ω-field', 'relaxation-rate field', 'relaxation-rate'),
    CellField('solid', 'sf', 'sigf', 'dsolid', 'p', 'zyx', False, 'solid_fraction',
              'solid-fraction field', 'σ-field', 'solid-fraction field', 'solid-fraction'),
)
