"""The ONE table of the lattice kernels' arguments: the printed parameter lists, the C entry points' ``P[]`` / ``S[]``
unpacking and the launcher's argument buffers (``_lattice_kernels``) are all read off ``kernel_args``."""
from typing import NamedTuple

from .fields import CELL_FIELDS
from .spec import ARRAYS

POINTER, EXTENT, STRIDE, REACH, RATE, CELLS, COUNT = 'pointer', 'extent', 'stride', 'reach', 'rate', 'cells', 'count'
KERNELS = ('fwd', 'adj', 'adj_rho', 'adj_fix')


class Arg(NamedTuple):
    """One kernel argument: its name, its kind, the C declaration as printed and the operand group it came with
    ('pdf': the pdf arrays, the mask and the wall ids; 'force'; 'omega'; 'solid'; 'scratch'; 'macro'; 'fix')."""
    name: str
    kind: str
    decl: str
    group: str


def rate_names(spec):
    """``(ω0, the rate argument)``: the cell's ω0 is ``omega``, with Smagorinsky ``omega_0`` (``omega`` is then the
    effective rate the collision reads); the scalar argument is ω0, or with an ω field — which the cell loads ω0
    from — the unused ``omega_s``."""
    om0 = 'omega_0' if spec.sm is not None else 'omega'
    return om0, 'omega_s' if spec.of else om0


def _ptr(name, group, const=True, ty='T'):
    return Arg(name, POINTER, f'{"const " if const else ""}{ty}* __restrict__ {name}', group)


def _strides(prefix, axes, group):
    return [Arg(f'{prefix}_{a}', STRIDE, f'const IDX {prefix}_{a}', group) for a in axes]


_EXTENTS = [Arg(n, EXTENT, f'const int {n}', 'pdf') for n in 'ZYX']
_MASK, _IDS = _ptr('nbmask', 'pdf', ty='unsigned'), _ptr('wallid', 'pdf', ty='unsigned char')


def macroscopic_pointers(spec, adj):
    """The 'macro' group's arrays (``macroscopic``), of the compute type, the last pointers of the table: the forward
    writes ``rho_out`` (strides ``r_*``) and ``vel_out`` (``v_*``); the adjoint reads the seeds ``drho`` / ``dvel``
    (the same strides) and, for a compressible rule alone, the recorded outputs."""
    if not spec.mo:
        return []
    ty = spec.ctype
    if not adj:
        return [_ptr('rho_out', 'macro', const=False, ty=ty), _ptr('vel_out', 'macro', const=False, ty=ty)]
    out = [_ptr('rho_out', 'macro', ty=ty), _ptr('vel_out', 'macro', ty=ty)] if spec.compressible else []
    return out + [_ptr('drho', 'macro', ty=ty), _ptr('dvel', 'macro', ty=ty)]


def kernel_args(spec, kernel):
    """The arguments of ``lbm_{kernel}`` (``kernel`` in ``KERNELS``) for ``spec``, in the order of the HIP parameter
    list; the C entry points' ``P`` and ``S`` arrays hold the pointer-kind and the stride-kind entries in this order."""
    if kernel == 'adj_fix':
        return kernel_args(spec, 'adj') + (Arg('cells', CELLS, 'const int* __restrict__ cells', 'fix'),
                                           Arg('ncell', COUNT, 'const int ncell', 'fix'))
    if kernel == 'adj_rho':
        rho = [_ptr('out', 'pdf', const=False), _MASK, _ptr('rho_adj', 'scratch')] + _EXTENTS + \
            _strides('o', 'qzyx', 'pdf')
        if spec.inl:
            # the programs' Jacobians read the cell's own pdfs and the neighbours' wall ids
            rho += [_ptr('src', 'pdf'), _IDS] + _strides('s', 'qzyx', 'pdf')
        return tuple(rho)
    adj = kernel == 'adj'
    pdfs = {'fwd': 'sd', 'adj': 'sgo'}[kernel]            # the pdf arrays of the cell function (the last one written)
    A = [_ptr(ARRAYS[p], 'pdf', const=p != pdfs[-1]) for p in pdfs] + [_MASK, _IDS]
    fields = [f for f in CELL_FIELDS if getattr(spec, f.flag)]
    for f in fields:
        A += [_ptr(f.operand, f.kind)] + ([_ptr(f.adjoint, f.kind, const=False)] if adj else [])
    if adj and spec.two:
        A += [_ptr('rho_adj', 'scratch', const=False)]
    A += macroscopic_pointers(spec, adj)
    A += _EXTENTS + [a for p in pdfs for a in _strides(p, 'qzyx', 'pdf')]
    A += [a for f in fields for a in _strides(f.prefix, f.axes, f.kind)]
    A += _strides('r', 'zyx', 'macro') + _strides('v', 'czyx', 'macro') if spec.mo else []
    A += [Arg(f'{p}_bytes', REACH, f'const long long {p}_bytes', 'pdf') for p in pdfs]
    # (with an ω field the scalar rate is not what the collision reads: the cell loads ``omega``)
    name = rate_names(spec)[1]
    return tuple(A + [Arg(name, RATE, f'const {spec.ctype} {name}', 'pdf')])


def struct_format(table, idx, ctype):
    """``struct`` codes of a launch's argument buffer, one per entry of ``table``: strides by the index type, the rate
    by the compute type."""
    code = {POINTER: 'Q', EXTENT: 'i', STRIDE: 'i' if idx == 'int' else 'q', REACH: 'q',
            RATE: 'd' if ctype == 'double' else 'f', CELLS: 'Q', COUNT: 'i'}
    return ''.join(code[a.kind] for a in table)
