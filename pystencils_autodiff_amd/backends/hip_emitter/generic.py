"""The ``generic`` schedule (one thread per cell, runtime strides) and the border-zeroing kernel."""
import numpy as np

from ..printer import KernelExprPrinter
from .common import PRELUDE, _ctype, _statements, _tag, field_params, scalar_params, storage_ctype


def magic_u32(d):
    """(m, l) with floor(n / d) == (umulhi(n, m) + n) >> l for every 32-bit n (the 33-bit-multiplier
    form of division by an invariant integer, the add folded into a 64-bit sum)."""
    if not 1 <= d < 2 ** 32:
        raise ValueError(f'divisor {d} out of range')
    l = (d - 1).bit_length()
    m = (2 ** 32 * (2 ** l - d)) // d + 1
    return m & 0xffffffff, l


def emit_generic(ir, name, idx32=False, contig=False, shared=False):
    """One thread per cell, runtime extents/strides, bound-checked zero-padded reads.

    ``idx32``: cells are numbered in 32 bits and split into coordinates by multiply-high with
    host-computed magic numbers (``magic_u32``) instead of 64-bit division per cell. ``contig``: the
    tensors are C-contiguous, so a vector field's component strides are compile-time constants and a
    cell's components are adjacent loads the compiler merges (one ``dwordx3`` for 3 fp32 components).
    Every field's cell base offset is formed once per cell; each access adds constant offsets times
    uniform strides. ``shared``: every tensor has the same shape and strides (e.g. the component planes of
    an fzyx lattice Boltzmann pdf array): ONE set of strides and ONE cell offset, in 32 bits (the launch
    checks the elements fit), serve all fields — no per-field 64-bit multiply-adds."""
    ct = _ctype(ir.compute_dtype)
    printer = KernelExprPrinter(ct, ir.symbol_names)
    n = ir.ndim
    params = field_params(ir)
    params += [f"const i64 N{d}" for d in range(n)]
    if shared:
        params += [f"const int st_{d}" for d in range(ir.fields[0].spatial_dimensions + ir.fields[0].index_dimensions)]
    else:
        for f in ir.fields:
            params += [f"const i64 st_{f.name}_{d}" for d in range(f.spatial_dimensions + f.index_dimensions)]
    params += [f"const i64 lo{d}, const i64 hi{d}" for d in range(n)]
    if idx32:
        params += ['const unsigned ncell32'] + [f"const unsigned mg{d}, const int sh{d}" for d in range(1, n)]
    params += scalar_params(ir)
    L = [PRELUDE]
    L.append(f'extern "C" __global__ void __launch_bounds__(256) {name}({", ".join(params)})\n{{')
    # strided iteration slices (pystencils' iteration_slice with steps): [lo, hi) numbers the cells, cell k of an
    # axis sits at lo + k·step (steps are compile-time constants of the kernel)
    steps = ir.isteps or (1,) * n
    sm = ['' if steps[d] == 1 else f'{steps[d]} * ' for d in range(n)]
    if idx32:
        L.append('  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < ncell32; i += gridDim.x * 256u) {')
        L.append('    unsigned r = i;')
        for d in reversed(range(1, n)):
            L.append(f'    const unsigned q{d} = (unsigned)(((unsigned long long)__umulhi(r, mg{d}) + r) >> sh{d});')
            L.append(f'    const i64 c{d} = lo{d} + {sm[d]}(i64)(r - q{d} * (unsigned)(hi{d} - lo{d}));')
            L.append(f'    r = q{d};')
        L.append(f'    const i64 c0 = lo0 + {sm[0]}(i64)r;')
    else:
        ext = ' * '.join(f"(hi{d} - lo{d})" for d in range(n))
        L.append(f'  const i64 ncell = {ext};')
        L.append('  const i64 stride = (i64)gridDim.x * 256;')
        L.append('  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < ncell; i += stride) {')
        L.append('    i64 r = i;')
        for d in reversed(range(n)):
            L.append(f'    const i64 c{d} = lo{d} + {sm[d]}(r % (hi{d} - lo{d})); r /= (hi{d} - lo{d});')

    def istride(field, k):
        if contig:
            return str(int(np.prod([int(v) for v in field.index_shape[k + 1:]]) if k + 1 < field.index_dimensions else 1))
        return f"st_{n + k}" if shared else f"st_{field.name}_{n + k}"

    def sst(field, d):
        return f"st_{d}" if shared else f"st_{field.name}_{d}"
    if shared:
        L.append('    const int b_ = ' + ' + '.join(f"(int)c{d} * st_{d}" for d in range(n)) + ';')
    else:
        for f in ir.fields:
            L.append(f'    const i64 b_{f.name} = ' + ' + '.join(f"c{d} * st_{f.name}_{d}" for d in range(n)) + ';')

    if ir.periodic:
        # periodic lattice: each shifted coordinate wraps once (|offset| < extent, checked at plan time)
        shifts = sorted({(d, int(o[d])) for o in [r.offsets for r in ir.reads] + [st[1] for st in ir.stores]
                         for d in range(n) if o[d] != 0})
        for d, o in shifts:
            L.append(f'    i64 w{d}_{_tag(o)} = c{d} + ({o}); w{d}_{_tag(o)} += w{d}_{_tag(o)} < 0 ? N{d} : 0; '
                     f'w{d}_{_tag(o)} -= w{d}_{_tag(o)} >= N{d} ? N{d} : 0;')

    def addr(field, offs, idx):
        terms = ["b_" if shared else f"b_{field.name}"]
        if ir.periodic:
            terms += [f"((int)(w{d}_{_tag(offs[d])} - c{d})) * {sst(field, d)}" if shared else
                      f"(w{d}_{_tag(offs[d])} - c{d}) * {sst(field, d)}" for d in range(n) if offs[d] != 0]
        else:
            terms += [f"({offs[d]}) * {sst(field, d)}" for d in range(n) if offs[d] != 0]
        terms += [f"({i}) * {istride(field, k)}" for k, i in enumerate(idx) if i != 0]
        return ' + '.join(terms)

    # reads grouped by (field, offsets): one predicate, the components loaded together inside it (adjacent
    # loads in one basic block, which the compiler merges into one wide load)
    groups = {}
    for r in ir.reads:
        groups.setdefault((r.field.name, r.offsets), []).append(r)
    for (fname, offs), rs in groups.items():
        rs = sorted(rs, key=lambda r: r.index)
        if ir.zeros and not ir.periodic and any(o != 0 for o in offs):
            cond = ' && '.join(f"(c{d} + ({offs[d]})) >= 0 && (c{d} + ({offs[d]})) < N{d}"
                               for d in range(n) if offs[d] != 0)
            for r in rs:
                L.append(f'    {ct} {r.var} = ({ct})0;')
            L.append(f'    if ({cond}) {{')
            for r in rs:
                L.append(f'      {r.var} = ({ct})f_{fname}[{addr(r.field, r.offsets, r.index)}];')
            L.append('    }')
        else:
            for r in rs:
                L.append(f'    const {ct} {r.var} = ({ct})f_{fname}[{addr(r.field, r.offsets, r.index)}];')

    def store(field, offs, idx, code):
        t = storage_ctype(field)
        a = addr(field, offs, idx)
        if any(o != 0 for o in offs) and not ir.periodic:
            cond = ' && '.join(f"(c{d} + ({offs[d]})) >= 0 && (c{d} + ({offs[d]})) < N{d}" for d in range(n))
            return f'    if ({cond}) f_{field.name}[{a}] = ({t})({code});'
        return f'    f_{field.name}[{a}] = ({t})({code});'
    L += _statements(ir, printer, '    ', store)
    L.append('  }')
    L.append('}')
    return '\n'.join(L) + '\n'


def emit_zero_border(esize, idx32=False):
    """One launch zeroing the cells an interior-only kernel leaves untouched (``boundary_handling=None``):
    the field is viewed as ``[Z, Y, L]`` (``L`` = x extent × components, elements of ``esize`` bytes);
    the z-border planes, then the y-border rows of the interior planes, then the x-border elements of the
    interior rows are numbered consecutively and written by a grid-stride loop (contiguous runs for the
    first two parts, two short runs per row for the third). ``idx32``: 32-bit index arithmetic (fields
    below 2³¹ elements — 64-bit division is a long instruction sequence on the GPU)."""
    t = {2: 'unsigned short', 4: 'unsigned int', 8: 'unsigned long long'}[esize]
    name = f'psad_zero_border_b{esize}' + ('_i32' if idx32 else '')
    it = 'unsigned' if idx32 else 'i64'
    src = [PRELUDE,
           f'extern "C" __global__ void __launch_bounds__(256) {name}({t}* __restrict__ p, const i64 Z_, const i64 Y_, '
           'const i64 L_, const i64 zlo_, const i64 zhi_, const i64 ylo_, const i64 yhi_, const i64 xlo_, const i64 xhi_)',
           '{',
           f'  const {it} Z = Z_, Y = Y_, L = L_, zlo = zlo_, zhi = zhi_, ylo = ylo_, yhi = yhi_, xlo = xlo_, xhi = xhi_;',
           f'  const {it} nzi = zhi - zlo, nyi = yhi - ylo, nyb = Y - nyi, nxb = L - (xhi - xlo);',
           f'  const {it} A = (Z - nzi) * Y * L, B = nzi * nyb * L, C = nzi * nyi * nxb;',
           f'  const {it} stride = ({it})gridDim.x * 256;',
           f'  for ({it} i = ({it})blockIdx.x * 256 + threadIdx.x; i < A + B + C; i += stride) {{',
           f'    {it} z, y, x;',
           '    if (i < A) {',
           f'      const {it} pl = i / (Y * L), r = i - pl * (Y * L);',
           '      z = pl < zlo ? pl : zhi + (pl - zlo);',
           '      y = r / L; x = r - y * L;',
           '    } else if (i < A + B) {',
           f'      const {it} j = i - A, row = j / L, yb = row % nyb;',
           '      z = zlo + row / nyb; x = j - row * L;',
           '      y = yb < ylo ? yb : yhi + (yb - ylo);',
           '    } else {',
           f'      const {it} j = i - A - B, row = j / nxb, e = j - row * nxb;',
           '      z = zlo + row / nyi; y = ylo + row % nyi;',
           '      x = e < xlo ? e : xhi + (e - xlo);',
           '    }',
           f'    p[((i64)z * Y + y) * L + x] = ({t})0;',
           '  }',
           '}']
    return '\n'.join(src), name
