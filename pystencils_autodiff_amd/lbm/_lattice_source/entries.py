"""The entry points that call the cell functions for every cell: HIP grid kernels, the HIP fix-up kernel over a cell
list, or C loop nests."""
from .args import POINTER, RATE, REACH, STRIDE
from .spec import FIX_BLOCK

C_LOOPS = ('  #pragma omp parallel for collapse(2) schedule(static)\n'
           '  for (int z = 0; z < Z; ++z)\n    for (int y = 0; y < Y; ++y)\n      for (int x = 0; x < X; ++x)')
CELL_ZYX = ('  const unsigned r = cell / (unsigned)X;\n'
            '  const int x = (int)(cell - r * (unsigned)X);\n'
            '  const int z = (int)(r / (unsigned)Y), y = (int)(r - (unsigned)z * Y);')


def hip_fix_entry(cx, L):
    """The fix-up kernel: one thread per listed cell (the fluid cells next to a link-program wall).
    One wave per workgroup (FIX_BLOCK lanes): the few listed cells spread over as many CUs as possible — each wave
    runs a long, branchy, latency-bound chain, and waves of one CU would share its scalar unit."""
    L.append(f'extern "C" __global__ void __launch_bounds__({FIX_BLOCK}) lbm_adj_fix({cx.sig["adj_fix"]})\n{{')
    L.append(f'  const int t = (int)(blockIdx.x * {FIX_BLOCK}u + threadIdx.x);')
    L.append('  if (t >= ncell) return;')
    L.append('  const unsigned cell = (unsigned)cells[t];')
    L.append(CELL_ZYX)
    L.append(f'  lbm_adj_cell({cx.args["adj"]}, z, y, x);\n}}')


def hip_grid_entries(cx, L):
    """``lbm_fwd``, ``lbm_adj`` (and ``lbm_adj_rho``): one thread per cell.
    A block = 256 consecutive cells of the lattice in C order (rows of x), and consecutive blocks on one XCD
    (bijective remap of the round-robin dispatch): a lattice row's x-shifted loads and the adjoint's
    x-shifted stores cover cache lines that the neighbouring wave also touches — in one block, or in a
    block on the same XCD's L2, not split between two L2s (partial-line write-backs)."""
    for k in ('fwd', 'adj') + (('adj_rho',) if cx.s.two else ()):
        L.append(f'extern "C" __global__ void __launch_bounds__(256) lbm_{k}({cx.sig[k]})\n{{')
        L.append('  const unsigned nb = gridDim.x, b = blockIdx.x;')
        L.append('  const unsigned per = nb >> 3, rem = nb & 7, xcd = b & 7, bi = b >> 3;')
        L.append('  const unsigned lb = (xcd < rem) ? xcd * (per + 1) + bi : rem * (per + 1) + (xcd - rem) * per + bi;')
        L.append('  const unsigned cell = lb * 256u + threadIdx.x;     // cells < 2^32 (checked at launch)')
        L.append('  if (cell >= (unsigned)X * (unsigned)Y * (unsigned)Z) return;')
        L.append(CELL_ZYX)
        L.append(f'  lbm_{k}_cell({cx.args[k]}, z, y, x);\n}}')


def c_entries(cx, L):
    """The C loop nests, with the CPU kernels' ctypes signature (``backends.cpu_kernel.compile_c``): pointers,
    extents, strides, -, scalars. ``P`` holds the table's pointers and ``S`` its strides, each in the table's order,
    one line per operand group. ``lbm_adj`` runs the second pass after every cell's scatter, in the same call."""
    for k in ('fwd', 'adj'):
        table = cx.tables[k]
        ptrs, strides = ([a for a in table if a.kind == kind] for kind in (POINTER, STRIDE))
        L.append(f'void lbm_{k}(void** P, const i64* N, const i64* S, const i64* B_, const double* Dv)\n{{')
        L.append('  (void)B_; const int Z = (int)N[0], Y = (int)N[1], X = (int)N[2];')
        L.append(''.join(f'  {a.decl} = ({cx.ct})Dv[0];' for a in table if a.kind == RATE))
        for group in dict.fromkeys(a.group for a in ptrs):
            types = [(a.decl.replace(' __restrict__', '').rsplit(' ', 1)[0], a) for a in ptrs if a.group == group]
            L.append('  ' + ' '.join(f'{ty} {a.name} = ({ty})P[{ptrs.index(a)}];' for ty, a in types))
            if any(a.group == group for a in strides):
                L.append('  const IDX ' + ', '.join(f'{a.name} = S[{i}]' for i, a in enumerate(strides)
                                                    if a.group == group) + ';')
        L.append('  const long long ' + ', '.join(f'{a.name} = 0' for a in table if a.kind == REACH) + ';')
        for cellfn in (k, 'adj_rho') if k == 'adj' and cx.s.two else (k,):
            # (the density pass after every cell's scatter: the C target runs both passes in one call)
            L.append(C_LOOPS)
            L.append(f'        lbm_{cellfn}_cell({cx.args[cellfn]}, z, y, x);')
        L.append('}')
