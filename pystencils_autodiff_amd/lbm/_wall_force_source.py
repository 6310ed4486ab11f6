"""The text of the boundary-force kernels (``_wall_force`` builds the link lists, compiles and launches them).

The force on a boundary object is the momentum-exchange sum over its links ``(x, d)`` — fluid cell ``x``, direction
``d``, ``x + c_d`` a cell of the boundary — of ``c_d·((1 + α_d)·f_d(x) + β_d)`` ("Boundary force"). One text
per (stencil, storage type) for both targets, in the lattice kernels' conventions: the pdf array addressed by strides
``(s_q, s_z, s_y, s_x)``, index type ``IDX``, buffer resources (``'buf'``) or plain pointers (``'ptr'``), ``_Float16``
storage. The link list is two arrays — C-order cell index (``IDX``) and direction (one byte) per link — and ``tab``
holds two doubles per direction: ``1 + α_d`` and ``β_d`` (plus ``(1 + α_d)·w_d`` for zero-centred storage), so the text
does not depend on the boundary object.

HIP:

* ``lbm_wall_force``: 256 threads, grid-stride over the links, D partial sums in double per thread; the wave's sum by
  shuffles of width 64, the four waves' through LDS in wave order; one ``double[D]`` per workgroup into ``part``.
* ``lbm_wall_force_sum``: one workgroup stages the partials through LDS; thread a adds component a in index order and
  stores it in the compute type.
* ``lbm_wall_force_adj``: one thread per link, ``g_d(x) += (1 + α_d)·Σ_a c_{d,a}·dF_a``: the value (at most three
  terms, added in double) rounded once to the compute type, added there and rounded once to the array's type. A
  (cell, direction) pair occurs once in a list: plain loads and stores.

No atomics anywhere: the same links and the same block count give the same bits. C: the same sums as plain loops
(``lbm_wall_force`` writes the force itself, there is no second stage).
"""

KERNELS = ('lbm_wall_force', 'lbm_wall_force_sum', 'lbm_wall_force_adj')
BLOCK = 256
SUM_CHUNK = 768          # doubles per LDS chunk of the second stage: a multiple of D = 2 and 3 (256 partials of D = 3)


def _types(dtype_name):
    """(storage type on HIP, on C, compute type, element size) of a pdf dtype."""
    return {'float64': ('double', 'double', 'double', 8), 'float32': ('float', 'float', 'float', 4),
            'float16': ('_Float16', 'uint16_t', 'float', 2)}[dtype_name]


def _decode(D):
    """``z, y, x`` of the C-order cell index ``cell`` (2-D: z = 0)."""
    L = ['    const IDX r = cell / X;', '    const int x = (int)(cell - r * X);']
    if D == 3:
        L.append('    const int z = (int)(r / Y), y = (int)(r - (IDX)z * Y);')
    else:
        L.append('    const int z = 0, y = (int)r; (void)Y;')
    return L


def _offset(p):
    return f'    const IDX off = (IDX)d * {p}_q + (IDX)z * {p}_z + (IDX)y * {p}_y + (IDX)x * {p}_x;'


def emit(stencil, dtype_name, target='hip', idx='int', addr='buf'):
    """Source of the three kernels (HIP) or of ``lbm_wall_force`` / ``lbm_wall_force_adj`` as loops (C) for pdfs of
    ``dtype_name`` on ``stencil``."""
    hip = target == 'hip'
    th, tc, ct, esize = _types(dtype_name)
    half = dtype_name == 'float16'
    D, Q = stencil.D, stencil.Q
    dirs = [tuple(int(v) for v in c) for c in stencil.directions]
    cvals = ', '.join(str(v) for c in dirs for v in c)
    buf = hip and addr == 'buf'
    bits, bty = {8: ('b64', 'u32x2'), 4: ('b32', 'unsigned'), 2: ('b16', 'unsigned short')}[esize]
    L = []
    if not hip:
        idx = 'long long'
        L.append('#include <stdint.h>\ntypedef long long i64;')
        if half:
            from ..backends.cpu_kernel import _HALF_HELPERS
            L.append('#include <string.h>' + _HALF_HELPERS.rstrip('\n'))
    L.append(f'typedef {th if hip else tc} T;\ntypedef {ct} CT;\ntypedef {idx} IDX;')
    if hip:
        L.append('typedef unsigned u32x2 __attribute__((ext_vector_type(2)));')
    L.append(f'{"__constant__" if hip else "static const"} int wf_c[{Q * D}] = {{{cvals}}};')

    def load(p, arr):
        if buf:
            return (f'(CT)__builtin_bit_cast(T, ({bty})__builtin_amdgcn_raw_buffer_load_{bits}(rs_{p}, '
                    f'(unsigned)off * {esize}u, 0, 0))')
        return f'(CT)psad_h2f({arr}[off])' if half and not hip else f'(CT){arr}[off]'

    def store(p, arr, val):
        if buf:
            return (f'__builtin_amdgcn_raw_buffer_store_{bits}(__builtin_bit_cast({bty}, (T)({val})), rs_{p}, '
                    f'(unsigned)off * {esize}u, 0, 0);')
        return f'{arr}[off] = psad_f2h((float)({val}));' if half and not hip else f'{arr}[off] = (T)({val});'

    def resource(p, arr):
        return (f'  const __amdgpu_buffer_rsrc_t rs_{p} = __builtin_amdgcn_make_buffer_rsrc((void*){arr}, (short)0, '
                f'(int){p}_bytes, 0x00020000);') if buf else f'  (void){p}_bytes;'

    term = ['    const double term = tab[2 * d] * (double)f + tab[2 * d + 1];']
    for a in range(D):
        term.append(f'    acc{a} += (double)wf_c[{D} * d + {a}] * term;')
    # (c_d·dF: at most three terms, added in double — for float gradients exact but for exponents 29 apart — then the
    # value is rounded once to the compute type)
    dot = ['    double dot = 0.0;']
    for a in range(D):
        dot.append(f'    if (wf_c[{D} * d + {a}]) dot += (double)wf_c[{D} * d + {a}] * (double)dF[{a}];')
    strides = lambda p: f'IDX {p}_q, IDX {p}_z, IDX {p}_y, IDX {p}_x, long long {p}_bytes'  # noqa: E731
    lists = 'const IDX* __restrict__ cells, const unsigned char* __restrict__ dirs, const double* __restrict__ tab'
    if hip:
        # -- the gather-reduce --------------------------------------------------------------------------------
        L.append(f'extern "C" __global__ void __launch_bounds__({BLOCK}) lbm_wall_force(const T* __restrict__ src, '
                 f'{lists}, double* __restrict__ part, long long n, int Y, int X, {strides("s")})\n{{')
        L.append(resource('s', 'src'))
        L.append('  double ' + ', '.join(f'acc{a} = 0.0' for a in range(D)) + ';')
        L.append(f'  const long long step = (long long)gridDim.x * {BLOCK};')
        L.append(f'  for (long long l = (long long)blockIdx.x * {BLOCK} + threadIdx.x; l < n; l += step) {{')
        L.append('    const IDX cell = cells[l];\n    const int d = dirs[l];')
        L += _decode(D)
        L.append(_offset('s'))
        L.append(f'    const CT f = {load("s", "src")};')
        L += term
        L.append('  }')
        L.append('  for (int o = 32; o > 0; o >>= 1) {')
        for a in range(D):
            L.append(f'    acc{a} += __shfl_down(acc{a}, o, 64);')
        L.append('  }')
        L.append(f'  __shared__ double red[{4 * D}];')
        L.append('  const int wave = (int)(threadIdx.x >> 6);')
        L.append('  if ((threadIdx.x & 63u) == 0u) { ' +
                 ' '.join(f'red[{D} * wave + {a}] = acc{a};' for a in range(D)) + ' }')
        L.append('  __syncthreads();')
        L.append(f'  if (threadIdx.x < {D}u) {{\n    const int a = (int)threadIdx.x;')
        L.append(f'    part[(long long)blockIdx.x * {D} + a] = ((red[a] + red[{D} + a]) + red[{2 * D} + a]) + '
                 f'red[{3 * D} + a];\n  }}\n}}')
        # -- the partials, in index order ---------------------------------------------------------------------
        # (the partials staged through LDS by the whole workgroup, SUM_CHUNK values — a multiple of D — at a time: one
        # round trip to memory per chunk instead of one per partial; thread a then adds its component in index order)
        L.append(f'extern "C" __global__ void __launch_bounds__({BLOCK}) lbm_wall_force_sum(const double* __restrict__ '
                 'part, CT* __restrict__ F, int nb)\n{')
        L.append(f'  __shared__ double buf[{SUM_CHUNK}];')
        L.append(f'  const int t = (int)threadIdx.x;\n  const long long total = (long long)nb * {D};\n  double s = 0.0;')
        L.append(f'  for (long long base = 0; base < total; base += {SUM_CHUNK}) {{')
        L.append(f'    const int m = (int)(total - base < {SUM_CHUNK} ? total - base : {SUM_CHUNK});')
        L.append(f'    for (int i = t; i < m; i += {BLOCK}) buf[i] = part[base + i];')
        L.append('    __syncthreads();')
        # (eight LDS reads in flight, then their adds in index order: read by read, the loop waits a whole LDS round
        # trip per partial — measured 7 µs on 163 partials)
        L.append(f'    if (t < {D}) {{\n      int i = t;\n      for (; i + {7 * D} < m; i += {8 * D}) {{')
        L.append('        const double ' + ', '.join(f'v{j} = buf[i + {j * D}]' for j in range(8)) + ';')
        L.append('        ' + ' '.join(f's += v{j};' for j in range(8)))
        L.append(f'      }}\n      for (; i < m; i += {D}) s += buf[i];\n    }}')
        L.append('    __syncthreads();\n  }')
        L.append(f'  if (t < {D}) F[t] = (CT)s;\n}}')
        # -- the scatter --------------------------------------------------------------------------------------
        L.append(f'extern "C" __global__ void __launch_bounds__({BLOCK}) lbm_wall_force_adj(T* __restrict__ g, '
                 f'{lists}, const CT* __restrict__ dF, long long n, int Y, int X, {strides("g")})\n{{')
        L.append(resource('g', 'g'))
        L.append(f'  const long long l = (long long)blockIdx.x * {BLOCK} + threadIdx.x;\n  if (l >= n) return;')
        L.append('  {\n    const IDX cell = cells[l];\n    const int d = dirs[l];')
        L += _decode(D)
        L.append(_offset('g'))
        L += dot
        L.append(f'    const CT v = {load("g", "g")} + (CT)(tab[2 * d] * dot);')
        L.append('    ' + store('g', 'g', 'v'))
        L.append('  }\n}')
        return '\n'.join(L) + '\n'
    # -- C: the ctypes signature of the CPU kernels (pointers, extents, strides, -, scalars) ------------------
    head = ('(void** P, const i64* N, const i64* S, const i64* B_, const double* Dv)\n{\n'
            '  (void)B_; (void)Dv; const long long n = N[0]; const IDX Y = N[1], X = N[2];\n'
            '  const IDX* cells = (const IDX*)P[1]; const unsigned char* dirs = (const unsigned char*)P[2]; '
            'const double* tab = (const double*)P[3];')
    L.append('void lbm_wall_force' + head)
    L.append('  const T* src = (const T*)P[0]; CT* F = (CT*)P[4];')
    L.append('  const IDX s_q = S[0], s_z = S[1], s_y = S[2], s_x = S[3];')
    L.append('  double ' + ', '.join(f'acc{a} = 0.0' for a in range(D)) + ';')
    L.append('  for (long long l = 0; l < n; ++l) {\n    const IDX cell = cells[l];\n    const int d = dirs[l];')
    L += _decode(D)
    L.append(_offset('s'))
    L.append(f'    const CT f = {load("s", "src")};')
    L += term
    L.append('  }')
    L.append('  ' + ' '.join(f'F[{a}] = (CT)acc{a};' for a in range(D)) + '\n}')
    L.append('void lbm_wall_force_adj' + head)
    L.append('  T* g = (T*)P[0]; const CT* dF = (const CT*)P[4];')
    L.append('  const IDX g_q = S[0], g_z = S[1], g_y = S[2], g_x = S[3];')
    L.append('  for (long long l = 0; l < n; ++l) {\n    const IDX cell = cells[l];\n    const int d = dirs[l];')
    L += _decode(D)
    L.append(_offset('g'))
    L += dot
    L.append(f'    const CT v = {load("g", "g")} + (CT)(tab[2 * d] * dot);')
    L.append('    ' + store('g', 'g', 'v'))
    L.append('  }\n}')
    return '\n'.join(L) + '\n'
