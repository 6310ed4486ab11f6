"""The ``pointwise`` schedule (all accesses at offset 0) and its module switches."""
import numpy as np

from ..printer import KernelExprPrinter
from .common import PRELUDE, _ctype, _statements, field_params, scalar_params, storage_ctype


_VEC4 = {'float': 'f32x4', 'double': 'f64x4', '_Float16': 'f16x4'}
_VEC2 = {'float': 'f32x2', '_Float16': 'f16x2'}
POINTWISE_UNROLL = 4
# one pass (a block per 256·4·U cells, no grid-stride loop: no wave waits on its own stores) with
# non-temporal loads: 1024³ fp32 copy 6.07 TB/s vs 5.53 TB/s grid-stride over 2048 blocks, torch.mul 6.27
POINTWISE_NT_LOAD = True
POINTWISE_MAX_BLOCKS = 0        # grid-stride cap of the vector kernel (0 = one pass)


def emit_pointwise(ir, name):
    """Two kernels: ``<name>_v4`` (4 cells per lane, vector loads) and ``<name>_v1``."""
    ct = _ctype(ir.compute_dtype)
    printer = KernelExprPrinter(ct, ir.symbol_names)
    params = ', '.join(field_params(ir) + ['const i64 n'] + scalar_params(ir))
    src = [PRELUDE]

    def body(vec, indent):
        lines = []
        k = '[k]' if vec else ''
        for r in ir.reads:
            src_expr = f"in_{r.field.name}{k}" if vec else f"f_{r.field.name}[i]"
            lines.append(f"{indent}const {ct} {r.var} = ({ct})({src_expr});")

        def store(field, offs, idx, code):
            t = storage_ctype(field)
            dst = f"out_{field.name}{k}" if vec else f"f_{field.name}[i]"
            return f"{indent}{dst} = ({t})({code});"
        lines += _statements(ir, printer, indent, store)
        return lines

    # vector kernel: each thread keeps U 16-byte-class vectors per field in flight (loads first,
    # then arithmetic, then non-temporal stores); a block covers 256*U consecutive vectors
    U = POINTWISE_UNROLL if max(np.dtype(f.dtype.numpy_dtype).itemsize for f in ir.fields) <= 4 else 2
    src.append(f'extern "C" __global__ void __launch_bounds__(256) {name}_v4({params})\n{{')
    src.append('  const i64 nvec = n >> 2;')
    src.append(f'  const i64 stride = (i64)gridDim.x * {256 * U};')
    src.append(f'  for (i64 b0 = (i64)blockIdx.x * {256 * U}; b0 < nvec; b0 += stride) {{')
    for u in range(U):
        src.append(f'    const i64 v{u} = b0 + threadIdx.x + {256 * u};')
    for u in range(U):
        for f in ir.fields_read:
            t = storage_ctype(f)
            src.append(f"    {_VEC4[t]} in_{f.name}_{u} = ({_VEC4[t]})(0);")
        src.append(f'    if (v{u} < nvec) {{')
        for f in ir.fields_read:
            t = storage_ctype(f)
            if POINTWISE_NT_LOAD:
                src.append(f"      in_{f.name}_{u} = __builtin_nontemporal_load((const {_VEC4[t]}*)(f_{f.name} + (v{u} << 2)));")
            else:
                src.append(f"      in_{f.name}_{u} = *(const {_VEC4[t]}*)(f_{f.name} + (v{u} << 2));")
        src.append('    }')
    for u in range(U):
        for f in ir.fields_written:
            t = storage_ctype(f)
            src.append(f"    {_VEC4[t]} out_{f.name}_{u};")
        src.append('    #pragma unroll')
        src.append('    for (int k = 0; k < 4; ++k) {')
        for r in ir.reads:
            src.append(f"      const {ct} {r.var} = ({ct})(in_{r.field.name}_{u}[k]);")

        def store(field, offs, idx, code, _u=u):
            t = storage_ctype(field)
            return f"      out_{field.name}_{_u}[k] = ({t})({code});"
        src += _statements(ir, printer, '      ', store)
        src.append('    }')
    for u in range(U):
        src.append(f'    if (v{u} < nvec) {{')
        for f in ir.fields_written:
            t = storage_ctype(f)
            src.append(f"      __builtin_nontemporal_store(out_{f.name}_{u}, ({_VEC4[t]}*)(f_{f.name} + (v{u} << 2)));")
        src.append('    }')
    src.append('  }')
    src.append('  for (i64 i = (nvec << 2) + (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {')
    src += body(False, '    ')
    src.append('  }')
    src.append('}')
    # scalar kernel (unaligned pointers)
    src.append(f'extern "C" __global__ void __launch_bounds__(256) {name}_v1({params})\n{{')
    src.append('  const i64 stride = (i64)gridDim.x * 256;')
    src.append('  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {')
    src += body(False, '    ')
    src.append('  }')
    src.append('}')
    return '\n'.join(src) + '\n'
