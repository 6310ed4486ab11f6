"""Row-band schedule for half-precision 3-D stencils (fp16 storage, fp32 arithmetic) on gfx950.

The ``zsum`` schedule tiles a plane in 256×8 tiles: a workgroup's share of a plane is eight 512-byte row segments,
and the stores of a sweep reach ~5.4 TB/s (``scripts/probes/store_patterns.py``). Here a workgroup owns a BAND:
``TY`` full rows of a plane, which in a dense row-major field is ONE contiguous block of ``TY·X`` halves.

* loader wave: the band's rows ``y0-1 … y0+TY`` of plane ``q`` are one contiguous block as well, streamed into an
  LDS slot by LDS-DMA (``buffer_load_dwordx4 … lds``, 1 KiB per wave instruction, rows outside the plane read as
  zeros by the buffer range check, planes outside the domain from the z-slab halo buffers or zeros);
  ``D`` planes in flight in a ring of ``D + 1`` slots, published by one workgroup barrier per plane.
* compute lanes: lane ``t`` owns the 16-byte chunk ``col = t mod X/8`` (8 x-adjacent cells) of the ``R`` rows of
  row group ``t div X/8``. Per plane it reads its ``R + 2`` input rows once (``ds_read_b128``), takes the x
  neighbours from the adjacent lanes (DPP ``wave_shr/shl:1``; the wave's end lanes read one LDS dword; full rows
  make columns 0 and X/8-1 the domain's x boundary), converts each value once to fp32 and runs packed FMAs over
  the cell pairs ``(x+e, x+e+4)`` so every tap operand is a register pair as converted.
* z partial sums (as ``zsum``): input plane ``q`` adds its taps to outputs ``q+1``, ``q``, ``q-1``; the three
  accumulator sets rotate with the plane index (loop unrolled by 3, no moves). (Skipping the taps of outputs outside
  a chunk in its first / last two planes behind uniform branches measured slower: profiles/r03_op_band_ab2.log.)
* stores: output ``q-1`` row by row, 16 bytes per lane, 1 KiB contiguous per wave instruction, non-temporal.

Eligible: 3-D, every field fp16 (fp32 storage compiles too: opt-in), one stencil field (radius ≤ 1), every store a linear combination of its taps
(``zsum_plan`` with no centre-plane remainder), rows a multiple of 16 bytes. Measured against the ``zsum`` half ring
in ``scripts/probes/rowblock27r.py`` (``profiles/r03_band_*.log``).

Plan, then print: ``geometry`` (eligibility, launch / LDS geometry, the band choice), ``tables`` (``BandTables``:
everything derived before the first printed line), and the printers of ``(T, ...)`` that return lines — ``loader``
(the loader wave), ``rows`` (a lane's task, a row's reads, conversion and taps), ``stores``, ``steps`` (a plane step
and the loops around it).
"""
from ..hip_emitter import PRELUDE, extra_params, field_params, scalar_params, start_signal_lines
from .geometry import band_choice, band_esize, band_geometry, band_plans
from .loader import loader_wave
from .rows import lane_setup
from .steps import plane_loops
from .tables import BandTables, band_tables

__all__ = ['band_plans', 'band_geometry', 'band_choice', 'band_esize', 'emit_band', 'BandTables', 'band_tables']


def emit_band(ir, name, cfg):
    """HIP source of the band kernel (signature identical to the march / zsum kernels: fields, 2 halo pointers
    per stencil field, Z Y X zlo zhi ylo yhi xlo xhi zc zstep ntx nty, scalars)."""
    T = band_tables(ir, cfg)
    g, et, S = T.g, T.et, T.S
    params = field_params(ir)
    params += [f'const {et}* __restrict__ hlo_{S.name}', f'const {et}* __restrict__ hhi_{S.name}']
    params += ['const int Z', 'const int Y', 'const int X', 'const int zlo', 'const int zhi', 'const int ylo',
               'const int yhi', 'const int xlo', 'const int xhi', 'const int zc', 'const int zstep', 'const int ntx',
               'const int nty']
    params += extra_params(cfg)
    params += scalar_params(ir)
    L = [PRELUDE, 'typedef unsigned u32x4 __attribute__((ext_vector_type(4)));',
         'typedef unsigned u32x3 __attribute__((ext_vector_type(3)));', 'typedef unsigned u32x2 __attribute__((ext_vector_type(2)));']
    L.append(f'// band schedule: {T.TY}-row bands of full {T.X}-element rows, {T.R} rows x {T.VE} cells per lane, {T.NCW} '
             f'compute waves + LDS-DMA loader wave, {g["NS"]}-slot {et} plane ring ({T.D} planes in flight), z partial sums '
             f'in 3 rotating register sets, LDS {g["lds_bytes"]} B')
    L.append(f'extern "C" __global__ void __launch_bounds__({g["NT"]}) {name}({", ".join(params)})\n{{')
    if cfg.SIG:
        L += start_signal_lines()
    L.append(f'  __shared__ __attribute__((aligned(1024))) {et} lds[{g["NS"] * g["SLOT"] + 64}];')
    L.append('  const int tid = threadIdx.x, lane = tid & 63;')
    L.append('  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);')
    if T.free:
        # hs[0]: planes landed (the loader's), hs[1 + w]: planes compute wave w has finished reading (its own word).
        # Set before the one workgroup barrier of the kernel; the plane steps then never meet at a barrier
        L.append(f'  __shared__ unsigned hs[{T.NCW + 1}];          // (relaxed workgroup atomics: ds_read / ds_write, not flat)')
        L.append('  auto hs_ld = [&](const int i) { return __hip_atomic_load(&hs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };')
        L.append('  auto hs_st = [&](const int i, const unsigned v) { __hip_atomic_store(&hs[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };')
        L.append(f'  if (tid <= {T.NCW}) hs[tid] = 0u;')
        L.append('  __syncthreads();')
    if cfg.MAP == 1:
        L.append('  const int lb = blockIdx.x;')
    else:
        L.append('  // XCD-aware, bijective block remap: consecutive bands share one XCD (and its L2)')
        L.append('  const int nb = gridDim.x, b = blockIdx.x;')
        L.append('  const int per = nb >> 3, rem = nb & 7, xcd = b & 7, bi = b >> 3;')
        L.append('  const int lb = (xcd < rem) ? xcd * (per + 1) + bi : rem * (per + 1) + (xcd - rem) * per + bi;')
    L.append('  const int band = lb % nty, chunk = lb / nty;')
    L.append(f'  const int y0 = band * {T.TY};')
    L.append('  const int zb = zlo + chunk * zstep;       // zstep = zc, or the gap of a two-range launch')
    L.append('  const int ze = min(zb + zc, zhi);')
    L.append('  if (zb >= ze) return;')
    L.append(f'  const i64 YX = (i64)Y * {T.X};')
    L.append('  const int nplanes = ze - zb + 2;')
    L += loader_wave(T) + lane_setup(T) + plane_loops(T)
    L.append('}')
    return '\n'.join(L) + '\n'
