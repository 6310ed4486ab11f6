"""The LDS-DMA loader wave of the warp-specialised schedules, and the z-slab sweep's optional kernel parameters
(start signal, halo wait)."""
from .common import ncomp, storage_ctype


def ws_plane_base(f, RZ, q='q', periodic=False):
    """Uniform pointer of plane ``q`` of stencil field ``f`` (domain, halo buffer, or nullptr). ``periodic``: a plane
    outside ``[0, Z)`` without a halo buffer is the kernel's own plane ``q ± Z`` (never nullptr)."""
    C = ncomp(f)
    yx = 'YX' if C == 1 else f'(YX * {C})'
    if periodic:
        return (f'({q} >= 0 && {q} < Z) ? f_{f.name} + (i64){q} * {yx}'
                f' : ({q} < 0 ? (hlo_{f.name} ? hlo_{f.name} + (i64)({q} + {RZ}) * {yx}'
                f' : f_{f.name} + (i64)({q} + Z) * {yx})'
                f' : (hhi_{f.name} ? hhi_{f.name} + (i64)({q} - Z) * {yx} : f_{f.name} + (i64)({q} - Z) * {yx}))')
    return (f'({q} >= 0 && {q} < Z) ? f_{f.name} + (i64){q} * {yx}'
            f' : ({q} < 0 ? (hlo_{f.name} ? hlo_{f.name} + (i64)({q} + {RZ}) * {yx} : nullptr)'
            f' : (hhi_{f.name} ? hhi_{f.name} + (i64)({q} - Z) * {yx} : nullptr))')


def _ws_piece_offsets(f, g, NI, VE, esize, xo=False, periodic=False):
    """Per-lane byte offsets (inside a plane) of field f's ``NI`` 16-byte pieces of the tile image; pieces
    outside the plane get an out-of-range offset (the buffer range check returns / writes zeros).

    ``xo`` (2-byte elements, rows on half dwords): two offset sets, ``vo0`` / ``vo1``, for a plane whose first
    element sits on a dword / on a half dword (the descriptor then starts one element early). A row whose first
    element is on a half dword loads from one element before it (``sh`` = 1): LDS-DMA addresses are dword
    granular; the loader shifts that image row back once it has landed (``_ws_loader``).

    ``periodic``: a piece's row and column wrap instead (true modulo, once per loader lane): with rows of whole
    16-byte pieces every wrapped piece is a whole, aligned piece of the same plane — a per-lane row gather, the
    destination in LDS stays lane-linear."""
    RY, H = g['RY'], g['H']
    fg = g['FG'][f.name]
    C, NCH, NCHUNK = fg['C'], fg['NCH'], fg['NCHUNK']
    if periodic and xo:
        raise ValueError('periodic kernels take no rows on half dwords (XO)')
    y, xe = f'y0 - {RY} + row', f'(x0 - {H}) * {C} + col * {VE}'
    L = [f'    int vo0_{f.name}[{NI}], vo1_{f.name}[{NI}];' if xo else f'    int vo_{f.name}[{NI}];',
         '    #pragma unroll',
         f'    for (int i = 0; i < {NI}; ++i) {{',
         '      const int ch = i * 64 + lane;',
         f'      const int row = ch / {NCH};',
         f'      const int col = ch - row * {NCH};']
    if periodic:
        L += [f'      const int y = (({y}) % Y + Y) % Y;          // wrapped row',
              f'      const int xe = (({xe}) % (X * {C}) + X * {C}) % (X * {C});   // wrapped piece',
              f'      vo_{f.name}[i] = ch < {NCHUNK} ? (y * X * {C} + xe) * {esize} : 0x7ffffff0;']
    elif xo:
        L += [f'      const int y = {y};',
              f'      const int xe = {xe};',
              f'      const bool yok = ch < {NCHUNK} && y >= 0 && y < Y;']
        for pp in (0, 1):
            L += [f'      {{ const int sh = (y * X * {C} + {pp}) & 1;      // row start on a half dword',
                  f'        const bool ok = yok && xe - sh + {VE} > 0 && xe - sh < X * {C};',
                  f'        vo{pp}_{f.name}[i] = ok ? ({pp} + y * X * {C} + xe - sh) * {esize} : 0x7ffffff0; }}']
    else:
        L += [f'      const int y = {y};',
              f'      const int xe = {xe};          // element of the interleaved row',
              f'      const bool ok = ch < {NCHUNK} && y >= 0 && y < Y && xe >= 0 && xe < X * {C};',
              f'      vo_{f.name}[i] = ok ? (y * X * {C} + xe) * {esize} : 0x7ffffff0;']
    return L + ['    }']


# The compute waves' plane barrier over an LDS-DMA ring: every LDS read of the previous plane completes (lgkmcnt) before
# the barrier and none moves past it (memory clobber). Once the loader passes this barrier it refills the slot read one
# plane earlier, and its DMA writes are invisible to the compiler: with __syncthreads() hipcc 7.2 sank reads below the
# next barrier in the band kernel (hip_band/steps.py, scripts/probes/band_determinism.py). Audited in the ISA of every WS
# schedule (scripts/probes/barrier_audit.py: no ds_read outstanding at any s_barrier).
WS_CONSUMER_BARRIER = 'asm volatile("s_waitcnt lgkmcnt(0)\\n\\ts_barrier" ::: "memory");'


def _ws_loader(ir, cfg, g, ws):
    """The loader wave (wave 4): per-lane piece offsets once, then per plane one buffer descriptor per
    stencil field and ``NI`` LDS-DMA pieces; a counted ``vmcnt`` wait leaves the next ``D-1`` planes
    in flight across each barrier (raw ``s_barrier``: ``__syncthreads()``'s fence would drain them)."""
    RZ = g['RZ']
    D, NS = ws['D'], ws['NS']
    esize = ws['esize']
    VE = cfg.VE
    xo = cfg.XO
    ring = ws['kind'] == 'ring'
    per = bool(ir.periodic)
    if per and (cfg.XM or cfg.XO):
        raise ValueError('periodic kernels need rows of whole 16-byte pieces (no XM / XO config)')

    def slot_of(f):
        # zsum rings: the caller passes the slot; the march ring (per-field slot counts): the plane's index
        return f"(slot % {ws['F'][f.name]['NS']})" if ring else 'slot'
    L = [f'  if (wave == {ws["block"] // 64 - 1}) {{   // loader wave']
    for f in ir.stencil_fields:
        L += _ws_piece_offsets(f, g, ws['F'][f.name]['NI'], VE, esize, xo=xo, periodic=per)
    if xo:
        # a plane's first element on a half dword (its pointer's bit 1, 2-byte elements): 0 / 1
        L.append('    auto hpar = [&](const void* b) { return b ? (int)(((unsigned long long)b >> 1) & 1) : 0; };')
    L.append('    auto issue = [&](const int q, const int slot) {')
    for f in ir.stencil_fields:
        t = storage_ctype(f)
        NI, SLOT = ws['F'][f.name]['NI'], ws['F'][f.name]['SLOT']
        if xo:
            L += [f'      {{',
                  f'        const {t}* b = {ws_plane_base(f, RZ)};',
                  '        const int pp = hpar(b);',
                  # (the range in whole dwords: the plane's last element may share a dword with the next one)
                  f'        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(b ? b - pp : f_{f.name}), '
                  f'(short)0, b ? (int)((YX * {ncomp(f) * esize} + 2 * pp + 3) & ~3ll) : 0, 0x00020000);',
                  f'        {t}* dst = lds_{f.name} + slot * {SLOT};',
                  '        #pragma unroll',
                  f'        for (int i = 0; i < {NI}; ++i)',
                  f'          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)'
                  f'(dst + i * {1024 // esize}), 16, pp ? vo1_{f.name}[i] : vo0_{f.name}[i], 0, 0, 0);',
                  '      }']
            continue
        if ring and cfg.BABL == 3:
            continue                       # timing probe: the loader only meets the barriers
        L += [f'      {{',
              f'        const {t}* b = {ws_plane_base(f, RZ, periodic=per)};',
              f'        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(b ? b : f_{f.name}), '
              f'(short)0, b ? (int)(YX * {ncomp(f) * esize}) : 0, 0x00020000);',
              f'        {t}* dst = lds_{f.name} + {slot_of(f)} * {SLOT};',
              '        #pragma unroll',
              f'        for (int i = 0; i < {NI}; ++i)',
              f'          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)'
              f'(dst + i * {1024 // esize}), 16, vo_{f.name}[i], 0, 0, 0);',
              '      }']
    L += ['    };']
    if cfg.HWAIT:
        L += halo_wait_lines()
    L += [f'    const int nplanes = ze - zb + {2 * RZ};',
          f'    for (int i = 0; i < {D}; ++i)',
          f'      if (i < nplanes) issue(zb - {RZ} + i, i);',
          '    for (int j = 0; j < nplanes; ++j) {',
          '      // barrier j publishes plane j: leave the planes issued behind it in flight',
          f'      const int after = min({D - 1}, nplanes - 1 - j);']
    for k in range(D - 1, 0, -1):
        L.append(f'      {"if" if k == D - 1 else "else if"} (after == {k}) '
                 f'asm volatile("s_waitcnt vmcnt({k * ws["per_plane"]})" ::: "memory");')
    L.append(f'      {"else " if D > 1 else ""}if (after >= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");')
    if xo:
        # plane j has landed. A row loaded one element early (sh = 1) holds element x at image column
        # x - (x0 - H) + 1; the compute waves realign it in registers (``_emit_zsum_half``). Zeros, per row at
        # ITS alignment, over the RX columns left of x = 0 (a shifted row's first loaded piece straddles x = 0 and
        # brought the previous row's last element) and right of x = X (pieces past the row end)
        for f in ir.stencil_fields:
            C, P_f = ncomp(f), g['FG'][f.name]['P']
            SLOT = ws['F'][f.name]['SLOT']
            RXC = max(1, g['RX']) * C
            L += [f'      {{',
                  f'        const int qj = zb - {RZ} + j;',
                  f'        const int pp = hpar({ws_plane_base(f, RZ, "qj")});',
                  f'        {ws["lds_type"]}* img = lds_{f.name} + (j % {NS}) * {SLOT};',
                  f'        const int xs = (X - (x0 - {g["H"]})) * {C};',
                  f'        for (int i = lane; i < {g["TR"]} * {2 * RXC}; i += 64) {{',
                  f'          const int r = i / {2 * RXC}, c = i - r * {2 * RXC};',
                  f'          const int sh = ((y0 - {g["RY"]} + r) * X * {C} + pp) & 1;',
                  f'          const int col = c < {RXC} ? (x0 < {g["H"]} ? {g["H"] * C} - {RXC} + c : -1) : xs + c - {RXC};',
                  f'          if (col >= 0 && col + sh < {P_f}) img[r * {P_f} + col + sh] = 0;',
                  '        }',
                  '        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");',
                  '      }']
    if cfg.XM and not xo:
        # plane j has landed: zeros over the RX image columns past the row end (the straddling last piece brought
        # the next row's first elements; only the right halo of the row's last cells is read for stored outputs),
        # before barrier j publishes it
        for f in ir.stencil_fields:
            C, P_f = ncomp(f), g['FG'][f.name]['P']
            SLOT = ws['F'][f.name]['SLOT']
            L += [f'      {{',
                  f'        const int xs = (X - (x0 - {g["H"]})) * {C};',
                  f'        if (xs < {P_f}) {{',
                  f'          const int w = min({P_f} - xs, {max(1, g["RX"]) * C});',
                  f'          {ws["lds_type"]}* img = lds_{f.name} + (j % {NS}) * {SLOT};',
                  f'          for (int i = lane; i < {g["TR"]} * w; i += 64) img[(i / w) * {P_f} + xs + i % w] = 0;',
                  '          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");',
                  '        }',
                  '      }']
    L += ['      __builtin_amdgcn_s_barrier();',
          f'      if (j + {D} < nplanes) issue(zb - {RZ} + j + {D}, ' + (f'j + {D});' if ring else f'(j + {D}) % {NS});'),
          '    }',
          '    return;',
          '  }']
    return L


SIG_PARAMS = ['unsigned* __restrict__ psad_sig', 'const unsigned psad_sigv']
HWAIT_PARAMS = ['const unsigned* __restrict__ psad_hw', 'const unsigned psad_hwv']


def extra_params(cfg):
    """The z-slab sweep's optional kernel parameters, after the extents: SIG, then HWAIT."""
    return (SIG_PARAMS if cfg.SIG else []) + (HWAIT_PARAMS if cfg.HWAIT else [])


def halo_wait_lines(indent='    '):
    """Loader-wave prologue of an ``HWAIT`` launch (z-slab faces on the compute stream): before its first plane load
    the wave waits until the halo stream has published the sweep's receive buffers (``*psad_hw >= psad_hwv``, written
    by a stream-memory operation behind the RCCL exchange) — relaxed system-scope polls (an acquire per poll
    invalidates the CU's caches every time: measured 2x slower), ``s_sleep`` between them, ONE agent-scope acquire
    after the last, and a bound (2²² polls, ~0.2 s) so a lost signal ends the kernel instead of hanging the GPU. Only the
    loader wave reads global memory in these kernels; the compute waves meet its loads at the plane barriers."""
    i = indent
    return [f'{i}if (psad_hw != nullptr) {{',
            f'{i}  for (unsigned it = 0; it < (1u << 22); ++it) {{',
            f'{i}    if (__hip_atomic_load(psad_hw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= psad_hwv) break;',
            f'{i}    __builtin_amdgcn_s_sleep(2);',
            f'{i}  }}',
            f'{i}  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");',
            f'{i}}}',
            f'{i}asm volatile("" ::: "memory");']


def start_signal_lines():
    """Kernel prologue of a ``SIG`` launch: when the launch starts — every earlier launch on its stream has completed
    — workgroup 0 stores ``psad_sigv`` to the signal word (a system-scope store, seen by another queue's stream-memory
    wait; a null pointer skips it). The z-slab sweep orders its halo stream after the compute stream this way instead of
    a ROCclr stream-op kernel on the compute queue (csrc/psad_torch.cpp run_sweep)."""
    return ['  if (psad_sig != nullptr && blockIdx.x == 0 && threadIdx.x == 0)',
            '    __hip_atomic_store(psad_sig, psad_sigv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);']
