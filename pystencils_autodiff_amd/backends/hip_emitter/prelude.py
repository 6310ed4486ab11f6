"""The kernel head the ``march`` and ``zsum`` schedules share."""
from .common import _ctype, _vec_type, field_params, scalar_params, storage_ctype
from .loader import extra_params, start_signal_lines, ws_plane_base


def _march_prelude(ir, name, cfg, g, slots, ws=None, lane_stride=1):
    """Kernel signature, LDS rings, XCD-aware tile/chunk mapping, plane loaders and LDS stashers
    shared by the ``march`` and ``zsum`` schedules."""
    RZ, RY, H, TR, P = (g[k] for k in ('RZ', 'RY', 'H', 'TR', 'P'))
    ct = _ctype(ir.compute_dtype)
    stencil = ir.stencil_fields
    VE = cfg.VE
    TX, TY, CX, WX, NR, PD = cfg.TX, cfg.TY, cfg.CX, cfg.WX, cfg.NR, cfg.PD
    params = field_params(ir)
    for f in stencil:
        t = storage_ctype(f)
        params += [f"const {t}* __restrict__ hlo_{f.name}", f"const {t}* __restrict__ hhi_{f.name}"]
    params += ['const int Z', 'const int Y', 'const int X', 'const int zlo', 'const int zhi', 'const int ylo',
               'const int yhi', 'const int xlo', 'const int xhi', 'const int zc', 'const int zstep', 'const int ntx',
               'const int nty']
    params += extra_params(cfg)
    params += scalar_params(ir)

    L = []
    L.append(f'extern "C" __global__ void __launch_bounds__({ws["block"] if ws else cfg.NT}) {name}({", ".join(params)})\n{{')
    if cfg.SIG:
        L += start_signal_lines()
    FG = g['FG']
    for f in stencil:
        n_el = ws['F'][f.name].get('NS', ws['NS']) * ws['F'][f.name]['SLOT'] if ws else slots[f.name] * TR * FG[f.name]['P']
        L.append(f"  __shared__ __attribute__((aligned({1024 if ws else 16}))) {ws['lds_type'] if ws else ct} "
                 f"lds_{f.name}[{n_el}];")
    L.append('  const int tid = threadIdx.x;')
    L.append('  const int lane = tid & 63;')
    L.append('  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);')
    L.append(f'  const int wx = wave % {WX};')
    L.append(f'  const int wy = wave / {WX};')
    if cfg.MAP == 1:
        L.append('  const int lb = blockIdx.x;             // dispatch order (consecutive tiles round-robin the XCDs)')
    else:
        L.append('  // XCD-aware, bijective block remap: consecutive logical tiles share one XCD (and its L2)')
        L.append('  const int nb = gridDim.x, b = blockIdx.x;')
        L.append('  const int per = nb >> 3, rem = nb & 7, xcd = b & 7, bi = b >> 3;')
        L.append('  const int lb = (xcd < rem) ? xcd * (per + 1) + bi : rem * (per + 1) + (xcd - rem) * per + bi;')
    L.append('  const int nt = ntx * nty;')
    L.append('  const int tile = lb % nt;')
    L.append('  const int chunk = lb / nt;')
    L.append(f'  const int x0 = (tile % ntx) * {TX};')
    L.append(f'  const int y0 = (tile / ntx) * {TY};')
    L.append('  const int zb = zlo + chunk * zstep;       // zstep = zc, or the gap of a two-range launch')
    L.append('  const int ze = min(zb + zc, zhi);')
    L.append('  if (zb >= ze) return;')
    L.append('  const i64 YX = (i64)Y * X;')
    L.append(f'  const bool interior = x0 >= {H} && x0 + {TX + H} <= X && y0 >= {RY} && y0 + {TY + RY} <= Y;')


    ln = 'lane' if lane_stride == 1 else f'{lane_stride} * lane'    # lanes own CX x-adjacent cells (half ring)

    def bases():
        B = [f'  const int lbase = (wy * {NR} + {RY}) * {P} + {H} + wx * {64 * CX} + {ln};',
             f'  const int ybase = y0 + wy * {NR};',
             f'  const int xbase = x0 + wx * {64 * CX} + {ln};']
        for f in stencil:      # per-field image offset of the lane's first cell (components interleaved)
            C = FG[f.name]['C']
            B.append(f'  const int lb_{f.name} = (wy * {NR} + {RY}) * {FG[f.name]["P"]} + '
                     f'({H} + wx * {64 * CX} + {ln}) * {C};')
        return B
    if ws:
        return L + bases()
    sets = ['A', 'B'][:PD]
    for f in stencil:
        t = storage_ctype(f)
        for s_ in sets:
            L.append(f"  {_vec_type(t, VE)} pre{s_}_{f.name}[{FG[f.name]['CPT']}];")

    for f in stencil:
        t = storage_ctype(f)
        vt = _vec_type(t, VE)
        C, P_f, NCH, NCHUNK, CPT = (FG[f.name][k] for k in ('C', 'P', 'NCH', 'NCHUNK', 'CPT'))
        L.append(f"  auto load_{f.name} = [&]({vt}* pre, const int p) {{")
        L.append(f"    const {t}* base = {ws_plane_base(f, RZ, 'p')};")

        def ld(ptr):
            return f'*(const {vt}*)({ptr})'
        L.append('    #pragma unroll')
        L.append(f'    for (int k = 0; k < {CPT}; ++k) {{')
        L.append(f'      const int ch = tid + k * {cfg.NT};')
        L.append(f'      {vt} v = ({vt})(0);')
        L.append(f'      if (base != nullptr && ch < {NCHUNK}) {{')
        L.append(f'        const int row = ch / {NCH};')
        L.append(f'        const int col = ch - row * {NCH};')
        L.append(f'        const int y = y0 - {RY} + row;')
        L.append(f'        const int xe = (x0 - {H}) * {C} + col * {VE};')
        L.append(f'        if (y >= 0 && y < Y && xe >= 0 && xe < X * {C})')
        L.append(f'          v = {ld(f"base + (i64)y * X * {C} + xe")};')
        L.append('      }')
        L.append('      pre[k] = v;')
        L.append('    }')
        L.append('  };')
        L.append(f"  auto stash_{f.name} = [&](const {vt}* pre, const int slot) {{")
        L.append(f"    {ct}* dst = lds_{f.name} + slot * {TR * P_f};")
        L.append('    #pragma unroll')
        L.append(f'    for (int k = 0; k < {CPT}; ++k) {{')
        L.append(f'      const int ch = tid + k * {cfg.NT};')
        L.append(f'      if (ch < {NCHUNK}) {{')
        L.append(f'        const int row = ch / {NCH};')
        L.append(f'        const int col = ch - row * {NCH};')
        if VE == 1:
            L.append(f'        dst[row * {P_f} + col] = ({ct})pre[k];')
        elif t == ct:
            L.append(f'        *({vt}*)(dst + row * {P_f} + col * {VE}) = pre[k];')
        else:
            L.append('        #pragma unroll')
            L.append(f'        for (int e = 0; e < {VE}; ++e) dst[row * {P_f} + col * {VE} + e] = ({ct})pre[k][e];')
        L.append('      }')
        L.append('    }')
        L.append('  };')
        S_f = slots[f.name]
        L.append(f'  auto slot_{f.name} = [&](const int p) {{ return ((p % {S_f}) + {S_f}) % {S_f}; }};')

    return L + bases()
