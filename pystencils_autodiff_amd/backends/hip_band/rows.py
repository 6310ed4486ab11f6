"""The compute lanes' view of a plane: a lane's task, the reads and conversion of one input row, and its taps."""
from .loader import hpar_lambda


def lane_setup(T):
    """A compute lane's task (row group, chunk column), its image and store offsets, the x-boundary and store masks."""
    cfg, X, VE, R, CPR, ntask, dw = T.cfg, T.X, T.VE, T.R, T.g['CPR'], T.g['ntask'], T.dw
    L = [hpar_lambda('  ')] if T.bo else []
    L += ['  const int ctid = (wave - (wave > ldw ? 1 : 0)) * 64 + lane;   // compute task',
          f'  const bool active = ctid < {ntask};',
          f'  const int t = active ? ctid : {ntask - 1};',
          f'  const int grp = t / {CPR}, col = t - grp * {CPR};',
          f'  const int lofs = grp * {R * T.XP} + {T.c0} + col * {VE};   // slot row grp*R = input row y0 + grp*R - 1',
          f'  const int x = col * {VE};',
          f'  const bool lmask = col == 0, rmask = col == {CPR - 1};']
    if T.bo:
        # the x-boundary zeros of half-dword rows as per-lane AND masks held in VGPRs (opaque to the compiler, so they
        # are not folded back into selects on 64-bit lane masks: those, with the per-plane v_perm selectors, ran the
        # kernel out of SGPRs — v_writelane / v_readlane spills in the plane loop)
        L.append('  unsigned lk0 = lmask ? 0xffff0000u : 0xffffffffu, rk = rmask ? 0u : 0xffffffffu, '
                 'rk0 = rmask ? 0xffff0000u : 0xffffffffu;')
        L.append('  asm volatile("" : "+v"(lk0), "+v"(rk), "+v"(rk0));')
    if cfg.BMASK:
        L.append(f'  const bool xfull = x >= xlo && x + {VE} <= xhi;')
        L.append(f'  const bool xtail = x + {VE} > {X};                 // the row\'s partial last chunk (unaligned rows)')
    L.append(f'  const int yrow0 = y0 + grp * {R};')
    L.append(f'  const unsigned sofs = (unsigned)(yrow0 * {X} + x) * {T.es}u;')
    if cfg.BMASK:
        L.append('  unsigned rowok = 0u;                           // rows of the lane inside [ylo, yhi), one bit each')
        L.append(f'  for (int o = 0; o < {R}; ++o) rowok |= (active && yrow0 + o >= ylo && yrow0 + o < yhi) ? (1u << o) : 0u;')
    L.append("  // edge dword (elements, from the lane's chunk): lane 0 the dword left of it, lane 63 the one right of it,")
    L.append("  // the other lanes dwords of the wave's block no other lane of their 32-lane half reads (unused): banks")
    L.append("  // (a/4) mod 32 all distinct per half (the compiler pairs these reads into ds_read2st64_b32). Lane 0 of")
    L.append("  // column 0 (x boundary, masked) reads its own first dword instead of the one before the slot.")
    # dword targets relative to the wave's block (64 chunks of 4 dwords): -1, 0 .. 30 | 33 .. 63, 256
    if T.padded:
        pass                                              # x neighbours read from the image (zero pads at row ends)
    elif cfg.BEDGE:
        L.append(f'  const int eoff = {dw} * (lane == 0 ? (col == 0 ? 0 : -1) : (lane == 63 ? 256 : (lane < 32 ? lane - 1 '
                 f': lane + 1))) - {VE} * lane;')
    else:
        L.append(f'  const int eoff = {dw} * (lane == 0 ? -1 : (lane == 63 ? 256 : lane)) - {VE} * lane;')
    for si in range(T.NP):
        for s in range(3):
            for o in range(R):
                L.append(f'  {T.at} ' + ', '.join(f'{T.A(si, s, o, a)} = {T.azero}' for a in range(4)) + ';')
    return L


def _edge_dpp(ind):
    """The lane's edge dword and, through it, the dwords left and right of its chunk ``d`` from the adjacent lanes."""
    return [f'{ind}    const unsigned e = *(const unsigned*)(rp + eoff);',
            f'{ind}    const unsigned lw = __builtin_amdgcn_update_dpp(e, d.w, 0x138, 0xf, 0xf, false);   // wave_shr:1',
            f'{ind}    const unsigned rw = __builtin_amdgcn_update_dpp(e, d.x, 0x130, 0xf, 0xf, false);   // wave_shl:1']


def _pairs(ind, c):
    """fp16: the ten elements x-1 .. x+8 (``l``, the eight cells ``c``, ``rr``) converted once, as the fp32 pairs
    P0 .. P5 of the elements (e, e+4)."""
    e = ['l'] + c + ['rr']
    P = [f'P{i} = {{(float){e[i]}, (float){e[i + 4]}}}' for i in range(6)]
    return [f'{ind}    const f32x2 {", ".join(P[:3])};', f'{ind}    const f32x2 {", ".join(P[3:])};']


def _floats(ind, h0, h5):
    """fp32: the six elements x-1 .. x+4 as H0 .. H5."""
    return [f'{ind}    const float H0 = {h0}, H5 = {h5};', f'{ind}    const float H1 = v.x, H2 = v.y, H3 = v.z, H4 = v.w;']


def _row_half_dwords(T, ind, r):
    """Image row r starts one element early when the input row starts on an odd element: realign the lane's 10 elements
    x-1 .. x+8 as five dwords (v_perm over adjacent dwords; selector per row and plane parity)."""
    sel = 'selA' if r % 2 else 'selB'
    cq = '' if T.czf else 'const '
    wz = (T.X % T.VE + 1) // 2
    B = [f'{ind}    const u32x4 d = *(const u32x4*)rp;'] + _edge_dpp(ind)
    B += [f'{ind}    {cq}f16x2 w0 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(d.x, lw, {sel}) & lk0), '
          f'w1 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(d.y, d.x, {sel}));',
          f'{ind}    {cq}f16x2 w2 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(d.z, d.y, {sel})), '
          f'w3 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(d.w, d.z, {sel}));',
          # the row's last chunk: x+7 and x+8 both lie at or past X (8·CPR - 1 >= X for odd X) and on a row
          # loaded one element early both come from the next lane, which may hold another row: zeros
          f'{ind}    const f16x2 w4 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(rw, d.w, {sel}) & rk);',
          f'{ind}    const _Float16 l = w0[0], rr = w4[1];',
          *([f'{ind}    w{wz} = __builtin_bit_cast(f16x2, __builtin_bit_cast(unsigned, '
             f'w{wz}) & rk0);   // the first element past the row end (no loader zero fill)']
            if T.czf and wz < 4 else [])]
    return B + _pairs(ind, [f'w{i // 2}[{i % 2}]' for i in range(1, 9)])


def row_prologue(T, ind, r):
    """Input row r of the lane's image rows: its chunk and both x neighbours read and converted once."""
    et, vt, half, X, VE = T.et, T.vt, T.half, T.X, T.VE
    B = [f'{ind}    const {et}* rp = sl + {r * T.XP};']
    if T.bo:
        return B + _row_half_dwords(T, ind, r)
    cells = [f'v[{i}]' for i in range(8)]
    if T.padded:
        # the dwords left and right of the lane's chunk straight from the image (a row's end chunks meet the zero
        # pads): no DPP, no boundary selects (one ds_read2_b32 per row)
        B += [f'{ind}    const unsigned el = *(const unsigned*)(rp - {T.dw}), er = *(const unsigned*)(rp + {VE});',
              f'{ind}    const {vt} v = *(const {vt}*)rp;']
        if not half:
            return B + _floats(ind, '__builtin_bit_cast(float, el)', '__builtin_bit_cast(float, er)')
        B.append(f'{ind}    const _Float16 l = __builtin_bit_cast(f16x2, el)[1], rr = __builtin_bit_cast(f16x2, er)[0];')
        return B + _pairs(ind, cells)
    if T.czf:
        # the last chunk's element X % VE is the next row's first (no loader zero fill): zero, as the right
        # neighbour of cell X-1
        B += [f'{ind}    {vt} v = *(const {vt}*)rp;',
              f'{ind}    v[{X % VE}] = rmask ? ({et})0 : v[{X % VE}];']
    else:
        B += [f'{ind}    const {vt} v = *(const {vt}*)rp;']
    B += [f'{ind}    const u32x4 d = __builtin_bit_cast(u32x4, v);'] + _edge_dpp(ind)
    if not half:
        return B + _floats(ind, 'lmask ? 0.f : __builtin_bit_cast(float, lw)',
                           'rmask ? 0.f : __builtin_bit_cast(float, rw)')
    B += [f'{ind}    const _Float16 l = lmask ? (_Float16)0 : __builtin_bit_cast(f16x2, lw)[1];',
          f'{ind}    const _Float16 rr = rmask ? (_Float16)0 : __builtin_bit_cast(f16x2, rw)[0];']
    return B + _pairs(ind, cells)


def taps(T, ind, r, sets, first):
    """FMA statements of input row r into the given (set, dz) accumulators, dx outer. ``first``: the step's set of
    (plan, row, slot) that already took a ``dz = -1`` tap this plane — the first one assigns, and is added here."""
    if T.cfg.BABL == 1:
        # ablation probe: one add per row and set (the row's loads and one convert stay live)
        o = min(max(r - 1, 0), T.R - 1)
        todo = [(st, dz, si, o, 0, T.operand(0, 0)) for st, dz in sets for si in range(T.NP)]
    else:
        todo = []
        for dx in (-1, 0, 1):
            for st, dz in sets:
                for si in range(T.NP):
                    for o in range(T.R):
                        dy = r - o - 1
                        wv = T.W[si].get((dz, dy, dx)) if -1 <= dy <= 1 else None
                        if wv is not None:
                            todo += [(st, dz, si, o, a, f'{wv} * {T.operand(a, dx)}') for a in range(4)]
    B = []
    for st, dz, si, o, a, term in todo:
        acc = T.A(si, st, o, a)
        if dz == -1 and (si, o, a) not in first:
            first.add((si, o, a))
            B.append(f'{ind}{acc} = {term};')
        else:
            B.append(f'{ind}{acc} = {acc} + {term};')
    return B
